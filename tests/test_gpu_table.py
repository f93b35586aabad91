"""categorical_table networks on the GPU: the table walk (csrc/vbn_table_walk.hip) behind the
engines and the CPD surface.

* every case of tests/golden/tabular/table7.pt is replayed with its recorded draws injected:
  samples exactly equal; pdf / weights / ESS to rtol 1e-4, log-densities to 1e-4 absolute (the
  tolerances of ``smoke()``); the fallback flag equal; ``cpd_log_prob`` on 1-dim nodes bit-equal;
* production draws: a 24-node random table model, MCM / LW / IS / ancestral at B = 8 x S = 128 and
  B = 3 x S = 80 (waves straddle queries, the last wave has idle lanes) against
  tests/table_reference.py on the kernel's own Philox words.  A particle may differ only where
  some draw lies within 2^-23 (CDF units) of a class boundary: the float32 CDF entries are float64
  sums rounded once (<= 2^-25 relative to 1) and u lies on the 2^-24 grid; such flagged particles
  must stay under 1 % (expected share ~ nodes * 2 (C - 1) * 2^-23 ~ 5e-5);
* the LDS-staged and the forced global path give identical outputs; ``run_if = 0`` writes
  nothing; out-of-support evidence raises the reference's ValueError on the host.
"""
import os
import sys

import networkx as nx
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import table_reference as TR  # noqa: E402
from vectorizedbayesiannetwork_amd import VBN, ops  # noqa: E402
from vectorizedbayesiannetwork_amd import engines as E  # noqa: E402
from vectorizedbayesiannetwork_amd import synthetic  # noqa: E402
from vectorizedbayesiannetwork_amd.cpd import cpd_forward, cpd_log_prob, cpd_params, cpd_sample  # noqa: E402
from vectorizedbayesiannetwork_amd.model import model_from_checkpoint, random_table_model  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tabular", "table7.pt")
MARGIN = 2.0 ** -23
_FX = {}


def fixture():
    if not _FX:
        _FX.update(torch.load(FIXTURE, weights_only=True))
        model = model_from_checkpoint(_FX["model"])
        _FX["vbn"] = VBN.from_model(model, device="cuda:0")
        _FX["tm"] = TR.TableModel(model)
    return _FX


def noise_of(case, model, phase=0):
    """Recorded CDF midpoints per node as the walk's injected uniforms: slot 0, [B | 1, S, D]."""
    s = int(case["n_samples"])
    per = {}
    for r in case["draws"]:
        if r["kind"] == "cat" and r["node"] is not None and r["phase"] == phase:
            per.setdefault(r["node"], []).append(r["value"].float().reshape(-1))
    return {n: (torch.cat(v).view(-1, s, model.out_dim(n)), None) for n, v in per.items()}


def close(got, want, what):
    assert torch.allclose(got.cpu().float(), want, rtol=1e-4, atol=1e-30), f"{what} differs"


# ---- fixture replay ------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(12))
def test_engine_cases_replay(i):
    fx = fixture()
    vbn, model = fx["vbn"], fx["vbn"].model
    case = [c for c in fx["cases"] if c["engine"] != "cpd"][i]
    q, n, p, ref = vbn._normalize_query(case["query"]), case["n_samples"], case["params"], case["outputs"]
    eng_name = case["engine"]
    kw = {"_noise": noise_of(case, model, 0)}
    if eng_name == "ancestral":
        xs = E.AncestralSampler(n_samples=n).sample(vbn, q, n, **kw)
        assert torch.equal(xs.cpu(), ref["samples"])
        return
    if eng_name == "monte_carlo_marginalization":
        eng = E.MonteCarloMarginalization(n_samples=n)
    elif eng_name == "likelihood_weighting":
        eng = E.LikelihoodWeighting(n_samples=n, normalize=p.get("normalize", True))
    elif eng_name == "importance_sampling":
        eng = E.ImportanceSampling(n_samples=n)
        eng.ess_threshold = p.get("ess_threshold", 0.1)
        kw["_noise_fallback"] = noise_of(case, model, 1)
    else:
        eng = E.CategoricalExact(n_samples=n)
    pdf, xs = eng.infer_posterior(vbn, q, **kw)
    assert tuple(pdf.shape) == tuple(ref["pdf"].shape) and tuple(xs.shape) == tuple(ref["samples"].shape)
    assert torch.equal(xs.cpu(), ref["samples"]), "samples differ"
    close(pdf, ref["pdf"], "pdf / weights")
    if eng_name == "importance_sampling":
        assert eng._last_fallback == ref["fallback"]
        close(eng._last_ess, ref["ess"], "ESS")
    if eng_name == "categorical_exact":
        assert eng._last_fallback == bool(case["draws"])


@pytest.mark.parametrize("i", range(7))
def test_cpd_cases_replay(i):
    fx = fixture()
    vbn, model = fx["vbn"], fx["vbn"].model
    case = [c for c in fx["cases"] if c["engine"] == "cpd"][i]
    node, n, par, ref = case["node"], case["n_samples"], case["parents"], case["outputs"]
    noise = noise_of(case, model, 0)
    xs = cpd_sample(vbn, node, par, n, _noise=noise)
    assert torch.equal(xs.cpu(), ref["sample"])
    fwd = cpd_forward(vbn, node, par, n, _noise=noise)
    assert torch.equal(fwd.samples.cpu(), ref["sample"])
    assert torch.allclose(fwd.log_prob.cpu(), ref["log_prob_sampled"], rtol=0, atol=1e-4)
    lp = cpd_log_prob(vbn, node, case["x"], par).cpu()
    if model.out_dim(node) == 1:
        assert lp.numpy().tobytes() == ref["log_prob_x"].numpy().tobytes(), "log_prob must be bit-equal"
    else:
        assert torch.allclose(lp, ref["log_prob_x"], rtol=0, atol=1e-4)
    # conditional parameters: the probability row of the parent configuration
    prm = cpd_params(vbn, node, par).cpu()
    tm = fx["tm"]
    b = 1 if par is None else par.shape[0]
    want = tm.cpds[node].probs(None if par is None else par.double().unsqueeze(1), b, 1)
    close(prm.view(b, -1), want.reshape(b, -1).float(), "conditional probabilities")


# ---- production draws ----------------------------------------------------------------------------

def production():
    if "prod" not in _FX:
        g = synthetic.random_dag(24, seed=2, max_parents=3)
        topo = list(nx.topological_sort(g))
        cards = {n: 2 + (5 * i) % 8 for i, n in enumerate(topo)}                  # 2..9, mixed
        model = random_table_model(g, cards, seed=1)
        gen = torch.Generator().manual_seed(5)
        ev_nodes = [topo[3], topo[11], topo[20]]
        ev = {n: torch.randint(0, cards[n], (8, 1), generator=gen).float() for n in ev_nodes}
        _FX["prod"] = (VBN.from_model(model, device="cuda:0"), TR.TableModel(model), topo[-1], ev)
    return _FX["prod"]


@pytest.mark.parametrize("b,s", [(8, 128), (3, 80)])
@pytest.mark.parametrize("engine", ["mcm", "lw", "is", "ancestral"])
def test_production_draws_match_the_reference(engine, b, s):
    vbn, tm, target, ev_all = production()
    ev = {k: v[:b] for k, v in ev_all.items()}
    q = vbn._normalize_query({"target": target, "evidence": ev})
    seed = (1234 << 32) | (77 + b)
    pk = E.packed_model(vbn, torch.device("cuda:0"))
    draws = TR.PhiloxTableDraws(pk.node_id, seed=seed, n_queries=b, n_samples=s)
    args = (tm, target, ev, {}, s, draws)
    if engine == "mcm":
        pdf, xs = E.MonteCarloMarginalization(n_samples=s).infer_posterior(vbn, q, seed=seed)
        ref_pdf, ref_xs = TR.mcm(*args)
    elif engine == "lw":
        pdf, xs = E.LikelihoodWeighting(n_samples=s).infer_posterior(vbn, q, seed=seed)
        ref_pdf, ref_xs, _ = TR.lw(*args)
    elif engine == "is":
        eng = E.ImportanceSampling(n_samples=s)
        eng.ess_threshold = 0.0
        pdf, xs = eng.infer_posterior(vbn, q, seed=seed)
        ref_pdf, ref_xs, ref_ess, fb = TR.importance(*args, None, ess_threshold=0.0)
        assert not fb and not eng._last_fallback
    else:
        xs = E.AncestralSampler(n_samples=s).sample(vbn, q, s, seed=seed)
        pdf, ref_pdf, ref_xs = None, None, TR.ancestral(*args)
    assert draws.n_draws > 0
    flagged = torch.from_numpy(draws.margin < MARGIN)                              # [b, s]
    share = float(flagged.float().mean())
    print(f"{engine} {b}x{s}: {int(flagged.sum())} of {b * s} particles within 2^-23 of a class boundary")
    assert share < 0.01
    same = (xs.cpu() == ref_xs.float()).all(-1)
    assert bool((same | flagged).all()), "a particle differs whose draws are all clear of the class boundaries"
    if pdf is None:
        return
    ok = torch.isclose(pdf.cpu(), ref_pdf.float(), rtol=1e-4, atol=1e-30)
    if engine == "mcm":
        assert bool((ok | flagged).all())
    else:                       # normalised over the query: compare the queries without a flagged particle
        clean = ~flagged.any(dim=1)
        assert bool(ok[clean].all())
        if engine == "is":
            assert torch.allclose(eng._last_ess.cpu()[clean], ref_ess.float()[clean], rtol=1e-4)


# ---- launch forms ---------------------------------------------------------------------------------

def test_staged_and_global_paths_agree(monkeypatch):
    fx = fixture()
    vbn = fx["vbn"]
    case = [c for c in fx["cases"] if c["engine"] == "likelihood_weighting"][0]
    q = vbn._normalize_query(case["query"])
    outs = {}
    for force in ("0", "1"):
        monkeypatch.setenv("VBN_TABLE_GLOBAL", force)
        w, xs = E.LikelihoodWeighting(n_samples=192).infer_posterior(vbn, q, seed=99)
        a = E.AncestralSampler(n_samples=70).sample(vbn, E.Query(target=None, evidence={}), 70, seed=5)
        torch.cuda.synchronize()
        assert ops.LAST_WALK["table_staged"] == (force == "0")
        outs[force] = (w.cpu(), xs.cpu(), torch.cat([a[n].cpu() for n in vbn.model.topo], dim=-1))
    for x, y in zip(outs["0"], outs["1"]):
        assert x.numpy().tobytes() == y.numpy().tobytes()


def test_run_if_zero_writes_nothing():
    fx = fixture()
    vbn = fx["vbn"]
    dev = torch.device("cuda:0")
    pk = E.packed_model(vbn, dev)
    case = [c for c in fx["cases"] if c["engine"] == "likelihood_weighting"][0]
    q = vbn._normalize_query(case["query"])
    lw = E.LikelihoodWeighting(n_samples=64)
    b, n = 3, 64
    for flag_value in (0, 1):
        flag = torch.full((1,), flag_value, dtype=torch.int32, device=dev)
        w = torch.full((b, n), -7.0, device=dev)
        x = torch.full((b, n, 1), -7.0, device=dev)
        lw.infer_into(vbn, q, n, seed=3, offset=1, run_if=flag, w_out=w, x_out=x)
        torch.cuda.synchronize()
        untouched = bool((w == -7.0).all()) and bool((x == -7.0).all())
        assert untouched == (flag_value == 0)
    assert pk.tabular


def test_out_of_support_evidence_raises_before_launch(monkeypatch):
    fx = fixture()
    vbn = fx["vbn"]
    launches = []
    monkeypatch.setattr(ops, "table_walk", lambda *a, **k: launches.append(a))
    monkeypatch.setattr(ops, "table_walk_ex", lambda *a, **k: launches.append(a))
    bad = {"target": "b5", "evidence": {"c9": torch.tensor([[2.0], [9.0], [3.0]])}}          # c9 has classes 0..8
    for eng in (E.LikelihoodWeighting(n_samples=16), E.ImportanceSampling(n_samples=16),
                E.MonteCarloMarginalization(n_samples=16)):
        q = vbn._normalize_query(bad if not isinstance(eng, E.MonteCarloMarginalization)
                                 else {"target": "c9", "evidence": {"r3": torch.tensor([[2.0]])}})
        with pytest.raises(ValueError, match="Found values outside support."):
            eng.infer_posterior(vbn, q)
    with pytest.raises(ValueError, match="Found values outside support."):
        cpd_log_prob(vbn, "a4", torch.tensor([[1.0]]), torch.tensor([[0.5]]))
    assert not launches


def test_walk_entry_points_refuse_each_others_plans():
    fx = fixture()
    vbn = fx["vbn"]
    dev = torch.device("cuda:0")
    pk = E.packed_model(vbn, dev)
    plan = E._plan(pk, ("test-anc",), latent=list(pk.model.topo), fixed=[], logp=[], out_nodes=["c9"],
                   shared_roots=True, mode=2)
    fx0 = torch.zeros(1, 1, device=dev)
    with pytest.raises(Exception, match="vbn_hip_table_walk"):
        ops.walk(plan.steps, plan.in_cols, pk.params, fx0, None, plan.out_cols, 1, 64, plan.n_slots, 1, 1, False, 1,
                 len(plan.noise_nodes), pk.dmax, 1, 2, 0, 1, 0, False, plan.kind_mask, 0, 0)
