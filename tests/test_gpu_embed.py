"""categorical_embedded_softmax networks on the GPU (csrc/vbn_table_embed.h) against the float64
restatement tests/embed_reference.py.  The bound is 4 e_ref, e_ref = the largest error of the
reference's own recorded float32 log-probs against the restatement on golden/embed/embed6.pt (1.9e-7).
A log-prob error d moves a CDF entry by at most d, so a particle's class may differ only where one of
its uniforms lies within 4 e_ref of a class boundary, and at most 0.1 % of a case's particles may.
Measured on MI355X (bound 7.4e-7): cpd_log_prob within 2.5e-7, cpd_params within 8.7e-8; no particle differed."""
import itertools
import os
import sys

import networkx as nx
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import embed_reference as ER  # noqa: E402
import table_reference as TR  # noqa: E402
from test_gpu_table import noise_of  # noqa: E402
from vectorizedbayesiannetwork_amd import VBN, synthetic  # noqa: E402
from vectorizedbayesiannetwork_amd import engines as E  # noqa: E402
from vectorizedbayesiannetwork_amd.cpd import cpd_forward, cpd_log_prob, cpd_params, cpd_sample  # noqa: E402
from vectorizedbayesiannetwork_amd.model import model_from_checkpoint, random_embed_model  # noqa: E402

pytestmark = pytest.mark.gpu

NODES = ("r2", "r3", "a4", "b9", "c3", "m6", "t2", "d4")
_FX = {}


def fixture():
    if not _FX:
        _FX.update(torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embed", "embed6.pt"),
                              weights_only=True))
        model = model_from_checkpoint(_FX["model"])
        _FX["vbn"] = VBN.from_model(model, device="cuda:0")
        _FX["dm"] = ER.DiscreteModel(model)
        _FX["bound"] = 4 * ER.reference_error(_FX["cases"], _FX["dm"])[0]
    return _FX


def check_particles(xs, ref_xs, margin, what):
    flagged = torch.from_numpy(margin < fixture()["bound"])
    same = (xs.cpu() == ref_xs.float()).all(-1)
    print(f"{what}: {int((~same).sum())} of {same.numel()} particles differ, {int(flagged.sum())} flagged")
    assert bool((same | flagged).all()), "a particle differs whose draws are all clear of the class boundaries"
    assert float((~same).float().mean()) <= 1e-3
    return same


def run_engine(name, vbn, q, n, params, dm, qq, draws, draws_fb, **kw):
    # -> kernel pdf, kernel samples, restatement pdf, restatement samples, margins
    args = (dm, qq["target"], qq["evidence"], qq["do"], n, draws)
    if name == "ancestral":
        return None, E.AncestralSampler(n_samples=n).sample(vbn, q, n, **kw), None, TR.ancestral(*args), draws.margin
    if name == "monte_carlo_marginalization":
        eng, (want, want_xs) = E.MonteCarloMarginalization(n_samples=n), TR.mcm(*args)
    elif name == "likelihood_weighting":
        eng = E.LikelihoodWeighting(n_samples=n, normalize=params.get("normalize", True))
        want, want_xs, _ = TR.lw(*args, normalize=params.get("normalize", True))
    elif name == "importance_sampling":
        eng = E.ImportanceSampling(n_samples=n)
        eng.ess_threshold = params.get("ess_threshold", 0.1)
        want, want_xs, ess, fb = TR.importance(*args, draws_fb, ess_threshold=eng.ess_threshold)
    else:
        eng = E.CategoricalExact(n_samples=n)
        want, want_xs, exact = ER.categorical_exact(*args)
    pdf, xs = eng.infer_posterior(vbn, q, **kw)
    if name == "importance_sampling":
        assert eng._last_fallback == fb and torch.allclose(eng._last_ess.cpu().double(), ess, rtol=1e-4)
        return pdf, xs, want, want_xs, (draws_fb if fb else draws).margin
    if name == "categorical_exact":
        assert eng._last_fallback == (not exact)
    return pdf, xs, want, want_xs, draws.margin


@pytest.mark.parametrize("node", NODES)
def test_log_prob_and_params_within_four_e_ref(node):
    fx = fixture()
    vbn, cpd, rec = fx["vbn"], fx["dm"].cpds[node], fx["vbn"].model.cpds[node]
    valid = [rec.state["_class_values"][d][rec.state["_class_mask"][d].bool()] for d in range(cpd.D)]
    par = None
    if cpd.n_in:                                    # every parent configuration
        par = torch.tensor(list(itertools.product(*[v.tolist() for v in rec.extra["parent_values"]])))
    b = 1 if par is None else par.shape[0]
    x = torch.stack([v[torch.arange(b) % v.numel()] for v in valid], dim=-1)       # classes cycle over the rows
    pp = None if par is None else par.double().unsqueeze(1)
    lp = cpd_log_prob(vbn, node, x, par).cpu().double().view(-1)
    err_lp = float((lp - cpd.log_prob(x.double().unsqueeze(1), pp).view(-1)).abs().max())
    prm = cpd_params(vbn, node, par).cpu().double().view(b, -1)
    err_p = float((prm - cpd.probs(pp, b, 1).reshape(b, -1)).abs().max())
    print(f"{node}: log_prob error {err_lp:.3e}, params error {err_p:.3e}, bound {fx['bound']:.3e}")
    assert err_lp <= fx["bound"] and err_p <= fx["bound"]


@pytest.mark.parametrize("i", range(17 + len(NODES)))
def test_recorded_cases_replay(i):
    fx = fixture()
    vbn, model, case = fx["vbn"], fx["vbn"].model, fx["cases"][i]
    n, ref, noise = case["n_samples"], case["outputs"], noise_of(case, model, 0)
    if case["engine"] == "cpd":
        node, par, tol = case["node"], case["parents"], model.out_dim(case["node"]) * 1.25 * fx["bound"]
        assert torch.equal(cpd_sample(vbn, node, par, n, _noise=noise).cpu(), ref["sample"])
        fwd = cpd_forward(vbn, node, par, n, _noise=noise)
        assert torch.equal(fwd.samples.cpu(), ref["sample"])
        # against the recorded float32 values: the kernel's bound plus the reference's own e_ref, per dim
        assert float((fwd.log_prob.cpu() - ref["log_prob_sampled"]).abs().max()) <= tol
        assert float((cpd_log_prob(vbn, node, case["x"], par).cpu() - ref["log_prob_x"]).abs().max()) <= tol
        return
    qq = case["query"]
    b = TR._batch(qq["evidence"], qq["do"])
    pdf, xs, want, want_xs, margin = run_engine(
        case["engine"], vbn, vbn._normalize_query(qq), n, case["params"], fx["dm"], qq,
        TR.ReplayDraws(case["draws"], b, n, 0), TR.ReplayDraws(case["draws"], b, n, 1), _noise=noise,
        **({"_noise_fallback": noise_of(case, model, 1)} if case["engine"] == "importance_sampling" else {}))
    if tuple(xs.shape[:2]) == margin.shape:
        check_particles(xs, want_xs, margin, case["engine"])
    assert torch.equal(xs.cpu(), ref["samples"]), "samples differ from the recorded ones"
    if pdf is not None:
        assert torch.allclose(pdf.cpu(), ref["pdf"], rtol=1e-4, atol=1e-30), "pdf / weights differ"
        assert torch.allclose(pdf.cpu().double(), want, rtol=1e-4, atol=1e-30)


def production():
    if "prod" not in _FX:
        g = synthetic.random_dag(24, seed=2, max_parents=3)
        topo = list(nx.topological_sort(g))
        cards = {n: 2 + (5 * i) % 8 for i, n in enumerate(topo)}                  # 2..9, mixed
        ov = {topo[5]: dict(hidden_dims=(20,), activation="tanh", embedding_dim=5),
              topo[9]: dict(hidden_dims=(), activation="gelu"), topo[14]: dict(hidden_dims=(33, 64), activation="elu")}
        model = random_embed_model(g, cards, seed=1, tables=topo[2::5], masked={topo[8]: 1, topo[12]: 2}, overrides=ov)
        gen = torch.Generator().manual_seed(5)
        ev = {n: torch.randint(0, cards[n], (4, 1), generator=gen).float() for n in (topo[3], topo[11], topo[20])}
        _FX["prod"] = (VBN.from_model(model, device="cuda:0"), ER.DiscreteModel(model), topo[-1], ev)
    return _FX["prod"]


@pytest.mark.parametrize("b,s", [(1, 40), (2, 50), (4, 1024)])       # 40, 100 and 4096 particles
@pytest.mark.parametrize("engine", ["monte_carlo_marginalization", "likelihood_weighting", "importance_sampling",
                                    "ancestral"])
def test_production_draws_match_the_restatement(engine, b, s):
    vbn, dm, target, ev_all = production()
    qq = {"target": target, "evidence": {k: v[:b] for k, v in ev_all.items()}, "do": {}}
    seed = (4321 << 32) | (91 + b)
    draws = TR.PhiloxTableDraws(E.packed_model(vbn, torch.device("cuda:0")).node_id, seed=seed, n_queries=b, n_samples=s)
    pdf, xs, want, want_xs, margin = run_engine(engine, vbn, vbn._normalize_query(qq), s, {"ess_threshold": 0.0}, dm, qq,
                                                draws, None, seed=seed)
    same = check_particles(xs, want_xs, margin, f"{engine} {b}x{s}")
    if pdf is not None:                 # weights are normalised over a query: compare where its particles all agree
        ok = torch.isclose(pdf.cpu().double(), want, rtol=1e-4, atol=1e-30)
        assert bool((ok | ~same).all()) if engine == "monte_carlo_marginalization" else bool(ok[same.all(dim=1)].all())
