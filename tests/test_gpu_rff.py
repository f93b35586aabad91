"""rff_gaussian on the GPU (csrc/vbn_walk_rff.h) and the gaussian_exact engine, against the
restatements of tests/rff_reference.py on the fixture tests/golden/rff/rff8.pt.

The yardstick of an rff node is its float64 evaluation; its error scale ``sigma_ref`` is the RMS
deviation of the reference's own float32 op sequence from that float64 value on the same rows
(ridge 1e-6 leaves sum |coef| ~ 1e5, so float32 rounding of each projection shows in loc).  The
step is held to RMS <= 2 sigma_ref and max <= 10 sigma_ref (a misplaced feature row or lane costs
O(|coef|) >= 1e3 sigma_ref).  Measured on MI355X (RMS / sigma_ref, max / sigma_ref; rows of the
fit data, then the same rows x 50):
  x2 (F 256, 2 parents) 0.71, 2.4 | 0.86, 5.1     x4 (F 72, 3 parents) 1.21, 5.0 | 1.07, 8.4
  x6 (F 256, 3 parents) 0.96, 3.2 | 0.90, 3.8     chain b (F 1, 1 parent) 0.72, 3.8 | 1.02, 5.8
  chain c (F 40, D 2)   0.81, 2.8 | 1.04, 5.6
Engine cases replay the recorded draws, so only the float32 evaluation differs from the oracle:
each output gets 10 x the deviation between the float32 oracle and the same case with every rff
loc evaluated in float64, on top of the float32 tolerances test_gpu_parity.py holds the other
kinds to (which alone apply where no rff node feeds the output).
"""
import math

import pytest
import torch

import rff_reference as R
from golden_noise import gibbs_noise, noise_dict, resample_uniforms
from oracle import vbn_oracle as O

pytestmark = pytest.mark.gpu

S_ATOL, S_RTOL = 1e-5, 1e-5          # test_gpu_parity.py: samples
P_ATOL, P_RTOL = 1e-30, 1e-4         # pdf / weights
LP_ATOL = 1e-4                       # log-densities

_VBN = {}


def _part(name):
    fx = R.load_rff8()
    return fx if name == "dag8" else fx[name]


def _vbn(name):
    if name not in _VBN:
        from vectorizedbayesiannetwork_amd import VBN
        from vectorizedbayesiannetwork_amd.model import model_from_checkpoint
        model = model_from_checkpoint(_part(name)["model"])
        _VBN[name] = (model, VBN.from_model(model, device="cuda"))
    return _VBN[name]


_SIGMA = {}


def _sigma(name, node, mult=1.0):
    """sigma_ref of a node on its fit rows (x mult), computed once on the CPU."""
    key = (name, node, mult)
    if key not in _SIGMA:
        model, _ = _vbn(name)
        _SIGMA[key] = R.sigma_ref(model.cpds[node], R.fit_rows(model, _part(name)["data"], node, mult))
    return _SIGMA[key]


def _rff_nodes(name, roots=False):
    from vectorizedbayesiannetwork_amd.model import model_from_checkpoint
    m = model_from_checkpoint(_part(name)["model"])
    return [n for n in m.topo if m.cpds[n].kind == "rff_gaussian" and (roots or not m.cpds[n].is_root)]


# ---- 6. fails without the feature ------------------------------------------------------------------
def test_rff_model_and_gaussian_exact_exist():
    from vectorizedbayesiannetwork_amd.registry import INFERENCE_REGISTRY
    model, vbn = _vbn("dag8")
    assert sum(r.kind == "rff_gaussian" for r in model.cpds.values()) == 4
    assert INFERENCE_REGISTRY["gaussian_exact"].__name__ == "GaussianExact"
    assert vbn.cpd("x2").cpd_type == "RFFGaussianCPD"


# ---- 1. per-node accuracy: the criterion for the cosine ---------------------------------------------
@pytest.mark.parametrize("name,node", [("dag8", n) for n in _rff_nodes("dag8")] + [("chain", n) for n in _rff_nodes("chain")])
@pytest.mark.parametrize("mult", [1.0, 50.0])
def test_node_accuracy_against_float64(name, node, mult):
    from vectorizedbayesiannetwork_amd import cpd as C
    model, vbn = _vbn(name)
    rec = model.cpds[node]
    par = R.fit_rows(model, _part(name)["data"], node, mult)
    assert par.shape[0] >= 400 if name == "chain" else par.shape[0] >= 512
    D = rec.output_dim
    got = C.cpd_params(vbn, node, par.cuda()).cpu()                       # [N, 1, loc ++ scale]
    loc64, scale64 = R.params64(rec, par.unsqueeze(1))
    sig = _sigma(name, node, mult)
    err = got[..., :D].double() - loc64
    rms, mx = float(err.pow(2).mean().sqrt()), float(err.abs().max())
    print(f"{name}.{node} x{mult:g}: sigma_ref {sig:.3e}  RMS/sigma {rms / sig:.3f}  max/sigma {mx / sig:.3f}")
    assert torch.equal(got[..., D:], scale64.float())
    assert rms <= 2.0 * sig, (rms / sig)
    assert mx <= 10.0 * sig, (mx / sig)


# ---- 2. walk semantics with replayed draws ----------------------------------------------------------
def _walk_all(name, case, mode, plan_jit):
    """One walk of the case's query with every node written out: (lp [B, S] or empty, {node: [B, S, D]})."""
    from vectorizedbayesiannetwork_amd import plan as P
    from vectorizedbayesiannetwork_amd.engines import _fixed_buffer, _fixed_values, packed_model, run_walk
    model, vbn = _vbn(name)
    pk = packed_model(vbn, torch.device("cuda", torch.cuda.current_device()))
    q = vbn._normalize_query(case["query"])
    vals = _fixed_values(q, pk.device)
    plan = R.all_nodes_plan(pk, case, mode == P.MODE_WEIGHTED)
    b = int(next(iter(vals.values())).shape[0])
    lp, xs = run_walk(pk, plan, _fixed_buffer(plan, vals, b, pk.device), b, case["n_samples"], seed=0,
                      noise=noise_dict(case, model, 0), plan_jit=plan_jit)
    torch.cuda.synchronize()
    out, c = {}, 0
    for n in model.topo:
        out[n] = xs[..., c:c + model.out_dim(n)].cpu()
        c += model.out_dim(n)
    return lp.cpu(), out


def _check_walk(name, case, lp, xs):
    model, _ = _vbn(name)
    nd = noise_dict(case, model, 0)
    ev = case["query"]["evidence"]
    fixed = set(ev) | set(case["query"]["do"])
    b, s = xs[model.topo[0]].shape[:2]
    want_lp = torch.zeros(b, s, dtype=torch.float64)
    lp_bound = torch.zeros(b, s, dtype=torch.float64)
    for n in model.topo:
        rec = model.cpds[n]
        pt = torch.cat([xs[p] for p in model.parents[n]], dim=-1) if model.parents[n] else None   # as the GPU sampled them
        if rec.kind == "rff_gaussian":
            tol = 10.0 * _sigma(name, n) if pt is not None else 0.0
            if pt is None:
                loc = rec.state["mean_y"].double().view(1, 1, -1).expand(b, s, -1)
                scale = R.scale32(rec).double().view(1, 1, -1).expand(b, s, -1)
            else:
                loc, scale = R.params64(rec, pt)
            if n not in fixed:
                eps = nd[n][1].double()
                want = loc + eps * scale
                err = float((xs[n].double() - want).abs().max())
                assert err <= tol + 1e-6 * float(1 + want.abs().max()), (n, err, tol)
            if n in ev:
                term = R.log_prob64(rec, xs[n], pt)
                want_lp += term
                # loc off by <= tol, then the float32 rounding of the quadratic itself (a few ulp of it)
                lp_bound += (((xs[n].double() - loc).abs() / scale ** 2 * tol + 0.5 * tol ** 2 / scale ** 2).sum(-1)
                             + 1e-5 + 1e-6 * term.abs())
        elif n in ev:
            # the other kinds: test_gpu_parity.py's log-density tolerance, plus its relative 1e-4 on the
            # term itself -- evidence far off the manifold (|z| ~ 80 below an observed rff node here)
            # multiplies the MLP's ~1e-6 relative error in loc and scale by z^2
            term = O.cpd_log_prob(rec, xs[n], pt).double()
            want_lp += term
            lp_bound += LP_ATOL + P_RTOL * term.abs()
    if lp.numel():
        assert ((lp.double() - want_lp).abs() <= lp_bound).all(), float(((lp.double() - want_lp).abs() - lp_bound).max())


def test_walk_semantics_with_replayed_draws():
    from vectorizedbayesiannetwork_amd import ops
    from vectorizedbayesiannetwork_amd import plan as P
    for case, weighted in R.jit_walk_cases(_part("dag8")):
        mode = P.MODE_WEIGHTED if weighted else P.MODE_SAMPLE
        lp0, xs0 = _walk_all("dag8", case, mode, 0)
        assert not ops.LAST_WALK.get("specialised")
        _check_walk("dag8", case, lp0, xs0)
        lp1, xs1 = _walk_all("dag8", case, mode, 2)                      # the plan-specialised walk
        assert ops.LAST_WALK.get("specialised")
        assert torch.equal(lp0, lp1) and all(torch.equal(xs0[n], xs1[n]) for n in xs0)
    # the chain: one feature, one input, a two-dimensional node
    for case in _part("chain")["cases"]:
        if case["engine"] == "ancestral":
            _check_walk("chain", case, *_walk_all("chain", case, P.MODE_SAMPLE, 0))
        elif case["engine"] == "likelihood_weighting":
            _check_walk("chain", case, *_walk_all("chain", case, P.MODE_WEIGHTED, 0))


# ---- 3. edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,node", [("chain", "a"), ("chain", "b"), ("chain", "c"), ("dag8", "x0"), ("dag8", "x4")])
def test_cpd_surface_edges(name, node):
    """F = 1 with one input (b), the two-dimensional node with 40 features (c), F = 72 (x4) and the
    root nodes (a, x0), through cpd_sample / cpd_log_prob against the recorded outputs."""
    from vectorizedbayesiannetwork_amd import cpd as C
    model, vbn = _vbn(name)
    rec = model.cpds[node]
    case = next(c for c in _part(name)["cases"] if c["engine"] == "cpd" and c["node"] == node)
    par, n = case["parents"], case["n_samples"]
    pc = None if par is None else par.cuda()
    tol = 0.0 if rec.is_root else 10.0 * _sigma(name, node)
    xs = C.cpd_sample(vbn, node, pc, n, _noise=noise_dict(case, model, 0)).cpu()
    ref = case["outputs"]["sample"]
    assert float((xs - ref).abs().max()) <= tol + 1e-6 * float(1 + ref.abs().max())
    scale = R.scale32(rec).view(1, 1, -1)
    for x, key in ((ref, "log_prob_sampled"), (case["x"], "log_prob_x")):
        lp = C.cpd_log_prob(vbn, node, x.cuda(), pc).cpu()
        x3 = O._x3(x)
        p3 = None if par is None else O._expand_s(par, x3.shape[1])
        want = R.log_prob64(rec, x3, p3)
        if rec.is_root:
            bound = torch.full_like(want, 1e-5)
        else:
            loc = R.params64(rec, p3)[0]
            bound = ((x3.double() - loc).abs() / scale ** 2 * tol + 0.5 * tol ** 2 / scale ** 2).sum(-1) + 1e-5
        assert ((lp.double() - want).abs() <= bound).all(), key
        assert ((lp - case["outputs"][key]).abs().double() <= 2 * bound + LP_ATOL).all(), key


def test_nan_parent_gives_nan_loc_and_ragged_fixed_logp():
    from vectorizedbayesiannetwork_amd import cpd as C
    model, vbn = _vbn("dag8")
    node = "x6"
    rec = model.cpds[node]
    par = R.fit_rows(model, _part("dag8")["data"], node)[:150].clone()       # 2 1/3 waves
    par[7, 1] = float("nan")
    par[133, 0] = float("nan")
    got = C.cpd_params(vbn, node, par.cuda()).cpu()
    nan = torch.isnan(got[:, 0, 0])
    assert nan.nonzero().flatten().tolist() == [7, 133]
    assert torch.isfinite(got[:, 0, 1]).all()
    # FIXED + LOGP at S = 50 per query: 150 particles, a ragged last wave, per-particle parents
    x = _part("dag8")["data"][node][:150].reshape(3, 50, 1)
    p3 = R.fit_rows(model, _part("dag8")["data"], node)[:150].reshape(3, 50, -1)
    lp = C.cpd_log_prob(vbn, node, x.cuda(), p3.cuda()).cpu()
    loc, scale = R.params64(rec, p3)
    tol = 10.0 * _sigma("dag8", node)
    bound = ((x.double() - loc).abs() / scale ** 2 * tol + 0.5 * tol ** 2 / scale ** 2).sum(-1) + 1e-5
    assert lp.shape == (3, 50) and ((lp.double() - R.log_prob64(rec, x, p3)).abs() <= bound).all()


# ---- 4. engines end to end against the patched oracle ---------------------------------------------
def _dev(model, case):
    """Per output: max |float32 oracle - the same case with every rff loc in float64|."""
    o32 = R.run_engine_case(model, case)
    with R.precision(64):
        o64 = R.run_engine_case(model, case)
    return o32, {k: float((o32[k].double() - o64[k].double()).abs().nan_to_num(0.0).max())
                 for k in o32 if isinstance(o32[k], torch.Tensor)}


def _close(name, got, ref, atol, rtol, extra):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), name
    err = (got - ref).abs().nan_to_num(0.0)
    bad = err > atol + rtol * ref.abs().nan_to_num(0.0) + 10.0 * extra
    print(f"{name}: max err {float(err.max()):.3g}, float32-vs-float64 deviation {extra:.3g}")
    assert not bad.any(), f"{name}: max err {float(err.max()):.3g}, bound 10 x {extra:.3g} + {atol} + {rtol} |x|"


def _engine_ids():
    keep = ("monte_carlo_marginalization", "likelihood_weighting", "importance_sampling", "ancestral",
            "resampled_importance_sampling", "rao_blackwellized_marginalization", "gibbs")
    return [pytest.param(i, id=f"{i}-{c['engine']}") for i, c in enumerate(_part("dag8")["cases"]) if c["engine"] in keep]


@pytest.mark.parametrize("idx", _engine_ids())
def test_engine_case_against_patched_oracle(idx):
    from vectorizedbayesiannetwork_amd import engines as E
    model, vbn = _vbn("dag8")
    case = _part("dag8")["cases"][idx]
    eng, n, p, q = case["engine"], case["n_samples"], case["params"], case["query"]
    qq = vbn._normalize_query(q)
    ref, dev = _dev(model, case)
    for k, v in case["outputs"].items():
        # the oracle here against the recorded reference: bit for bit on the host that recorded it
        # (tests/test_rff_reference.py); another CPU's cosine and sgemm may differ in the last ulp
        if isinstance(v, torch.Tensor) and k in dev:
            _close(f"oracle-vs-recorded {k}", ref[k], v, S_ATOL, max(S_RTOL, P_RTOL), dev[k])
    print(f"{eng}: float32-vs-float64 deviation {dev}")
    nd0 = noise_dict(case, model, 0) if eng != "gibbs" else None
    if eng == "monte_carlo_marginalization":
        pdf, xs = E.MonteCarloMarginalization(n_samples=n).infer_posterior(vbn, qq, _noise=nd0)
    elif eng == "likelihood_weighting":
        pdf, xs = E.LikelihoodWeighting(n_samples=n, normalize=p.get("normalize", True)).infer_posterior(vbn, qq, _noise=nd0)
    elif eng == "importance_sampling":
        e = E.ImportanceSampling(n_samples=n)
        e.ess_threshold = p.get("ess_threshold", 0.1)
        pdf, xs = e.infer_posterior(vbn, qq, _noise=nd0, _noise_fallback=noise_dict(case, model, 1))
        assert e._last_fallback == ref["fallback"]
        _close("ess", e._last_ess, ref["ess"], 1e-5, 1e-4, dev["ess"])
    elif eng == "ancestral":
        pdf, xs = None, E.AncestralSampler(n_samples=n).sample(vbn, qq, n, _noise=nd0)
    elif eng == "resampled_importance_sampling":
        e = E.ResampledImportanceSampling(n_samples=n, **p)
        pdf, xs = e.infer_posterior(vbn, qq, _noise=nd0, _resample_u=[u.cuda() for u in resample_uniforms(case)])
        assert e._last_resampled == ref["resampled"] is True
    elif eng == "rao_blackwellized_marginalization":
        e = E.RaoBlackwellizedMarginalization(n_samples=n, n_particles=p["n_particles"])
        pdf, xs = e.infer_posterior(vbn, qq, _noise=nd0, _noise_fallback=noise_dict(case, model, 1))
        assert e._last_fallback == ref["fallback"] is False and (e._last_reason or "") == ref["reason"]
    else:
        latent = [x for x in model.topo if x not in q["evidence"] and x not in q["do"]]
        noise = gibbs_noise(case, model, latent, max(model.out_dim(x) for x in model.topo))
        pdf, xs = None, E.GibbsSampler(n_samples=n, **p).sample(vbn, qq, n, _noise=noise)
    torch.cuda.synchronize()
    _close("samples", xs, ref["samples"], S_ATOL, S_RTOL, dev["samples"])
    if pdf is not None:
        _close("pdf", pdf, ref["pdf"], P_ATOL, P_RTOL, dev["pdf"])


def test_gibbs_half_wave_launch_matches_full_wave():
    """wave_particles 32 (lanes 32-63 mirror 0-31, group 0 only) gives the full-wave launch's chains
    bit for bit: the two lane halves' float64 partial sums of a particle are the same numbers added
    in either order.  301 chains: a partial last wave."""
    from vectorizedbayesiannetwork_amd import VBN, synthetic
    from vectorizedbayesiannetwork_amd.engines import GibbsSampler
    from vectorizedbayesiannetwork_amd.model import random_init_model
    g = synthetic.random_dag(10, seed=4)
    data = synthetic.sem_data(g, 512, seed=0)
    kinds = synthetic.round_robin_kinds(g, ("rff_gaussian", "gaussian_nn", "rff_gaussian", "linear_gaussian"))
    model = random_init_model(g, kinds, data, seed=0, overrides={"rff_gaussian": {"n_features": 72}})
    vbn = VBN.from_model(model, device="cuda")
    target, ev_nodes = synthetic.default_query_nodes(g, seed=1)
    B = 301
    ev = {n: data[n][:B].reshape(B, 1).clone() for n in ev_nodes}
    q = vbn._normalize_query({"target": target, "evidence": ev})
    outs = [GibbsSampler(n_samples=4, burn_in=2, n_steps=1, collect="chain", seed=11, wave_particles=wp).sample(vbn, q)
            for wp in (64, 32)]
    assert outs[0].shape == (B, 4, 1) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


# ---- 5. gaussian_exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(R.load_rff8()["exact"]["cases"])))
def test_gaussian_exact_case(idx):
    from vectorizedbayesiannetwork_amd.engines import GaussianExact
    model, vbn = _vbn("exact")
    case = _part("exact")["cases"][idx]
    q, n = case["query"], case["n_samples"]
    ref, dev = _dev(model, case)
    e = GaussianExact(n_samples=n, **case["params"])
    pdf, xs = e.infer_posterior(vbn, vbn._normalize_query(q), _noise=noise_dict(case, model, 0))
    torch.cuda.synchronize()
    assert e._last_fallback == ref["fallback"] == case["outputs"]["fallback"]
    # linear_gaussian / gaussian_nn targets: the RB gaussian-grid tolerance of test_gpu_parity.py;
    # an rff target's loc (and with it the grid) also gets 10 x its float32-vs-float64 deviation;
    # the pdf is a function of z and the fixed scale alone
    extra = dev["samples"]
    _close("samples", xs, ref["samples"], S_ATOL, S_RTOL, extra)
    _close("pdf", pdf, ref["pdf"], P_ATOL, P_RTOL, 0.0)
    assert pdf.shape == case["outputs"]["pdf"].shape and xs.shape == case["outputs"]["samples"].shape


def test_gaussian_exact_through_the_facade():
    model, vbn = _vbn("exact")
    vbn.set_inference_method("gaussian_exact", n_samples=9)
    pdf, xs = vbn.infer_posterior({"target": "t_rff", "evidence": {"r": torch.tensor([[0.1], [-0.4]])}})
    assert pdf.shape == (2, 9) and xs.shape == (2, 9, 1) and vbn._inference._last_fallback is False
    z = torch.linspace(-4.0, 4.0, 9)
    scale = float(R.scale32(model.cpds["t_rff"]))
    want = torch.exp(-0.5 * (z ** 2 + 2 * math.log(scale) + math.log(2 * math.pi)))
    assert torch.allclose(pdf.cpu(), want.expand(2, -1), rtol=1e-5)
    from vectorizedbayesiannetwork_amd.engines import GaussianExact
    with pytest.raises(RuntimeError, match="has no fallback"):
        GaussianExact(fallback=None).infer_posterior(vbn, vbn._normalize_query({"target": "t_mdn", "evidence": {}}))
