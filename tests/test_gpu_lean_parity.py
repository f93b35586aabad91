"""The production (lean) walk against the oracle, on the kernel's own Philox draws.

Every other parity test injects recorded draws, which selects the walk instantiations that
read a noise buffer.  The bench and every production call run the *lean* instantiation
(no injected draws, no segment state: csrc ``vbn_walk.hip`` kind-set bit 7), which makes its
own Philox draws and pairs Box-Muller normals across steps.  Here the oracle
(oracle/vbn_oracle.py, the reference op sequence) is fed a host replica of exactly those
draws (tests/philox_draws.py) and the two are compared per particle on every DAG of SURVEY
§8(d): cfg2 / cfg3 (32 nodes, B = 8 x S = 1024), cfg4 (64 KDE nodes with M = 10,000 points,
B = 2 x S = 1024) and cfg5 (128 nodes, five families, KDE M = 4096, B = 1 x S = 2048, the
config's own sample count; cfg4's MCM B = 8), for MCM, IS (the whole engine at B = 32 on cfg2 /
cfg3), LW and ancestral, on the step-table interpreter and
the plan-specialised kernel, with the shared-sample precompute on; then one full-size launch
per config (cfg2, cfg4, cfg5) is checked statistically against the oracle with the
reference's own torch RNG.

Tolerances: samples |d| <= 1e-5 + 1e-5 |x|; pdf |d| <= 1e-4 |pdf| (log-density
1e-4); log-weights |d| <= 1e-4.  A categorical (mdn component / softmax_nn class / KDE point)
choice is made from fp32 probabilities on the GPU and from float64 ones on the host; a
particle may differ only if one of its categorical uniforms lies within ``TIE`` (CDF units) of
a class boundary, and the number of such particles is capped and reported.  Reference:
monte_carlo_marginalization.py:60-91, importance_sampling.py:37-93,
likelihood_weighting.py:36-82, sampling/ancestral.py:13-41, cpds/kde.py:151-182.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import vbn_oracle as O
from philox_draws import PhiloxDraws
from workloads import synthetic_workload

pytestmark = pytest.mark.gpu

S_ATOL, S_RTOL = 1e-5, 1e-5
P_ATOL, P_RTOL = 1e-30, 1e-4
LW_ATOL = 1e-4
# |u - CDF boundary| (in units of the row total) below which a class choice may flip: two units
# of float32 roundoff of the total, 2^-23.  The GPU forms the CDF at the draw from float32
# weights and float32 partial sums (KDE: 16 float32 chunk sums added in float64, then a float32
# scan inside the chunk; mdn / softmax_nn: K float32 class probabilities), the oracle in float64
# from the reference's float32 probabilities; their difference at the draw is a few roundoffs of
# the partial sums involved, which are at most the total.  Measured: every particle that has
# differed (cfg4, M = 10,000 points per draw) had its smallest margin at 6e-10 .. 6e-9, 20-200x
# inside this bound, while 6-7 % of cfg4's particles carry a draw inside it (round 5's fixed
# 1e-5 flagged 99.8 %).
# This figure counts partial-sum rounding alone.  The per-particle bound derived stage by stage
# (operand and a' rounding, v_exp_f32, the chunk sums, the scan) is tests/kde_reference.margin:
# a few 1e-6 for KDE nodes on the MFMA pass at M = 10,000, and KDE nodes whose pass 1 comes from
# a moment table carry the table's row bound on top (4e-7 per row, tests/test_kde_moments.py),
# itself larger than TIE -- so a flip on such a node with its margin between TIE and that bound
# would be legitimate and would still be reported here as unexplained.  None has been seen;
# tests/test_gpu_kde_paths.py judges KDE choices against the derived bound, particle by particle.
TIE = 2.0 ** -23
# (B, S) of the per-particle comparisons: sizes the oracle finishes in seconds (cfg4's MCM runs
# 8 queries, its other engines 2)
SIZES = {"cfg2": (8, 1024), "cfg3": (8, 1024), "cfg4": (2, 1024), "cfg5": (1, 2048)}
SIZES_MCM = {**SIZES, "cfg4": (8, 1024)}
SIZES_IS = {"cfg2": (32, 1024), "cfg3": (32, 1024)}
# oracle results shared by the interpreter and plan-specialised runs of one case (same plan,
# same draws): key -> (outputs, draws)
_ORACLE = {}


def _oracle(key, fn, draws):
    if key not in _ORACLE:
        _ORACLE[key] = (fn(draws), draws)
    return _ORACLE[key]


def _workload(cfg_name: str, n_queries: int):
    return synthetic_workload(cfg_name, n_queries, "cuda")


def _provider(plan, pk, seed, b, s, offset=0):
    return PhiloxDraws(plan.steps, pk.node_id, seed=seed, offset=offset, n_queries=b, n_samples=s)


def _mismatch(got, ref, atol, rtol):
    """[B, S] particles whose value differs beyond tolerance (NaN / inf patterns included)."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    if got.dim() == 3:
        got, ref = got.reshape(got.shape[0], got.shape[1], -1), ref.reshape(ref.shape[0], ref.shape[1], -1)
    same_special = (torch.isnan(got) == torch.isnan(ref)) & \
        ((torch.isinf(got) & (got > 0)) == (torch.isinf(ref) & (ref > 0))) & \
        ((torch.isinf(got) & (got < 0)) == (torch.isinf(ref) & (ref < 0)))
    fin = torch.isfinite(ref) & torch.isfinite(got)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(got))
    bad = (~same_special) | (fin & (err > atol + rtol * ref.abs()))
    if bad.dim() == 3:
        bad = bad.any(-1)
    return bad.numpy(), float(err[fin].max()) if fin.any() else 0.0


def _check(name, bad, draws, n_expect):
    """Every differing particle must carry a categorical near-tie (a draw within TIE of a class
    boundary), near-ties must stay a minority of the particles (< 10 %, so the mask
    discriminates), and few particles may differ: at most 0.1 % of the particles plus 1 % of the
    near-tie ones (at least 2).  Measured: cfg4 2 of 2048 differing particles (both with margins
    < 6e-9), 116-141 near-ties; mdn / softmax_nn DAGs 0 of 8192."""
    ties = draws.min_margin() < TIE
    unexplained = bad & ~ties
    print(f"{name}: {int(bad.sum())} differing particles of {bad.size}, "
          f"{int(ties.sum())} with a categorical near-tie (< {TIE}), {draws.n_categorical} categorical draws")
    if bad.any():
        mm = np.sort(draws.min_margin()[bad])
        print(f"{name}: smallest categorical margins of the differing particles {mm[:8].tolist()}; "
              f"particles with a margin < 1e-7 / 3e-7 / 1e-6: {int((draws.min_margin() < 1e-7).sum())} / "
              f"{int((draws.min_margin() < 3e-7).sum())} / {int((draws.min_margin() < 1e-6).sum())}")
    assert bad.shape == (n_expect[0], n_expect[1])
    assert not unexplained.any(), (
        f"{name}: {int(unexplained.sum())} particles differ without a categorical near-tie "
        f"(first at {np.argwhere(unexplained)[0].tolist()})")
    cap = max(2, bad.size // 1000 + int(ties.sum()) // 100)
    assert bad.sum() <= cap, f"{name}: {int(bad.sum())} differing particles (cap {cap})"
    assert ties.sum() < 0.1 * bad.size, f"{name}: the near-tie mask flags {int(ties.sum())} of {bad.size}"


def _errors(got, ref, bad):
    """max |d| over the particles that agree (the tolerance check above covers them)."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    ok = torch.from_numpy(~bad)
    if got.dim() == 3:
        ok = ok.unsqueeze(-1).expand_as(got)
    fin = torch.isfinite(ref) & torch.isfinite(got) & ok
    return float((got - ref).abs()[fin].max()) if fin.any() else 0.0


def _q(target, ev):
    from vectorizedbayesiannetwork_amd.engines import Query
    return Query(target, {k: v.cuda() for k, v in ev.items()})


def _lean_launch(plan_jit):
    """the last launch was the production walk (lean: no injected draws, no segment state), in
    the requested form, with the shared-sample precompute wherever the plan has one"""
    from vectorizedbayesiannetwork_amd import engines as E, ops
    last = E.LAST_LAUNCH
    assert last["noise"] is None and last["state"] is None, "the production walk must be the lean one"
    assert last["precomputed"] == (last["plan"].pc is not None)
    if plan_jit != "auto":
        assert bool(ops.LAST_WALK.get("specialised")) == plan_jit
    return last


@pytest.mark.parametrize("plan_jit", [False, True])
@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg3", "cfg4", "cfg5"])
def test_lean_mcm_matches_oracle(cfg_name, plan_jit):
    from vectorizedbayesiannetwork_amd.engines import MonteCarloMarginalization
    b, s = SIZES_MCM[cfg_name]
    model, vbn, target, ev = _workload(cfg_name, b)
    seed = 20260417
    pdf, xs = MonteCarloMarginalization(n_samples=s, plan_jit=plan_jit).infer_posterior(
        vbn, _q(target, ev), seed=seed)
    torch.cuda.synchronize()
    last = _lean_launch(plan_jit)
    (rpdf, rxs), draws = _oracle(("mcm", cfg_name, seed, b, s),
                                 lambda d: O.monte_carlo_marginalization(model, target, ev, {}, s, d),
                                 _provider(last["plan"], last["pk"], seed, b, s))
    bad_x, _ = _mismatch(xs, rxs, S_ATOL, S_RTOL)
    bad_p, _ = _mismatch(pdf, rpdf, P_ATOL, P_RTOL)
    bad = bad_x | bad_p
    lerr = _errors(torch.log(pdf), torch.log(rpdf), bad)
    print(f"{cfg_name} MCM max |dx| {_errors(xs, rxs, bad):.3g}, max |dlog pdf| {lerr:.3g}")
    _check(f"{cfg_name} MCM", bad, draws, (b, s))


@pytest.mark.parametrize("plan_jit", [False, True])
@pytest.mark.parametrize("cfg_name,engine", [("cfg2", "importance_sampling"), ("cfg2", "likelihood_weighting"),
                                             ("cfg3", "importance_sampling"), ("cfg3", "likelihood_weighting"),
                                             ("cfg4", "likelihood_weighting"), ("cfg5", "likelihood_weighting")])
def test_lean_weighted_walk_matches_oracle(cfg_name, engine, plan_jit):
    """IS (per-query root draws, raw evidence) and LW (shared roots, clamped evidence)
    log-weights and target samples per particle, before normalisation; step-table interpreter
    and plan-specialised kernel."""
    from vectorizedbayesiannetwork_amd.engines import ImportanceSampling, LikelihoodWeighting
    b, s = SIZES[cfg_name]
    model, vbn, target, ev = _workload(cfg_name, b)
    seed = 77001
    is_ = engine == "importance_sampling"
    cls = ImportanceSampling if is_ else LikelihoodWeighting
    eng = cls(n_samples=s, plan_jit=plan_jit)
    log_w, xs = eng._walk(vbn, _q(target, ev), s, clamp=not is_, shared_roots=not is_,
                          kwargs={"_seed_value": seed})
    torch.cuda.synchronize()
    last = _lean_launch(plan_jit)
    draws = _provider(last["plan"], last["pk"], seed, b, s)
    parts, rlw, cols = O._walk_weighted(model, ev, {}, s, draws, clamp=not is_, per_query=is_)
    rxs = parts[..., cols[target]]
    bad_x, _ = _mismatch(xs, rxs, S_ATOL, S_RTOL)
    bad_w, _ = _mismatch(log_w, rlw, LW_ATOL, 0.0)
    bad = bad_x | bad_w
    print(f"{cfg_name} {engine} max |dx| {_errors(xs, rxs, bad):.3g}, max |dlogw| {_errors(log_w, rlw, bad):.3g}")
    _check(f"{cfg_name} {engine} walk", bad, draws, (b, s))


@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg3"])
def test_lean_is_engine_matches_oracle(cfg_name):
    """The whole IS call: walk + wave-reduced softmax / ESS + batch-global fallback decision;
    a query may differ only if one of its particles had a categorical near-tie."""
    from vectorizedbayesiannetwork_amd import engines as E
    from vectorizedbayesiannetwork_amd.engines import ImportanceSampling
    b, s = SIZES_IS[cfg_name]
    model, vbn, target, ev = _workload(cfg_name, b)
    seed = 5150
    eng = ImportanceSampling(n_samples=s)
    w, xs = eng.infer_posterior(vbn, _q(target, ev), seed=seed)
    torch.cuda.synchronize()
    if eng._last_fallback:
        pytest.skip("the IS -> LW fallback fired on this workload (LW walk covered above)")
    last = E.LAST_LAUNCH
    draws = _provider(last["plan"], last["pk"], seed, b, s)
    rw, rxs, ress, rfb = O.importance_sampling(model, target, ev, {}, s, draws)
    assert rfb is False
    tie_q = (draws.min_margin() < TIE).any(axis=1)
    bad_w, ew = _mismatch(w.cpu(), rw, P_ATOL, P_RTOL)
    bad_e, ee = _mismatch(eng._last_ess.cpu().view(-1, 1), ress.view(-1, 1), 1e-5, P_RTOL)
    bad_q = bad_w.any(axis=1) | bad_e[:, 0]
    print(f"{cfg_name} IS engine: {int(bad_q.sum())} differing queries of {b} "
          f"({int(tie_q.sum())} with a categorical near-tie), max |dw| {ew:.3g}, max |dESS| {ee:.3g}")
    assert not (bad_q & ~tie_q).any(), "a query differs without a categorical near-tie"


@pytest.mark.parametrize("plan_jit", [False, True])
@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg3", "cfg4", "cfg5"])
def test_lean_ancestral_matches_oracle(cfg_name, plan_jit):
    from vectorizedbayesiannetwork_amd.engines import AncestralSampler
    b, s = SIZES[cfg_name]
    model, vbn, target, ev = _workload(cfg_name, b)
    seed = 31337
    xs = AncestralSampler(n_samples=s, plan_jit=plan_jit).sample(vbn, _q(target, ev), s, seed=seed)
    torch.cuda.synchronize()
    last = _lean_launch(plan_jit)
    rxs, draws = _oracle(("ancestral", cfg_name, seed, b, s), lambda d: O.ancestral(model, target, ev, {}, s, d),
                         _provider(last["plan"], last["pk"], seed, b, s))
    bad, _ = _mismatch(xs, rxs, S_ATOL, S_RTOL)
    print(f"{cfg_name} ancestral max |dx| {_errors(xs, rxs, bad):.3g}")
    _check(f"{cfg_name} ancestral", bad, draws, (b, s))


def _moments(x: torch.Tensor):
    """per-row mean, std and the standard errors of both (S iid draws per row)."""
    x = x.double()
    s = x.shape[1]
    m = x.mean(1)
    c = x - m[:, None]
    var = (c ** 2).mean(1)
    m4 = (c ** 4).mean(1)
    se_m = (var / s).sqrt()
    se_sd = ((m4 - var ** 2).clamp_min(0) / (4 * var.clamp_min(1e-30) * s)).sqrt()
    return m, var.sqrt(), se_m, se_sd


@pytest.mark.parametrize("cfg_name,nq", [("cfg2", 16), ("cfg4", 4), ("cfg5", 2)])
def test_lean_full_size_statistics(cfg_name, nq):
    """Each MCM config at its full single-GPU size (cfg2 / cfg4: 4096 queries x 1024 samples,
    cfg5: 8192 x 2048; one lean launch, the bench's form) against the oracle with the
    reference's own torch RNG on the first ``nq`` queries: per query, the target sample mean /
    std and the mean pdf agree within 5 Monte-Carlo standard errors."""
    from vectorizedbayesiannetwork_amd import synthetic
    from vectorizedbayesiannetwork_amd.engines import MonteCarloMarginalization
    cfg = synthetic.CONFIGS[cfg_name]
    b, s = cfg["B"], cfg["S"]
    model, vbn, target, ev = _workload(cfg_name, b)
    pdf, xs = MonteCarloMarginalization(n_samples=s).infer_posterior(vbn, _q(target, ev), seed=99)
    torch.cuda.synchronize()
    _lean_launch("auto")
    assert pdf.shape == (b, s) and torch.isfinite(pdf).all() and torch.isfinite(xs).all()
    torch.manual_seed(123)
    rpdf, rxs = O.monte_carlo_marginalization(model, target, {k: v[:nq] for k, v in ev.items()}, {}, s,
                                              O.TorchDraws())
    g_m, g_sd, g_sem, g_sesd = _moments(xs[:nq, :, 0].cpu())
    r_m, r_sd, r_sem, r_sesd = _moments(rxs[:, :, 0])
    gp_m, _, gp_se, _ = _moments(pdf[:nq].cpu())
    rp_m, _, rp_se, _ = _moments(rpdf)
    z_m = (g_m - r_m).abs() / (g_sem ** 2 + r_sem ** 2).sqrt()
    z_sd = (g_sd - r_sd).abs() / (g_sesd ** 2 + r_sesd ** 2).sqrt()
    z_p = (gp_m - rp_m).abs() / (gp_se ** 2 + rp_se ** 2).sqrt()
    print(f"{cfg_name} full size ({b} x {s}): max z mean {float(z_m.max()):.2f}, std {float(z_sd.max()):.2f}, "
          f"pdf {float(z_p.max()):.2f}")
    assert float(z_m.max()) < 5 and float(z_sd.max()) < 5 and float(z_p.max()) < 5


def test_lean_cfg3_is_statistics():
    """cfg3 (mdn + softmax_nn, importance sampling) at 64 queries: self-normalised posterior
    mean of the target per query within 5 standard errors (delta-method SE) of the oracle's
    with the reference's torch RNG; median ESS ratio within 10 %."""
    from vectorizedbayesiannetwork_amd.engines import ImportanceSampling
    nq = 64
    model, vbn, target, ev = _workload("cfg3", nq)
    eng = ImportanceSampling(n_samples=1024)
    w, xs = eng.infer_posterior(vbn, _q(target, ev), seed=7)
    torch.cuda.synchronize()
    torch.manual_seed(321)
    rw, rxs, ress, rfb = O.importance_sampling(model, target, ev, {}, 1024, O.TorchDraws())
    assert eng._last_fallback == rfb

    def post(w, x):
        w, x = w.double(), x[..., 0].double()
        m = (w * x).sum(1)
        se = ((w ** 2) * (x - m[:, None]) ** 2).sum(1).sqrt()
        return m, se
    gm, gse = post(w.cpu(), xs.cpu())
    rm, rse = post(rw, rxs)
    ok = torch.isfinite(gm) & torch.isfinite(rm)
    assert torch.equal(torch.isfinite(gm), torch.isfinite(rm))
    z = ((gm - rm).abs() / (gse ** 2 + rse ** 2).sqrt().clamp_min(1e-12))[ok]
    print(f"cfg3 IS statistics: {int(ok.sum())} finite queries, max z {float(z.max()):.2f}")
    assert float(z.max()) < 5
    if not rfb:
        ratio = (eng._last_ess.cpu().double() / ress.double())[ok]
        assert abs(float(ratio.median()) - 1) < 0.1
