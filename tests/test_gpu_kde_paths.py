"""The KDE step's wave-uniform and per-lane branches, two of them per wave, against the float64
reference of tests/kde_reference.py (csrc kde_index_mfma, kde_index_moments, kde_scan,
kde_logp_mfma, kde_index_valu).

Every case is a single-node walk with per-particle parents (B = 1, S = 64 x waves <= 512,
``fixed_per_particle``; no precompute) and injected draws, so each lane has its own parent value
and its own categorical uniform.  A wave is 64 consecutive particles:

| wave | parents | branch |
|---|---|---|
| W0  | on the data | moment table (one feature, set A); factored MFMA otherwise |
| W1  | W0, lane 37 off the table's grid, |x'|^2 = 36 | the whole wave on MFMA <1,1>, factored |
| W2- | W0, lane 21 at |x'| = sqrt(96) (1 - 1e-3) | still factored |
| W2+ | W0, lane 21 at |x'| = sqrt(96) (1 + 1e-3) | full form for the whole wave |
| W3  | odd lanes >= 13 scaled units beyond the data | odd lanes rescued, full form |
| W4  | set B, x' ~ -9.5 | factored form, every weight underflows: rescue with sigma = max a' |
| W5- / W5+ | set B widened, all |x'|^2 <= 96 / some beyond | cancelling terms of ~66 on both sides |
| W6  | largest a' - sigma graded from -90 to below -149 | sums that lost mass to v_exp_f32's flush: rescue (kde_tiny) |

(tests/test_kde_reference.py asserts these lane sets on the host.)  Lanes 0-6 of every wave carry
crafted uniforms (0, 2^-24, 0.5, 1 - 2^-24, the CDF at the end of the first chunk, at a half-chunk
boundary, at the start of the last chunk), the others seeded multiples of 2^-24.

Sampling: every particle's index must lie within ``kde_reference.margin`` (derived, per
particle) of its float64 CDF interval.  Path identity: the same model packed without moment
tables must give bit-identical W1, W2+-, W3, W6 (and set B's waves): one off-grid lane takes the
whole wave off the table.  ``plan_jit=2`` must equal the interpreter bit for bit; ``kde_valu`` is judged against
the reference.  Log-density: the reused-denominator form (sample + score in one step, ``lsp``)
and the two-pass form (node fixed) against ``kde_logp64`` at the sampled value, 1e-4 absolute,
identical NaN / inf pattern, with a wave whose odd lanes' target value is >= 13 scaled units from
every target point (``sy`` underflows on those lanes only: per-lane VALU fallback; wave FB), and
one whose odd lanes' values are graded 9.5 .. 12.6 units away (wave NB: ``sy`` positive but with
terms below 2^-126 flushed).

Sizes (kde_reference.SAMPLING_CASES ...): set A at M = 1 .. 10000 for one feature and 100, 4096,
7169 for two and three; set B at 100 and 1000.  Set B's a' has terms of ~150, so its derived margin
is 1.2e-5 .. 2.4e-5 at any M; at M = 7169 a point holds less mass than that (18-26 % of the
particles have two acceptable indices), at M = 1000 under 10 %.  The log-density cases keep set B
at M = 7169 too (the log-density is judged at the value returned, whichever acceptable index was
chosen); tests/test_kde_reference.py asserts the share of every other case on the host.

Measured on MI355X (largest miss = how far a uniform lies outside the chosen index's interval,
over every case of a wave; beside it the smallest derived margin of any particle of that wave):

| wave | largest miss | smallest margin |   | wave | largest miss | smallest margin |
|---|---|---|---|---|---|---|
| A W0 (table, dp = 1)  | 2.7e-08 | 8.9e-07 | | B W0  | 2.9e-08 | 1.2e-05 |
| A W0 (MFMA)           | 6.0e-09 | 1.7e-06 | | B W4  | 1.9e-07 | 8.3e-05 |
| A W1                  | 1.4e-09 | 1.7e-06 | | B W5- | 2.8e-08 | 1.2e-05 |
| A W2- / W2+           | 2.6e-09 / 5.5e-09 | 1.7e-06 | | B W5+ | 2.2e-08 | 1.2e-05 |
| A W3                  | 1.3e-08 | 1.7e-06 | | B W6  | 6.9e-08 | 3.4e-05 |
| A W6                  | 2.5e-07 | 3.1e-05 | | kde_valu W0 / W3 | 2.4e-09 / 0 | 1.3e-06 |

The worst miss / margin ratio of any particle is 0.029 (table wave, M = 7168): the derived bound
is a worst-case one and holds with a factor of 35 to spare.  Log-density, largest |error| against
float64 over all cases: reused denominator 3.2e-05, two-pass 3.2e-05 (both on NB / W6 lanes, whose
terms are ~100 in magnitude); on-manifold W0 1.2e-05 / 1.2e-05.  Reused against two-pass at W5
(cancelling terms of ~66 on both sides of |x'|^2 = 96): at most 1.0e-05 (W5-), 1.9e-06 (W5+).
Before the ``kde_tiny`` threshold (csrc), waves W6 / NB failed: index misses up to 0.29 of the
total mass and log-density errors up to 1.2, from sums that were positive but had lost the terms
v_exp_f32 flushes below 2^-126.
"""
import math

import numpy as np
import pytest
import torch

import kde_reference as K

pytestmark = pytest.mark.gpu

SEED_PARENTS, SEED_U = K.SEED_PARENTS, K.SEED_U


def _ids(cases):
    return [f"{c[0]}-{c[1]}-{c[2]}" for c in cases]


def _vbn(model):
    from vectorizedbayesiannetwork_amd import VBN
    return VBN.from_model(model, device="cuda")


def _pk(vbn):
    from vectorizedbayesiannetwork_amd.engines import _device_of, packed_model
    return packed_model(vbn, _device_of(vbn))


def _launch(vbn, parents, *, u=None, z=None, x=None, logp=False, plan_jit=0, kde_valu=False):
    """One single-node walk as cpd.py builds it.  ``x`` None: the node is sampled (``u`` [S]
    categorical uniforms, ``z`` [S] normals injected) and, with ``logp``, scored in the same
    step; ``x`` [S]: the node is fixed at x and scored (both passes).  Returns (lp, xs) [S]."""
    from vectorizedbayesiannetwork_amd import ops
    from vectorizedbayesiannetwork_amd.engines import run_walk
    from vectorizedbayesiannetwork_amd.plan import MODE_SAMPLE, MODE_WEIGHTED, build_plan
    pk = _pk(vbn)
    model = pk.model
    pa = model.parents[K.NODE]
    dev = pk.device
    s = len(u) if x is None else len(x)
    vals = {}
    if pa:
        par = torch.from_numpy(np.ascontiguousarray(parents, np.float32)).to(dev)
        for i, p in enumerate(pa):
            vals[p] = par[:, i:i + 1]
    if x is None:
        plan = build_plan(pk, latent=[K.NODE], fixed=[p for p in model.topo if p in pa],
                          logp=[K.NODE] if logp else [], out_nodes=[K.NODE], shared_roots=False,
                          mode=MODE_WEIGHTED if logp else MODE_SAMPLE, kde_valu=kde_valu,
                          skip=[q for q in model.topo if q != K.NODE and q not in pa])
        noise = {K.NODE: (torch.from_numpy(np.asarray(u, np.float32))[None],
                          torch.from_numpy(np.asarray(z, np.float32))[None, :, None])}
    else:
        vals[K.NODE] = torch.from_numpy(np.asarray(x, np.float32).reshape(-1, 1)).to(dev)
        plan = build_plan(pk, latent=[], fixed=[p for p in model.topo if p in pa or p == K.NODE], logp=[K.NODE],
                          out_nodes=[], shared_roots=False, mode=MODE_WEIGHTED, kde_valu=kde_valu,
                          skip=[q for q in model.topo if q != K.NODE and q not in pa])
        noise = None
    if plan.fixed_nodes:
        fx = torch.cat([vals[p] for p in plan.fixed_nodes], dim=1).contiguous()
    else:
        fx = torch.zeros(1, 1, device=dev)
    lp, xs = run_walk(pk, plan, fx, 1, s, seed=0, noise=noise, fixed_per_particle=bool(plan.fixed_nodes),
                      plan_jit=plan_jit)
    torch.cuda.synchronize()
    assert bool(ops.LAST_WALK.get("specialised")) == (plan_jit == 2)
    lp = lp.reshape(-1).cpu().numpy() if (logp or x is not None) else None
    return lp, (xs.reshape(-1).cpu().numpy() if x is None else None)


def _indices(xs, m):
    idx = np.rint(xs).astype(np.int64)
    assert np.array_equal(idx.astype(np.float32), xs), "index model: the sample is the chosen index"
    assert idx.min() >= 0 and idx.max() < m
    return idx


def _judge(label, names, cdf, u, idx, mg):
    """Prints per wave (particles, largest miss, margin there) and asserts every particle."""
    ms = K.miss(cdf, u, idx)
    ok = K.accept_index(cdf, u, idx, mg)
    for w, name in enumerate(names):
        sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
        j = int(np.argmax(ms[sl]))
        print(f"{label} {name}: {K.WAVE} particles, largest miss {ms[sl][j]:.3g} (margin {mg[sl][j]:.3g}; "
              f"smallest margin {mg[sl].min():.3g}), {int((~ok[sl]).sum())} rejected")
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (label, [(int(b), names[b // K.WAVE], int(idx[b]), float(u[b]), float(ms[b]), float(mg[b]))
                                   for b in bad[:8]])
    return ms


def _case(dataset, dp, m, kind, names=None):
    model = K.make_model(m, dp, dataset, kind)
    vbn = _vbn(model)
    pk = _pk(vbn)
    pp, py = K.node_points(model)
    s_p, s_y = K.scales(model.cpds[K.NODE])
    names = names or (K.WAVES_A if dataset == "A" else K.WAVES_B)
    par = K.case_parents(names, pp, s_p, SEED_PARENTS) if dp else None
    return model, vbn, pk, pp, py, (s_p, s_y), names, par


# the cases (kde_reference.SAMPLING_CASES and its neighbours) are shared with
# tests/test_kde_reference.py, which asserts on the host that fewer than 10 % of each case's
# random-uniform particles have more than one acceptable index at the derived margin
@pytest.mark.parametrize("dataset,dp,m,names,valu", K.SAMPLING_CASES, ids=_ids(K.SAMPLING_CASES))
def test_sampling_waves(dataset, dp, m, names, valu, monkeypatch):
    from vectorizedbayesiannetwork_amd import plan as P
    model, vbn, pk, pp, _, (s_p, _), names, par = _case(dataset, dp, m, "index", names)
    tab = K.node_table(pk)
    tabled = dataset == "A" and dp == 1
    assert ("kmt" in pk.nodes[K.NODE].offs) == tabled            # the waves rely on it
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = K.crafted_uniforms(cdf, m, SEED_U, tab)
    zero = np.zeros(len(u), np.float32)
    _, xs = _launch(vbn, par, u=u, z=zero)
    _judge(f"{dataset} dp={dp} M={m}", names, cdf, u, _indices(xs, m), K.margin(pp, par, s_p, tab))
    if dp != 1:
        return
    # the same model packed without moment tables: a fresh model object and a fresh VBN
    monkeypatch.setattr(P, "KDE_MOMENTS", False)
    vbn2 = _vbn(K.make_model(m, dp, dataset, "index"))
    assert "kmt" not in _pk(vbn2).nodes[K.NODE].offs
    _, xs2 = _launch(vbn2, par, u=u, z=zero)
    _judge(f"{dataset} dp={dp} M={m} no tables", names, cdf, u, _indices(xs2, m), K.margin(pp, par, s_p, None))
    for w, name in enumerate(names):
        if name != "W0" or not tabled:
            sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
            assert np.array_equal(xs[sl], xs2[sl]), f"{name}: differs with / without moment tables"


@pytest.mark.parametrize("dataset,dp,m,names,valu", K.JIT_CASES, ids=_ids(K.JIT_CASES))
def test_plan_specialised_walk_is_bit_identical(dataset, dp, m, names, valu):
    """plan_jit=2 (the plan-specialised kernel, compiled in the call) on the same injected draws."""
    model, vbn, pk, pp, _, (s_p, _), names, par = _case(dataset, dp, m, "index", names)
    tab = K.node_table(pk)
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = K.crafted_uniforms(cdf, m, SEED_U, tab)
    zero = np.zeros(len(u), np.float32)
    _, xs0 = _launch(vbn, par, u=u, z=zero, plan_jit=0)
    _, xs2 = _launch(vbn, par, u=u, z=zero, plan_jit=2)
    assert np.array_equal(xs0, xs2)
    _judge(f"plan_jit=2 dp={dp} M={m}", names, cdf, u, _indices(xs2, m), K.margin(pp, par, s_p, tab))


@pytest.mark.parametrize("dataset,dp,m,names,valu", K.VALU_CASES, ids=_ids(K.VALU_CASES))
def test_valu_pass_waves(dataset, dp, m, names, valu):
    """kde_valu=True (packed-VALU pass 1) on W0 and W3, against the reference."""
    model, vbn, pk, pp, _, (s_p, _), names, par = _case(dataset, dp, m, "index", names)
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = K.crafted_uniforms(cdf, m, SEED_U)
    _, xs = _launch(vbn, par, u=u, z=np.zeros(len(u), np.float32), kde_valu=True)
    _judge(f"kde_valu dp={dp} M={m}", names, cdf, u, _indices(xs, m), K.margin(pp, par, s_p, valu=True))


def _sampled_miss(py, ns, cdf, u, z, xs, mg):
    """Density model: the indices whose target + z * noise_scale is the returned sample (to two
    float32 ulps); the smallest miss among them, and whether one of them is acceptable."""
    t = py.reshape(-1).astype(np.float32)
    cand = (t[None, :] + (np.asarray(z, np.float32) * np.float32(ns))[:, None]).astype(np.float32)
    hit = np.abs(cand.astype(np.float64) - xs[:, None].astype(np.float64)) <= 2.0 ** -22 * np.maximum(1.0, np.abs(xs))[:, None]
    assert hit.any(axis=1).all(), "a sample is no target point plus its injected normal"
    lo = np.concatenate([np.zeros((len(u), 1)), cdf[:, :-1]], axis=1)
    uu = np.asarray(u, np.float64)[:, None]
    ms = np.where(hit, np.maximum(np.maximum(lo - uu, uu - cdf), 0.0), np.inf).min(axis=1)
    return ms, ms <= mg


LOGP = K.LOGP_ROOT_CASES + K.LOGP_CASES


@pytest.mark.parametrize("dataset,dp,m,names,valu", LOGP, ids=_ids(LOGP))
def test_log_density_forms(dataset, dp, m, names, valu):
    model, vbn, pk, pp, py, sc, _, par = _case(dataset, dp, m, "density", K.parent_waves(names))
    s_p, s_y = sc
    tab = K.node_table(pk)
    s = K.WAVE * len(names)
    rng = np.random.default_rng([m, dp, 21])
    t = py.reshape(-1).astype(np.float64)
    ns = float(np.float32(s_y))
    z = rng.standard_normal(s).astype(np.float32)
    far = float(t.max()) + 13.2 / float(K.c_scale(s_y))     # >= 13 scaled units beyond every target
    if dp:
        cdf = K.kde_index_cdf64(pp, par, s_p)
        u = K.crafted_uniforms(cdf, m, SEED_U, tab)
        mg = K.margin(pp, par, s_p, tab)
        ref_idx = K.ref_index(cdf, u)
    else:
        u = (rng.integers(0, 2 ** 24, s).astype(np.float64) * K.U24).astype(np.float32)
        ref_idx = np.minimum((u * np.float32(m)).astype(np.int64), m - 1)
    fb = slice((len(names) - 1) * K.WAVE + 1, s, 2)              # the last wave's odd lanes
    z[fb] = ((far - t[ref_idx[fb]]) / ns).astype(np.float32)
    # NB: the wave before it, odd lanes graded 9.5 .. 12.6 scaled units beyond the targets -- the
    # largest term of sy from 2^-90 down across v_exp_f32's flush limit 2^-126 to 2^-158
    nb = slice((len(names) - 2) * K.WAVE + 1, (len(names) - 1) * K.WAVE, 2)
    z[nb] = ((float(t.max()) + rng.uniform(9.5, 12.6, K.WAVE // 2) / float(K.c_scale(s_y)) - t[ref_idx[nb]]) / ns).astype(np.float32)
    lp1, xs = _launch(vbn, par, u=u, z=z, logp=True)
    if dp:
        ms, ok = _sampled_miss(py, ns, cdf, u, z, xs, mg)
    else:
        want = (py.reshape(-1)[ref_idx] + z * np.float32(ns)).astype(np.float32)
        ms, ok = np.abs(xs - want), xs == want
    n_far = int((xs[fb] >= np.float32(t.max() + 13.0 / float(K.c_scale(s_y)))).sum())
    assert n_far >= 24, "the fallback wave's odd lanes must carry far target values"
    # which lanes' sy the kernel must treat as underflowed, decided on the host at the returned
    # values (kde_reference.joint_sums: the full-form sum with the weights v_exp_f32 flushes left
    # out, against csrc kde_tiny): every far FB lane; of NB's odd lanes those below the threshold,
    # at least 8 of them with a largest weight above 2^-149 (a positive sum); printed: how many of
    # those sums have lost more than 2^-17 of their mass to the flush
    js = K.joint_sums(pp, py, par, xs, sc)
    assert js["fallback"][fb][xs[fb] >= np.float32(t.max() + 13.0 / float(K.c_scale(s_y)))].all()
    lossy = js["fallback"][nb] & (js["kept"][nb] > 0) & (js["lost"][nb] > 2.0 ** -17)
    print(f"{dataset} dp={dp} M={m} NB: {int(js['fallback'][nb].sum())} of 32 odd lanes below kde_tiny, "
          f"{int(lossy.sum())} of them with a positive sum that lost mass")
    zone = js["fallback"][nb] & (js["amax"][nb] > K.UNDERFLOW)     # a positive sum the kernel may not trust
    assert js["fallback"][nb][js["amax"][nb] < -109].all() and zone.sum() >= 8
    ref = K.kde_logp64(pp, py, par, xs, sc)
    lp2, _ = _launch(vbn, par, x=xs)
    e1, e2 = np.abs(lp1.astype(np.float64) - ref), np.abs(lp2.astype(np.float64) - ref)
    d12 = np.abs(lp1.astype(np.float64) - lp2.astype(np.float64))
    for w, name in enumerate(names):
        sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
        print(f"{dataset} dp={dp} M={m} {name}: {K.WAVE} particles, largest miss {ms[sl].max():.3g}, "
              f"largest log-density error reused {np.nanmax(e1[sl]):.3g} two-pass {np.nanmax(e2[sl]):.3g}, "
              f"reused vs two-pass {np.nanmax(d12[sl]):.3g}" + (f" ({n_far} far lanes)" if name == "FB" else ""))
    assert ok.all(), np.flatnonzero(~ok)[:8]
    assert np.isfinite(ref).all()
    bad1, bad2 = np.flatnonzero(~K.logp_close(lp1, ref)), np.flatnonzero(~K.logp_close(lp2, ref))
    assert bad1.size == 0, ("reused denominator", [(int(b), names[b // K.WAVE], float(lp1[b]), float(ref[b])) for b in bad1[:8]])
    assert bad2.size == 0, ("two-pass", [(int(b), names[b // K.WAVE], float(lp2[b]), float(ref[b])) for b in bad2[:8]])
