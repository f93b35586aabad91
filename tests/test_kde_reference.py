"""The float64 KDE reference and the crafted waves of tests/test_gpu_kde_paths.py, checked on the
host: the reference agrees with the pinned oracle, every crafted wave has exactly the lane sets
it claims (off the moment table's grid, beyond the factored form's limit, all-underflow), and
the checker rejects a chunk boundary off by one block and a dropped sigma correction while
leaving fewer than 10 % of the particles ambiguous at the derived margin.
"""
import math

import numpy as np
import pytest
import torch

import kde_reference as K
from oracle import vbn_oracle as O
from vectorizedbayesiannetwork_amd import plan as P

S = 256


class _Inverse:
    """Draw provider: the float64 inverse-CDF choice from the oracle's own probabilities."""

    def __init__(self, u, z):
        self.u, self.z = torch.as_tensor(u, dtype=torch.float64).reshape(-1), z

    def categorical(self, probs, replacement=True):
        cdf = probs.double().cumsum(-1)
        cdf = cdf / cdf[:, -1:]
        return (cdf <= self.u[:, None]).sum(-1).clamp(max=probs.shape[1] - 1)

    def randint(self, n, count):
        return (self.u.float() * float(n)).long().clamp(max=n - 1)

    def normal(self, shape):
        return self.z.reshape(shape)


def _packed(model):
    return P.PackedModel(model, torch.device("cpu"))


@pytest.mark.parametrize("dataset,dp,m", [("A", 1, 7169), ("B", 1, 7169), ("A", 2, 100), ("B", 3, 100)])
def test_reference_matches_oracle_sampling(dataset, dp, m):
    """Index model, on-manifold parents: the oracle's index (float32 softmax, float64 inverse
    CDF of it) equals the reference's wherever exactly one index is acceptable."""
    model = K.make_model(m, dp, dataset, "index")
    rec = model.cpds[K.NODE]
    s_p, _ = K.scales(rec)
    pp, _ = K.node_points(model)
    par = K.case_parents(("W0",) * (S // K.WAVE), pp, s_p, 1)
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = K.crafted_uniforms(cdf, m, 2)
    xs = O.cpd_sample(rec, torch.from_numpy(par)[None], S, _Inverse(u, torch.zeros(S, 1)))
    idx = xs.reshape(-1).numpy().astype(np.int64)
    mg = K.margin(pp, par, s_p)
    one = K.n_acceptable(cdf, u, mg) == 1
    ref = K.ref_index(cdf, u)
    print(f"{dataset} dp={dp} M={m}: {int(one.sum())} of {S} unambiguous, margin <= {mg.max():.3g}")
    assert one.sum() > S // 4
    assert np.array_equal(idx[one], ref[one])
    assert K.accept_index(cdf, u, idx, mg).all()


@pytest.mark.parametrize("dataset,dp,m", [("A", 0, 100), ("A", 1, 7169), ("B", 1, 100), ("A", 2, 100), ("B", 3, 7169)])
def test_reference_matches_oracle_log_prob(dataset, dp, m):
    model = K.make_model(m, dp, dataset, "density")
    rec = model.cpds[K.NODE]
    pp, py = K.node_points(model)
    rng = np.random.default_rng(m + dp)
    x = rng.standard_normal((S, 1)).astype(np.float32) * 1.3
    par = K.case_parents(("W0",) * (S // K.WAVE), pp, K.scales(rec)[0], 3) if dp else None
    ref = K.kde_logp64(pp, py, par, x, K.scales(rec))
    got = O.cpd_log_prob(rec, torch.from_numpy(x)[None], None if par is None else torch.from_numpy(par)[None])
    err = np.abs(got.reshape(-1).double().numpy() - ref)
    print(f"{dataset} dp={dp} M={m}: oracle vs float64 log-density, largest difference {err.max():.3g}")
    assert K.logp_close(got.reshape(-1).numpy(), ref).all()


def _expect(name, ls, lanes, tabled):
    odd = set(range(1, K.WAVE, 2))
    every = set(range(K.WAVE))
    got = {k: set(np.flatnonzero(ls[k][lanes] if k in ls else []).tolist()) for k in ("over", "off", "under")}
    full, table = bool(ls["full"][lanes].all()), bool(ls["table"][lanes].all())
    assert ls["full"][lanes].all() == ls["full"][lanes].any()
    want = {
        "W0": (set(), set(), set(), False, tabled),
        "W1": (set(), {K.LANE_OFF} if tabled else set(), set(), False, False),
        "W2-": (set(), {K.LANE_EDGE} if tabled else set(), set(), False, False),
        "W2+": ({K.LANE_EDGE}, {K.LANE_EDGE} if tabled else set(), set(), True, False),
        "W3": (odd, odd if tabled else set(), odd, True, False),
        "W4": (set(), set(), every, False, False),
    }
    if name in want:
        assert (got["over"], got["off"], got["under"], full, table) == want[name], name
        # exactly the all-underflow lanes are rescued; no other lane loses mass to the flush
        assert set(np.flatnonzero(ls["rescued"][lanes]).tolist()) == got["under"], name
        assert (ls["lost"][lanes][~ls["rescued"][lanes]] == 0).all(), name
    elif name == "W5-":
        assert not got["over"] and not got["under"] and not full and not table
        assert ls["sq"][lanes][K.LANE_B] > 95.9 and (ls["sq"][lanes] > 85).sum() >= 3
    elif name == "W5+":
        assert K.LANE_B in got["over"] and not got["under"] and full and not table
        assert ls["sq"][lanes][K.LANE_B] < 96.1 and (~ls["over"][lanes]).sum() >= 32
    elif name == "W6":
        # graded across the limit: some lanes all-underflow, many with their largest weight in
        # v_exp_f32's flush zone (2^-149 .. 2^-110: a positive sum that has lost mass), none clear
        # The rescue runs where pass 1's sum with the flushed weights left out is below kde_tiny(M)
        # = M 2^-109 (lane_sets' float64 replay; no lane within 1 % of the threshold, so the
        # replay decides).  Certain either way: largest weight below 2^-109 -> rescued; largest
        # weight above M 2^-109 -> not.
        a, m = ls["amax"][lanes], ls["m"]
        resc, ratio = ls["rescued"][lanes], ls["ratio"][lanes]
        assert full == (got["over"] == every) and not table
        decided = np.abs(np.log2(np.maximum(ratio, 1e-300))) > 0.015
        assert decided.sum() >= K.WAVE - 2
        assert resc[a < -109].all() and not resc[(a >= -109 + np.log2(m)) & decided].any()
        assert set(np.flatnonzero(resc).tolist()) >= got["under"]
        zone = resc & decided & (a > K.UNDERFLOW)              # a positive sum that had lost mass: the fixed case
        assert len(got["under"]) >= 3 and zone.sum() >= 16 and a.max() < -85
        if m > 1:
            assert (ls["lost"][lanes][zone] > 2.0 ** -17).sum() >= 8
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("dataset,dp,m", [("A", 1, 1), ("A", 1, 17), ("A", 1, 100), ("A", 1, 4096), ("A", 1, 7168),
                                          ("A", 1, 7169), ("A", 1, 10000), ("A", 1, 1000), ("A", 2, 1000), ("A", 3, 1000), ("A", 2, 100), ("A", 2, 7169), ("A", 3, 100),
                                          ("A", 3, 4096), ("A", 3, 7169), ("B", 1, 100), ("B", 1, 1000), ("B", 1, 7169), ("B", 2, 100),
                                          ("B", 2, 1000), ("B", 2, 7169), ("B", 3, 100), ("B", 3, 1000), ("B", 3, 7169)])
def test_crafted_waves_are_what_they_claim(dataset, dp, m):
    """Host decision of every wave's lane sets: off-grid lanes from the packed table header
    (kde_index_moments' rintf replay), |x'|^2 against 96 in kde_own's float32, all-underflow
    lanes by the largest a' - sigma < -149."""
    model = K.make_model(m, dp, dataset, "index")
    pk = _packed(model)
    tab = K.node_table(pk)
    assert (tab is not None) == (dataset == "A" and dp == 1)
    s_p, _ = K.scales(model.cpds[K.NODE])
    pp, _ = K.node_points(model)
    names = K.WAVES_A if dataset == "A" else K.WAVES_B
    par = K.case_parents(names, pp, s_p, K.SEED_PARENTS)      # the GPU cases' own lanes
    ls = K.lane_sets(pp, par, s_p, tab)
    for w, name in enumerate(names):
        _expect(name, ls, slice(w * K.WAVE, (w + 1) * K.WAVE), tab is not None)


def test_standard_normal_parent_data_gets_no_table():
    """With unit-variance parent data the table is declined from M = 4096 upward: the GPU cases
    must assert the presence ("kmt" in offs) they rely on."""
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(4096).astype(np.float32) * K.c_scale(0.5001)).astype(np.float32)
    assert P.kde_moment_table(y) is None


@pytest.mark.parametrize("m", [100, 4096, 7168, 7169, 10000])
def test_checker_discriminates(m):
    """Set A index model, random uniforms on the k 2^-24 grid: the reference's own index passes;
    the index one 32-point block further fails for every particle whose interval is not
    ambiguous; fewer than 10 % of the particles are ambiguous at the derived margin, with and
    without the moment table (shares printed)."""
    model = K.make_model(m, 1, "A", "index")
    tab = K.node_table(_packed(model))
    assert tab is not None
    s_p, _ = K.scales(model.cpds[K.NODE])
    pp, _ = K.node_points(model)
    n = 512
    par = K.case_parents(("W0",) * (n // K.WAVE), pp, s_p, 7)
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = np.random.default_rng(m).integers(0, 2 ** 24, n).astype(np.float64) * K.U24
    ref = K.ref_index(cdf, u)
    for label, t in (("table", tab), ("mfma", None)):
        mg = K.margin(pp, par, s_p, t)
        amb = K.n_acceptable(cdf, u, mg) > 1
        print(f"M={m} {label}: margin {mg.min():.3g} .. {mg.max():.3g}, ambiguous share {amb.mean():.4f}")
        assert amb.mean() < 0.10
        assert K.accept_index(cdf, u, ref, mg).all()
        shifted = (ref + 32) % m
        assert not K.accept_index(cdf, u, shifted, mg)[~amb].any()
        assert (K.miss(cdf, u, ref) == 0).all() and (K.miss(cdf, u, shifted)[~amb] > mg[~amb]).all()


def test_checker_rejects_dropped_sigma_correction():
    """A log-density off by |x'|^2 ln 2 (the factored form's correction left out) fails."""
    model = K.make_model(7169, 1, "A", "density")
    rec = model.cpds[K.NODE]
    pp, py = K.node_points(model)
    par = K.case_parents(("W0", "W2-"), pp, K.scales(rec)[0], 9)
    x = np.random.default_rng(1).standard_normal((len(par), 1)).astype(np.float32)
    ref = K.kde_logp64(pp, py, par, x, K.scales(rec))
    _, sq = K.own32(par, K.c_scale(K.scales(rec)[0]))
    off = sq.astype(np.float64) * math.log(2.0)
    big = off > 2 * K.LP_ATOL
    assert big.sum() > len(par) // 2
    assert K.logp_close(ref.astype(np.float32), ref).all()
    assert not K.logp_close(ref + off, ref)[big].any()
    bad = ref.copy()
    bad[0] = np.nan
    assert not K.logp_close(bad, ref)[0] and not K.logp_close(ref, bad)[0]


ALL_GPU_CASES = K.SAMPLING_CASES + K.JIT_CASES + K.VALU_CASES + K.LOGP_CASES


@pytest.mark.parametrize("dataset,dp,m,names,valu", ALL_GPU_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{len(c[3])}w{'-valu' if c[4] else ''}" for c in ALL_GPU_CASES])
def test_ambiguous_share_of_every_gpu_case(dataset, dp, m, names, valu):
    """Every case tests/test_gpu_kde_paths.py judges an index in, rebuilt from its seeds (parents,
    crafted and random uniforms) on the host: the share of random-uniform particles with more than
    one acceptable index at the derived margin is below 10 % -- per case, and for each of the W5
    waves on its own; printed per wave.  With and without the moment table where there is one."""
    model = K.make_model(m, dp, dataset, "density" if "FB" in names else "index")
    tab = K.node_table(_packed(model))
    par, cdf, u = K.case_inputs(model, names, tab)
    pp, _ = K.node_points(model)
    s_p, _ = K.scales(model.cpds[K.NODE])
    rnd = K.random_lanes(len(u))
    weak = (dataset, dp, m, names, valu) in K.LOGP_WEAK_INDEX
    for label, t in ((("table", tab), ("no table", None)) if tab is not None and not valu else (("", None),)):
        mg = K.margin(pp, par, s_p, t, valu=valu)
        amb = K.n_acceptable(cdf, u, mg) > 1
        per = {}
        for w, name in enumerate(names):
            sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
            per[name] = float(amb[sl][rnd[sl]].mean())
        share = float(amb[rnd].mean())
        print(f"{dataset} dp={dp} M={m} {label}: ambiguous share {share:.3f}; per wave "
              + ", ".join(f"{k} {v:.2f}" for k, v in per.items()) + f"; margin {mg.min():.2g} .. {mg.max():.2g}")
        if weak:
            assert share >= 0.10, "no longer weak: take the case out of LOGP_WEAK_INDEX"
            continue
        assert share < 0.10
        for name in ("W5-", "W5+"):
            assert per.get(name, 0.0) < 0.10, name
