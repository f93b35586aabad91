"""Float64 reference of the KDE step (reference kde.py:105-182) and the crafted-wave cases of
tests/test_kde_reference.py (CPU) and tests/test_gpu_kde_paths.py (GPU).  Host only: numpy
float64, nothing here touches a GPU.

* ``kde_index_cdf64`` / ``kde_logp64``: the sampling CDF and the log-density, from the float32
  inputs as they are (points, parents, bandwidth scale), every operation in float64.
* ``accept_index`` / ``n_acceptable`` / ``miss``: a chosen index passes iff the categorical
  uniform lies in its CDF interval widened by ``margin`` -- each particle judged on its own.
* ``margin``: the derived bound on the kernel's CDF error (docstring there).
* ``SAMPLING_CASES`` ..: the cases both test modules run; ``joint_sums``: the log-density sum replayed.
* ``make_model`` / ``wave`` / ``crafted_uniforms``: seeded models and 64-lane parent sets that
  put two of the step's per-wave / per-lane branches into one wave; ``lane_sets`` decides on the
  host, replaying the kernel's float32 arithmetic, which lanes are off the moment table's grid,
  beyond the factored form's limit, or all-underflow.
"""
import math

import numpy as np
import torch

from vectorizedbayesiannetwork_amd import plan as P

WAVE = 64
U24 = 2.0 ** -24                  # float32 unit roundoff
FFORM_MAX = np.float32(96.0)      # csrc KDE_FFORM_MAX
HALF_MIN = 16                     # csrc KDE_HALF_MIN: 32-point blocks per chunk for half sums
UNDERFLOW = -149.0                # exp2 below the smallest float32 denormal
LP_ATOL = 1e-4                    # the project's log-density tolerance (tests/test_gpu_parity.py)
TABLE_ROW_BOUND = 4e-7            # tests/test_kde_moments.py: relative error of every table row


# ---- the reference -------------------------------------------------------------------------

def scales(rec):
    """(parent scale, target scale) = max(bandwidth, 1e-3) + min_scale (kde.py:106)."""
    bw = float(rec.hp("bandwidth"))
    pbw = rec.hp("parent_bandwidth")
    pbw = bw if pbw is None else float(pbw)
    ms = float(rec.hp("min_scale"))
    return max(pbw, 1e-3) + ms, max(bw, 1e-3) + ms


def _f64(a, cols=None):
    a = np.asarray(a, np.float32).astype(np.float64)
    return a.reshape(a.shape[0], -1) if cols is None else a.reshape(-1, cols)


def _sqdist(x, y, s):
    q = np.zeros((x.shape[0], y.shape[0]))
    for k in range(x.shape[1]):
        d = (x[:, None, k] - y[None, :, k]) / s
        q += d * d
    return q


def kde_index_cdf64(points_p, parents, bw_scale):
    """CDF over the points of softmax_j(log K_p) (kde.py:172-178) per particle, [n, M] float64,
    normalised to end at 1."""
    y = _f64(points_p)
    x = _f64(parents, y.shape[1])
    logk = -0.5 * _sqdist(x, y, float(bw_scale))
    w = np.exp(logk - logk.max(axis=1, keepdims=True))
    cdf = np.cumsum(w, axis=1)
    return cdf / cdf[:, -1:]


def _lse(a):
    m = a.max(axis=1)
    return m + np.log(np.exp(a - m[:, None]).sum(axis=1))


def kde_logp64(points_p, points_y, parents, x, scales_):
    """log p(x | parents) of kde.py:114-146 with a float64 log-sum-exp: root (no parent
    features) LSE_j log K_y - log M, otherwise LSE_j (log K_p + log K_y) - LSE_j log K_p."""
    s_p, s_y = (float(v) for v in scales_)
    ty = _f64(points_y)
    xx = _f64(x, ty.shape[1])
    logky = -0.5 * _sqdist(xx, ty, s_y) - 0.5 * ty.shape[1] * (math.log(2 * math.pi) + 2 * math.log(s_y))
    yp = np.asarray(points_p, np.float32)
    dp = 0 if yp.ndim < 2 else yp.shape[1]
    if dp == 0:
        return _lse(logky) - math.log(ty.shape[0])
    y = _f64(yp)
    logkp = -0.5 * _sqdist(_f64(parents, dp), y, s_p)      # the constant cancels in the ratio
    return _lse(logkp + logky) - _lse(logkp)


def ref_index(cdf, u):
    """The float64 inverse-CDF choice: the first index whose CDF exceeds u."""
    u = np.asarray(u, np.float64)
    return np.minimum((cdf <= u[:, None]).sum(axis=1), cdf.shape[1] - 1)


def _interval(cdf, idx):
    r = np.arange(cdf.shape[0])
    idx = np.asarray(idx, np.int64)
    lo = np.where(idx > 0, cdf[r, np.maximum(idx - 1, 0)], 0.0)
    return lo, cdf[r, idx]


def miss(cdf, u, idx):
    """How far u lies outside the chosen index's CDF interval (0 inside)."""
    lo, hi = _interval(cdf, idx)
    u = np.asarray(u, np.float64)
    return np.maximum(np.maximum(lo - u, u - hi), 0.0)


def accept_index(cdf, u, idx, margin_):
    """idx passes iff cdf[idx-1] - margin <= u <= cdf[idx] + margin (cdf[-1] := 0)."""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < cdf.shape[1])
    lo, hi = _interval(cdf, np.clip(idx, 0, cdf.shape[1] - 1))
    u = np.asarray(u, np.float64)
    return ok & (lo - margin_ <= u) & (u <= hi + margin_)


def n_acceptable(cdf, u, margin_):
    """Number of indices that pass accept_index, per particle."""
    lo = np.concatenate([np.zeros((cdf.shape[0], 1)), cdf[:, :-1]], axis=1)
    u = np.asarray(u, np.float64)[:, None]
    m = np.broadcast_to(np.asarray(margin_, np.float64), (cdf.shape[0],))[:, None]
    return ((lo - m <= u) & (u <= cdf + m)).sum(axis=1)


def logp_close(got, ref, atol=LP_ATOL):
    """Per particle: identical NaN / +-inf pattern and |got - ref| <= atol where finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    same = (np.isnan(got) == np.isnan(ref)) & (np.isposinf(got) == np.isposinf(ref)) \
        & (np.isneginf(got) == np.isneginf(ref))
    with np.errstate(invalid="ignore"):
        return same & (~fin | (np.abs(got - ref) <= atol))


# ---- the kernel's float32 operands (csrc kde_own, plan._pack_node) ---------------------------

def c_scale(s):
    return np.float32(P._KDE_C / float(s))


def own32(parents, c):
    """kde_own: x'_k = c x_k and |x'|^2 accumulated by fmaf, float32."""
    x = np.asarray(parents, np.float32)
    x = x.reshape(x.shape[0], -1)
    xv = (np.float32(c) * x).astype(np.float32)
    sq = np.zeros(x.shape[0], np.float32)
    for f in range(x.shape[1]):
        v = xv[:, f].astype(np.float64)
        sq = (v * v + sq.astype(np.float64)).astype(np.float32)
    return xv, sq


def points32(points_p, c):
    """The packed points: y' = c y (float32) and |y'|^2 (float64 sum, one rounding)."""
    y = np.asarray(points_p, np.float32)
    yp = (y.reshape(y.shape[0], -1) * np.float32(c)).astype(np.float32)
    return yp, (yp.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)


def wave_any(flag):
    """A per-lane flag -> per lane, whether any lane of its wave (64 consecutive) has it."""
    flag = np.asarray(flag, bool)
    out = np.zeros_like(flag)
    for b in range(0, flag.size, WAVE):
        out[b:b + WAVE] = flag[b:b + WAVE].any()
    return out


def table_header(tab):
    lo, inv, dl = np.float32(tab[0]), np.float32(tab[1]), np.float32(tab[2])
    n, nch, per = (int(v) for v in np.asarray(tab[3:6], np.float32).view(np.int32))
    return lo, inv, dl, n, nch, per


def off_grid(tab, xv0):
    """kde_index_moments' cell choice replayed in float32: gr = rintf((2 x' - u_lo) inv_d), off
    the grid unless 0 <= gr < n_cells (as tests/test_kde_moments._kernel_rows)."""
    lo, inv, _, n, _, _ = table_header(tab)
    u = (np.float32(2.0) * np.asarray(xv0, np.float32)).astype(np.float32)
    gr = np.rint(((u - lo).astype(np.float32) * inv).astype(np.float32))
    return ~((gr >= 0) & (gr < n))


def lane_sets(points_p, parents, bw_scale, tab=None):
    """Per lane, decided on the host: ``over`` (|x'|^2 > 96 in kde_own's float32), ``full`` (its
    wave runs the full form), ``off`` (off the moment table's grid; all False without a table),
    ``table`` (its wave takes the table pass), ``under`` (every weight underflows: the largest
    a' - sigma is below -149, sigma = |x'|^2 in the full form, 0 in the factored one),
    ``rescued`` (pass 1's sum, replayed with every weight below 2^-126 flushed to 0 as
    v_exp_f32 does, is below csrc kde_tiny(M) = M 2^-109: the rescue runs), ``ratio`` (that sum
    over kde_tiny(M); a lane within a factor 1.01 of 1 is not decided by a float64 replay) and
    ``lost`` (the flushed share of the exact sum)."""
    c = c_scale(bw_scale)
    xv, sq = own32(parents, c)
    yp, ysq = points32(points_p, c)
    over = sq > FFORM_MAX
    full = wave_any(over)
    off = off_grid(tab, xv[:, 0]) if tab is not None else np.zeros(len(sq), bool)
    table = (np.zeros(len(sq), bool) if tab is None else ~wave_any(off | over))
    a = 2.0 * xv.astype(np.float64) @ yp.astype(np.float64).T - ysq.astype(np.float64)[None, :]
    a -= np.where(full, sq.astype(np.float64), 0.0)[:, None]
    amax = a.max(axis=1)
    w = np.exp2(np.maximum(a, -1000.0))
    kept = np.where(a >= -126.0, w, 0.0).sum(axis=1)
    tot = w.sum(axis=1)
    tiny = yp.shape[0] * 2.0 ** -109
    lost = np.where(tot > 0, 1.0 - kept / np.where(tot > 0, tot, 1.0), 1.0)
    return dict(over=over, full=full, off=off, table=table, under=amax < UNDERFLOW, sq=sq, amax=amax, m=yp.shape[0],
                rescued=(kept < tiny) & ~table, ratio=kept / tiny, lost=lost)


def joint_sums(points_p, points_y, parents, x, scales_):
    """kde_logp_mfma's numerator sum sy in the full form, exp2(-|x' - y'_j|^2) over parent and
    target features, replayed in float64 at the float32 operands: ``amax`` (largest exponent),
    ``kept`` (the sum without the weights below 2^-126, which v_exp_f32 gives as 0), ``lost``
    (their share of the exact sum) and ``fallback`` (kept < csrc kde_tiny(M) = M 2^-109: the lane
    must take the shifted path)."""
    s_p, s_y = scales_
    ty, tsq = points32(points_y, c_scale(s_y))
    xv, _ = own32(np.asarray(x, np.float32).reshape(-1, 1), c_scale(s_y))
    a = -((xv.astype(np.float64) - ty.astype(np.float64).T) ** 2)
    yp = np.asarray(points_p, np.float32)
    if yp.ndim == 2 and yp.shape[1]:
        pv, _ = own32(parents, c_scale(s_p))
        pq, _ = points32(yp, c_scale(s_p))
        for k in range(yp.shape[1]):
            a -= (pv[:, None, k].astype(np.float64) - pq[None, :, k].astype(np.float64)) ** 2
    w = np.exp2(np.maximum(a, -1000.0))
    kept = np.where(a >= -126.0, w, 0.0).sum(axis=1)
    tot = w.sum(axis=1)
    lost = np.where(tot > 0, 1.0 - kept / np.where(tot > 0, tot, 1.0), 1.0)
    return dict(amax=a.max(axis=1), kept=kept, lost=lost, fallback=kept < ty.shape[0] * 2.0 ** -109)


# ---- the derived margin ----------------------------------------------------------------------

def margin(points_p, parents, bw_scale, tab=None, valu=False):
    """Per-particle bound on |kernel CDF - float64 CDF| relative to the total mass, derived from
    the stated error of each stage of the sampling step -- not fitted to any GPU output.

    The kernel's weight of point j is exp2(a'_j - sigma), a' = u.y' - |y'|^2 with u = 2x',
    x' = c x, y' = c y, c = float32(sqrt(log2(e)/2) / scale); sigma is common to a particle, and
    so is every error that multiplies all of a particle's weights by one factor: it cancels in
    the normalised CDF.  p_j is point j's share of the mass, d_j = |x' - y'_j|.

    1. *Operands.*  c, x' and y'_j each carry a relative rounding of 2^-24 against the float64
       reference (y'_j two: c and its own).  The stored |y'|^2 is formed from the rounded y', so
       the kernel's exact argument is a'(x~', y~'_j) = |x~'|^2 - |x~' - y~'_j|^2.  Moving y'_j by
       delta changes it by 2 (x' - y'_j) . delta <= 2 d_j |y'_j| 2 2^-24; moving x' by delta
       changes it by 2 y'_j . delta = 2 x' . delta (common to the particle) + 2 (y'_j - x') . delta
       <= common + 2 d_j |x'| 2 2^-24.  Together 4 d_j (|x'| + |y'_j|) 2^-24.
    2. *Arithmetic of a'.*  The stored |y'_j|^2 rounds once (2^-24 Q_j, Q_j = |y'_j|^2); the
       chain of nf + 1 FMAs (kde_arg_rec, the scan's lambdas; sigma enters as an addend) rounds
       each at most 2^-24 A_j, A_j = max(P_j, Q_j, |sigma|), P_j = sum_k |u_k y'_jk|; the bf16x3
       MFMA contraction equals the chain to float32 rounding (tests/test_plan.py) and drops
       products below 2^-25 of u y', three per feature: 2^-24 P_j.  So
       delta a'_j <= 2^-24 [4 d_j (|x'| + |y'_j|) + (nf + 1) A_j + Q_j + P_j].
       The VALU form -(x' - y')^2 (kde_arg_valu) has the same operand term, one rounding per
       difference and nf for the squares and FMAs: 2^-24 [4 d_j (|x'| + |y'_j|) + (nf + 2) d_j^2].
       Relative weight error eps_j = ln2 delta a'_j.
    3. *v_exp_f32*: 1 ulp, eps_e = 2^-23 relative.
    4. *From weights to the CDF.*  Relative weight errors |e_j| <= eps_j move the normalised CDF
       at index k by at most (1 - F_k) S_k + F_k (E - S_k), S_k = sum_{j <= k} p_j eps_j,
       E = S_M (worst case: + below the threshold, - above); the bound W is its maximum over k.
       For a uniform eps this is 2 eps F (1 - F) <= eps / 2; the same holds for the relative
       errors gamma of the chunk sums.
    5. *Chunk sums.*  MFMA pass: an accumulator takes 4 exps per 32-point block in sequence, then
       the 4 accumulators and the two half-tiles are added: gamma = (4 blocks + 3) 2^-24.  The
       rescue's sums are sequential, gamma = (chunk points) 2^-24; the VALU pass's two packed
       accumulators take chunk points / 2 each: (chunk points / 2 + 1) 2^-24, its rescue again
       (chunk points) 2^-24.  A particle whose replayed sum is within a factor 2 of kde_tiny(M)
       gets the larger of its two gammas.  The chunk sums are added in float64.
    6. *Flushed weights.*  v_exp_f32 gives 0 below 2^-126.  A particle that is not rescued has
       a sum >= M 2^-109 (csrc kde_tiny) and has lost at most M 2^-126 of it: its CDF moves by at
       most the lost share, lost <= 2^-17, taken from the replay (lane_sets) -- 0 for particles
       whose smallest relevant weights are far above 2^-126, all of it one-sided.
    7. *Moment table wave*: the rows (chunk, group, total) are each within 4e-7 of the exact
       float32-operand sums (tests/test_kde_moments.py) but not consistent with each other, so
       they count in full, twice (threshold and running sum): 2 x 4e-7 instead of gamma / 2.
    8. *Inside the chunk*: the scan walks from the nearer end of its range r (the chunk, or the
       half chunk where pass 1 keeps half sums), so its running float32 sum takes at most r / 2
       adds; with the mismatch between the chunk / half sum and the scan's own sum (gamma, eps_e),
       the float32 roundings of rem and csum (2 x 2^-24) this acts on the chunk's mass only,
       phi = the largest chunk's share of the mass; the weights' own errors inside a chunk are at
       most C = max over chunks of sum_{j in chunk} p_j eps_j.

       margin = W + (eps_e + gamma) / 2 + lost + C + phi (eps_e + gamma + (r / 2 + 2) 2^-24)
       table:   W +  eps_e / 2 + 8e-7          + C + phi (eps_e + 4e-7  + (r / 2 + 2) 2^-24)
    """
    c = c_scale(bw_scale)
    xv, sq = own32(parents, c)
    yp, ysq = points32(points_p, c)
    m, nf = yp.shape
    ls = lane_sets(points_p, parents, bw_scale, tab)
    x64, y64, q = xv.astype(np.float64), yp.astype(np.float64), ysq.astype(np.float64)
    x2 = sq.astype(np.float64)
    d2 = np.zeros((len(sq), m))
    pj = np.zeros((len(sq), m))
    for k in range(nf):
        d2 += (x64[:, None, k] - y64[None, :, k]) ** 2
        pj += np.abs(2.0 * x64[:, None, k] * y64[None, :, k])
    dj = np.sqrt(d2)
    operand = 4.0 * dj * (np.sqrt(x2)[:, None] + np.sqrt(q)[None, :])
    near = (ls["ratio"] < 2.0) & ~ls["table"]                 # the rescue runs, or may run
    if valu:
        da = operand + (nf + 2) * d2
    else:
        a_raw_max = ls["amax"] + np.where(ls["full"], x2, 0.0)
        sigma = np.maximum(np.where(ls["full"], x2, 0.0), np.where(near, np.abs(a_raw_max), 0.0))
        aj = np.maximum(np.maximum(pj, q[None, :]), sigma[:, None])
        da = operand + (nf + 1) * aj + q[None, :] + pj
    eps_j = math.log(2.0) * U24 * da
    eps_e = 2.0 ** -23
    cdf = kde_index_cdf64(points_p, parents, bw_scale)
    pe = np.diff(np.concatenate([np.zeros((cdf.shape[0], 1)), cdf], axis=1), axis=1) * eps_j
    s_k = np.cumsum(pe, axis=1)
    e_tot = s_k[:, -1:]
    w_term = ((1.0 - cdf) * s_k + cdf * (e_tot - s_k)).max(axis=1)
    cb = P._kde_cb(m)
    if valu:
        pts = ((m + P.KDE_CHUNKS - 1) // P.KDE_CHUNKS + 7) & ~7
        rng_pts = pts
        gamma = np.where(near, pts * U24, (pts // 2 + 1) * U24)
    else:
        pts = 16 * cb
        rng_pts = pts // 2 if chunk_points(m)[1] else pts
        gamma = np.where(near, pts * U24, (4 * (cb // 2) + 3) * U24)
    lost = np.where(ls["rescued"] & (ls["ratio"] < 0.5), 0.0, np.minimum(ls["lost"], 2.0 ** -17))

    def per_chunk(per):
        z = np.zeros((cdf.shape[0], 1))
        ends = np.unique(np.concatenate([np.arange(per - 1, m, per), [m - 1]]))
        phi = np.diff(np.concatenate([z, cdf[:, ends]], axis=1), axis=1).max(axis=1)
        inside = np.diff(np.concatenate([z, s_k[:, ends]], axis=1), axis=1).max(axis=1)
        return phi, inside
    phi, inside = per_chunk(pts)
    out = w_term + 0.5 * (eps_e + gamma) + lost + inside + phi * (eps_e + gamma + (rng_pts // 2 + 2) * U24)
    if tab is not None and not valu:
        per = table_header(tab)[5]
        phi, inside = per_chunk(per)
        t = w_term + 0.5 * eps_e + 2 * TABLE_ROW_BOUND + inside + phi * (eps_e + TABLE_ROW_BOUND + (per // 2 + 2) * U24)
        out = np.where(ls["table"], t, out)
    return out


# ---- case builders -----------------------------------------------------------------------------

NODE = "k"
DATA_SD = 0.21


def make_model(m, dp, dataset, kind, seed=0):
    """A (dp + 1)-node model: linear_gaussian parents p0.. -> KDE node ``k`` of m points (point
    order kept: m <= max_points).  dataset "A": parent points N(0, 0.21^2) (with the default
    parent bandwidth 0.5 a scaled sd of ~0.36: one-parent nodes get a moment table); "B":
    N(5 / sqrt(dp), 0.21^2) per feature (|x'|^2 ~ 72 on the data, up to ~90: no table).  kind
    "index": targets arange(m) (with zero normals the sample is the chosen index); "density":
    targets N(0, 1)."""
    import networkx as nx
    from vectorizedbayesiannetwork_amd.model import random_init_model
    rng = np.random.default_rng([m, dp, ord(dataset), seed])
    mu = 0.0 if dataset == "A" else 5.0 / math.sqrt(max(dp, 1))
    g = nx.DiGraph()
    g.add_node(NODE)
    data, kinds = {}, {NODE: "kde"}
    for i in range(dp):
        g.add_edge(f"p{i}", NODE)
        kinds[f"p{i}"] = "linear_gaussian"
        data[f"p{i}"] = torch.from_numpy((mu + DATA_SD * rng.standard_normal((m, 1))).astype(np.float32))
    if kind == "index":
        data[NODE] = torch.arange(m, dtype=torch.float32)[:, None]
    else:
        data[NODE] = torch.from_numpy(rng.standard_normal((m, 1)).astype(np.float32))
    return random_init_model(g, kinds, data, seed=1, overrides={"kde": {"max_points": max(m, 4096)}})


def node_points(model):
    rec = model.cpds[NODE]
    return rec.extra["parents"].float().numpy(), rec.extra["targets"].float().numpy()


def node_table(pk):
    """The packed moment table of the KDE node (header + rows), or None."""
    npk = pk.nodes[NODE]
    if "kmt" not in npk.offs:
        return None
    blob = pk.params.cpu().numpy()
    o = npk.offs["kmt"]
    n, nch, _ = (int(v) for v in blob[o + 3:o + 6].view(np.int32))
    return blob[o:o + P.KDE_MT_HEADER + n * P.kde_moment_rows(nch) * P.KDE_MT_TERMS].copy()


WAVES_A = ("W0", "W1", "W2-", "W2+", "W3", "W6")
WAVES_B = ("W0", "W4", "W5-", "W5+", "W6")
SEED_PARENTS, SEED_U = 11, 12
N_CRAFTED = 7                     # lanes 0-6 of every wave carry crafted uniforms (crafted_uniforms)

# The cases tests/test_gpu_kde_paths.py runs: (data set, parent features, M, waves, kde_valu).
# Set A keeps the sizes up to 7169 (the smallest M with half chunks).  Set B's terms of a' are
# ~150, so its derived margin is 1.3e-5 .. 2.4e-5 whatever M is: at M = 7169 a point holds less
# mass than that and 18-26 % of the random-uniform particles have two acceptable indices; its
# large size is therefore 1000 (16 chunks of 64 points, the last one partial; below 10 %).
# M = 10000 (one feature, set A) meets the condition too: margin 3.5e-6 .. 3.8e-6, share 7 %.
SAMPLING_CASES = ([("A", 1, m, WAVES_A, False) for m in (1, 17, 100, 4096, 7168, 7169, 10000)]
                  + [("A", dp, m, WAVES_A, False) for dp in (2, 3) for m in (100, 4096, 7169)]
                  + [("B", dp, m, WAVES_B, False) for dp in (1, 2, 3) for m in (100, 1000)])
JIT_CASES = [("A", dp, 100, WAVES_A, False) for dp in (1, 2, 3)]
VALU_CASES = [("A", dp, 1000, ("W0", "W3"), True) for dp in (1, 2, 3)]
LOGP_WAVES_A = ("W0", "W2-", "W2+", "W3", "W6", "NB", "FB")
LOGP_WAVES_B = ("W0", "W5-", "W5+", "W6", "NB", "FB")
# the log-density cases keep set B at the issue's M = 7169 as well: the log-density is judged at
# the value the kernel returned, whichever acceptable index it chose; the index check there is
# the weak one described above (LOGP_WEAK_INDEX: share printed, not asserted)
LOGP_CASES = ([("A", dp, m, LOGP_WAVES_A, False) for dp in (1, 2, 3) for m in (100, 7169)]
              + [("B", dp, m, LOGP_WAVES_B, False) for dp in (1, 2, 3) for m in (100, 1000, 7169)])
LOGP_ROOT_CASES = [("A", 0, m, ("W0", "NB", "FB"), False) for m in (100, 7169)]
LOGP_WEAK_INDEX = [c for c in LOGP_CASES if c[0] == "B" and c[2] == 7169]


def parent_waves(names):
    """NB and FB (log-density waves: far target values on odd lanes) have W0's parents."""
    return tuple("W0" if n in ("NB", "FB") else n for n in names)


def case_inputs(model, names, tab=None):
    """(parents [S, dp], float64 CDF [S, M], uniforms [S]) of a GPU case, from its seeds."""
    pp, _ = node_points(model)
    s_p, _ = scales(model.cpds[NODE])
    par = case_parents(parent_waves(names), pp, s_p, SEED_PARENTS)
    cdf = kde_index_cdf64(pp, par, s_p)
    return par, cdf, crafted_uniforms(cdf, pp.shape[0], SEED_U, tab)


def random_lanes(n):
    """Mask of the lanes that carry random uniforms (not the crafted lanes 0-6 of each wave)."""
    return (np.arange(n) % WAVE) >= N_CRAFTED
LANE_OFF, LANE_EDGE, LANE_B = 37, 21, 9
R96 = math.sqrt(96.0)


def wave(name, points_p, bw_scale, rng):
    """64 lanes of parent values [64, dp] float32 of one crafted wave (module docstring of
    tests/test_gpu_kde_paths.py)."""
    y = np.asarray(points_p, np.float64)
    dp = y.shape[1]
    c = float(c_scale(bw_scale))
    mean = y.mean(axis=0)
    x = mean[None, :] + DATA_SD * rng.standard_normal((WAVE, dp))
    if name == "W0":
        pass
    elif name == "W1":                       # one lane off the table's grid, |x'|^2 = 36
        x[LANE_OFF, 0] = 6.0 / c
    elif name in ("W2-", "W2+"):             # one lane just inside / outside the factored form
        x[LANE_EDGE] = 0.0
        x[LANE_EDGE, 0] = R96 * (1.0 - 1e-3 if name == "W2-" else 1.0 + 1e-3) / c
    elif name == "W3":                       # odd lanes >= 13 scaled units beyond the data
        x[1::2, 0] = y[:, 0].max() + (13.0 + rng.uniform(0.0, 1.0, WAVE // 2)) / c
    elif name == "W4":                       # x' ~ -9.5 on the data's axis: factored, all underflow
        x = (-9.5 / math.sqrt(dp) + 0.1 * rng.uniform(-1.0, 1.0, (WAVE, dp))) / c
    elif name in ("W5-", "W5+"):             # widened around the data: |x'|^2 on both sides of 96
        x = mean[None, :] + 0.45 * rng.standard_normal((WAVE, dp))
        unit = mean / np.linalg.norm(mean)
        if name == "W5-":
            r = np.linalg.norm(x, axis=1) * c
            x *= np.minimum(1.0, R96 * (1.0 - 1e-4) / r)[:, None]
            x[LANE_B] = unit * R96 * (1.0 - 2e-4) / c
        else:
            x[LANE_B] = unit * R96 * (1.0 + 2e-4) / c
    elif name == "W6":                       # the largest a' - sigma graded across the underflow limit
        if np.linalg.norm(mean) * c > 4.0:   # set B: factored, x' = -r along the data's axis
            x = -(mean / np.linalg.norm(mean))[None, :] * rng.uniform(3.0, 7.6, (WAVE, 1)) / c
        else:                                # set A: full form, 10 .. 12.7 scaled units beyond the data
            x[:, 0] = y[:, 0].max() + rng.uniform(10.0, 12.7, WAVE) / c
    else:
        raise ValueError(name)
    return x.astype(np.float32)


def case_parents(names, points_p, bw_scale, seed):
    rng = np.random.default_rng([seed, len(names)])
    return np.concatenate([wave(n, points_p, bw_scale, rng) for n in names], axis=0)


def chunk_points(m, tab=None, valu=False):
    """(points per inverse-CDF chunk, points before the half-chunk boundary or 0)."""
    if tab is not None:
        return table_header(tab)[5], 0
    if valu:
        return ((m + P.KDE_CHUNKS - 1) // P.KDE_CHUNKS + 7) & ~7, 0
    cb = P._kde_cb(m)
    cb32 = cb // 2
    return 16 * cb, (32 * ((cb32 // 2) & ~1) if cb32 >= HALF_MIN else 0)


def crafted_uniforms(cdf, m, seed, tab=None):
    """[S] float32 categorical uniforms: lanes 0-6 of every wave hold 0, 2^-24, 0.5, 1 - 2^-24
    and the float32 nearest the lane's own float64 CDF at the end of the first chunk, at a
    half-chunk boundary (second chunk; only where chunks have half sums) and at the start of the
    last chunk (MFMA chunks, and the table's finer chunks where the wave may take the table);
    every other lane a seeded random multiple of 2^-24."""
    s = cdf.shape[0]
    rng = np.random.default_rng([seed, s, m])
    u = (rng.integers(0, 2 ** 24, s).astype(np.float64) * U24)
    top = 1.0 - U24
    for b in range(0, s, WAVE):
        u[b:b + 4] = [0.0, U24, 0.5, top]
        pts, half = chunk_points(m, tab if (tab is not None and (b // WAVE) % 2 == 0) else None)
        u[b + 4] = cdf[b + 4, min(m, pts) - 1]
        if half and pts + half <= m:
            u[b + 5] = cdf[b + 5, pts + half - 1]
        j0 = pts * ((m - 1) // pts)
        if j0 > 0:
            u[b + 6] = cdf[b + 6, j0 - 1]
    return np.minimum(u.astype(np.float32), np.float32(top)).astype(np.float32)
