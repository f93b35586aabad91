"""2-D moment tables of two-feature KDE nodes (plan.kde_moment_table2, csrc kde_index_moments2).

The kernel's sampling step of a two-feature node with a table evaluates, per row of the cell
nearest u = 2 x' (the MFMA pass's 16 chunks and, where that pass keeps half sums, the first half
of each), sum_{a+b<K} d0^a d1^b T[g][row][a,b] by nested Horner, then runs the MFMA path's own
chunk location, half choice and scan.  These CPU checks replay the kernel's float32 arithmetic
(cell choice, centre value, Horner order) and compare the row sums with float64 sums of the exact
weights exp2(u.y' - |y'|^2): relative error <= 4e-7 (the one-feature tables' bound,
tests/test_kde_moments.py); and the located index with the exact inverse-CDF index (differing
only at near-ties).
"""
import math

import numpy as np
import pytest
import torch

from vectorizedbayesiannetwork_amd import plan as P

CASES = [(10000, 0.36), (4096, 0.6), (100, 0.3), (17, 1.0), (1, 0.5)]
_tables = {}


def _data(m, sd):
    return (np.random.default_rng(m).standard_normal((m, 2)) * sd).astype(np.float32)


def _table_of(m, sd):
    """One table per case, built once and shared (read-only)."""
    if (m, sd) not in _tables:
        _tables[(m, sd)] = P.kde_moment_table2(_data(m, sd))
    return _tables[(m, sd)]


def header(tab):
    lo = (np.float32(tab[0]), np.float32(tab[4]))
    inv = (np.float32(tab[1]), np.float32(tab[5]))
    dl = (np.float32(tab[2]), np.float32(tab[6]))
    n = tuple(int(v) for v in tab[[3, 7]].view(np.int32))
    rows, rowf, k = (int(v) for v in tab[8:11].view(np.int32))
    return lo, inv, dl, n, rows, rowf, k


def kernel_cell(tab, u):
    """kde_index_moments2's cell choice in float32: (cell index, d0, d1), or None off the grid
    (or NaN)."""
    lo, inv, dl, n, _, _, _ = header(tab)
    g, d = [], []
    for f in range(2):
        uf = np.float32(u[f])
        with np.errstate(invalid="ignore"):
            gr = np.float32(np.rint(np.float32(np.float32(uf - lo[f]) * inv[f])))
        if not (0 <= gr < n[f]):
            return None
        ug = np.float32(np.float64(gr) * np.float64(dl[f]) + np.float64(lo[f]))     # fmaf(gr, dl, lo)
        g.append(int(gr))
        d.append(np.float64(np.float32(uf - ug)))
    return g[0] * n[1] + g[1], d[0], d[1]


def kernel_rows(tab, u):
    """The kernel's float32 sums of every row of u's cell (kde_mt2_row: one rounding per fmaf),
    or None outside the grid."""
    _, _, _, n, rows, rowf, k = header(tab)
    cell = kernel_cell(tab, u)
    if cell is None:
        return None
    c, d0, d1 = cell
    o = P.KDE_MT2_HEADER + c * rows * rowf
    t = tab[o:o + rows * rowf].reshape(rows, rowf).astype(np.float64)
    s = t[:, 0]
    i = 1
    for a in range(k - 2, -1, -1):
        p = t[:, i]
        i += 1
        for _ in range(k - 2 - a, -1, -1):
            p = (p * d1 + t[:, i]).astype(np.float32).astype(np.float64)
            i += 1
        s = (s * d0 + p).astype(np.float32).astype(np.float64)
    assert i == k * (k + 1) // 2
    return s


def exact_rows(y, u, m):
    """float64 sums of the exact weights over the table's rows (chunks, then first halves)."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    sq = (y64 ** 2).sum(axis=1).astype(np.float32).astype(np.float64)
    u64 = np.asarray(u, np.float32).astype(np.float64)
    w = np.exp2(y64 @ u64 - sq)
    per, half, halves = P.kde_moment2_geometry(m)
    ch = [w[c * per:(c + 1) * per].sum() for c in range(P.KDE_CHUNKS)]
    hf = [w[c * per:min(m, c * per + half)].sum() for c in range(P.KDE_CHUNKS)] if halves else []
    return np.array(ch + hf), w


def kernel_index(tab, y, u, ucat):
    """kde_index_mfma after a table pass 1, replayed: the chunk whose float64 running sum of the
    float32 chunk rows passes ucat * total, the half holding the rest (the chunk's half row), then
    the point inside it (exact float64 weights here: the kernel's float32 scan only moves
    near-ties)."""
    m = len(y)
    rows = kernel_rows(tab, u)
    per, half, halves = P.kde_moment2_geometry(m)
    thr = float(np.float32(ucat)) * float(rows[:P.KDE_CHUNKS].sum())
    cum, ch = 0.0, P.KDE_CHUNKS - 1
    for c in range(P.KDE_CHUNKS):
        if cum + rows[c] > thr:
            ch = c
            break
        cum += rows[c]
    j0, j1 = min(m, ch * per), min(m, (ch + 1) * per)
    rem = thr - cum
    if halves:
        pk = rows[P.KDE_CHUNKS + ch]
        if rem >= pk:
            j0, rem = min(m, j0 + half), rem - pk
        else:
            j1 = min(m, j0 + half)
    _, w = exact_rows(y, u, m)
    if j1 <= j0:
        return min(max(j0 - 1, 0), m - 1)
    k = int(np.searchsorted(np.cumsum(w[j0:j1]), rem, side="right"))
    return min(j0 + k, j1 - 1)


def _probe_points(tab, y, rng):
    """u across the grid: random, the grid's corners, cell corners, the origin, the data extremes."""
    lo, _, dl, n, _, _, _ = header(tab)
    hi = [float(lo[f]) + (n[f] - 1) * float(dl[f]) for f in range(2)]
    us = [rng.uniform([float(lo[0]), float(lo[1])], hi) for _ in range(120)]
    us += [(a, b) for a in (float(lo[0]), hi[0]) for b in (float(lo[1]), hi[1])]
    for _ in range(40):                                  # cell corners: half a cell from a centre
        g = [int(rng.integers(0, n[f] - 1)) for f in range(2)]
        us.append(tuple(float(lo[f]) + (g[f] + 0.5) * float(dl[f]) for f in range(2)))
    us.append((0.0, 0.0))
    for f in range(2):
        us += [tuple(2.0 * y[int(np.argmax(y[:, f]))]), tuple(2.0 * y[int(np.argmin(y[:, f]))])]
    us += [tuple(2.0 * y[int(j)]) for j in rng.integers(0, len(y), 20)]
    return us, hi


@pytest.mark.parametrize("m,sd", CASES)
def test_moment2_rows_match_exact(m, sd):
    """Every row (16 chunks, 16 first halves where kept) of the kernel's replay against float64
    sums of the exact weights, across the grid; the index located equals the exact inverse-CDF
    index except where the draw lies within 1e-6 of a point boundary (at most 2 per case)."""
    rng = np.random.default_rng([m, 2])
    y = _data(m, sd)
    tab = _table_of(m, sd)
    assert tab is not None
    lo, inv, dl, n, rows, rowf, k = header(tab)
    per, half, halves = P.kde_moment2_geometry(m)
    assert rows == P.KDE_CHUNKS * (2 if halves else 1) and halves == (P._kde_cb(m) // 2 >= P.KDE_HALF_MIN)
    assert k == P.KDE_MT2_K and rowf == P.KDE_MT2_ROW and rowf % 4 == 0 and rowf >= k * (k + 1) // 2
    assert tab.size == P.KDE_MT2_HEADER + n[0] * n[1] * rows * rowf
    us, hi = _probe_points(tab, y, rng)
    for f in range(2):                                   # the data range with margin on both sides
        w = min(P.KDE_MT2_MARGINS) - 0.1
        assert lo[f] <= 2 * (float(y[:, f].min()) - w) and hi[f] >= 2 * (float(y[:, f].max()) + w)
        assert math.log(2.0) * float(dl[f]) / 2 * float(np.abs(y[:, f]).max()) <= P.KDE_MT2_Z / 2 * (1 + 1e-6)
    worst, flips, seen = 0.0, 0, 0
    for u in us:
        got = kernel_rows(tab, u)
        if got is None:
            continue
        seen += 1
        ref, w = exact_rows(y, u, m)
        mask = ref > 0
        assert np.all(got[~mask] == 0)
        worst = max(worst, float(np.max(np.abs(got[mask] - ref[mask]) / ref[mask])))
        cdf = np.cumsum(w)
        for ucat in rng.uniform(0, 1, 5):
            idx = kernel_index(tab, y, u, ucat)
            thr = float(np.float32(ucat)) * cdf[-1]
            exact = min(int(np.searchsorted(cdf, thr, side="right")), m - 1)
            if idx != exact:
                margin = np.min(np.abs(cdf - thr)) / cdf[-1]
                assert margin < 1e-6, (u, ucat, idx, exact, margin)
                flips += 1
    print(f"M={m} sd={sd}: {seen} probes, worst relative row error {worst:.3g}, {flips} near-tie flips")
    assert seen >= 150
    assert worst <= 4e-7, worst
    assert flips <= 2
    # outside the grid (either feature) and NaN: the kernel takes the MFMA pass
    mid = (0.5 * (float(lo[0]) + hi[0]), 0.5 * (float(lo[1]) + hi[1]))
    assert kernel_rows(tab, (float(lo[0]) - 10 * float(dl[0]), mid[1])) is None
    assert kernel_rows(tab, (mid[0], hi[1] + 10 * float(dl[1]))) is None
    assert kernel_rows(tab, (float("nan"), mid[1])) is None and kernel_rows(tab, (mid[0], float("nan"))) is None


def test_moment2_coefficient_order():
    """The stored order is the nested Horner's: a from K - 1 down, inside it b from K - 1 - a down."""
    order = P.kde_moment2_order(4)
    assert order == [(3, 0), (2, 1), (2, 0), (1, 2), (1, 1), (1, 0), (0, 3), (0, 2), (0, 1), (0, 0)]
    assert len(P.kde_moment2_order()) == P.KDE_MT2_COEFS == 45 and P.KDE_MT2_ROW == 48


def test_moment2_series_bound():
    """Z bounds ln2 |d.y'| at a cell corner: the truncated series' relative error per weight."""
    z, k = P.KDE_MT2_Z, P.KDE_MT2_K
    assert z ** k / math.factorial(k) * math.exp(z) < 3e-8


def test_moment2_table_declines_wide_data():
    """Wide data: the table would exceed the size cap (or its weights the exponent range)."""
    y = (np.random.default_rng(0).standard_normal((2000, 2)) * 3.6).astype(np.float32)
    assert P.kde_moment_table2(y) is None
    # far from the origin and few cells: the cells' weights leave [2^-80, 2^100]
    y = (np.random.default_rng(1).standard_normal((100, 2)) * 0.02 + 6.0).astype(np.float32)
    (_, _, _, n0), (_, _, _, n1) = P.kde_moment2_cells(y)     # the widest margin fits
    assert n0 * n1 * P.KDE_CHUNKS * P.KDE_MT2_ROW * 4 <= P.KDE_MT2_MAX_BYTES
    assert P.kde_moment_table2(y) is None


def test_cfg4_two_feature_steps_carry_tables():
    """The packed cfg4 model (M = 10,000): every two-parent KDE node has a 2-D table (step
    off_w1 = its blob offset), every other step -1 there; off_kmt still holds the one-feature
    tables only; the rows match the exact sums at the node's own data points; x9 and x41 stay
    precomputed (per sample / per query) and keep their 17 floats."""
    import bench
    cfg, model, target, ev = bench.build_model("cfg4")
    pk = P.PackedModel(model, torch.device("cpu"))
    two = [n for n in model.topo if pk.nodes[n].kind == P.KIND_ID["kde"] and pk.nodes[n].aux0 == 2]
    assert two and len(two) == sum(1 for n in model.topo if len(model.parents[n]) == 2)
    for n in model.topo:
        assert ("kmt2" in pk.nodes[n].offs) == (n in two), n
        assert ("kmt" in pk.nodes[n].offs) == (pk.nodes[n].aux0 == 1 and len(model.parents[n]) == 1), n
    node = two[0]
    npk = pk.nodes[node]
    blob = pk.params.cpu().numpy()
    o = npk.offs["kmt2"]
    _, _, _, n, rows, rowf, _ = header(blob[o:o + P.KDE_MT2_HEADER])
    tab = blob[o:o + P.KDE_MT2_HEADER + n[0] * n[1] * rows * rowf]
    assert tab.size * 4 <= P.KDE_MT2_MAX_BYTES
    rec = model.cpds[node]
    c_p = np.float32(P._KDE_C / (max(float(rec.hparams["parent_bandwidth"]), 1e-3) + float(rec.hparams["min_scale"])))
    pts = rec.extra["parents"].float().numpy()
    y = (pts * c_p).astype(np.float32)
    for x in pts[:20]:
        u = np.float32(2.0) * (c_p * x.astype(np.float32))
        got, (ref, _) = kernel_rows(tab, u), exact_rows(y, u, len(y))
        assert np.max(np.abs(got - ref) / ref) <= 4e-7
    latent = [n for n in model.topo if n not in ev]
    plan = P.build_plan(pk, latent=latent, fixed=[n for n in model.topo if n in ev],
                        out_nodes=[target], logp=[target], skip=[], shared_roots=True, mode=P.MODE_MCM)
    name_of = {pk.node_id[n]: n for n in model.topo}
    for r in plan.steps._vbn_host[0]:
        n = name_of[int(r[P.S_NODEID])]
        assert r[P.S_KIND] == P.KIND_ID["kde"]           # cfg4 is a KDE DAG: every step
        assert r[P.S_OFF_KMT2] == (pk.nodes[n].offs["kmt2"] if n in two else -1), n
        assert r[P.S_OFF_KMT] == pk.nodes[n].offs.get("kmt", -1), n
    pc = P.precompute_plans(pk, plan)
    assert pc is not None
    pre = {name_of[int(r[P.S_NODEID])] for r in pc[0].steps._vbn_host[0] if r[P.S_FLAGS] & P.F_PRECOMP}
    assert {"x9", "x41"} <= pre
