"""The 2-D moment-table pass 1 of two-feature KDE nodes (csrc kde_index_moments2) on the GPU,
against the float64 reference of tests/kde_reference.py.

Single-node walks as in tests/test_gpu_kde_paths.py: B = 1, S = 64 x waves <= 512, per-particle
parents, injected draws.  Set A, two parent features, M = 100, 4096 and 7169 (7169: the smallest M
whose chunks have half rows).  A wave is 64 consecutive particles:

| wave | parents | pass 1 |
|---|---|---|
| W0  | on the data | the table |
| W1  | W0, lane 37's second feature 3/4 of a cell beyond the grid's last centre | MFMA for the whole wave |
| W2+ | W0, lane 21 at |x'| = sqrt(96) (1 + 1e-3) | MFMA, full form, for the whole wave |

(the host replays the kernel's float32 cell choice and asserts these lane sets).  Lanes 0-6 of
every wave carry the harness's crafted uniforms (0, 2^-24, 0.5, 1 - 2^-24, a chunk end, a
half-chunk boundary, the start of the last chunk), the others seeded multiples of 2^-24.

Margin of a table wave.  Everything after pass 1 is the MFMA path's code on the MFMA path's chunk
geometry, so its errors are those of ``kde_reference.margin`` without a table (operands, the scan's
chain and exps, the float32 roundings of rem and csum; its chunk-sum term gamma is kept although
the table's rows carry no accumulation error).  The table adds the error of the rows it supplies,
each within ROW = 4e-7 of the exact float32-operand sum (tests/test_kde_moments2.py), relative to
the total mass:
  * the threshold u * total: the total is the sum of the 16 chunk rows, ROW of the whole mass,
    scaled by u: ROW u;
  * the running sum cum: the chunk rows before the located chunk, whose exact mass is at most
    min(1, u + phi) (phi = the largest chunk's share: the located chunk starts below the
    threshold, up to a neighbouring chunk at a near-tie): ROW min(1, u + phi);
  * the located chunk's own row (csum) and its first-half row: ROW phi each.
  margin_table = margin_mfma + ROW (u + min(1, u + phi) + 2 phi)   <= margin_mfma + 1.6e-6.

Path identity: the same model packed with ``KDE_MOMENTS2`` off must give bit-identical W1 and
W2+ (one off-grid or over-limit lane takes the whole wave off the table).  That W0 does read the
table is shown by overwriting it: with the chunk rows 1-15 of every cell zeroed in the packed blob
the table's total is chunk 0's sum, so every W0 particle must land in chunk 0 (it did not before),
while W1 and W2+ stay bit-identical.  ``plan_jit=2`` equals
the interpreter bit for bit.  Log-density (sample and score in one step): ``lsp`` comes from the
table's total; against ``kde_logp64`` at the returned value, 1e-4 absolute, identical NaN / inf
pattern.  Set B (terms of ~150): the builder declines, no ``kmt2``.
"""
import numpy as np
import pytest
import torch

import kde_reference as K
from test_gpu_kde_paths import _case, _indices, _judge, _launch, _pk, _sampled_miss, _vbn

pytestmark = pytest.mark.gpu

ROW = K.TABLE_ROW_BOUND            # 4e-7: tests/test_kde_moments2.py asserts it for every row
WAVES = ("W0", "W1", "W2+")
LANE_OFF = K.LANE_OFF
SIZES = (100, 4096, 7169)


def _table2(pk):
    """Header fields of the node's 2-D table: per feature (u_lo, 1 / delta, delta, n_cells)."""
    from vectorizedbayesiannetwork_amd import plan as P
    o = pk.nodes[K.NODE].offs["kmt2"]
    h = pk.params[o:o + P.KDE_MT2_HEADER].cpu().numpy()
    n = h[[3, 7]].view(np.int32)
    return [(np.float32(h[4 * f]), np.float32(h[4 * f + 1]), np.float32(h[4 * f + 2]), int(n[f])) for f in range(2)]


def _off_grid(tab2, xv):
    """kde_index_moments2's cell choice replayed in float32, per lane: off the grid in a feature."""
    off = np.zeros(len(xv), bool)
    for f, (lo, inv, _, n) in enumerate(tab2):
        u = (np.float32(2.0) * xv[:, f]).astype(np.float32)
        gr = np.rint(((u - lo).astype(np.float32) * inv).astype(np.float32))
        off |= ~((gr >= 0) & (gr < n))
    return off


def _parents(pp, s_p, tab2):
    """[192, 2] parents of W0, W1, W2+ and, per lane, whether its wave takes the table (host
    replay: every lane on the grid and within the factored form's limit)."""
    rng = np.random.default_rng([K.SEED_PARENTS, 2, len(pp)])
    c = K.c_scale(s_p)
    w0 = K.wave("W0", pp, s_p, rng)
    w1 = w0.copy()
    lo, _, dl, n = tab2[1]
    u_off = float(lo) + (n - 1 + 0.75) * float(dl)          # rintf -> n: the first value off the grid
    w1[LANE_OFF, 1] = np.float32(u_off / (2.0 * float(c)))
    w2 = w0.copy()
    w2[K.LANE_EDGE] = 0.0
    w2[K.LANE_EDGE, 0] = K.R96 * (1.0 + 1e-3) / float(c)
    par = np.concatenate([w0, w1, w2]).astype(np.float32)
    xv, sq = K.own32(par, c)
    off, over = _off_grid(tab2, xv), sq > K.FFORM_MAX
    assert not off[:K.WAVE].any() and not over[:K.WAVE].any()                      # W0: the table
    assert np.flatnonzero(off[K.WAVE:2 * K.WAVE]).tolist() == [LANE_OFF]          # W1: that lane only
    assert not over[K.WAVE:2 * K.WAVE].any() and float(sq[K.WAVE + LANE_OFF]) < 96.0
    assert np.flatnonzero(over[2 * K.WAVE:]).tolist() == [K.LANE_EDGE]            # W2+: full form
    return par, ~K.wave_any(off | over)


def _margin(pp, par, s_p, cdf, u, table):
    """The derived margin (module docstring): the harness's MFMA-path margin, plus the rows'
    bound on the lanes whose wave takes the table."""
    m = pp.shape[0]
    pts = K.chunk_points(m)[0]
    ends = np.unique(np.concatenate([np.arange(pts - 1, m, pts), [m - 1]]))
    phi = np.diff(np.concatenate([np.zeros((cdf.shape[0], 1)), cdf[:, ends]], axis=1), axis=1).max(axis=1)
    u64 = np.asarray(u, np.float64)
    rows = ROW * (u64 + np.minimum(1.0, u64 + phi) + 2.0 * phi)
    return K.margin(pp, par, s_p, None) + np.where(table, rows, 0.0)


def _setup(m, kind):
    model, vbn, pk, pp, py, (s_p, s_y), _, _ = _case("A", 2, m, kind, WAVES)
    assert "kmt2" in pk.nodes[K.NODE].offs and "kmt" not in pk.nodes[K.NODE].offs
    par, table = _parents(pp, s_p, _table2(pk))
    cdf = K.kde_index_cdf64(pp, par, s_p)
    u = K.crafted_uniforms(cdf, m, K.SEED_U)
    return vbn, pk, pp, py, (s_p, s_y), par, table, cdf, u


@pytest.mark.parametrize("m", SIZES)
def test_table_waves(m, monkeypatch):
    from vectorizedbayesiannetwork_amd import plan as P
    vbn, pk, pp, _, (s_p, _), par, table, cdf, u = _setup(m, "index")
    zero = np.zeros(len(u), np.float32)
    _, xs = _launch(vbn, par, u=u, z=zero)
    _judge(f"A dp=2 M={m} tables", WAVES, cdf, u, _indices(xs, m), _margin(pp, par, s_p, cdf, u, table))
    # the same model packed without 2-D tables: a fresh model object and a fresh VBN
    monkeypatch.setattr(P, "KDE_MOMENTS2", False)
    vbn2 = _vbn(K.make_model(m, 2, "A", "index"))
    assert "kmt2" not in _pk(vbn2).nodes[K.NODE].offs
    _, xs2 = _launch(vbn2, par, u=u, z=zero)
    _judge(f"A dp=2 M={m} no tables", WAVES, cdf, u, _indices(xs2, m), K.margin(pp, par, s_p, None))
    changed = int((xs[:K.WAVE] != xs2[:K.WAVE]).sum())
    print(f"A dp=2 M={m}: W0 indices differing with / without the table: {changed} of {K.WAVE}")
    for w, name in enumerate(WAVES):
        if name != "W0":
            sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
            assert np.array_equal(xs[sl], xs2[sl]), f"{name}: differs with / without 2-D moment tables"
    # W0 reads the table, W1 and W2+ do not: zero the chunk rows 1-15 of every cell in the blob
    o = pk.nodes[K.NODE].offs["kmt2"]
    h = pk.params[o:o + P.KDE_MT2_HEADER].cpu().numpy()
    n0, n1 = (int(v) for v in h[[3, 7]].view(np.int32))
    rows, rowf = (int(v) for v in h[8:10].view(np.int32))
    tab = pk.params[o + P.KDE_MT2_HEADER:o + P.KDE_MT2_HEADER + n0 * n1 * rows * rowf].view(n0 * n1, rows, rowf)
    tab[:, 1:P.KDE_CHUNKS, :] = 0.0
    _, xs3 = _launch(vbn, par, u=u, z=zero)
    per = P.kde_moment2_geometry(m)[0]
    assert (xs[:K.WAVE] >= per).any(), "W0 has particles beyond chunk 0 with the table as packed"
    assert (xs3[:K.WAVE] < per).all(), "W0 did not follow the overwritten table"
    assert np.array_equal(xs3[K.WAVE:], xs[K.WAVE:]), "W1 / W2+ read the table"


@pytest.mark.parametrize("m", (100, 7169))
def test_plan_specialised_walk_is_bit_identical(m):
    """plan_jit=2 (the plan-specialised kernel, compiled in the call) on the same injected draws;
    M = 7169 has half rows (the located chunk's half sum is one more table row)."""
    vbn, pk, pp, _, (s_p, _), par, table, cdf, u = _setup(m, "index")
    zero = np.zeros(len(u), np.float32)
    _, xs0 = _launch(vbn, par, u=u, z=zero, plan_jit=0)
    _, xs2 = _launch(vbn, par, u=u, z=zero, plan_jit=2)
    assert np.array_equal(xs0, xs2)
    _judge(f"plan_jit=2 dp=2 M={m} tables", WAVES, cdf, u, _indices(xs2, m), _margin(pp, par, s_p, cdf, u, table))


@pytest.mark.parametrize("m", SIZES)
def test_log_density_from_table_total(m):
    """Sample and score in one step: the denominator ``lsp`` is ln(table total) - |x'|^2 ln 2 on
    the table wave; against the float64 log-density at the returned value."""
    vbn, pk, pp, py, sc, par, table, cdf, u = _setup(m, "density")
    s_p, s_y = sc
    z = np.random.default_rng([m, 2, 22]).standard_normal(len(u)).astype(np.float32)
    lp, xs = _launch(vbn, par, u=u, z=z, logp=True)
    ms, ok = _sampled_miss(py, float(np.float32(s_y)), cdf, u, z, xs, _margin(pp, par, s_p, cdf, u, table))
    assert ok.all(), np.flatnonzero(~ok)[:8]
    ref = K.kde_logp64(pp, py, par, xs, sc)
    err = np.abs(lp.astype(np.float64) - ref)
    for w, name in enumerate(WAVES):
        sl = slice(w * K.WAVE, (w + 1) * K.WAVE)
        print(f"A dp=2 M={m} {name}: largest miss {ms[sl].max():.3g}, largest log-density error {np.nanmax(err[sl]):.3g}")
    assert np.isfinite(ref).all()
    bad = np.flatnonzero(~K.logp_close(lp, ref))
    assert bad.size == 0, [(int(b), WAVES[b // K.WAVE], float(lp[b]), float(ref[b])) for b in bad[:8]]


@pytest.mark.parametrize("m", (100, 1000))
def test_set_b_declines(m):
    """Set B (|y'| ~ 6 per feature, terms of ~150): the grid is too fine for the size cap."""
    from vectorizedbayesiannetwork_amd.plan import PackedModel
    pk = PackedModel(K.make_model(m, 2, "B", "index"), torch.device("cpu"))
    assert "kmt2" not in pk.nodes[K.NODE].offs
