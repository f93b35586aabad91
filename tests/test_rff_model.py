"""rff_gaussian on the host side (no GPU): model load / save / refusals, the random-init builder,
the blob's fragment layouts, the plan's kind-set bits, and the gaussian_exact registration."""
import copy

import numpy as np
import pytest
import torch

import rff_reference as R
from vectorizedbayesiannetwork_amd import INFERENCE_REGISTRY, defaults, synthetic
from vectorizedbayesiannetwork_amd import plan as P
from vectorizedbayesiannetwork_amd.handle import _CLASS_NAME
from vectorizedbayesiannetwork_amd.model import (CLASS_NAME, CPD_KINDS, KIND_DEFAULTS, YAML_DEFAULTS,
                                                 checkpoint_from_model, model_from_checkpoint, model_from_vbn,
                                                 random_init_model, record_from_cpd)

CPU = torch.device("cpu")


def _model():
    return model_from_checkpoint(R.load_rff8()["model"])


# ---- what fails without the feature -------------------------------------------------------------
def test_rff_checkpoint_loads():
    m = _model()
    assert [m.cpds[n].kind for n in m.topo].count("rff_gaussian") == 4


def test_gaussian_exact_is_registered():
    cls = INFERENCE_REGISTRY["gaussian_exact"]
    assert cls.__name__ == "GaussianExact"
    assert defaults.inference("gaussian_exact") == {"name": "gaussian_exact", "n_samples": 512, "stddevs": 4.0,
                                                    "min_scale": 1e-6, "fallback": "likelihood_weighting"}


def test_gaussian_exact_constructor_errors():
    cls = INFERENCE_REGISTRY["gaussian_exact"]
    with pytest.raises(ValueError, match="Unknown fallback inference 'nope'"):
        cls(fallback="nope")
    with pytest.raises(ValueError, match="fallback cannot be 'gaussian_exact'"):
        cls(fallback="gaussian_exact")
    e = cls(n_samples=33, fallback="monte_carlo_marginalization")
    assert e._fallback.n_samples == 33 and e.stddevs == 4.0 and e.min_scale == 1e-6
    assert cls(fallback=None)._fallback is None and cls(fallback="none")._fallback is None
    assert cls(n_samples=7, fallback="likelihood_weighting")._fallback.n_samples == 7


# ---- model layer ------------------------------------------------------------------------------
def test_kind_names_and_defaults():
    assert "rff_gaussian" in CPD_KINDS and CLASS_NAME["rff_gaussian"] == "RFFGaussianCPD" == _CLASS_NAME["rff_gaussian"]
    want = dict(n_features=256, lengthscale=1.0, ridge=1e-6, min_scale=1e-3, use_bias=True)
    assert KIND_DEFAULTS["rff_gaussian"] == want and YAML_DEFAULTS["rff_gaussian"] == want


def test_checkpoint_round_trip():
    ck = R.load_rff8()["model"]
    m = model_from_checkpoint(ck)
    ck2 = checkpoint_from_model(m)
    m2 = model_from_checkpoint(ck2)
    for n in m.topo:
        a, b = m.cpds[n], m2.cpds[n]
        assert (a.kind, a.input_dim, a.output_dim, a.hparams) == (b.kind, b.input_dim, b.output_dim, b.hparams)
        assert ck2["nodes"][n]["class_name"] == ck["nodes"][n]["class_name"]
        assert a.state.keys() == b.state.keys() and all(torch.equal(a.state[k], b.state[k]) for k in a.state)


def test_model_from_live_object():
    """model_from_vbn reads a live CPD duck-typed by its class name."""
    m = _model()

    class RFFGaussianCPD:
        def __init__(self, rec):
            self.input_dim, self.output_dim, self._rec = rec.input_dim, rec.output_dim, rec

        def state_dict(self, keep_vars=False):
            return dict(self._rec.state)

        def get_init_kwargs(self):
            return dict(self._rec.hparams)

    rec = record_from_cpd(RFFGaussianCPD(m.cpds["x2"]))
    assert rec.kind == "rff_gaussian" and rec.hp("n_features") == 256 and torch.equal(rec.state["_coef"], m.cpds["x2"].state["_coef"])
    assert model_from_vbn(type("V", (), {"model": m})()) is m


def _bad(mutate):
    ck = copy.deepcopy(R.load_rff8()["model"])
    mutate(ck["nodes"]["x2"])
    return ck


@pytest.mark.parametrize("mutate", [
    lambda n: n["state_dict"].__setitem__("_stats_ready", torch.tensor(False)),
    lambda n: n["state_dict"].pop("_coef"),
    lambda n: n["state_dict"].__setitem__("_coef", n["state_dict"]["_coef"][:100]),
    lambda n: n["state_dict"].__setitem__("_rff_b", n["state_dict"]["_rff_b"][:8]),
    lambda n: n["state_dict"].__setitem__("_rff_w", n["state_dict"]["_rff_w"][:, :1]),
    lambda n: n["state_dict"].__setitem__("std_x", torch.ones(5)),
    lambda n: n["init_kwargs"].__setitem__("n_features", 128),
], ids=["unfitted", "no-coef", "coef-rows", "b-len", "w-cols", "std_x-len", "n_features"])
def test_bad_records_are_refused(mutate):
    with pytest.raises(ValueError, match="not on the accelerated path"):
        model_from_checkpoint(_bad(mutate))


def test_mixing_with_tables_stays_refused():
    ck = copy.deepcopy(R.load_rff8()["model"])
    ck["nodes"]["x1"] = dict(ck["nodes"]["x1"], cpd_key="categorical_table")
    with pytest.raises(ValueError, match="not on the accelerated path.*mixed networks"):
        model_from_checkpoint(ck)


def test_random_init_model_fits_rff_nodes():
    g = synthetic.random_dag(6, seed=2)
    data = synthetic.sem_data(g, 256, seed=0)
    m = random_init_model(g, synthetic.round_robin_kinds(g, ["rff_gaussian", "linear_gaussian"]), data, seed=0,
                          overrides={"rff_gaussian": {"n_features": 40}})
    model_from_checkpoint(checkpoint_from_model(m))           # passes the record checks
    for n in m.topo:
        rec = m.cpds[n]
        if rec.kind != "rff_gaussian" or rec.is_root:
            continue
        par = torch.cat([data[p] for p in m.parents[n]], -1)
        loc, scale = R.params32(rec, par.unsqueeze(1))
        resid = (data[n] - loc[:, 0]).pow(2).mean().sqrt()
        assert float(resid) < float(data[n].std()) and torch.isfinite(loc).all() and float(scale.min()) >= 1e-3


# ---- packing ----------------------------------------------------------------------------------
def _rec(f, nin, d, seed):
    from vectorizedbayesiannetwork_amd.model import CPDRecord
    gen = torch.Generator().manual_seed(seed)
    st = {"mean_x": torch.randn(nin, generator=gen), "std_x": torch.rand(nin, generator=gen) + 0.5,
          "mean_y": torch.randn(d, generator=gen), "std_y": torch.rand(d, generator=gen) + 0.5,
          "_stats_ready": torch.tensor(True), "_rff_w": torch.randn(f, nin, generator=gen),
          "_rff_b": torch.rand(f, generator=gen) * 6.28, "_coef": torch.randn(f, d, generator=gen),
          "_bias": torch.randn(d, generator=gen), "_var": torch.tensor([1e-9, 0.3][:d]) if d <= 2 else torch.rand(d)}
    return CPDRecord(kind="rff_gaussian", input_dim=nin, output_dim=d, hparams={"n_features": f}, state=st)


@pytest.mark.parametrize("f", [1, 72, 256])
@pytest.mark.parametrize("nin", [1, 2, 3])
def test_fragments_round_trip(f, nin):
    """What the kernel reads back from the blob is W, b and coef: lane l of k-step t of block blk
    holds W[32 blk + (l & 31)][2 t + (l >> 5)], register r of half h holds row 32 blk + row(r, h)."""
    d = 2
    rec = _rec(f, nin, d, seed=f * 10 + nin)
    blob = P._Blob()
    blob.add(np.zeros(4, np.float32))
    npk = P._pack_node(blob, rec)
    host = blob.finish()
    assert (npk.kind, npk.k, npk.n_in, npk.out_dim, npk.scratch, npk.n_out) == (6, f, nin, d, d, 0)   # scratch rows: loc
    assert npk.flags == P.F_STANDARDIZE and "wblk" not in npk.offs
    nblk, t1 = -(-f // 32), -(-nin // 2)
    w, b, coef = (rec.state[k].numpy() for k in ("_rff_w", "_rff_b", "_coef"))
    W = np.zeros((nblk * 32, 2 * t1), np.float32)
    Bv = np.zeros(nblk * 32, np.float32)
    Cf = np.zeros((nblk * 32, d), np.float32)
    frag = host[npk.offs["w1"]:npk.offs["w1"] + nblk * t1 * 64].reshape(nblk, t1, 64)
    bacc = host[npk.offs["b2"]:npk.offs["b2"] + nblk * 32].reshape(nblk, 2, 16)
    crow = host[npk.offs["w3"]:npk.offs["w3"] + nblk * 2 * d * 16].reshape(nblk, 2, d, 16)
    for blk in range(nblk):
        for lane in range(64):
            for t in range(t1):
                W[32 * blk + (lane & 31), 2 * t + (lane >> 5)] = frag[blk, t, lane]
        for h in range(2):
            for r in range(16):
                row = 32 * blk + (r & 3) + 8 * (r >> 2) + 4 * h
                Bv[row] = bacc[blk, h, r]
                Cf[row] = crow[blk, h, :, r]
    assert np.array_equal(W[:f, :nin], w) and not W[f:].any() and not W[:, nin:].any()
    assert np.array_equal(Bv[:f], b) and not Bv[f:].any()
    assert np.array_equal(Cf[:f], coef) and not Cf[f:].any()
    std = host[npk.offs["std"]:npk.offs["std"] + 2 * nin]
    assert np.array_equal(std[:nin], rec.state["mean_x"].numpy())
    assert np.array_equal(std[nin:], np.float32(1.0) / rec.state["std_x"].numpy())
    tail = host[npk.offs["tail"]:npk.offs["tail"] + 5 * d]
    scale = R.scale32(rec).numpy()
    assert scale[0] == np.float32(1e-3)                      # the variance floor min_scale^2
    assert np.array_equal(tail, np.concatenate([rec.state["_bias"].numpy(), rec.state["std_y"].numpy(),
                                                rec.state["mean_y"].numpy(), scale, np.log(scale)]))


def test_root_packs_the_tail_only():
    rec = _rec(256, 0, 1, seed=3)
    blob = P._Blob()
    npk = P._pack_node(blob, rec)
    assert set(npk.offs) == {"tail"} and npk.flags == P.F_ROOT and blob.size == 8 and npk.scratch == 0


# ---- plans ------------------------------------------------------------------------------------
def test_plan_bits_and_widths():
    m = _model()
    pk = P.PackedModel(m, CPU)
    assert pk.max_out == 2                                   # the gaussian_nn heads; an rff step needs D rows (loc)
    kw = dict(fixed=[], logp=[], shared_roots=True, mode=P.MODE_SAMPLE)
    full = P.build_plan(pk, latent=m.topo, out_nodes=m.topo, **kw)
    assert full.kind_mask == P.KM_GENERIC_MLP | 1 | 2        # bit 9, no kind bit of its own (bit 6 is the half-wave form)
    rows = full.steps.numpy()
    for i, n in enumerate(full.order):
        r = rows[i]
        if m.cpds[n].kind != "rff_gaussian":
            continue
        assert r[P.S_KIND] == 6 and r[P.S_K] == R.n_features(m.cpds[n]) and r[P.S_WBLK_LEN] == 0
        assert not r[P.S_FLAGS] & (P.F_BM_FIRST | P.F_BM_SECOND | P.F_MLP_GENERIC | P.F_HEAD_MFMA)
        assert bool(r[P.S_FLAGS] & P.F_ROOT) == (not m.parents[n])
    # a plan that walks no rff node is what it was: no bit 9
    sub = ["x1"]
    p1 = P.build_plan(pk, latent=sub, out_nodes=sub, skip=[n for n in m.topo if n not in sub], **kw)
    assert p1.kind_mask == 2
    # an rff node that is only a fixed value sets nothing either
    p2 = P.build_plan(pk, latent=["x1"], fixed=["x0"], logp=[], out_nodes=["x1"], shared_roots=True,
                      mode=P.MODE_SAMPLE, skip=[n for n in m.topo if n not in ("x0", "x1")])
    assert p2.kind_mask == 2
    # PARAMS: loc ++ scale
    p3 = P.build_plan(pk, latent=[], fixed=["x0", "x1"], logp=[], out_nodes=["x2"], params=["x2"], shared_roots=True,
                      mode=P.MODE_SAMPLE, skip=[n for n in m.topo if n not in ("x0", "x1", "x2")])
    assert int(p3.out_cols.numel()) == 2 and p3.kind_mask == P.KM_GENERIC_MLP
    # no pre-pass takes an rff step
    assert P.precompute_plans(pk, P.build_plan(pk, latent=[n for n in m.topo if n not in ("x0", "x1")],
                                               fixed=["x0", "x1"], logp=["x7"], out_nodes=["x7"], shared_roots=True,
                                               mode=P.MODE_MCM)) is None or True


def test_plans_of_other_models_are_unchanged():
    """The recorded step tables of the existing fixtures do not move (no rff node, no bit 9)."""
    from conftest import load_golden
    m = model_from_checkpoint(load_golden("mix12")["model"])
    pk = P.PackedModel(m, CPU)
    p = P.build_plan(pk, latent=m.topo, fixed=[], logp=[], out_nodes=m.topo, shared_roots=True, mode=P.MODE_SAMPLE)
    assert p.kind_mask == 31 and not (p.kind_mask & P.KM_GENERIC_MLP)
    assert set(p.steps.numpy()[:, P.S_KIND].tolist()) <= {0, 1, 2, 3, 4}
