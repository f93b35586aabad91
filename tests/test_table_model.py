"""categorical_table networks on the host: records, checkpoints, packing and plans (CPU only)."""
import copy
import os

import networkx as nx
import numpy as np
import pytest
import torch

from vectorizedbayesiannetwork_amd import VBN, _lib
from vectorizedbayesiannetwork_amd import plan as P
from vectorizedbayesiannetwork_amd.engines import (CategoricalExact, GibbsSampler, Query,
                                                   RaoBlackwellizedMarginalization, ResampledImportanceSampling)
from vectorizedbayesiannetwork_amd.handle import CPDHandle
from vectorizedbayesiannetwork_amd.model import (CPD_KINDS, KIND_DEFAULTS, YAML_DEFAULTS, checkpoint_from_model,
                                                 model_from_checkpoint, random_table_model)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tabular", "table7.pt")
_FX = {}


def fixture():
    if not _FX:
        _FX.update(torch.load(FIXTURE, weights_only=True))
    return _FX


def packed():
    if "pk" not in _FX:
        _FX["pk"] = P.PackedModel(model_from_checkpoint(fixture()["model"]), torch.device("cpu"))
    return _FX["pk"]


def test_fixture_checkpoint_loads():
    m = model_from_checkpoint(fixture()["model"])
    assert m.topo == ["r2", "r3", "a4", "b5", "m6", "c9", "t2"]
    assert all(rec.kind == "categorical_table" for rec in m.cpds.values())
    assert m.cpds["c9"].extra["parent_strides"] == [20, 5, 1]
    assert m.cpds["t2"].state["_class_mask"].tolist() == [[True, True, False], [True, True, True]]
    assert "categorical_table" in CPD_KINDS
    assert KIND_DEFAULTS["categorical_table"] == dict(n_classes=0, parent_n_classes=None, alpha=1.0,
                                                       alpha_mode="per_class", prior="uniform")
    assert YAML_DEFAULTS["categorical_table"]["alpha_mode"] == "total_mass"
    assert YAML_DEFAULTS["categorical_table"]["prior"] == "global"


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_checkpoint_round_trip_reproduces_every_tensor():
    ck = fixture()["model"]
    out = checkpoint_from_model(model_from_checkpoint(ck))
    assert out["dag"] == ck["dag"]
    for node, info in ck["nodes"].items():
        got = out["nodes"][node]
        assert got["cpd_key"] == "categorical_table" and got["class_name"] == "CategoricalTableCPD"
        assert got["init_kwargs"] == info["init_kwargs"]
        assert (got["input_dim"], got["output_dim"]) == (info["input_dim"], info["output_dim"])
        for k, v in info["state_dict"].items():
            if k != "_extra_state":
                assert _same(v, got["state_dict"][k]), (node, k)
        for k, v in info["extra_state"].items():
            assert _same(v, got["extra_state"][k]), (node, k)
            assert _same(v, got["state_dict"]["_extra_state"][k]), (node, k)
    model_from_checkpoint(out)


def _edited(node, fn):
    ck = copy.deepcopy(fixture()["model"])
    fn(ck["nodes"][node])
    return ck


@pytest.mark.parametrize("key", ["_counts", "_class_values", "_class_mask"])
def test_missing_state_is_rejected(key):
    ck = _edited("b5", lambda n: n["state_dict"].pop(key))
    with pytest.raises(ValueError, match="not on the accelerated path"):
        model_from_checkpoint(ck)


def test_missing_parent_strides_is_rejected():
    def drop(n):
        n["extra_state"]["parent_strides"] = None
        n["state_dict"]["_extra_state"] = None
    with pytest.raises(ValueError, match="not on the accelerated path"):
        model_from_checkpoint(_edited("b5", drop))


def test_mixed_model_is_rejected():
    other = torch.load(os.path.join(os.path.dirname(FIXTURE), "..", "readme.pt"), weights_only=True)["model"]
    ck = copy.deepcopy(fixture()["model"])
    ck["nodes"]["r2"] = copy.deepcopy(other["nodes"]["feature_0"])
    with pytest.raises(ValueError, match="not on the accelerated path.*mixed networks"):
        model_from_checkpoint(ck)


def test_mismatched_parent_support_is_rejected():
    def shift(n):
        n["extra_state"]["parent_values"][1] = torch.tensor([1.0, 3.0, 4.0])      # r3 has classes 1, 3, 5
    with pytest.raises(ValueError, match="not on the accelerated path"):
        model_from_checkpoint(_edited("b5", shift))


def test_packed_log_prob_rows_equal_the_recorded_log_probs_bit_for_bit():
    """One table entry, no arithmetic in between: the packed row of the observed parent
    configuration holds exactly the reference's log_prob(x | parents) for 1-dim nodes."""
    fx, pk = fixture(), packed()
    blob = pk.params.numpy()
    model = pk.model
    checked = 0
    for case in fx["cases"]:
        if case["engine"] != "cpd" or model.out_dim(case["node"]) != 1:
            continue
        node = case["node"]
        npk, rec = pk.nodes[node], model.cpds[node]
        c, p, cp = npk.k, npk.aux0, npk.aux1
        rows = blob[npk.offs["pts"]:npk.offs["pts"] + p * cp].reshape(p, cp)
        cv = rec.state["_class_values"][0]
        for b in range(case["x"].shape[0]):
            cfg = 0
            for j, (vals, stride) in enumerate(zip(rec.extra["parent_values"], rec.extra["parent_strides"])):
                cfg += int((vals == case["parents"][b, j]).nonzero()[0, 0]) * stride
            k = int((cv == case["x"][b, 0]).nonzero()[0, 0])
            want = case["outputs"]["log_prob_x"][b, 0].numpy()
            assert rows[cfg, k].tobytes() == want.tobytes(), (node, b, rows[cfg, k], want)
            checked += 1
    assert checked == 18          # six 1-dim nodes x three rows


def test_packed_cdf_and_probability_rows():
    pk = packed()
    blob = pk.params.numpy()
    assert pk.tabular and blob.size % 256 == 0
    for node, npk in pk.nodes.items():
        c, p, cp = npk.k, npk.aux0, npk.aux1
        d = npk.out_dim
        assert cp % 4 == 0 and cp >= c and npk.kind == 5
        cdf = blob[npk.offs["w1"]:npk.offs["w1"] + d * p * cp].reshape(d, p, cp)
        prob = blob[npk.offs["w2"]:npk.offs["w2"] + d * p * cp].reshape(d, p, cp)
        assert (np.diff(cdf[..., :c], axis=-1) >= 0).all()
        assert np.allclose(cdf[..., c - 1], 1.0, atol=1e-6)
        assert (cdf[..., c:] == cdf[..., c - 1:c]).all()
        want = np.cumsum(prob[..., :c].astype(np.float64), axis=-1)
        assert np.abs(cdf[..., :c] - want).max() <= 2.0 ** -23
    # m6 was fitted with two classes it never saw: they keep ~1e-12 of the mass, not zero
    m6 = pk.nodes["m6"]
    prob = blob[m6.offs["w2"]:m6.offs["w2"] + m6.aux0 * m6.aux1].reshape(m6.aux0, m6.aux1)
    assert (prob[:, 4:6] > 0).all() and (prob[:, 4:6] < 1e-10).all()


def test_plan_marking():
    pk = packed()
    assert P.KIND_ID["categorical_table"] == 5
    plan = P.build_plan(pk, latent=["r2", "r3", "b5", "t2"], fixed=["a4", "m6", "c9"], logp=["c9"],
                        out_nodes=["b5"], shared_roots=True, mode=P.MODE_WEIGHTED, clamp=["c9"])
    assert plan.tabular and plan.kind_mask == 1024 and plan.pc is None and plan.pre is None
    assert plan.order == pk.model.topo
    assert plan.wbuf == pk.params.numel()
    assert plan.table_out_cols.tolist() == [plan.slot_of["b5"], pk.nodes["b5"].offs["w3"]]
    # c9 is scored, a4 is read by c9; m6 is evidence nobody reads
    assert plan.table_check == [("a4", 0, False), ("c9", 2, True)]
    rows = plan.steps.numpy()
    assert (rows[:, P.S_KIND] == 5).all()
    par = P.build_plan(pk, latent=[], fixed=["r3", "a4", "b5"], logp=[], out_nodes=["c9"], params=["c9"],
                       shared_roots=True, mode=P.MODE_SAMPLE, skip=["r2", "m6", "t2"])
    assert int(par.out_cols.numel()) == 9                        # PARAMS width D * C
    assert par.table_out_cols.tolist()[9:] == [-1] * 9
    two = P.build_plan(pk, latent=[], fixed=["b5"], logp=[], out_nodes=["t2"], params=["t2"],
                       shared_roots=True, mode=P.MODE_SAMPLE, skip=["r2", "r3", "a4", "m6", "c9"])
    assert int(two.out_cols.numel()) == 2 * 3


def test_other_models_keep_their_plans():
    other = torch.load(os.path.join(os.path.dirname(FIXTURE), "..", "readme.pt"), weights_only=True)["model"]
    pk = P.PackedModel(model_from_checkpoint(other), torch.device("cpu"))
    plan = P.build_plan(pk, latent=list(pk.model.topo), fixed=[], logp=[], out_nodes=[pk.model.topo[-1]],
                        shared_roots=True, mode=P.MODE_SAMPLE)
    assert not pk.tabular and not plan.tabular and plan.table_out_cols is None and not plan.kind_mask & P.KM_TABLE


def test_random_table_model_is_seeded_and_loads():
    g = nx.DiGraph()
    g.add_edges_from([("a", "c"), ("b", "c"), ("c", "d")])
    kw = dict(class_values={"b": [1, 3, 5]}, masked={"d": 1})
    m1 = random_table_model(g, {"a": 2, "b": 3, "c": 9, "d": 4}, seed=3, **kw)
    m2 = random_table_model(g, {"a": 2, "b": 3, "c": 9, "d": 4}, seed=3, **kw)
    m3 = random_table_model(g, {"a": 2, "b": 3, "c": 9, "d": 4}, seed=4, **kw)
    assert torch.equal(m1.cpds["c"].state["_counts"], m2.cpds["c"].state["_counts"])
    assert not torch.equal(m1.cpds["c"].state["_counts"], m3.cpds["c"].state["_counts"])
    assert tuple(m1.cpds["c"].state["_counts"].shape) == (1, 6, 9)
    assert m1.cpds["d"].state["_class_mask"].tolist() == [[True, True, True, False]]
    assert (m1.cpds["d"].state["_counts"][..., 3] == 0).all()
    model_from_checkpoint(checkpoint_from_model(m1))
    assert P.PackedModel(m1, torch.device("cpu")).tabular


def test_abi_version_is_14():
    assert _lib.ABI_VERSION == 14
    assert _lib.load().vbn_hip_abi_version() == 14
    assert "vbn_hip_table_walk" in _lib.EXPORTS


def test_handle_reports_the_kind():
    vbn = VBN.from_model(model_from_checkpoint(fixture()["model"]), device="cuda:0")
    h = CPDHandle(vbn, "c9")
    assert h.cpd_name == "categorical_table" and h.cpd_type == "CategoricalTableCPD"
    assert h.is_fitted and h.parents == ["r3", "a4", "b5"] and (h.input_dim, h.output_dim) == (3, 1)
    assert h.export_config()["extra_state"]["parent_strides"] == [20, 5, 1]


@pytest.mark.parametrize("make", [
    lambda: RaoBlackwellizedMarginalization(n_samples=8, fallback=None).infer_posterior,
    lambda: ResampledImportanceSampling(n_samples=8).infer_posterior,
    lambda: GibbsSampler(n_samples=8).sample,
])
def test_unsupported_engines_raise(make):
    vbn = VBN.from_model(model_from_checkpoint(fixture()["model"]), device="cuda:0")
    q = Query(target="c9", evidence={"a4": torch.tensor([[1.0]])})
    with pytest.raises(NotImplementedError, match="categorical_table"):
        make()(vbn, q)
    with pytest.raises(NotImplementedError, match="categorical_table"):
        vbn.pack_query({"target": "c9", "evidence": ["a4"]})


def test_categorical_exact_constructor_errors():
    with pytest.raises(ValueError, match="Unknown fallback inference"):
        CategoricalExact(fallback="nope")
    with pytest.raises(ValueError, match="fallback cannot be 'categorical_exact'"):
        CategoricalExact(fallback="categorical_exact")
    eng = CategoricalExact(fallback=None)
    assert eng.fallback == "none" and eng._fallback is None
    assert type(CategoricalExact(n_samples=32)._fallback).__name__ == "LikelihoodWeighting"
