"""categorical_embedded_softmax networks on the host (CPU only): records, checkpoints, refusals, plan
marking, and tests/embed_reference.py against the recorded float32 outputs of golden/embed/embed6.pt."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import embed_reference as ER  # noqa: E402
from vectorizedbayesiannetwork_amd import VBN  # noqa: E402
from vectorizedbayesiannetwork_amd import plan as P  # noqa: E402
from vectorizedbayesiannetwork_amd.engines import GibbsSampler, Query  # noqa: E402
from vectorizedbayesiannetwork_amd.model import checkpoint_from_model, model_from_checkpoint  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embed", "embed6.pt")
_FX = {}


def fixture():
    if not _FX:
        _FX.update(torch.load(FIXTURE, weights_only=True))
        _FX["m"] = model_from_checkpoint(_FX["model"])
        _FX["dm"] = ER.DiscreteModel(_FX["m"])
    return _FX


def test_restatement_reproduces_the_fixture():
    fx = fixture()
    e_ref, margins = ER.reference_error(fx["cases"], fx["dm"])
    share = max(float((m < e_ref).mean()) for m in margins)
    print(f"e_ref = {e_ref:.3e}; largest share of particles within e_ref of a class boundary = {share:.4f}")
    assert 0 < e_ref < 1e-5          # float32 forward pass of logits of a few units
    assert share <= 1e-3             # the replay tests' cap holds for float32 vs float64 on these draws


def test_fixture_checkpoint_round_trips():
    fx = fixture()
    m, ck = fx["m"], fx["model"]
    assert [m.cpds[n].kind == "categorical_table" for n in m.topo] == [n in ("r3", "d4") for n in m.topo]
    assert m.cpds["c3"].state["_class_values"].tolist() == [[1.0, 3.0, 5.0]]
    # n_classes = 6 keeps the two classes the data never showed valid; only a narrower dim is masked
    assert m.cpds["m6"].state["_class_mask"].tolist() == [[True] * 6]
    assert m.cpds["t2"].state["_class_mask"].tolist() == [[True, True, False], [True, True, True]]
    out = checkpoint_from_model(m)
    for node, info in ck["nodes"].items():
        got = out["nodes"][node]
        assert all(got[k] == info[k] for k in ("cpd_key", "class_name", "init_kwargs", "input_dim", "output_dim"))
        pairs = [(v, got["state_dict"][k]) for k, v in info["state_dict"].items() if k != "_extra_state"]
        pairs += list(zip(info["extra_state"]["parent_values"], got["extra_state"]["parent_values"]))
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in pairs), node
        assert info["extra_state"]["parent_cards"] == got["extra_state"]["parent_cards"]
    model_from_checkpoint(out)


@pytest.mark.parametrize("edit", [
    lambda n: n["state_dict"].update(_stats_ready=torch.tensor(False)),                       # unfitted
    lambda n: n["state_dict"].update({"net.2.weight": n["state_dict"]["net.2.weight"][:, :-1]}),   # shapes do not chain
    lambda n: n.update(init_kwargs=dict(n["init_kwargs"], activation="selu")),                # no such activation
    lambda n: n["extra_state"]["parent_values"].__setitem__(1, torch.tensor([1.0, 3.0, 4.0])),    # r3 has 1, 3, 5
    lambda n: n["state_dict"].update({"net.0.weight": torch.zeros(96, 16), "net.0.bias": torch.zeros(96),
                                      "net.2.weight": torch.zeros(64, 96)}),                  # hidden layer > 64
])
def test_unsupported_records_are_refused(edit):
    ck = copy.deepcopy(fixture()["model"])
    edit(ck["nodes"]["b9"])
    with pytest.raises(ValueError, match="not on the accelerated path"):
        model_from_checkpoint(ck)


def test_plan_marking_and_unsupported_engines():
    m = fixture()["m"]
    pk = P.PackedModel(m, torch.device("cpu"))
    assert P.KIND_ID["categorical_embedded_softmax"] == 7 and P.KM_EMBED == 2048
    assert pk.nodes["r2"].kind == 5 and pk.nodes["b9"].kind == 7          # an embedded root walks as a table
    plan = P.build_plan(pk, latent=["r2", "r3", "a4", "b9", "t2"], fixed=["c3", "m6", "d4"], logp=["c3"],
                        out_nodes=["b9"], shared_roots=True, mode=P.MODE_WEIGHTED)
    assert plan.tabular and plan.kind_mask == 1024 | 2048 and plan.max_out == 9
    roots = P.build_plan(pk, latent=["r2", "r3"], fixed=[], logp=[], out_nodes=["r2"], shared_roots=True,
                         mode=P.MODE_SAMPLE, skip=["a4", "b9", "c3", "m6", "t2", "d4"])
    assert roots.kind_mask == 1024                                         # no embedded step walked
    vbn = VBN.from_model(m, device="cuda:0")
    with pytest.raises(NotImplementedError, match="categorical_table / categorical_embedded_softmax networks"):
        GibbsSampler(n_samples=8).sample(vbn, Query(target="c3", evidence={"a4": torch.tensor([[1.0]])}))
    with pytest.raises(NotImplementedError, match="categorical_embedded_softmax"):
        vbn.pack_query({"target": "c3", "evidence": ["a4"]})
