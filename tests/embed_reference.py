"""Float64 restatement of the reference's ``categorical_embedded_softmax`` CPD (test helper; imports
no reference): a plain forward pass -- embedding rows gathered and concatenated, the MLP layer by
layer, masked classes filled with -1e9 (categorical_embedded_softmax.py:306-329, 469-511) -- behind
the interface of ``table_reference.TableCPD``, so that the engines and draw providers of
tests/table_reference.py run discrete models that mix both kinds."""
from __future__ import annotations

from typing import Optional

import torch

import table_reference as TR

F64 = torch.float64
_ACT = {"relu": torch.relu, "tanh": torch.tanh, "gelu": torch.nn.functional.gelu, "elu": torch.nn.functional.elu}


class EmbedCPD(TR.TableCPD):
    def __init__(self, rec):
        st = rec.state
        self.D = int(rec.output_dim)
        self.n_in = int(rec.input_dim)
        self.class_values = st["_class_values"].to(F64)
        self.class_mask = st["_class_mask"].bool()
        self.sample_values = st["_sample_values"].to(F64)
        self.parent_values = [v.to(F64) for v in ((rec.extra or {}).get("parent_values") or [])]
        self.root_logits = st["_logits"].to(F64) if self.n_in == 0 else None
        self.emb = [st[f"embeddings.{j}.weight"].to(F64) for j in range(self.n_in)]
        self.layers = [(w.to(F64), b.to(F64)) for w, b in rec.mlp_layers()]
        self.act = _ACT[str(rec.hp("activation"))]

    def logits(self, parents: Optional[torch.Tensor], b: int, s: int) -> torch.Tensor:
        """[b, s, D, C] (316-329); ``parents`` [b, s, n_in] or None."""
        if self.n_in == 0:
            out = self.root_logits.view(1, 1, self.D, -1).expand(b, s, -1, -1)
        else:
            flat = parents.reshape(b * s, -1)
            x = torch.cat([self.emb[j][TR.map_values(flat[:, j], self.parent_values[j])] for j in range(self.n_in)],
                          dim=-1)
            for i, (w, bias) in enumerate(self.layers):
                x = x @ w.t() + bias
                if i + 1 < len(self.layers):
                    x = self.act(x)
            out = x.reshape(b, s, self.D, -1)
        return out.masked_fill(~self.class_mask.view(1, 1, self.D, -1), -1e9)


class DiscreteModel(TR.TableModel):
    """``table_reference.TableModel`` over categorical_table and categorical_embedded_softmax nodes."""

    def __init__(self, model):
        self.model = model
        self.cpds = {n: (EmbedCPD if model.cpds[n].kind == "categorical_embedded_softmax" else TR.TableCPD)(model.cpds[n])
                     for n in model.topo}


def categorical_exact(tm: DiscreteModel, target, evidence, do, n, draws):
    """categorical_exact.py:89-128; an embedded root's row is softmax(_logits) as stored (58-66: no mask)."""
    cpd = tm.cpds[target]
    vals = TR._fixed(evidence or {}, do or {}, clamp=True)
    if isinstance(cpd, EmbedCPD) and cpd.n_in == 0 and cpd.D == 1 and target not in vals:
        b = TR._batch(evidence or {}, do or {})
        probs = torch.softmax(cpd.root_logits, dim=-1)[0].expand(b, -1)
        return probs, cpd.sample_values[0].view(1, -1, 1).expand(b, -1, 1), True
    return TR.categorical_exact(tm, target, evidence, do, n, draws)


def reference_error(cases, dm: DiscreteModel):
    """(e_ref, margins): the largest error of the recorded float32 log-probs of a fixture's CPD cases
    against this restatement, and per case the distance [B, S] of every recorded draw to a class boundary."""
    e_ref, margins = 0.0, []
    for case in cases:
        if case["engine"] != "cpd":
            continue
        cpd, par, out, n = dm.cpds[case["node"]], case["parents"], case["outputs"], case["n_samples"]
        b = 1 if par is None else par.shape[0]
        pp = None if par is None else par.double().unsqueeze(1)
        pn = None if pp is None else pp.expand(b, n, -1)
        draws = TR.ReplayDraws(case["draws"], b, n)
        xs = cpd.sample(case["node"], pn, b, n, draws, False)
        assert torch.equal(xs.float(), out["sample"]) and draws.exhausted()
        for got, want in ((cpd.log_prob(case["x"].double().unsqueeze(1), pp), out["log_prob_x"]),
                          (cpd.log_prob(xs, pn), out["log_prob_sampled"])):
            e_ref = max(e_ref, float((got - want.double()).abs().max()))
        margins.append(draws.margin)
    return e_ref, margins
