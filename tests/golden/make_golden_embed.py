#!/usr/bin/env python3
"""Generate the categorical_embedded_softmax fixture from the Python reference (build container only).

Writes ``tests/golden/embed/embed6.pt`` with make_golden_table.py's recipe: a briefly fitted
discrete network, the reference's outputs for the engines the table walk serves and every draw
the reference made (class index + CDF midpoint, make_golden.Recorder).  It lives in a
subdirectory so that the frozen oracle's fixture glob does not pick it up.

The model (8 nodes, one-dimensional unless noted; E = embedding_dim):

* ``r2`` embedded root, 2 classes;  ``r3`` categorical_table root, class values 1, 3, 5;
* ``a4`` <- r2: hidden (20,), tanh, E = 5, 4 classes;
* ``b9`` <- r2, r3: hidden (64, 64), relu, E = 8, 9 classes (a table parent feeds an embedded child);
* ``c3`` <- r3, a4, b9 (3 parents, cardinalities 3, 4, 9): no hidden layer, gelu, fitted without
  ``n_classes`` on the values 1, 3, 5;
* ``m6`` <- a4: hidden (64, 64), elu, ``n_classes=6`` on data that shows classes 0..3 only (this
  CPD keeps all six valid: categorical_embedded_softmax.py:213-227);
* ``t2`` <- b9: two output dims with 2 and 3 classes (dim 0 has a masked class, filled with -1e9), hidden (20,), relu;
* ``d4`` <- c3: a categorical_table child of an embedded parent, 4 classes.

Usage: python tests/golden/make_golden_embed.py [--out tests/golden/embed]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, checkpoint_dict, fit_model, run_case, run_cpd_case  # noqa: E402

import torch  # noqa: E402

NODES = ("r2", "r3", "a4", "b9", "c3", "m6", "t2", "d4")
EDGES = (("r2", "a4"), ("r2", "b9"), ("r3", "b9"), ("r3", "c3"), ("a4", "c3"), ("b9", "c3"), ("a4", "m6"),
         ("b9", "t2"), ("c3", "d4"))
KINDS = {n: "categorical_embedded_softmax" for n in NODES}
KINDS.update(r3="categorical_table", d4="categorical_table")
KWARGS = {
    "a4": {"hidden_dims": (20,), "activation": "tanh", "embedding_dim": 5},
    "c3": {"hidden_dims": (), "activation": "gelu"},
    "m6": {"activation": "elu", "n_classes": 6},
    "t2": {"hidden_dims": (20,)},
}


def embed_data(n: int = 600, seed: int = 13):
    gen = torch.Generator().manual_seed(seed)

    def ri(hi):
        return torch.randint(0, hi, (n,), generator=gen)
    r2 = ri(2)
    k3 = ri(3)
    a4 = (r2 + ri(3)) % 4
    b9 = (4 * r2 + 2 * k3 + ri(3)) % 9
    c3 = (a4 + b9 + k3 + ri(2)) % 3
    m6 = (a4 + ri(2)) % 4
    t2 = torch.stack([b9 % 2, (b9 + ri(2)) % 3], dim=1)
    d4 = (c3 + ri(2)) % 4
    cols = {"r2": r2, "r3": 2 * k3 + 1, "a4": a4, "b9": b9, "c3": 2 * c3 + 1, "m6": m6, "d4": d4}
    data = {k: v.float().unsqueeze(-1) for k, v in cols.items()}
    data["t2"] = t2.float()
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "embed"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(REF, "vbn")):
        print(f"reference not found at {REF}; nothing to do")
        return 0
    sys.path.insert(0, REF)
    os.environ.setdefault("CI", "1")
    import networkx as nx
    import vbn as vbn_mod

    torch.manual_seed(0)
    g = nx.DiGraph()
    g.add_nodes_from(NODES)
    g.add_edges_from(EDGES)
    data = embed_data()
    vbn = fit_model(vbn_mod, g, KINDS, data, extra_kwargs=KWARGS, epochs=8)

    B, S = 3, 16
    rows = torch.arange(B) * 7 + 3

    def ev(*nodes, r=rows):
        return {n: data[n][r].clone() for n in nodes}

    s = 9500
    mcm, lw, imp, cex = ("monte_carlo_marginalization", "likelihood_weighting", "importance_sampling",
                         "categorical_exact")
    cases = [
        run_case(vbn, s + 1, mcm, {"target": "c3", "evidence": ev("a4", "m6")}, S),
        run_case(vbn, s + 2, mcm, {"target": "c3", "evidence": ev("r3", "a4", "b9")}, S),
        run_case(vbn, s + 3, mcm, {"target": "b9", "do": ev("b9")}, S),
        run_case(vbn, s + 4, mcm, {"target": "r2", "evidence": ev("a4", r=rows[:1])}, S),
        run_case(vbn, s + 5, mcm, {"target": "d4", "evidence": ev("t2")}, S),
        run_case(vbn, s + 6, lw, {"target": "b9", "evidence": ev("c3", "m6", "d4")}, S),
        run_case(vbn, s + 7, lw, {"target": "a4", "evidence": ev("c3", "t2"), "do": ev("r3")}, S, normalize=False),
        run_case(vbn, s + 8, imp, {"target": "b9", "evidence": ev("c3", "m6")}, S, ess_threshold=0.0),
        run_case(vbn, s + 9, imp, {"target": "b9", "evidence": ev("c3", "m6")}, S, ess_threshold=1.1),
        run_case(vbn, s + 10, "ancestral", {"target": "c3", "evidence": ev("r2")}, S),
        run_case(vbn, s + 11, "ancestral", {"target": "t2", "evidence": ev("r3")}, S),
        run_case(vbn, s + 12, cex, {"target": "c3", "evidence": ev("r3", "a4", "b9")}, S),
        run_case(vbn, s + 13, cex, {"target": "c3", "evidence": ev("a4")}, S),
        run_case(vbn, s + 14, cex, {"target": "r2", "evidence": ev("a4")}, S),
        run_case(vbn, s + 15, cex, {"target": "m6", "evidence": ev("a4")}, S),
        run_case(vbn, s + 16, cex, {"target": "d4", "evidence": ev("c3")}, S),
        run_case(vbn, s + 17, cex, {"target": "t2", "evidence": ev("b9")}, S),
    ]
    for i, node in enumerate(NODES):
        pa = list(g.predecessors(node))
        par = torch.cat([data[p][rows] for p in pa], dim=-1) if pa else None
        cases.append(run_cpd_case(vbn, node, s + 100 + i, par, S, x=data[node][rows]))

    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "embed6.pt")
    torch.save({"model": checkpoint_dict(vbn), "cases": cases}, path)
    torch.load(path, weights_only=True)        # must be loadable without unpickling code
    print(f"embed6: {len(cases)} cases -> {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
