#!/usr/bin/env python3
"""Generate the categorical_table fixtures from the Python reference (build container only).

Writes ``tests/golden/tabular/table7.pt``: a fitted all-``categorical_table`` network, the
reference's outputs for the engines the table walk serves and every draw the reference made
(class index + CDF midpoint, make_golden.Recorder).  The fixtures live in a subdirectory because
``tests/conftest.py::golden_names`` feeds every ``tests/golden/*.pt`` to the frozen oracle, which
does not know this CPD.

The model (7 nodes, one-dimensional unless noted):

* ``r2`` root, 2 classes;  ``r3`` root, class values 1, 3, 5;
* ``a4`` <- r2, 4 classes;  ``b5`` <- r2, r3, 5 classes;
* ``c9`` <- r3, a4, b5 (3 parents), 9 classes: rows longer than two float4 loads;
* ``m6`` <- a4, fitted with ``n_classes=6`` on data that shows classes 0..3 only: classes 4 and 5
  keep no counts (mass ~1e-12);
* ``t2`` <- b5, two output dims with 2 and 3 classes: dim 0 has a masked class.

Usage: python tests/golden/make_golden_table.py [--out tests/golden/tabular]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, Recorder, checkpoint_dict, fit_model, run_case, run_cpd_case  # noqa: E402,F401

import torch  # noqa: E402

NODES = ("r2", "r3", "a4", "b5", "c9", "m6", "t2")
EDGES = (("r2", "a4"), ("r2", "b5"), ("r3", "b5"), ("r3", "c9"), ("a4", "c9"), ("b5", "c9"), ("a4", "m6"),
         ("b5", "t2"))


def table_data(n: int = 600, seed: int = 11):
    gen = torch.Generator().manual_seed(seed)

    def ri(hi):
        return torch.randint(0, hi, (n,), generator=gen)
    r2 = ri(2)
    k3 = ri(3)
    a4 = (r2 + ri(3)) % 4
    b5 = (2 * r2 + k3 + ri(2)) % 5
    c9 = (a4 + b5 + k3 + ri(3)) % 9
    m6 = (a4 + ri(2)) % 4
    t2 = torch.stack([b5 % 2, (b5 + ri(2)) % 3], dim=1)
    cols = {"r2": r2, "r3": 2 * k3 + 1, "a4": a4, "b5": b5, "c9": c9, "m6": m6}
    data = {k: v.float().unsqueeze(-1) for k, v in cols.items()}
    data["t2"] = t2.float()
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "tabular"))
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
    data = table_data()
    kinds = {n: "categorical_table" for n in NODES}
    vbn = fit_model(vbn_mod, g, kinds, data, extra_kwargs={"m6": {"n_classes": 6}}, epochs=1)

    B, S = 3, 16
    rows = torch.arange(B) * 7 + 3

    def ev(*nodes, r=rows):
        return {n: data[n][r].clone() for n in nodes}

    s = 9000
    cases = [
        run_case(vbn, s + 1, "monte_carlo_marginalization", {"target": "c9", "evidence": ev("a4", "m6")}, S),
        run_case(vbn, s + 2, "monte_carlo_marginalization", {"target": "c9", "evidence": ev("r3", "a4", "b5")}, S),
        run_case(vbn, s + 3, "monte_carlo_marginalization", {"target": "b5", "do": ev("b5")}, S),
        run_case(vbn, s + 4, "monte_carlo_marginalization", {"target": "r3", "evidence": ev("a4", r=rows[:1])}, S),
        run_case(vbn, s + 5, "likelihood_weighting", {"target": "b5", "evidence": ev("c9", "m6")}, S),
        run_case(vbn, s + 6, "likelihood_weighting", {"target": "a4", "evidence": ev("c9"), "do": ev("r3")}, S,
                 normalize=False),
        run_case(vbn, s + 7, "importance_sampling", {"target": "b5", "evidence": ev("c9", "m6")}, S,
                 ess_threshold=0.0),
        run_case(vbn, s + 8, "importance_sampling", {"target": "b5", "evidence": ev("c9", "m6")}, S,
                 ess_threshold=1.1),
        run_case(vbn, s + 9, "ancestral", {"target": "c9", "evidence": ev("r2")}, S),
        run_case(vbn, s + 10, "categorical_exact", {"target": "c9", "evidence": ev("r3", "a4", "b5")}, S),
        run_case(vbn, s + 11, "categorical_exact", {"target": "c9", "evidence": ev("a4")}, S),
        run_case(vbn, s + 12, "monte_carlo_marginalization", {"target": "c9", "evidence": ev("c9")}, S),
    ]
    for i, node in enumerate(NODES):
        pa = list(g.predecessors(node))
        par = torch.cat([data[p][rows] for p in pa], dim=-1) if pa else None
        cases.append(run_cpd_case(vbn, node, s + 100 + i, par, S, x=data[node][rows]))

    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table7.pt")
    torch.save({"model": checkpoint_dict(vbn), "cases": cases}, path)
    torch.load(path, weights_only=True)        # must be loadable without unpickling code
    print(f"table7: {len(cases)} cases -> {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
