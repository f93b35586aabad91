#!/usr/bin/env python3
"""Timing of the categorical_table walk (csrc/vbn_table_walk.hip) on one MI355X.

Workload: a 64-node ``random_table_model`` (synthetic.random_dag(64), 4 classes per node), the
synthetic query generator's target and N / 4 evidence nodes, likelihood weighting and Monte
Carlo marginalisation at B = 4096 queries x S = 1024 samples.  Per engine it records, HIP-event
timed on the launch stream, the whole ``infer_posterior`` step and the walk launch alone, the
particle-nodes per second of the walk (particles x walked steps / kernel time) and, as the bound
the kernel is judged against, the output-write floor: 8 bytes per particle (one weight, one
sample) at HBM speed.  Nothing ran such a model before, so there is no target and no baseline.

Usage: python scripts/bench_table.py [--steps K] [--warmup W] [--out profiles/bench_table.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vectorizedbayesiannetwork_amd import VBN, ops, synthetic  # noqa: E402
from vectorizedbayesiannetwork_amd import engines as E  # noqa: E402
from vectorizedbayesiannetwork_amd.model import random_table_model  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E peak, as bench.py prices traffic


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_table.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = synthetic.random_dag(args.nodes, seed=2)
    model = random_table_model(g, args.classes, seed=1)
    vbn = VBN.from_model(model, device="cuda:0")
    target, ev_nodes = synthetic.default_query_nodes(g, seed=1)
    gen = torch.Generator().manual_seed(3)
    b, s = args.queries, args.samples
    ev = {n: torch.randint(0, args.classes, (b, 1), generator=gen).float().to(dev) for n in ev_nodes}
    q = vbn._normalize_query({"target": target, "evidence": ev})
    pk = E.packed_model(vbn, dev)
    results = {}
    for name, eng in (("likelihood_weighting", E.LikelihoodWeighting(n_samples=s, seed=1)),
                      ("monte_carlo_marginalization", E.MonteCarloMarginalization(n_samples=s, seed=1))):
        step_ms = timed(lambda: eng.infer_posterior(vbn, q), args.steps, args.warmup)
        last = dict(E.LAST_LAUNCH)
        plan = last["plan"]
        rows = plan.steps._vbn_host[0]

        n_out = int(plan.out_cols.numel())

        def walk():              # the launch alone (engines._run_table_walk without the host-side support check)
            return ops.table_walk(plan.steps, plan.in_cols, pk.params, last["fixed"], None, plan.table_out_cols, b, s,
                                  plan.n_slots, plan.fixed_ld, False, 1, len(plan.noise_nodes), pk.dmax, n_out,
                                  plan.mode, 0, 7, 0, plan.mode != 2)
        kern_ms = timed(walk, args.steps, args.warmup)
        staged = bool(ops.LAST_WALK.get("table_staged"))
        walked = int((rows[:, 1] != 0).sum())
        particles = b * s
        floor_ms = particles * 8 / (HBM_PEAK_GBS * 1e9) * 1e3
        results[name] = {
            "ms_per_step": round(step_ms, 4), "walk_kernel_ms": round(kern_ms, 4),
            "queries_per_s": round(b / (step_ms * 1e-3), 1),
            "particle_nodes_per_s": round(particles * walked / (kern_ms * 1e-3), 1),
            "walked_steps": walked, "latent_steps": int((rows[:, 1] == 1).sum()), "n_slots": plan.n_slots,
            "tables": "LDS-staged" if staged else "global / L2",
            "output_write_floor_ms": round(floor_ms, 5), "floor_frac": round(floor_ms / kern_ms, 4),
        }
    out = {
        "metric": "categorical_table walk, ms per step and particle-nodes/s on 1 MI355X",
        "config": {"nodes": args.nodes, "classes": args.classes, "queries": b, "samples": s,
                   "evidence_nodes": len(ev_nodes), "blob_bytes": int(pk.params.numel()) * 4,
                   "dag": "synthetic.random_dag(seed=2)", "steps": args.steps, "warmup": args.warmup},
        "bound": f"output write: 8 B per particle at {HBM_PEAK_GBS:.0f} GB/s",
        "device": torch.cuda.get_device_name(0),
        "results": results,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
