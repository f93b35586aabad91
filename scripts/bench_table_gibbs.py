#!/usr/bin/env python3
"""Timing of the Gibbs sweeps on a categorical_table network (csrc/vbn_table_gibbs.h) on one MI355X.

Workload: a 24-node ``random_table_model`` (synthetic.random_dag(24), 4 classes per node), the
synthetic query generator's target and evidence nodes, ``GibbsSampler(tables=True)`` with the YAML
defaults (512 samples, burn-in 50, 5 steps between samples: 2610 sweeps) at 4096 chains.  HIP-event
timed on the launch stream: the whole ``sample`` step (start-state walk, host-side support check,
sweep launch) and the sweep launch alone, under the three table placements --

* ``rule``:   what vbn_hip_table_walk's staging rule chooses for the launch,
* ``global``: VBN_TABLE_GLOBAL=1, tables gathered from global / L2,
* ``staged``: VBN_TABLE_STAGE=1 (A/B only), tables in LDS whenever the workgroup fits 64 KiB --

alternated over ``--rounds`` rounds so that drift on a shared host shows as spread, not as a
difference.  It also checks that the three give bit-identical chains.  Nothing ran such a sweep
before, so there is no target and no baseline.

Usage: python scripts/bench_table_gibbs.py [--steps K] [--warmup W] [--rounds R] [--out profiles/bench_table_gibbs.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vectorizedbayesiannetwork_amd import VBN, defaults, ops, synthetic  # noqa: E402
from vectorizedbayesiannetwork_amd import engines as E  # noqa: E402
from vectorizedbayesiannetwork_amd import plan as P  # noqa: E402
from vectorizedbayesiannetwork_amd.model import random_table_model  # noqa: E402

PLACEMENTS = {"rule": {}, "global": {"VBN_TABLE_GLOBAL": "1"}, "staged": {"VBN_TABLE_STAGE": "1"}}


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


def placed(name: str):
    for k in ("VBN_TABLE_GLOBAL", "VBN_TABLE_STAGE"):
        os.environ.pop(k, None)
    os.environ.update(PLACEMENTS[name])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=24)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_table_gibbs.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = synthetic.random_dag(args.nodes, seed=2)
    model = random_table_model(g, args.classes, seed=1)
    vbn = VBN.from_model(model, device="cuda:0")
    target, ev_nodes = synthetic.default_query_nodes(g, seed=1)
    gen = torch.Generator().manual_seed(3)
    b = args.chains
    ev = {n: torch.randint(0, args.classes, (b, 1), generator=gen).float().to(dev) for n in ev_nodes}
    q = vbn._normalize_query({"target": target, "evidence": ev})
    pk = E.packed_model(vbn, dev)
    cfg = {k: v for k, v in defaults.sampling("gibbs").items() if k != "name"}
    eng = E.GibbsSampler(tables=True, seed=1, **cfg)
    n = cfg["n_samples"]
    iters = cfg["burn_in"] + n * max(cfg["n_steps"], 1)
    gp = eng._gibbs_plan(pk, target, {k: v for k, v in ev.items()})
    init = gp.init
    fx = E._fixed_buffer(init, ev, b, dev)
    state = torch.empty(init.n_slots + 1, b, device=dev, dtype=torch.float32)
    E.run_walk(pk, init, fx, b, 1, seed=1, state=state, state_flags=2)
    chains = state.view(init.n_slots + 1, b, 1).expand(-1, -1, 8).reshape(init.n_slots + 1, b * 8).contiguous()
    dt = model.out_dim(target)

    def sweeps():                # the sweep launch alone, the final sweep collected (collect="reference")
        return ops.gibbs_walk(gp.steps, gp.in_cols, pk.params, fx, None, chains, b, init.n_slots, init.max_out,
                              init.fixed_ld, b, gp.n_noise, pk.dmax, dt, iters, iters - 1, 1, 0, 7, 1, gp.kind_mask)

    rows = gp.steps.cpu().numpy()
    scored = int(((rows[:, P.S_ROLE] == P.ROLE_LATENT) | (rows[:, P.S_ROLE] == P.ROLE_FIXED)).sum())
    times = {name: {"step": [], "kernel": []} for name in PLACEMENTS}
    outs, staged = {}, {}
    for _ in range(args.rounds):
        for name in PLACEMENTS:
            placed(name)
            times[name]["kernel"].append(timed(sweeps, args.steps, args.warmup))
            staged[name] = bool(ops.LAST_WALK.get("table_staged"))
            times[name]["step"].append(timed(lambda: eng.sample(vbn, q, n), args.steps, args.warmup))
            outs[name] = sweeps().cpu()
    placed("rule")
    same = all(torch.equal(outs["rule"], o) for o in outs.values())
    results = {}
    for name, t in times.items():
        k = sorted(t["kernel"])
        results[name] = {
            "tables": "LDS-staged" if staged[name] else "global / L2",
            "sweep_kernel_ms": [round(x, 3) for x in t["kernel"]], "sweep_kernel_ms_median": round(k[len(k) // 2], 3),
            "sample_step_ms": [round(x, 3) for x in t["step"]],
            "us_per_sweep": round(k[len(k) // 2] * 1e3 / iters, 3),
            "scored_rows_per_s": round(b * 8 * scored * iters / (k[len(k) // 2] * 1e-3), 1),
        }
    out = {
        "metric": "categorical_table Gibbs sweeps, ms per launch of all sweeps on 1 MI355X",
        "config": {"nodes": args.nodes, "classes": args.classes, "chains": b, "sweeps": iters, **cfg,
                   "evidence_nodes": len(ev_nodes), "blob_bytes": int(pk.params.numel()) * 4, "n_slots": init.n_slots,
                   "sweep_rows": int(gp.n_steps), "scored_rows": scored, "dag": "synthetic.random_dag(seed=2)",
                   "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds},
        "device": torch.cuda.get_device_name(0),
        "placements_bit_identical": same,
        "results": results,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
