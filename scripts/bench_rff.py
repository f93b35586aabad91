#!/usr/bin/env python3
"""Timing of the rff_gaussian step (csrc/vbn_walk_rff.h) on one MI355X.

Workload: a 32-node all-``rff_gaussian`` random DAG (synthetic.random_dag(32), F = 256 features per
node, random-init models fitted on SEM data), the synthetic query generator's target and N / 4
evidence nodes, Monte Carlo marginalisation at B = 4096 queries x S = 1024 samples.  The whole
``infer_posterior`` step (one walk launch) is HIP-event timed on the launch stream, 20 steps
after 5.  Next to it, two floors per particle-node, summed over the walked non-root rff steps:

* the cosine issue floor: F cosines of ``COS_VALU`` VALU instructions each (the float64 reduction,
  both polynomials, the quadrant select and the product with coef; counted in the disassembly of
  ``rff_loc``), one wave64 instruction per 4 cycles per SIMD;
* the MFMA floor: 2 ceil(F / 32) ceil(n_in / 2) v_mfma_f32_32x32x2_f32 per wave, 64 cycles per SIMD each.

Nothing ran such a model before, so there is no target and no baseline.

Usage: python scripts/bench_rff.py [--steps K] [--warmup W] [--out profiles/bench_rff.json]
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
from vectorizedbayesiannetwork_amd import plan as P  # noqa: E402
from vectorizedbayesiannetwork_amd.model import random_init_model  # noqa: E402

CUS, SIMDS, CLOCK_GHZ = 256, 4, 2.4      # MI355X
COS_VALU = 31                            # VALU instructions per feature and particle in rff_loc's inner block
VALU_CYCLES, MFMA_CYCLES = 4, 64         # per wave64 instruction, per SIMD


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
    ap.add_argument("--nodes", type=int, default=32)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_rff.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = synthetic.random_dag(args.nodes, seed=0)
    data = synthetic.sem_data(g, 2048, seed=0)
    model = random_init_model(g, synthetic.round_robin_kinds(g, ("rff_gaussian",)), data, seed=0,
                              overrides={"rff_gaussian": {"n_features": args.features}})
    vbn = VBN.from_model(model, device="cuda:0")
    target, ev_nodes = synthetic.default_query_nodes(g, seed=1)
    b, s = args.queries, args.samples
    rows = torch.randint(0, 2048, (b,), generator=torch.Generator().manual_seed(3))
    ev = {n: data[n][rows].to(dev) for n in ev_nodes}
    q = vbn._normalize_query({"target": target, "evidence": ev})
    results = {}
    for label, pj in (("interpreter", False),):      # the step-table interpreter: no hiprtc compile on GPU time
        eng = E.MonteCarloMarginalization(n_samples=s, seed=1, plan_jit=pj)
        ms = timed(lambda: eng.infer_posterior(vbn, q), args.steps, args.warmup)
        results[label] = {"ms_per_step": round(ms, 4), "specialised": bool(ops.LAST_WALK.get("specialised"))}
    pk = E.packed_model(vbn, dev)
    plan = next(v for k, v in model._cache.items() if k[:2] == ("plan", "mcm"))
    tab = plan.steps._vbn_host[0]
    walked = [r for r in tab if r[P.S_KIND] == P.KIND_ID["rff_gaussian"] and r[P.S_NIN] > 0
              and (r[P.S_ROLE] == P.ROLE_LATENT or r[P.S_FLAGS] & P.F_LOGP)]
    waves = b * s / 64
    slots = CUS * SIMDS * CLOCK_GHZ * 1e9
    cos_cycles = sum(int(r[P.S_K]) * COS_VALU * VALU_CYCLES for r in walked)           # per wave: F per lane (2 groups x F / 2 halves)
    mfma_cycles = sum(2 * -(-int(r[P.S_K]) // 32) * -(-int(r[P.S_NIN]) // 2) * MFMA_CYCLES for r in walked)
    out = {
        "metric": "rff_gaussian walk (MCM), ms per step on 1 MI355X",
        "config": {"nodes": args.nodes, "features": args.features, "queries": b, "samples": s,
                   "evidence_nodes": len(ev_nodes), "walked_rff_steps": len(walked), "n_slots": plan.n_slots,
                   "max_out": plan.max_out, "kind_mask": plan.kind_mask, "steps": args.steps, "warmup": args.warmup,
                   "blob_bytes": int(pk.params.numel()) * 4},
        "floors_ms": {"cosine_issue": round(waves * cos_cycles / slots * 1e3, 3),
                      "mfma": round(waves * mfma_cycles / slots * 1e3, 3),
                      "cos_valu_per_feature": COS_VALU},
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
