#!/usr/bin/env python3
"""Precompile the plan-specialised walks of the benchmark workloads on the build host (CPU,
hiprtc) into the package's plan cache (vectorizedbayesiannetwork_amd/plan_cache), so a fresh
GPU box loads them instead of compiling inside the first call.

    python scripts/precompile_plans.py [cfg2 cfg3 ...]        (default: --bench, every bench config;
                                                               --tests: the GPU tests' extra plans)

Per config: the bench engine's production plan (MCM / IS / LW) and, for shared-root engines,
its shared-sample precompute variant (plan.precompute_plans) -- the same step tables the
engines build, so the cache keys match.
"""
from __future__ import annotations

import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


ENGINES = {"mcm": "monte_carlo_marginalization", "is": "importance_sampling", "lw": "likelihood_weighting",
           "ancestral": "ancestral"}


def plans_for(name):
    """``cfg`` (the bench engine) or ``cfg:engine`` (mcm / is / lw / ancestral: the engines'
    plans for the GPU tests' workloads, which share the bench configs' DAGs).  Built through
    the engines' own ``engines._plan`` with their arguments (walk order and precompute
    included), so the step tables and cache keys are the engines'."""
    import bench
    from vectorizedbayesiannetwork_amd import engines as E
    from vectorizedbayesiannetwork_amd import plan as P
    cfg_name, _, eng_name = name.partition(":")
    cfg, model, target, ev = bench.build_model(cfg_name)
    pk = P.PackedModel(model, "cpu")
    vals = set(ev)
    fixed = [x for x in model.topo if x in vals]
    latent = [x for x in model.topo if x not in vals]
    logp_ev = [x for x in model.topo if x in ev]
    eng = ENGINES[eng_name] if eng_name else cfg["engine"]
    common = dict(latent=latent, fixed=fixed, out_nodes=[target], skip=[], exact_f32=False, kde_valu=False)
    if eng in ("likelihood_weighting", "importance_sampling"):
        lw = eng == "likelihood_weighting"
        key = ("weighted", target, tuple(sorted(ev)), (), lw, lw, False, False, False)
        plan = E._plan(pk, key, logp=logp_ev, shared_roots=lw, mode=P.MODE_WEIGHTED,
                       clamp=list(ev) if lw else (), **common)
    elif eng == "ancestral":
        key = ("ancestral", target, tuple(sorted(vals)), False, False, False)
        plan = E._plan(pk, key, logp=[], shared_roots=True, mode=P.MODE_SAMPLE, **common)
    elif eng == "monte_carlo_marginalization":
        key = ("mcm", target, tuple(sorted(vals)), False, False, False)
        plan = E._plan(pk, key, logp=[target], shared_roots=True, mode=P.MODE_MCM, **common)
    else:
        return cfg, []
    out = [("plain", plan, False)]
    if plan.pc is not None:
        out.append(("precompute", plan.pc, plan.pre is not None))
    return cfg, out


RFF8 = "rff8"          # the rff_gaussian fixture's walks (tests/test_gpu_rff.py), not a bench config


def rff8_plans():
    """The two every-node-out walks of tests/golden/rff/rff8.pt that tests/test_gpu_rff.py also runs
    plan-specialised, with injected draws: the full-wave kind set with the out-of-line steps (bit 9)
    and every kind, which is what vbn_hip_walk_kind_set gives such a launch."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import rff_reference as R
    from vectorizedbayesiannetwork_amd import jit
    from vectorizedbayesiannetwork_amd import plan as P
    from vectorizedbayesiannetwork_amd.model import model_from_checkpoint
    fx = R.load_rff8()
    pk = P.PackedModel(model_from_checkpoint(fx["model"]), "cpu")
    lines = []
    for case, weighted in R.jit_walk_cases(fx):
        plan = R.all_nodes_plan(pk, case, weighted)
        assert plan.kind_mask & P.KM_GENERIC_MLP
        steps, ic, _ = plan.steps._vbn_host
        t0, c0 = time.perf_counter(), jit.STATS["compile_s"]
        key, _ = jit.code_object(steps, ic, P.KM_GENERIC_MLP | P.KM_KINDS)
        lines.append(f"{RFF8} {'weighted' if weighted else 'sample'}: {key} "
                     f"({'compiled' if jit.STATS['compile_s'] > c0 else 'cached'} in {time.perf_counter() - t0:.1f} s)")
    return lines


BENCH = ["cfg2", "cfg3", "cfg4", "cfg5", "anchor64"]
# the extra plans of the GPU tests' workloads
TESTS = ["cfg2:is", "cfg2:lw", "cfg3:lw", "cfg3:mcm", "cfg3:ancestral", "cfg4:lw", "cfg4:ancestral",
         "cfg5:lw", "cfg5:ancestral", RFF8]
TAGS = ("plain", "precompute")


def _one(task):
    """One plan of one workload: (name, tag).  The precompute variant of a workload without one
    gives no line."""
    from vectorizedbayesiannetwork_amd import jit
    name, want = task
    if name == RFF8:
        return rff8_plans() if want == TAGS[0] else []
    cfg, plans = plans_for(name)
    lines = []
    for tag, plan, pre in plans:
        if tag != want:
            continue
        t0 = time.perf_counter()
        key, comp = jit.precompile(plan, cfg["B"], cfg["S"], precomp=pre)
        lines.append(f"{name} {tag}: {key} ({'compiled' if comp else 'cached'} in {time.perf_counter() - t0:.1f} s)")
    return lines


def main(names):
    from concurrent.futures import ProcessPoolExecutor, as_completed
    from vectorizedbayesiannetwork_amd import synthetic
    expanded = []
    for name in names or ["--bench"]:        # --bench / --tests may stand among config names
        expanded += BENCH if name == "--bench" else TESTS if name == "--tests" else [name]
    names = list(dict.fromkeys(expanded))
    for name in names:
        if name == RFF8:
            continue
        if name.partition(":")[0] not in synthetic.CONFIGS or name.partition(":")[2] not in ("", *ENGINES):
            raise SystemExit(f"unknown config {name}")
    # one task per plan, not per workload (a 128-node plan compiles for minutes, and a workload's
    # two plans need not wait for each other), the workloads with most nodes first; one hiprtc
    # compile per process at a time (single-threaded, ~1-2 GB each)
    names.sort(key=lambda n: -(8 if n == RFF8 else synthetic.CONFIGS[n.partition(":")[0]]["n_nodes"]))
    tasks = [(name, tag) for name in names for tag in TAGS]
    workers = max(1, min(len(tasks), (os.cpu_count() or 1), 8))
    with ProcessPoolExecutor(workers) as ex:
        for fut in as_completed([ex.submit(_one, t) for t in tasks]):
            for ln in fut.result():
                print(ln, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
