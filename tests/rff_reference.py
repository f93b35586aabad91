"""rff_gaussian and gaussian_exact restated for the tests (reference vbn/cpds/rff_gaussian.py:131-146,
183-211, 257-291; vbn/inference/gaussian_exact.py:65-183; the gaussian branch of
rao_blackwellized_marginalization.py for a ``_params`` target).

* :func:`params32` / :func:`sample32` / :func:`log_prob32` -- float32 torch in the reference's op
  order: they reproduce its recorded outputs bit for bit (tests/test_rff_reference.py);
* :func:`params64` -- the same formulas in float64 from the float32 parameters and parents: the
  yardstick the GPU step and the float32 restatement are both measured against;
* importing this module registers ``rff_gaussian`` in ``oracle.vbn_oracle``'s ``_SAMPLE`` / ``_LOGP``
  tables (at run time; nothing under oracle/ changes), so the oracle's engines walk models that hold
  the kind.  :func:`precision` switches the registered functions to a float64 ``loc`` (rounded to
  float32 once), which is how the tests measure what float32 evaluation costs a whole engine case;
* :func:`rao_blackwellized` and :func:`gaussian_exact` -- the two engines the oracle cannot restate
  for an rff target.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional

import torch

from oracle import vbn_oracle as O

_PRECISION = [32]


@contextlib.contextmanager
def precision(bits: int):
    """Within the block the registered oracle functions compute loc in float64 (bits = 64)."""
    old = _PRECISION[0]
    _PRECISION[0] = int(bits)
    try:
        yield
    finally:
        _PRECISION[0] = old


def scale32(rec) -> torch.Tensor:
    return torch.sqrt(rec.state["_var"].clamp(min=float(rec.hp("min_scale")) ** 2))       # 183-185


def n_features(rec) -> int:
    return int(rec.state["_rff_w"].shape[0])


def params32(rec, parents3: torch.Tensor):
    """_params (187-211) for parents [B, S, n_in]: (loc, scale) [B, S, D], float32."""
    st = rec.state
    b, s, d = parents3.shape
    flat = parents3.reshape(b * s, d)
    z = (flat - st["mean_x"].view(1, -1)) / st["std_x"].view(1, -1)                         # 131-136
    proj = z @ st["_rff_w"].t() + st["_rff_b"]                                               # 144
    feats = math.sqrt(2.0 / float(n_features(rec))) * torch.cos(proj)                        # 145-146
    loc_norm = (feats @ st["_coef"] + st["_bias"]).reshape(b, s, rec.output_dim)             # 201-202
    loc = loc_norm * st["std_y"].view(1, 1, -1) + st["mean_y"].view(1, 1, -1)                # 209
    return loc, scale32(rec).view(1, 1, -1).expand(b, s, -1)


def params64(rec, parents3: torch.Tensor):
    """The same formulas in float64 on the float32 parameters and parents (scale: the float32
    value, which is what every implementation holds)."""
    st = {k: v.double() for k, v in rec.state.items() if v.is_floating_point()}
    b, s, d = parents3.shape
    flat = parents3.double().reshape(b * s, d)
    z = (flat - st["mean_x"].view(1, -1)) / st["std_x"].view(1, -1)
    proj = z @ st["_rff_w"].t() + st["_rff_b"]
    feats = math.sqrt(2.0 / float(n_features(rec))) * torch.cos(proj)
    loc_norm = (feats @ st["_coef"] + st["_bias"]).reshape(b, s, rec.output_dim)
    loc = loc_norm * st["std_y"].view(1, 1, -1) + st["mean_y"].view(1, 1, -1)
    return loc, scale32(rec).double().view(1, 1, -1).expand(b, s, -1)


def _loc_scale(rec, parents3):
    if _PRECISION[0] == 64:
        loc, _ = params64(rec, parents3)
        return loc.float(), scale32(rec).view(1, 1, -1).expand(loc.shape[0], loc.shape[1], -1)
    return params32(rec, parents3)


def sample32(rec, parents: Optional[torch.Tensor], n: int, draws) -> torch.Tensor:
    """sample (257-269)"""
    if rec.is_root:
        b = 1 if parents is None else parents.shape[0]
        loc = rec.state["mean_y"].view(1, 1, -1).expand(b, n, -1)
        scale = scale32(rec).view(1, 1, -1).expand(b, n, -1)
    else:
        p = O._expand_s(parents, n)
        if p.dim() == 2:
            p = p.unsqueeze(1)
        loc, scale = _loc_scale(rec, p)
    eps = draws.normal(scale.shape)
    return loc + eps * scale


def log_prob32(rec, x: torch.Tensor, parents: Optional[torch.Tensor]) -> torch.Tensor:
    """log_prob (271-291)"""
    x = O._x3(x)
    b, s, _ = x.shape
    if rec.is_root:
        loc = rec.state["mean_y"].view(1, 1, -1).expand(b, s, -1)
        scale = scale32(rec).view(1, 1, -1).expand(b, s, -1)
    else:
        loc, scale = _loc_scale(rec, O._expand_s(parents, s))
    var = scale ** 2
    return -0.5 * (((x - loc) ** 2) / var + 2 * torch.log(scale) + math.log(2 * math.pi)).sum(dim=-1)


def log_prob64(rec, x: torch.Tensor, parents3: Optional[torch.Tensor]) -> torch.Tensor:
    """log_prob in float64 for x [B, S, D], parents [B, S, n_in] (None for a root)."""
    x = x.double()
    if rec.is_root:
        loc = rec.state["mean_y"].double().view(1, 1, -1)
        scale = scale32(rec).double().view(1, 1, -1)
    else:
        loc, scale = params64(rec, parents3)
    return -0.5 * (((x - loc) ** 2) / scale ** 2 + 2 * torch.log(scale) + math.log(2 * math.pi)).sum(dim=-1)


def register() -> None:
    """Teach the oracle's per-kind tables the kind (idempotent)."""
    O._SAMPLE["rff_gaussian"] = sample32
    O._LOGP["rff_gaussian"] = log_prob32


register()


def target_loc_scale(model, target: str, parents3: Optional[torch.Tensor], b: int):
    """(loc, scale) [B | 1, S | 1, D] of a Gaussian target the way the reference's ``_weight`` /
    ``_params`` branches give them (gaussian_exact.py:76-105; rao_blackwellized_marginalization.py
    :100-130), or None for a kind without Gaussian parameters."""
    rec = model.cpds[target]
    if rec.kind == "linear_gaussian":
        if parents3 is None:
            return rec.state["_bias"].view(1, 1, -1), O._lg_scale(rec).view(1, 1, -1)
        loc = parents3 @ rec.state["_weight"] + rec.state["_bias"]
        return loc, O._lg_scale(rec).view(1, 1, -1).expand_as(loc)
    if rec.kind == "gaussian_nn":
        return O._gnn_root_loc_scale(rec) if parents3 is None else O._gnn_loc_scale(rec, parents3)
    if rec.kind == "rff_gaussian":
        if parents3 is None:
            return rec.state["mean_y"], scale32(rec)
        return _loc_scale(rec, parents3)
    return None


def gaussian_exact(model, target: str, evidence: Dict, do: Dict, n_samples: int, *, stddevs: float = 4.0,
                   min_scale: float = 1e-6):
    """gaussian_exact.py:134-183.  Returns (pdf, samples, fallback): ``fallback`` True means the
    reference hands the query to its fallback engine (pdf / samples None)."""
    b = O._batch(evidence, do)
    if model.out_dim(target) != 1:                                                    # 146-147
        return None, None, True
    fixed = O._fixed(evidence, do, clamp=True)                                        # 141
    if target in fixed:                                                               # 149-153
        return torch.ones(b, 1), fixed[target].unsqueeze(1).expand(b, 1, -1), False
    ps = model.parents[target]
    if not all(p in fixed for p in ps):                                               # 155-158
        return None, None, True
    pt = torch.cat([fixed[p].unsqueeze(1).expand(b, 1, -1) for p in ps], dim=-1) if ps else None
    prm = target_loc_scale(model, target, pt, b)
    if prm is None:                                                                   # 168-170
        return None, None, True
    loc, scale = O._rb_to3d(prm[0], b), O._rb_to3d(prm[1], b)                         # 111-112
    scale = torch.nan_to_num(scale, nan=min_scale, posinf=min_scale, neginf=min_scale).abs().clamp_min(min_scale)
    loc, scale = loc[:, :1, :], scale[:, :1, :]
    z = torch.linspace(-stddevs, stddevs, n_samples).view(1, n_samples, 1)            # 173-176
    samples = loc + scale * z
    log_pdf = -0.5 * (z ** 2 + 2.0 * torch.log(scale) + math.log(2.0 * math.pi)).sum(dim=-1)
    return torch.exp(log_pdf), samples, False


def rao_blackwellized(model, target: str, evidence: Dict, do: Dict, n_samples: int, n_particles: int, draws,
                      stddevs: float = 4.0, min_scale: float = 1e-6):
    """oracle.rao_blackwellized with an rff_gaussian target served by the gaussian branch (the
    reference reaches it through ``_params``, rao_blackwellized_marginalization.py:125-130); every
    other target goes to the oracle."""
    rec = model.cpds[target]
    if rec.kind != "rff_gaussian":
        return O.rao_blackwellized(model, target, evidence, do, n_samples, n_particles, draws, stddevs, min_scale)
    b = O._batch(evidence, do)
    desc = O.descendants(model, target)
    if any(x in evidence or x in do for x in desc):
        return None, None, "target has observed/intervened descendants"
    fixed = O._fixed(evidence, do, clamp=True)
    if target in fixed:
        return torch.ones(b, 1), fixed[target].unsqueeze(1).expand(b, 1, -1), None
    cols, total = O._layout(model)
    P = n_particles
    particles = torch.zeros(b, P, total)
    log_w = torch.zeros(b, P)
    for node in model.topo:
        if node in desc or node == target:
            continue
        pt = O._gather_parents(model, node, particles, cols)
        if node in fixed:
            value = fixed[node].unsqueeze(1).expand(b, P, -1)
            particles[..., cols[node]] = value
            if node in evidence:
                log_w = log_w + O.cpd_log_prob(model.cpds[node], value, pt)
            continue
        particles[..., cols[node]] = O.cpd_sample(model.cpds[node], pt, P, draws)
    w = O.rb_normalized_weights(log_w)
    pt = O._gather_parents(model, target, particles, cols)
    loc, scale = target_loc_scale(model, target, pt, b)
    loc, scale = O._rb_to3d(loc, b), O._rb_to3d(scale, b)
    if loc.shape[-1] != 1 or scale.shape[-1] != 1:
        return None, None, "unsupported target CPD for RB marginalization"
    if scale.shape[1] == 1 and loc.shape[1] > 1:
        scale = scale.expand(-1, loc.shape[1], -1)
    elif loc.shape[1] == 1 and scale.shape[1] > 1:
        loc = loc.expand(-1, scale.shape[1], -1)
    scale = torch.nan_to_num(scale, nan=min_scale, posinf=min_scale, neginf=min_scale).abs().clamp_min(min_scale)
    if loc.shape[1] != P:
        loc = loc.expand(-1, P, -1)
        scale = scale.expand(-1, P, -1)
    comp_var = scale.squeeze(-1) ** 2
    comp_mean = loc.squeeze(-1)
    mix_mean = (w * comp_mean).sum(dim=1)
    second = (w * (comp_var + comp_mean ** 2)).sum(dim=1)
    mix_std = (second - mix_mean ** 2).clamp_min(min_scale ** 2).sqrt()
    z = torch.linspace(0.0, 1.0, n_samples).view(1, n_samples, 1)
    lo = (mix_mean - stddevs * mix_std).view(b, 1, 1)
    hi = (mix_mean + stddevs * mix_std).view(b, 1, 1)
    grid = lo + (hi - lo) * z
    x = grid.squeeze(-1).unsqueeze(1)
    mu = loc.squeeze(-1).unsqueeze(-1)
    sigma = scale.squeeze(-1).unsqueeze(-1).clamp_min(min_scale)
    comp_pdf = torch.exp(-0.5 * ((x - mu) / sigma) ** 2) / (math.sqrt(2.0 * math.pi) * sigma)
    return (w.unsqueeze(-1) * comp_pdf).sum(dim=1), grid, None


# ----------------------------------------------------------------------------------------
# what the tests share: the fixture, the per-node float32 error scale, the engine cases
# ----------------------------------------------------------------------------------------
_FIXTURE = []


def load_rff8():
    """tests/golden/rff/rff8.pt (make_golden_rff.py), loaded once."""
    import os
    if not _FIXTURE:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rff", "rff8.pt")
        _FIXTURE.append(torch.load(path, weights_only=True))
    return _FIXTURE[0]


def fit_rows(model, data, node: str, mult: float = 1.0) -> torch.Tensor:
    """The node's parent rows of the fit data [N, n_in], scaled by ``mult``."""
    return (torch.cat([data[p] for p in model.parents[node]], dim=-1) * mult).contiguous()


def sigma_ref(rec, parents: torch.Tensor) -> float:
    """RMS deviation of the float32 restatement's loc from the float64 one on ``parents`` [N, n_in]:
    the error scale of a float32 evaluation of this node on these rows."""
    p3 = parents.unsqueeze(1)
    return float((params32(rec, p3)[0].double() - params64(rec, p3)[0]).pow(2).mean().sqrt())


def run_engine_case(model, case):
    """The patched oracle on one recorded engine case -> the outputs dict the fixture records."""
    q, n, p, eng = case["query"], case["n_samples"], case["params"], case["engine"]
    draws = O.ReplayDraws(case["draws"])
    t, ev, do = q["target"], q["evidence"], q["do"]
    if eng == "monte_carlo_marginalization":
        pdf, xs = O.monte_carlo_marginalization(model, t, ev, do, n, draws)
        out = {"pdf": pdf, "samples": xs}
    elif eng == "likelihood_weighting":
        w, xs = O.likelihood_weighting(model, t, ev, do, n, draws, normalize=p.get("normalize", True))
        out = {"pdf": w, "samples": xs}
    elif eng == "importance_sampling":
        w, xs, ess, fb = O.importance_sampling(model, t, ev, do, n, draws, ess_threshold=p.get("ess_threshold", 0.1))
        out = {"pdf": w, "samples": xs, "ess": ess, "fallback": fb}
    elif eng == "ancestral":
        out = {"samples": O.ancestral(model, t, ev, do, n, draws)}
    elif eng == "resampled_importance_sampling":
        w, xs, ess, rs = O.resampled_importance_sampling(model, t, ev, do, n, draws,
                                                         ess_threshold=p.get("ess_threshold", 0.5),
                                                         resample=p.get("resample", True),
                                                         clamp_obs=p.get("clamp_obs", True))
        out = {"pdf": w, "samples": xs, "resampled": rs}
        if ess is not None:
            out["ess"] = ess
    elif eng == "rao_blackwellized_marginalization":
        pdf, xs, reason = rao_blackwellized(model, t, ev, do, n, p["n_particles"], draws)
        if reason:
            pdf, xs = O.likelihood_weighting(model, t, ev, do, n, draws)
        out = {"pdf": pdf, "samples": xs, "fallback": bool(reason), "reason": reason or ""}
    elif eng == "gibbs":
        out = {"samples": O.gibbs(model, t, ev, do, n, draws, burn_in=p["burn_in"], n_steps=p["n_steps"])}
    elif eng == "gaussian_exact":
        pdf, xs, fb = gaussian_exact(model, t, ev, do, n, **p)
        if fb:
            pdf, xs = O.likelihood_weighting(model, t, ev, do, n, draws)
        out = {"pdf": pdf, "samples": xs, "fallback": fb}
    else:
        raise AssertionError(eng)
    assert draws.exhausted(), "the oracle consumed fewer draws than the reference"
    return out


def all_nodes_plan(pk, case, weighted: bool):
    """The walk of a recorded case's query with every node written out (MODE_WEIGHTED: the evidence
    nodes' log-probs accumulated; else MODE_SAMPLE).  tests/test_gpu_rff.py walks it;
    scripts/precompile_plans.py compiles its plan-specialised form ahead of time."""
    from vectorizedbayesiannetwork_amd import plan as P
    model = pk.model
    ev, do = list(case["query"]["evidence"]), list(case["query"]["do"])
    fixed = [x for x in model.topo if x in ev or x in do]
    return P.build_plan(pk, latent=[x for x in model.topo if x not in fixed], fixed=fixed,
                        logp=[x for x in model.topo if x in ev] if weighted else [], out_nodes=model.topo,
                        shared_roots=True, mode=P.MODE_WEIGHTED if weighted else P.MODE_SAMPLE)


def jit_walk_cases(fx):
    """(case, weighted) of the two dag8 walks that also run plan-specialised."""
    cases = fx["cases"]
    anc = next(c for c in cases if c["engine"] == "ancestral" and c["query"]["evidence"])
    lw = next(c for c in cases if c["engine"] == "likelihood_weighting" and "x2" in c["query"]["evidence"])
    return [(anc, False), (lw, True)]
