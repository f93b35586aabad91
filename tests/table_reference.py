"""Float64 restatement of the reference's ``categorical_table`` CPD and of the engines' op
sequence on all-tabular models, with pluggable draws (test helper; imports no reference).

* CPD (reference ``vbn/cpds/categorical_table.py:359-417``): ``probs = counts[:, cfg] /
  sum.clamp_min(1e-12)``, ``logits = log(probs.clamp_min(1e-12))``, ``log_prob =
  log_softmax(logits)[class]``, ``sample ~ Categorical(logits)`` returned as class values;
  ``_map_values_to_indices`` (12-20) raises ``ValueError("Found values outside support.")``.
* Engines: monte_carlo_marginalization.py:18-92, likelihood_weighting.py:24-82,
  importance_sampling.py:24-93, sampling/ancestral.py:13-65, categorical_exact.py:89-128 --
  the same branches, topological loops and weight arithmetic.

Draws come from a provider with ``categorical(node, probs [Bq, S, D, C], shared, q0) -> index
[Bq, S, D]``:

* :class:`ReplayDraws` replays a fixture's recorded class indices (make_golden.Recorder: one
  ``cat`` record per CPD call, flattened [b, s, d]);
* :class:`PhiloxTableDraws` recomputes the table walk's production draws: stream 1, word 0 of
  ``rng_words`` (csrc/vbn_walk_common.h) keyed by (seed, offset, node id, dim, query key -- 0 for
  shared root draws --, sample), and picks "the smallest k with cdf[k] > u * total, else C - 1"
  on the float64 CDF of the float64 probabilities.

Both record, per particle, the smallest distance (CDF units, total = 1) of any draw's uniform to
a class boundary (``margin`` [B, S]): the kernel's float32 CDF row may only pick a neighbouring
class where that distance is below its rounding.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from philox_draws import philox2x32, u01

F64 = torch.float64


# ---- the CPD ---------------------------------------------------------------------------------

def map_values(values: torch.Tensor, support: torch.Tensor) -> torch.Tensor:
    """categorical_table.py:12-20"""
    support = support.to(F64).contiguous()
    values = values.to(F64).contiguous()
    idx = torch.searchsorted(support, values)
    if bool((idx >= support.shape[0]).any()):
        raise ValueError("Found values outside support.")
    if not bool((support[idx] == values).all()):
        raise ValueError("Found values outside support.")
    return idx


class TableCPD:
    def __init__(self, rec):
        st = rec.state
        self.D = int(rec.output_dim)
        self.n_in = int(rec.input_dim)
        self.counts = st["_counts"].to(F64)
        self.class_values = st["_class_values"].to(F64)
        self.class_mask = st["_class_mask"].bool()
        self.sample_values = st["_sample_values"].to(F64)
        extra = rec.extra or {}
        self.parent_values = [v.to(F64) for v in (extra.get("parent_values") or [])]
        self.parent_strides = [int(s) for s in (extra.get("parent_strides") or [])]

    def parents_to_index(self, parents: Optional[torch.Tensor], rows: int) -> torch.Tensor:
        if self.n_in == 0:
            return torch.zeros(rows, dtype=torch.long)
        idx = torch.zeros(parents.shape[0], dtype=torch.long)
        for d, support in enumerate(self.parent_values):
            idx = idx + map_values(parents[:, d], support) * self.parent_strides[d]
        return idx

    def logits(self, parents: Optional[torch.Tensor], b: int, s: int) -> torch.Tensor:
        """[b, s, D, C] (359-377); ``parents`` [b, s, n_in] or None."""
        flat = None if parents is None else parents.reshape(b * s, -1)
        cfg = self.parents_to_index(flat, b * s)
        probs = self.counts[:, cfg, :]
        probs = probs / probs.sum(dim=-1, keepdim=True).clamp_min(1e-12)
        return torch.log(probs.clamp_min(1e-12)).permute(1, 0, 2).reshape(b, s, self.D, -1)

    def probs(self, parents, b, s) -> torch.Tensor:
        return torch.softmax(self.logits(parents, b, s), dim=-1)

    def log_prob(self, x: torch.Tensor, parents: Optional[torch.Tensor]) -> torch.Tensor:
        """x [b, s, D], parents [b, s, n_in] | None -> [b, s] (398-417)"""
        b, s, _ = x.shape
        lp = torch.log_softmax(self.logits(parents, b, s), dim=-1)
        xf = x.reshape(-1, self.D)
        tgt = torch.zeros(xf.shape[0], self.D, dtype=torch.long)
        for d in range(self.D):
            tgt[:, d] = map_values(xf[:, d], self.class_values[d][self.class_mask[d]])
        tgt = tgt.reshape(b, s, self.D)
        return lp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1).sum(dim=-1)

    def sample(self, node: str, parents: Optional[torch.Tensor], b: int, s: int, draws, shared: bool, q0: int = 0
               ) -> torch.Tensor:
        idx = draws.categorical(node, self.probs(parents, b, s), shared, q0)            # [b, s, D]
        vals = self.class_values.view(1, 1, self.D, -1).expand(b, s, -1, -1)
        return vals.gather(-1, idx.unsqueeze(-1)).squeeze(-1)


# ---- draw providers ----------------------------------------------------------------------------

def _choose(p: np.ndarray, u: np.ndarray):
    """(index, margin) of "smallest k with cdf[k] > u * total, else C - 1" on float64 rows."""
    c = p.shape[1]
    cdf = np.cumsum(p, axis=1)
    tot = cdf[:, -1]
    thr = u.astype(np.float64) * tot
    inner = cdf[:, :c - 1]
    idx = (inner <= thr[:, None]).sum(axis=1)
    if c == 1:
        return idx, np.full(len(idx), np.inf)
    lo = np.take_along_axis(inner, np.clip(idx - 1, 0, c - 2)[:, None], 1)[:, 0]
    hi = np.take_along_axis(inner, np.clip(idx, 0, c - 2)[:, None], 1)[:, 0]
    lo_gap = np.where(idx > 0, np.abs(thr - lo), np.inf)
    hi_gap = np.where(idx < c - 1, np.abs(hi - thr), np.inf)
    return idx, np.minimum(lo_gap, hi_gap) / np.where(tot > 0, tot, 1.0)


class _Margins:
    def __init__(self, n_queries: int, n_samples: int):
        self.B, self.S = int(n_queries), int(n_samples)
        self.margin = np.full((self.B, self.S), np.inf)
        self.n_draws = 0

    def _note(self, margin: np.ndarray, bq: int, s: int, d: int, shared_rows: bool, q0: int) -> None:
        m = margin.reshape(bq, s, d).min(axis=2)
        if shared_rows:                              # one row of draws used by every query
            self.margin = np.minimum(self.margin, m[:1])
        else:
            self.margin[q0:q0 + bq] = np.minimum(self.margin[q0:q0 + bq], m)
        self.n_draws += margin.size


class ReplayDraws(_Margins):
    """Recorded draws of one fixture case (one phase): class indices in call order per node."""

    def __init__(self, records: List[dict], n_queries: int, n_samples: int, phase: Optional[int] = 0):
        super().__init__(n_queries, n_samples)
        self.idx: Dict[str, List[torch.Tensor]] = {}
        self.mid: Dict[str, List[torch.Tensor]] = {}
        for r in records:
            if r["kind"] != "cat" or r["node"] is None or (phase is not None and r["phase"] != phase):
                continue
            self.idx.setdefault(r["node"], []).append(r["index"].long().reshape(-1))
            self.mid.setdefault(r["node"], []).append(r["value"].double().reshape(-1))
        self.pos = {n: 0 for n in self.idx}

    def categorical(self, node: str, probs: torch.Tensor, shared: bool, q0: int = 0) -> torch.Tensor:
        bq, s, d, c = probs.shape
        n = bq * s * d
        allv, allm = torch.cat(self.idx[node]), torch.cat(self.mid[node])
        at = self.pos[node]
        if at + n > allv.numel():
            raise RuntimeError(f"replay: node {node} has {allv.numel()} recorded draws, asked for {at + n}")
        self.pos[node] = at + n
        idx = allv[at:at + n]
        # the recorded uniform is the midpoint of the chosen class's CDF interval
        chosen, margin = _choose(probs.reshape(n, c).numpy(), allm[at:at + n].numpy())
        assert (chosen == idx.numpy()).all(), f"replay: node {node}: recorded midpoints choose other classes"
        self._note(margin, bq, s, d, shared and bq == 1 and self.B > 1, q0)
        return idx.reshape(bq, s, d)

    def exhausted(self) -> bool:
        return all(self.pos[n] == sum(v.numel() for v in self.idx[n]) for n in self.idx)


class PhiloxTableDraws(_Margins):
    """The table walk's own Philox uniforms (csrc rng_words, stream 1 word 0)."""

    def __init__(self, node_ids: Dict[str, int], *, seed: int, offset: int = 0, q_base: int = 0,
                 n_queries: int, n_samples: int):
        super().__init__(n_queries, n_samples)
        self.node_ids = dict(node_ids)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.offset = int(offset)
        self.q_base = int(q_base)

    def uniforms(self, node: str, bq: int, s: int, d: int, shared: bool, q0: int) -> np.ndarray:
        q, ss, dd = np.meshgrid(np.arange(bq) + q0, np.arange(s), np.arange(d), indexing="ij")
        sid = ((self.offset & 0xFF) << 24) | (self.node_ids[node] << 10) | (dd.astype(np.int64) << 2) | 1
        qkey = np.zeros_like(q) if shared else (self.q_base + q + 1)
        c1 = (qkey.astype(np.uint64) & np.uint64(0xFFFFFFFF)) ^ np.uint64((self.seed >> 32) & 0xFFFFFFFF)
        key = (np.uint64(self.seed & 0xFFFFFFFF) + sid.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        a, _ = philox2x32(ss.reshape(-1), c1.reshape(-1), key.reshape(-1))
        return u01(a)

    def categorical(self, node: str, probs: torch.Tensor, shared: bool, q0: int = 0) -> torch.Tensor:
        bq, s, d, c = probs.shape
        u = self.uniforms(node, bq, s, d, shared, q0)
        idx, margin = _choose(probs.reshape(-1, c).numpy(), u)
        self._note(margin, bq, s, d, shared and bq == 1 and self.B > 1, q0)
        return torch.from_numpy(idx.astype(np.int64)).reshape(bq, s, d)


# ---- the engines -------------------------------------------------------------------------------

def _as2d(v: torch.Tensor) -> torch.Tensor:
    v = torch.as_tensor(v).to(F64)
    return v.unsqueeze(-1) if v.dim() == 1 else v


def _batch(evidence: dict, do: dict) -> int:
    for d in (evidence, do):
        if d:
            return int(next(iter(d.values())).shape[0])
    return 1


def _clamp(x: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(x, nan=0.0, posinf=1e6, neginf=-1e6).clamp(min=-1e6, max=1e6)


def _fixed(evidence: dict, do: dict, clamp: bool = False) -> Dict[str, torch.Tensor]:
    vals = {k: _as2d(v) for k, v in (do or {}).items()}
    for k, v in (evidence or {}).items():
        vals[k] = _clamp(_as2d(v)) if clamp else _as2d(v)
    return vals


class TableModel:
    def __init__(self, model):
        self.model = model
        self.cpds = {n: TableCPD(model.cpds[n]) for n in model.topo}

    def parents_of(self, node: str, vals: Dict[str, torch.Tensor]) -> Optional[torch.Tensor]:
        pa = self.model.parents[node]
        return torch.cat([vals[p] for p in pa], dim=-1) if pa else None

    def walk(self, vals_in: Dict[str, torch.Tensor], b: int, s: int, draws, *, shared_roots: bool,
             weigh: List[str] = (), per_query: bool = False):
        """The engines' topological loop: fixed nodes broadcast, evidence in ``weigh`` adds its
        log-prob in topological order, every other node is sampled (``per_query``: one CPD call
        per query, importance_sampling.py:36-52).  Returns (values by node [b, s, D], log-weights)."""
        vals: Dict[str, torch.Tensor] = {}
        lw = torch.zeros(b, s, dtype=F64)
        for node in self.model.topo:
            cpd = self.cpds[node]
            if node in vals_in:
                vals[node] = vals_in[node].unsqueeze(1).expand(b, s, -1)
                if node in weigh:
                    lw = lw + cpd.log_prob(vals[node], self.parents_of(node, vals))
                continue
            par = self.parents_of(node, vals)
            root = par is None
            if root and not per_query:                   # sample(None, S) -> [1, S, D], broadcast
                v = cpd.sample(node, None, 1, s, draws, shared_roots)
                vals[node] = v.expand(b, s, -1)
            elif per_query and b > 1:
                vals[node] = torch.cat([cpd.sample(node, None if root else par[i:i + 1], 1, s, draws, False, q0=i)
                                        for i in range(b)], dim=0)
            else:
                vals[node] = cpd.sample(node, par, b, s, draws, False)
        return vals, lw


def mcm(tm: TableModel, target, evidence, do, n, draws):
    """monte_carlo_marginalization.py:18-92 -> (pdf, samples)"""
    evidence, do = evidence or {}, do or {}
    b = _batch(evidence, do)
    vals = _fixed(evidence, do)
    cpd = tm.cpds[target]
    if target in do:
        return torch.ones(b, n, dtype=F64), vals[target].unsqueeze(1).expand(b, n, -1)
    pa = tm.model.parents[target]
    if all(p in vals for p in pa):
        par = torch.cat([vals[p].unsqueeze(1).expand(b, n, -1) for p in pa], dim=-1) if pa else None
        if target in vals:
            xs = vals[target].unsqueeze(1).expand(b, n, -1)
        elif par is None:
            xs = cpd.sample(target, None, 1, n, draws, True)
        else:
            xs = cpd.sample(target, par, b, n, draws, False)
        lp = cpd.log_prob(xs, None if par is None else par[:xs.shape[0]])
        return torch.exp(lp), xs
    out, _ = tm.walk(vals, b, n, draws, shared_roots=True)
    xs = out[target]
    return torch.exp(cpd.log_prob(xs, tm.parents_of(target, out))), xs


def _normalize(lw: torch.Tensor, normalize: bool, eps: float) -> torch.Tensor:
    if normalize:
        return torch.softmax(lw, dim=1)
    lw = lw - lw.max(dim=-1, keepdim=True).values
    return torch.exp(lw).clamp_min(eps)


def lw(tm: TableModel, target, evidence, do, n, draws, normalize: bool = True, eps: float = 1e-12):
    """likelihood_weighting.py:24-82 -> (weights, samples, log-weights)"""
    evidence, do = evidence or {}, do or {}
    b = _batch(evidence, do)
    vals = _fixed(evidence, do, clamp=True)
    out, logw = tm.walk(vals, b, n, draws, shared_roots=True, weigh=list(evidence))
    return _normalize(logw, normalize, eps), out[target], logw


def importance(tm: TableModel, target, evidence, do, n, draws, draws_fallback=None, ess_threshold: float = 0.1):
    """importance_sampling.py:24-93 -> (weights, samples, ess, fallback)"""
    evidence, do = evidence or {}, do or {}
    b = _batch(evidence, do)
    vals = _fixed(evidence, do)
    out, logw = tm.walk(vals, b, n, draws, shared_roots=False, weigh=list(evidence), per_query=True)
    w = torch.softmax(logw, dim=1)
    ess = 1.0 / (w ** 2).sum(dim=1)
    if bool((ess < max(1.0, ess_threshold * float(n))).any()):
        w2, xs2, _ = lw(tm, target, evidence, do, n, draws_fallback)
        return w2, xs2, ess, True
    return w, out[target], ess, False


def ancestral(tm: TableModel, target, evidence, do, n, draws):
    """sampling/ancestral.py:13-65 -> samples of the target, or a dict of every node's"""
    evidence, do = evidence or {}, do or {}
    b = _batch(evidence, do)
    out, _ = tm.walk(_fixed(evidence, do), b, n, draws, shared_roots=True)
    return out[target] if target else out


def categorical_exact(tm: TableModel, target, evidence, do, n, draws):
    """categorical_exact.py:89-128 (fallback: likelihood weighting) -> (pdf, samples, exact?)"""
    evidence, do = evidence or {}, do or {}
    b = _batch(evidence, do)
    vals = _fixed(evidence, do, clamp=True)
    if target in vals:
        return torch.ones(b, 1, dtype=F64), vals[target].unsqueeze(1).expand(b, 1, -1), True
    pa = tm.model.parents[target]
    cpd = tm.cpds[target]
    if not all(p in vals for p in pa) or cpd.D != 1:
        w, xs, _ = lw(tm, target, evidence, do, n, draws)
        return w, xs, False
    par = torch.cat([vals[p].unsqueeze(1) for p in pa], dim=-1) if pa else None
    probs = cpd.probs(par, b if pa else 1, 1)[:, 0, 0, :].expand(b, -1)
    return probs, cpd.sample_values[0].view(1, -1, 1).expand(b, -1, 1), True
