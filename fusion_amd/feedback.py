"""Pseudo-relevance feedback (PRF): the stage between a first search and the second.

The first few documents of a query's own top-k list move the query towards them (Rocchio): q' = alpha * q + sum_r coef[q, r] * d_r.
The arithmetic is fixed -- one float32 rounding per product and per add, the documents added in list order -- and runs in two kernels
(csrc/feedback.hip: ops.sparse_feedback for weighted sparse queries over a forward index, ops.dense_feedback for embeddings).  This
module holds what sits around them:

  coefficients   a planes.RankedTopk -> (fb_ids, fb_len, coef): which documents feed back, and with what weight;
  gather_rows    the multi-shard route: every rank packs the feedback rows it owns, ONE all_reduce(MAX) per tensor leaves every slot its
                 owner's row on every rank, and the rows become a batch-local index of Q * F pseudo-documents the same kernels read --
                 so the expanded queries do not depend on the number of shards.

distributed.ShardedSparseIndex / ShardedDenseIndex .feedback and .search_feedback are built from these.
"""
from __future__ import annotations

import torch

from .distributed import reduce_max
from .planes import RankedTopk

WEIGHTINGS = ("uniform", "score")


def coefficients(topk: RankedTopk, fb_docs: int, beta: float = 1.0, weighting: str = "uniform"):
    """The feedback lists of a first-pass result: -> (fb_ids [Q, F] int64, fb_len [Q] int32, coef [Q, F] float32) with F = min(fb_docs, k),
    fb_ids the lists' first F ids and fb_len = min(fb_docs, lens).
      'uniform'  coef = beta / fb_len for every listed slot;
      'score'    coef[q, r] = beta * s_r / (sum of the listed scores of q); where that sum is not a positive finite number (an empty
                 list, scores that cancel, an infinity) the row falls back to uniform.
    Computed in float64 and rounded to float32 once; slots past fb_len get 0.0 (the kernels never read them)."""
    if not isinstance(topk, RankedTopk):
        raise TypeError(f"coefficients: expected a RankedTopk, got {type(topk).__name__}")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"coefficients(weighting): expected one of {WEIGHTINGS}, got {weighting!r}")
    fb_docs = int(fb_docs)
    if fb_docs < 0:
        raise ValueError(f"coefficients: fb_docs = {fb_docs} must not be negative")
    F = min(fb_docs, topk.k)
    fb_ids = topk.ids[:, :F]
    fb_len = torch.clamp(topk.lens, min=0, max=F).to(torch.int32)
    listed = torch.arange(F, device=fb_ids.device)[None, :] < fb_len[:, None]
    n = fb_len.to(torch.float64).clamp(min=1.0)[:, None]
    coef = (float(beta) / n).expand(-1, F)
    if weighting == "score":
        s = torch.where(listed, topk.scores[:, :F].to(torch.float64), torch.zeros((), dtype=torch.float64, device=fb_ids.device))
        total = s.sum(1, keepdim=True)
        ok = torch.isfinite(total) & (total > 0)
        coef = torch.where(ok, float(beta) * s / torch.where(ok, total, torch.ones_like(total)), coef)
    coef = torch.where(listed, coef, torch.zeros((), dtype=torch.float64, device=fb_ids.device)).to(torch.float32)
    return fb_ids, fb_len, coef.contiguous()


def pack_rows(source, fb_ids: torch.Tensor, id_base: int = 0, group=None):
    """The rows of the feedback slots, padded and combined over the group's shards.  source: this rank's ops.SparseForward, or its [N, dim]
    float32 row matrix; its document d has the global id id_base + d.
      sparse -> (terms [Q, F, L] int32, fill -1; weights [Q, F, L] float32, fill -inf), L = the longest row of the batch on any rank
                (one all_reduce(MAX) and one host read);
      dense  -> rows [Q, F, dim] float32, fill -inf.
    A slot no rank owns (a negative id, padding) stays all fill."""
    dense = isinstance(source, torch.Tensor)
    Q, F = int(fb_ids.shape[0]), int(fb_ids.shape[1])
    dev = fb_ids.device
    N = int(source.shape[0]) if dense else int(source.N)
    d = fb_ids - int(id_base)
    own = (fb_ids >= int(id_base)) & (d >= 0) & (d < N)
    d = torch.where(own, d, torch.zeros_like(d))
    if dense:
        rows = torch.full((Q, F, int(source.shape[1])), float("-inf"), dtype=torch.float32, device=dev)
        if N > 0 and own.any():
            rows[own] = source[d[own]]
        return reduce_max(rows, group, skip_empty=True)
    if N > 0:
        start = source.foff[d]
        lens = torch.where(own, source.foff[d + 1] - start, torch.zeros_like(d))
    else:
        start, lens = torch.zeros_like(d), torch.zeros_like(d)
    L = reduce_max(lens.max().reshape(1) if lens.numel() else torch.zeros(1, dtype=torch.int64, device=dev), group)
    L = int(L.item())
    terms = torch.full((Q, F, L), -1, dtype=torch.int32, device=dev)
    weights = torch.full((Q, F, L), float("-inf"), dtype=torch.float32, device=dev)
    at = torch.arange(L, device=dev)
    live = at[None, None, :] < lens[:, :, None]
    if L > 0 and live.any():
        src = (start[:, :, None] + at[None, None, :])[live]
        terms[live] = source.rows[src, 0]
        weights[live] = source.rows[src, 1].view(torch.float32)
    return reduce_max(terms, group, skip_empty=True), reduce_max(weights, group, skip_empty=True)


def gather_rows(source, fb_ids: torch.Tensor, id_base: int = 0, group=None):
    """The multi-shard route of feedback: pack_rows, then the packed rows as a batch-local index of Q * F pseudo-documents -- slot (q, r)
    is pseudo-document q * F + r -- which ops.sparse_feedback / ops.dense_feedback read with id_base = 0.
    -> (ops.SparseForward over the source's vocabulary | rows [Q * F, dim], fb_ids' [Q, F] int64): fb_ids' holds q * F + r where the slot
    was filled by some rank and -1 elsewhere, so the kernels' slot rules skip what nobody owns.  (A document without postings fills
    nothing and is skipped: it would add nothing.)"""
    from . import ops
    Q, F = int(fb_ids.shape[0]), int(fb_ids.shape[1])
    pseudo = torch.arange(Q * F, dtype=torch.int64, device=fb_ids.device).view(Q, F)
    none = torch.full_like(pseudo, -1)
    if isinstance(source, torch.Tensor):
        rows = pack_rows(source, fb_ids, id_base, group)
        filled = ~torch.isneginf(rows[:, :, 0]) if rows.shape[2] > 0 else torch.zeros((Q, F), dtype=torch.bool, device=fb_ids.device)
        return rows.view(Q * F, rows.shape[2]), torch.where(filled, pseudo, none)
    terms, weights = pack_rows(source, fb_ids, id_base, group)
    live = terms >= 0
    lens = live.sum(2)
    foff = torch.zeros(Q * F + 1, dtype=torch.int64, device=fb_ids.device)
    foff[1:] = torch.cumsum(lens.reshape(-1), 0)
    rows = torch.empty((int(foff[-1].item()) if Q * F else 0, 2), dtype=torch.int32, device=fb_ids.device)
    rows[:, 0] = terms[live]
    rows[:, 1] = weights[live].view(torch.int32)
    return ops.SparseForward(foff, rows, Q * F, source.V), torch.where(lens > 0, pseudo, none)
