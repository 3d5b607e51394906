"""Pseudo-relevance feedback (PRF): the stage between a first search and the second.

The first few documents of a query's own top-k list move the query towards them (Rocchio): q' = alpha * q + sum_r coef[q, r] * d_r.
The arithmetic is fixed -- one float32 rounding per product and per add, the documents added in list order -- and runs in two kernels
(csrc/feedback.hip: ops.sparse_feedback for weighted sparse queries over a forward index, ops.dense_feedback for embeddings).  This
module holds what sits around them:

  coefficients   a planes.RankedTopk -> (fb_ids, fb_len, coef): which documents feed back, and with what weight;
  gather_rows    the multi-shard route: every rank packs the feedback rows it owns, ONE all_reduce(MAX) per tensor leaves every slot its
                 owner's row on every rank, and the rows become a batch-local index of Q * F pseudo-documents the same kernels read --
                 so the expanded queries do not depend on the number of shards.

  pack_lexical_rows / lexical_rows   the same for the lexical models (BM25 / TF-IDF, float64, csrc/feedback_lexical.hip): a shard's rows
                 as (term id in the COMMON term space, the model's weight of the term in the document), combined by MAX, then the rows
                 the rows kernel (ops.lexical_feedback_rows) reads.

distributed.ShardedSparseIndex / ShardedDenseIndex / ShardedLexicalIndex .feedback and .search_feedback are built from these.
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


def global_term_table(model):
    """The common term space of the shards of one lexical corpus: a word's id is its position in the merged statistics' df table
    (LexicalStats.merge: Counter.update keeps first-occurrence order, so the table is the same on every rank, and for contiguous shards
    it is the whole corpus's own term numbering); a model built without `stats` is the whole corpus: its own vocabulary.
    -> (words: list, the word of every global id; local_to_global [V_local] int64 host array)."""
    import numpy as np
    if model.global_stats is None:
        return list(model.vocab), np.arange(len(model.vocab), dtype=np.int64)
    words = list(model.global_stats.df)
    gid = {w: i for i, w in enumerate(words)}
    return words, np.fromiter((gid[w] for w in model.vocab), dtype=np.int64, count=len(model.vocab))


def global_to_local(local_to_global, n_global: int):
    """[n_global] int64 host array: the local term id of every global id, -1 where the shard lacks the word."""
    import numpy as np
    g2l = np.full(int(n_global), -1, dtype=np.int64)
    g2l[local_to_global] = np.arange(len(local_to_global), dtype=np.int64)
    return g2l


def lexical_row_lengths(model, fb_ids: torch.Tensor) -> torch.Tensor:
    """[Q, F] int64: the number of distinct terms of the document each feedback slot names, 0 for a slot this shard does not own
    (model: a retrievers.bm25 model with a forward index; its document d has the global id model.id_base + d)."""
    fwd, N = model.forward, int(model.corpus_size)
    d = fb_ids - int(model.id_base)
    own = (fb_ids >= int(model.id_base)) & (d >= 0) & (d < N)
    d = torch.where(own, d, torch.zeros_like(d))
    if N == 0:
        return torch.zeros_like(d)
    return torch.where(own, fwd.foff[d + 1] - fwd.foff[d], torch.zeros_like(d))


def pack_lexical_rows(model, local_to_global: torch.Tensor, fb_ids: torch.Tensor, width: int | None = None):
    """ONE shard's part of the feedback rows, a pure function of the shard: -> (terms [Q, F, L] int32 in the common term space, fill -1;
    values [Q, F, L] float64, fill -inf).  values = the model's weight of the term in the document, exactly what its posting walk adds:
    pval[p] (BM25 / AtireBM25) or float64(ptf[p]) * idf[t] (TF-IDF; one rounding).  local_to_global: [V_local] int64 device tensor
    (global_term_table).  width L: at least the longest row of the batch on ANY shard (None: this shard's own longest).  A slot's owner
    fills it, every other shard leaves the fill: an element-wise MAX over the shards (torch.maximum, or one all_reduce(MAX) per tensor)
    gives every slot its owner's row."""
    mode = model.lexical_mode()
    if mode is None:
        raise ValueError("pack_lexical_rows: this model's scoring has no range walk (no postings, or BM25.USE_POSTING_VALUES = False)")
    if model.forward is None:
        model.build_forward()
    fwd = model.forward
    vals, idf = model.lexical_tables()
    Q, F = int(fb_ids.shape[0]), int(fb_ids.shape[1])
    dev = fb_ids.device
    lens = lexical_row_lengths(model, fb_ids)
    own_L = int(lens.max().item()) if lens.numel() else 0
    L = own_L if width is None else int(width)
    if L < own_L:
        raise ValueError(f"pack_lexical_rows: width = {L} is below this shard's longest row ({own_L})")
    terms = torch.full((Q, F, L), -1, dtype=torch.int32, device=dev)
    values = torch.full((Q, F, L), float("-inf"), dtype=torch.float64, device=dev)
    at = torch.arange(L, device=dev)
    live = at[None, None, :] < lens[:, :, None]
    if L > 0 and bool(live.any()):
        d = (fb_ids - int(model.id_base)).clamp(min=0, max=max(int(model.corpus_size) - 1, 0))
        src = (fwd.foff[d][:, :, None] + at[None, None, :])[live]
        t_local = fwd.fterm[src].long()
        p = fwd.fpos[src].long()
        terms[live] = local_to_global[t_local].to(torch.int32)
        values[live] = vals[p] if mode == "pv" else vals[p].to(torch.float64) * idf[t_local]
        # a row in ascending GLOBAL term order (the local order is the shard's own numbering), the fill last: the same pack from any sharding
        order = torch.argsort(torch.where(live, terms, torch.iinfo(torch.int32).max), dim=2, stable=True)
        terms, values = torch.gather(terms, 2, order), torch.gather(values, 2, order)
    return terms, values


def lexical_rows(terms: torch.Tensor, values: torch.Tensor):
    """The combined pack as the rows ops.lexical_feedback_rows reads: slot (q, r) is pseudo-document q * F + r.
    -> (foff [Q * F + 1] int64, fterm int32, fval float64, fb_ids' [Q, F] int64): fb_ids' holds q * F + r where some shard filled the
    slot and -1 elsewhere, so the kernel's slot rules skip what nobody owns (a document without terms fills nothing: it adds nothing)."""
    Q, F = int(terms.shape[0]), int(terms.shape[1])
    dev = terms.device
    live = terms >= 0
    lens = live.sum(2)
    foff = torch.zeros(Q * F + 1, dtype=torch.int64, device=dev)
    foff[1:] = torch.cumsum(lens.reshape(-1), 0)
    pseudo = torch.arange(Q * F, dtype=torch.int64, device=dev).view(Q, F)
    return foff, terms[live].contiguous(), values[live].contiguous(), torch.where(lens > 0, pseudo, torch.full_like(pseudo, -1))
