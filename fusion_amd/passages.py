"""Long documents as PASSAGES: window splitting, and the step from passage-level lists to document-level lists (MaxP).

Every neural system here encodes at most 512 tokens of a document; a longer one is split into passages, the passages are indexed and
searched like any corpus (distributed.Sharded*Index return planes.RankedTopk over PASSAGE ids), and a document gets the score of its
best passage.  PassageGroups holds the passage -> document table on the device and offers the two steps that were missing between the
passage lists and Aggregator.fuse_topk / complete_topk / tune_topk / evaluate_topk over DOCUMENT ids:

  collapse     a passage top-k list -> the document list (ops.lists_collapse: one workgroup per query, no reduction, no sort);
  pair_scores  the exact MaxP score of candidate documents: expand to passages (ops.group_expand), score them with any passage pair
               scorer, take each document's maximum (ops.group_max) -- the scorer complete_topk asks a passage index for.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .planes import RankedTopk


def split_passages(texts, words: int, stride: int | None = None):
    """Split every text into windows of `words` whitespace words (str.split(): the unit BM25 uses) that start every `stride` words
    (default: stride = words, no overlap).  A window at start s is emitted iff s == 0 or s + (words - stride) < n_words: no window
    consists only of overlap the previous one already covers, and every document yields at least one passage (an empty text: one empty
    passage).  -> (passages: list[str], poff: int64 [len(texts) + 1]); document d owns passages poff[d] .. poff[d + 1] - 1."""
    words = int(words)
    stride = words if stride is None else int(stride)
    if words < 1:
        raise ValueError(f"split_passages: words = {words} must be at least 1")
    if stride < 1 or stride > words:
        raise ValueError(f"split_passages: stride = {stride} must be in [1, words = {words}] (a larger stride would skip words)")
    overlap = words - stride
    passages, poff = [], [0]
    for text in texts:
        toks = text.split()
        n = len(toks)
        s = 0
        while s == 0 or s + overlap < n:
            passages.append(" ".join(toks[s:s + words]))
            s += stride
        poff.append(len(passages))
    return passages, np.asarray(poff, dtype=np.int64)


class PassageGroups:
    """The passage -> document table of a split corpus, on the device.  poff [D + 1] int64 (CSR: document d owns passages
    poff[d] .. poff[d + 1] - 1); passage p has the global id p + id_base, document d the global id d + doc_id_base.  poff is
    non-decreasing, so is the table group_of [P] int32 -- ascending passage id is ascending document id, which makes list order the tie
    rule of every search here, (score desc, id asc), on the document level too."""

    BUDGET = 256 << 20      # pair_scores: bytes of expanded passage ids (Q x ldp x 8) per block of candidate slots

    def __init__(self, poff, id_base: int = 0, doc_id_base: int = 0, device="cuda"):
        poff = np.asarray(poff.cpu() if isinstance(poff, torch.Tensor) else poff)
        if poff.dtype != np.int64:
            raise TypeError(f"PassageGroups: poff must be int64, got {poff.dtype}")
        if poff.ndim != 1 or poff.size < 1:
            raise ValueError(f"PassageGroups: poff must be a [D + 1] vector, got shape {poff.shape}")
        if poff[0] != 0:
            raise ValueError(f"PassageGroups: poff must start at 0, got {int(poff[0])}")
        counts = np.diff(poff)
        if (counts < 0).any():
            raise ValueError("PassageGroups: poff must be non-decreasing")
        self.D, self.P = int(poff.size - 1), int(poff[-1])
        if self.D >= 2 ** 31 or self.P >= 2 ** 31:
            raise ValueError(f"PassageGroups: {self.D} documents / {self.P} passages do not fit the int32 group table")
        self.id_base, self.doc_id_base = int(id_base), int(doc_id_base)
        self.pmax = int(counts.max()) if self.D else 0
        self.poff_host = poff
        self.poff = torch.from_numpy(poff).to(device)
        self.group_of = torch.from_numpy(np.repeat(np.arange(self.D, dtype=np.int32), counts)).to(device)

    def collapse(self, topk: RankedTopk, k: int | None = None):
        """A passage-level RankedTopk (in (score desc, id asc) order, as the searches return it) -> (the document-level RankedTopk,
        best_passage [Q, k] int64): every document once, at the rank and with the score bits (scores64 included) of its best passage,
        whose id is best_passage; padding is (-1, -inf) and -1.  k cuts the lists to their first k documents and clamps lens.
        ValueError for a passage id outside the table, a list that is not ranked, and a list wider than ops.lists_max_entries()."""
        if not isinstance(topk, RankedTopk):
            raise TypeError(f"PassageGroups.collapse: expected a RankedTopk, got {type(topk).__name__}")
        ids, sc, sc64, best, lens = ops.lists_collapse(topk.ids, topk.scores, topk.lens, self.group_of, id_base=self.id_base,
                                                       doc_id_base=self.doc_id_base, scores64=topk.scores64)
        n = ids.shape[1]
        if k is not None:
            if int(k) < 1:
                raise ValueError(f"PassageGroups.collapse: k = {k} must be at least 1")
            if int(k) < n:
                k = int(k)
                ids, sc, best, lens = ids[:, :k], sc[:, :k], best[:, :k], torch.clamp(lens, max=k)
                sc64 = sc64[:, :k] if sc64 is not None else None
        return RankedTopk(ids=ids, scores=sc, lens=lens, scores64=sc64), best

    def pair_scores(self, passage_scorer, doc_ids: torch.Tensor, lens: torch.Tensor | None = None):
        """The exact MaxP score of candidate documents.  doc_ids [Q, W] int64, lens [Q] int32 or None; passage_scorer(ids [Q, W'] int64,
        lens [Q] int32) -> [Q, W'] float32 or float64 scores of the batch's queries against those PASSAGE ids (a closure over any
        Sharded*Index.pair_scores).  -> (scores [Q, W], best [Q, W] int64): the maximum over the document's passages with the winning
        passage's own bits, and that passage's id (the lowest among equals); (-inf, -1) for a padded slot, an unknown id and a document
        without passages.
        The candidates are expanded to ldp = min(W * pmax, P) passage slots per query.  The scorer is a closure over the WHOLE batch of
        queries, so where Q * ldp * 8 bytes would exceed BUDGET the work is cut into blocks of candidate SLOTS (every block: all
        queries, some columns of doc_ids), never into blocks of queries."""
        ops._dev(doc_ids, torch.int64, "PassageGroups.pair_scores(doc_ids)")
        if doc_ids.dim() != 2:
            raise ValueError(f"PassageGroups.pair_scores: doc_ids must be [Q, W], got {tuple(doc_ids.shape)}")
        Q, W = int(doc_ids.shape[0]), int(doc_ids.shape[1])
        dev = doc_ids.device
        if lens is None:
            lens = torch.full((Q,), W, dtype=torch.int32, device=dev)
        if Q == 0 or W == 0:
            return ops.alloc_plane(Q, W, torch.float32, dev), ops.alloc_plane(Q, W, torch.int64, dev)
        per_slot = max(self.pmax, 1)
        block = W if Q * min(W * per_slot, self.P) * 8 <= self.BUDGET else max(1, self.BUDGET // (8 * max(Q, 1) * per_slot))
        out, best = None, None
        for w0 in range(0, W, block):
            w1 = min(W, w0 + block)
            ldp = min((w1 - w0) * self.pmax, self.P)
            blens = torch.clamp(lens - w0, min=0, max=w1 - w0).to(torch.int32)
            pcand, seg, plen = ops.group_expand(doc_ids[:, w0:w1], blens, self.poff, ldp, id_base=self.id_base, doc_id_base=self.doc_id_base)
            P = passage_scorer(pcand, plen) if ldp > 0 else torch.empty((Q, 0), dtype=torch.float32, device=dev)   # no passage at all
            ops.check_pair_plane(P, Q, ldp, "PassageGroups.pair_scores: the passage scorer")
            if out is None:
                out = ops.alloc_plane(Q, W, P.dtype, dev)
                best = ops.alloc_plane(Q, W, torch.int64, dev)
            elif P.dtype != out.dtype:
                raise TypeError(f"PassageGroups.pair_scores: the passage scorer returned {P.dtype} after {out.dtype}")
            ops.group_max(P, pcand, seg, blens, out=out[:, w0:w1], best=best[:, w0:w1])
        return out, best

    def doc_scorer(self, passage_scorer):
        """passage_scorer (see pair_scores) -> a document-level scorer with the signature Aggregator.complete_topk takes in `scorers`:
        f(ids [Q, W] int64, lens [Q] int32) -> [Q, W] MaxP scores."""
        def score(ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
            return self.pair_scores(passage_scorer, ids, lens)[0]
        return score
