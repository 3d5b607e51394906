"""MI355X-native drop-in for the reference's lexical module `src/retrievers/bm25.py` (291 lines): the three retrieval classes --
TFIDF (:33-127), BM25 (:129-161), AtireBM25 (:164-173) -- with the reference's exact arithmetic, and the working form of its driver
(`main`, :176-272; `scripts/run_bm25.sh`): the k1 x b grid search, the evaluation run and the hard-negatives extraction.

The inverted index is built on the host from whitespace tokens (as the reference builds it: the text is pre-processed BEFORE it gets
here, bm25.py:216-220); every (query, document) pair is scored on the device in float64 in the reference's expression and addition order
(csrc/bm25.hip) and ranked by the stable row sort (csrc/sort.hip): scores, lists and therefore every metric are bit-identical to the
Python loops (tests/golden/bm25.json, bm25_family.json -- outputs of the reference itself).

The grid search (`BM25.tune`) is to BM25 what `Aggregator.tune` is to the fusion weights: the index and the queries' postings stay
resident, each of the 187 (k1, b) pairs is one norm pass + one scoring launch + one row sort, and only the ranks of the gold documents
come back -- every metric of bm25.py:223,230 is a function of them.  Past one sort row there is no plane and no sort either: a gold
document's rank is the count of the documents ranked before it, taken on the posting walk (csrc/bm25_count.hip, `gold_ranks`).

Reference defects in the driver, not reproduced (documented in DESIGN.md):
  * bm25.py:235 `scores.pop('recall')` raises KeyError with the Metrics of src/utils/metrics.py (its results are flat), :236
    `DataFrame.append` left pandas in 2.0: the grid loop dies on its first row.  The CSV the loop was meant to write -- one row per
    (k1, b) with the recall columns -- is written here;
  * the k1 = 0 column: with np.float64 parameters (np.arange, :226) a document that lacks a query term scores idf * 0 / 0 = NaN (:154) and
    sorted() is handed NaN keys.  Here a posting-less (term, document) pair adds nothing, i.e. k1 = 0 is the binary model sum(idf).
"""
from __future__ import annotations

import argparse
import itertools
import json
import math
import os
import pickle
import time
from collections import Counter
from os.path import join
from statistics import mean

import numpy as np
import torch

from .. import ops
from ..planes import RankedSystem, RankedTopk


LEXICAL_MIN_ZERO_SHARE = 0.3   # expected share of exact zeros per row from which the ranking sort's zero-compacting instantiation is asked for
SLICE_TABLE_MAX_BYTES = 1 << 30   # the per-index slice-offset table (V x (N / 3,584 + 1) int64) is built only below this size; above it the
                                  # scoring kernel finds every term's slice sub-range by binary search (same bits, no table)
DEVICE_BUDGET_BYTES = 48 << 30    # device memory the planes of one chunk of queries may take (ranked_positions, BM25.tune)


def _cut_widths(n: int, k: int, W: int) -> list[int]:
    """Row widths of the hierarchical top-k cut of an n-wide score row (TFIDF.ranked_positions): each level sorts every W-wide stretch of
    the row and keeps its first min(k, W) entries, so the next row is ceil(n / W) * min(k, W) wide.  With min(k, W) > W / 2 the widths can
    stop falling (and with k >= W nothing is cut), or fall by a few columns a level (k = W - 1 over 8.8 M documents: 157 levels), so a level
    is taken only while it keeps at most three quarters of the row it comes from -- strictly narrower, at most log4/3(n / W) + 2 levels --
    and the last row is sorted whole (sort_rows_desc: chunk-sort + merge for rows of any length).  The last width is the row sorted whole."""
    if n <= 0 or k <= 0 or W <= 0:
        return [max(n, 0)]
    widths, kk = [n], min(k, W)
    while n > W:
        nxt = -(-n // W) * kk
        if 4 * nxt > 3 * n:
            break
        widths.append(nxt)
        n = nxt
    return widths


def expected_zero_share(df: np.ndarray, n_docs: int, query_terms: list[list[int]]) -> float:
    """Mean over the queries of prod over a query's DISTINCT in-vocabulary terms of (1 - df_t / N): the share of documents expected to hold
    none of its terms (terms taken as independent) -- i.e. to score exactly 0.0.  Host arithmetic on the index's df table (one np.unique over
    the batch's (query, term) pairs), no device work."""
    Q = len(query_terms)
    if Q == 0 or n_docs <= 0:
        return 0.0
    lens = np.fromiter((len(t) for t in query_terms), dtype=np.int64, count=Q)
    flat = np.fromiter((x for t in query_terms for x in t), dtype=np.int64, count=int(lens.sum()))
    qid = np.repeat(np.arange(Q, dtype=np.int64), lens)
    keep = flat >= 0
    V = max(int(df.shape[0]), 1)
    pairs = np.unique(qid[keep] * V + flat[keep])                     # distinct (query, term) pairs
    miss = 1.0 - df.astype(np.float64) / float(n_docs)
    with np.errstate(divide="ignore"):
        logs = np.log(miss[pairs % V])                                # (-inf for a term every document holds: that query expects no zeros)
    per_query = np.exp(np.bincount(pairs // V, weights=logs, minlength=Q)) if pairs.size else np.ones(Q)
    per_query = np.nan_to_num(per_query, nan=0.0)
    return float(per_query.mean())


def expansion_words(wq, words: list) -> list[list[tuple]]:
    """(word, weight) per entry of every weighted query, words[t] the word of term id t (None for -1)."""
    off, terms, w = wq.qoff.cpu().tolist(), wq.qterms.cpu().tolist(), wq.qw.cpu().tolist()
    return [[(words[terms[j]] if terms[j] >= 0 else None, w[j]) for j in range(off[q], off[q + 1])] for q in range(len(off) - 1)]


class LexicalStats:
    """The collection statistics a lexical model's idf table and BM25's avgdl are made from: number of documents, document frequency of
    every word, total length in words.  Those of a whole corpus are the sums of its shards' (`merge`), so a shard's model built with the
    merged statistics scores its documents exactly as the model of the whole corpus does."""

    def __init__(self, n_docs: int, df: dict[str, int], total_len: int):
        self.n_docs, self.df, self.total_len = int(n_docs), df, int(total_len)

    @property
    def avgdl(self) -> float:
        """total_len / n_docs on Python ints: correctly rounded, as statistics.mean of the lengths is (bm25.py:138)."""
        return self.total_len / self.n_docs if self.n_docs else 0.0

    @classmethod
    def merge(cls, parts: list["LexicalStats"]) -> "LexicalStats":
        df: Counter = Counter()
        for p in parts:
            df.update(p.df)
        return cls(sum(p.n_docs for p in parts), dict(df), sum(p.total_len for p in parts))

    def __eq__(self, other):
        return isinstance(other, LexicalStats) and (self.n_docs, self.total_len, self.df) == (other.n_docs, other.total_len, other.df)

    def __repr__(self):
        return f"LexicalStats(n_docs={self.n_docs}, words={len(self.df)}, total_len={self.total_len})"


class WeightedQueries:
    """Lexical queries whose entries carry a float64 weight, as the weighted posting walks take them (csrc/bm25_weighted.hip): qoff
    [Q + 1] int64, qterms int32 term ids of ONE model's vocabulary (repetitions and -1 kept), qw float64 one weight per entry.  What
    TFIDF.feedback returns: the original entries at alpha, then the expansion terms.  flags: ops.lexical_feedback's (bit 0: the capacity
    rule skipped feedback slots of some query)."""

    def __init__(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, flags: int = 0):
        if qoff.dtype != torch.int64 or qterms.dtype != torch.int32 or qw.dtype != torch.float64:
            raise TypeError(f"WeightedQueries: expected int64 offsets, int32 terms and float64 weights, got {qoff.dtype} / {qterms.dtype} / {qw.dtype}")
        if qoff.dim() != 1 or qoff.numel() < 1 or qterms.dim() != 1 or tuple(qw.shape) != tuple(qterms.shape):
            raise ValueError("WeightedQueries: qoff [Q + 1], and qterms and qw with one entry each per query entry expected")
        self.qoff, self.qterms, self.qw, self.flags = qoff, qterms, qw, int(flags)

    @property
    def Q(self) -> int:
        return self.qoff.numel() - 1

    def __repr__(self):
        return f"WeightedQueries(Q={self.Q}, entries={int(self.qoff[-1])}, flags={self.flags})"


FEEDBACK_DEFAULTS = dict(fb_docs=10, fb_terms=10, alpha=1.0, beta=0.5, weighting="uniform")   # the usual RM3 settings; tuned on nothing


class TFIDF:
    """bm25.py:33-127: score(q, d) = sum over q.split(), in order, of tf(t, d) * idf(t), idf = log10((N + 1) / (df + 1)).

    stats (a LexicalStats, default None): the index is one SHARD of a larger corpus -- idf comes from the global document count and the
    global df of each local word (and BM25's avgdl from the global lengths); postings and vocabulary stay local.  id_base: the id of
    document 0 in search_topk's lists.  Without them everything is as the reference has it."""

    CAP = 7168            # candidate slots per query and window of the streamed search_topk (k + CAP: one float64 sort row)
    CHUNK = 64 * 3584     # documents per feed of the streamed search_topk (whole slices of either walk)
    HEAD = 28672          # at most this many leading documents get the exact top-k before the stream starts
    STREAM_QUERIES = 1024 # queries per block of the streamed route

    def __init__(self, corpus: list[str], device="cuda", slice_table_max_bytes: int | None = None, stats: LexicalStats | None = None,
                 id_base: int = 0):
        self.corpus = corpus
        self.corpus_size = len(corpus)
        self.device = torch.device(device)
        self.global_stats, self.id_base = stats, int(id_base)
        self._idf_n = self.corpus_size if stats is None else stats.n_docs      # the N of the idf formulas
        self.last_path, self.last_overflow = None, 0                           # of the last search_topk: 'stream' | 'plane', windows redone exactly
        toks = [doc.split() for doc in corpus]
        self.vocab: dict[str, int] = {}
        for t in toks:
            for w in t:
                self.vocab.setdefault(w, len(self.vocab))
        V = len(self.vocab)
        # tf postings (bm25.py:58-65) and df (bm25.py:67-75)
        tid = np.fromiter((self.vocab[w] for t in toks for w in t), dtype=np.int64, count=sum(len(t) for t in toks))
        did = np.repeat(np.arange(len(toks), dtype=np.int64), [len(t) for t in toks])
        key = tid * max(self.corpus_size, 1) + did
        uniq, tf = np.unique(key, return_counts=True)
        pt, pd = uniq // max(self.corpus_size, 1), uniq % max(self.corpus_size, 1)
        self.df_host = np.bincount(pt, minlength=V).astype(np.int64)
        idf_df = self.df_host if stats is None else np.array([stats.df[w] for w in self.vocab], dtype=np.int64)   # (vocab: insertion order = term id)
        self.idf_host = np.array([self._compute_idf(int(x)) for x in idf_df], dtype=np.float64)
        self.doc_len_host = np.array([len(t) for t in toks], dtype=np.int32)
        toff = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(self.df_host, out=toff[1:])
        self._toff_host, self._pdoc_host, self._ptf_host = toff, pd.astype(np.int32), tf.astype(np.int32)
        d = self.device
        self.toff = torch.from_numpy(toff).to(d)
        self.pdoc = torch.from_numpy(self._pdoc_host).to(d)
        self.ptf = torch.from_numpy(self._ptf_host).to(d)
        self.idf = torch.from_numpy(self.idf_host).to(d)
        self.doc_len = torch.from_numpy(self.doc_len_host).to(d)
        # where every term's postings cross the document slices one workgroup scores: per index, like the idf table -- when it fits the cap
        # (a multi-million-term vocabulary over millions of documents would make it tens of GB; without it the kernel binary-searches)
        self.slice_off = None
        if self.device.type == "cuda" and V > 0:
            cap = SLICE_TABLE_MAX_BYTES if slice_table_max_bytes is None else slice_table_max_bytes
            if ops.bm25_slice_table_bytes(V, self.corpus_size) < cap:
                self.slice_off = ops.bm25_slice_offsets(self.toff, self.pdoc, self.corpus_size)
        self._qcache = None
        self.zero_share_estimate = 0.0   # of the last list of queries (set by _query_csr)

    def __repr__(self):
        return f"{self.__class__.__name__}".lower()                       # bm25.py:45-46: names the pickles of save_indexes

    def get_vocab(self):
        """bm25.py:48-50: the vocabulary in alphabetical order."""
        return sorted(self.vocab)

    def _compute_idf(self, df: int) -> float:
        return math.log10((self._idf_n + 1) / (df + 1))                   # bm25.py:86-88

    def stats(self) -> LexicalStats:
        """This index's own collection statistics (of a shard: the shard's)."""
        return LexicalStats(self.corpus_size, {w: int(self.df_host[t]) for w, t in self.vocab.items()}, int(self.doc_len_host.sum(dtype=np.int64)))

    # -- what the range / filter walks of csrc/bm25_stream.hip take (ops._lexical_source) --
    def lexical_mode(self) -> str | None:
        """'tfidf' | 'pv' | None: the walk this model's scores() launches, if it has a range form."""
        return "tfidf" if self.pdoc.numel() else None

    def lexical_tables(self):
        """(per-posting values, idf table or None) of that walk."""
        return self.ptf, self.idf

    # -- queries -> CSR of term ids (kept for the last list of queries: the grid search scores the same queries 187 times) --
    def _query_csr(self, queries: list[str]):
        if self._qcache is not None and (self._qcache[0] is queries or self._qcache[0] == queries):
            return self._qcache[1], self._qcache[2]
        qt = [[self.vocab.get(w, -1) for w in q.split()] for q in queries]   # query terms are NOT de-duplicated (bm25.py:112,152)
        qoff = np.zeros(len(qt) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in qt], out=qoff[1:])
        flat = np.array([t for x in qt for t in x] or [0], dtype=np.int32)
        qoff_d, flat_d = torch.from_numpy(qoff).to(self.device), torch.from_numpy(flat).to(self.device)
        self._qcache = (list(queries), qoff_d, flat_d)   # (a copy: a caller that edits its list in place gets a fresh CSR)
        self.zero_share_estimate = expected_zero_share(self.df_host, self.corpus_size, qt)
        return qoff_d, flat_d

    def scores(self, queries: list[str], want_f32: bool = False):
        """[Q, N] float64 plane (want_f32: and its float32 rounding, from the same launch)."""
        qoff, flat = self._query_csr(queries)
        return ops.tfidf_scores(self.toff, self.pdoc, self.ptf, self.idf, qoff, flat, len(queries), self.corpus_size,
                                slice_off=self.slice_off, want_f32=want_f32)

    def search_device(self, queries: list[str], ids: np.ndarray | None = None) -> RankedSystem:
        sc64, sc32 = self.scores(queries, want_f32=True)
        Q, N = sc64.shape
        stats4 = None   # mean | std | min | max of every list's float32 scores: by-products of the ranking sort (rows that fit one workgroup)
        if N <= ops.sort_max_n(torch.float64) and Q > 0:
            stats4 = torch.empty((4, Q), dtype=torch.float32, device=self.device)
        # ranks from the float64 scores, ties -> ascending index.  lexical: when the batch's rows are expected to be mostly exact zeros (documents
        # that share no term with the query) the sort's zero-compacting instantiation orders only the non-zero keys -- a host-side ESTIMATE picks
        # the instantiation (it costs rows without zeros 1-7 %), the kernel decides row by row from the actual count; same outputs either way
        order, _, rank = ops.sort_rows_desc(sc64, want_keys=False, want_rank=True, stats_out=stats4, lexical=self.zero_share_estimate >= LEXICAL_MIN_ZERO_SHARE)
        lens = torch.full((Q,), N, dtype=torch.int32, device=self.device)
        # float32 plane for the normalisations (torch.tensor(scores, dtype=float32), hybrid.py:255), written by the scoring kernel from
        # the accumulators it holds (no conversion pass); the float64 scores stay for the 'none' passthrough, which keeps BM25's Python
        # floats (hybrid.py:280).  Rounding is monotone: the float32 scores are in descending order along the float64 ranking too.
        return RankedSystem(scores=sc32, order=order, rank=rank, lens=lens,
                            ids=np.arange(N, dtype=np.int64) if ids is None else ids, full=True,
                            scores64=sc64, score_sorted=True, stats4=stats4)

    def ranked_positions(self, queries: list[str], top_k: int, budget_bytes: int = DEVICE_BUDGET_BYTES) -> np.ndarray:
        """[Q, min(top_k, N)] corpus positions of the first top_k entries of every ranked list (what the driver keeps of search_all,
        bm25.py:248-249), the queries taken in chunks whose planes fit the budget.  A corpus that fits one workgroup's row (28,672 documents)
        is ranked in full (search_device); a longer one -- mMARCO's 8.8 M passages -- is CUT, not ranked (_top_positions)."""
        N, k = self.corpus_size, max(0, min(top_k, self.corpus_size))
        out = np.empty((len(queries), k), dtype=np.int64)
        if k == 0:
            return out
        W = ops.sort_max_n(torch.float64)
        step = self._query_step(k, budget_bytes)
        for lo in range(0, len(queries), step):
            chunk = queries[lo:lo + step]
            if N <= W:
                out[lo:lo + len(chunk)] = self.search_device(chunk).order[:, :k].cpu().numpy()
            else:
                out[lo:lo + len(chunk)] = self._top_positions(self.scores(chunk), k).cpu().numpy()
        return out

    def search_topk(self, queries: list[str], k: int, budget_bytes: int = DEVICE_BUDGET_BYTES, streaming: bool | None = None) -> RankedTopk:
        """The first min(k, N) entries of every ranked list as device-resident top-k lists (what Aggregator.fuse_topk takes): the positions
        ranked_positions computes, kept on the device, with their float64 scores gathered next to them (scores64; `scores` holds the
        float32 roundings the normalisations take, hybrid.py:255).  ids = id_base + corpus position.

        streaming: False -- the plane route: the whole [q, N] float64 plane per chunk of queries, ranked (N within one sort row) or cut
        (_top_positions).  True -- the streamed route wherever it can run (_streams): an exact top-k of the first head_docs(k) documents,
        then the posting walk with the threshold filter as its epilogue over the rest (no plane; ops.TopkStream64 folds the candidates a
        few times) -- the same lists, bit for bit.  None: stream when N exceeds one float64 sort row.  BM25.USE_POSTING_VALUES = False
        (the per-posting expression has no range walk) keeps the plane route.  last_path / last_overflow record what ran."""
        sc64, ids = self._topk_device(queries, k, budget_bytes, streaming)
        lens = torch.full((len(queries),), ids.shape[1], dtype=torch.int32, device=self.device)
        return RankedTopk(ids=ids, scores=sc64.to(torch.float32), lens=lens, scores64=sc64)

    def head_docs(self, k: int) -> int:
        """Leading documents that get the exact top-k: 8,192 at k = 1000, rounded up to whole slices of the walk (10,752 / 14,336)."""
        return ops.stream_head_docs(k, ops.lexical_slice_docs(self.lexical_mode()), self.HEAD)

    def _streams(self, k: int) -> bool:
        if self.lexical_mode() is None or k <= 0:
            return False
        return ops.stream_fits(k, self.CAP, self.head_docs(k), self.corpus_size, torch.float64)

    def _topk_device(self, queries: list[str], k: int, budget_bytes: int = DEVICE_BUDGET_BYTES, streaming: bool | None = None, mark=None):
        """search_topk's ([Q, k] float64 scores, [Q, k] int64 ids); mark(name): optional instrumentation hook, called after every launch
        group ('shard_lexical': a plane, 'shard_lexical_filter': a filter walk, 'shard_topk_stream': top-k work)."""
        mark = mark or (lambda name: None)
        N, k = self.corpus_size, max(0, min(k, self.corpus_size))
        Q = len(queries)
        if streaming is None:
            streaming = N > ops.sort_max_n(torch.float64)
        self.last_overflow = 0
        if streaming and Q > 0 and self._streams(k):
            self.last_path = "stream"
            return self._stream_topk(queries, k, mark)
        self.last_path = "plane"
        pos = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        sc64 = torch.empty((Q, k), dtype=torch.float64, device=self.device)
        W = ops.sort_max_n(torch.float64)
        step = self._query_step(k, budget_bytes)
        for lo in range(0, Q if k else 0, step):
            chunk = queries[lo:lo + step]
            if N <= W:
                rs = self.search_device(chunk); mark("shard_lexical")
                p, plane = rs.order[:, :k].long(), rs.scores64
            else:
                plane = self.scores(chunk); mark("shard_lexical")
                p = self._top_positions(plane, k)
            pos[lo:lo + len(chunk)] = p
            sc64[lo:lo + len(chunk)] = torch.gather(plane, 1, p); mark("shard_topk_exact")
        return sc64, (pos + self.id_base if self.id_base else pos)

    def _stream_topk(self, queries: list[str], k: int, mark):
        Q = len(queries)
        head, chunk = self.head_docs(k), ops.stream_chunk(self.CHUNK, ops.lexical_slice_docs(self.lexical_mode()))
        ids = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        sc64 = torch.empty((Q, k), dtype=torch.float64, device=self.device)
        for lo in range(0, Q, self.STREAM_QUERIES):
            block = queries[lo:lo + self.STREAM_QUERIES]
            qoff, flat = self._query_csr(block)
            src = ops._lexical_source(self, qoff, flat, self.id_base)
            sc64[lo:lo + len(block)], ids[lo:lo + len(block)], redone = ops.stream_search(
                src, k, head, chunk, self.CAP, "shard_lexical", mark, ops.TopkStream64, top_positions=self._top_positions)
            self.last_overflow += redone
        return sc64, ids

    # -- pseudo-relevance feedback (csrc/feedback_lexical.hip) and the weighted walks (csrc/bm25_weighted.hip); DESIGN.md, 'Lexical feedback' --
    def feedback(self, queries: list[str], topk: RankedTopk, *, fb_docs: int = 10, fb_terms: int = 10, alpha: float = 1.0, beta: float = 0.5,
                 weighting: str = "uniform") -> WeightedQueries:
        """The queries expanded from the first fb_docs documents of their own lists (topk: the RankedTopk of a first search_topk; ids
        outside this index are skipped).  w[t] = sum over the feedback documents, in list order, of coef * (the model's weight of t in the
        document: exactly what the walk adds for that posting), coef from feedback.coefficients(topk, fb_docs, 1.0, weighting); of the terms
        with w > 0 that the query does not hold, the fb_terms of largest w (ties: the lower term id) are appended at beta * (w / w_max),
        the original entries keep their order at weight alpha.  The defaults are the usual RM3 settings, tuned on nothing.  The forward
        index is built on first use.  ValueError for a model without a range walk (BM25.USE_POSTING_VALUES = False)."""
        from .. import feedback as fb
        mode, vals, idf = self._walk_tables("feedback")
        if self.forward is None:
            self.build_forward()
        qoff, flat = self._query_csr(queries)
        fb_ids, fb_len, coef = fb.coefficients(topk, fb_docs, 1.0, weighting)
        if fb_ids.shape[0] != len(queries):
            raise ValueError(f"feedback: {len(queries)} queries but lists for {fb_ids.shape[0]}")
        return WeightedQueries(*ops.lexical_feedback(mode, self.forward, vals, idf, qoff, flat, fb_ids, fb_len, coef, alpha, beta, fb_terms,
                                                     id_base=self.id_base))

    def _weighted_plane(self, wq: WeightedQueries, lo: int, hi: int, tables) -> torch.Tensor:
        mode, vals, idf = tables
        return ops.lexical_scores_range(mode, self.toff, self.pdoc, vals, idf, wq.qoff[lo:hi + 1], wq.qterms, hi - lo, self.corpus_size, 0,
                                        self.corpus_size, slice_off=self.slice_off, qw=wq.qw)

    def scores_weighted(self, wq: WeightedQueries, budget_bytes: int = DEVICE_BUDGET_BYTES) -> torch.Tensor:
        """[Q, N] float64: score(q', d) = the chain, in entry order, of acc + qw[j] * (the walk's term of entry j's posting in d) -- the
        weighted range walk over [0, N), the queries in chunks whose planes fit budget_bytes.  With every weight 1.0: scores()'s plane."""
        tables = self._walk_tables("scores_weighted")
        Q, N = wq.Q, self.corpus_size
        step = min(32768, max(1, int(budget_bytes // (8 * ops.round_up(max(N, 1), 64)))))
        if Q <= step:
            return self._weighted_plane(wq, 0, Q, tables)
        out = ops.alloc_plane(Q, N, torch.float64, self.device)
        for lo in range(0, Q, step):
            hi = min(Q, lo + step)
            out[lo:hi] = self._weighted_plane(wq, lo, hi, tables)
        return out

    def search_device_weighted(self, wq: WeightedQueries, ids: np.ndarray | None = None) -> RankedSystem:
        """search_device for weighted queries: the full ranking of the weighted plane (float32 plane = its rounding), ties -> ascending index."""
        sc64 = self.scores_weighted(wq)
        Q, N = sc64.shape
        sc32 = ops.as_plane(sc64.to(torch.float32))
        stats4 = None
        if N <= ops.sort_max_n(torch.float64) and Q > 0:
            stats4 = torch.empty((4, Q), dtype=torch.float32, device=self.device)
        order, _, rank = ops.sort_rows_desc(sc64, want_keys=False, want_rank=True, stats_out=stats4)
        lens = torch.full((Q,), N, dtype=torch.int32, device=self.device)
        return RankedSystem(scores=sc32, order=order, rank=rank, lens=lens, ids=np.arange(N, dtype=np.int64) if ids is None else ids,
                            full=True, scores64=sc64, score_sorted=True, stats4=stats4)

    def search_topk_weighted(self, wq: WeightedQueries, k: int, budget_bytes: int = DEVICE_BUDGET_BYTES, streaming: bool | None = None,
                             mark=None) -> RankedTopk:
        """search_topk for weighted queries, by the same two routes (streaming as there: the weighted filter walk under ops.TopkStream64,
        or the weighted plane ranked / cut) -- the same lists either way; last_path / last_overflow record what ran."""
        tables = self._walk_tables("search_topk_weighted")
        mark = mark or (lambda name: None)
        N, k, Q = self.corpus_size, max(0, min(k, self.corpus_size)), wq.Q
        if streaming is None:
            streaming = N > ops.sort_max_n(torch.float64)
        self.last_overflow = 0
        ids = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        sc64 = torch.empty((Q, k), dtype=torch.float64, device=self.device)
        if streaming and Q > 0 and self._streams(k):
            self.last_path = "stream"
            head, chunk = self.head_docs(k), ops.stream_chunk(self.CHUNK, ops.lexical_slice_docs(tables[0]))
            for lo in range(0, Q, self.STREAM_QUERIES):
                hi = min(Q, lo + self.STREAM_QUERIES)
                src = ops._lexical_source(self, wq.qoff[lo:hi + 1], wq.qterms, self.id_base, qw=wq.qw)
                sc64[lo:hi], ids[lo:hi], redone = ops.stream_search(src, k, head, chunk, self.CAP, "shard_lexical", mark, ops.TopkStream64,
                                                                    top_positions=self._top_positions)
                self.last_overflow += redone
        else:
            self.last_path = "plane"
            W = ops.sort_max_n(torch.float64)
            step = min(32768, self._query_step(k, budget_bytes))
            for lo in range(0, Q if k else 0, step):
                hi = min(Q, lo + step)
                plane = self._weighted_plane(wq, lo, hi, tables); mark("shard_lexical")
                if N <= W:
                    p = ops.sort_rows_desc(plane, want_keys=False)[0][:, :k].long()
                else:
                    p = self._top_positions(plane, k)
                sc64[lo:hi] = torch.gather(plane, 1, p); mark("shard_topk_exact")
                ids[lo:hi] = p + self.id_base
        lens = torch.full((Q,), k, dtype=torch.int32, device=self.device)
        return RankedTopk(ids=ids, scores=sc64.to(torch.float32), lens=lens, scores64=sc64)

    def search_feedback(self, queries: list[str], k: int, budget_bytes: int = DEVICE_BUDGET_BYTES, streaming: bool | None = None,
                        **feedback) -> RankedTopk:
        """search_topk -> feedback -> search_topk_weighted: the top-k lists of the expanded queries (**feedback: feedback()'s keywords).
        alpha = 1, fb_terms = 0 gives search_topk's lists."""
        first = self.search_topk(queries, k, budget_bytes, streaming)
        return self.search_topk_weighted(self.feedback(queries, first, **feedback), k, budget_bytes, streaming)

    def expansion_words(self, wq: WeightedQueries) -> list[list[tuple]]:
        """Host lists, one per query, of (word, weight) for every entry of the weighted queries in order (None for an entry outside the
        vocabulary): what feedback() made of the queries, for inspection."""
        return expansion_words(wq, list(self.vocab))

    # -- ranks of listed documents as counts on the posting walk (csrc/bm25_count.hip): no plane, no list, no sort --
    def _walk_tables(self, what: str):
        mode = self.lexical_mode()
        if mode is None:
            raise ValueError(f"{what}: this model's scoring has no range walk (no postings, or BM25.USE_POSTING_VALUES = False)")
        return (mode,) + tuple(self.lexical_tables())

    def _gold_plane(self, what: str, t, Q: int, dtype) -> torch.Tensor:
        t = torch.as_tensor(t).to(device=self.device, dtype=dtype)
        if t.dim() != 2 or t.shape[0] != Q or t.shape[1] < 1:
            raise ValueError(f"{what}: expected a [Q = {Q}, G >= 1] array, got {tuple(t.shape)}")
        return t.contiguous()

    forward = None               # the ops.ForwardIndex build_forward() made, or None
    # doc_scores(route=None) follows the faster route at the measured shape (Q = 1024, G = 3,000, 200,000 documents): the inverted one, 1.58 ms
    # against the forward route's 3.20 ms (profiles/r21_forward_pairs.json; DESIGN.md, 'Forward index') -- the forward route is opt-in here
    PREFER_FORWARD = False

    def build_forward(self):
        """Build and keep the document-major view of the postings (ops.forward_index, fpos kept: 16 bytes per document + 8 per posting)
        that doc_scores' forward route searches.  The per-posting values are read through fpos, so update_params needs nothing redone."""
        self.forward = ops.forward_index(self.toff, self.pdoc, self.corpus_size)
        return self.forward

    def doc_scores(self, queries: list[str], positions, route: str | None = None) -> torch.Tensor:
        """[Q, G] float64: scores()[q, positions[q, g]] bit for bit, without the plane (one binary search per query term and listed
        document).  A position of -1 -- not a document of this index -- gives -inf.  route: 'inverted' searches the term's posting list,
        'forward' the document's row of the forward index (a ValueError without one); None: ops.sparse_dot_pairs' rule, with
        PREFER_FORWARD."""
        forward = ops._pair_route("doc_scores", route, self.forward, None, self.PREFER_FORWARD)
        Q = len(queries)
        pos = self._gold_plane("doc_scores(positions)", positions, Q, torch.int64)
        if Q == 0:
            return torch.empty(tuple(pos.shape), dtype=torch.float64, device=self.device)
        if not (isinstance(positions, torch.Tensor) and positions.is_cuda):      # (a device tensor is not read back: the kernel gives -inf)
            host = np.asarray(torch.as_tensor(positions))
            if host.size and (host.max() >= self.corpus_size or host.min() < -1):
                raise ValueError(f"doc_scores: positions must be -1 or in [0, {self.corpus_size})")
        mode, vals, idf = self._walk_tables("doc_scores")
        qoff, flat = self._query_csr(queries)
        if forward:
            return ops.lexical_doc_scores_fwd(mode, self.toff, self.pdoc, vals, idf, self.forward, qoff, flat, Q, self.corpus_size,
                                              pos.to(torch.int32), block=self.STREAM_QUERIES)
        return ops.lexical_doc_scores(mode, self.toff, self.pdoc, vals, idf, qoff, flat, Q, self.corpus_size, pos.to(torch.int32),
                                      block=self.STREAM_QUERIES)

    def count_before(self, queries: list[str], gold_scores, gold_ids, counts: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, G] int64: for every (query, gold) the number of THIS index's documents that the stable descending float64 ranking puts
        before the gold -- gold_scores [Q, G] float64, gold_ids [Q, G] int64 GLOBAL ids (this index's documents are id_base ..
        id_base + N - 1; the gold may be another shard's; an id < 0 is skipped: its count stays).  A document precedes a gold when its score
        ranks before the gold's, or equals it and its id is lower.  counts: added to and returned (shards, or several indexes, sum into
        one tensor); default zeros.  One count launch per CHUNK documents (int32 on the device), summed in int64."""
        Q = len(queries)
        gs = self._gold_plane("count_before(gold_scores)", gold_scores, Q, torch.float64)
        gi = self._gold_plane("count_before(gold_ids)", gold_ids, Q, torch.int64)
        if gs.shape != gi.shape:
            raise ValueError("count_before: gold_scores and gold_ids differ in shape")
        if counts is None:
            counts = torch.zeros(tuple(gs.shape), dtype=torch.int64, device=self.device)
        elif counts.dtype != torch.int64 or counts.shape != gs.shape or counts.device != gs.device:
            raise ValueError("count_before: counts must be an int64 tensor of the golds' shape on the model's device")
        N = self.corpus_size
        if Q == 0 or N == 0:
            return counts
        mode, vals, idf = self._walk_tables("count_before")
        qoff, flat = self._query_csr(queries)
        chunk = ops.stream_chunk(self.CHUNK, ops.lexical_slice_docs(mode))
        part = torch.empty(tuple(gs.shape), dtype=torch.int32, device=self.device)
        for lo in range(0, N, chunk):
            part.zero_()
            ops.lexical_count(mode, self.toff, self.pdoc, vals, idf, qoff, flat, Q, N, lo, min(N, lo + chunk), self.id_base, gs, gi, part,
                              slice_off=self.slice_off, block=self.STREAM_QUERIES)
            counts += part
        return counts

    def gold_ranks(self, queries: list[str], positions) -> torch.Tensor:
        """[Q, G] int64: the rank of document positions[q, g] in query q's full ranking (search_device(queries).rank gathered at the
        positions), for a corpus of any size: the document's score, then the count of the documents ranked before it.  -1 -> -1."""
        Q = len(queries)
        pos = self._gold_plane("gold_ranks(positions)", positions, Q, torch.int64)
        sc = self.doc_scores(queries, pos)
        ids = torch.where(pos >= 0, pos + self.id_base, -1)
        return torch.where(pos >= 0, self.count_before(queries, sc, ids), -1)

    def _query_step(self, k: int, budget_bytes: int) -> int:
        """Queries per chunk whose planes fit budget_bytes (at least one)."""
        N, W = self.corpus_size, ops.sort_max_n(torch.float64)
        per_pair = 20 if N <= W else 12 + 24 * min(1.0, (k + 1) / W)      # planes alive per (query, document)
        if N > W and _cut_widths(N, k, W)[-1] > W:
            per_pair = 36                                                  # a row longer than W sorted whole: scores, order, 24 B of merge workspace
        return max(1, int(budget_bytes // max(1, int(per_pair * ops.round_up(max(N, 1), 64)))))

    @staticmethod
    def _top_positions(sc: torch.Tensor, k: int) -> torch.Tensor:
        """[q, k] int64 corpus positions of the first k entries of the stable descending ranking of every row of the float64 plane sc [q, n]
        (0 < k <= n), by the hierarchical cut (_cut_widths): every W-wide stretch of the row is sorted on its own, its first k entries survive,
        and the survivors (stretch by stretch, so that the stable sort breaks ties by ascending index as the full sort does) go round again
        while that narrows the row; the last row is sorted whole.  The same first k entries as the full ranking, without its cross-chunk
        ranking of all n documents."""
        W = ops.sort_max_n(torch.float64)
        q = sc.shape[0]
        widths = _cut_widths(sc.shape[1], k, W)
        ids = None                                                         # [q, n] corpus positions of the surviving columns (None: the identity)
        for n, nxt in zip(widths[:-1], widths[1:]):
            C = -(-n // W)
            pad = C * W - n                                                # pad to whole stretches: -inf never survives a real score, NaN sorts first as everywhere
            if pad:
                sc = torch.cat([sc, torch.full((q, pad), float("-inf"), dtype=sc.dtype, device=sc.device)], 1)
                if ids is not None:
                    ids = torch.cat([ids, torch.full((q, pad), -1, dtype=torch.int64, device=sc.device)], 1)
            order, keys, _ = ops.sort_rows_desc(ops.as_plane(sc.reshape(q * C, W).contiguous()), want_keys=True)
            kk = min(k, W)
            base = (torch.arange(C, device=sc.device) * W).repeat(q)[:, None]
            cols = (order[:, :kk].long() + base).reshape(q, C * kk)       # columns of this level's row, stretch by stretch: corpus order is kept
            if cols.shape[1] != nxt or 4 * nxt > 3 * n:                    # (_cut_widths takes only levels that narrow the row)
                raise RuntimeError(f"ranked_positions: the cut of a {n}-wide row to {cols.shape[1]} columns makes no progress (planned {nxt})")
            ids = cols if ids is None else torch.gather(ids, 1, cols)
            sc = keys[:, :kk].reshape(q, C * kk)
        order, _, _ = ops.sort_rows_desc(ops.as_plane(sc.contiguous()), want_keys=False)
        order = order[:, :k].long()
        return order if ids is None else torch.gather(ids, 1, order)

    def search_all(self, queries: list[str], top_k: int) -> list:
        """bm25.py:90-106: every document scored (zero scores included), stable sort desc, [:top_k]."""
        t0 = time.perf_counter()
        out = self.search_device(queries).to_lists(top_k)
        if queries:
            print(f"Avg. latency (ms/quey): {((time.perf_counter() - t0) / len(queries)) * 1000}")   # (sic) bm25.py:97
        return out

    def search(self, query: str, top_k: int) -> list:
        return self.search_device([query]).to_lists(top_k)[0]

    def save_indexes(self, output_dir: str, dataset: str) -> None:
        """bm25.py:117-126: the four indexes as pickles, in the reference's own Python types (vocab: set, tf: {word: {doc: count}},
        df: Counter, idf: {word: float}) so that whatever read the reference's files reads these."""
        words = list(self.vocab)
        tf = {}
        for w, t in self.vocab.items():
            lo, hi = int(self._toff_host[t]), int(self._toff_host[t + 1])
            tf[w] = dict(zip(self._pdoc_host[lo:hi].tolist(), self._ptf_host[lo:hi].tolist()))
        payload = {"vocab": set(words), "tf": tf, "df": Counter({w: int(self.df_host[t]) for w, t in self.vocab.items()}),
                   "idf": {w: float(self.idf_host[t]) for w, t in self.vocab.items()}}
        for name, obj in payload.items():
            with open(join(output_dir, f"{self.__repr__()}_{name}_{dataset}.pkl"), "wb") as f:
                pickle.dump(obj, f)


class BM25(TFIDF):
    """bm25.py:129-161: score(q, d) = sum of idf * tf (k1 + 1) / (tf + k1 (1 - b + b |d| / avgdl)), idf = log10((N - df + .5) / (df + .5))
    (can be <= 0), avgdl = statistics.mean(doc_len)."""

    USE_POSTING_VALUES = True   # False: the per-posting expression (fz_bm25_scores_f64_f32): A/B runs and tests of the two forms
    last_tune_path = None       # of the last tune: 'count' | 'plane'

    def __init__(self, corpus: list[str], k1: float, b: float, device="cuda", slice_table_max_bytes: int | None = None,
                 stats: LexicalStats | None = None, id_base: int = 0):
        self.k1, self.b = k1, b
        self._pval = None
        super().__init__(corpus, device=device, slice_table_max_bytes=slice_table_max_bytes, stats=stats, id_base=id_base)
        if stats is None:
            self.avgdl = float(mean(self.doc_len_host.tolist())) if self.corpus_size else 0.0   # bm25.py:138
        else:
            self.avgdl = stats.avgdl                                       # the whole corpus's mean length, the same correctly rounded quotient
        self._norm_key, self._norm = None, None

    def _compute_idf(self, df: int) -> float:
        N = self._idf_n
        return math.log10((N - df + 0.5) / (df + 0.5))                    # bm25.py:145-147

    def lexical_mode(self) -> str | None:
        """'pv' with the posting-value table (the default); USE_POSTING_VALUES = False -- the per-posting expression -- has no range walk."""
        return "pv" if self.USE_POSTING_VALUES and self.pdoc.numel() else None

    def lexical_tables(self):
        self._doc_norm()                                                  # (re)tabulates the posting values for the current (k1, b)
        return self._pval, None

    def update_params(self, k1: float, b: float) -> None:
        self.k1, self.b = k1, b

    def _doc_norm(self) -> torch.Tensor:
        key = (float(self.k1), float(self.b))
        if self._norm_key != key:
            self._norm = ops.bm25_doc_norms(self.doc_len, self.avgdl, self.k1, self.b)
            # every posting's whole term idf * (tf (k1 + 1)) / (tf + norm_d) for this (k1, b): per index, like the idf table -- the scoring
            # walk then only adds (no float64 division per (query, posting)); same bits
            self._pval = ops.bm25_posting_values(self.toff, self.pdoc, self.ptf, self.idf, self._norm, self.k1) if self.pdoc.numel() else None
            self._norm_key = key
        return self._norm

    def scores(self, queries: list[str], want_f32: bool = False):
        """[Q, N] float64 plane (want_f32: and its float32 rounding, from the same launch); query terms are NOT de-duplicated (bm25.py:152)."""
        qoff, flat = self._query_csr(queries)
        norm = self._doc_norm()
        return ops.bm25_scores(self.toff, self.pdoc, self.ptf, self.idf, self.doc_len, self.avgdl, self.k1, self.b,
                               qoff, flat, len(queries), self.corpus_size,
                               doc_norm=norm, slice_off=self.slice_off, want_f32=want_f32, pval=self._pval if self.USE_POSTING_VALUES else None)

    # -- the grid search of bm25.py:221-237 on the device --------------------------------------------------------------
    def tune(self, queries: list[str], labels: list[list], ids=None, k1_range=None, b_range=None,
             recall_at_k=(10, 100, 200, 500, 1000), top_k: int = 1000, budget_bytes: int = DEVICE_BUDGET_BYTES,
             counting: bool | None = None) -> list[dict]:
        """For every (k1, b) of itertools.product(k1_range, b_range) (bm25.py:226-228): what
        `update_params(k1, b); search_all(queries, top_k); Metrics(recall_at_k).compute_all_metrics(labels, ids of the lists)` reports
        (bm25.py:231-234) -- recall@k for the given cut-offs and r-precision -- as one dict per pair: {'k1', 'b', 'recall@10', ...}.
        The lists are never built: one scoring launch + one row sort per pair, and the ranks of the gold documents (a gold document at
        rank >= top_k was cut from the list: never retrieved) come back.  ids: corpus position -> dataset id (idx2id, bm25.py:214).
        The queries are taken in chunks whose planes fit budget_bytes, as in ranked_positions; a corpus longer than one sort row is cut to
        its first top_k entries (_top_positions), not ranked in full: a gold document's rank is its place in that head, or none.

        counting: True -- no plane either, wherever the model has a range walk: a gold document's rank is the COUNT of the documents ranked
        before it (gold_ranks: its score by binary search, then the posting walk with the counting epilogue, csrc/bm25_count.hip), the same
        ranks and therefore the same dicts.  False -- the plane route above.  None: count when N exceeds one float64 sort row, i.e. exactly
        where the plane route cuts instead of ranking.  USE_POSTING_VALUES = False (no range walk) keeps the plane route.  last_tune_path
        records 'count' or 'plane'.  The model's own k1 / b are restored afterwards."""
        from ..utils.metrics import metrics_from_gold_ranks
        k1_range = np.arange(0., 8.5, 0.5) if k1_range is None else k1_range      # bm25.py:226
        b_range = np.arange(0., 1.1, 0.1) if b_range is None else b_range        # bm25.py:227
        combos = list(itertools.product(*[k1_range, b_range]))
        Q, N = len(queries), self.corpus_size
        ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids)
        id2pos = {c: j for j, c in enumerate(ids.tolist())}
        gold_pos = [[id2pos.get(g, -1) for g in dict.fromkeys(gl)] for gl in labels]
        G = max(1, max((len(g) for g in gold_pos), default=1))
        gp = np.full((Q, G), -1, dtype=np.int64)
        for q, gl in enumerate(gold_pos):
            gp[q, :len(gl)] = gl
        gp_dev = torch.from_numpy(np.maximum(gp, 0)).to(self.device)
        n_gold = np.array([len(gl) for gl in labels], dtype=np.int64)             # the reference divides by len(ground_truths)
        k = max(0, min(top_k, N))
        list_len = np.full(Q, k, dtype=np.int64)
        INF = np.iinfo(np.int64).max
        W = ops.sort_max_n(torch.float64)
        step = self._query_step(k, budget_bytes)
        keep = (self.k1, self.b)
        got = torch.full((len(combos), Q, G), k, dtype=torch.int64, device=self.device)   # k: not among the first top_k
        if counting is None:
            counting = N > W
        counting = bool(counting) and self.lexical_mode() is not None and Q > 0 and k > 0
        self.last_tune_path = "count" if counting else "plane"
        gp_pos = torch.from_numpy(gp).to(self.device) if counting else None              # -1: not in the corpus
        for w, (k1, b) in enumerate(combos):
            self.update_params(k1, b)
            if counting:
                got[w] = self.gold_ranks(queries, gp_pos)                  # full ranks: one at or past k was cut from the list (below)
                continue
            for lo in range(0, Q if k else 0, step):
                chunk = queries[lo:lo + step]
                g = gp_dev[lo:lo + len(chunk)]
                sc = self.scores(chunk)
                if N <= W:
                    _, _, rank = ops.sort_rows_desc(sc, want_keys=False, want_rank=True, lexical=self.zero_share_estimate >= LEXICAL_MIN_ZERO_SHARE)
                    got[w, lo:lo + len(chunk)] = torch.gather(rank, 1, g).long()
                    continue
                pos = self._top_positions(sc, k)                           # [q, k]: a corpus position appears at most once per row
                at = torch.arange(k, dtype=torch.int64, device=self.device)
                for j in range(G):
                    got[w, lo:lo + len(chunk), j] = torch.where(pos == g[:, j:j + 1], at, k).min(1).values
        self.update_params(*keep)
        ranks = got.cpu().numpy()
        ranks = np.where((gp[None] >= 0) & (ranks < k), ranks, INF)
        names = [f"recall@{k}" for k in recall_at_k] + ["r-precision"]
        perfs = metrics_from_gold_ranks(ranks, n_gold, list_len, recall_ks=list(recall_at_k), only=names)
        return [{"k1": float(k1), "b": float(b), **p} for (k1, b), p in zip(combos, perfs)]


class AtireBM25(BM25):
    """bm25.py:164-173 (https://www.cs.otago.ac.nz/homepages/andrew/papers/2014-2.pdf): BM25's score with TFIDF's idf."""

    def _compute_idf(self, df: int) -> float:
        return math.log10((self._idf_n + 1) / (df + 1))


# ---------------------------------------------------------------------------------------------------
# driver (bm25.py:176-291) -- same flags; data comes from local files because there is no network
# ---------------------------------------------------------------------------------------------------
def preprocess(texts: list[str], lemmatize: bool = True) -> list[str]:
    """src/data/preprocessor.py:15-76 (spaCy fr_core_news_md: punctuation, numbers and stop words dropped, lemmas, lower case).  The model is
    third-party and not installed offline: asking for it without it is an error, not a silent no-op."""
    try:
        import spacy
        nlp = spacy.load("fr_core_news_md")
    except Exception as ex:   # noqa: BLE001
        raise RuntimeError("--do_preprocessing needs spaCy with fr_core_news_md (requirements.txt:25-26 of the reference); it is not installed here. "
                           "Pass text that is already pre-processed (lower-cased lemmas, whitespace-separated) and drop the flag.") from ex
    import re
    out = []
    for doc in nlp.pipe(texts):
        toks = [(t.lemma_ if lemmatize else t.text) for t in doc
                if not t.is_punct and not (t.is_digit or t.like_num or re.match(r".*\d+", t.text)) and not t.is_stop]
        out.append(" ".join(toks).lower())
    return out


def load_data(args):
    """bm25.py:181-212 offline: `--data_dir` with corpus.jsonl ({'id', 'article'}) + questions_<split>.jsonl ({'id', 'question',
    'article_ids'}) -- the split main() picks: train for the negatives, validation for the grid search, test otherwise -- or
    `--synthetic N,Q`.  -> corpus {id: text}, qids, queries, pos_pids."""
    if getattr(args, "synthetic", None):
        n, q = (int(x) for x in args.synthetic.split(","))
        rng = np.random.default_rng(0)
        vocab = np.array([f"mot{i}" for i in range(5000)])
        p = 1.0 / np.arange(1, 5001); p /= p.sum()
        corpus = {int(i + 1): " ".join(rng.choice(vocab, size=int(rng.integers(20, 200)), p=p)) for i in range(n)}
        queries = [" ".join(rng.choice(vocab, size=int(rng.integers(4, 16)), p=p)) for _ in range(q)]
        pos = [sorted(rng.choice(np.arange(1, n + 1), size=int(rng.integers(1, 5)), replace=False).tolist()) for _ in range(q)]
        return corpus, list(range(q)), queries, pos
    d = args.data_dir
    if not d or not os.path.isdir(d):
        raise FileNotFoundError("no network: pass --data_dir with corpus.jsonl + questions_<split>.jsonl, or --synthetic N,Q")
    corpus = {}
    with open(join(d, "corpus.jsonl")) as f:
        for line in f:
            r = json.loads(line); corpus[r["id"]] = r["article"]
    if args.dataset == "lleqa":
        split = "train" if args.do_negatives_extraction else ("validation" if args.do_hyperparameter_tuning else "test")   # bm25.py:189
    else:
        split = "train" if args.do_negatives_extraction else "dev_small"                                                  # bm25.py:199
    qids, queries, pos = [], [], []
    with open(join(d, f"questions_{split}.jsonl")) as f:
        for i, line in enumerate(f):
            r = json.loads(line); qids.append(r.get("id", i)); queries.append(r["question"]); pos.append(r["article_ids"])
    return corpus, qids, queries, pos


def main(args):
    import pandas as pd
    from ..utils.metrics import Metrics
    os.makedirs(args.output_dir, exist_ok=True)
    print("Loading documents and queries...")
    corpus, qids, queries, pos_pids = load_data(args)
    documents = list(corpus.values())
    ids = np.array(list(corpus.keys()))                                   # idx2id (bm25.py:214)
    if args.do_preprocessing:
        print("Preprocessing documents and queries (lemmatizing=True)...")
        documents, queries = preprocess(documents), preprocess(queries)

    if args.do_hyperparameter_tuning:
        print("Starting hyperparameter tuning...")
        retriever = BM25(corpus=documents, k1=0., b=0.)
        rows = retriever.tune(queries, pos_pids, ids=ids)                  # bm25.py:221-237, all 187 pairs
        grid_df = pd.DataFrame(rows)
        grid_df.to_csv(join(args.output_dir, "bm25_tuning_results.csv"), sep=",", float_format="%.5f", index=False)
        heat = grid_df.pivot_table(values="recall@100", index="k1", columns="b")[::-1] * 100    # bm25.py:240
        try:   # bm25.py:241-242 draws it with seaborn; matplotlib alone gives the same annotated heat map
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            fig, ax = plt.subplots(figsize=(8, 9))
            ax.imshow(heat.values, cmap="YlOrBr", vmin=40, vmax=60, aspect="auto")
            ax.set_xticks(range(len(heat.columns))); ax.set_xticklabels([f"{c:.1f}" for c in heat.columns]); ax.set_xlabel("b")
            ax.set_yticks(range(len(heat.index))); ax.set_yticklabels([f"{r:.1f}" for r in heat.index]); ax.set_ylabel("k1")
            for (i, j), v in np.ndenumerate(heat.values):
                ax.text(j, i, f"{v:.1f}", ha="center", va="center", fontsize=7)
            fig.savefig(join(args.output_dir, "bm25_tuning_heatmap.pdf"))
            plt.close(fig)
        except Exception as ex:   # noqa: BLE001  (a plot is not worth a failed sweep)
            print(f"(no heat map: {type(ex).__name__}: {ex})")
        print("Done.")
        return rows

    print("Initializing the BM25 retriever model...")
    retriever = BM25(corpus=documents, k1=args.k1, b=args.b)
    print("Running BM25 model on queries...")
    out = {}
    ranked_lists = [ids[row].tolist() for row in retriever.ranked_positions(queries, top_k=1000)]   # search_all(queries, top_k=1000) -> idx2id (bm25.py:248-249)
    if args.do_evaluation:
        print("Computing the retrieval scores...")
        evaluator = Metrics(recall_at_k=[5, 10, 20, 50, 100, 200, 500, 1000], map_at_k=[10, 100], mrr_at_k=[10, 100], ndcg_at_k=[10, 100])
        out = evaluator.compute_all_metrics(all_ground_truths=pos_pids, all_results=ranked_lists)
        with open(join(args.output_dir, f"performance_bm25_{args.dataset}_dev.json"), "w") as f:   # (the reference names it _dev whatever the split)
            json.dump(out, f, indent=2)
    if args.do_negatives_extraction:
        print(f"Extracting top-{args.num_negatives} negatives for each question...")
        results = dict()
        for q_id, truths_i, preds_i in zip(qids, pos_pids, ranked_lists):
            truths = set(truths_i)
            results[q_id] = [y for y in preds_i if y not in truths][:args.num_negatives]
        results = dict(sorted(results.items()))
        with open(join(args.output_dir, "negatives_bm25.json"), "w") as f:
            json.dump(results, f, indent=2)
    retriever.save_indexes(output_dir=args.output_dir, dataset=args.dataset)
    print("Done.")
    return out


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset", type=str, help="Dataset to use.", choices=["lleqa"] + [f"mmarco-{x}" for x in (
        "ar", "de", "en", "es", "fr", "hi", "id", "it", "ja", "nl", "pt", "ru", "vi", "zh")], default="lleqa")
    parser.add_argument("--do_preprocessing", action="store_true", default=False)
    parser.add_argument("--k1", type=float, default=1.5)
    parser.add_argument("--b", type=float, default=0.75)
    parser.add_argument("--do_evaluation", action="store_true", default=False)
    parser.add_argument("--do_negatives_extraction", action="store_true", default=False)
    parser.add_argument("--num_negatives", type=int, default=10)
    parser.add_argument("--do_hyperparameter_tuning", action="store_true", default=False)
    parser.add_argument("--output_dir", type=str)
    # offline additions (no HF hub / ir_datasets): local data or synthetic LLeQA-shaped data
    parser.add_argument("--data_dir", type=str, default=os.environ.get("LLEQA_DIR"))
    parser.add_argument("--synthetic", type=str, default=None, help="N,Q: synthetic corpus/queries of that size")
    return parser


if __name__ == "__main__":
    a, _ = build_parser().parse_known_args()   # unknown flags ignored, as bm25.py:290
    main(a)
