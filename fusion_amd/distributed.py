"""Corpus-sharded dense retrieval with ONE collective (BASELINE.json configs[4]: mMARCO-fr, 8.8 M passages).

Reference spec: InformationRetrievalEvaluatorCustom.compute_metrices (src/utils/sentence_transformers.py:314-393):
corpus in chunks, per chunk score -> torch.topk -> heap merge keeping max_k = 1000 per query.  The reference does
this on one GPU, one query at a time (1.2 M launches for mMARCO).  Here:

  * the corpus-embedding matrix is row-sharded over the ranks (one process per GPU, 288 GB HBM each);
  * every rank scores ALL queries against its shard in document chunks: fp32-MFMA GEMM -> per-row top-k
    (csrc/topk.hip) -> merge into the running top-k -- no host round trip;
  * ONE all-gather of the per-shard [Q, k] (score fp32, id int64) lists over RCCL/xGMI (8.2 MB + 8.2 MB per rank at
    Q = 1024, k = 1000: < 1 % of the GEMM time) and an identical local G-way merge on every rank;
  * the query ENCODER is data-parallel over the queries: every rank runs the transformer on its 1/G of the batch and the
    [Q, 768] embeddings (3 MB) are all-gathered -- the only other exchange step.
Ties are broken by ascending global document id everywhere, so the result does not depend on the number of shards.
"""
from __future__ import annotations

import torch

from . import ops


def shard_bounds(n: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous, balanced row shards: the first n % world shards get one extra row."""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def world(group=None) -> int:
    """How many ranks the group has; 1 without an initialised process group."""
    import torch.distributed as dist
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def reduce_max(t: torch.Tensor, group=None, skip_empty: bool = False) -> torch.Tensor:
    """The tree's convention for slots a shard does not own: they hold the type's lowest value (-inf in a pair plane), so ONE
    all_reduce(MAX) leaves every slot its owner's value on every rank.  The collective takes the contiguous block, not a padded plane:
    a contiguous t is reduced in place.  skip_empty: no collective for an empty t (feedback.pack_rows; the pair planes reduce even then)."""
    if world(group) > 1 and not (skip_empty and t.numel() == 0):
        import torch.distributed as dist
        t = t.contiguous()
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return t


def reduce_sum(t: torch.Tensor, group=None) -> torch.Tensor:
    """Per-shard counts -> the whole corpus's: one all_reduce(SUM), as reduce_max takes its block."""
    if world(group) > 1:
        import torch.distributed as dist
        t = t.contiguous()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def allgather_rows(local: torch.Tensor, total: int, group=None) -> torch.Tensor:
    """Rows sharded by shard_bounds(total, world, rank) -> the full [total, d] tensor on every rank, in rank order:
    one all-gather of equal-size (zero-padded) blocks."""
    G = world(group)
    if G == 1:
        return local
    import torch.distributed as dist
    per = -(-total // G)
    block = local.new_zeros((per, local.shape[1]))
    block[: local.shape[0]] = local
    out = local.new_empty((G * per, local.shape[1]))
    dist.all_gather_into_tensor(out, block, group=group)
    if total == G * per:
        return out
    return torch.cat([out[r * per: r * per + (hi - lo)] for r in range(G) for lo, hi in [shard_bounds(total, G, r)]])


def allgather_topk(local_scores: torch.Tensor, local_ids: torch.Tensor, group=None, merge_fn=None):
    """local [Q, k] lists (each sorted by score desc, id asc; padding = (-inf, -1)) -> global [Q, k] on every rank.
    merge_fn([G,Q,k] scores, [G,Q,k] ids) -> ([Q,k], [Q,k]); defaults to the HIP merge."""
    if merge_fn is None:
        merge_fn = ops.topk_merge
    G = world(group)
    if G == 1:
        return merge_fn(local_scores.unsqueeze(0).contiguous(), local_ids.unsqueeze(0).contiguous())
    import torch.distributed as dist
    Q, k = local_scores.shape
    gs = torch.empty((G, Q, k), dtype=local_scores.dtype, device=local_scores.device)
    gi = torch.empty((G, Q, k), dtype=local_ids.dtype, device=local_ids.device)
    # concatenated-along-dim-0 output form: accepted by RCCL and gloo alike
    dist.all_gather_into_tensor(gs.view(G * Q, k), local_scores.contiguous(), group=group)
    dist.all_gather_into_tensor(gi.view(G * Q, k), local_ids.contiguous(), group=group)
    return merge_fn(gs, gi)


def rank_order(ids: torch.Tensor, scores: torch.Tensor, row_len: torch.Tensor | None = None) -> torch.Tensor:
    """[Q, k0] int64: the columns of every row in (score desc, id asc) order -- one id sort gives the incoming sequence, the stable
    descending row sort (ops.sort_rows_desc; float32 or float64 scores) does the rest.  row_len [Q] int32: only the first row_len[q]
    columns of row q take part; the rest of its order is -1."""
    key = ids
    if row_len is not None:      # columns past a row's length go last in the sequence, where the sort does not look
        past = torch.arange(ids.shape[1], device=ids.device)[None, :] >= row_len[:, None]
        key = ids.masked_fill(past, torch.iinfo(torch.int64).max)
    by_id = torch.argsort(key, dim=1, stable=True).to(torch.int32)
    order, _, _ = ops.sort_rows_desc(scores, init_order=by_id, row_len=row_len, want_keys=False)
    return order.long()


def rank_pairs(ids: torch.Tensor, scores: torch.Tensor, k: int | None = None, *, row_len: torch.Tensor | None = None, ties: str = "id"):
    """Candidate ids [Q, k0] int64 and their (reduced) pair scores [Q, k0], float32 or float64 -> planes.RankedTopk of the candidates in
    descending score order, cut to the first k: the one place that turns pair scores into lists.  Among equal scores (a NaN ranks first,
    as in every sort here)
      ties="id"    the ascending global id decides, the order of every corpus-scale search here (rank_order);
      ties="list"  the candidates keep their incoming order: the stable row sort alone, no id sort.
    A slot no shard owned (-inf) goes last as (-inf, -1); lens counts the others.  row_len [Q] int32: only the first row_len[q] columns of
    row q take part, and exactly those are owned, whatever they score (Aggregator.complete_topk: a listed id keeps its place in the list).
    float64 scores are ranked as float64 and kept as scores64 (scores = their float32 roundings)."""
    from .planes import RankedTopk
    if ties not in ("id", "list"):
        raise ValueError(f"rank_pairs(ties): expected 'id' or 'list', got {ties!r}")
    Q, k0 = ids.shape
    k = k0 if k is None else max(0, min(int(k), k0))
    wide = scores.dtype == torch.float64
    if Q == 0 or k0 == 0:
        s32 = torch.empty((Q, k), dtype=torch.float32, device=ids.device)
        return RankedTopk(ids=ids[:, :k].clone(), scores=s32, lens=torch.zeros(Q, dtype=torch.int32, device=ids.device),
                          scores64=s32.double() if wide else None)
    if ties == "id":
        order = rank_order(ids, scores, row_len)[:, :k]
    else:                                                    # the incoming sequence is the list itself; cut before the widening to int64
        order = ops.sort_rows_desc(scores, row_len=row_len, want_keys=False)[0][:, :k].long()
    if row_len is None:
        ss = torch.gather(scores, 1, order)                  # the scores' own bits (the sort's key plane canonicalises -0.0 and NaN)
        owned = ss != float("-inf")
    else:                                                    # the order past a row's length is -1
        owned, order = order >= 0, order.clamp(min=0)
        ss = torch.gather(scores, 1, order).masked_fill_(~owned, float("-inf"))
    out_ids = torch.where(owned, torch.gather(ids, 1, order), torch.full_like(order, -1))
    return RankedTopk(ids=out_ids, scores=ss.to(torch.float32), lens=owned.sum(1, dtype=torch.int32), scores64=ss if wide else None)


def _candidates(candidates):
    from .planes import FusedTopk, RankedTopk
    return (candidates.ids, candidates.lens) if isinstance(candidates, (RankedTopk, FusedTopk)) else (candidates, None)


class _PairScores:
    """Exact scores of (query, candidate id) pairs over a sharded corpus, and candidate lists reranked by them.  A subclass supplies
    local_pair_scores(*query, cand_ids, cand_len=None) -> [Q, W] float32 or float64 over its own shard, -inf for a slot it does not own
    (r >= cand_len[q], a negative id, a document of another shard), and its tie rule."""

    TIES = "id"             # rank_pairs' rule among equal scores
    # What an empty candidate batch does.  True: it goes through the scorer and the collective like any other (every rank of the group
    # must then call, empty or not).  False: it returns before both.  Each class keeps what it always did: changing either side would
    # leave a rank of an older caller waiting in the collective.
    EMPTY_REDUCES = True

    def local_pair_scores(self, *args, **kw) -> torch.Tensor:
        """The token and text indexes call theirs local_scores: that name is the one to override there."""
        return self.local_scores(*args, **kw)

    def pair_scores(self, *args, **kw) -> torch.Tensor:
        """pair_scores(*query, cand_ids, cand_len=None): local_pair_scores for the whole corpus -- the shards' planes under ONE
        all_reduce(MAX) over the group (reduce_max)."""
        return reduce_max(self.local_pair_scores(*args, **kw), self.group)

    def rerank(self, *args, k: int | None = None):
        """rerank(*query, candidates, k=None).  candidates: a planes.RankedTopk or FusedTopk (its ids and lens are used) or a [Q, k0]
        int64 id tensor (negative ids = padding) -> RankedTopk of the candidates by their exact scores in descending order, ties by the
        class's rule, cut to the first k (rank_pairs).  lens[q] = the slots some shard owned; the others go last as (-inf, -1).  A score
        of -inf itself -- possible only with non-finite inputs -- is indistinguishable from "owned by no shard" and counts as such."""
        if not args or isinstance(args[-1], int):
            raise TypeError(f"{type(self).__name__}.rerank(*query, candidates, k=None): the candidates go last by position, k by keyword")
        *query, candidates = args
        return self._rerank(query, *_candidates(candidates), k)

    def _rerank(self, query, ids: torch.Tensor, cand_len, k):
        if ids.numel() == 0 and not self.EMPTY_REDUCES:
            return rank_pairs(ids, torch.empty(ids.shape, dtype=torch.float32, device=ids.device), k, ties=self.TIES)
        return rank_pairs(ids, self.pair_scores(*query, ids, cand_len), k, ties=self.TIES)


def _fill_blocks(what: str, blocks, rows: int, device, fill) -> None:
    """Drive an iterator of token-row blocks that together hold exactly `rows` rows: every block is moved to the device as contiguous
    float16 and handed to fill(at, blk), at = the row it starts on.  ValueError, under the caller's name `what`, for more or fewer rows."""
    at = 0
    for blk in blocks:
        blk = blk.to(device=device, dtype=torch.float16).contiguous()
        n = blk.shape[0]
        if at + n > rows:
            raise ValueError(f"{what}: the blocks hold more than Doff[N] = {rows} token rows")
        if n:
            fill(at, blk)
        at += n
    if at != rows:
        raise ValueError(f"{what}: the blocks hold {at} token rows, Doff[N] = {rows}")


class _ShardedIndex:
    """One rank's shard of a corpus + the chunked score -> top-k search over it; a subclass supplies its constants and the scoring source of its
    shard for a set of queries (_source: what ops.TopkStream is fed from).  The first head_docs(k) documents are scored into a plane and get an
    exact top-k (one sort-kernel row per query); after that only scores above a query's running k-th best can enter, so the rest goes through the
    source's filter kernel -- no score plane, no filter pass -- in CHUNK-document feeds and the candidates are folded into the list a few times
    per shard (ops.TopkStream).  A window in which a row overflowed its candidate buffer is redone exactly, on its own (flag read at every fold: 4
    small reads per shard).  `mark(name)`: optional instrumentation hook (bench.py records a HIP event per call).
    Everything runs on ONE stream: issuing the top-k work of chunk c on a second stream under the GEMM of chunk c + 1 was
    measured twice and lost both times (17.3 vs 15.5 ms per 1.1 M-document shard in round 2: the persistent GEMM owns every
    CU, and what squeezes in next to it costs the matrix pipe more than it hides)."""

    CAP = 7168          # candidate slots per row and window on the streaming path (k + CAP = one 8192-key sort row at k = 1024)
    HEAD = 28672        # at most this many leading documents get the exact top-k (one sort-kernel row); 8 k of them (>= 8192) are enough
    _grain = 1          # document ranges start on a multiple of it
    last_overflow = 0   # windows of the last local_topk whose candidate buffers overflowed (each was redone exactly, ops.TopkStream)

    def head_docs(self, k: int) -> int:
        """8,192 at k = 1000 (a 0.09 ms sort instead of 0.35, one fold more), rounded up to whole grains (sparse: 14,336)."""
        return ops.stream_head_docs(k, self._grain, self.HEAD)

    def _streams(self, k: int, n: int) -> bool:
        return ops.stream_fits(k, self.CAP, self.head_docs(k), n)

    def _chunk(self) -> int:
        return ops.stream_chunk(self.CHUNK, self._grain)

    def _topk(self, q: tuple, k: int, streaming: bool, mark):
        mark = mark or (lambda name: None)
        src = self._source(*q)
        self.last_overflow = 0
        if not (streaming and self._streams(k, src.n)):
            return self.two_pass_topk(q, k, mark)
        best_s, best_i, self.last_overflow = ops.stream_search(src, k, self.head_docs(k), self._chunk(), self.CAP, self.PLANE_MARK, mark)
        return best_s, best_i

    def two_pass_topk(self, q: tuple, k: int, mark=None):
        """Per chunk a score plane, its top-k, a merge: for a small shard or a k beyond the streaming sort's reach (and the fused paths' yardstick)."""
        mark = mark or (lambda name: None)
        src, best_s, best_i = self._source(*q), None, None
        for c0 in range(0, max(src.n, 1), self._chunk()):
            S, base = src.plane(c0, min(src.n, c0 + self._chunk())); mark(self.PLANE_MARK)
            s, i = ops.topk_rows(S, k, id_base=base)
            if best_s is not None:   # merge two id-ascending lists (chunks arrive in id order)
                s, i = ops.topk_merge(torch.stack([best_s, s]), torch.stack([best_i, i]))
            best_s, best_i = s, i; mark("shard_topk_exact")
        return best_s, best_i

    def _no_lists(self, Q: int, k: int, dev):
        """An empty shard's (or no query's) lists: all padding, (-inf, -1)."""
        self.last_overflow = 0
        return torch.full((Q, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((Q, k), -1, dtype=torch.int64, device=dev)

    def _search(self, q: tuple, k: int, mark):
        out = allgather_topk(*self.local_topk(*q, k, mark=mark), group=self.group)
        if mark: mark("allgather_merge")
        return out

    def _search_feedback(self, q: tuple, k: int, mark, feedback: dict):
        """search -> feedback -> search: the first pass's lists feed the queries back (the subclass's feedback(*q, first, **feedback): one
        tensor or a tuple, as its search takes them), the expanded queries are searched again -> planes.RankedTopk of the second pass."""
        from .planes import RankedTopk
        first = RankedTopk.from_search(*self.search(*q, k, mark=mark))
        q = self.feedback(*q, first, **feedback)
        return RankedTopk.from_search(*self.search(*(q if isinstance(q, tuple) else (q,)), k, mark=mark))


class ShardedDenseIndex(_PairScores, _ShardedIndex):
    """One rank's shard of the L2-normalised corpus embeddings: the fp32-MFMA GEMM scores it, and after the head the GEMM's epilogue is
    the threshold filter (fz_dot_scores_filter_f32: per shard 4.5 GB less written and 4.5 GB less read than a plane and a filter pass)."""

    CHUNK = 8 * 28672   # documents per GEMM launch: 8 sort-kernel rows per query
    FUSED = True        # after the head, score and filter in one kernel (fz_dot_scores_filter_f32); False: GEMM, then the filter pass
    PLANE_MARK = "shard_gemm"

    def __init__(self, Dn_local: torch.Tensor, id_base: int, group=None):
        self.Dn, self.id_base, self.group = Dn_local, int(id_base), group

    def _source(self, Qn):
        return ops._gemm_source(Qn, self.Dn, self.id_base)

    def local_topk(self, Qn: torch.Tensor, k: int, streaming: bool = True, mark=None):
        """[Q, k] (score desc, id asc) over this shard; streaming=False forces the two-pass path."""
        if streaming and self._streams(k, self.Dn.shape[0]) and not (self.FUSED and Qn.shape[1] % 4 == 0):
            return self._unfused_topk(Qn, k, mark or (lambda name: None))
        return self._topk((Qn,), k, streaming, mark)

    def _unfused_topk(self, Qn, k, mark):
        """Streaming with the filter as a pass of its own over each chunk's GEMM plane (FUSED = False, or a d the fused kernel does not take).
        The stream holds no score plane (one chunk alive at a time): after a window that overflowed, this shard again on the two-pass path."""
        n, head, stream = self.Dn.shape[0], self.head_docs(k), None
        for c0 in range(0, n, self.CHUNK):
            c1 = min(n, c0 + self.CHUNK)
            S = ops.dot_scores(Qn, self.Dn[c0:c1]); mark("shard_gemm")
            lo = 0
            if stream is None:
                lo = min(head, c1 - c0)
                bs, bi = ops.topk_rows(S[:, :lo], k, id_base=self.id_base + c0)
                stream = ops.TopkStream(bs, bi, seen=lo, cap=self.CAP)
            stream.feed(S[:, lo:], self.id_base + c0 + lo); mark("shard_topk_stream")
            if stream.unrepairable:   # a window of scores the stream does not hold overflowed: the rest of the streaming pass would be wasted
                break
        best_s, best_i, flag = stream.result(); mark("shard_topk_stream")
        self.last_overflow = 0
        if int(flag.item()) != 0:
            best_s, best_i = self.local_topk(Qn, k, streaming=False, mark=mark)
            self.last_overflow = 1
        return best_s, best_i

    def search(self, Qn: torch.Tensor, k: int = 1000, mark=None):
        return self._search((Qn,), k, mark)

    def local_pair_scores(self, Qn: torch.Tensor, cand_ids: torch.Tensor, cand_len: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, W] float32: the GEMM's score of query q and candidate cand_ids[q, r], bit for bit, without the plane (ops.dot_pairs)."""
        return ops.dot_pairs(Qn, self.Dn, cand_ids, cand_len, id_base=self.id_base)

    def feedback(self, Qn: torch.Tensor, topk, *, fb_docs: int = 10, alpha: float = 1.0, beta: float = 1.0, weighting: str = "uniform",
                 normalize: bool = True) -> torch.Tensor:
        """Pseudo-relevance feedback: the queries moved towards the first fb_docs documents of their own lists (topk: a planes.RankedTopk
        of a first search), q' = alpha * q + sum_r coef_r * d_r in list order (ops.dense_feedback; feedback.coefficients gives coef from
        beta and `weighting`).  -> [Q, dim] float32, L2-normalised by ops.normalize_rows when `normalize`.  With more than one rank the
        rows are gathered first (feedback.gather_rows): the result does not depend on the number of shards."""
        from . import feedback as fb
        fb_ids, fb_len, coef = fb.coefficients(topk, fb_docs, beta, weighting)
        Dn = self.Dn[:, :Qn.shape[1]]                       # (a corpus matrix padded past the queries' width)
        if world(self.group) > 1:
            rows, slots = fb.gather_rows(Dn, fb_ids, self.id_base, self.group)
            out = ops.dense_feedback(Qn, rows, slots, fb_len, coef, alpha)
        else:
            out = ops.dense_feedback(Qn, Dn, fb_ids, fb_len, coef, alpha, id_base=self.id_base)
        return ops.normalize_rows(out) if normalize else out

    def search_feedback(self, Qn: torch.Tensor, k: int = 1000, *, mark=None, **feedback):
        """search -> feedback -> search -> planes.RankedTopk of the second pass.  **feedback: the keyword arguments of feedback()."""
        return self._search_feedback((Qn,), k, mark, feedback)


class ShardedSparseIndex(_PairScores, _ShardedIndex):
    """One rank's shard of a SPLADE corpus as an inverted index (ops.SparseIndex, documents 0 .. N-1 = global ids id_base ..) + the
    chunked score -> top-k loop of splade/base.py:199-251 (BaseModel.search) at corpus scale: ops.sparse_dot scores the head, the rest
    streams through fz_sparse_dot_filter_f32, the posting walk whose epilogue is the filter.  Ties go to the ascending global id (SPLADE
    rows are mostly exact zeros: this rule decides the tail of a query that matches fewer than k documents)."""

    CHUNK = 32 * 7168   # documents per feed (rounded down to whole slices of the kernels, 7,168 documents each; at least one)
    PLANE_MARK = "shard_sparse"
    _grain = property(lambda self: ops.sparse_slice_docs())

    def __init__(self, index, id_base: int, group=None):
        self.index, self.id_base, self.group = index, int(id_base), group

    def _source(self, qoff, qterms, qw):
        return ops._sparse_source(self.index, qoff, qterms, qw, self.id_base)

    def local_topk(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, k: int, mark=None):
        """[Q, k] (score desc, id asc) over this shard for the queries' term lists (ops.sparse_rows); short lists padded with (-inf, -1)."""
        Q = qoff.numel() - 1
        if self.index.N == 0 or Q == 0:
            return self._no_lists(Q, k, qoff.device)
        return self._topk((qoff, qterms, qw), k, True, mark)

    def search(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, k: int = 1000, mark=None):
        return self._search((qoff, qterms, qw), k, mark)

    def build_forward(self):
        """The shard's forward index (ops.SparseIndex.build_forward): local_pair_scores, pair_scores and rerank then follow
        ops.sparse_dot_pairs' route rule."""
        return self.index.build_forward()

    def local_pair_scores(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, cand_ids: torch.Tensor,
                          cand_len: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, W] float32: the posting walk's score of query q and candidate cand_ids[q, r], bit for bit, without the plane
        (ops.sparse_dot_pairs, by the route it picks)."""
        return ops.sparse_dot_pairs(self.index, qoff, qterms, qw, cand_ids, cand_len, id_base=self.id_base)

    def feedback(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, topk, *, fb_docs: int = 10, fb_terms: int = 32,
                 alpha: float = 1.0, beta: float = 1.0, weighting: str = "uniform", normalize: bool = True):
        """Pseudo-relevance feedback: the queries expanded from the first fb_docs documents of their own lists (topk: a planes.RankedTopk
        of a first search).  q' = alpha * q + sum_r coef_r * d_r in list order over the shard's forward rows (ops.sparse_feedback); of the
        terms the documents bring in, the fb_terms strongest are kept.  -> (qoff', qterms', qw') as search() takes them, L2-normalised
        when `normalize`.  ValueError without build_forward() and for a vocabulary beyond ops.sparse_feedback_max_vocab().  With more
        than one rank the rows are gathered first (feedback.gather_rows): the result does not depend on the number of shards."""
        from . import feedback as fb
        fwd = self.index.forward
        if fwd is None:
            raise ValueError("ShardedSparseIndex.feedback: the index has no forward index (build_forward())")
        if self.index.V > ops.sparse_feedback_max_vocab():
            raise ValueError(f"ShardedSparseIndex.feedback: V = {self.index.V} is beyond the kernel's accumulator "
                             f"({ops.sparse_feedback_max_vocab()} terms, ops.sparse_feedback_max_vocab)")
        fb_ids, fb_len, coef = fb.coefficients(topk, fb_docs, beta, weighting)
        base = self.id_base
        if world(self.group) > 1:
            fwd, fb_ids = fb.gather_rows(fwd, fb_ids, self.id_base, self.group)
            base = 0
        return ops.sparse_feedback(fwd, self.index.V, qoff, qterms, qw, fb_ids, fb_len, coef, alpha, fb_terms, id_base=base, normalize=normalize)

    def search_feedback(self, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, k: int = 1000, *, mark=None, **feedback):
        """search -> feedback -> search -> planes.RankedTopk of the second pass.  **feedback: the keyword arguments of feedback()."""
        return self._search_feedback((qoff, qterms, qw), k, mark, feedback)


class ShardedLexicalIndex(_PairScores):
    """One rank's shard of a BM25 / AtireBM25 / TF-IDF corpus: a retrievers.bm25 model of the shard's documents built with the WHOLE corpus's
    statistics (`stats=LexicalStats.merge(...)`: global idf and avgdl) and its `id_base`, so every document scores what the whole index
    gives it, bit for bit.  local_topk is the model's own streamed (or plane) top-k in float64; the shards' lists are all-gathered and merged
    by one stable float64 row sort (ops.topk_merge64): ties go to the ascending global id, whatever the number of shards.  CAP, CHUNK and
    HEAD are the model's."""

    last_overflow = 0   # windows of the last local_topk that were redone exactly (the model's)

    def __init__(self, model, group=None):
        self.model, self.id_base, self.group = model, int(model.id_base), group

    def local_topk(self, queries: list[str], k: int, mark=None, streaming: bool | None = True):
        """([Q, k] float64 scores, [Q, k] int64 global ids), score desc / id asc, over this shard (k cut to the shard's size).  Marks:
        'shard_lexical' after a plane launch, 'shard_lexical_filter' after a filter launch, 'shard_topk_stream' after a fold."""
        out = self.model._topk_device(queries, k, streaming=streaming, mark=mark)
        self.last_overflow = self.model.last_overflow
        return out

    def search(self, queries: list[str], k: int = 1000, mark=None):
        """-> planes.RankedTopk of the global top-k (scores64 kept; scores = their float32 roundings)."""
        from .planes import RankedTopk
        s, i = self.local_topk(queries, k, mark=mark)
        if s.shape[1] < k:     # a shard smaller than k: pad to the common width of the collective
            pad = k - s.shape[1]
            s = torch.cat([s, torch.full((s.shape[0], pad), float("-inf"), dtype=s.dtype, device=s.device)], 1)
            i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=i.dtype, device=i.device)], 1)
        s, i = allgather_topk(s, i, group=self.group, merge_fn=ops.topk_merge64)
        if mark: mark("allgather_merge")
        return RankedTopk.from_search(s.to(torch.float32), i, scores64=s)

    def local_pair_scores(self, queries: list[str], cand_ids: torch.Tensor, cand_len: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, W] float64: the model's score of query q and candidate cand_ids[q, r] (model.doc_scores on the positions id - id_base: the
        bits of the full plane's entry); -inf for a slot this shard does not own.  rerank ranks by the float64 scores and keeps them as
        scores64."""
        m = self.model
        ci = torch.as_tensor(cand_ids).to(device=m.device, dtype=torch.int64)
        if ci.dim() != 2 or ci.shape[0] != len(queries):
            raise ValueError(f"ShardedLexicalIndex.pair_scores: cand_ids must be [Q = {len(queries)}, W], got {tuple(ci.shape)}")
        if ci.numel() == 0:
            return torch.empty(tuple(ci.shape), dtype=torch.float64, device=m.device)
        local = ci - self.id_base
        mine = (ci >= 0) & (local >= 0) & (local < m.corpus_size)
        if cand_len is not None:
            mine &= torch.arange(ci.shape[1], device=m.device)[None, :] < cand_len.to(m.device)[:, None]
        return m.doc_scores(queries, torch.where(mine, local, -1))

    # -- pseudo-relevance feedback: the rows of the feedback documents in the corpus's common term space (feedback.global_term_table) --
    def _term_space(self):
        """(words of the global ids, local -> global [V_local] int64 device, global -> local [n_global] int64 device), built once."""
        if getattr(self, "_terms", None) is None:
            from . import feedback as fb
            words, l2g = fb.global_term_table(self.model)
            g2l = fb.global_to_local(l2g, len(words))
            dev = self.model.device
            self._terms = (words, torch.from_numpy(l2g).to(dev), torch.from_numpy(g2l).to(dev), {w: i for i, w in enumerate(words)})
        return self._terms

    def global_feedback(self, queries: list[str], topk, *, fb_docs: int = 10, fb_terms: int = 10, alpha: float = 1.0, beta: float = 0.5,
                        weighting: str = "uniform"):
        """The expanded queries over the GLOBAL term ids (a retrievers.bm25.WeightedQueries; feedback.global_term_table's words name the
        ids): every rank packs the rows of the feedback documents it owns (feedback.pack_lexical_rows), one all_reduce(MAX) per tensor
        (and one for the row width) leaves every slot its owner's row on every rank, and the rows kernel (ops.lexical_feedback_rows) runs
        on the queries' terms mapped to global ids.  Ties are broken on the global id: the expansions do not depend on the number of
        shards.  The arithmetic and the keywords are TFIDF.feedback's."""
        from . import feedback as fb
        from .retrievers.bm25 import WeightedQueries
        import numpy as np
        m = self.model
        words, l2g, _, gid = self._term_space()
        fb_ids, fb_len, coef = fb.coefficients(topk, fb_docs, 1.0, weighting)
        walks = m.lexical_mode() is not None                           # (a shard without postings owns no row)
        if walks and m.forward is None:
            m.build_forward()
        lens = fb.lexical_row_lengths(m, fb_ids) if walks else torch.zeros_like(fb_ids)
        L = int(reduce_max(lens.max().reshape(1) if lens.numel() else torch.zeros(1, dtype=torch.int64, device=m.device), self.group).item())
        if walks:
            terms, values = fb.pack_lexical_rows(m, l2g, fb_ids, L)
        else:
            terms = torch.full(tuple(fb_ids.shape) + (L,), -1, dtype=torch.int32, device=m.device)
            values = torch.full(tuple(fb_ids.shape) + (L,), float("-inf"), dtype=torch.float64, device=m.device)
        foff, fterm, fval, slots = fb.lexical_rows(reduce_max(terms, self.group, skip_empty=True), reduce_max(values, self.group, skip_empty=True))
        qt = [[gid.get(w, -1) for w in q.split()] for q in queries]
        qoff = np.zeros(len(qt) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in qt], out=qoff[1:])
        flat = np.array([t for x in qt for t in x] or [0], dtype=np.int32)
        return WeightedQueries(*ops.lexical_feedback_rows(foff, fterm, fval, torch.from_numpy(qoff).to(m.device), torch.from_numpy(flat).to(m.device),
                                                          slots, fb_len, coef, alpha, beta, fb_terms))

    def localize(self, wq):
        """Global-id weighted queries -> this shard's: every term mapped to the shard's own id, -1 (adds nothing) where it lacks the word."""
        from .retrievers.bm25 import WeightedQueries
        g2l = self._term_space()[2]
        t = wq.qterms.long()
        local = torch.where(t >= 0, g2l[t.clamp(min=0)], torch.full_like(t, -1)) if g2l.numel() else torch.full_like(t, -1)
        return WeightedQueries(wq.qoff, local.to(torch.int32), wq.qw, wq.flags)

    def expansion_words(self, wq) -> list[list[tuple]]:
        """(word, weight) per entry of global_feedback's queries."""
        from .retrievers.bm25 import expansion_words
        return expansion_words(wq, self._term_space()[0])

    def feedback(self, queries: list[str], topk, **feedback):
        """global_feedback mapped to this shard's term ids: what the model's weighted walks take (model.search_topk_weighted)."""
        return self.localize(self.global_feedback(queries, topk, **feedback))

    def search_feedback(self, queries: list[str], k: int = 1000, *, mark=None, **feedback):
        """search -> feedback -> the weighted search over every shard, merged as search() merges -> planes.RankedTopk of the second pass."""
        from .planes import RankedTopk
        wq = self.feedback(queries, self.search(queries, k, mark=mark), **feedback)
        second = self.model.search_topk_weighted(wq, k, streaming=True, mark=mark)
        self.last_overflow = self.model.last_overflow
        s, i = second.scores64, second.ids
        if s.shape[1] < k:     # a shard smaller than k: pad to the common width of the collective
            pad = k - s.shape[1]
            s = torch.cat([s, torch.full((s.shape[0], pad), float("-inf"), dtype=s.dtype, device=s.device)], 1)
            i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=i.dtype, device=i.device)], 1)
        s, i = allgather_topk(s, i, group=self.group, merge_fn=ops.topk_merge64)
        if mark: mark("allgather_merge")
        return RankedTopk.from_search(s.to(torch.float32), i, scores64=s)

    def gold_ranks(self, queries: list[str], gold_ids) -> torch.Tensor:
        """[Q, G] int64: the rank of global id gold_ids[q, g] in query q's ranking of the WHOLE corpus (what the grid search needs of it),
        the same on every rank; an id < 0 gives -1.  Every shard scores the golds it holds (-inf for the others: all_reduce(MAX) leaves each
        gold's score), counts its own documents ranked before each gold (the model's count_before), and the counts add: all_reduce(SUM).
        With the merged statistics a document scores the same in any shard, so the sums are the whole index's ranks for any number of
        shards.  The ids must be documents of the corpus."""
        m = self.model
        gi = torch.as_tensor(gold_ids).to(device=m.device, dtype=torch.int64)
        local = gi - self.id_base
        mine = (gi >= 0) & (local >= 0) & (local < m.corpus_size)
        sc = reduce_max(m.doc_scores(queries, torch.where(mine, local, -1)), self.group)
        counts = reduce_sum(m.count_before(queries, sc, gi), self.group)
        return torch.where(gi >= 0, counts, -1)


class ShardedCentroidIndex(_ShardedIndex):
    """The candidate stage of one rank's ColBERT shard: an ops.CentroidIndex (per centroid the shard's documents that carry it, documents
    0 .. N-1 = global ids id_base ..) + the chunked score -> top-k loop over it.  A query is its probe table (ops.centroid_probes); a
    document's candidate score (ops.centroid_scores) does not depend on its shard, so the merged list is the same for any number of
    shards.  Two routes with the same lists: a plane per chunk, its top-k and a merge (the default, see STREAMING), or the exact top-k of
    the head's plane and the rest streamed through fz_centroid_scores_filter_f32.  Most documents score an exact +0.0 for most queries:
    ties go to the ascending global id, as everywhere."""

    CHUNK = 64 * 3584   # documents per feed (rounded down to whole slices of the kernels, 3,584 documents each; at least one)
    PLANE_MARK = "shard_centroid"
    # Measured (profiles/r13_colbert_search.json, 1,105,228 documents, Q = 1024): the two-pass route takes 24-42 ms where the streamed one takes
    # 40-90 (alternated runs).  Documents reached through one probe share that probe's score exactly, so a list's cut falls inside a run of equal
    # scores: 36-70 documents on average, up to 110, per 229,376 (measured in the same file), where the fold of unordered candidates puts only 64
    # entries behind the cut in id order -- 2-6 windows per search overflow and are redone exactly.  The streamed route stays
    # (local_topk(streaming=True), the same lists); the default is the faster one.
    STREAMING = False
    _grain = property(lambda self: ops.centroid_slice_docs())

    def __init__(self, index, id_base: int, group=None):
        self.index, self.id_base, self.group = index, int(id_base), group

    def _source(self, pc, ps, Lq, nprobe):
        return ops._centroid_source(self.index, pc, ps, Lq, nprobe, self.id_base)

    def local_topk(self, pc: torch.Tensor, ps: torch.Tensor, Lq: int, nprobe: int, k: int, mark=None, streaming: bool | None = None):
        """[Q, k] (score desc, id asc) over this shard for the probe tables pc / ps [Q, Lq * nprobe]; short lists padded with (-inf, -1).
        streaming=True: exact head, streamed rest, an overflowed window redone exactly (where streaming applies); False: a plane per chunk, its
        top-k, a merge; None: the class's STREAMING.  The lists are the same either way."""
        streaming = self.STREAMING if streaming is None else bool(streaming)
        Q = pc.shape[0]
        if self.index.N == 0 or Q == 0:
            return self._no_lists(Q, k, pc.device)
        return self._topk((pc, ps, Lq, nprobe), k, streaming, mark)

    def search(self, pc: torch.Tensor, ps: torch.Tensor, Lq: int, nprobe: int, k: int = 1000, mark=None):
        return self._search((pc, ps, Lq, nprobe), k, mark)


class ShardedTokenIndex(_PairScores):
    """One rank's shard of a ColBERT corpus as its packed token matrix (Dtok_local [sumL, 128] float16, Doff_local [N + 1] int64;
    documents 0 .. N-1 = global ids id_base ..) + the exact rerank of candidate lists over it: the corpus-scale counterpart of
    ops.maxsim's [Q, N] plane, which the reference never builds either (its PLAID searcher scores candidates only, hybrid.py:108-137).
    fz_maxsim_pairs_f16 scores every query against its own candidate ids with the bits of the all-pairs kernel; a slot this shard does
    not own gets -inf, so the shards' [Q, k] planes combine by ONE all_reduce(MAX), and one stable descending row sort turns the plane
    into lists (ties keep candidate-list order, whatever the number of shards).  No host synchronisation on the single-rank path.
    With build_centroids the shard also generates its own candidates (ShardedCentroidIndex) and `search` is a first-stage search:
    candidates from token centroids, every returned score exact.
    Storage: the float16 token matrix (256 B per token), or after `compress` / from `build_compressed` the residual code of
    include/fusion_hip.h 'Residual-compressed token rows' (the centroid id of the candidate stage + 2 or 4 bits per dimension: 36 or 68 B
    per token).  Decompression is a fixed function of the stored bytes, and fz_maxsim_pairs_residual_f16 scores a compressed shard with the
    bits ops.maxsim_pairs gives over the decompressed matrix: everything above holds for either storage, with D = the decompressed rows.
    A third storage needs no training at all: after `quantize` / from `build_e4m3` the rows are OCP e4m3 bytes (ops.quantize_e4m3: a fixed
    function of the float16 token, 128 B per token, no centroid table, no buckets).  fz_maxsim_pairs_e4m3 scores such a shard; the queries
    are quantised per call at the class's q_exp, and every score is the exact MaxSim of the DEQUANTISED pair, the bits ops.maxsim_e4m3
    gives it (`dequantized` returns the rows).  The shards still combine by one all_reduce(MAX); every rank must use the same exponents
    (scale_exp of the documents, q_exp of the queries), or the shards' scores are not on one scale.  One storage decides the score:
    a shard is either compressed or quantised, never both."""

    centroids = None        # [K, dim] float16, the same table on every rank (build_centroids)
    candidates = None       # the ShardedCentroidIndex of this shard
    codes = None            # [sumL] int32: every token row's centroid (build_centroids keeps them: half of the compressed index)
    packed = None           # [sumL, 16 * nbits] uint8: the residual buckets (compress / build_compressed)
    cutoffs = None          # [2^nbits - 1] float32, the same on every rank
    weights = None          # [2^nbits] float16, the same on every rank
    nbits = None
    tok8 = None             # [sumL, 128] uint8: the e4m3 rows (quantize / build_e4m3)
    d_exp = None            # their quantiser exponent
    q_exp = 8               # the exponent the queries are quantised with per call over an e4m3 shard (the same on every rank)
    TIES = "list"           # rerank keeps candidate-list order among equal scores
    EMPTY_REDUCES = False   # an empty batch returns before the scorer and the all_reduce

    def __init__(self, Dtok_local: torch.Tensor, Doff_local: torch.Tensor, id_base: int, group=None, max_doc_len: int = 512):
        self.Dtok, self.Doff, self.id_base, self.group, self.max_doc_len = Dtok_local, Doff_local, int(id_base), group, int(max_doc_len)

    def build_centroids(self, C: torch.Tensor, codes: torch.Tensor | None = None):
        """Keep the centroid table C [K, dim] (ops.kmeans_centroids; trained on one rank and broadcast, the same on every rank) and build
        this shard's candidate index: every token row is assigned its nearest centroid (ops.centroid_assign) unless `codes` [sumL] are given."""
        if codes is None:
            codes = ops.centroid_assign(self.Dtok, C)
        self.centroids = C
        self.codes = codes.to(torch.int32).contiguous()
        self.candidates = ShardedCentroidIndex(ops.centroid_index(codes, self.Doff, C.shape[0]), self.id_base, group=self.group)
        return self

    def compress(self, nbits: int = 2, cutoffs: torch.Tensor | None = None, weights: torch.Tensor | None = None, keep_tokens: bool = False):
        """Replace the float16 token matrix by its residual code against the centroid table of build_centroids: train the buckets on this
        shard's rows unless (cutoffs, weights) are given (ops.residual_buckets; multi-rank callers train on ONE rank and broadcast both, as
        for the centroids), pack every row (ops.residual_compress) and drop Dtok (None) unless keep_tokens.  From here on every score is the
        exact MaxSim over the DECOMPRESSED rows (ops.residual_decompress), the same for any number of shards."""
        if self.candidates is None or self.codes is None:
            raise ValueError("ShardedTokenIndex.compress: no centroid index (call build_centroids first)")
        if (cutoffs is None) != (weights is None):
            raise ValueError("ShardedTokenIndex.compress: give both cutoffs and weights, or neither")
        if self.tok8 is not None:
            raise ValueError("ShardedTokenIndex.compress: the shard is quantised to e4m3 (one storage decides the score)")
        if self.Dtok is None:
            raise ValueError("ShardedTokenIndex.compress: the token matrix is gone (already compressed)")
        nbits = ops._residual_nbits("ShardedTokenIndex.compress", nbits)
        C = self.centroids.to(torch.float16).contiguous()
        ops.residual_check_codes(self.codes, C.shape[0])
        if cutoffs is None:
            cutoffs, weights = ops.residual_buckets(self.Dtok, C, self.codes, nbits)
        self.packed = ops.residual_compress(self.Dtok, self.codes, C, cutoffs, nbits)
        self.centroids, self.cutoffs, self.weights, self.nbits = C, cutoffs, weights.contiguous(), nbits
        if not keep_tokens:
            self.Dtok = None
        return self

    @classmethod
    def build_compressed(cls, blocks, Doff: torch.Tensor, C: torch.Tensor, cutoffs: torch.Tensor, weights: torch.Tensor, nbits: int, id_base: int,
                         group=None, max_doc_len: int = 512, device=None):
        """A compressed shard from an ITERATOR of token-row blocks ([rows_i, 128] float16, in corpus order, together the Doff[N] rows of the
        shard; as ops.sparse_index_from_blocks takes its blocks): every block is moved to the device, assigned (ops.centroid_assign) and
        packed (ops.residual_compress) into its rows of the shard's arrays, then dropped -- the float16 matrix of the shard is never
        resident.  C, cutoffs and weights are the tables every rank shares.  The result equals build_centroids(C) + compress(nbits, cutoffs,
        weights) of the whole matrix: the same codes, bytes and candidate index."""
        nbits = ops._residual_nbits("ShardedTokenIndex.build_compressed", nbits)
        if device is None:
            device = C.device if C.is_cuda else torch.device("cuda", torch.cuda.current_device())
        C = C.to(device=device, dtype=torch.float16).contiguous()
        cutoffs, weights, Doff = cutoffs.to(device), weights.to(device).contiguous(), Doff.to(device)
        sumL = int(Doff[-1]) if Doff.numel() else 0
        codes = torch.empty(sumL, dtype=torch.int32, device=device)
        packed = torch.empty((sumL, 16 * nbits), dtype=torch.uint8, device=device)

        def fill(at, blk):
            rows = slice(at, at + blk.shape[0])
            codes[rows] = ops.centroid_assign(blk, C)
            ops.residual_compress(blk, codes[rows], C, cutoffs, nbits, out=packed[rows])
        _fill_blocks("ShardedTokenIndex.build_compressed", blocks, sumL, device, fill)
        self = cls(None, Doff, id_base, group=group, max_doc_len=max_doc_len)
        self.centroids, self.codes = C, codes
        self.candidates = ShardedCentroidIndex(ops.centroid_index(codes, Doff, C.shape[0]), self.id_base, group=group)
        self.packed, self.cutoffs, self.weights, self.nbits = packed, cutoffs, weights, nbits
        return self

    def decompressed(self, row_lo: int = 0, row_hi: int | None = None) -> torch.Tensor:
        """Rows [row_lo, row_hi) of the matrix a compressed shard scores against ([rows, 128] float16; ops.residual_decompress)."""
        if self.packed is None:
            raise ValueError("ShardedTokenIndex.decompressed: the shard is not compressed")
        return ops.residual_decompress(self.packed, self.codes, self.centroids, self.weights, row_lo, row_hi)

    def quantize(self, scale_exp: int = 8, keep_tokens: bool = False):
        """Replace the float16 token matrix by its e4m3 bytes (ops.quantize_e4m3 at 2^scale_exp: 128 B per token, nothing trained) and drop
        Dtok (None) unless keep_tokens.  From here on every score is the exact MaxSim of the DEQUANTISED queries and rows (`dequantized`;
        ops.maxsim_e4m3's bits), the same for any number of shards as long as every rank uses the same scale_exp and q_exp.  A centroid
        index built before (build_centroids) stays: `search` draws its candidates as before and scores them over the e4m3 rows."""
        if self.packed is not None:
            raise ValueError("ShardedTokenIndex.quantize: the shard is residual-compressed (one storage decides the score)")
        if self.tok8 is not None:
            raise ValueError("ShardedTokenIndex.quantize: the shard is already quantised")
        if self.Dtok is None:
            raise ValueError("ShardedTokenIndex.quantize: the token matrix is gone")
        scale_exp = ops._e4m3_exp(scale_exp, "ShardedTokenIndex.quantize")
        self.tok8, self.d_exp = ops.quantize_e4m3(self.Dtok, scale_exp), scale_exp
        if not keep_tokens:
            self.Dtok = None
        return self

    @classmethod
    def build_e4m3(cls, blocks, Doff: torch.Tensor, id_base: int, *, scale_exp: int = 8, C: torch.Tensor | None = None, group=None,
                   max_doc_len: int = 512, device=None):
        """An e4m3 shard from an ITERATOR of token-row blocks ([rows_i, 128] float16, in corpus order, together the Doff[N] rows of the shard;
        as build_compressed takes its blocks): every block is moved to the device and quantised (ops.quantize_e4m3) into its rows of the
        shard's [sumL, 128] uint8 array, then dropped -- the float16 matrix of the shard is never resident.  With C [K, 128] every block is
        also assigned (ops.centroid_assign) and the codes and the candidate index are built, so `search` works.  The result equals
        cls(...).build_centroids(C).quantize(scale_exp) of the whole matrix: the same bytes, codes and candidate index."""
        scale_exp = ops._e4m3_exp(scale_exp, "ShardedTokenIndex.build_e4m3")
        if device is None:
            device = C.device if C is not None and C.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if C is not None:
            C = C.to(device=device)
        Doff = Doff.to(device)
        sumL = int(Doff[-1]) if Doff.numel() else 0
        tok8 = torch.empty((sumL, 128), dtype=torch.uint8, device=device)
        codes = None if C is None else torch.empty(sumL, dtype=torch.int32, device=device)

        def fill(at, blk):
            rows = slice(at, at + blk.shape[0])
            tok8[rows] = ops.quantize_e4m3(blk, scale_exp)
            if C is not None:
                codes[rows] = ops.centroid_assign(blk, C)
        _fill_blocks("ShardedTokenIndex.build_e4m3", blocks, sumL, device, fill)
        self = cls(None, Doff, id_base, group=group, max_doc_len=max_doc_len)
        if C is not None:
            self.build_centroids(C, codes=codes)
        self.tok8, self.d_exp = tok8, scale_exp
        return self

    def dequantized(self, row_lo: int = 0, row_hi: int | None = None) -> torch.Tensor:
        """Rows [row_lo, row_hi) of the matrix a quantised shard scores against ([rows, 128] float32; ops.dequantize_e4m3)."""
        if self.tok8 is None:
            raise ValueError("ShardedTokenIndex.dequantized: the shard is not quantised")
        return ops.dequantize_e4m3(self.tok8[row_lo: row_hi], self.d_exp)

    def memory_bytes(self) -> dict:
        """Resident bytes by part: the token matrix of whatever type (float16 rows, e4m3 rows, or both after quantize(keep_tokens=True)),
        the codes, the packed residuals, the candidate index (lists + slice table), and their total.  The centroid and bucket tables are
        shared by every shard and not counted."""
        size = lambda t: 0 if t is None else t.numel() * t.element_size()      # noqa: E731
        ix = None if self.candidates is None else self.candidates.index
        out = dict(tokens=size(self.Dtok) + size(self.tok8), codes=size(self.codes), packed=size(self.packed),
                   candidates=0 if ix is None else size(ix.coff) + size(ix.cdoc) + size(ix.slice_off))
        out["total"] = sum(out.values())
        return out

    @staticmethod
    def search_defaults(k: int) -> tuple[int, int]:
        """(nprobe, ncand) of `search` for a list of k.  nprobe 1 / 2 / 4 for k <= 10 / <= 100 / larger and a candidate list of 4k (at least
        256) follow colbert-ai's published search settings in spirit; they are UNMEASURED here in the sense that no measurement chose
        them (tools/bench_colbert_search.py records their recall on a synthetic corpus, profiles/r13_colbert_search.json: no ground to
        retune them).  3,584 is the longest list the streaming top-k ranks; a longer one takes the two-pass path in any case."""
        return (1 if k <= 10 else 2 if k <= 100 else 4), max(k, min(max(4 * k, 256), 3584))

    def search(self, Qtok: torch.Tensor, k: int = 1000, nprobe: int | None = None, ncand: int | None = None, mark=None):
        """First-stage ColBERT search over the sharded corpus -> planes.RankedTopk of the k best of the ncand candidates: (1) probes: every
        query token's nprobe best centroids; (2) the global top-ncand documents by candidate score (ShardedCentroidIndex.search: one
        all-gather); (3) `rerank` of those ids: exact MaxSim, one all_reduce(MAX); (4) the cut to k.  What is approximate is the candidate
        set; every returned score is the exact MaxSim of its pair, the bits of ops.maxsim.  Query tokens must be finite."""
        k = int(k)
        d_nprobe, d_ncand = self.search_defaults(k)
        nprobe = d_nprobe if nprobe is None else int(nprobe)
        ncand = d_ncand if ncand is None else int(ncand)
        if self.candidates is None:
            raise ValueError("ShardedTokenIndex.search: no centroid index (call build_centroids first)")
        if k < 1 or k > ncand or nprobe < 1:
            raise ValueError(f"ShardedTokenIndex.search: k = {k} must be in 1 .. ncand = {ncand}, nprobe = {nprobe} at least 1")
        mark = mark or (lambda name: None)
        Qtok = Qtok.contiguous()
        pc, ps = ops.centroid_probes(Qtok, self.centroids, nprobe); mark("colbert_probes")
        _, cand_ids = self.candidates.search(pc, ps, Qtok.shape[1], nprobe, ncand, mark=mark)
        out = self.rerank(Qtok, cand_ids, k=k); mark("colbert_rerank")
        return out

    @classmethod
    def from_encoder(cls, model, documents: list[str], id_base: int = 0, group=None, batch_size: int = 64, device=None):
        """Encode this shard's documents with a ColBERT encoder (fusion_amd.encoders: encode_docs -> packed token rows + offsets)."""
        Dtok, Doff = model.encode_docs(documents, batch_size=batch_size)
        if device is None:
            device = Dtok.device if Dtok.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return cls(Dtok.to(device), Doff.to(device), id_base, group=group, max_doc_len=model.max_doc_length)

    @property
    def N(self) -> int:
        return self.Doff.numel() - 1

    def local_scores(self, Qtok: torch.Tensor, cand_ids: torch.Tensor, cand_len: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, k] float32: exact MaxSim of query q and candidate cand_ids[q, r]; -inf for a slot this shard does not own (r >= cand_len[q],
        a negative id, a document of another shard).  A compressed shard scores its decompressed rows (also when compress kept the tokens);
        a quantised shard scores its dequantised rows against the queries quantised at q_exp (also when quantize kept the tokens)."""
        if self.packed is not None:
            return ops.maxsim_pairs_residual(Qtok, self.packed, self.codes, self.centroids, self.weights, self.Doff, cand_ids, cand_len,
                                             id_base=self.id_base, max_doc_len=self.max_doc_len)
        if self.tok8 is not None:
            return ops.maxsim_pairs_e4m3(ops.quantize_e4m3(Qtok, self.q_exp), self.tok8, self.Doff, cand_ids, cand_len, q_exp=self.q_exp,
                                         d_exp=self.d_exp, id_base=self.id_base, max_doc_len=self.max_doc_len)
        return ops.maxsim_pairs(Qtok, self.Dtok, self.Doff, cand_ids, cand_len, id_base=self.id_base, max_doc_len=self.max_doc_len)


class ShardedTextIndex(_PairScores):
    """One rank's shard of the corpus as TOKEN IDS, for the cross-encoder rerank of top-k lists (hybrid.py:139-163): tok [sumL] int32,
    Doff [N + 1] int64, documents 0 .. N-1 = global ids id_base ..; the pattern of ShardedTokenIndex.  A document holds the first
    min(len, max_length - (2 + nsep)) plain tokens of its text, no specials -- the most any pair can keep of it, since pair truncation
    only ever removes from the tail -- and full_len [N] int32 (or None: nothing was cut) remembers len: the tokenizer's longest_first
    rule gives the odd token of an odd budget to the STRICTLY longer sequence, which the stored prefix alone cannot tell once it is cut.
    encoders.CrossEncoder.score_candidates assembles the (query, document) rows of the packed forward from these ids on the device
    (fz_pair_plan / fz_pair_fill): no string is built, no document re-tokenised, no padded id matrix uploaded.  A slot this shard does not
    own gets -inf, so the shards' [Q, W] planes combine by ONE all_reduce(MAX) and every rank forwards only the pairs whose documents it
    holds: the forward is split across the ranks by the sharding alone."""

    TIES = "list"           # rerank keeps candidate-list order among equal scores, as ShardedTokenIndex
    EMPTY_REDUCES = False   # an empty batch returns before the forward and the all_reduce

    def __init__(self, tok: torch.Tensor, Doff: torch.Tensor, id_base: int, group=None, full_len: torch.Tensor | None = None):
        ops._pair_store("ShardedTextIndex", tok, Doff, full_len)
        self.tok, self.Doff, self.id_base, self.group, self.full_len = tok, Doff, int(id_base), group, full_len

    @classmethod
    def from_texts(cls, model, documents: list[str], id_base: int = 0, group=None, device=None):
        """Tokenise this shard's documents ONCE with the cross-encoder's tokenizer (tokenizer.encode_plain), cut at what `model` can keep."""
        import numpy as np
        if device is None:
            device = model._device
        if torch.device(device).type != "cuda":
            raise TypeError(f"ShardedTextIndex.from_texts: the index lives on the GPU (fusion_amd has no CPU path), got device {device}")
        keep = model.max_length - (2 + model.tokenizer.pair_spec()["nsep"])
        ids, full = model.tokenizer.encode_plain(documents, keep)
        held = np.minimum(full.numpy().astype(np.int64), max(keep, 0))
        Doff = np.zeros(len(documents) + 1, dtype=np.int64)
        np.cumsum(held, out=Doff[1:])
        tok = ids.numpy()[np.arange(ids.shape[1])[None, :] < held[:, None]]
        cut = bool((full.numpy() > held).any())
        return cls(torch.from_numpy(np.ascontiguousarray(tok, dtype=np.int32)).to(device), torch.from_numpy(Doff).to(device), id_base, group=group,
                   full_len=full.to(device) if cut else None)

    @property
    def N(self) -> int:
        return self.Doff.numel() - 1

    def local_scores(self, model, qtok: torch.Tensor, qlen: torch.Tensor, cand_ids: torch.Tensor, cand_len: torch.Tensor | None = None) -> torch.Tensor:
        """[Q, W] float32: model.score_candidates over this shard; -inf for a slot it does not own.  (pair_scores as an
        Aggregator.complete_topk scorer: lambda ids, lens: index.pair_scores(model, qtok, qlen, ids, lens).)"""
        return model.score_candidates(self, qtok, qlen, cand_ids, cand_len)

    def rerank(self, model, qtok: torch.Tensor, qlen: torch.Tensor, candidates, k: int | None = None, depth: int | None = None):
        """_PairScores.rerank by the cross-encoder's scores.  depth: only the first `depth` slots of every list are scored (and returned)."""
        ids, cand_len = _candidates(candidates)
        ops._dev(ids, torch.int64, "ShardedTextIndex.rerank(candidates)")
        if depth is not None:
            if int(depth) < 1:
                raise ValueError(f"ShardedTextIndex.rerank: depth = {depth} must be at least 1")
            ids = ids[:, : int(depth)]
        return self._rerank((model, qtok, qlen), ids, cand_len, k)
