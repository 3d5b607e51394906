"""Cross-encoder rerank of top-k lists on the GPU: fz_pair_plan / fz_pair_fill against their numpy restatements (crosspack_cases) and against
the rows the host route builds, CrossEncoder.score_candidates against PackedBertForward.hidden bit for bit and against CrossEncoder.predict,
the shard ownership rules, ShardedTextIndex.rerank and Ranker.cross_encoder_rerank.  Tiny models (hidden 128, 2 heads, 2 layers); the smallest
shapes at which the kernels can go wrong: Q = 5, W = 7, N = 23, lengths around the pair budget B, id_base beyond 2^33."""
import numpy as np
import pytest
import torch

import crosspack_cases as X
from checkpoint_utils import write_monobert_checkpoint

pytestmark = pytest.mark.gpu
KINDS = ("hash", "hf")          # HashTokenizer: 'tail' rule, one separator; the word-level fast tokenizer: 'longest_first', two
LENGTHS = (16, 17)              # B = 13 / 14 (hash) and 12 / 13 (hf): an odd and an even budget for both rules
TOL = 1e-4                      # what test_packed_cross_encoder_matches_padded_forward grants the packed forward on this model size
_cache = {}


def _model(kind, tmp_path_factory):
    from fusion_amd import encoders
    if kind not in _cache:
        if kind == "hf":
            path = str(tmp_path_factory.mktemp("monobert"))
            write_monobert_checkpoint(path, heads=2, hidden=128)
            _cache[kind] = encoders.from_pretrained(path, "monobert", device="cuda")
        else:
            from transformers import CamembertConfig, CamembertForSequenceClassification
            cfg = dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256)
            torch.manual_seed(2)
            _cache[kind] = encoders.CrossEncoder(CamembertForSequenceClassification(CamembertConfig(num_labels=1, **cfg)),
                                                 encoders.HashTokenizer(cfg["vocab_size"]), "cuda")
    return _cache[kind]


class Case:
    """One (tokenizer, max_length): texts, the token store built from them, the queries' ids, the candidate plane, and the restated plan."""

    def __init__(self, ce, ml, id_base=X.BIG_BASE):
        from fusion_amd.distributed import ShardedTextIndex
        self.ce, self.ml, self.id_base = ce, ml, id_base
        ce.max_length, ce.packed_tokens = ml, 65536
        self.spec = ce.tokenizer.pair_spec()
        self.B = X.budget(ml, self.spec["nsep"])
        self.queries, self.docs = X.corpus(self.B)
        self.index = ShardedTextIndex.from_texts(ce, self.docs, id_base)
        qtok, qlen = ce.tokenizer.encode_plain(self.queries, ml - 2)
        self.qtok, self.qlen = qtok.cuda(), qlen.cuda()
        self.cand_h, self.lens_h = X.candidates(id_base)
        self.cand, self.lens = torch.from_numpy(self.cand_h).cuda(), torch.from_numpy(self.lens_h).cuda()
        self.full = np.array(X.doc_lengths(self.B))
        self.held = np.minimum(self.full, self.B)
        self.plan = X.plan(self.spec["mode"], ml, self.spec["nsep"], self.cand_h, self.lens_h, id_base, self.held, self.full,
                           X.query_lengths(self.B), self.qtok.shape[1])
        self.owned = np.flatnonzero(self.plan[2].reshape(-1))

    def use(self, packed_tokens=65536):
        self.ce.max_length, self.ce.packed_tokens = self.ml, packed_tokens
        return self

    def strings(self, slots):
        return X.pair_strings(slots, self.cand_h, self.id_base, self.queries, self.docs)


@pytest.fixture(params=[(k, ml) for k in KINDS for ml in LENGTHS], ids=lambda p: f"{p[0]}-{p[1]}")
def case(request, tmp_path_factory):
    kind, ml = request.param
    if (kind, ml) not in _cache:
        _cache[kind, ml] = Case(_model(kind, tmp_path_factory), ml)
    return _cache[kind, ml].use()


def _plan_device(c, cand=None, lens="own"):
    from fusion_amd import ops
    return ops.pair_plan(c.cand if cand is None else cand, c.lens if lens == "own" else lens, c.index.Doff, c.index.full_len, c.id_base, c.qlen,
                         c.qtok.shape[1], c.ml, c.spec["mode"], c.spec["nsep"])


def test_store_and_plan_equal_the_restatement(case):
    c = case
    assert c.index.N == X.N and c.index.Doff.cpu().tolist() == np.concatenate([[0], np.cumsum(c.held)]).tolist()
    assert c.index.full_len.cpu().tolist() == c.full.tolist() and c.index.tok.dtype == torch.int32
    plain = c.ce.tokenizer.encode_plain(c.docs, 10 ** 6)[0].numpy()
    assert c.index.tok.cpu().tolist() == [int(t) for d in range(X.N) for t in plain[d, : c.held[d]]]
    got = _plan_device(c)
    for name, g, w in zip(("kq", "kd", "L"), got, c.plan):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), name
    own = X.owned(c.cand_h, c.lens_h, c.id_base, X.N)
    assert np.array_equal(c.plan[2] > 0, own) and own.sum(1).tolist() == [5, 0, 3, 6, 7]
    assert {int(c.plan[2][4, r]) for r in range(X.W)} == {c.ml} and c.plan[2].max() == c.ml                 # the over-long query fills every row
    # a strided candidate plane, and no cand_len: every slot with a document of the shard
    wide = torch.full((X.Q, X.W + 5), c.id_base, dtype=torch.int64, device="cuda")
    wide[:, : X.W] = c.cand
    assert all(torch.equal(a, b) for a, b in zip(_plan_device(c, wide[:, : X.W]), got))
    free = X.plan(c.spec["mode"], c.ml, c.spec["nsep"], c.cand_h, None, c.id_base, c.held, c.full, X.query_lengths(c.B), c.qtok.shape[1])
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(_plan_device(c, lens=None), free))


def test_fill_equals_the_restatement_and_the_host_route(case):
    from fusion_amd import ops
    c = case
    kq, kd, L = _plan_device(c)
    slots = np.random.default_rng(5).permutation(c.owned)
    want_ids, want_pos, cu = X.fill(slots, *c.plan, c.cand_h, c.id_base, c.qtok.cpu().numpy(), c.index.tok.cpu().numpy(), c.index.Doff.cpu().numpy(),
                                    c.spec["bos"], c.spec["sep"], c.spec["eos"], 1)
    assert np.array_equal(np.diff(cu), c.plan[2].reshape(-1)[slots])
    T = int(cu[-1])
    ids, pos = ops.pair_fill(torch.from_numpy(slots.astype(np.int32)).cuda(), torch.from_numpy(cu).cuda(), T, kq, kd, c.cand, c.id_base, c.qtok,
                             c.index.tok, c.index.Doff, c.spec["bos"], c.spec["sep"], c.spec["eos"], 1, c.spec["nsep"])
    assert ids.dtype == pos.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(pos.cpu().numpy(), want_pos)
    # the rows PackedBertForward.hidden derives from the host-built pair ids of the same pairs, in the same order
    host_ids, mask = c.ce._pair_ids(c.strings(slots), c.ml)
    assert np.array_equal(np.concatenate([[0], np.cumsum(mask.sum(1).numpy())]), cu)
    assert np.array_equal(host_ids[mask.bool()].numpy(), want_ids)
    cols = np.arange(T) - np.repeat(cu[:-1], np.diff(cu))
    assert np.array_equal(want_pos, cols + 2)                                                              # pad_idx + 1 + column


def _reference_bits(c, slots):
    """hidden() of the host-built padded ids of these pairs, in this order, then the classifier: what predict does with one sub-batch."""
    ce = c.ce
    fwd = ce._packed_forward(getattr(ce.model, ce.model.base_model_prefix))
    ids, mask = ce._pair_ids(c.strings(slots), c.ml)
    with torch.no_grad():
        x, cu_d = fwd.hidden(ids.cuda(), mask.sum(1).numpy())
        score = ce.model.classifier(x.index_select(0, cu_d[:-1].long()).unsqueeze(1)).reshape(len(slots), -1)[:, 0].float()
    return torch.sigmoid(score) if ce.activation == "sigmoid" else score


def test_one_sub_batch_has_the_bits_of_the_host_route(case):
    c = case
    out = c.ce.score_candidates(c.index, c.qtok, c.qlen, c.cand, c.lens)
    assert out.shape == (X.Q, X.W) and out.dtype == torch.float32
    lengths = c.plan[2].reshape(-1)[c.owned]
    slots = c.owned[np.argsort(-lengths, kind="stable")]                                                   # the forward order: longest first
    got = out.reshape(-1)[torch.from_numpy(slots).cuda()]
    assert torch.equal(got, _reference_bits(c, slots))                                                     # same T, same launches: same bits
    rest = np.setdiff1d(np.arange(X.Q * X.W), c.owned)
    assert (out.reshape(-1)[torch.from_numpy(rest).cuda()] == float("-inf")).all() and torch.isfinite(got).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ml", (36, 37))
def test_sub_batches_agree_with_predict(kind, ml, tmp_path_factory):
    """packed_tokens = 64: several sub-batches, pairs longer than half of one; against CrossEncoder.predict on the pair strings."""
    c = Case(_model(kind, tmp_path_factory), ml).use(64)
    lengths = c.plan[2].reshape(-1)[c.owned]
    assert lengths.max() == ml > 32 and lengths.sum() > 5 * 64
    out = c.ce.score_candidates(c.index, c.qtok, c.qlen, c.cand, c.lens)
    ref = c.ce.predict(c.strings(c.owned), batch_size=4)
    diff = (out.reshape(-1)[torch.from_numpy(c.owned).cuda()] - ref).abs().max().item()
    print(f"score_candidates vs predict, {kind} max_length {ml}: max |diff| = {diff:.3g}")
    assert diff <= TOL
    assert torch.isinf(out).sum().item() == X.Q * X.W - len(c.owned)


def test_two_shards_own_every_slot_once(case):
    from fusion_amd.distributed import ShardedTextIndex
    c = case
    one = c.ce.score_candidates(c.index, c.qtok, c.qlen, c.cand, c.lens)
    own = torch.from_numpy(X.owned(c.cand_h, c.lens_h, c.id_base, X.N)).cuda()
    assert torch.equal(torch.isfinite(one), own) and (one[~own] == float("-inf")).all()
    cut = 11
    halves = [ShardedTextIndex.from_texts(c.ce, c.docs[:cut], c.id_base), ShardedTextIndex.from_texts(c.ce, c.docs[cut:], c.id_base + cut)]
    a, b = (c.ce.score_candidates(h, c.qtok, c.qlen, c.cand, c.lens) for h in halves)
    assert torch.equal(torch.isfinite(a) ^ torch.isfinite(b), own) and not (torch.isfinite(a) & torch.isfinite(b)).any()
    assert torch.isfinite(a).any() and torch.isfinite(b).any()
    both = torch.maximum(a, b)
    assert torch.equal(torch.isfinite(both), own) and (both[own] - one[own]).abs().max().item() <= TOL
    assert torch.equal(halves[0].pair_scores(c.ce, c.qtok, c.qlen, c.cand, c.lens), a)                     # one rank: the reduction is the identity


def _ranked(plane, ids, k):
    """The stable descending sort of a score plane, in numpy: ties keep candidate order, -inf slots end as (-inf, -1)."""
    s, i = plane.cpu().numpy(), ids.cpu().numpy()
    order = np.stack([np.array(sorted(range(s.shape[1]), key=lambda r: -s[q, r])) for q in range(s.shape[0])])[:, :k]
    ss = np.take_along_axis(s, order, 1)
    return ss, np.where(np.isfinite(ss), np.take_along_axis(i, order, 1), -1), np.isfinite(ss).sum(1)


def test_rerank_is_the_stable_sort_of_the_plane(case):
    from fusion_amd.planes import FusedTopk, RankedTopk
    c = case
    plane = c.index.pair_scores(c.ce, c.qtok, c.qlen, c.cand, c.lens)
    assert plane[3, 1] == plane[3, 4] and torch.isfinite(plane[3, 1])                                      # the duplicate: a tie
    lists = RankedTopk(ids=c.cand, scores=torch.zeros((X.Q, X.W), device="cuda"), lens=c.lens)
    for k in (None, 3, 100):
        got = c.index.rerank(c.ce, c.qtok, c.qlen, lists, k=k)
        ss, ii, ll = _ranked(plane, c.cand, X.W if k is None else min(k, X.W))
        assert isinstance(got, RankedTopk) and got.ids.dtype == torch.int64 and got.lens.dtype == torch.int32
        assert np.array_equal(got.scores.cpu().numpy(), ss) and np.array_equal(got.ids.cpu().numpy(), ii) and got.lens.cpu().tolist() == ll.tolist()
    full = c.index.rerank(c.ce, c.qtok, c.qlen, lists)
    assert full.lens.cpu().tolist() == [5, 0, 3, 6, 7] and (full.ids[1] == -1).all() and (full.scores[1] == float("-inf")).all()
    row = full.ids[3].cpu().tolist()
    assert row.count(int(c.cand_h[3, 1])) == 2 and row[6:] == [-1]
    fused = c.index.rerank(c.ce, c.qtok, c.qlen, FusedTopk(ids=c.cand, scores=torch.zeros((X.Q, X.W), dtype=torch.float64, device="cuda"), lens=c.lens))
    assert torch.equal(fused.ids, full.ids) and torch.equal(fused.scores, full.scores) and torch.equal(fused.lens, full.lens)
    # depth: only the first slots of every list are scored
    deep = c.index.rerank(c.ce, c.qtok, c.qlen, lists, depth=4)
    head = c.index.pair_scores(c.ce, c.qtok, c.qlen, c.cand[:, :4], c.lens)     # its own forward: fewer rows, so not the bits of plane[:, :4]
    assert torch.equal(torch.isfinite(head), torch.isfinite(plane[:, :4])) and (head - plane[:, :4]).nan_to_num(0.0, 0.0, 0.0).abs().max().item() <= TOL
    ss, ii, ll = _ranked(head, c.cand[:, :4], 4)
    assert deep.ids.shape == (X.Q, 4) and np.array_equal(deep.scores.cpu().numpy(), ss) and np.array_equal(deep.ids.cpu().numpy(), ii)
    assert deep.lens.cpu().tolist() == ll.tolist() == [2, 0, 3, 3, 4]
    # a plain id tensor: every row W long
    free = c.index.rerank(c.ce, c.qtok, c.qlen, c.cand)
    ss, ii, ll = _ranked(c.index.pair_scores(c.ce, c.qtok, c.qlen, c.cand), c.cand, X.W)
    assert np.array_equal(free.scores.cpu().numpy(), ss) and np.array_equal(free.ids.cpu().numpy(), ii) and free.lens.cpu().tolist() == [5, 7, 7, 6, 7]
    with pytest.raises(ValueError, match="depth"):
        c.index.rerank(c.ce, c.qtok, c.qlen, lists, depth=0)


GAP = 2e-4


def close_share(ranked_lists):
    """The share of adjacent pairs of the reference's lists whose scores are closer than GAP."""
    gaps = [a["score"] - b["score"] for lst in ranked_lists for a, b in zip(lst, lst[1:])]
    return sum(g <= GAP for g in gaps) / len(gaps)


def _spread_model(ce):
    """The case's tokenizer with a classifier whose scores spread (initializer_range 0.2: the default 0.02 leaves the <s> state, and so the
    logit, nearly the same for every pair -- 22 of 30 adjacent reference scores closer than GAP)."""
    from fusion_amd import encoders
    from transformers import CamembertConfig, CamembertForSequenceClassification
    cfg = dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256, vocab_size=ce.model.config.vocab_size,
               initializer_range=0.2)
    g = torch.random.get_rng_state()
    torch.manual_seed(7)
    model = CamembertForSequenceClassification(CamembertConfig(num_labels=1, **cfg))
    torch.random.set_rng_state(g)
    return encoders.CrossEncoder(model, ce.tokenizer, "cuda", max_length=ce.max_length)


def test_ranker_rerank_agrees_with_the_string_route(case):
    from fusion_amd.distributed import ShardedTextIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Ranker
    c = case
    ce = _spread_model(c.ce)
    queries, cand = X.e2e_inputs(c.B, c.id_base)
    index = ShardedTextIndex.from_texts(ce, c.docs, c.id_base)
    ref = Ranker.cross_encoder_search(queries, [{int(i): c.docs[int(i) - c.id_base] for i in row} for row in cand], None, model=ce)
    print(f"share of adjacent reference scores within {GAP}: {close_share(ref):.3f}")
    assert close_share(ref) <= 1 / 20                                                                      # the inputs were chosen for this
    cand_d = torch.from_numpy(cand).cuda()
    lists = RankedTopk(ids=cand_d, scores=torch.zeros((X.Q, X.W), device="cuda"), lens=torch.full((X.Q,), X.W, dtype=torch.int32, device="cuda"))
    got = Ranker.cross_encoder_rerank(queries, index, lists, model=ce)
    assert isinstance(got, RankedTopk) and got.lens.cpu().tolist() == [X.W] * X.Q
    ids, scores = got.ids.cpu().numpy(), got.scores.cpu().numpy()
    checked = 0
    for q, lst in enumerate(ref):
        s = [x["score"] for x in lst]
        for r, x in enumerate(lst):
            if (r == 0 or s[r - 1] - s[r] > GAP) and (r == len(lst) - 1 or s[r] - s[r + 1] > GAP):
                assert ids[q, r] == x["corpus_id"], (q, r)
                checked += 1
    assert checked >= 0.9 * X.Q * X.W
    top3 = Ranker.cross_encoder_rerank(queries, index, cand_d, model=ce, return_topk=3, depth=5)
    assert top3.ids.shape == (X.Q, 3) and all(set(top3.ids[q].cpu().tolist()) <= set(cand[q, :5].tolist()) for q in range(X.Q))


AMP_MEASURED = 2.88e-6   # the largest |float16-Linear score - float32 predict| measured on these pairs on an MI355X
AMP_BOUND = 2e-5         # four times it, rounded up to one digit: the vendor GEMM's solution choice differs between boxes


def test_amp_is_opt_in_and_close_to_float32(case):
    from fusion_amd import encoders
    c = case
    ref = c.ce.predict(c.strings(c.owned), batch_size=64)
    amp = encoders.CrossEncoder(c.ce.model, c.ce.tokenizer, "cuda", max_length=c.ml, activation=c.ce.activation, amp=True)
    assert amp.amp and not c.ce.amp
    out = amp.score_candidates(c.index, c.qtok, c.qlen, c.cand, c.lens)
    assert amp._packed.amp_dtype == torch.float16 and c.ce._packed.amp_dtype is None
    diff = (out.reshape(-1)[torch.from_numpy(c.owned).cuda()] - ref).abs().max().item()
    print(f"amp=True vs float32 predict, max_length {c.ml}: max |diff| = {diff:.3g}")
    assert 0 < diff <= AMP_BOUND


def test_empty_shapes(case):
    from fusion_amd.distributed import ShardedTextIndex
    from fusion_amd.planes import RankedTopk
    c = case
    none = c.ce.score_candidates(c.index, c.qtok[:0], c.qlen[:0], c.cand[:0])
    assert none.shape == (0, X.W)
    thin = c.ce.score_candidates(c.index, c.qtok, c.qlen, c.cand[:, :0])
    assert thin.shape == (X.Q, 0)
    empty = ShardedTextIndex.from_texts(c.ce, [], c.id_base)
    assert empty.N == 0 and empty.tok.numel() == 0 and empty.full_len is None
    plane = c.ce.score_candidates(empty, c.qtok, c.qlen, c.cand, c.lens)
    assert plane.shape == (X.Q, X.W) and (plane == float("-inf")).all()
    got = empty.rerank(c.ce, c.qtok, c.qlen, c.cand)
    assert (got.ids == -1).all() and (got.scores == float("-inf")).all() and got.lens.cpu().tolist() == [0] * X.Q
    for cand in (c.cand[:0], c.cand[:, :0]):
        got = c.index.rerank(c.ce, c.qtok[: cand.shape[0]], c.qlen[: cand.shape[0]], cand)
        assert isinstance(got, RankedTopk) and got.ids.shape == cand.shape and got.lens.cpu().tolist() == [0] * cand.shape[0]
    # a query of no tokens at all: qtok has no column
    bare = c.ce.score_candidates(c.index, c.qtok[:1, :0].contiguous(), c.qlen[:1] * 0, c.cand[:1], c.lens[:1])
    assert torch.equal(bare, c.ce.score_candidates(c.index, c.qtok[:1], c.qlen[:1], c.cand[:1], c.lens[:1]))
