"""Inputs, expectation and case table of the e4m3 candidate-list MaxSim tests (test_gpu_maxsim_pairs_fp8.py on the GPU,
test_maxsim_pairs_fp8_cpu.py without one).  Not collected by pytest.  maxsim_pairs_cases.py (slots, candidates, launches, expectation)
and maxsim_fp8_cases.py (the reference quantiser and the exact e4m3 grid values) are imported unchanged.

The corpus is maxsim_pairs_cases.py's -- clean documents of every EDGE_LENS length and three empty ones at the even positions,
poison-only guard documents at the odd ones, 37 poisoned rows before Doff[0], 41 after Doff[N], a last clean document of 530 tokens that
every max_doc_len of the sweep truncates -- with five more clean documents in front of the last one: csrc/rerank8.hip keeps 8 row blocks
in flight, so a round has eight shapes (1 .. 8 row blocks) where the float16 kernel's has four.  80, 96, 97 and 112 tokens are rounds of
5, 6, 7 (its last block partial) and 7 row blocks; 130 tokens is a full round of 8 and a second one of a single partial block.  Values:
maxsim_fp8_cases.grid_queries8 / grid_corpus8, integers in {-2 .. 2} with the poison 448 in dimensions 120-127, exact in e4m3 at
exponent 0; every partial sum is an integer below 2^19, exact in float32 in any order, so the kernel must equal the float64 formula bit
for bit whatever the instruction's internal order.

The case table restates the loop of csrc/rerank8.hip (row_blocks, with its MP8_RB = 8 row blocks per round; the launch arithmetic is
maxsim_pairs.h's: maxsim_pairs_cases.pairs_plan) and names, for every k and max_doc_len of the sweep, the wave-uniform branches that value
is there for (K_CLAIMS, M_CLAIMS); BRANCHES lists every branch the sweep as a whole must land on."""
import functools

import numpy as np

import maxsim_cases as M
import maxsim_fp8_cases as F
import maxsim_pairs_cases as P

# csrc/rerank8.hip
MP8_RB = 8
MP_WAVES, MP_CPW, MP_SLICE = P.MP_WAVES, P.MP_CPW, P.MP_SLICE

QS, KS, MAX_DOC_LENS, ID_BASES = P.QS, P.KS, P.MAX_DOC_LENS, P.ID_BASES
PRE, POST, SENTINEL = P.PRE, P.POST, P.SENTINEL
MORE = (80, 96, 97, 112, 130)
CLEAN = P.CLEAN[:-1] + MORE + P.CLEAN[-1:]      # the 530-token document stays the last one
LENS = M.alternate(CLEAN)[:-1]                  # 49 documents
N = len(LENS)
assert CLEAN[-1] == 530 and LENS[-1] == 530 and LENS[: len(P.LENS) - 1] == P.LENS[:-1]

candidates = functools.partial(P.candidates, N=N)      # maxsim_pairs_cases' draws and special slots, over this corpus
cand_lens, launches, expected, pairs_plan, slot_state = P.cand_lens, P.launches, P.expected, P.pairs_plan, P.slot_state


# ---- the kernel's loop over one document, restated -----------------------------------------------------------------------------------
def row_blocks(length):
    """The kernel's walk over one document of `length` (> 0) tokens: per round of up to MP8_RB row blocks, (blocks loaded, whether the
    last of them is partial, i.e. has rows clamped to the document's last token)."""
    out = []
    for c0 in range(0, length, 16 * MP8_RB):
        nb = (length - c0 + 15) >> 4
        out.append((min(nb, MP8_RB), nb <= MP8_RB and length % 16 != 0))
    return out


BRANCHES = {
    **{("absent", why): "a slot that gets -inf" for why in ("past-cand_len", "negative-id", "below-id_base", "past-N")},
    ("empty-document",): "len == 0: the score is 0, nothing is loaded",
    ("empty-row",): "cand_len[q] == 0: every slot of the row absent",
    ("idle-wave",): "a wave with no candidate in its slice (r_first >= k)",
    **{("wave-slots", n): "slots a wave walks: one / some / all MP_CPW" for n in ("one", "some", "all")},
    **{("slices", n): "workgroups per query" for n in ("one", "two")},
    **{("blocks", nb): "row blocks loaded in one round" for nb in range(1, MP8_RB + 1)},
    **{("rounds", n): "rounds of MP8_RB row blocks per document" for n in ("one", "two", "many")},
    **{("last-block", kind): "the document's last row block: every row real / rows clamped to the last token" for kind in ("full", "partial")},
    ("partial-round", 7): "a round of 7 row blocks whose last one is partial (97 tokens)",
    ("second-round-of-one",): "a full round, then a round of one partial block (130 tokens)",
    ("one-block-document",): "len <= 16",
    ("truncated",): "a document longer than max_doc_len",
    ("truncated-last",): "the corpus's last document truncated: its clamped rows stop in front of its own poisoned tail",
    ("duplicate",): "the same id twice in a row",
}
K_CLAIMS = dict(P.K_CLAIMS)      # they depend on k and the candidate draws only
M_CLAIMS = {
    512: (*((("blocks", nb)) for nb in range(1, MP8_RB + 1)), ("rounds", "one"), ("rounds", "two"), ("rounds", "many"), ("last-block", "full"),
          ("last-block", "partial"), ("partial-round", 7), ("second-round-of-one",), ("truncated-last",)),
    33: (("blocks", 3), ("blocks", 2), ("blocks", 1), ("rounds", "one"), ("truncated",)),
    16: (("blocks", 1), ("one-block-document",), ("last-block", "full"), ("truncated",)),
    1: (("blocks", 1), ("one-block-document",), ("last-block", "partial"), ("truncated",)),
}


def branches_of(cand, cand_len, id_base, max_doc_len, lens=LENS):
    """The branches one launch lands on (cand [Q, k] ids, cand_len [Q])."""
    Q, k = cand.shape
    plan = pairs_plan(k)
    hit = {("slices", "one" if plan["nslices"] == 1 else "two")}
    for q in range(Q):
        state = slot_state(cand[q], int(cand_len[q]), id_base, lens, max_doc_len)
        if int(cand_len[q]) == 0:
            hit.add(("empty-row",))
        live = [int(c) for c, s in zip(cand[q], state) if s[0] == "doc"]
        if len(set(live)) < len(live):
            hit.add(("duplicate",))
        for wv in plan["waves"]:
            n = len(wv["slots"])
            if n == 0:
                hit.add(("idle-wave",))
                continue
            hit.add(("wave-slots", "one" if n == 1 else "all" if n == MP_CPW else "some"))
            for r in wv["slots"]:
                s = state[r]
                if s[0] == "absent":
                    hit.add(s)
                    continue
                _, pos, length = s
                if lens[pos] > max_doc_len:
                    hit.add(("truncated",))
                    if pos == len(lens) - 1:
                        hit.add(("truncated-last",))
                if length == 0:
                    hit.add(("empty-document",))
                    continue
                rounds = row_blocks(length)
                hit.add(("rounds", "one" if len(rounds) == 1 else "two" if len(rounds) == 2 else "many"))
                hit |= {("blocks", nb) for nb, _ in rounds}
                hit.add(("last-block", "partial" if rounds[-1][1] else "full"))
                if rounds[-1] == (7, True):
                    hit.add(("partial-round", 7))
                if len(rounds) == 2 and rounds[-1] == (1, True):
                    hit.add(("second-round-of-one",))
                if length <= 16:
                    hit.add(("one-block-document",))
    return hit


def sweep_branches():
    """Every branch the whole sweep lands on, and the claims of each k / max_doc_len checked on the way."""
    hit = set()
    by_k = {k: set() for k in KS}
    by_m = {m: set() for m in MAX_DOC_LENS}
    for m in MAX_DOC_LENS:
        for Q in QS:
            for k in KS:
                for id_base in ID_BASES:
                    cand = candidates(Q, k, id_base)
                    for cl in launches(Q, k):
                        b = branches_of(cand, np.full(Q, k) if cl is None else cl, id_base, m)
                        hit |= b; by_k[k] |= b; by_m[m] |= b
    return hit, by_k, by_m


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus_values(max_doc_len):
    """(values [PRE + sum(LENS) + POST, 128] float64, Doff [N + 1] int64) at exponent 0."""
    rng = np.random.default_rng(8000 + max_doc_len)
    Dv, Doff = F.grid_corpus8(rng, LENS, max_doc_len, guards=True, pre=PRE, post=POST)
    Dv.setflags(write=False); Doff.setflags(write=False)
    return Dv, Doff


@functools.lru_cache(maxsize=None)
def query_values(Lq, Q):
    q = F.grid_queries8(np.random.default_rng(800 * Lq + Q), Q, Lq)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def corpus(max_doc_len):
    """(e4m3 bytes [rows, 128] uint8 by the reference quantiser at exponent 0, Doff)."""
    Dv, Doff = corpus_values(max_doc_len)
    D8 = F.quantize_ref(Dv)
    assert np.array_equal(F.dequantize_ref(D8), Dv), "a grid value is not exact in e4m3"
    D8.setflags(write=False)
    return D8, Doff


@functools.lru_cache(maxsize=None)
def queries(Lq, Q):
    Qv = query_values(Lq, Q)
    Q8 = F.quantize_ref(Qv)
    assert np.array_equal(F.dequantize_ref(Q8), Qv), "a grid value is not exact in e4m3"
    Q8.setflags(write=False)
    return Q8


@functools.lru_cache(maxsize=None)
def reference64(Lq, Q, max_doc_len):
    """[Q, N] float64: the formula over the grid values (computed once per shape and shared)."""
    Dv, Doff = corpus_values(max_doc_len)
    ref = M.maxsim_ref(query_values(Lq, Q), Dv, Doff, max_doc_len)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(Lq, Q, max_doc_len):
    """[Q, N] float32, exactly the float64 formula."""
    ref = M.exact_f32(reference64(Lq, Q, max_doc_len))
    ref.setflags(write=False)
    return ref
