"""Inputs, expectation and case table of the candidate-list MaxSim tests (test_gpu_maxsim_pairs.py on the GPU, test_maxsim_pairs_cpu.py
without one).  Not collected by pytest.  Corpus, queries and the float64 reference come from maxsim_cases.py, unchanged.

The corpus: clean documents of every EDGE_LENS length and three empty ones at the even positions, poison-only guard documents at the odd
ones, 37 poisoned rows before Doff[0], 41 after Doff[N], and a last clean document of 530 tokens that every max_doc_len of the sweep
truncates, so its tail -- the last rows any document owns -- is poison as well.

The case table restates the launch arithmetic of csrc/maxsim_pairs.h (with rerank.hip's 4 row blocks in flight) in plain Python
(pairs_plan) and names, for every k and max_doc_len of the sweep, the wave-uniform branches of the kernel that value is there for (K_CLAIMS, M_CLAIMS; branches_of checks them); BRANCHES lists
every branch the sweep as a whole must land on."""
import functools

import numpy as np

import maxsim_cases as M

# csrc/maxsim_pairs.h; MP_RB: csrc/rerank.hip
MP_WAVES, MP_CPW, MP_RB = 4, 32, 4
MP_SLICE = MP_WAVES * MP_CPW

QS = (1, 2, 5, 9)
KS = (1, 2, 7, 64, 65, 100, 130)       # 130: a second slice with two slots, past the issue's list (every k <= 128 is one workgroup per query)
MAX_DOC_LENS = (512, 33, 16, 1)
ID_BASES = (0, 2 ** 33 + 5)
CLEAN = M.EDGE_LENS + (0, 40, 0, 0, 530)
LENS = M.alternate(CLEAN)[:-1]         # 39 documents; the last one is the clean 530-token document
PRE, POST = 37, 41
SENTINEL = 12345.0


# ---- the launcher and the kernel's loop structure, restated ----------------------------------------------------------------------
def pairs_plan(k):
    """What fz_maxsim_pairs_f16 and maxsim_pairs_kernel derive from k for one query: per slice and wave, the slots the wave walks."""
    nslices = -(-k // MP_SLICE)
    waves = []
    for sl in range(nslices):
        for w in range(MP_WAVES):
            r_first = sl * MP_SLICE + w
            if r_first >= k:
                waves.append(dict(slice=sl, w=w, slots=[]))
                continue
            nmine = min(-(-(k - r_first) // MP_WAVES), MP_CPW)
            waves.append(dict(slice=sl, w=w, slots=[r_first + MP_WAVES * i for i in range(nmine)]))
    return dict(nslices=nslices, waves=waves)


def row_blocks(length):
    """The kernel's walk over one document of `length` (> 0) tokens: per round of up to MP_RB row blocks, (blocks loaded, whether the
    last of them is partial, i.e. has rows clamped to the document's last token)."""
    out = []
    for c0 in range(0, length, 16 * MP_RB):
        nb = (length - c0 + 15) >> 4
        out.append((min(nb, MP_RB), nb <= MP_RB and length % 16 != 0))
    return out


def slot_state(cand_row, cand_len, id_base, lens, max_doc_len):
    """Per slot of one row: ('absent', why) or ('doc', position, effective length)."""
    out = []
    N = len(lens)
    for r, cid in enumerate(cand_row):
        cid = int(cid)
        if r >= cand_len:
            out.append(("absent", "past-cand_len"))
        elif cid < 0:
            out.append(("absent", "negative-id"))
        elif cid - id_base < 0:
            out.append(("absent", "below-id_base"))
        elif cid - id_base >= N:
            out.append(("absent", "past-N"))
        else:
            out.append(("doc", cid - id_base, min(int(lens[cid - id_base]), max_doc_len)))
    return out


BRANCHES = {
    **{("absent", why): "a slot that gets -inf" for why in ("past-cand_len", "negative-id", "below-id_base", "past-N")},
    ("empty-document",): "len == 0: the score is 0, nothing is loaded",
    ("empty-row",): "cand_len[q] == 0: every slot of the row absent",
    ("idle-wave",): "a wave with no candidate in its slice (r_first >= k)",
    **{("wave-slots", n): "slots a wave walks: one / some / all MP_CPW" for n in ("one", "some", "all")},
    **{("slices", n): "workgroups per query" for n in ("one", "two")},
    **{("blocks", nb): "row blocks loaded in one round" for nb in range(1, MP_RB + 1)},
    **{("rounds", n): "rounds of MP_RB row blocks per document" for n in ("one", "two", "many")},
    **{("last-block", kind): "the document's last row block: every row real / rows clamped to the last token" for kind in ("full", "partial")},
    ("one-block-document",): "len <= 16",
    ("truncated",): "a document longer than max_doc_len",
    ("truncated-last",): "the corpus's last document truncated: its clamped rows stop in front of its own poisoned tail",
    ("duplicate",): "the same id twice in a row",
}
K_CLAIMS = {
    1: (("idle-wave",), ("wave-slots", "one")),
    2: (("idle-wave",), ("duplicate",)),
    7: (("absent", "negative-id"), ("absent", "below-id_base"), ("absent", "past-N"), ("wave-slots", "some")),
    64: (("wave-slots", "some"), ("slices", "one")),
    65: (("wave-slots", "some"), ("absent", "past-cand_len")),
    100: (("empty-document",), ("slices", "one")),
    130: (("slices", "two"), ("wave-slots", "all"), ("idle-wave",)),
}
M_CLAIMS = {
    512: (("blocks", 4), ("rounds", "many"), ("rounds", "two"), ("last-block", "full"), ("last-block", "partial"), ("truncated-last",)),
    33: (("blocks", 3), ("blocks", 2), ("rounds", "one"), ("truncated",)),
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
                if length <= 16:
                    hit.add(("one-block-document",))
    return hit


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(max_doc_len):
    rng = np.random.default_rng(4000 + max_doc_len)
    Dtok, Doff = M.grid_corpus(rng, LENS, max_doc_len, guards=True, pre=PRE, post=POST)
    Dtok.setflags(write=False); Doff.setflags(write=False)
    return Dtok, Doff


@functools.lru_cache(maxsize=None)
def queries(Lq, Q):
    q = M.grid_queries(np.random.default_rng(100 * Lq + Q), Q, Lq)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def reference(Lq, Q, max_doc_len):
    """[Q, N] float32, exactly the float64 formula (computed once per shape and shared)."""
    Dtok, Doff = corpus(max_doc_len)
    ref = M.exact_f32(M.maxsim_ref(queries(Lq, Q), Dtok, Doff, max_doc_len))
    ref.setflags(write=False)
    return ref


def candidates(Q, k, id_base, N=len(LENS)):
    """Seeded draws with repetition over all N documents (row 0 of a k >= N launch lists every document first), then the slots the
    sweep must hold: the same id twice, -1 in the middle and at the tail, the ids just outside the shard on either side."""
    rng = np.random.default_rng(7919 * Q + k)
    pos = rng.integers(0, N, (Q, k)).astype(np.int64)
    if k >= N:
        pos[0, :N] = rng.permutation(N)
    if k >= 64:
        pos[Q - 1, 4:4 + len(CLEAN)] = 2 * rng.permutation(len(CLEAN))      # every clean document in the last row
    cand = pos + id_base
    if k >= 2:
        cand[0, 1] = cand[0, 0]
    if k >= 7:
        for q in range(Q):
            cand[q, 2 + q % 2] = id_base - 1
            cand[q, 3 - q % 2] = id_base + N
            cand[q, k // 2 + 2] = -1
            cand[q, k - 1] = -1
    return cand


def cand_lens(Q, k):
    """Row lengths of the second launch: shorter than k, 0, k, k - 1, 1, ... over the rows (Q = 1: the short one; its empty row is a launch
    of its own, zero_lens)."""
    pattern = (k // 2, 0, k, max(k - 1, 0), min(k, 1))
    return np.array([pattern[q % len(pattern)] for q in range(Q)], dtype=np.int32)


def expected(ref, cand, cand_len, id_base):
    """The scores the kernel must give, from the [Q, N] reference plane: -inf for every absent slot."""
    Q, k = cand.shape
    N = ref.shape[1]
    out = np.full((Q, k), -np.inf, dtype=np.float32)
    for q in range(Q):
        for r in range(min(int(cand_len[q]), k)):
            cid = int(cand[q, r])
            if cid >= 0 and 0 <= cid - id_base < N:
                out[q, r] = ref[q, cid - id_base]
    return out


def launches(Q, k):
    """(cand_len or None) of the launches run for one (Q, k)."""
    out = [None, cand_lens(Q, k)]
    if Q == 1:
        out.append(np.zeros(1, dtype=np.int32))
    return out


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
