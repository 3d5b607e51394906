"""Shared by tests/test_lists_join_cpu.py and tests/test_gpu_lists_fusion.py: loading the list-form fusion fixtures (fuse_*.npz /
topkfuse_*.npz: inputs and the reference's own outputs) and the comparison rule of tests/test_gpu_parity.py -- ranked-list identity,
ids and scores bit for bit, for rrf / bcf / nsf-none / nsf-min-max / nsf-percentile-rank; the scores looked up by id within 2e-6
(z-score), 1e-6 (arctan), 1e-4 (NCE) with the same id set and the same finiteness otherwise."""
import numpy as np

METHODS = [("rrf", "none"), ("bcf", "none"), ("nsf", "none"), ("nsf", "min-max"), ("nsf", "z-score"), ("nsf", "arctan"),
           ("nsf", "percentile-rank"), ("nsf", "normal-curve-equivalent")]
EXACT = {("rrf", "none"), ("bcf", "none"), ("nsf", "none"), ("nsf", "min-max"), ("nsf", "percentile-rank")}
TOL = {("nsf", "z-score"): 2e-6, ("nsf", "arctan"): 1e-6, ("nsf", "normal-curve-equivalent"): 1e-4}


class Case:
    def __init__(self, path):
        z = np.load(path, allow_pickle=False)
        self.z = z
        self.systems = [str(s) for s in z["systems"]]
        self.ids, self.scores, self.lens = z["in_ids"], z["in_scores"], z["in_len"]   # [S, Q, L] int64 / float64, [S, Q]
        self.Q = self.ids.shape[1]
        self.weights = {s: float(w) for s, w in zip(self.systems, z["weights"])}
        self.distr = {s: z[f"distr_{s}"] for s in self.systems}
        self.raises = set(str(x) for x in z["raises"]) if "raises" in z.files else set()

    def max_entries(self) -> int:
        """The largest number of entries one query's lists hold together."""
        return int(self.lens.sum(0).max()) if self.Q else 0

    def lists(self) -> dict:
        return {s: [[{"corpus_id": int(self.ids[si, q, r]), "score": float(self.scores[si, q, r])} for r in range(self.lens[si, q])]
                    for q in range(self.Q)] for si, s in enumerate(self.systems)}

    def expected(self, pair, oracle):
        """The fused lists a pair must give: the reference's stored output, or -- for a pair the reference raised on (an empty list
        under min-max) -- the project's rule, oracle.fuse_lists."""
        method, norm = pair
        key = f"{method}__{norm}"
        if key in self.raises:
            assert f"out_ids__{key}" not in self.z.files
            return lists_of(oracle.fuse_lists(self.lists(), method, norm, self.weights, self.distr))
        e_ids, e_sc, e_len = self.z[f"out_ids__{key}"], self.z[f"out_scores__{key}"], self.z[f"out_len__{key}"]
        return [(e_ids[q, :int(e_len[q])], e_sc[q, :int(e_len[q])]) for q in range(self.Q)]


def lists_of(fused) -> list:
    """list[Q] of list of {'corpus_id', 'score'} -> list[Q] of (ids int64, scores float64)."""
    return [(np.array([x["corpus_id"] for x in l], dtype=np.int64), np.array([float(x["score"]) for x in l], dtype=np.float64)) for l in fused]


def assert_fused_equal(got, exp, pair, what=""):
    """got / exp: list[Q] of (ids, scores).  The rule of tests/test_gpu_parity.py::test_aggregator_matches_reference_golden."""
    assert len(got) == len(exp), (what, pair)
    for q, ((g_ids, g_sc), (e_ids, e_sc)) in enumerate(zip(got, exp)):
        assert len(g_ids) == len(e_ids), (what, pair, q, len(g_ids), len(e_ids))
        if pair in EXACT:
            np.testing.assert_array_equal(g_ids, e_ids, err_msg=f"{what} {pair} q={q}")      # ranked-list identity
            np.testing.assert_array_equal(g_sc, e_sc, err_msg=f"{what} {pair} q={q}")
        else:
            assert sorted(g_ids.tolist()) == sorted(e_ids.tolist()), (what, pair, q)
            ref_of = {int(i): s for i, s in zip(e_ids, e_sc)}
            ref = np.array([ref_of[int(i)] for i in g_ids], dtype=np.float64)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(g_sc), fin), (what, pair, q)
            assert np.max(np.abs(g_sc[fin] - ref[fin]), initial=0.0) <= TOL[pair], (what, pair, q)
