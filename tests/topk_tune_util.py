"""Shared by tests/test_lists_tune_cpu.py and tests/test_gpu_lists_tune.py: loading the topktune_*.npz fixtures (the reference's
weight-grid loop on the lists of a topkfuse_*.npz case: tools/gen_golden_topktune.py) and the rule both files compare metrics by."""
import os

import numpy as np

from topk_fuse_util import Case

NORMS = ["min-max", "z-score", "arctan", "percentile-rank", "normal-curve-equivalent", "none"]
FIVE = NORMS[:5]


class TuneCase:
    def __init__(self, path):
        self.z = z = np.load(path, allow_pickle=False)
        base = Case(os.path.join(os.path.dirname(path), os.path.basename(path).replace("topktune_", "topkfuse_")))
        keep = z["queries"].astype(np.int64)
        self.systems = [str(s) for s in z["systems"]]
        assert self.systems == base.systems
        self.ids, self.scores, self.lens = base.ids[:, keep], base.scores[:, keep], base.lens[:, keep]     # [S, Q, L], [S, Q]
        self.Q = len(keep)
        self.distr = base.distr
        self.labels = [[int(x) for x in str(s).split(",")] for s in z["labels"]]
        self.weights = z["weights"]
        self.metric_names = [str(x) for x in z["metric_names"]]
        self.raises = set(str(x) for x in z["raises"])

    def lists(self) -> dict:
        return {s: [[{"corpus_id": int(self.ids[si, q, r]), "score": float(self.scores[si, q, r])} for r in range(self.lens[si, q])]
                    for q in range(self.Q)] for si, s in enumerate(self.systems)}

    def grid(self, kind=np.float64) -> list:
        return [{s: kind(w) for s, w in zip(self.systems, row)} for row in self.weights]


def defined_rows(case, norm):
    """The weight vectors whose metrics the reference defines.  Under NCE a zero weight meets a real -inf (-inf * 0 = NaN keys handed
    to sorted(); tests/test_gpu_parity_r2.py::test_tune_matches_reference_loop excludes the same rows); and whenever the reference's
    own fused lists held a NaN score (the fixture's nan__<norm> mask: the z-score of a single-entry list) its sorted() compared NaN
    keys as well -- the stored order is an artefact of timsort's comparison sequence, which nothing reproduces."""
    ok = ~case.z[f"nan__{norm}"]
    return ok & np.all(case.weights != 0.0, axis=1) if norm == "normal-curve-equivalent" else ok


def metric_rows(results, names):
    assert all(list(r) == names for r in results)
    assert all(type(v) is float for r in results for v in r.values())
    return np.array([[r[k] for k in names] for r in results], dtype=np.float64).reshape(len(results), len(names))
