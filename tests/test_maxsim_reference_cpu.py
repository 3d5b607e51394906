"""The yardstick of test_gpu_maxsim_edges.py, checked without a GPU: the float64 reference against the CPU oracle, the exactness claim
of the grid inputs, and the pure-Python restatement of the launcher that tells which branch of maxsim_kernel a case lands on."""
import numpy as np
import pytest

import maxsim_cases as M


@pytest.mark.parametrize("Lq", M.LQS)
def test_reference_equals_the_oracle_on_grid_inputs(oracle, Lq):
    rng = np.random.default_rng(Lq)
    lens = M.alternate((40, 0, 17, 70, 5, 33, 64, 1, 200))
    Qtok = M.grid_queries(rng, 9, Lq)
    Dtok, Doff = M.grid_corpus(rng, lens, 100)          # the 200-token document ends in poison: the oracle does not truncate
    ref = M.maxsim_ref(Qtok, Dtok, Doff, None)
    got = oracle.maxsim(Qtok.astype(np.float32), Dtok.astype(np.float32), Doff)
    assert np.array_equal(got, M.exact_f32(ref))
    assert len(np.unique(ref[:, ::2])) > ref[:, ::2].size // 2, "the clean scores do not discriminate"
    cut = M.maxsim_ref(Qtok, Dtok, Doff, 100)
    assert np.array_equal(cut[:, :16], ref[:, :16]) and np.all(ref[:, 16] - cut[:, 16] > 900 * Lq)   # the poisoned tail is worth ~1024 a token


@pytest.mark.parametrize("Lq", M.LQS)
def test_reference_is_close_to_the_oracle_on_unit_norm_inputs(oracle, Lq):
    rng = np.random.default_rng(Lq + 1)
    Qtok = M.unit_queries(rng, 7, Lq)
    Dtok, Doff = M.unit_corpus(rng, [int(x) for x in rng.integers(0, 150, 40)])
    ref = M.maxsim_ref(Qtok, Dtok, Doff, None)
    got = oracle.maxsim(Qtok.astype(np.float32), Dtok.astype(np.float32), Doff)     # accumulates in fp32
    assert np.max(np.abs(got - ref)) <= 1e-5


def test_reference_truncates_and_skips_rows_outside_the_documents():
    rng = np.random.default_rng(3)
    Qtok = M.unit_queries(rng, 3, 32)
    Dtok, Doff = M.unit_corpus(rng, [5, 0, 9, 2], pre=4, post=6)
    ref = M.maxsim_ref(Qtok, Dtok, Doff, 3)
    q, d = Qtok.astype(np.float64), Dtok.astype(np.float64)
    for j, (a, L) in enumerate(((4, 3), (9, 0), (9, 3), (18, 2))):
        exp = [sum(max(float(q[i, t] @ d[a + k]) for k in range(L)) for t in range(32)) if L else 0.0 for i in range(3)]
        assert np.allclose(ref[:, j], exp, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_grid_case_is_exact_in_float32_and_lands_its_branches(case):
    """float32(ref) == ref at every size the GPU module uses, poison included; the clean documents of a poisoned corpus stay below the
    poison; the case lands on the branches it claims."""
    Qtok, Dtok, Doff = case.inputs()
    ref = M.maxsim_ref(Qtok, Dtok, Doff, case.max_doc_len)
    M.exact_f32(ref)
    assert np.abs(ref).max() < 2 ** 18
    if case.guards:
        lens = np.asarray(case.lens)
        clean, guard = ref[:, 0::2], ref[:, 1::2]
        assert np.all(clean < 128 * case.Lq)
        assert np.all(guard[:, lens[1::2] > 0] > 800 * case.Lq)
    b = M.branches_of(case)
    assert set(case.claims) and set(case.claims) <= b, sorted(map(str, set(case.claims) - b))


def test_branch_table_is_covered():
    hit = set().union(*(M.branches_of(c) for c in M.CASES))
    assert set(M.BRANCHES) <= hit, sorted(map(str, set(M.BRANCHES) - hit))
    # what the issue of this module lists, spelled out
    for Lq in M.LQS:
        assert {h[2] for h in hit if h[:2] == ("nq", Lq)} == set(range(128 // Lq + 1))
        assert {h[2] for h in hit if h[:2] == ("tiles", Lq)} >= set(M.TILE_COUNTS) | {512}
    assert {h[2] for h in hit if h[0] == "ncb"} == {0, 2, 4, 6, 8}
    assert ("nq", 32, 1) in hit and ("nq", 32, 3) in hit


@pytest.mark.parametrize("Lq", M.LQS)
def test_launch_plan_gives_every_query_to_one_wave(Lq):
    for Q in range(1, 200):
        p = M.launch_plan(Q, Lq, (1,), 512)
        owned = [q for w in p["waves"] for q in range(w["q0"], w["q0"] + w["nq"])]
        assert owned == list(range(Q))
        assert all(w["nq"] <= p["qpw"] and w["ncb"] in (0, 2, 4, 6, 8) for w in p["waves"])
        assert p["blocks"] == 8 * p["QG"] and len(p["waves"]) == 8 * p["QG"]


def test_launch_plan_documents_per_workgroup():
    for m, dpw in list(M.DOCS_PER_WG.items()) + [(1, 32), (480, 32), (544, 30), (8192, 2), (8193, 1)]:
        p = M.launch_plan(1, 64, (m,) * 70, m)
        assert p["docs_per_wg"] == dpw and p["DR"] == -(-70 // dpw)
        assert max(len(r["tiles"]) for r in p["ranges"]) <= M.MS_TABLE


def test_special_value_inputs_mean_what_the_gpu_test_says():
    Qtok, Dtok, Doff = M.special_inputs()
    ref = M.maxsim_ref(Qtok, Dtok, Doff, 512)
    M.check_special_reference(ref)
    pinned = M.maxsim_fmax_ref(Qtok, Dtok, Doff)
    defined = ~np.isnan(ref)
    assert np.array_equal(ref[defined], pinned[defined]) and np.isneginf(pinned[:, 3]).all() and np.isfinite(pinned[:, 2]).all()
