"""Cross-encoder pairs from token ids, without a GPU: the restated pair rules (crosspack_cases.keep) against the installed tokenizer and
against CrossEncoder._pair_ids, encode_plain against the tokenizers' own calls, the argument checks of fz_pair_plan / fz_pair_fill
(reported before any HIP call), the Python-level errors, and the build's resource report."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import crosspack_cases as X
from checkpoint_utils import write_monobert_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fz_pair_max_sep", "fz_pair_plan", "fz_pair_fill")
GRID = [(ml, lq, ld) for ml in (8, 9, 12, 13) for lq in range(14) for ld in range(14)]        # 784 cases: even and odd budgets


def _rows(ids, mask):
    return [ids[i, : int(mask[i].sum())].tolist() for i in range(ids.shape[0])]


# ---- the pair rules ---------------------------------------------------------------------------------------------------------------------
def test_longest_first_restated_equals_the_installed_tokenizer(tmp_path):
    from fusion_amd import encoders
    write_monobert_checkpoint(str(tmp_path))
    tok = encoders.from_pretrained(str(tmp_path), "monobert", device="cpu").tokenizer
    spec = tok.pair_spec()
    assert spec == dict(mode="longest_first", nsep=2, bos=0, sep=2, eos=2)
    plain = lambda n, salt: tok.encode_plain([X.text(n, salt)], 64)[0][0, :n].tolist()      # noqa: E731
    assert len(GRID) == 784
    for ml in (8, 9, 12, 13):
        cases = [(lq, ld) for m, lq, ld in GRID if m == ml]
        ids, mask = tok.encode_pairs([X.text(lq, 100 + lq) for lq, _ in cases], [X.text(ld, ld) for _, ld in cases], ml)
        for (lq, ld), row in zip(cases, _rows(ids, mask)):
            kq, ks, kd = X.keep(X.LONGEST_FIRST, ml, 2, lq, ld)
            assert ks == 2 and len(row) == 2 + kq + ks + kd <= ml, (ml, lq, ld)
            assert row == [0] + plain(lq, 100 + lq)[:kq] + [2, 2] + plain(ld, ld)[:kd] + [2], (ml, lq, ld)


def test_tail_restated_equals_pair_ids_with_the_hash_tokenizer():
    from fusion_amd import encoders
    ce = encoders.random_cross_encoder("cpu", "tiny")
    tok = ce.tokenizer
    spec = tok.pair_spec()
    assert spec["mode"] == "tail" and spec["nsep"] == 1 and spec["sep"] == tok._tok("</s>") and (spec["bos"], spec["eos"]) == (tok.bos_id, tok.eos_id)
    plain = lambda n, salt: tok.encode_plain([X.text(n, salt)], 64)[0][0, :n].tolist()      # noqa: E731
    cut_sep = 0
    for ml in (8, 9, 12, 13):
        cases = [(lq, ld) for m, lq, ld in GRID if m == ml]
        ids, mask = ce._pair_ids([(X.text(lq, 100 + lq), X.text(ld, ld)) for lq, ld in cases], ml)
        for (lq, ld), row in zip(cases, _rows(ids, mask)):
            kq, ks, kd = X.keep(X.TAIL, ml, 1, lq, ld)
            cut_sep += ks == 0
            assert len(row) == 2 + kq + ks + kd <= ml, (ml, lq, ld)
            assert row == [spec["bos"]] + plain(lq, 100 + lq)[:kq] + [spec["sep"]] * ks + plain(ld, ld)[:kd] + [spec["eos"]], (ml, lq, ld)
    assert cut_sep > 50                                                                          # the rows where the query fills the row


def test_the_stored_prefix_and_the_full_length_give_the_rule():
    """What the plan computes from a store cut at B tokens plus the lengths before the cut is the rule on the uncut lengths -- and the
    stored prefix alone is not: with an odd budget the odd token goes to the STRICTLY longer sequence."""
    differs = 0
    for mode, nsep in ((X.LONGEST_FIRST, 2), (X.TAIL, 1)):
        for ml, lq, ld in GRID:
            B = X.budget(ml, nsep)
            held = np.array([min(ld, B)])
            cand = np.zeros((1, 1), dtype=np.int64)
            kq, kd, L = X.plan(mode, ml, nsep, cand, None, 0, held, np.array([ld]), [lq], ml - 2)
            a, s, b = X.keep(mode, ml, nsep, lq, ld)
            assert (kq[0, 0], kd[0, 0], L[0, 0]) == (a, b, 2 + a + s + b), (mode, ml, lq, ld)
            differs += X.plan(mode, ml, nsep, cand, None, 0, held, None, [lq], ml - 2)[0][0, 0] != a
    assert differs > 0


def test_encode_plain_is_the_call_minus_its_specials(tmp_path):
    from fusion_amd import encoders
    write_monobert_checkpoint(str(tmp_path))
    texts = ["le chat est un chien", "", "loi", "le juge peut, de droit; un bail !", X.text(30, 3)]
    for tok in (encoders.from_pretrained(str(tmp_path), "monobert", device="cpu").tokenizer, encoders.HashTokenizer(512)):
        full_ids, full_mask = tok(texts, 66)
        want = [r[1:-1] for r in _rows(full_ids, full_mask)]
        for cut in (64, 7, 1, 0):
            ids, lengths = tok.encode_plain(texts, cut)
            assert ids.dtype == torch.int32 and lengths.dtype == torch.int32 and lengths.tolist() == [len(r) for r in want]
            assert ids.shape == (len(texts), min(cut, max(len(r) for r in want)))
            for i, r in enumerate(want):
                k = min(len(r), cut)
                assert ids[i, :k].tolist() == r[:k] and (ids[i, k:] == tok.pad_token_id).all()
        ids, lengths = tok.encode_plain([], 8)
        assert ids.shape == (0, 0) and lengths.shape == (0,)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if not v else C.c_void_p(v)


def plan(L, **kw):
    a = dict(cand=0x1000, ldc=7, cand_len=None, Q=5, W=7, id_base=X.BIG_BASE, Doff=0x2000, full=None, N=23, qlen=0x3000, Lq=16, max_length=16,
             mode=0, nsep=2, kq=0x4000, kd=0x5000, rows=0x6000)
    a.update(kw)
    return L.fz_pair_plan(_p(a["cand"]), a["ldc"], _p(a["cand_len"]), a["Q"], a["W"], a["id_base"], _p(a["Doff"]), _p(a["full"]), a["N"],
                          _p(a["qlen"]), a["Lq"], a["max_length"], a["mode"], a["nsep"], _p(a["kq"]), _p(a["kd"]), _p(a["rows"]), None)


def fill(L, **kw):
    a = dict(pairs=0x1000, cu=0x2000, P=4, T=40, kq=0x3000, kd=0x4000, cand=0x5000, ldc=7, Q=5, W=7, id_base=X.BIG_BASE, qtok=0x6000, ldq=16,
             Lq=16, tok=0x7000, Doff=0x8000, N=23, bos=5, sep=9, eos=6, pad=1, nsep=2, ids=0x9000, pos=0xa000)
    a.update(kw)
    return L.fz_pair_fill(_p(a["pairs"]), _p(a["cu"]), a["P"], a["T"], _p(a["kq"]), _p(a["kd"]), _p(a["cand"]), a["ldc"], a["Q"], a["W"],
                          a["id_base"], _p(a["qtok"]), a["ldq"], a["Lq"], _p(a["tok"]), _p(a["Doff"]), a["N"], a["bos"], a["sep"], a["eos"],
                          a["pad"], a["nsep"], _p(a["ids"]), _p(a["pos"]), None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert set(NEW) <= set(_lib.EXPORTS) and L.fz_abi_version() == 20                                 # additive entries
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    assert all(name + "(" in header for name in NEW)
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    cap = L.fz_pair_max_sep()
    assert cap == 2
    # -- plan: null pointers where a non-empty tensor is needed, leading dimension, negative sizes, the mode, the budget
    for name in ("cand", "qlen", "kq", "kd", "rows", "Doff"):
        assert plan(L, **{name: 0}) == ARG, name
    for name in ("Q", "W", "N", "Lq", "nsep"):
        assert plan(L, **{name: -1}) == ARG, name
    assert plan(L, ldc=6) == ARG and plan(L, mode=2) == ARG and plan(L, mode=-1) == ARG
    assert plan(L, max_length=3) == ARG and plan(L, max_length=3, Q=0) == ARG and plan(L, max_length=2, nsep=1, mode=1) == ARG
    assert plan(L, nsep=cap + 1, max_length=64) == UNS and plan(L, Q=1 << 16, W=1 << 15, ldc=1 << 15) == UNS
    # the order: argument errors, then unsupported shapes, then the empty batch
    assert plan(L, nsep=cap + 1, max_length=64, ldc=6) == ARG and plan(L, Q=0, ldc=6) == ARG and plan(L, Q=0, mode=7) == ARG
    assert plan(L, nsep=cap + 1, max_length=64, Q=0) == UNS and plan(L, nsep=cap + 1, max_length=64, W=0, ldc=0) == UNS
    # nothing to do: no launch, null pointers welcome
    empty = dict(cand=0, qlen=0, kq=0, kd=0, rows=0, Doff=0)
    assert plan(L, Q=0, **empty) == OK and plan(L, W=0, ldc=0, **empty) == OK and plan(L, Q=0, N=0, Doff=0) == OK
    for mode, nsep in ((0, 2), (1, 1), (1, 0)):
        assert plan(L, Q=0, mode=mode, nsep=nsep, max_length=2 + nsep) == OK
    # -- fill
    for name in ("pairs", "cu", "kq", "kd", "cand", "Doff", "ids", "pos", "qtok"):
        assert fill(L, **{name: 0}) == ARG, name
    for name in ("P", "T", "Q", "W", "N", "Lq", "nsep", "bos", "sep", "eos", "pad"):
        assert fill(L, **{name: -1}) == ARG, name
    assert fill(L, ldc=6) == ARG and fill(L, ldq=15) == ARG
    assert fill(L, nsep=cap + 1) == UNS and fill(L, Q=1 << 16, W=1 << 15, ldc=1 << 15) == UNS
    assert fill(L, nsep=cap + 1, ldq=15) == ARG and fill(L, P=0, ldc=6) == ARG and fill(L, nsep=cap + 1, P=0) == UNS
    assert fill(L, P=0) == OK
    assert fill(L, P=0, T=0, pairs=0, cu=0, kq=0, kd=0, cand=0, qtok=0, tok=0, Doff=0, ids=0, pos=0) == OK
    assert fill(L, P=0, Q=0, W=0, ldc=0, N=0, Lq=0, ldq=0) == OK


# ---- Python-level errors -------------------------------------------------------------------------------------------------------------
def _cpu_cross_encoder(**cfg):
    from fusion_amd import encoders
    from transformers import CamembertConfig, CamembertForSequenceClassification
    cfg = dict(dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_labels=1), **cfg)
    torch.manual_seed(0)
    return encoders.CrossEncoder(CamembertForSequenceClassification(CamembertConfig(**cfg)), encoders.HashTokenizer(cfg["vocab_size"]), "cpu",
                                 max_length=16)


def test_python_level_errors():
    from fusion_amd import encoders, ops
    from fusion_amd.distributed import ShardedTextIndex
    tok, Doff = torch.zeros(4, dtype=torch.int32), torch.tensor([0, 1, 4])
    qtok, qlen, cand = torch.zeros((2, 3), dtype=torch.int32), torch.ones(2, dtype=torch.int32), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="GPU"):
        ShardedTextIndex(tok, Doff, 0)                                                                 # there is no CPU path
    with pytest.raises(TypeError, match="GPU"):
        ops.pair_plan(cand, None, Doff, None, 0, qlen, 3, 16, "tail", 1)
    with pytest.raises(ValueError, match="mode"):
        ops.pair_plan(cand, None, Doff, None, 0, qlen, 3, 16, "shortest_first", 1)                     # the mode is looked at first
    with pytest.raises(TypeError, match="GPU"):
        ops.pair_fill(torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 0, cand.int(), cand.int(), cand, 0, qtok, tok, Doff,
                      5, 9, 6, 1, 1)
    ce = _cpu_cross_encoder()
    assert ce.amp is False and _cpu_cross_encoder().max_length == 16
    index = SimpleNamespace(tok=tok, Doff=Doff, full_len=None, id_base=0)
    with pytest.raises(TypeError, match="GPU"):
        ce.score_candidates(index, qtok, qlen, cand)
    with pytest.raises(TypeError, match="GPU"):
        ShardedTextIndex.from_texts(ce, ["le chat", "la loi"])
    # refused whatever the tensors are: more than one token type (the packed forward carries type 0 only), more than one label
    with pytest.raises(ValueError, match="token types"):
        _cpu_cross_encoder(type_vocab_size=2).score_candidates(index, qtok, qlen, cand)
    with pytest.raises(ValueError, match="labels"):
        _cpu_cross_encoder(num_labels=3).score_candidates(index, qtok, qlen, cand)
    assert encoders.CrossEncoder(ce.model, ce.tokenizer, "cpu", amp=True).amp is False                  # mixed precision is the GPU forward's


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
def test_the_crosspack_kernels_hold_everything_in_registers(tmp_path):
    """The report the compile left next to the object (fusion_amd/csrc/crosspack.res); if the objects predate it, the one source is compiled
    once more into a temporary directory -- never into the tree -- as tests/test_forward_cpu.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if "crosspack" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no crosspack.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "crosspack.hip"), "-o", str(tmp_path / "crosspack.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "crosspack.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    mine = {kernel_resources.short(n): r for n, r in res["crosspack"].items()}
    assert len(mine) == 2 and any("pair_plan_kernel" in n for n in mine) and any("pair_fill_kernel" in n for n in mine), sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("lds", 0) == 0, f"{name}: {r}"
        assert r["vgprs"] + r.get("agprs", 0) <= 64, (name, r)                                          # integer index work: full occupancy
