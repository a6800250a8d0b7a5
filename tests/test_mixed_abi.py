"""CPU: the mixed-code batches' ABI (include/quic_fec.h, "Mixed-code batches"): the symbols, their
ctypes rows against the header's declarations, qfec_mixed_layout against a Python restatement,
the wrappers' array checks before the library is touched, and the construction of
tests/test_gpu_mixed.py's batches from the oracle alone."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from quic_amd import _lib, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qfec_codeset_create", "qfec_codeset_destroy", "qfec_codeset_dims",
           "qfec_codeset_reserve", "qfec_mixed_layout", "qfec_encode_batch_mixed",
           "qfec_decode_batch_mixed_recovered", "qfec_encode_batch_mixed_host",
           "qfec_decode_batch_mixed_recovered_host"]
PRESETS = [(5, 5), (10, 10), (10, 15), (10, 20), (15, 15), (250, 5)]


def _ctype(arg):
    """The ctypes type the table holds for one parameter of a declaration."""
    arg = " ".join(arg.split())
    if "*" in arg or "[" in arg:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong}[arg.rsplit(" ", 1)[0]]


def test_symbols_exported_declared_and_typed():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "quic_fec.h")) as f:
        text = f.read()
    for s in SYMBOLS:
        assert s in exported, s
        decl = re.search(r"QFEC_API (int|void) %s\(([^;]*)\);" % s, text)
        assert decl, s
        res, args = _lib.SIGNATURES[s]
        assert res is (ctypes.c_int if decl.group(1) == "int" else None)
        want = [_ctype(a) for a in decl.group(2).split(",")]
        # out-parameters are typed pointers in the table
        got = [ctypes.c_void_p if isinstance(a, type(ctypes.POINTER(ctypes.c_int))) else a
               for a in args]
        assert got == want, s
    assert "Mixed-code batches" in text and "typedef struct qfec_codeset qfec_codeset;" in text
    for name in ("codeset", "encode_mixed", "decode_mixed_recovered"):
        assert callable(getattr(fec.FecEngine, name))
    for name in ("mixed_layout", "encode_mixed_host_into", "decode_mixed_recovered_host_into"):
        assert callable(getattr(fec, name))
    # the queue's switch: exported, declared in the group layer's header, typed
    from quic_amd import fec_group
    with open(os.path.join(ROOT, "include", "quic_fec_group.h")) as f:
        assert "QFEC_API int qfec_batch_set_mixed(qfec_batch *b, int on);" in f.read()
    assert "qfec_batch_set_mixed" in exported
    assert fec_group._SIG["qfec_batch_set_mixed"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert callable(fec_group.FecBatch.set_mixed)


def test_null_arguments_are_minus_two():
    L = _lib.load()
    h = ctypes.c_void_p()
    k = (ctypes.c_int * 1)(5)
    assert L.qfec_codeset_create(None, 1, k, k, ctypes.byref(h)) == -2
    assert L.qfec_codeset_dims(None, None, None, None) == -2
    assert L.qfec_codeset_reserve(None, 1) == -2
    L.qfec_codeset_destroy(None)
    assert L.qfec_encode_batch_mixed(None, None, 0, None, None, None, None, None, None, None,
                                     None) == -2
    assert L.qfec_decode_batch_mixed_recovered(None, None, 0, None, None, None, None, None, None,
                                               None, None, None, None) == -2


def layout_py(codes, code, bb):
    """qfec_mixed_layout restated: k_g, m_g and min(k_g, m_g) blocks of bb[g] bytes per group,
    every group rounded up to 16 bytes."""
    offs, run = ([], [], []), [0, 0, 0]
    for c, b in zip(code, bb):
        k, m = codes[c]
        for a, n in enumerate((k, m, min(k, m))):
            offs[a].append(run[a])
            run[a] = (run[a] + n * int(b) + 15) & ~15
    return [np.array(o, np.int64) for o in offs], tuple(run)


def test_mixed_layout_matches_restatement():
    rng = np.random.default_rng(5)
    codes = PRESETS + [(1, 3), (10, 1), (250, 7)]
    code = rng.integers(0, len(codes), 500).astype(np.uint8)
    bb = rng.integers(1, 2100, 500).astype(np.int32)
    d, p, r, totals = fec.mixed_layout(codes, code, bb)
    offs, run = layout_py(codes, code, bb)
    for got, want in zip((d, p, r), offs):
        np.testing.assert_array_equal(got, want)
        assert (got % 16 == 0).all()
    assert totals == run and all(t % 16 == 0 for t in totals)
    # one code: qfec_ragged_layout's answer
    one = fec.mixed_layout([(10, 20)], np.zeros(500, np.uint8), bb)
    rag = fec.ragged_layout(10, 20, bb)
    for got, want in zip(one[:3], rag[:3]):
        np.testing.assert_array_equal(got, want)
    assert one[3] == rag[3]
    # G = 0
    assert fec.mixed_layout(codes, np.zeros(0, np.uint8), np.zeros(0, np.int32))[3] == (0, 0, 0)


def test_mixed_layout_errors():
    good = ([(5, 5), (10, 1)], np.array([0, 1, 1], np.uint8), np.array([8, 1, 1352], np.int32))
    fec.mixed_layout(*good)
    for codes, code, bb in [
            (good[0], np.array([0, 2, 1], np.uint8), good[2]),          # code index out of range
            (good[0], np.array([0, 255, 1], np.uint8), good[2]),
            (good[0], good[1], np.array([8, 0, 1352], np.int32)),       # bb < 1
            (good[0], good[1], np.array([8, -5, 1352], np.int32)),
            ([], np.zeros(0, np.uint8), np.zeros(0, np.int32)),         # ncodes 0
            ([(5, 5)] * 33, good[1], good[2]),                          # ncodes 33
            ([(0, 5), (10, 1)], good[1], good[2]),                      # bad codes
            ([(256, 5), (10, 1)], good[1], good[2]),
            ([(5, 0), (10, 1)], good[1], good[2])]:
        with pytest.raises(ValueError):
            fec.mixed_layout(codes, code, bb)
    # overflow: 2^31 - 1 parity blocks of 2^31 - 1 bytes are 2^62 bytes a group; the third group
    # passes 2^63
    big = [(255, 2 ** 31 - 1)]
    fec.mixed_layout(big, np.zeros(1, np.uint8), np.full(1, 2 ** 31 - 1, np.int32))
    with pytest.raises(ValueError):
        fec.mixed_layout(big, np.zeros(3, np.uint8), np.full(3, 2 ** 31 - 1, np.int32))
    with pytest.raises(ValueError):
        fec.mixed_layout(good[0], good[1][:2], good[2])                 # lengths differ
    # the C entry point itself: NULL arrays and groups < 0
    L = _lib.load()
    k = np.array([5], np.int32)
    assert L.qfec_mixed_layout(1, None, fec._vp(k), 0, None, None, None, None, None, None) == -2
    assert L.qfec_mixed_layout(1, fec._vp(k), fec._vp(k), -1, None, None, None, None, None,
                               None) == -2
    assert L.qfec_mixed_layout(1, fec._vp(k), fec._vp(k), 1, None, None, None, None, None,
                               None) == -2
    assert L.qfec_mixed_layout(1, fec._vp(k), fec._vp(k), 0, None, None, None, None, None,
                               None) == 0


def test_wrappers_check_arrays_before_the_call():
    """dtype and shape of code, bb, the offsets, rows, rec_rows and status: neither the engine nor
    the set is touched (None / a stand-in), so a wrong argument cannot reach the library."""
    import torch
    G, kmax, rmax = 4, 32, 10
    cs = types.SimpleNamespace(_h=None, kmax=kmax, rmax=rmax)
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    good = dict(code=torch.zeros(G, dtype=u8), bb=torch.full((G,), 64, dtype=i32),
                buf=torch.zeros(4096, dtype=u8), off=torch.zeros(G, dtype=i64),
                rows=torch.zeros((G, kmax), dtype=u8), rr=torch.zeros((G, rmax), dtype=u8),
                st=torch.zeros(G, dtype=i32))

    def enc(a):
        fec.FecEngine.encode_mixed(None, cs, a["code"], a["bb"], a["buf"], a["off"], a["buf"],
                                   a["off"], status=a["st"])

    def dec(a):
        fec.FecEngine.decode_mixed_recovered(None, cs, a["code"], a["bb"], a["buf"], a["off"],
                                             a["rows"], a["buf"], a["off"], a["rr"],
                                             status=a["st"])

    bad_both = [dict(code=good["code"].to(i32)), dict(code=good["code"].to(torch.int8)),
                dict(code=torch.zeros((G, 1), dtype=u8)), dict(code=good["code"].numpy()),
                dict(code=None), dict(code=[0] * G),
                dict(bb=good["bb"].to(i64)), dict(bb=good["bb"][:-1]),
                dict(off=good["off"].to(i32)), dict(off=torch.zeros(G + 1, dtype=i64)),
                dict(st=good["st"].to(i64)), dict(st=good["st"][:-1])]
    bad_dec = [dict(rows=torch.zeros((G, kmax - 1), dtype=u8)),       # not [G][kmax]
               dict(rows=torch.zeros((G, 5), dtype=u8)), dict(rows=torch.zeros(G * kmax, dtype=u8)),
               dict(rows=torch.zeros((G + 1, kmax), dtype=u8)), dict(rows=good["rows"].to(i32)),
               dict(rr=torch.zeros((G, rmax + 1), dtype=u8)), dict(rr=good["rr"].to(i32))]
    for call, bad in ((enc, bad_both), (dec, bad_both + bad_dec)):
        for b in bad:
            with pytest.raises((TypeError, ValueError)) as e:
                call(dict(good, **b))
            assert "ROCm device" not in str(e.value), b     # refused for what is wrong with it
        # everything right but the device: refused where the pointer is taken, before the call
        with pytest.raises(TypeError, match="ROCm device"):
            call(good)


def test_host_wrappers_check_arrays_before_the_call():
    """The host forms: every array is a contiguous CPU tensor of its dtype and shape, sizes are
    >= 1, offsets multiples of 16, and every group lies inside its buffer (by its code's block
    count), before the library is touched (the engine is None)."""
    import torch
    codes = [(5, 5), (10, 1), (250, 5)]
    cs = types.SimpleNamespace(_h=None, kmax=250, rmax=5, codes=codes)
    code = np.array([0, 2, 1, 3], np.uint8)                # the last names no code: no blocks
    bb = np.array([64, 8, 24, 64], np.int32)
    d, p, r, tot = fec.mixed_layout(codes + [(1, 1)], code, bb)
    t = torch.from_numpy
    good = dict(code=t(code), bb=t(bb), data=torch.zeros(tot[0] - 64, dtype=torch.uint8),
                d_off=t(d), par=torch.zeros(tot[1] - 64, dtype=torch.uint8), p_off=t(p),
                rec=torch.zeros(tot[2] - 64, dtype=torch.uint8), r_off=t(r),
                rows=torch.zeros((4, 250), dtype=torch.uint8),
                rr=torch.zeros((4, 5), dtype=torch.uint8), st=torch.zeros(4, dtype=torch.int32))

    def enc(a):
        fec.encode_mixed_host_into(None, cs, a["code"], a["bb"], a["data"], a["d_off"], a["par"],
                                   a["p_off"], a["st"])

    def dec(a):
        fec.decode_mixed_recovered_host_into(None, cs, a["code"], a["bb"], a["data"], a["d_off"],
                                             a["rows"], a["rec"], a["r_off"], a["rr"], a["st"])

    bad_enc = [dict(code=good["code"].to(torch.int32)), dict(code=good["code"][:-1]),
               dict(code=code), dict(bb=good["bb"].to(torch.int64)), dict(bb=t(np.array([64, 0, 24, 64], np.int32))),
               dict(d_off=good["d_off"] + 8), dict(d_off=good["d_off"].to(torch.int32)),
               dict(data=good["data"][:-16]), dict(par=good["par"][:-16]),
               dict(st=torch.zeros(5, dtype=torch.int32))]
    bad_dec = [dict(rows=torch.zeros((4, 5), dtype=torch.uint8)), dict(rec=good["rec"][:-16]),
               dict(rr=torch.zeros((4, 250), dtype=torch.uint8)), dict(code=good["code"].to(torch.int8))]
    for call, bad in ((enc, bad_enc), (dec, bad_dec)):
        for b in bad:
            with pytest.raises((TypeError, ValueError)):
                call(dict(good, **b))
        with pytest.raises(AttributeError):                # every check passed: the engine is None
            call(good)


def test_gpu_batch_construction(oracle):
    """tests/test_gpu_mixed.py's main batch, from the oracle alone: every group built as
    decodable has oracle status 0, every kind occurs at least twice, every code at least four
    times, the special groups are there, and the shuffle mixes the codes."""
    from tests import test_gpu_mixed as M
    from tests.test_gpu_ragged import GF_SIZES, KINDS, POISON
    for seed in (1, 2):
        c = M.main_case(oracle, seed)
        G, nc = c["G"], len(M.CODES)
        assert G == 72 + 5
        assert (c["dec_status"][c["decodable"]] == 0).all() and c["decodable"].sum() >= 50
        live = [g for g in range(G) if c["code"][g] < nc and c["bb"][g] > 0]
        for kind in KINDS:
            assert sum(1 for g in live if c["kind"][g] == kind) >= 2, kind
        for ci in range(nc):
            assert (c["code"] == ci).sum() >= 4
        # the special groups
        gf = [g for g in live if min(M.CODES[c["code"][g]]) > 1 and c["bb"][g] % 8]
        assert len(gf) == 2 and (c["enc_status"][gf] == -1).all() and (c["dec_status"][gf] == -1).all()
        assert (c["bb"] == 0).sum() == 1
        assert sorted(c["code"][c["enc_status"] == -2].tolist()) == [nc, 255]
        assert (c["dec_status"] == -3).sum() >= 2
        band = c["code"] == M.CODES.index((250, 7))
        assert (c["enc_status"][band] == -1).all() and set(c["dec_status"][band]) == {0, -1}
        assert set(GF_SIZES) <= set(c["bb"].tolist())
        # a workgroup's four waves (consecutive groups) hold different codes
        assert sum(len(set(c["code"][i:i + 4].tolist())) > 1 for i in range(0, G - 3, 4)) >= 15
        # rows past k_g hold poison; rec_rows is 255 past the count up to the set's rmax
        for g in live:
            k = M.CODES[c["code"][g]][0]
            assert (c["rows"][g, k:] == M.ROW_POISON).all()
            assert (c["rec_rows"][g, c["nrec"][g]:] == 255).all()
        # expected outputs differ from the poison only inside the groups' regions
        for n in ("par", "rec"):
            exp, written = c[n + "_exp"], np.zeros(c[n + "_bytes"], bool)
            for g in live:
                k, m = M.CODES[c["code"][g]]
                nb = (m if c["enc_status"][g] == 0 else 1) if n == "par" else int(c["nrec"][g])
                o = int(c[n + "_off"][g])
                written[o:o + nb * int(c["bb"][g])] = True
            assert (exp[~written] == POISON).all()
            assert (exp[-64:] == POISON).all()
    assert not np.array_equal(M.main_case(oracle, 1)["code"], M.main_case(oracle, 2)["code"])
    # the host forms' batch: no size < 1, ascending offsets, more than 2 MiB of data
    h = M.host_case(oracle)
    assert h["bb"].min() >= 1 and h["data_bytes"] > 2 << 20
    for n in ("data", "par", "rec"):
        assert (np.diff(h[n + "_off"]) >= 0).all()


def test_large_matrix_sets_construct(oracle):
    """The two sets of test_mixed_large_matrices: a malformed group and a solve of at least 100
    erasures in each; whether the matrices fit in LDS follows from the launcher's own rule."""
    from tests import test_gpu_mixed as M
    for codes in ([(128, 16), (100, 100)], M.BIG_CODES):
        cenc = sum((k * m + 15) & ~15 for k, m in codes)
        solve = max(min(k, m) for k, m in codes)
        scratch = (1280 + 2 * solve * solve + 15) & ~15
        assert (768 + 128 + cenc + scratch > 64 * 1024) == (codes is M.BIG_CODES)
