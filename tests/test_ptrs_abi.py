"""CPU: the pointer-table batches' ABI (include/quic_fec.h, "Pointer-table batches"): the two
symbols, their ctypes rows against the header's declarations, the wrappers' checks of every
table before the library is touched, fec.block_ptrs, and the construction of
tests/test_gpu_ptrs.py's scattered arenas."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from quic_amd import _lib, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qfec_encode_batch_ptrs", "qfec_decode_batch_ptrs_recovered"]
KERNELS = ["gf_ptrs_kernel<encode>", "gf_ptrs_kernel<decode>", "xor_ptrs_kernel",
           "copy_ptrs_kernel"]


def _ctype(arg):
    """The ctypes type the table holds for one parameter of a declaration."""
    arg = " ".join(arg.split())
    if "*" in arg:
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
        decl = re.search(r"QFEC_API int %s\(([^;]*)\);" % s, text)
        assert decl, s
        res, args = _lib.SIGNATURES[s]
        assert res is ctypes.c_int
        assert [_ctype(a) for a in decl.group(1).split(",")] == args, s
    # the header's own form of the tables: arrays of const pointers
    assert "const unsigned char *const *d_data_ptrs" in text
    assert "unsigned char *const *d_parity_ptrs" in text
    assert "const unsigned char *const *d_block_ptrs" in text
    assert "unsigned char *const *d_rec_ptrs" in text
    assert "Pointer-table batches" in text
    for name in KERNELS:
        assert name in text, name
    assert callable(fec.FecEngine.encode_ptrs) and callable(fec.FecEngine.decode_ptrs_recovered)


def test_null_context_is_minus_two():
    L = _lib.load()
    assert L.qfec_encode_batch_ptrs(None, 10, 1, 0, None, 1352, None, None, None, None) == -2
    assert L.qfec_decode_batch_ptrs_recovered(None, 10, 1, 0, None, 1352, None, None, None, None,
                                              None, None) == -2


def test_block_ptrs_arithmetic():
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8)
    off = np.array([[0, 7, 4095], [16, 1352, 2704]], np.int64)
    for o in (off, torch.from_numpy(off), off.tolist(), off.astype(np.int32)):
        p = fec.block_ptrs(buf, o)
        assert p.dtype == torch.int64 and tuple(p.shape) == (2, 3) and p.device == buf.device
        assert (p.numpy() - buf.data_ptr() == off).all()
    view = buf[100:]                                  # a view: its own data_ptr counts
    assert int(fec.block_ptrs(view, [5])[0]) == buf.data_ptr() + 105
    assert tuple(fec.block_ptrs(buf, np.zeros((0, 4), np.int64)).shape) == (0, 4)


def test_wrappers_check_tables_before_the_call():
    """dtype, shape and device of every table, of bb, rows, rec_rows and status: the engine is
    never touched (None), so a wrong argument cannot reach the library."""
    import torch
    k, m, G = 5, 3, 4
    rmax = min(k, m)
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    good = dict(bb=torch.full((G,), 64, dtype=i32), tin=torch.zeros((G, k), dtype=i64),
                par=torch.zeros((G, m), dtype=i64), rec=torch.zeros((G, rmax), dtype=i64),
                rows=torch.zeros((G, k), dtype=u8), rr=torch.zeros((G, rmax), dtype=u8),
                st=torch.zeros(G, dtype=i32))

    def enc(a):
        fec.FecEngine.encode_ptrs(None, k, m, a["bb"], a["tin"], a["par"], status=a["st"])

    def dec(a):
        fec.FecEngine.decode_ptrs_recovered(None, k, m, a["bb"], a["tin"], a["rows"], a["rec"],
                                            a["rr"], status=a["st"])

    bad_enc = [dict(tin=good["tin"].to(i32)), dict(tin=good["tin"].double()),
               dict(tin=torch.zeros((G, k + 1), dtype=i64)), dict(tin=torch.zeros(G * k, dtype=i64)),
               dict(tin=good["tin"].numpy()), dict(tin=None),
               dict(par=good["par"].to(u8)), dict(par=torch.zeros((G, k), dtype=i64)),
               dict(par=torch.zeros((G + 1, m), dtype=i64)), dict(par=None),
               dict(bb=good["bb"].to(i64)), dict(bb=good["bb"][:-1]), dict(bb=None),
               dict(bb=64.0), dict(st=good["st"].to(i64)), dict(st=good["st"][:-1])]
    bad_dec = [dict(tin=good["tin"].to(i32)), dict(tin=torch.zeros((G, k - 1), dtype=i64)),
               dict(rec=good["rec"].to(i32)), dict(rec=torch.zeros((G, m + 1), dtype=i64)),
               dict(rec=torch.zeros((G - 1, rmax), dtype=i64)), dict(rec=None),
               dict(rows=good["rows"].to(i32)), dict(rows=torch.zeros((G, k + 1), dtype=u8)),
               dict(rr=good["rr"].to(i32)), dict(rr=torch.zeros((G, rmax + 1), dtype=u8)),
               dict(bb=good["bb"].to(u8)), dict(st=torch.zeros(G + 1, dtype=i32))]
    for call, bad in ((enc, bad_enc), (dec, bad_dec)):
        for b in bad:
            a = dict(good)
            a.update(b)
            with pytest.raises(TypeError) as e:
                call(a)
            assert "ROCm device" not in str(e.value), b     # refused for what is wrong with it
    # everything right but the device: tables in host memory are refused where their pointer is
    # taken, still before the call
    for call in (enc, dec):
        with pytest.raises(TypeError, match="ROCm device"):
            call(good)
        with pytest.raises(TypeError, match="ROCm device"):
            call(dict(good, bb=64))


@pytest.mark.parametrize("align", ["all", "aligned", "mixed"])
@pytest.mark.parametrize("k,m,G", [(32, 4, 7), (10, 1, 203), (5, 5, 23), (1, 3, 7), (250, 5, 12)])
def test_gpu_cases_construct(oracle, k, m, G, align):
    """tests/test_gpu_ptrs.py's arenas, from the oracle alone: no two blocks closer than 16
    bytes, every residue mod 16 used, the tables inside the arena, trap entries exactly where the
    contract says an entry is never dereferenced, and an expected image that differs from the
    first one only inside output blocks."""
    from tests import test_gpu_ptrs as P
    from tests.test_gpu_ragged import GF_SIZES, POISON, mixed_case
    c = mixed_case(oracle, k, m, G)
    zero = tuple(g for g in range(G) if c["bb"][g] % 8 == 0)[:2] if G > 2 else ()
    s = P.scatter(c, align, seed=G, zero=zero)
    if G >= 12 and m > 1:
        assert set(GF_SIZES) <= set(c["bb"].tolist())
    spans = sorted((o, o + (P.TRAP_BYTES if kind == "trap" else int(c["bb"][g])))
                   for (kind, g, i), o in s["off"].items())
    assert spans[0][0] >= 16 and spans[-1][1] + 16 <= s["total"]
    assert all(b[0] - a[1] >= 16 for a, b in zip(spans, spans[1:]))
    if align == "all":
        assert s["residues"] == set(range(16))
    elif align == "aligned":
        assert s["residues"] == {0}
    else:
        assert 0 in s["residues"] and any(r % 2 for r in s["residues"])
    trap, t = s["trap"], s["tabs"]
    assert (s["image"][trap:trap + P.TRAP_BYTES] == POISON).all()
    assert (s["exp"][trap:trap + P.TRAP_BYTES] == POISON).all()
    for g in range(G):
        if g in zero:
            assert all((t[n][g] == trap).all() for n in t) and s["bb"][g] == 0
            continue
        assert (t["data"][g] != trap).all() and (t["recv"][g] != trap).all()
        npar = m if c["enc_status"][g] == 0 else 1
        assert (t["par"][g, :npar] != trap).all() and (t["par"][g, npar:] == trap).all()
        nrec = int(c["nrec"][g]) if c["dec_status"][g] >= 0 else 0
        assert (t["rec"][g, :nrec] != trap).all() and (t["rec"][g, nrec:] == trap).all()
    # the images differ only inside parity and recovered blocks
    out = np.zeros(s["total"], bool)
    for (kind, g, i), o in s["off"].items():
        if kind in ("par", "rec"):
            out[o:o + int(c["bb"][g])] = True
    assert not (s["image"] != s["exp"])[~out].any()
    assert (s["image"][out] == POISON).all()
    # mixed: some group can take the 16-byte XOR path and some group cannot
    if align == "mixed" and G > 2:
        wide = [g for g in range(G) if g not in zero and c["bb"][g] % 8 == 0 and
                all(int(x) % 8 == 0 for x in list(t["data"][g]) + [t["par"][g, 0]])]
        narrow = [g for g in range(G) if g not in zero and
                  any(int(x) % 8 for x in t["data"][g])]
        assert wide and narrow
