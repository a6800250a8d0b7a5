"""Ragged batches, host side (no GPU): the packed layout of qfec_ragged_layout and the argument
checks of the Python host wrappers, and what the host wrappers hand to the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from quic_amd import fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up16(v):
    return (v + 15) & ~15


def test_layout_hand_written():
    k, m = 10, 4                      # min(k, m) = 4 = m: use (3, 5) below for rec != par
    bb = [8, 1352, 1, 24, 2064, 17]
    d, p, r, tot = fec.ragged_layout(k, m, bb)
    # data: 80 -> 80; 13520 -> 13600; 10 -> 13616; 240 -> 13856; 20640 -> 34496; 170 -> 34672
    assert d.tolist() == [0, 80, 13600, 13616, 13856, 34496]
    # parity: 32; 5408 -> 5440; 4 -> 5456; 96 -> 5552; 8256 -> 13808; 68 -> 13888
    assert p.tolist() == [0, 32, 5440, 5456, 5552, 13808]
    assert r.tolist() == p.tolist()
    assert tot == (34672, 13888, 13888)
    assert d.dtype == p.dtype == r.dtype == np.int64


def test_layout_rec_uses_min_k_m():
    k, m = 3, 5
    bb = [40, 7, 104]
    d, p, r, tot = fec.ragged_layout(k, m, bb)
    assert d.tolist() == [0, up16(120), up16(120) + up16(21)]
    assert p.tolist() == [0, up16(200), up16(200) + up16(35)]
    assert r.tolist() == d.tolist()               # min(k, m) = k
    assert tot == (128 + 32 + 312 + 8, 208 + 48 + 520 + 8, 128 + 32 + 312 + 8)
    for off in (d, p, r):
        assert all(int(o) % 16 == 0 for o in off)
    assert all(t % 16 == 0 for t in tot)


def test_layout_random_matches_running_sum():
    rng = np.random.default_rng(5)
    for k, m in ((10, 1), (5, 5), (32, 4), (10, 20), (1, 3), (250, 5)):
        bb = rng.integers(1, 2100, size=57).astype(np.int32)
        d, p, r, tot = fec.ragged_layout(k, m, bb)
        for off, n, t in ((d, k, tot[0]), (p, m, tot[1]), (r, min(k, m), tot[2])):
            run = 0
            for g, b in enumerate(bb):
                assert off[g] == run
                run = up16(run + n * int(b))
            assert t == run
    assert fec.ragged_layout(4, 2, [])[3] == (0, 0, 0)


def test_layout_past_4gib_matches_python_sums():
    """40,000 groups of (128, 16): every buffer's total and most of its offsets need more than
    32 bits (data 1.5e10 bytes); they equal running sums kept in Python integers."""
    k, m, G = 128, 16, 40000
    bb = np.resize(np.array([1352, 1350, 9000, 1, 1352], np.int32), G)
    d, p, r, tot = fec.ragged_layout(k, m, bb)
    assert r.tolist() == p.tolist()
    for off, n, t in ((d, k, tot[0]), (p, m, tot[1])):
        run, exp = 0, []
        for b in bb.tolist():
            exp.append(run)
            run = up16(run + n * b)
        assert off.tolist() == exp
        assert t == run
    assert tot[0] > 3 * 2**32 and d[-1] > 3 * 2**32 and int((d >= 2**32).sum()) > G // 2
    # uniform (128, 16) x 1352: offsets are g * k * bb, past 2^32 from group 24,819 on
    d, p, r, tot = fec.ragged_layout(k, m, np.full(G, 1352, np.int32))
    assert d.tolist() == [g * k * 1352 for g in range(G)]
    assert tot == (G * k * 1352, G * m * 1352, G * m * 1352) and tot[0] == 6_922_240_000


def test_layout_overflow_returns_minus_two():
    """Block sizes near 2^31 - 1 with k = 255: about 1.7e7 of them pass 2^63 bytes of data.  The
    longest array whose running sum (with its last round-up) still fits is laid out exactly; one
    more entry returns -2 and writes no total, instead of wrapping."""
    k, m, top = 255, 1, 2**31 - 1
    sizes = [top - j for j in range(7)]                  # cycled
    steps = [up16(k * b) for b in sizes]

    def run_after(n):                                    # the data total of the first n entries
        return (n // 7) * sum(steps) + sum(steps[:n % 7])

    def entry_fits(n):                                   # entry n (0-based) on top of run_after(n)
        return run_after(n) + k * sizes[n % 7] + 15 <= 2**63 - 1
    n_ok = 2**63 // max(steps) - 8
    while entry_fits(n_ok):
        n_ok += 1                                        # entries 0 .. n_ok - 1 fit
    assert 16_800_000 < n_ok < 16_900_000
    bb = np.resize(np.array(sizes, np.int32), n_ok + 1)
    L = fec.load()
    tot = np.full(3, -7, np.int64)
    assert L.qfec_ragged_layout(k, m, n_ok, bb.ctypes.data, None, None, None, tot.ctypes.data) == 0
    assert int(tot[0]) == run_after(n_ok) and 2**63 - 2**40 < int(tot[0]) < 2**63
    assert int(tot[1]) == int(tot[2])
    assert int(tot[1]) == (n_ok // 7) * sum(up16(b) for b in sizes) + sum(up16(b) for b in sizes[:n_ok % 7])
    tot[:] = -7
    assert L.qfec_ragged_layout(k, m, n_ok + 1, bb.ctypes.data, None, None, None,
                                tot.ctypes.data) == -2
    assert tot.tolist() == [-7, -7, -7]
    with pytest.raises(ValueError):
        fec.ragged_layout(k, m, bb)
    one = np.array([top], np.int32)
    assert L.qfec_ragged_layout(k, m, 1, one.ctypes.data, None, None, None, tot.ctypes.data) == 0
    assert int(tot[0]) == up16(k * top)


def test_layout_rejects_bad_sizes():
    L = fec.load()
    bb = np.array([8, 0, 8], np.int32)
    tot = np.zeros(3, np.int64)
    assert L.qfec_ragged_layout(4, 2, 3, bb.ctypes.data, None, None, None, tot.ctypes.data) == -2
    neg = np.array([-8], np.int32)
    assert L.qfec_ragged_layout(4, 2, 1, neg.ctypes.data, None, None, None, tot.ctypes.data) == -2
    assert L.qfec_ragged_layout(4, 2, -1, bb.ctypes.data, None, None, None, tot.ctypes.data) == -2
    assert L.qfec_ragged_layout(4, 2, 1, None, None, None, None, tot.ctypes.data) == -2
    with pytest.raises(ValueError):
        fec.ragged_layout(4, 2, [8, 0, 8])
    # offsets may be omitted one by one
    good = np.array([8, 24], np.int32)
    only = np.zeros(2, np.int64)
    assert L.qfec_ragged_layout(4, 2, 2, good.ctypes.data, None, only.ctypes.data, None, None) == 0
    assert only.tolist() == [0, 16]


def test_device_entry_points_reject_null_and_negative_groups():
    """Argument errors are -2 before anything touches a GPU."""
    L = fec.load()
    assert L.qfec_encode_batch_ragged(None, 4, 2, 1, 16, 16, 16, 16, 16, None, None) == -2
    assert L.qfec_decode_batch_ragged_recovered(None, 4, 2, 1, 16, 16, 16, 16, 16, 16, 16, None,
                                                None) == -2
    assert L.qfec_encode_batch_ragged_host(None, 4, 2, 1, 16, 16, 16, 16, 16, None) == -2
    assert L.qfec_decode_batch_ragged_recovered_host(None, 4, 2, 1, 16, 16, 16, 16, 16, 16, 16,
                                                     None) == -2


def _host_args(k, m, bb):
    import torch
    d, p, r, tot = fec.ragged_layout(k, m, bb)
    G = len(bb)
    return dict(
        bb=torch.tensor(bb, dtype=torch.int32),
        data=torch.zeros(tot[0], dtype=torch.uint8), data_off=torch.from_numpy(d),
        par=torch.zeros(tot[1], dtype=torch.uint8), par_off=torch.from_numpy(p),
        rec=torch.zeros(tot[2], dtype=torch.uint8), rec_off=torch.from_numpy(r),
        rows=torch.zeros((G, k), dtype=torch.uint8),
        rec_rows=torch.zeros((G, min(k, m)), dtype=torch.uint8),
        status=torch.zeros(G, dtype=torch.int32))


def _enc(a, **kw):
    a = dict(a, **kw)
    return fec.encode_ragged_host_into(None, 4, 2, a["bb"], a["data"], a["data_off"], a["par"],
                                       a["par_off"], a["status"])


def _dec(a, **kw):
    a = dict(a, **kw)
    return fec.decode_ragged_recovered_host_into(None, 4, 2, a["bb"], a["data"], a["data_off"],
                                                 a["rows"], a["rec"], a["rec_off"],
                                                 a["rec_rows"], a["status"])


def test_host_wrappers_reject_bad_buffers():
    """Non-contiguous, mis-typed or short host arrays are refused before the library is called
    (engine None: a call that got through would fail differently).  A buffer of the wrong kind
    (not a tensor, not contiguous) is a TypeError, a wrong dtype, shape or value a ValueError."""
    import torch
    a = _host_args(4, 2, [8, 24, 1352])
    bad = [
        (dict(bb=a["bb"].to(torch.int64)), ValueError),                  # sizes must be int32
        (dict(bb=torch.tensor([8, 0, 1352], dtype=torch.int32)), ValueError),   # a size < 1
        (dict(data_off=a["data_off"].to(torch.int32)), ValueError),      # offsets must be int64
        (dict(data_off=a["data_off"] + 8), ValueError),                  # not a multiple of 16
        (dict(data_off=a["data_off"][:2]), ValueError),                  # one offset per group
        (dict(data=a["data"][:-16]), ValueError),             # too short for the last group
        (dict(data=torch.zeros(2 * a["data"].numel(), dtype=torch.uint8)[::2]),
         TypeError),                                                     # non-contiguous
        (dict(data=a["data"].to(torch.int8)), ValueError),               # wrong dtype
        (dict(data=a["data"].numpy()), TypeError),                       # not a tensor
        (dict(status=a["status"].to(torch.int64)), ValueError),
    ]
    for kw, exc in bad:
        with pytest.raises(exc) as e:
            _enc(a, **kw)
        assert e.type is exc, kw
        with pytest.raises(exc) as e:
            _dec(a, **kw)
        assert e.type is exc, kw
    for kw, exc in ((dict(par=a["par"][:-1]), ValueError),
                    (dict(par_off=a["par_off"].flip(0)[::1] * 0 - 16), ValueError)):
        with pytest.raises(exc) as e:
            _enc(a, **kw)
        assert e.type is exc, kw
    for kw, exc in ((dict(rec=a["rec"][:-1]), ValueError), (dict(rows=a["rows"][:, :3]), TypeError),
                    (dict(rows=a["rows"].t().contiguous().t()), TypeError),
                    (dict(rec_rows=a["rec_rows"][:2]), ValueError)):
        with pytest.raises(exc) as e:
            _dec(a, **kw)
        assert e.type is exc, kw


# ---- what a wrapper hands to the library: a stand-in engine records the call
class RecordingLib:
    """Stands in for the loaded library: every symbol records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


CTX = 0x5eed0


def recording_engine():
    """A FecEngine that was never created: its library records, its context is CTX."""
    eng = fec.FecEngine.__new__(fec.FecEngine)
    eng.lib, eng._h = RecordingLib(), ctypes.c_void_p(CTX)
    return eng


def header_params(symbol):
    """The parameter names of `symbol`, in the order include/quic_fec.h declares them."""
    with open(os.path.join(ROOT, "include", "quic_fec.h")) as f:
        text = f.read()
    decl = re.search(r"^QFEC_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % re.escape(symbol), text, re.M)
    assert decl, symbol
    return [re.search(r"(\w+)\s*(\[\d*\])?\s*$", p).group(1) for p in decl.group(1).split(",")]


def assert_call(eng, symbol, **expected):
    """The one call `eng` recorded is `symbol`, and its arguments are `expected` (by the header's
    parameter names: a tensor stands for its data_ptr(), None for a null pointer) in the header's
    order."""
    calls = [c for c in eng.lib.calls if c[0] != "qfec_ctx_destroy"]
    assert [c[0] for c in calls] == [symbol]
    del eng.lib.calls[:]
    names = header_params(symbol)
    assert sorted(names) == sorted(expected), symbol
    got = [a.value if isinstance(a, ctypes.c_void_p) else a for a in calls[0][1]]
    want = [expected[n].data_ptr() if hasattr(expected[n], "data_ptr") else expected[n]
            for n in names]
    assert got == want, (symbol, list(zip(names, got, want)))


def test_host_wrappers_marshal_in_header_order():
    """The uniform and the ragged codec host wrappers: every pointer, stride and scalar is in the
    place include/quic_fec.h gives it, and an absent optional array is a null pointer."""
    import torch
    k, m, bb, G = 2, 1, 8, 2
    n, rmax = G * (k + m), 1
    u8, i32 = torch.uint8, torch.int32
    eng = recording_engine()
    data, par = torch.zeros((G, k, bb), dtype=u8), torch.zeros((G, m, bb), dtype=u8)
    rows, st = torch.zeros((G, k), dtype=u8), torch.zeros(G, dtype=i32)
    rec, rr = torch.zeros((G, rmax, bb), dtype=u8), torch.zeros((G, rmax), dtype=u8)
    hdr, pkt = torch.zeros((n, 20), dtype=u8), torch.zeros((n, 48), dtype=u8)
    hl, pl, kl, ol = (torch.zeros(n, dtype=i32) for _ in range(4))
    uni = dict(ctx=CTX, k=k, m=m, block_bytes=bb, groups=G)

    assert fec.encode_host_into(eng, k, m, bb, data, par) == 0
    assert_call(eng, "qfec_encode_batch_host", **uni, h_data=data, h_parity=par)
    assert fec.decode_host_into(eng, k, m, bb, data, rows) == 0
    assert_call(eng, "qfec_decode_batch_host", **uni, h_blocks=data, h_rows=rows, h_status=None)
    fec.decode_host_into(eng, k, m, bb, data, rows, st)
    assert_call(eng, "qfec_decode_batch_host", **uni, h_blocks=data, h_rows=rows, h_status=st)
    assert fec.decode_recovered_host_into(eng, k, m, bb, data, rows, rec, rr) == 0
    assert_call(eng, "qfec_decode_batch_recovered_host", **uni, h_blocks=data, h_rows=rows,
                h_rec=rec, h_rec_rows=rr, h_status=None)
    fec.decode_recovered_host_into(eng, k, m, bb, data, rows, rec, rr, st)
    assert_call(eng, "qfec_decode_batch_recovered_host", **uni, h_blocks=data, h_rows=rows,
                h_rec=rec, h_rec_rows=rr, h_status=st)

    assert fec.encode_seal_groups_host_into(eng, k, m, bb, data, hdr, hl, pl, pkt, kl) == 0
    assert_call(eng, "qfec_encode_seal_groups_batch_host", **uni, h_data=data, h_hdr=hdr,
                hdr_stride=20, h_hdr_len=hl, hdr_len_all=0, h_pt_len=pl, pt_len_all=0, h_pkt=pkt,
                pkt_stride=48, h_pkt_len=kl)
    fec.encode_seal_groups_host_into(eng, k, m, bb, data, None, 0, 7, pkt, kl)
    assert_call(eng, "qfec_encode_seal_groups_batch_host", **uni, h_data=data, h_hdr=None,
                hdr_stride=0, h_hdr_len=None, hdr_len_all=0, h_pt_len=None, pt_len_all=7,
                h_pkt=pkt, pkt_stride=48, h_pkt_len=kl)
    assert fec.open_decode_host_into(eng, k, m, bb, pkt, kl, 13, rec, rr) == 0
    assert_call(eng, "qfec_open_decode_batch_host", **uni, h_pkt=pkt, pkt_stride=48, h_pkt_len=kl,
                h_ad_len=None, ad_len_all=13, h_rec=rec, h_rec_rows=rr, h_status=None,
                h_open_len=None)
    fec.open_decode_host_into(eng, k, m, bb, pkt, kl, hl, rec, rr, st, ol)
    assert_call(eng, "qfec_open_decode_batch_host", **uni, h_pkt=pkt, pkt_stride=48, h_pkt_len=kl,
                h_ad_len=hl, ad_len_all=0, h_rec=rec, h_rec_rows=rr, h_status=st, h_open_len=ol)

    a = _host_args(k, m, [8, 24])
    rag = dict(ctx=CTX, k=k, m=m, groups=G, h_bb=a["bb"])
    assert fec.encode_ragged_host_into(eng, k, m, a["bb"], a["data"], a["data_off"], a["par"],
                                       a["par_off"]) == 0
    assert_call(eng, "qfec_encode_batch_ragged_host", **rag, h_data=a["data"],
                h_data_off=a["data_off"], h_parity=a["par"], h_par_off=a["par_off"],
                h_status=None)
    fec.encode_ragged_host_into(eng, k, m, a["bb"], a["data"], a["data_off"], a["par"],
                                a["par_off"], a["status"])
    assert_call(eng, "qfec_encode_batch_ragged_host", **rag, h_data=a["data"],
                h_data_off=a["data_off"], h_parity=a["par"], h_par_off=a["par_off"],
                h_status=a["status"])
    assert fec.decode_ragged_recovered_host_into(eng, k, m, a["bb"], a["data"], a["data_off"],
                                                 a["rows"], a["rec"], a["rec_off"],
                                                 a["rec_rows"]) == 0
    assert_call(eng, "qfec_decode_batch_ragged_recovered_host", **rag, h_blocks=a["data"],
                h_blocks_off=a["data_off"], h_rows=a["rows"], h_rec=a["rec"],
                h_rec_off=a["rec_off"], h_rec_rows=a["rec_rows"], h_status=None)
    fec.decode_ragged_recovered_host_into(eng, k, m, a["bb"], a["data"], a["data_off"], a["rows"],
                                          a["rec"], a["rec_off"], a["rec_rows"], a["status"])
    assert_call(eng, "qfec_decode_batch_ragged_recovered_host", **rag, h_blocks=a["data"],
                h_blocks_off=a["data_off"], h_rows=a["rows"], h_rec=a["rec"],
                h_rec_off=a["rec_off"], h_rec_rows=a["rec_rows"], h_status=a["status"])
