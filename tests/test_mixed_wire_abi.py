"""CPU: the mixed-code wire path's ABI (include/quic_fec.h, "Mixed-code wire path"): the five
symbols and their ctypes rows against the header, the three host helpers against NumPy and
against the uniform helpers run per code, the acceptance rule with k per group (accept_mixed,
written from the header's text and pinned to tests.test_arrivals_abi.accept per code), the
wrappers' array checks before the library is touched, and the construction of
tests/test_gpu_mixed_wire.py's batches."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from quic_amd import _lib, fec
from tests.test_arrivals_abi import accept
from tests.test_mixed_abi import _ctype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qfec_mixed_packet_layout", "qfec_framed_layout_mixed",
           "qfec_arrivals_rx_block_bytes_mixed", "qfec_frame_encode_seal_groups_batch_mixed",
           "qfec_open_decode_extract_arrivals_mixed"]
PRESETS = [(5, 5), (10, 10), (10, 15), (10, 20), (15, 15), (250, 5)]
CODES = PRESETS + [(10, 1), (2, 2), (32, 4)]


def accept_mixed(km, arrivals):
    """The five acceptance steps of the arrival-order receiver with k and k + m read per group.
    km[g] = (k_g, m_g), (-1, -1) for a group the call does not run (no code, or a span that does
    not fit); arrivals: (group, index, pl) in arrival order, pl < 0 for a packet that fails the
    length checks or whose tag does not match.  Returns (accepted, states)."""
    G = len(km)
    accepted = [[] for _ in range(G)]
    seen = [set() for _ in range(G)]
    states = []
    for a, (g, i, pl) in enumerate(arrivals):
        if not 0 <= g < G or km[g][0] < 0 or not 0 <= i < km[g][0] + km[g][1]:
            states.append(fec.ARR_IGNORED)                   # 1. no slot of this batch
        elif pl < 0:
            states.append(fec.ARR_REJECTED)                  # 2. never reaches its group
        elif i in seen[g]:
            states.append(fec.ARR_DUPLICATE)                 # 3. an earlier copy opened
        elif len(seen[g]) >= km[g][0]:
            seen[g].add(i)
            states.append(fec.ARR_LATE)                      # 4. k_g distinct indices opened earlier
        else:
            seen[g].add(i)
            accepted[g].append(a)
            states.append(pl)                                # 5. accepted
    return accepted, states


def _stream(rng, G, n, code):
    """A hostile tagged stream over G groups of CODES[code[g]]."""
    grp = rng.integers(-1, G + 1, n).astype(np.int32)
    idx = rng.choice([0, 1, 2, 3, 4, 9, 10, 11, 29, 30, 35, 36, 249, 254, 255], n).astype(np.uint8)
    wlen = rng.choice([-1, 0, 20, 27, 28, 29, 100, 1378], n).astype(np.int32)
    ad = rng.choice([-1, 0, 13, 16], n).astype(np.int32)
    return grp, idx, wlen, ad


def test_symbols_exported_declared_and_typed():
    """Fails on the parent commit: none of the five symbols exists there."""
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
        assert list(args) == [_ctype(a) for a in decl.group(1).split(",")], s
    assert "Mixed-code wire path" in text
    for name in ("frame_encode_seal_mixed", "open_decode_extract_arrivals_mixed"):
        assert callable(getattr(fec.FecEngine, name))
    for name in ("mixed_packet_layout", "framed_layout_mixed", "arrivals_rx_block_bytes_mixed"):
        assert callable(getattr(fec, name))
    L = _lib.load()
    assert L.qfec_frame_encode_seal_groups_batch_mixed(*[None] * 2, 0, *[None] * 4, 0, 0,
                                                       *[None] * 5, 0, None, 0, None, 0, None,
                                                       None, 0, None, 0, None, None, None) == -2
    assert L.qfec_open_decode_extract_arrivals_mixed(*[None] * 2, 0, *[None] * 3, 0, 0, None, 0,
                                                     None, None, 0, None, 0, *[None] * 13, 0,
                                                     None, None, None) == -2


def test_mixed_packet_layout():
    rng = np.random.default_rng(1)
    ks, ms = np.array([k for k, _ in CODES]), np.array([m for _, m in CODES])
    for G in (0, 1, 7, 300):
        code = rng.integers(0, len(CODES), G).astype(np.uint8)
        if G > 3:
            code[[1, G - 1]] = [len(CODES), 255]               # groups without a code
        has = code < len(CODES)
        per = np.where(has, ks[np.minimum(code, len(CODES) - 1)] + ms[np.minimum(code, len(CODES) - 1)], 0)
        kk = np.where(has, ks[np.minimum(code, len(CODES) - 1)], 0)
        pkt_first, pay_first = fec.mixed_packet_layout(CODES, code)
        np.testing.assert_array_equal(pkt_first, np.concatenate([[0], np.cumsum(per)]))
        np.testing.assert_array_equal(pay_first, np.concatenate([[0], np.cumsum(kk)]))
        assert pkt_first.dtype == np.int32 and pkt_first.shape == (G + 1,)
        if G > 3:
            assert pkt_first[1] == pkt_first[2] and pay_first[G - 1] == pay_first[G]
    # a total above INT32_MAX: 2^31 / 255 groups of (250, 5) and one more
    G = (1 << 31) // 255 + 1
    L = _lib.load()
    k, m = np.array([250], np.int32), np.array([5], np.int32)
    code = np.zeros(G, np.uint8)
    first = np.zeros(G + 1, np.int32)
    assert L.qfec_mixed_packet_layout(1, fec._vp(k), fec._vp(m), G, fec._vp(code), fec._vp(first),
                                      None) == -2
    assert L.qfec_mixed_packet_layout(1, fec._vp(k), fec._vp(m), G - 2, fec._vp(code),
                                      fec._vp(first), None) == 0
    # the argument errors qfec_mixed_layout rejects
    assert L.qfec_mixed_packet_layout(0, fec._vp(k), fec._vp(m), 0, None, None, None) == -2
    assert L.qfec_mixed_packet_layout(33, fec._vp(k), fec._vp(m), 0, None, None, None) == -2
    assert L.qfec_mixed_packet_layout(1, None, fec._vp(m), 0, None, None, None) == -2
    assert L.qfec_mixed_packet_layout(1, fec._vp(k), fec._vp(m), -1, None, None, None) == -2
    assert L.qfec_mixed_packet_layout(1, fec._vp(k), fec._vp(m), 1, None, None, None) == -2
    assert L.qfec_mixed_packet_layout(1, fec._vp(m * 0), fec._vp(m), 0, None, None, None) == -2
    with pytest.raises(ValueError):
        fec.mixed_packet_layout([(0, 1)], [0])


def test_framed_layout_mixed_equals_framed_layout_per_group():
    rng = np.random.default_rng(2)
    G = 120
    code = rng.integers(0, len(CODES), G).astype(np.uint8)
    _, pay_first = fec.mixed_packet_layout(CODES, code)
    pay_len = rng.choice([0, 1, 6, 7, 46, 1000, 1343, 1346, 1350, 0x3fff], pay_first[-1]).astype(np.int32)
    bb, d, p, r, totals = fec.framed_layout_mixed(CODES, code, pay_len)
    for g in range(G):
        k, m = CODES[code[g]]
        one = fec.framed_layout(k, m, pay_len[pay_first[g]:pay_first[g] + k])
        assert bb[g] == one[0][0]
    for got, want in zip((d, p, r, totals), fec.mixed_layout(CODES, code, bb)):
        np.testing.assert_array_equal(got, want)
    again = fec.framed_layout_mixed(CODES, code, pay_len, pay_first)
    np.testing.assert_array_equal(again[0], bb)
    # groups that share lengths through an explicit table
    shared = np.zeros(G + 1, np.int32)
    np.testing.assert_array_equal(
        fec.framed_layout_mixed(CODES, code, pay_len, shared)[0],
        [fec.framed_layout(*CODES[c], pay_len[:CODES[c][0]])[0][0] for c in code])
    for bad in (-1, 0x4000):
        x = pay_len.copy()
        x[int(pay_first[G // 2])] = bad
        with pytest.raises(ValueError):
            fec.framed_layout_mixed(CODES, code, x)
    with pytest.raises(ValueError):                          # the last group's span leaves pay_len
        fec.framed_layout_mixed(CODES, code, pay_len[:-1])
    with pytest.raises(ValueError):
        fec.framed_layout_mixed(CODES, code, pay_len, -1 - shared)
    with pytest.raises(ValueError):                          # a group without a code has no layout
        fec.framed_layout_mixed(CODES, np.where(np.arange(G) == 3, 99, code), pay_len)
    empty = fec.framed_layout_mixed(CODES, np.zeros(0, np.uint8), np.zeros(0, np.int32))
    assert empty[0].shape == (0,) and empty[4] == (0, 0, 0)


def test_arrivals_rx_block_bytes_mixed_equals_per_code():
    rng = np.random.default_rng(3)
    G, n = 60, 5000
    code = rng.integers(0, len(CODES), G).astype(np.uint8)
    code[[5, 17]] = [len(CODES), 200]
    grp, idx, wlen, ad = _stream(rng, G, n, code)
    for ad_arg in (ad, 16):
        bb = fec.arrivals_rx_block_bytes_mixed(CODES, code, grp, idx, wlen, ad_arg)
        assert bb[5] == 0 and bb[17] == 0 and bb.max() > 0
        for ci, (k, m) in enumerate(CODES):
            mine = np.flatnonzero(code == ci)
            if not mine.size:
                continue
            # the code's sub-stream, its groups renumbered; other tags leave the batch
            renum = np.full(G + 2, -1, np.int64)
            renum[mine] = np.arange(mine.size)
            sub = np.flatnonzero((grp >= 0) & (grp < G) & (renum[np.clip(grp, 0, G - 1)] >= 0))
            one = fec.arrivals_rx_block_bytes(k, m, mine.size, renum[grp[sub]].astype(np.int32),
                                              idx[sub], wlen[sub],
                                              ad_arg if isinstance(ad_arg, int) else ad_arg[sub])
            np.testing.assert_array_equal(bb[mine], one, str((k, m)))
    np.testing.assert_array_equal(fec.arrivals_rx_block_bytes_mixed(CODES, code, [], [], [], 16),
                                  np.zeros(G, np.int32))
    with pytest.raises(ValueError):
        fec.arrivals_rx_block_bytes_mixed(CODES + [(250, 6)], code, grp, idx, wlen, ad)


def test_accept_mixed_equals_accept_per_code():
    """accept_mixed on a hostile stream against tests.test_arrivals_abi.accept (pinned to the
    group layer) run per code on that code's sub-stream."""
    rng = np.random.default_rng(4)
    G, n = 40, 6000
    code = rng.integers(0, len(CODES), G)
    km = [CODES[c] for c in code]
    km[7] = km[23] = (-1, -1)
    arr = [(int(g), int(i), int(pl)) for g, i, pl in
           zip(rng.integers(-1, G + 1, n), rng.choice([0, 1, 2, 3, 5, 9, 10, 11, 20, 35, 254, 255], n),
               rng.choice([-1, -1, 0, 12, 1350], n))]
    acc, states = accept_mixed(km, arr)
    assert {fec.ARR_IGNORED, fec.ARR_REJECTED, fec.ARR_DUPLICATE, fec.ARR_LATE} <= set(states)
    for g in (7, 23):
        assert not acc[g] and all(states[a] == fec.ARR_IGNORED for a, x in enumerate(arr) if x[0] == g)
    for kmc in set(CODES):
        mine = [g for g in range(G) if km[g] == kmc]
        renum = {g: j for j, g in enumerate(mine)}
        sub = [a for a, x in enumerate(arr) if x[0] in renum]
        acc1, st1 = accept(kmc[0], kmc[1], len(mine), [(renum[arr[a][0]],) + arr[a][1:] for a in sub])
        assert [states[a] for a in sub] == st1
        for g in mine:
            assert acc[g] == [sub[a] for a in acc1[renum[g]]]
    outside = [a for a, x in enumerate(arr) if not 0 <= x[0] < G]
    assert outside and all(states[a] == fec.ARR_IGNORED for a in outside)


def test_wrappers_check_arrays_before_the_call():
    """dtype, shape and device of the arrays: the engine is never touched (None)."""
    import types
    import torch
    G, n, npkt, npay = 3, 50, 33, 30
    cs = types.SimpleNamespace(_h=None, kmax=10, rmax=1)
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    TE, VE = TypeError, ValueError
    buf = torch.zeros(G * 16000, dtype=u8)
    good = dict(code=torch.zeros(G, dtype=u8), bb=torch.full((G,), 1352, dtype=i32),
                first=torch.zeros(G + 1, dtype=i32), pfirst=torch.zeros(G + 1, dtype=i32),
                off=torch.arange(G, dtype=i64) * 16000, pkt=torch.zeros((n, 1400), dtype=u8),
                pkt_len=torch.zeros(n, dtype=i32), ad_len=16, pn=torch.ones(n, dtype=u8),
                grp=torch.zeros(n, dtype=i32), idx=torch.zeros(n, dtype=u8),
                state=torch.zeros(n, dtype=i32), at=torch.zeros(npkt, dtype=i32),
                rows=torch.zeros((G, 10), dtype=u8), ol=torch.zeros(npkt, dtype=i32),
                rr=torch.zeros((G, 1), dtype=u8), rev=torch.zeros((G, 1351), dtype=u8),
                rl=torch.zeros(G, dtype=i32), rpn=torch.zeros(G, dtype=u8),
                st=torch.zeros(G, dtype=i32))
    bad = [(dict(code=good["code"].to(i32)), TE), (dict(code=[0, 0, 0]), TE),
           (dict(bb=good["bb"][:-1]), TE), (dict(first=good["first"][:-1]), TE),
           (dict(first=good["first"].to(i64)), TE), (dict(off=good["off"].to(i32)), TE),
           (dict(pkt_len=good["pkt_len"][:-1]), VE), (dict(grp=good["grp"].to(i64)), TE),
           (dict(idx=good["idx"][:-1]), VE), (dict(state=good["state"][:-1]), VE),
           (dict(at=good["at"].to(i64)), TE), (dict(at=None), TE), (dict(ol=good["ol"][:-1]), VE),
           (dict(rows=torch.zeros((G, 9), dtype=u8)), TE), (dict(rr=torch.zeros((G, 2), dtype=u8)), TE),
           (dict(rev=torch.zeros((G + 1, 1351), dtype=u8)), VE), (dict(rl=good["rl"].to(i64)), TE),
           (dict(st=good["st"][:-1]), TE)]
    for b, exc in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(exc) as e:
            fec.FecEngine.open_decode_extract_arrivals_mixed(
                None, cs, a["code"], a["bb"], a["first"], a["pkt"], a["pkt_len"], a["ad_len"],
                a["pn"], a["grp"], a["idx"], a["state"], a["at"], buf, a["off"], a["rows"], a["ol"],
                buf, a["off"], a["rr"], a["rev"], a["rl"], rev_pn_len=a["rpn"], status=a["st"])
        assert e.type is exc, b
    # every good array on the CPU: refused where the first pointer is taken, before any call
    with pytest.raises(TypeError):
        fec.FecEngine.open_decode_extract_arrivals_mixed(
            None, cs, good["code"], good["bb"], good["first"], good["pkt"], good["pkt_len"], 16,
            good["pn"], good["grp"], good["idx"], good["state"], good["at"], buf, good["off"],
            good["rows"], good["ol"], buf, good["off"], good["rr"], good["rev"], good["rl"])
    send = dict(code=good["code"], bb=good["bb"], first=good["first"], pfirst=good["pfirst"],
                off=good["off"], hdr=torch.zeros((npkt, 16), dtype=u8),
                hdr_len=torch.zeros(npkt, dtype=i32), pay=torch.zeros((npay, 1351), dtype=u8),
                pay_len=torch.zeros(npay, dtype=i32), pn=torch.ones(npay, dtype=u8),
                pkt=torch.zeros((npkt, 1400), dtype=u8), pkt_len=torch.zeros(npkt, dtype=i32),
                st=good["st"])
    bad = [(dict(code=send["code"].to(i32)), TE), (dict(pfirst=send["pfirst"][:-1]), TE),
           (dict(first=send["first"].to(i64)), TE), (dict(hdr=send["hdr"][:-1]), VE),
           (dict(hdr_len=send["hdr_len"][:-1]), VE), (dict(pay_len=send["pay_len"][:-1]), VE),
           (dict(pay_len=send["pay_len"].to(i64)), TE), (dict(pn=send["pn"][:-1]), VE),
           (dict(pkt_len=send["pkt_len"][:-1]), VE), (dict(pkt=send["pkt"].to(torch.int8)), TE),
           (dict(st=send["st"].to(i64)), TE), (dict(), TE)]
    for b, exc in bad:
        a = dict(send)
        a.update(b)
        with pytest.raises(exc) as e:
            fec.FecEngine.frame_encode_seal_mixed(
                None, cs, a["code"], a["bb"], a["first"], a["pfirst"], buf, a["off"], buf, a["off"],
                a["hdr"], a["hdr_len"], a["pay"], a["pay_len"], a["pn"], a["pkt"], a["pkt_len"],
                status=a["st"])
        assert e.type is exc, b


def test_gpu_batches_are_what_they_claim(oracle):
    """tests/test_gpu_mixed_wire.py's batches: nine codes, every kind at least twice per code,
    tiles that really mix codes, and the forced properties of the packet geometry."""
    from tests import test_gpu_arrivals as A
    from tests import test_gpu_mixed_wire as W
    assert len(W.CODES) == 9 and W.CODES[:6] == W.SHAPES and W.CODES[8] == (5, 5)
    assert (W.KMAX, W.RMAX) == (250, 15)
    r, s = W.build_rx(oracle), W.build_tx(oracle)
    for b in (r, s):
        order, first, code = b["order"], b["pkt_first"], b["code"]
        G = b["G"]
        assert order.count(None) == 1 and 16 < order.index(None) < G - 16
        assert code[order.index(None)] == W.NOCODE
        assert {2, 8} <= set(code.tolist()) and set(code.tolist()) - {W.NOCODE} <= set(range(9))
        assert all(W.CODES[code[g]] == W.SHAPES[og[0]] for g, og in enumerate(order) if og is not None)
        # one tile of 16 groups of (2, 2); a (250, 5) group with a tile wholly inside it
        assert list(first[:17]) == list(range(0, 68, 4))
        big = [g for g, og in enumerate(order) if og is not None and W.SHAPES[og[0]] == (250, 5)]
        assert big and all((first[g] + 63) // 64 + 2 <= first[g + 1] // 64 for g in big)
        tile = np.searchsorted(first, np.arange(0, b["npkt"], 64), side="right") - 1
        last = np.searchsorted(first, np.minimum(np.arange(0, b["npkt"], 64) + 63, b["npkt"] - 1),
                               side="right") - 1
        mixes = [len({int(b["bb"][g]) for g in range(t0, t1 + 1) if order[g] is not None}) >= 3 and
                 len({int(code[g]) for g in range(t0, t1 + 1)}) >= 3 for t0, t1 in zip(tile, last)]
        assert sum(mixes) >= 3                                 # three codes, three sizes in a tile
        assert any(first[g] % 64 > first[g + 1] % 64 > 0 for g in range(G))   # a group straddles
        assert b["npkt"] % 64 != 0                             # the last tile is partial
    for ci, c in r["cases"].items():
        assert all(c["kinds"].count(kind) >= 2 for kind in A.KINDS), W.SHAPES[ci]
        assert sorted(g for (cj, g) in r["where"] if cj == ci) == list(range(c["G"]))
    assert r["n"] == sum(c["n"] for c in r["cases"].values()) + 8 and r["n"] % 64 != 0
    assert len({int(r["code"][g]) for g in r["grp"][:64] if 0 <= g < r["G"]}) >= 3
    # each group's arrivals keep their order: the mixed stream's states are the per-code states
    km = [(-1, -1) if og is None else W.SHAPES[og[0]] for og in r["order"]]
    _, states = accept_mixed(km, r["arr"])
    for a, src in enumerate(r["src"]):
        assert states[a] == (-2 if src is None else r["cases"][src[0]]["states"][src[1]])
    tagged = np.flatnonzero(r["grp"] == r["nocode"][0])
    assert tagged.size == 8
    # the sender's batch holds every length of LENS, 0 and bb - 2 among them
    assert set(A.T.LENS) <= set(s["pay_len"].tolist())
    assert any(int(s["pay_len"][q]) == int(s["bb"][g]) - 2 for g, og in enumerate(s["order"])
               if og is not None for q in range(s["pay_first"][g], s["pay_first"][g + 1]))
    other = W.build_rx(oracle, 1)
    assert other["G"] == r["G"] and other["n"] == r["n"] and other["npkt"] == r["npkt"]
    assert not np.array_equal(other["code"], r["code"])
