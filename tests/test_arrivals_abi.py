"""CPU: the arrival-order receiver's acceptance rule (include/quic_fec.h, "Arrival-order
receiver") restated in Python and pinned three ways: against the group layer and
tests/ref_framing.revive (duplicates dropped among the packets that opened, then the first k),
against the slot-order helper (qfec_framed_rx_block_bytes), and the ABI (symbols, ctypes table,
wrappers that check their arrays before any call).  tests/test_gpu_arrivals.py checks the device
result against accept()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from quic_amd import _lib, fec
from quic_amd import fec_group as F
from tests import ref_framing as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1000
SYMBOLS = ["qfec_arrivals_rx_block_bytes", "qfec_open_decode_extract_arrivals_ragged"]
KERNELS = ["arrivals_init_kernel", "arrivals_pre_kernel", "open_arrivals_kernel",
           "arrivals_assemble_kernel", "arrivals_state_kernel"]


def accept(k, m, G, arrivals):
    """The five acceptance steps, sequentially.  arrivals: (group, index, pl) per arrival in
    arrival order, pl = the plaintext length of a packet that passes the length checks and whose
    tag matches, < 0 for one that does not (step 2 is the caller's: it needs the bytes).
    Returns (accepted, states): accepted[g] = the arrival indices group g took, in arrival order;
    states[a] = pl of an accepted arrival, else ARR_IGNORED / REJECTED / DUPLICATE / LATE."""
    accepted = [[] for _ in range(G)]
    seen = [set() for _ in range(G)]
    states = []
    for a, (g, i, pl) in enumerate(arrivals):
        if not 0 <= g < G or not 0 <= i < k + m:
            states.append(fec.ARR_IGNORED)
        elif pl < 0:
            states.append(fec.ARR_REJECTED)
        elif i in seen[g]:
            states.append(fec.ARR_DUPLICATE)
        elif len(seen[g]) >= k:
            seen[g].add(i)              # a late first copy still makes later copies duplicates
            states.append(fec.ARR_LATE)
        else:
            seen[g].add(i)
            accepted[g].append(a)
            states.append(pl)
    return accepted, states


def test_accept_pinned():
    """A hand-made stream, k = 2, m = 2, two groups."""
    arr = [(0, 0, 10), (0, 0, 10), (1, 3, -1), (0, 3, 16), (0, 1, 12), (1, 3, 16), (0, 1, 12),
           (-1, 0, 5), (2, 0, 5), (1, 4, 5), (1, 255, 5), (0, 2, 16), (1, 0, 0)]
    acc, st = accept(2, 2, 2, arr)
    assert acc == [[0, 3], [5, 12]]
    assert st == [10, -3, -1, 16, -4, 16, -3, -2, -2, -2, -2, -4, 0]


# ---------------------------------------------------------------- 1. the group layer
def _oracle_group(oracle, conf):
    """A QuicFecGroup whose codec is the CPU oracle (qfec_group_new_with_codec): no GPU."""
    L, O = F.lib(), oracle.lib()
    g = F.QuicFecGroup.__new__(F.QuicFecGroup)
    g._L = L
    g._h = L.qfec_group_new_with_codec(BASE, conf, ctypes.cast(O.oracle_encode, ctypes.c_void_p),
                                       ctypes.cast(O.oracle_decode, ctypes.c_void_p))
    g.fec_configuration = conf
    assert g._h
    return g


@pytest.mark.parametrize("k,m", [(5, 5), (10, 1), (2, 2), (10, 20), (32, 4)])
def test_accept_is_the_group_layers_rule(oracle, k, m):
    """Raw arrival streams of one group (shuffled, with duplicates, more than k packets, and
    packets that do not open, which never reach the group) go to qfec_group_update_received in
    arrival order, and the group is revived the moment it can be, as the connection does it
    (MaybeProcessRevivedPacket after every packet): the group takes exactly accept()'s packets,
    what it revives is ref_framing.revive on accept()'s list, and every packet behind that point
    is one accept() calls late or duplicate."""
    rng = np.random.default_rng(100 * k + m)
    F.set_fec_overrides(k, m)
    try:
        late_data = 0
        for trial in range(12):
            pays = [rng.integers(0, 256, int(rng.choice([0, 1, 7, 46, 300])), dtype=np.uint8)
                    .tobytes() for _ in range(k)]
            pns = [int(x) for x in rng.choice([1, 2, 4, 6], k)]
            red, rc = R.redundancy(oracle, k, m, BASE, [(BASE + i, pays[i], pns[i])
                                                        for i in range(k)])
            assert rc == 0
            par = {pn - BASE: d for pn, d, _ in red}
            # every packet once, some twice, in a random order; a few lost, a few rejected
            order = [int(x) for x in rng.permutation(k + m)]
            order += [int(x) for x in rng.choice(k + m, 3)]
            if trial % 3 == 0:
                order = [i for i in order if i >= k or rng.random() > 0.4]   # losses
            if trial % 4 == 1:
                order = list(range(k + m)) + order[:2]                      # in order first
            opens = [rng.random() > 0.15 for _ in order]
            stored = lambda i: R.prefix(pays[i], pns[i]) if i < k else par[i]   # noqa: E731
            arr = [(0, i, (len(pays[i]) if i < k else len(par[i])) if ok else -1)
                   for i, ok in zip(order, opens)]
            acc, st = accept(k, m, 1, arr)
            late_data += sum(1 for (g, i, pl), s in zip(arr, st) if s == fec.ARR_LATE and i < k)
            exp, erc = R.revive(oracle, k, m, BASE, [(BASE + arr[a][1], stored(arr[a][1]))
                                                     for a in acc[0]])
            grp = _oracle_group(oracle, F.FEC_5_5)
            got, grc, closed = [], 0, False
            for (g, i, pl), s in zip(arr, st):
                if pl < 0:
                    continue                                    # quic_framer.cc:657
                if closed:
                    # the connection revived and deleted the group with its k-th packet
                    # (quic_connection.cc:2477-2485): the rest of the stream is not the group's
                    assert s in (fec.ARR_LATE, fec.ARR_DUPLICATE), (trial, i, s)
                    continue
                took = grp.UpdateReceivedList(2, BASE + i, pns[i] if i < k else 1,
                                              pays[i] if i < k else par[i], i >= k)
                assert took == (s >= 0), (trial, i, s)
                assert s >= 0 or s == fec.ARR_DUPLICATE
                if grp.CanRevive():
                    got, grc = grp.getRevivedPackets()
                    closed = True
            assert closed == (len(acc[0]) == k)
            assert grc == erc == 0
            assert sorted(got) == sorted(exp), trial
            for pn, pay, pnl in got:                            # a revived packet is the sent one
                assert pay == pays[pn - BASE]
                assert pnl == {1: 1, 2: 2, 4: 0, 6: 2}[pns[pn - BASE]]
        assert late_data or m == 1, "no trial made a data packet late"
    finally:
        F.set_fec_overrides(0, 0)


# ---------------------------------------------------------------- 2. the host helper
def _bb_by_accept(k, m, G, grp, idx, pkt_len, ad_len):
    pl = pkt_len.astype(np.int64) - ad_len - 12
    ok = (pkt_len >= 0) & (ad_len >= 0) & (pl >= 0)
    arr = [(int(g), int(i), int(p) if o else -1) for g, i, p, o in zip(grp, idx, pl, ok)]
    acc, _ = accept(k, m, G, arr)
    return [max([arr[a][2] + (2 if arr[a][1] < k else 0) for a in acc[g]], default=0)
            for g in range(G)]


@pytest.mark.parametrize("k,m", [(5, 3), (10, 1), (2, 2), (32, 4)])
def test_arrivals_rx_block_bytes(k, m):
    rng = np.random.default_rng(7 * k + m)
    G, per = 9, k + m
    # a stream without duplicates and with at most k arrivals per group: the slot-order helper's
    # answer on the same packets placed by slot
    slots = np.concatenate([g * per + rng.permutation(per)[:int(rng.integers(0, k + 1))]
                            for g in range(G)]).astype(np.int64)
    slots = rng.permutation(slots)
    ad_slot = rng.choice([0, 13, 16], G * per).astype(np.int32)
    len_slot = (ad_slot + 12 + rng.integers(0, 1351, G * per)).astype(np.int32)
    len_slot[rng.random(G * per) < 0.1] = 11                   # too short to hold a tag
    placed = np.full(G * per, -1, np.int32)
    placed[slots] = len_slot[slots]
    grp, idx = (slots // per).astype(np.int32), (slots % per).astype(np.uint8)
    bb = fec.arrivals_rx_block_bytes(k, m, G, grp, idx, len_slot[slots], ad_slot[slots])
    np.testing.assert_array_equal(bb, fec.framed_rx_block_bytes(k, m, placed, ad_slot))
    assert bb.tolist() == _bb_by_accept(k, m, G, grp, idx, len_slot[slots], ad_slot[slots])
    # any stream: duplicates, more than k arrivals, stray tags, a tag at the last group
    n = 4 * (k + 8) * G
    grp = rng.integers(-1, G + 1, n).astype(np.int32)
    grp[-1] = G - 1
    idx = rng.integers(0, per + 2, n).astype(np.uint8)
    idx[::17] = 255
    ad = rng.choice([0, 13, 16], n).astype(np.int32)
    ln = (ad + 12 + rng.integers(0, 1351, n)).astype(np.int32)
    ln[::13] = -1
    ln[5::13] = ad[5::13] + 11
    bb = fec.arrivals_rx_block_bytes(k, m, G, grp, idx, ln, ad)
    assert bb.tolist() == _bb_by_accept(k, m, G, grp, idx, ln, ad)
    assert (np.bincount(grp[(grp >= 0) & (grp < G)], minlength=G) > k).all()
    # one associated-data length for every arrival; no arrival at all
    ln16 = np.where(ln < 0, ln, ln - ad + 16).astype(np.int32)
    np.testing.assert_array_equal(fec.arrivals_rx_block_bytes(k, m, G, grp, idx, ln16, 16),
                                  fec.arrivals_rx_block_bytes(k, m, G, grp, idx, ln16,
                                                              np.full(n, 16, np.int32)))
    none = np.zeros(0, np.int32)
    assert fec.arrivals_rx_block_bytes(k, m, G, none, none.astype(np.uint8), none, 16).tolist() \
        == [0] * G
    with pytest.raises(ValueError):
        fec.arrivals_rx_block_bytes(k, m, G, grp[:-1], idx, ln, ad)
    with pytest.raises(ValueError):
        fec.arrivals_rx_block_bytes(250, 6, G, grp, idx, ln, ad)


# ---------------------------------------------------------------- 3. the ABI
def test_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "quic_fec.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^QFEC_API\s+[\w\s\*]*?\b(\w+)\s*\(", text, re.M))
    for s in SYMBOLS:
        assert s in exported, s
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    for name in KERNELS:
        assert name in text, name
    for name, value in (("REJECTED", -1), ("IGNORED", -2), ("DUPLICATE", -3), ("LATE", -4)):
        assert re.search(r"#define QFEC_ARR_%s \(%d\)" % (name, value), text), name
        assert getattr(fec, "ARR_" + name) == value
    assert callable(fec.arrivals_rx_block_bytes)
    assert callable(fec.FecEngine.open_decode_extract_arrivals_ragged)
    # the declaration and the ctypes table agree on the number of arguments
    decl = re.search(r"QFEC_API int qfec_open_decode_extract_arrivals_ragged\(([^;]*)\);", text)
    assert len(decl.group(1).split(",")) == \
        len(_lib.SIGNATURES["qfec_open_decode_extract_arrivals_ragged"][1]) == 30


def test_null_context_is_minus_two():
    L = _lib.load()
    assert L.qfec_open_decode_extract_arrivals_ragged(
        None, 10, 1, 0, None, 0, None, 1400, None, None, 16, None, 1, None, None, None, None,
        None, None, None, None, None, None, None, None, None, 0, None, None, None) == -2


def test_wrapper_checks_arrays_before_the_call():
    """dtype and rows of the per-arrival arrays and of arr_at: the engine is never touched
    (None), so a wrong argument cannot reach the library."""
    import torch
    k, m, G, n = 10, 1, 3, 50
    slots, rmax = G * (k + m), 1
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    TE, VE = TypeError, ValueError
    buf = torch.zeros(G * 16000, dtype=u8)
    good = dict(bb=torch.full((G,), 1352, dtype=i32), off=torch.arange(G, dtype=i64) * 16000,
                pkt=torch.zeros((n, 1400), dtype=u8), pkt_len=torch.zeros(n, dtype=i32),
                ad_len=16, pn=torch.ones(n, dtype=u8), grp=torch.zeros(n, dtype=i32),
                idx=torch.zeros(n, dtype=u8), state=torch.zeros(n, dtype=i32),
                at=torch.zeros(slots, dtype=i32), rows=torch.zeros((G, k), dtype=u8),
                ol=torch.zeros(slots, dtype=i32), rr=torch.zeros((G, rmax), dtype=u8),
                rev=torch.zeros((G * rmax, 1351), dtype=u8), rl=torch.zeros(G * rmax, dtype=i32),
                rpn=torch.zeros(G * rmax, dtype=u8), st=torch.zeros(G, dtype=i32))
    bad = [(dict(pkt_len=good["pkt_len"][:-1]), VE), (dict(ad_len=torch.zeros(n + 1, dtype=i32)), VE),
           (dict(pn=good["pn"][:-1]), VE), (dict(grp=good["grp"][:-1]), VE),
           (dict(grp=good["grp"].to(i64)), TE), (dict(idx=good["idx"][:-1]), VE),
           (dict(idx=good["idx"].to(i32)), TE), (dict(state=good["state"][:-1]), VE),
           (dict(state=good["state"].to(i64)), TE), (dict(at=good["at"][:-1]), VE),
           (dict(at=torch.zeros(n, dtype=i32)), VE), (dict(at=good["at"].to(i64)), TE),
           (dict(ol=good["ol"][:-1]), VE), (dict(pkt=good["pkt"].to(torch.int8)), TE),
           (dict(bb=good["bb"][:-1]), TE), (dict(rl=good["rl"].to(i64)), TE)]
    for b, exc in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(exc) as e:
            fec.FecEngine.open_decode_extract_arrivals_ragged(
                None, k, m, a["bb"], a["pkt"], a["pkt_len"], a["ad_len"], a["pn"], a["grp"],
                a["idx"], a["state"], a["at"], buf, a["off"], a["rows"], a["ol"], buf, a["off"],
                a["rr"], a["rev"], a["rl"], rev_pn_len=a["rpn"], status=a["st"])
        assert e.type is exc, b


# ---------------------------------------------------------------- 4. the GPU tests' cases
@pytest.mark.parametrize("k,m", [(10, 1), (2, 2), (5, 5), (32, 4), (10, 20), (250, 5)])
def test_gpu_cases_are_what_they_claim(oracle, k, m):
    """tests/test_gpu_arrivals.py's streams, from the oracle, ref_framing and accept() alone.
    build_arrivals asserts each kind's outcome (which copy is accepted, which packet is late,
    what is revived); here: the shapes, the kinds, the tags and the helper's sizes."""
    from tests import test_gpu_arrivals as A
    c = A.build_arrivals(oracle, k, m)
    assert set(A.SHAPES) == {(10, 1), (2, 2), (5, 5), (32, 4), (10, 20), (250, 5)}
    assert all(c["kinds"].count(kind) >= 2 for kind in A.KINDS)
    assert c["n"] % 64 != 0 and c["n"] == len(c["arr"])
    s = c["sender"]
    assert s["G"] == A.SHAPES[(k, m)] and set(s["pay_len"].tolist()) == set(A.T.LENS)
    states = set(c["states"].tolist())
    assert {fec.ARR_REJECTED, fec.ARR_IGNORED, fec.ARR_DUPLICATE, fec.ARR_LATE} <= states
    assert (c["states"] >= 0).sum() == (c["arr_at"] >= 0).sum() == sum(map(len, c["acc"]))
    np.testing.assert_array_equal(
        np.where(np.array(c["kinds"]) == "bb0", 0,
                 fec.arrivals_rx_block_bytes(k, m, c["G"], c["grp"], c["idx"],
                                             np.where(np.array(c["what"]) == "toolong", -1,
                                                      c["wire_len"]), c["hdr_len"])), c["bb"])
    # another interleaving: the same packets per group, other arrival indices
    d = A.build_arrivals(oracle, k, m, 1)
    assert d["n"] == c["n"] and (d["grp"] != c["grp"]).any()
    np.testing.assert_array_equal(d["bb"], c["bb"])
    assert [len(x) for x in d["acc"]] == [len(x) for x in c["acc"]]
