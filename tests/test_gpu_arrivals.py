"""GPU: the arrival-order receiver (qfec_open_decode_extract_arrivals_ragged) against the
sequential acceptance rule (tests/test_arrivals_abi.accept), against the slot-order receiver run
on the accepted packets placed by slot on the host, and against tests/ref_framing.revive.
Everything is bit-exact.

The packets are tests/test_gpu_framed.build_send's sealed wire packets.  A receiver batch has
more groups than the sender's (receiver group r takes the packets of sender group r mod G), so
that every shape holds each kind of group at least twice; the groups' arrivals are interleaved
by a seeded merge, so one wave of 64 arrivals mixes groups, kinds and lengths.  The case builder
runs on the CPU and is cached; tests/test_arrivals_abi.py checks its construction without a
GPU."""
import numpy as np
import pytest

from tests import ref_framing as R
from tests import test_gpu_framed as T
from tests.guarded import FILL, guarded, guarded_from
from tests.test_arrivals_abi import KERNELS, accept
from tests.test_gpu_pp_ragged import dev, host, packed_gaps

pytestmark = pytest.mark.gpu

BASE = T.BASE
SHAPES = dict(T.SHAPES)
SHAPES[(250, 5)] = 2                  # the loops over more than 64 slots per group
KINDS = ["inorder", "shuffled_loss", "dup_data", "dup_fec", "tamper_first", "tamper_only",
         "late_data", "late_fec", "fewer", "toolong", "bb0", "nofec", "stress"]
STRESS_COPIES = 200
REV_STRIDE = 1351


def sender(O, k, m):
    """tests/test_gpu_framed.py's sender batch of the shape; (250, 5), which that file does not
    have, takes its LENS in turn below a longest payload of 1350 and of 1349 bytes."""
    G = SHAPES[(k, m)]
    if (k, m) in T.SHAPES:
        return T.build_send(O, k, m, G)
    lens = np.zeros(G * k, np.int32)
    for g, top in enumerate(T.LENS[:G]):
        pool = [v for v in T.LENS if v <= top]
        lens[g * k:(g + 1) * k] = [pool[(g + i) % len(pool)] for i in range(k)]
    return T.build_send(O, k, m, G, lens=lens, stride=1351)


def sender_groups(s, kinds):
    """The sender group whose packets receiver group r gets: r mod G, but a 'nofec' group takes
    one whose bb is not a multiple of 8 once its FEC packets are gone."""
    odd = [g for g in range(s["G"])
           if (int(s["pay_len"][g * s["k"]:(g + 1) * s["k"]].max()) + 2) % 8]
    assert odd
    return [odd[(r // len(KINDS)) % len(odd)] if kind == "nofec" else r % s["G"]
            for r, kind in enumerate(kinds)]


def group_events(kind, k, m, rng):
    """One group's arrivals in order: (index, what), what in 'good' / 'tamper' / 'toolong'.
    Returns (events, x): x = the data packet the kind is about (None: none)."""
    per = k + m
    good = lambda idx: [(int(i), "good") for i in idx]        # noqa: E731
    x = int(rng.integers(k))
    others = [i for i in range(k) if i != x]
    if kind == "inorder":
        return good(range(per)), None
    if kind == "shuffled_loss":
        lost = {x} | {int(i) for i in rng.choice(per, int(rng.integers(0, m)), replace=False)}
        return good(rng.permutation([i for i in range(per) if i not in lost])), x
    if kind == "dup_data":
        ev = good(rng.permutation(per))
        at = ev.index((x, "good"))
        ev.insert(int(rng.integers(at + 1, len(ev) + 1)), (x, "good"))
        return ev, x
    if kind == "dup_fec":                                      # data x lost, FEC 0 twice
        return good([k, k] + list(rng.permutation(others)) + list(range(k + 1, per))), x
    if kind == "tamper_first":
        return [(x, "tamper")] + good(range(per)), x
    if kind == "tamper_only":
        return good([k]) + [(i, "tamper" if i == x else "good") for i in range(k)] + \
            good(range(k + 1, per)), x
    if kind == "late_data":                                    # k others first, one of them FEC
        return good([k] + list(rng.permutation(others)) + [x] + list(range(k + 1, per))), x
    if kind == "late_fec":
        return good(list(rng.permutation(k)) + list(range(k, per))), None
    if kind == "fewer":                                        # k - 1 distinct packets, one twice
        ev = good(rng.permutation([i for i in range(per) if i != x])[:k - 1])
        return ev + ev[:1], x
    if kind == "toolong":
        return [(x, "toolong")] + good([k] + others + list(range(k + 1, per))), x
    if kind == "bb0":
        return good(rng.permutation(per)), None
    if kind == "nofec":
        return good(rng.permutation(k)), None
    if kind == "stress":
        return good([x] * STRESS_COPIES + [k] + others + list(range(k + 1, per))), x
    raise AssertionError(kind)


_CASES = {}


def build_arrivals(O, k, m, order_seed=0):
    """One arrival stream and what the rule says about it (cached, read-only).  order_seed
    changes only how the groups' arrivals are interleaved: every group sees the same packets in
    the same order, so bb and every per-group result are the same for all seeds, while the
    arrival indices (arr_state, arr_at) are not."""
    from quic_amd import fec
    key = (k, m, order_seed)
    if key in _CASES:
        return _CASES[key]
    s = sender(O, k, m)
    G, per, rmax, stride = max(s["G"], 2 * len(KINDS)), k + m, min(k, m), s["pkt_stride"]
    rng = np.random.default_rng(1234 * k + 7 * m)              # the groups' own events
    kinds = [KINDS[g % len(KINDS)] for g in range(G)]
    sgs = sender_groups(s, kinds)
    events, about = [], []
    for g in range(G):
        ev, x = group_events(kinds[g], k, m, rng)
        events.append(ev)
        about.append(x)
    # the merge: which group the next arrival belongs to; four stray tags among them
    merge = np.repeat(np.arange(G), [len(ev) for ev in events])
    strays = [(-1, 0), (G, 1), (0, per), (G - 1, 255)]
    merge = np.concatenate([merge, -1 - np.arange(len(strays))])
    if merge.size % 64 == 0:
        strays.append((-7, 3))
        merge = np.append(merge, -len(strays))
    merge = np.random.default_rng(99 + order_seed).permutation(merge)
    n = merge.size
    wire = np.zeros((n, stride), np.uint8)
    wlen, ad = np.zeros(n, np.int32), np.zeros(n, np.int32)
    grp, idx = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    pn = np.ones(n, np.uint8)
    what = [None] * n
    nxt = [0] * G
    trng = np.random.default_rng(55)
    for a, g in enumerate(merge):
        if g < 0:                                              # a stray tag on a real packet
            grp[a], idx[a] = strays[-1 - g]
            p, what[a] = int(trng.integers(s["n"])), "stray"
        else:
            i, what[a] = events[g][nxt[g]]
            nxt[g] += 1
            grp[a], idx[a] = g, i
            sg = sgs[g]
            p = sg * per + i
            if i < k:
                pn[a] = s["pn"][sg * k + i]
        wire[a], wlen[a], ad[a] = s["pkt"][p], s["plen"][p], s["hdr_len"][p]
        if what[a] == "tamper":                                # a tag byte or a plaintext byte
            cl = int(wlen[a] - ad[a])
            wire[a, ad[a] + int(trng.integers(12 + max(1, cl - 12))) % cl] ^= 0x10
        if what[a] == "toolong":
            wlen[a] = -1                                       # sealed below, once bb is known
    bb = fec.arrivals_rx_block_bytes(k, m, G, grp, idx, wlen, ad)
    for g in range(G):
        if kinds[g] == "bb0":
            bb[g] = 0
    for a in range(n):
        if what[a] == "toolong":
            g = int(grp[a])
            ln = int(bb[g]) - 1
            p = sgs[g] * per + int(idx[a])
            row, rl = O.null_seal_batch(s["hdr"][p:p + 1], s["hdr_len"][p:p + 1],
                                        trng.integers(0, 256, (1, ln), dtype=np.uint8),
                                        np.array([ln], np.int32), stride)
            assert rl[0] == ad[a] + 12 + ln
            wire[a], wlen[a] = row[0], rl[0]
    bbs = [int(b) for b in bb]
    # step 2 of the rule: the oracle's NullDecrypter and the length checks
    plain, res = O.null_open_batch(wire, wlen, ad, (max(bbs) + 12 + 3) // 4 * 4 + 64)
    arr = []
    for a in range(n):
        g, i = int(grp[a]), int(idx[a])
        pl = int(res[a])
        if 0 <= g < G and i < per:
            lim = bbs[g] - 2 if i < k else bbs[g]
            if bbs[g] < 1 or pl > lim:
                pl = -1
        arr.append((g, i, pl))
    acc, states = accept(k, m, G, arr)
    arr_at = np.full(G * per, -1, np.int32)
    for g in range(G):
        for a in acc[g]:
            arr_at[g * per + arr[a][1]] = a
    c = dict(k=k, m=m, G=G, per=per, n=n, rmax=rmax, pkt_stride=stride, kinds=kinds, about=about,
             wire=wire, wire_len=wlen, hdr_len=ad, pn=pn, grp=grp, idx=idx, what=what, bb=bb,
             bbs=bbs, arr=arr, acc=acc, states=np.array(states, np.int32), arr_at=arr_at,
             sender=s, sgs=sgs, rev_stride=REV_STRIDE)
    lrng = np.random.default_rng(77 * k + m)
    c["blocks_off"], c["blocks_bytes"] = packed_gaps(k, bbs, lrng)
    c["rec_off"], c["rec_bytes"] = packed_gaps(rmax, bbs, lrng)
    # the accepted packets placed by slot, for the slot-order receiver
    c["slot_wire"] = np.zeros((G * per, stride), np.uint8)
    c["slot_len"] = np.full(G * per, -1, np.int32)
    c["slot_ad"] = np.zeros(G * per, np.int32)
    c["slot_pn"] = np.ones(G * per, np.uint8)
    for p in np.flatnonzero(arr_at >= 0):
        a = arr_at[p]
        c["slot_wire"][p], c["slot_len"][p] = wire[a], wlen[a]
        c["slot_ad"][p], c["slot_pn"][p] = ad[a], pn[a]
    # ref_framing.revive on the accepted lists
    c["revived"] = {}
    for g in range(G):
        if len(acc[g]) < k:
            continue
        stored = []
        for a in acc[g]:
            i, pt = arr[a][1], plain[a, :arr[a][2]].tobytes()
            stored.append((BASE + i, R.prefix(pt, int(pn[a])) if i < k else pt))
        rev, rc = R.revive(O, k, m, BASE, stored)
        assert rc == 0
        c["revived"][g] = {pnum - BASE: (pay, pnl) for pnum, pay, pnl in rev}
    # the kinds did what they were built for
    st = c["states"]
    of = lambda g, i: [a for a in range(n) if grp[a] == g and idx[a] == i]   # noqa: E731
    for g, kind in enumerate(kinds):
        x, sg = about[g], sgs[g]
        mine = [a for a in range(n) if grp[a] == g and what[a] != "stray"]
        if kind in ("inorder", "late_fec"):
            assert sorted(arr[a][1] for a in acc[g]) == list(range(k))
            # the FEC packets are late; where the k data packets alone give a bb that is not a
            # multiple of 8, an FEC packet is longer than bb and rejected before it can be late
            fate = -4 if bbs[g] == s["bbs"][sg] else -1
            assert all(st[a] == fate for a in mine if idx[a] >= k) and not c["revived"][g]
        if kind == "shuffled_loss":
            assert len(acc[g]) == k and x in c["revived"][g]
        if kind == "dup_data":
            assert [st[a] >= 0 or st[a] == -4 for a in of(g, x)[:1]] == [True]
            assert st[of(g, x)[1]] == -3
        if kind == "dup_fec":
            assert st[of(g, k)[0]] == bbs[g] and st[of(g, k)[1]] == -3 and x in c["revived"][g]
        if kind == "tamper_first":
            assert [st[a] for a in of(g, x)] == [-1, int(s["pay_len"][sg * k + x])]
        if kind == "tamper_only":
            assert [st[a] for a in of(g, x)] == [-1] and x in c["revived"][g]
        if kind == "late_data":
            assert [st[a] for a in of(g, x)] == [-4]
            assert c["revived"][g][x][0] == s["payloads"][sg][x]   # the bytes it was sent with
        if kind == "fewer":
            assert len(acc[g]) == k - 1 and -3 in [st[a] for a in mine]
        if kind == "toolong":
            assert [st[a] for a in of(g, x)] == [-1] and wlen[of(g, x)[0]] - \
                ad[of(g, x)[0]] - 12 == bbs[g] - 1 and x in c["revived"][g]
        if kind == "bb0":
            assert all(st[a] == -1 for a in mine) and not acc[g]
        if kind == "nofec":
            assert len(acc[g]) == k and not c["revived"][g]
        if kind == "stress":
            assert [st[a] for a in of(g, x)].count(-3) == STRESS_COPIES - 1
    assert any(bbs[g] % 8 for g in range(G) if kinds[g] == "nofec")
    assert any(st[a] == -4 and idx[a] >= k for a in range(n))  # a late FEC packet
    assert any(st[a] == -4 and idx[a] < k for a in range(n))   # a late data packet
    assert [int(st[a]) for a in range(n) if what[a] == "stray"] == [-2] * len(strays)
    assert n % 64 and len({int(g) for g in grp[:64]}) > 8      # a wave mixes groups
    _CASES[key] = c
    return c


# ---------------------------------------------------------------- device runs
def pn_arg(c, key):
    pn = T.PN_ALL.get((c["k"], c["m"]))
    return dev(c[key]) if pn is None else pn


def out_tensors(c, with_state=True):
    import torch
    t = T.recv_tensors(dict(c, n=c["G"] * c["per"]))         # open_len is per slot
    t["arr_at"] = torch.full((c["G"] * c["per"],), 7, dtype=torch.int32, device="cuda")
    if with_state:
        t["arr_state"] = torch.full((c["n"],), 7, dtype=torch.int32, device="cuda")
    return t


def ring_args(c):
    """The ring as the socket left it: packet rows at odd addresses, guarded."""
    import torch
    if c["n"]:
        wire, hw = guarded_from(c["wire"], offset=1)
    else:                                                    # an empty tensor has no address
        wire, hw = torch.zeros((0, c["pkt_stride"]), dtype=torch.uint8, device="cuda"), None
    return dict(wire=wire, hw=hw, wire_len=dev(c["wire_len"]), hdr_len=dev(c["hdr_len"]),
                pn=pn_arg(c, "pn"), grp=dev(c["grp"]), idx=dev(c["idx"]), bb=dev(c["bb"]),
                blocks_off=dev(c["blocks_off"]), rec_off=dev(c["rec_off"]))


def call_arrivals(engine, c, a, blocks, rec, rev, t, stream=None):
    engine.open_decode_extract_arrivals_ragged(
        c["k"], c["m"], a["bb"], a["wire"], a["wire_len"], a["hdr_len"], a["pn"], a["grp"],
        a["idx"], t.get("arr_state"), t["arr_at"], blocks, a["blocks_off"], t["rows"],
        t["open_len"], rec, a["rec_off"], t["rec_rows"], rev, t["rev_len"],
        rev_pn_len=t["rev_pn"], status=t["status"], stream=stream)


def run_arrivals(engine, c, with_state=True):
    from quic_amd import fec
    blocks, hb = guarded((c["blocks_bytes"],))
    rec, hr = guarded((c["rec_bytes"],))
    rev, hv = guarded((c["G"] * c["rmax"], c["rev_stride"]), offset=5)
    t = out_tensors(c, with_state)
    a = ring_args(c)
    call_arrivals(engine, c, a, blocks, rec, rev, t)
    out = dict(kernels=fec.last_kernels(), blocks=host(blocks), rec=host(rec), rev=host(rev))
    out.update({name: host(v) for name, v in t.items()})
    for h in (hb, hr, hv, a["hw"]):
        if h is not None:
            h.check_guards()
    return out


_SLOT = {}


def run_slot_order(engine, c):
    """qfec_open_decode_extract_batch_ragged on the accepted packets placed by slot on the host
    (once per shape: the placement does not depend on how the groups were interleaved)."""
    key = (c["k"], c["m"])
    if key in _SLOT:
        return _SLOT[key]
    blocks, hb = guarded((c["blocks_bytes"],))
    rec, hr = guarded((c["rec_bytes"],))
    rev, hv = guarded((c["G"] * c["rmax"], c["rev_stride"]), offset=5)
    t = T.recv_tensors(dict(c, n=c["G"] * c["per"]))
    engine.open_decode_extract_ragged(
        c["k"], c["m"], dev(c["bb"]), dev(c["slot_wire"]), dev(c["slot_len"]), dev(c["slot_ad"]),
        pn_arg(c, "slot_pn"), blocks, dev(c["blocks_off"]), t["rows"], t["open_len"], rec,
        dev(c["rec_off"]), t["rec_rows"], rev, t["rev_len"], rev_pn_len=t["rev_pn"],
        status=t["status"])
    out = dict(blocks=host(blocks), rec=host(rec), rev=host(rev))
    out.update({name: host(v) for name, v in t.items()})
    for h in (hb, hr, hv):
        h.check_guards()
    _SLOT[key] = out
    return out


def check_arrivals(c, out, ref):
    """out: the arrivals call; ref: the slot-order call on the accepted packets."""
    k, G, per, rmax = c["k"], c["G"], c["per"], c["rmax"]
    # 1. the rule
    if "arr_state" in out:
        np.testing.assert_array_equal(out["arr_state"], c["states"])
    np.testing.assert_array_equal(out["arr_at"], c["arr_at"])
    # 2. everything else is the slot-order call's
    exp_ol = np.full(G * per, -1, np.int32)
    for p in np.flatnonzero(c["arr_at"] >= 0):
        exp_ol[p] = c["arr"][c["arr_at"][p]][2]
    np.testing.assert_array_equal(out["open_len"], exp_ol)
    for name in ("open_len", "rows", "status", "rec_rows", "rev_len", "rev_pn", "rev"):
        np.testing.assert_array_equal(out[name], ref[name], err_msg=name)
    # blocks: every filled slot; a slot whose row is 255 is unspecified; gaps keep the fill
    filled = np.zeros(c["blocks_bytes"], bool)
    inside = np.zeros(c["blocks_bytes"], bool)
    for g, b in enumerate(c["bbs"]):
        o = int(c["blocks_off"][g])
        inside[o:o + k * b] = True
        for i in range(k):
            if ref["rows"][g, i] != 255:
                filled[o + i * b:o + (i + 1) * b] = True
    np.testing.assert_array_equal(out["blocks"][filled], ref["blocks"][filled])
    assert (out["blocks"][~inside] == FILL).all()
    # rec: the recovered blocks of the status-0 groups; unused entries and gaps keep the fill
    used = np.zeros(c["rec_bytes"], bool)
    free = np.zeros(c["rec_bytes"], bool)
    for g, b in enumerate(c["bbs"]):
        o = int(c["rec_off"][g])
        if ref["status"][g] != 0:
            free[o:o + rmax * b] = True
        for j in range(rmax):
            if ref["rec_rows"][g, j] != 255:
                used[o + j * b:o + (j + 1) * b] = True
    np.testing.assert_array_equal(out["rec"][used], ref["rec"][used])
    assert (out["rec"][~used & ~free] == FILL).all()
    # 3. ref_framing.revive on the accepted lists
    for g in range(G):
        rows = [int(x) for x in out["rec_rows"][g] if x != 255]
        if len(c["acc"][g]) < k:
            assert out["status"][g] == -3 and not rows
            assert (out["rev_len"][g * rmax:(g + 1) * rmax] == -1).all()
            continue
        assert out["status"][g] == 0, (g, c["kinds"][g])
        assert rows == sorted(c["revived"][g])
        for j, x in enumerate(rows):
            pay, pnl = c["revived"][g][x]
            q = g * rmax + j
            assert out["rev_len"][q] == len(pay) and out["rev_pn"][q] == pnl
            assert bytes(out["rev"][q, :len(pay)]) == pay


# ---------------------------------------------------------------- 1. every shape
@pytest.mark.parametrize("k,m", sorted(SHAPES))
def test_arrivals_vs_rule_and_slot_order(engine, oracle, k, m):
    """arr_state and arr_at equal accept(); open_len, rows, the placed blocks, rec, rec_rows,
    status, rev, rev_len and rev_pn_len equal the slot-order call on the accepted packets; the
    revived payloads equal ref_framing.revive on the accepted lists; guards and gaps are
    untouched."""
    c = build_arrivals(oracle, k, m)
    check_arrivals(c, run_arrivals(engine, c), run_slot_order(engine, c))


def test_late_data_packet_is_revived(engine, oracle):
    """A data packet behind its group's k-th (an FEC packet among those) carries state -4 and
    comes back revived, byte for byte what was sent."""
    c = build_arrivals(oracle, 5, 5)
    out = run_arrivals(engine, c)
    gs = [g for g in range(c["G"]) if c["kinds"][g] == "late_data"]
    assert len(gs) >= 2
    for g in gs:
        x, s = c["about"][g], c["sender"]
        (a,) = [a for a in range(c["n"]) if c["grp"][a] == g and c["idx"][a] == x]
        assert out["arr_state"][a] == -4 and out["arr_at"][g * c["per"] + x] == -1
        j = [int(r) for r in out["rec_rows"][g]].index(x)
        q = g * c["rmax"] + j
        sent = s["payloads"][c["sgs"][g]][x]
        assert out["rev_len"][q] == len(sent) and bytes(out["rev"][q, :len(sent)]) == sent


# ---------------------------------------------------------------- 2. n = 0, no arr_state
def test_no_arrivals(engine, oracle):
    """n = 0: every group status -3, no slot bound, no block placed and nothing revived (the rec
    bytes of a group whose status is not 0 are unspecified, as in the slot-order call)."""
    import torch
    c = dict(build_arrivals(oracle, 10, 1))
    c.update(n=0, wire=c["wire"][:0], wire_len=c["wire_len"][:0], hdr_len=c["hdr_len"][:0],
             pn=c["pn"][:0], grp=c["grp"][:0], idx=c["idx"][:0])
    out = run_arrivals(engine, c)
    G, per = c["G"], c["per"]
    assert (out["status"] == -3).all() and (out["arr_at"] == -1).all()
    assert (out["open_len"] == -1).all() and (out["rows"] == 255).all()
    assert (out["rec_rows"] == 255).all() and (out["rev_len"] == -1).all()
    assert out["arr_state"].size == 0 and out["arr_at"].size == G * per
    for name in ("blocks", "rev"):
        assert (out[name] == FILL).all(), name
    assert "open_arrivals_kernel" not in out["kernels"]
    torch.cuda.synchronize()


def test_without_arr_state(engine, oracle):
    c = build_arrivals(oracle, 2, 2)
    out = run_arrivals(engine, c, with_state=False)
    assert "arr_state" not in out and "arrivals_state_kernel" not in out["kernels"]
    check_arrivals(c, out, run_slot_order(engine, c))


@pytest.mark.parametrize("k,m", [(5, 5), (32, 4), (250, 5)])
def test_without_the_optimistic_write(oracle, k, m):
    """arr_optimistic = 0: no pre-pass, the assemble places every accepted packet; the same
    results."""
    from quic_amd.fec import FecEngine
    c = build_arrivals(oracle, k, m)
    eng = FecEngine(0)
    try:
        assert eng.get_option("arr_optimistic") == 1
        eng.set_option("arr_optimistic", 0)
        out = run_arrivals(eng, c)
        assert out["kernels"].split(" + ")[:4] == [x for x in KERNELS if x != "arrivals_pre_kernel"]
        check_arrivals(c, out, run_slot_order(eng, c))
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. names and limits
def test_arrivals_kernel_names_and_limits(engine, oracle):
    import ctypes
    import torch
    c = build_arrivals(oracle, 5, 5)
    names = run_arrivals(engine, c)["kernels"].split(" + ")
    assert names[:5] == KERNELS
    assert names[-1] == "extract_revived_kernel" and "gf_ragged_kernel<decode>" in names
    assert not any(x.startswith("open_group_kernel") for x in names)

    L, h = engine.lib, engine._h
    vp = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731

    def recv(k, m, null=None, n=7, groups=1, rev_stride=1351, pkt_stride=1400):
        per, rmax = k + m, min(k, m)
        t = dict(bb=dev(np.array([1352], np.int32)), off=dev(np.zeros(1, np.int64)),
                 pkt=torch.zeros((7, 1400), dtype=torch.uint8, device="cuda"),
                 plen=torch.full((7,), -1, dtype=torch.int32, device="cuda"),
                 grp=torch.zeros((7,), dtype=torch.int32, device="cuda"),
                 idx=torch.zeros((7,), dtype=torch.uint8, device="cuda"),
                 state=torch.full((7,), 7, dtype=torch.int32, device="cuda"),
                 at=torch.full((per,), 7, dtype=torch.int32, device="cuda"),
                 blocks=torch.full((k * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rows=torch.full((k,), 9, dtype=torch.uint8, device="cuda"),
                 ol=torch.full((per,), 7, dtype=torch.int32, device="cuda"),
                 rec=torch.full((rmax * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rr=torch.full((rmax,), 9, dtype=torch.uint8, device="cuda"),
                 st=torch.full((1,), 7, dtype=torch.int32, device="cuda"),
                 rev=torch.full((rmax, 1351), FILL, dtype=torch.uint8, device="cuda"),
                 rl=torch.full((rmax,), 7, dtype=torch.int32, device="cuda"))
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        rc = L.qfec_open_decode_extract_arrivals_ragged(
            h, k, m, groups, a["bb"], n, a["pkt"], pkt_stride, a["plen"], None, 16, None, 1,
            a["grp"], a["idx"], a["state"], a["at"], a["blocks"], a["off"], a["rows"], a["ol"],
            a["rec"], a["off"], a["rr"], a["st"], a["rev"], rev_stride, a["rl"], None, None)
        torch.cuda.synchronize()
        if rc:
            for name, fill in (("state", 7), ("at", 7), ("blocks", FILL), ("rows", 9), ("ol", 7),
                               ("rec", FILL), ("rr", 9), ("st", 7), ("rev", FILL), ("rl", 7)):
                assert (host(t[name]) == fill).all(), name
        elif groups == 0:                                    # every tag is outside the batch
            assert (host(t["state"]) == -2).all()
            assert (host(t["at"]) == 7).all() and (host(t["st"]) == 7).all()
        else:
            assert (host(t["at"]) == -1).all() and (host(t["st"]) == -3).all()
            assert (host(t["state"]) == (7 if null == "state" or n == 0 else -1)).all()
        return rc

    assert recv(250, 5) == 0                                 # k + m = 255
    assert recv(250, 6) == -2
    assert recv(10, 1, null="state") == 0                    # arr_state may be NULL
    assert recv(10, 1, n=0) == 0
    assert recv(10, 1, groups=0) == 0
    assert recv(10, 1, n=-1) == -2
    assert recv(10, 1, n=1 << 31) == -2                      # arrival indices are int32
    assert recv(10, 1, groups=(1 << 31) // 11 + 1) == -2     # and so are slots
    assert recv(10, 1, groups=-1) == -2
    assert recv(10, 1, rev_stride=-1) == -2
    assert recv(10, 1, pkt_stride=0) == -2
    for null in ("bb", "pkt", "plen", "grp", "idx", "at", "blocks", "off", "rows", "ol", "rec",
                 "rr", "rev", "rl"):
        assert recv(10, 1, null=null) == -2, null


# ---------------------------------------------------------------- 4. graph capture
def test_arrivals_graph_capture(oracle):
    """One capture after qfec_reserve, replayed twice with two arrival orders written into the
    same buffers between the replays: each replay gives its own order's eager result, so the
    binding table is set up again inside the call."""
    import torch
    from quic_amd.fec import FecEngine
    k, m = 32, 4
    orders = [build_arrivals(oracle, k, m, seed) for seed in (1, 2)]
    c = orders[0]
    assert orders[1]["n"] == c["n"] and (orders[1]["grp"] != c["grp"]).any()
    assert (orders[1]["arr_at"] != c["arr_at"]).any()
    np.testing.assert_array_equal(orders[1]["bb"], c["bb"])
    eng = FecEngine(0)
    try:
        ref = run_slot_order(eng, c)
        eng.reserve(k, m, int(c["bb"].max()), c["G"])
        a = ring_args(c)
        assert not isinstance(a["pn"], int)
        t = out_tensors(c)
        fills = dict(rows=9, open_len=7, rec_rows=9, status=7, rev_len=7, rev_pn=FILL, arr_at=7,
                     arr_state=7)
        bufs = dict(blocks=torch.full((c["blocks_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                    rec=torch.full((c["rec_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                    rev=torch.full((c["G"] * c["rmax"], c["rev_stride"]), FILL,
                                   dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call_arrivals(eng, c, a, bufs["blocks"], bufs["rec"], bufs["rev"], t,
                          stream=s.cuda_stream)
        torch.cuda.synchronize()
        for o in (orders[1], orders[0]):
            for name, v in t.items():
                v.fill_(fills[name])
            for v in bufs.values():
                v.fill_(FILL)
            a["hw"].load(o["wire"])
            for name, key in (("wire_len", "wire_len"), ("hdr_len", "hdr_len"), ("pn", "pn"),
                              ("grp", "grp"), ("idx", "idx")):
                a[name].copy_(torch.from_numpy(o[key]))
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            got = {name: host(v) for name, v in {**t, **bufs}.items()}
            check_arrivals(o, got, ref)
            a["hw"].check_guards()
    finally:
        eng.close()
