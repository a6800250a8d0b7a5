"""GPU: the receiver window (qfec_rxwin_*) against the one-shot arrival-order call over the whole
ring (the code tests/test_gpu_arrivals.py checks against the rule) and against the carried rule
(tests/test_rxwin_abi.Carry).  Everything is bit-exact.

The streams are tests/test_gpu_arrivals.build_arrivals' as they stand, pushed whole, cut in the
middle, cut at seeded random points into 5 and 11 pieces with an empty push among them, and for
(2, 2) and (10, 1) one arrival per push.  Every push writes outputs of its own (stacked, guard
filled), so that what a push must leave alone can be seen; they are read back once, after the
last push.

A script is a list of steps ("push", arrival indices, bb) / ("release", groups or None); plan()
runs it through Carry on the host, run() through the window on the device, expect() turns the
plan and the one-shot reference into the arrays run() must give."""
import numpy as np
import pytest

from quic_amd import fec
from tests import test_gpu_arrivals as A
from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_pp_ragged import dev, host, packed_gaps
from tests.test_rxwin_abi import CUT_KINDS, HOLD, KERNELS, SHAPES, Carry, cut_points

pytestmark = pytest.mark.gpu

REV_STRIDE = A.REV_STRIDE


# ---------------------------------------------------------------- host side
def raw_pl(c):
    """The plaintext length each arrival opens with where the length checks let it: every packet
    of the streams is sealed properly but the tampered ones."""
    pl = (c["wire_len"].astype(np.int64) - c["hdr_len"] - 12)
    return np.where(np.array(c["what"]) == "tamper", -1, pl)


def eff_arr(c, idx, bb):
    """accept()'s (group, index, pl) of the arrivals idx under the block sizes bb of one push."""
    k, per, G, raw = c["k"], c["per"], c["G"], raw_pl(c)
    out = []
    for a in idx:
        g, i, pl = int(c["grp"][a]), int(c["idx"][a]), int(raw[a])
        if 0 <= g < G and i < per:
            b = int(bb[g])
            if b < 1 or b > HOLD or pl > (b - 2 if i < k else b):
                pl = -1
        out.append((g, i, pl))
    return out


def plan(c, script):
    """Per push: dict(idx, bb, states, done, neg3, before) with done = the groups that take their
    k-th packet (neg3: those among them that hold a packet larger than the push's bb) and
    before = the groups delivered before this push and not released since."""
    k, carry, delivered, sizes, out = c["k"], Carry(c["k"], c["m"], c["G"]), set(), {}, []
    for step in script:
        if step[0] == "release":
            gs = range(c["G"]) if step[1] is None else [g for g in step[1] if 0 <= g < c["G"]]
            carry.release(gs)
            delivered -= set(gs)
            for g in gs:
                sizes.pop(g, None)
            continue
        _, idx, bb = step
        arr = eff_arr(c, idx, bb)
        before = set(delivered)
        states, done = carry.push(arr)
        for (g, i, pl), s in zip(arr, states):
            if s >= 0:
                sizes.setdefault(g, []).append(pl + (2 if i < k else 0))
        neg3 = {g for g in done if max(sizes[g]) > int(bb[g])}
        delivered |= set(done)
        out.append(dict(idx=np.asarray(idx, np.int64), bb=np.asarray(bb, np.int32),
                        states=np.array(states, np.int32).reshape(-1), done=set(done), neg3=neg3,
                        before=before))
    return out


def pushes_of(c, cuts, bb=None):
    bb = c["bb"] if bb is None else bb
    return [("push", np.arange(a, b), bb) for a, b in zip(cuts[:-1], cuts[1:])]


def expect(c, ref, pl):
    """What run() must give for the plan pl; ref: the one-shot call over a ring whose accepted
    packets per completing group are the plan's, with the bb the group completes with."""
    G, rmax, P = c["G"], c["rmax"], len(pl)
    e = dict(status=np.full((P, G), fec.WIN_OPEN, np.int32),
             rec_rows=np.full((P, G, rmax), 255, np.uint8),
             rev_len=np.full((P, G * rmax), -1, np.int32),
             rev_pn=np.full((P, G * rmax), FILL, np.uint8),
             rec=np.full((P, c["rec_bytes"]), FILL, np.uint8),
             rev=np.full((P, G * rmax, REV_STRIDE), FILL, np.uint8),
             states=[p["states"] for p in pl])
    for p, step in enumerate(pl):
        for g in step["before"]:
            e["status"][p, g] = fec.WIN_DELIVERED
        for g in step["done"]:
            if g in step["neg3"]:
                e["status"][p, g] = -3
                continue
            b, o = int(step["bb"][g]), int(c["rec_off"][g])
            assert b == c["bbs"][g]                            # ref was made with this size
            e["status"][p, g] = ref["status"][g]
            e["rec_rows"][p, g] = ref["rec_rows"][g]
            for j in range(rmax):
                q = g * rmax + j
                if ref["rec_rows"][g, j] != 255:
                    e["rec"][p, o + j * b:o + (j + 1) * b] = ref["rec"][o + j * b:o + (j + 1) * b]
                e["rev_len"][p, q] = ref["rev_len"][q]
                if ref["rev_len"][q] >= 0:
                    e["rev"][p, q, :ref["rev_len"][q]] = ref["rev"][q, :ref["rev_len"][q]]
                    e["rev_pn"][p, q] = ref["rev_pn"][q]
    return e


# ---------------------------------------------------------------- device side
_REF = {}


def one_shot(engine, c):
    """qfec_open_decode_extract_arrivals_ragged over the whole ring (once per shape)."""
    key = (c["k"], c["m"])
    if key not in _REF:
        _REF[key] = A.run_arrivals(engine, c)
        np.testing.assert_array_equal(_REF[key]["arr_state"], c["states"])
    return _REF[key]


def run(win, c, script, with_state=True, stream=None):
    """The script on the window.  Returns the pushes' outputs, stacked by push."""
    import torch
    G, rmax = c["G"], c["rmax"]
    steps = [s for s in script if s[0] == "push"]
    P, nmax = len(steps), max([len(s[1]) for s in script if s[0] == "push"] + [1])
    i32 = torch.int32
    t = dict(status=torch.full((P, G), 7, dtype=i32, device="cuda"),
             rec_rows=torch.full((P, G, rmax), 9, dtype=torch.uint8, device="cuda"),
             rev_len=torch.full((P, G * rmax), 7, dtype=i32, device="cuda"),
             rev_pn=torch.full((P, G * rmax), FILL, dtype=torch.uint8, device="cuda"))
    state = torch.full((P, nmax), 7, dtype=i32, device="cuda")
    rec, hr = guarded((P, c["rec_bytes"]))
    rev, hv = guarded((P, G * rmax, REV_STRIDE), offset=5)
    wire, hw = guarded_from(c["wire"], offset=1)              # the ring: rows at odd addresses
    rec_off, pn_all = dev(c["rec_off"]), A.T.PN_ALL.get((c["k"], c["m"]))
    kernels, p = [], 0
    for step in script:
        if step[0] == "release":
            win.release(None if step[1] is None else dev(np.asarray(step[1], np.int32)))
            continue
        _, idx, bb = step
        idx = np.asarray(idx, np.int64)
        n = idx.size
        if n and (np.diff(idx) == 1).all():                   # a piece of the ring, where it lies
            pkt = wire[int(idx[0]):int(idx[0]) + n]
        else:                                                  # a ring of its own
            pkt = wire[:0] if n == 0 else guarded_from(c["wire"][idx], offset=1)[0]
        win.push(dev(np.asarray(bb, np.int32)), pkt, dev(c["wire_len"][idx]),
                 dev(c["hdr_len"][idx]), dev(c["pn"][idx]) if pn_all is None else pn_all,
                 dev(c["grp"][idx]), dev(c["idx"][idx]), state[p, :n] if with_state else None,
                 rec[p], rec_off, t["rec_rows"][p], rev[p], t["rev_len"][p],
                 rev_pn_len=t["rev_pn"][p], status=t["status"][p], stream=stream)
        kernels.append(fec.last_kernels())
        p += 1
    out = {name: host(v) for name, v in t.items()}
    out.update(rec=host(rec), rev=host(rev), kernels=kernels)
    st = host(state)
    out["states"] = [st[q, :len(s[1])] for q, s in enumerate(steps)]
    for h in (hr, hv, hw):
        h.check_guards()
    return out


def check(out, e, with_state=True):
    if with_state:
        for p, (got, want) in enumerate(zip(out["states"], e["states"])):
            np.testing.assert_array_equal(got, want, err_msg=f"arr_state of push {p}")
    for name in ("status", "rec_rows", "rev_len", "rev_pn", "rec", "rev"):
        np.testing.assert_array_equal(out[name], e[name], err_msg=name)


def window(engine, c):
    return engine.rxwin(c["k"], c["m"], c["G"], HOLD)


# ---------------------------------------------------------------- 1. every shape, every cut
@pytest.mark.parametrize("kind", CUT_KINDS)
@pytest.mark.parametrize("k,m", SHAPES)
def test_pushes_equal_the_one_shot_call(engine, oracle, k, m, kind):
    """The concatenated arr_state is the one-shot call's; every group's status, rec_rows,
    recovered blocks, revived payloads, rev_len and rev_pn_len are the one-shot call's in the push
    that brings its k-th packet; before it the group is WIN_OPEN, after it WIN_DELIVERED, with
    rec_rows 255, rev_len -1 and its rec and rev bytes still the guard fill; a group with fewer
    than k stays WIN_OPEN."""
    c = A.build_arrivals(oracle, k, m)
    assert c["G"] >= 26 and int(c["bb"].max()) <= HOLD
    ref = one_shot(engine, c)
    script = pushes_of(c, cut_points(c["n"], kind, k, m))
    pl = plan(c, script)
    np.testing.assert_array_equal(np.concatenate([p["states"] for p in pl]), ref["arr_state"])
    assert set().union(*[p["done"] for p in pl]) == \
        {g for g in range(c["G"]) if len(c["acc"][g]) == k} and not any(p["neg3"] for p in pl)
    win = window(engine, c)
    try:
        check(run(win, c, script), expect(c, ref, pl))
    finally:
        win.close()


@pytest.mark.parametrize("k,m", [(2, 2), (10, 1)])
def test_one_arrival_per_push(engine, oracle, k, m):
    """Every arrival a push of its own: each slot is bound against state alone."""
    c = A.build_arrivals(oracle, k, m)
    ref = one_shot(engine, c)
    script = pushes_of(c, cut_points(c["n"], "each", k, m))
    win = window(engine, c)
    try:
        check(run(win, c, script), expect(c, ref, plan(c, script)))
    finally:
        win.close()


# ---------------------------------------------------------------- 2. options
@pytest.mark.parametrize("k,m", [(5, 5), (10, 1), (250, 5)])
def test_without_the_optimistic_write(oracle, k, m):
    """arr_optimistic = 0: no pre-pass, the assemble places every accepted packet from the ring
    into its row; the same outputs."""
    from quic_amd.fec import FecEngine
    c = A.build_arrivals(oracle, k, m)
    eng = FecEngine(0)
    try:
        ref = A.run_arrivals(eng, c)
        eng.set_option("arr_optimistic", 0)
        script = pushes_of(c, cut_points(c["n"], "r5", k, m))
        win = window(eng, c)
        out = run(win, c, script)
        assert all("rxwin_pre_kernel" not in names for names in out["kernels"])
        check(out, expect(c, ref, plan(c, script)))
        win.close()
    finally:
        eng.close()


def test_without_arr_state(engine, oracle):
    c = A.build_arrivals(oracle, 2, 2)
    script = pushes_of(c, cut_points(c["n"], "r5", 2, 2))
    win = window(engine, c)
    try:
        out = run(win, c, script, with_state=False)
        assert all("arrivals_state_kernel" not in names for names in out["kernels"])
        assert all((s == 7).all() for s in out["states"])
        check(out, expect(c, one_shot(engine, c), plan(c, script)), with_state=False)
    finally:
        win.close()


# ---------------------------------------------------------------- 3. release
@pytest.mark.parametrize("k,m", [(5, 5), (32, 4)])
def test_release_and_push_again(engine, oracle, k, m):
    """The ring, then half the groups released (with a stray and a repeated entry in the list),
    then the ring again: the released groups complete again with the same outputs, in the others
    every arrival that opens is a duplicate or late, exactly as Carry says.  Then release(None)
    and the ring a third time: as the first."""
    c = A.build_arrivals(oracle, k, m)
    ref, whole = one_shot(engine, c), pushes_of(c, [0, c["n"]])
    half = list(range(0, c["G"], 2))
    script = whole + [("release", half + [c["G"], -1, half[0]])] + whole + [("release", None)] + whole
    pl = plan(c, script)
    kept = np.isin(c["grp"], half, invert=True) & (pl[0]["states"] >= 0)
    assert kept.any() and np.isin(pl[1]["states"][kept], [fec.ARR_DUPLICATE, fec.ARR_LATE]).all()
    assert pl[1]["done"] == {g for g in pl[0]["done"] if g in half} and pl[1]["done"]
    assert pl[2]["done"] == pl[0]["done"] and not pl[2]["before"]
    np.testing.assert_array_equal(pl[2]["states"], pl[0]["states"])
    win = window(engine, c)
    try:
        check(run(win, c, script), expect(c, ref, pl))
    finally:
        win.close()


# ---------------------------------------------------------------- 4. bb per push
def grow_case(c):
    """A ring of its own: every data arrival of the stream, then every FEC arrival, each part in
    its order.  Returns (order, bb1, bb2): bb1 = the running value of the helper after the data
    part, bb2 = its final value (0 for the 'bb0' groups in both)."""
    k, m, G = c["k"], c["m"], c["G"]
    ln = np.where(np.array(c["what"]) == "toolong", -1, c["wire_len"]).astype(np.int32)
    data = np.flatnonzero(c["idx"] < k)
    order = np.concatenate([data, np.flatnonzero(c["idx"] >= k)])
    seen, bb = np.zeros((G, 32), np.uint8), np.zeros(G, np.int32)
    out = []
    for part in (order[:data.size], order[data.size:]):
        fec.arrivals_rx_block_bytes_carry(k, m, G, c["grp"][part], c["idx"][part], ln[part],
                                          c["hdr_len"][part], seen, bb)
        out.append(np.where(np.array(c["kinds"]) == "bb0", 0, bb).astype(np.int32))
    np.testing.assert_array_equal(
        bb, fec.arrivals_rx_block_bytes(k, m, G, c["grp"][order], c["idx"][order], ln[order],
                                        c["hdr_len"][order]))
    return order, out[0], out[1]


@pytest.mark.parametrize("k,m", [(5, 5), (32, 4)])
def test_bb_that_grows(engine, oracle, k, m):
    """A group's data packets pushed with the running bb of qfec_arrivals_rx_block_bytes_carry,
    then its FEC packets with the final one: a held row is the block of any bb up to
    hold_stride, so the result is the one-shot call's over the same ring with the final bb."""
    c = A.build_arrivals(oracle, k, m)
    order, bb1, bb2 = grow_case(c)
    assert (bb1 < bb2).any() and (bb1 <= bb2).all()
    d = dict(c)
    for name in ("wire", "wire_len", "hdr_len", "pn", "grp", "idx"):
        d[name] = c[name][order]
    d["what"] = [c["what"][a] for a in order]
    d["bb"], d["bbs"] = bb2, [int(b) for b in bb2]
    lrng = np.random.default_rng(31 * k + m)
    d["blocks_off"], d["blocks_bytes"] = packed_gaps(k, d["bbs"], lrng)
    d["rec_off"], d["rec_bytes"] = packed_gaps(c["rmax"], d["bbs"], lrng)
    ref = A.run_arrivals(engine, d)
    ndata = int((c["idx"] < k).sum())
    script = [("push", np.arange(ndata), bb1), ("push", np.arange(ndata, c["n"]), bb2)]
    pl = plan(d, script)
    # the construction: growing bb changes no arrival's fate
    np.testing.assert_array_equal(np.concatenate([p["states"] for p in pl]), ref["arr_state"])
    assert pl[1]["done"] and not pl[1]["neg3"]
    assert any(ref["rec_rows"][g, 0] != 255 and bb1[g] < bb2[g] for g in pl[1]["done"])
    win = window(engine, d)
    try:
        check(run(win, d, script), expect(d, ref, pl))
    finally:
        win.close()


def test_bb_shrunk_below_a_held_packet(engine, oracle):
    """A group's k-th packet, a short one, pushed with a bb that its held packets exceed: the
    group completes with status -3 and revives nothing; the groups beside it are not touched by
    it, and afterwards it is delivered."""
    k, m = 5, 5
    c = A.build_arrivals(oracle, k, m)
    ref, raw = one_shot(engine, c), raw_pl(c)
    pick = None
    for g in range(c["G"]):
        mine = [a for a in c["acc"][g] if c["idx"][a] < k]
        if len(mine) == k and min(raw[a] for a in mine) <= 6 and max(raw[a] for a in mine) > 6:
            pick = (g, mine)
            break
    assert pick, "no group with a short and a long data packet"
    g, mine = pick
    short = min(mine, key=lambda a: raw[a])
    others = np.array([a for a in range(c["n"]) if c["grp"][a] != g])
    small = c["bb"].copy()
    small[g] = 8
    script = [("push", np.array([a for a in mine if a != short]), c["bb"]),
              ("push", others, c["bb"]), ("push", np.array([short]), small),
              ("push", np.array(mine), c["bb"])]
    pl = plan(c, script)
    assert pl[2]["done"] == {g} and pl[2]["neg3"] == {g} and g in pl[3]["before"]
    assert pl[1]["done"] == {x for x in range(c["G"]) if len(c["acc"][x]) == k and x != g}
    win = window(engine, c)
    try:
        check(run(win, c, script), expect(c, ref, pl))
    finally:
        win.close()


def test_bb_zero_and_above_hold_stride_beside_healthy_groups(engine, oracle):
    """bb[g] = 0 and bb[g] > hold_stride: every packet of the group is rejected, the group stays
    open, nothing of it is written; the other groups complete as ever."""
    k, m = 32, 4
    c = A.build_arrivals(oracle, k, m)
    ref = one_shot(engine, c)
    full = [g for g in range(c["G"]) if len(c["acc"][g]) == k]
    bb = c["bb"].copy()
    bb[full[0]], bb[full[1]] = HOLD + 8, 0
    script = pushes_of(c, cut_points(c["n"], "half", k, m), bb)
    pl = plan(c, script)
    for p in pl:
        assert not p["done"] & set(full[:2])
        theirs = np.isin(c["grp"][p["idx"]], full[:2]) & (c["idx"][p["idx"]] < c["per"])
        assert theirs.any() and (p["states"][theirs] == fec.ARR_REJECTED).all()
    assert set().union(*[p["done"] for p in pl]) == set(full[2:])
    win = window(engine, c)
    try:
        check(run(win, c, script), expect(c, ref, pl))
    finally:
        win.close()


# ---------------------------------------------------------------- 5. late data, names, limits
def test_late_data_packet_in_a_later_push_is_revived(engine, oracle):
    """A data packet that arrives a push after its group's k-th is late there, and the group
    revived it, byte for byte, in the push before."""
    k, m = 5, 5
    c = A.build_arrivals(oracle, k, m)
    ref = one_shot(engine, c)
    gs = [g for g in range(c["G"]) if c["kinds"][g] == "late_data"]
    late = [int(np.flatnonzero((c["grp"] == g) & (c["idx"] == c["about"][g]))[0]) for g in gs]
    rest = np.array([a for a in range(c["n"]) if a not in late])
    script = [("push", rest, c["bb"]), ("push", np.array(late), c["bb"])]
    pl = plan(c, script)
    assert len(gs) >= 2 and set(gs) <= pl[0]["done"] and (pl[1]["states"] == fec.ARR_LATE).all()
    win = window(engine, c)
    try:
        out = run(win, c, script)
        check(out, expect(c, ref, pl))
        for g in gs:
            x, sent = c["about"][g], c["sender"]["payloads"][c["sgs"][g]][c["about"][g]]
            j = [int(r) for r in out["rec_rows"][0, g]].index(x)
            q = g * c["rmax"] + j
            assert out["rev_len"][0, q] == len(sent) and bytes(out["rev"][0, q, :len(sent)]) == sent
            assert out["status"][1, g] == fec.WIN_DELIVERED
    finally:
        win.close()


def test_kernel_names(engine, oracle):
    """The window's own kernels, the pointer-table decode's, and none of the ragged decode's, of
    the one-shot open's or a copy kernel's."""
    for (k, m), decode in (((5, 5), "gf_ptrs_kernel<decode>"), ((10, 1), "xor_ptrs_kernel")):
        c = A.build_arrivals(oracle, k, m)
        win = window(engine, c)
        try:
            names = run(win, c, pushes_of(c, [0, c["n"]]))["kernels"][0].split(" + ")
            win.release()
            assert fec.last_kernels() == "rxwin_release_kernel"
        finally:
            win.close()
        assert names[:5] == KERNELS
        assert names[-2:] == ["rxwin_finish_kernel", "extract_revived_kernel"] and decode in names
        assert not any(x.startswith(("gf_ragged", "xor_ragged", "copy_", "open_group", "open_arrivals",
                                     "arrivals_init", "arrivals_pre", "arrivals_assemble",
                                     "open_status")) for x in names), names


def test_create_and_push_limits(engine):
    import ctypes
    import torch
    L, h = engine.lib, engine._h

    def create(k, m, groups, hold):
        out = ctypes.c_void_p()
        rc = L.qfec_rxwin_create(h, k, m, groups, hold, ctypes.byref(out))
        if rc == 0:
            L.qfec_rxwin_destroy(out)
        else:
            assert out.value is None
        return rc, L.qfec_last_error().decode()

    assert create(250, 5, 1, 16)[0] == 0 and create(10, 1, 0, 16)[0] == 0
    for args, text in (((0, 1, 1, 16), "bad k"), ((256, 1, 1, 16), "k > 255"),
                       ((10, 1, -1, 16), "groups < 0"), ((250, 6, 1, 16), "k + m > 255"),
                       ((10, 1, (2**31 - 1) // 11 + 1, 16), "INT32_MAX"),
                       ((10, 1, 1, 8), "hold_stride"), ((10, 1, 1, 24), "hold_stride"),
                       ((10, 1, 1, 0), "hold_stride")):
        rc, msg = create(*args)
        assert rc == -2 and text in msg, (args, msg)
    rc, msg = create(10, 1, 1 << 24, 1 << 20)                # 176 TiB of hold rows
    assert rc < -2 and "memory" in msg, (rc, msg)
    assert create(10, 1, 4, 16)[0] == 0                      # and the context is as it was

    k, m, G = 10, 1, 2
    win = engine.rxwin(k, m, G, HOLD)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731
    t = dict(bb=dev(np.full(G, 1352, np.int32)), off=dev(np.arange(G, dtype=np.int64) * 1360),
             pkt=torch.zeros((7, 1400), dtype=torch.uint8, device="cuda"),
             plen=torch.full((7,), -1, dtype=torch.int32, device="cuda"),
             grp=torch.zeros((7,), dtype=torch.int32, device="cuda"),
             idx=torch.zeros((7,), dtype=torch.uint8, device="cuda"),
             state=torch.full((7,), 7, dtype=torch.int32, device="cuda"),
             rec=torch.full((G * 1360,), FILL, dtype=torch.uint8, device="cuda"),
             rr=torch.full((G,), 9, dtype=torch.uint8, device="cuda"),
             st=torch.full((G,), 7, dtype=torch.int32, device="cuda"),
             rev=torch.full((G, 1351), FILL, dtype=torch.uint8, device="cuda"),
             rl=torch.full((G,), 7, dtype=torch.int32, device="cuda"))

    def push(null=None, n=7, rev_stride=1351, pkt_stride=1400, rec_shift=0):
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        if rec_shift:
            a["rec"] = ctypes.c_void_p(t["rec"].data_ptr() + rec_shift)
        rc = L.qfec_rxwin_push(win._h, a["bb"], n, a["pkt"], pkt_stride, a["plen"], None, 16, None,
                               1, a["grp"], a["idx"], a["state"], a["rec"], a["off"], a["rr"],
                               a["st"], a["rev"], rev_stride, a["rl"], None, None)
        torch.cuda.synchronize()
        got = {name: host(v) for name, v in t.items()}
        if rc:
            for name, fill in (("state", 7), ("rec", FILL), ("rr", 9), ("st", 7), ("rev", FILL),
                               ("rl", 7)):
                assert (got[name] == fill).all(), name
        else:
            assert (got["st"] == (7 if null == "st" else fec.WIN_OPEN)).all()
            assert (got["rr"] == 255).all()
            assert (got["rl"] == -1).all() and (got["rec"] == FILL).all()
            assert (got["state"] == (7 if null == "state" or n == 0 else -1)).all()
            for name, fill in (("state", 7), ("rr", 9), ("st", 7), ("rl", 7)):
                t[name].fill_(fill)
        return rc

    try:
        for null in ("bb", "pkt", "plen", "grp", "idx", "rec", "off", "rr", "rev", "rl"):
            assert push(null=null) == -2, null
        assert push(n=-1) == -2 and push(n=1 << 31) == -2
        assert push(rev_stride=-1) == -2 and push(pkt_stride=0) == -2 and push(rec_shift=8) == -2
        assert push() == 0 and push(null="state") == 0 and push(null="st") == 0
        assert push(n=0) == 0
        for null in ("pkt", "plen", "grp", "idx"):            # nothing of them is read at n = 0
            assert push(null=null, n=0) == 0, null
        assert L.qfec_rxwin_release(win._h, -1, None, None) == -2
        assert L.qfec_rxwin_release(win._h, 1 << 31, vp(t["grp"]), None) == -2
        assert L.qfec_rxwin_release(win._h, 0, vp(t["grp"]), None) == 0
    finally:
        win.close()


# ---------------------------------------------------------------- 6. graph capture, two windows
def test_push_graph_capture(oracle):
    """One capture of push, replayed once per piece with each piece written into the same ring
    buffers (a short piece is filled up with arrivals tagged to no group): the state is carried
    from replay to replay, and the replays give what the eager pushes of the same pieces give."""
    import torch
    from quic_amd.fec import FecEngine
    k, m = 32, 4
    c = A.build_arrivals(oracle, k, m)
    G, rmax, n = c["G"], c["rmax"], c["n"]
    cap = (n + 3) // 4
    eng = FecEngine(0)
    try:
        ref = A.run_arrivals(eng, c)
        script = pushes_of(c, [0, cap, 2 * cap, 3 * cap, n])
        pl = plan(c, script)
        e = expect(c, ref, pl)
        eager = window(eng, c)
        check(run(eager, c, script), e)
        eager.close()
        win = window(eng, c)
        wire, hw = guarded((cap, c["pkt_stride"]), offset=1)
        a = dict(wire_len=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                 hdr_len=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                 pn=torch.ones(cap, dtype=torch.uint8, device="cuda"),
                 grp=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                 idx=torch.zeros(cap, dtype=torch.uint8, device="cuda"))
        t = dict(status=(torch.int32, (G,), 7), rec_rows=(torch.uint8, (G, rmax), 9),
                 rev_len=(torch.int32, (G * rmax,), 7), rev_pn=(torch.uint8, (G * rmax,), FILL),
                 states=(torch.int32, (cap,), 7), rec=(torch.uint8, (c["rec_bytes"],), FILL),
                 rev=(torch.uint8, (G * rmax, REV_STRIDE), FILL))
        fills = {name: f for name, (_, _, f) in t.items()}
        t = {name: torch.full(shape, f, dtype=dt, device="cuda") for name, (dt, shape, f) in t.items()}
        bb, rec_off = dev(c["bb"]), dev(c["rec_off"])
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            win.push(bb, wire, a["wire_len"], a["hdr_len"], a["pn"], a["grp"], a["idx"],
                     t["states"], t["rec"], rec_off, t["rec_rows"], t["rev"], t["rev_len"],
                     rev_pn_len=t["rev_pn"], status=t["status"], stream=s.cuda_stream)
        torch.cuda.synchronize()
        win.release()                                        # whatever the capture itself ran
        for p, step in enumerate(pl):
            idx, fill = step["idx"], cap - step["idx"].size
            for name, v in t.items():
                v.fill_(fills[name])
            hw.load(np.concatenate([c["wire"][idx], np.zeros((fill, c["pkt_stride"]), np.uint8)]))
            for name, key, pad in (("wire_len", "wire_len", 0), ("hdr_len", "hdr_len", 0),
                                   ("pn", "pn", 1), ("grp", "grp", -1), ("idx", "idx", 0)):
                a[name].copy_(torch.from_numpy(np.concatenate(
                    [c[key][idx], np.full(fill, pad, c[key].dtype)])))
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            got = {name: host(v) for name, v in t.items()}
            np.testing.assert_array_equal(got["states"][:idx.size], e["states"][p])
            assert (got["states"][idx.size:] == fec.ARR_IGNORED).all()
            for name in ("status", "rec_rows", "rev_len", "rev_pn", "rec", "rev"):
                np.testing.assert_array_equal(got[name], e[name][p], err_msg=f"{name}, replay {p}")
            hw.check_guards()
        win.close()
    finally:
        eng.close()


def test_two_windows_on_one_context(engine, oracle):
    """Two windows of different codes fed in turn, piece by piece, on one context: each gives what
    it gives alone (they share the context's decode workspace, not their state)."""
    cs = [A.build_arrivals(oracle, 5, 5), A.build_arrivals(oracle, 10, 1)]
    refs = [one_shot(engine, c) for c in cs]
    scripts = [pushes_of(c, cut_points(c["n"], "r5", c["k"], c["m"])) for c in cs]
    wins = [window(engine, c) for c in cs]
    try:
        # run() feeds a whole script; interleave the two by single-push scripts on live windows
        outs = [[], []]
        for p in range(5):
            for w in (0, 1):
                outs[w].append(run(wins[w], cs[w], [scripts[w][p]]))
        for w in (0, 1):
            e = expect(cs[w], refs[w], plan(cs[w], scripts[w]))
            got = {name: np.concatenate([o[name] for o in outs[w]])
                   for name in ("status", "rec_rows", "rev_len", "rev_pn", "rec", "rev")}
            got["states"] = [o["states"][0] for o in outs[w]]
            check(got, e)
    finally:
        for w in wins:
            w.close()
