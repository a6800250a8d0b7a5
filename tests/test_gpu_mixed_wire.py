"""GPU: the mixed-code wire path (qfec_frame_encode_seal_groups_batch_mixed,
qfec_open_decode_extract_arrivals_mixed) against the ragged calls run once per code on that
code's groups, which the existing tests pin to the oracle and tests/ref_framing.py, and
directly against accept_mixed() and ref_framing.revive.  Everything is bit-exact.

The cases are the per-shape cases of tests/test_gpu_framed.py and tests/test_gpu_arrivals.py,
taken as they are: their groups are interleaved by a seeded shuffle into one batch over a
nine-code set, their arrivals by a seeded merge that keeps each group's own order.  The batch
starts with 16 groups of (2, 2) (one 64-packet tile, the longest per-lane walk), holds (250, 5)
groups that span four tiles, and has one group without a code (code 200) in its middle, with
arrivals tagged to it.  The builders run on the CPU and are cached;
tests/test_mixed_wire_abi.py checks their construction without a GPU."""
import numpy as np
import pytest

from tests import test_gpu_arrivals as A
from tests import test_gpu_framed as T
from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_pp_ragged import dev, host

pytestmark = pytest.mark.gpu

SHAPES = [(10, 1), (2, 2), (5, 5), (32, 4), (10, 20), (250, 5)]
CODES = SHAPES + [(10, 10), (15, 15), (5, 5)]        # index 8: a second (5, 5)
KMAX = max(k for k, _ in CODES)
RMAX = max(min(k, m) for k, m in CODES)
NOCODE = 200
ROW_FILL = 9
KERNELS_RX = ["mixed_wire_plan_kernel", "arrivals_init_kernel", "arrivals_pre_kernel<mixed>",
              "open_arrivals_kernel<mixed>", "arrivals_assemble_kernel<mixed>",
              "arrivals_unowned_kernel", "arrivals_state_kernel<mixed>"]
KERNELS_TX = ["mixed_wire_plan_kernel", "frame_blocks_kernel<mixed>", "null_seal_kernel<mixed>"]


def up16(v):
    return (v + 15) & ~15


def code_index(ci, g):
    """The set index group g of shape ci names: every other (5, 5) group the duplicate."""
    return 8 if SHAPES[ci] == (5, 5) and g % 2 else ci


def group_order(counts, seed):
    """The batch's groups as (shape index, group of the shape's case), None for the group
    without a code: 16 groups of (2, 2) first, the rest shuffled, the codeless one in the middle."""
    two = SHAPES.index((2, 2))
    rest = [(ci, g) for ci, n in enumerate(counts) for g in range(n) if (ci, g) >= (two, 16) or ci != two]
    rng = np.random.default_rng(4242 + seed)
    rest = [rest[i] for i in rng.permutation(len(rest))]
    order = [(two, g) for g in range(16)] + rest
    order.insert(len(order) // 2, None)
    return order


def layout(order, bbs, nblk, rng):
    """Byte offsets (multiples of 16, with gaps) of each group's nblk(ci) blocks of bbs[g] bytes."""
    off, run = np.zeros(len(order), np.int64), 0
    for g, og in enumerate(order):
        off[g] = run
        if og is not None:
            run += up16(nblk(*SHAPES[og[0]]) * bbs[g]) + 16 * int(rng.integers(0, 3))
    return off, run + 16


# ---------------------------------------------------------------- receiver case
_RX = {}


def build_rx(O, seed=0, shapes=None):
    """The mixed arrival stream and where each piece of the per-code cases went (cached)."""
    from quic_amd import fec
    key = (seed, shapes)
    if key in _RX:
        return _RX[key]
    use = list(range(len(SHAPES))) if shapes is None else [SHAPES.index(s) for s in shapes]
    cases = {ci: A.build_arrivals(O, *SHAPES[ci]) for ci in use}
    order = group_order([cases[ci]["G"] if ci in cases else 0 for ci in range(len(SHAPES))], seed) \
        if shapes is None else [(ci, g) for ci in use for g in range(cases[ci]["G"])]
    G = len(order)
    where = {og: g for g, og in enumerate(order) if og is not None}
    code = np.array([NOCODE if og is None else code_index(*og) for og in order], np.uint8)
    bb = np.array([1352 if og is None else cases[og[0]]["bb"][og[1]] for og in order], np.int32)
    pkt_first, _ = fec.mixed_packet_layout(CODES, code)
    rng = np.random.default_rng(31 + seed)
    blocks_off, blocks_bytes = layout(order, bb, lambda k, m: k, rng)
    rec_off, rec_bytes = layout(order, bb, lambda k, m: min(k, m), rng)
    # the merge: which case the next arrival comes from; each case keeps its own order
    which = np.concatenate([np.full(cases[ci]["n"], ci) for ci in use])
    nocode = [g for g, og in enumerate(order) if og is None]
    if nocode:
        which = np.concatenate([which, np.full(8, -1)])
    which = np.random.default_rng(77 + seed).permutation(which)
    n = which.size
    stride = max(c["pkt_stride"] for c in cases.values())
    wire = np.zeros((n, stride), np.uint8)
    wlen, ad = np.zeros(n, np.int32), np.zeros(n, np.int32)
    grp, idx, pn = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.ones(n, np.uint8)
    src = [None] * n                                          # (shape index, arrival of its case)
    nxt = {ci: 0 for ci in use}
    amap = {ci: np.zeros(cases[ci]["n"], np.int64) for ci in use}
    arr = []
    first = cases[use[0]]
    for a, ci in enumerate(which):
        if ci < 0:                                            # a real packet tagged to the codeless group
            b = a % first["n"]
            wire[a, :first["pkt_stride"]] = first["wire"][b]
            wlen[a], ad[a] = first["wire_len"][b], first["hdr_len"][b]
            grp[a], idx[a] = nocode[0], a % 4
            arr.append((int(grp[a]), int(idx[a]), -1))
            continue
        c, b = cases[ci], nxt[ci]
        nxt[ci] += 1
        src[a] = (ci, b)
        amap[ci][b] = a
        wire[a, :c["pkt_stride"]] = c["wire"][b]
        wlen[a], ad[a], pn[a], idx[a] = c["wire_len"][b], c["hdr_len"][b], c["pn"][b], c["idx"][b]
        g = int(c["grp"][b])
        grp[a] = where[(ci, g)] if 0 <= g < c["G"] else (-1 if g < 0 else G)
        arr.append((int(grp[a]), int(idx[a]), c["arr"][b][2]))
    r = dict(seed=seed, cases=cases, use=use, order=order, where=where, G=G, code=code, bb=bb,
             pkt_first=pkt_first, npkt=int(pkt_first[-1]), blocks_off=blocks_off,
             blocks_bytes=blocks_bytes, rec_off=rec_off, rec_bytes=rec_bytes, n=n, wire=wire,
             wire_len=wlen, hdr_len=ad, grp=grp, idx=idx, pn=pn, src=src, amap=amap, arr=arr,
             pkt_stride=stride, rev_stride=A.REV_STRIDE, nocode=nocode)
    _RX[key] = r
    return r


def run_rx(engine, cs, r, with_state=True, pkt_first=None, npkt=None, n=None, rmax=RMAX,
           kmax=KMAX):
    """The mixed receiver into guarded buffers; every output on the host."""
    import torch
    from quic_amd import fec
    npkt = r["npkt"] if npkt is None else npkt
    n = r["n"] if n is None else n
    blocks, hb = guarded((r["blocks_bytes"],))
    rec, hr = guarded((r["rec_bytes"],))
    rev, hv = guarded((r["G"] * rmax, r["rev_stride"]), offset=5)
    handles = [hb, hr, hv]
    if n:
        wire, hw = guarded_from(r["wire"][:n], offset=1)
        handles.append(hw)
    else:
        wire = torch.zeros((0, r["pkt_stride"]), dtype=torch.uint8, device="cuda")
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")    # noqa: E731
    t = dict(rows=full((r["G"], kmax), ROW_FILL, torch.uint8),
             open_len=full((npkt,), 7, torch.int32), arr_at=full((npkt,), 7, torch.int32),
             rec_rows=full((r["G"], rmax), ROW_FILL, torch.uint8),
             status=full((r["G"],), 7, torch.int32), rev_len=full((r["G"] * rmax,), 7, torch.int32),
             rev_pn=full((r["G"] * rmax,), FILL, torch.uint8))
    if with_state:
        t["arr_state"] = full((n,), 7, torch.int32)
    engine.open_decode_extract_arrivals_mixed(
        cs, dev(r["code"]), dev(r["bb"]), dev(r["pkt_first"] if pkt_first is None else pkt_first),
        wire, dev(r["wire_len"][:n]), dev(r["hdr_len"][:n]), dev(r["pn"][:n]), dev(r["grp"][:n]),
        dev(r["idx"][:n]), t.get("arr_state"), t["arr_at"], blocks, dev(r["blocks_off"]), t["rows"],
        t["open_len"], rec, dev(r["rec_off"]), t["rec_rows"], rev, t["rev_len"],
        rev_pn_len=t["rev_pn"], status=t["status"])
    out = dict(kernels=fec.last_kernels(), blocks=host(blocks), rec=host(rec), rev=host(rev))
    out.update({name: host(v) for name, v in t.items()})
    for h in handles:
        h.check_guards()
    return out


_REF_RX = {}


def ref_rx(engine, r):
    """The parent's route: the ragged arrivals call once per code, on that code's case."""
    for ci in r["use"]:
        if ci not in _REF_RX:
            _REF_RX[ci] = A.run_arrivals(engine, r["cases"][ci])
    return _REF_RX


def check_group_rx(r, out, ref, g, og, rmax=RMAX, skip=()):
    """Group g of the mixed call against group og[1] of shape og[0]'s ragged call."""
    ci, sg = og
    c, o = r["cases"][ci], ref[ci]
    k, m = SHAPES[ci]
    per, rm, b = k + m, min(k, m), int(r["bb"][g])
    f = int(r["pkt_first"][g])
    tag = f"group {g} = shape {SHAPES[ci]} group {sg} ({c['kinds'][sg]})"
    np.testing.assert_array_equal(out["open_len"][f:f + per], o["open_len"][sg * per:(sg + 1) * per], tag)
    at = o["arr_at"][sg * per:(sg + 1) * per]
    np.testing.assert_array_equal(out["arr_at"][f:f + per],
                                  np.where(at >= 0, r["amap"][ci][np.maximum(at, 0)], -1), tag)
    np.testing.assert_array_equal(out["rows"][g, :k], o["rows"][sg], tag)
    assert (out["rows"][g, k:] == ROW_FILL).all(), tag
    np.testing.assert_array_equal(out["status"][g], o["status"][sg], tag)
    np.testing.assert_array_equal(out["rec_rows"][g, :rm], o["rec_rows"][sg], tag)
    assert (out["rec_rows"][g, rm:] == 255).all(), tag
    bo, co = int(r["blocks_off"][g]), int(c["blocks_off"][sg])
    for i in range(k):
        if o["rows"][sg, i] != 255:
            np.testing.assert_array_equal(out["blocks"][bo + i * b:bo + (i + 1) * b],
                                          o["blocks"][co + i * b:co + (i + 1) * b], tag)
    ro, so = int(r["rec_off"][g]), int(c["rec_off"][sg])
    np.testing.assert_array_equal(out["rec"][ro:ro + rm * b], o["rec"][so:so + rm * b], tag)
    for j in range(rmax):
        q = g * rmax + j
        if j >= rm:
            assert out["rev_len"][q] == -1 and (out["rev"][q] == FILL).all(), tag
            assert out["rev_pn"][q] == FILL, tag
            continue
        p = sg * rm + j
        np.testing.assert_array_equal(out["rev_len"][q], o["rev_len"][p], tag)
        np.testing.assert_array_equal(out["rev_pn"][q], o["rev_pn"][p], tag)
        np.testing.assert_array_equal(out["rev"][q], o["rev"][p], tag)
    if "revived" not in skip and sg in c["revived"] and o["status"][sg] == 0:
        got = {int(out["rec_rows"][g, j]): out["rev"][g * rmax + j, :out["rev_len"][g * rmax + j]].tobytes()
               for j in range(rm) if out["rec_rows"][g, j] != 255}
        assert got == {x: pay for x, (pay, _) in c["revived"][sg].items()}, tag


def check_nothing_written_rx(r, out, g, rmax=RMAX):
    """A rejected group: status -2, rec_rows 255, and nothing else of it written."""
    assert out["status"][g] == -2
    assert (out["rec_rows"][g] == 255).all() and (out["rows"][g] == ROW_FILL).all()
    q = slice(g * rmax, (g + 1) * rmax)
    assert (out["rev_len"][q] == -1).all() and (out["rev"][q] == FILL).all()


def check_rx(r, out, ref, skip_groups=(), rmax=RMAX):
    from tests.test_mixed_wire_abi import accept_mixed
    for g, og in enumerate(r["order"]):
        if g in skip_groups:
            continue
        if og is None:
            check_nothing_written_rx(r, out, g, rmax)
        else:
            check_group_rx(r, out, ref, g, og, rmax)
    if "arr_state" in out and not skip_groups:
        for a, s in enumerate(r["src"]):
            exp = -2 if s is None else ref[s[0]]["arr_state"][s[1]]
            assert out["arr_state"][a] == exp, (a, s)
        km = [(-1, -1) if og is None else SHAPES[og[0]] for og in r["order"]]
        _, states = accept_mixed(km, r["arr"])
        np.testing.assert_array_equal(out["arr_state"], np.array(states, np.int32))
    # a slot below npkt that no group the call runs owns (a rejected group's clipped span, a gap,
    # the capacity past the table's total): arr_at -1 and open_len -1; the others: never the
    # init pass's INT32_MAX
    npkt = out["arr_at"].shape[0]
    owned = np.zeros(npkt, bool)
    for g, og in enumerate(r["order"]):
        if og is not None and g not in skip_groups:
            f = int(r["pkt_first"][g])
            owned[f:f + sum(SHAPES[og[0]])] = True
    assert out["open_len"].shape[0] == npkt
    assert (out["arr_at"][~owned] == -1).all() and (out["open_len"][~owned] == -1).all()
    assert (out["arr_at"] < (r["n"] if "arr_state" in out else 1 << 30)).all()
    assert (out["open_len"] < 1 << 14).all() and (out["open_len"] >= -1).all()
    # every byte of blocks and rec outside the groups' own areas keeps the fill
    used = np.zeros(r["blocks_bytes"], bool)
    for g, og in enumerate(r["order"]):
        if og is not None:
            o = int(r["blocks_off"][g])
            used[o:o + SHAPES[og[0]][0] * int(r["bb"][g])] = True
    assert (out["blocks"][~used] == FILL).all()


@pytest.fixture(scope="module")
def codeset(engine):
    cs = engine.codeset(CODES)
    yield cs
    cs.close()


# ---------------------------------------------------------------- receiver tests
def test_arrivals_mixed_vs_ragged_per_code(engine, oracle, codeset):
    """Every output of the mixed call equals the ragged call of the group's own code, group by
    group and arrival by arrival; arr_state equals accept_mixed(); revived payloads equal
    ref_framing.revive's; the group without a code has status -2 and nothing written."""
    r = build_rx(oracle)
    out = run_rx(engine, codeset, r)
    assert out["kernels"].split(" + ")[:7] == KERNELS_RX, out["kernels"]
    assert out["kernels"].endswith("open_status_kernel<mixed> + extract_revived_kernel<mixed>")
    check_rx(r, out, ref_rx(engine, r))
    g = r["nocode"][0]
    tagged = np.flatnonzero(r["grp"] == g)
    assert tagged.size == 8 and (out["arr_state"][tagged] == -2).all()


def test_arrivals_mixed_second_order(engine, oracle, codeset):
    """Another shuffle of the groups and another merge of the arrivals."""
    r = build_rx(oracle, 1)
    assert not np.array_equal(r["code"], build_rx(oracle)["code"])
    check_rx(r, run_rx(engine, codeset, r), ref_rx(engine, r))


def test_arrivals_mixed_optimistic_off_and_no_state(oracle):
    """arr_optimistic = 0 gives the same outputs (no pre-pass); so does a call without arr_state
    (no state pass)."""
    from quic_amd.fec import FecEngine
    r = build_rx(oracle)
    eng = FecEngine(0)
    cs = eng.codeset(CODES)
    try:
        ref = ref_rx(eng, r)
        on = run_rx(eng, cs, r)
        none = run_rx(eng, cs, r, with_state=False)
        assert "arrivals_state_kernel<mixed>" not in none["kernels"]
        check_rx(r, none, ref)
        eng.set_option("arr_optimistic", 0)
        off = run_rx(eng, cs, r)
        assert "arrivals_pre_kernel<mixed>" not in off["kernels"]
        check_rx(r, off, ref)
        for name in ("arr_state", "arr_at", "open_len", "rows", "rec", "rec_rows", "status", "rev",
                     "rev_len", "rev_pn"):
            np.testing.assert_array_equal(on[name], off[name], name)
    finally:
        cs.close()
        eng.close()


def test_arrivals_mixed_nothing_arrived(engine, oracle, codeset):
    """n = 0: every group with a code has status -3, every slot -1."""
    r = build_rx(oracle)
    out = run_rx(engine, codeset, r, n=0)
    for g, og in enumerate(r["order"]):
        assert out["status"][g] == (-2 if og is None else -3)
    assert (out["arr_at"] == -1).all() and (out["open_len"] == -1).all()
    assert (out["rec_rows"] == 255).all() and (out["rev_len"] == -1).all()
    # (rec is not looked at: the m = 1 decode XORs a group's slots before open_status calls the
    # group malformed, in the ragged call too)
    assert (out["rev"] == FILL).all()


@pytest.mark.parametrize("k,m", [(32, 4), (10, 1)])
def test_arrivals_mixed_one_code_equals_ragged(engine, oracle, k, m):
    """A set of one code on the ragged call's own input: byte-identical outputs."""
    c = A.build_arrivals(oracle, k, m)
    ref = A.run_arrivals(engine, c)
    r = build_rx(oracle, 0, ((k, m),))
    cs = engine.codeset([(k, m)])
    try:
        code = np.zeros(c["G"], np.uint8)
        r1 = dict(r, code=code, grp=c["grp"], blocks_off=c["blocks_off"],
                  blocks_bytes=c["blocks_bytes"], rec_off=c["rec_off"], rec_bytes=c["rec_bytes"])
        from quic_amd import fec
        r1["pkt_first"], _ = fec.mixed_packet_layout([(k, m)], code)
        np.testing.assert_array_equal(r1["wire"][:, :c["pkt_stride"]], c["wire"])
        out = run_rx(engine, cs, r1, rmax=min(k, m), kmax=k)
        for name in ("arr_state", "arr_at", "open_len", "rows", "rec", "rec_rows", "status", "rev",
                     "rev_len", "rev_pn"):
            np.testing.assert_array_equal(out[name], ref[name], name)
        # blocks: the placed slots (a slot whose row is 255 is unspecified in both calls)
        for g in range(c["G"]):
            o, b = int(c["blocks_off"][g]), int(c["bb"][g])
            for i in np.flatnonzero(ref["rows"][g] != 255):
                np.testing.assert_array_equal(out["blocks"][o + i * b:o + (i + 1) * b],
                                              ref["blocks"][o + i * b:o + (i + 1) * b])
        assert (ref["rows"] != 255).any()
    finally:
        cs.close()


def hostile(r, what):
    """(pkt_first, npkt, the groups the table names as rejected): r's table made hostile."""
    first = r["pkt_first"].copy()
    g = next(x for x in range(20, r["G"]) if r["order"][x] is not None and
             r["order"][x + 1] is not None and r["order"][x - 1] is not None)
    if what == "short":          # group g's span one too short: g + 1 starts one early, so its
        first[g + 1] -= 1        # own span is one too long
        return first, r["npkt"], [g, g + 1]
    if what == "past":           # the last groups' spans reach past npkt
        npkt = r["npkt"] - 3
        return first, npkt, [x for x in range(r["G"]) if r["order"][x] is not None and
                             first[x + 1] > npkt]
    first[g + 1] = first[g] - 5  # one descending entry
    return first, r["npkt"], [g, g + 1]


@pytest.mark.parametrize("optimistic", [1, 0])
@pytest.mark.parametrize("what", ["short", "past", "descending"])
def test_arrivals_mixed_hostile_tables(engine, oracle, codeset, what, optimistic):
    """A malformed pkt_first, under both forms of the data write: the groups it names get -2 and
    nothing written but arr_at -1 and open_len -1 over their spans clipped to npkt (check_rx),
    every other group its exact result, and no byte outside the guarded buffers is touched."""
    r = build_rx(oracle)
    first, npkt, bad = hostile(r, what)
    assert bad and len(bad) < 8
    engine.set_option("arr_optimistic", optimistic)
    try:
        out = run_rx(engine, codeset, r, pkt_first=first, npkt=npkt)
    finally:
        engine.set_option("arr_optimistic", 1)
    assert ("arrivals_pre_kernel<mixed>" in out["kernels"]) == bool(optimistic)
    for g in bad:                       # some slot of each rejected span lies below npkt
        assert max(int(first[g]), 0) < npkt
    for g in bad:
        check_nothing_written_rx(r, out, g)
        o = int(r["blocks_off"][g])
        k = SHAPES[r["order"][g][0]][0]
        assert (out["blocks"][o:o + k * int(r["bb"][g])] == FILL).all()
    tagged = np.isin(r["grp"], bad)
    assert (out["arr_state"][tagged] == -2).all()
    check_rx(dict(r, pkt_first=first), out, ref_rx(engine, r), skip_groups=set(bad))
    ok = ~tagged
    ref = ref_rx(engine, r)
    exp = np.array([-2 if s is None else ref[s[0]]["arr_state"][s[1]] for s in r["src"]])
    np.testing.assert_array_equal(out["arr_state"][ok], exp[ok])


@pytest.mark.parametrize("optimistic", [1, 0])
def test_arrivals_mixed_capacity_above_total(engine, oracle, codeset, optimistic):
    """npkt is a capacity: 100 slots past the table's total, and the codeless group given a span
    of its own in the middle (a gap no group owns).  Those slots get arr_at -1 and open_len -1 in
    both forms of the data write; every group keeps its exact result."""
    r = build_rx(oracle)
    g0 = r["nocode"][0]
    first = r["pkt_first"].copy()
    first[g0 + 1:] += 7                                       # slots first[g0] .. + 6 belong to nobody
    engine.set_option("arr_optimistic", optimistic)
    try:
        out = run_rx(engine, codeset, r, pkt_first=first, npkt=int(first[-1]) + 100)
    finally:
        engine.set_option("arr_optimistic", 1)
    assert out["arr_at"].shape[0] == r["npkt"] + 107
    check_rx(dict(r, pkt_first=first), out, ref_rx(engine, r))
    gap = slice(int(first[g0]), int(first[g0]) + 7)
    assert (out["arr_at"][gap] == -1).all() and (out["open_len"][gap] == -1).all()
    assert (out["arr_at"][-100:] == -1).all() and (out["open_len"][-100:] == -1).all()


def test_arrivals_mixed_no_groups(engine, oracle, codeset):
    """groups = 0 with a ring and a capacity, through the C entry point (an empty tensor has no
    address to pass): every arrival ignored, every slot -1, nothing else written."""
    import ctypes
    import torch
    r = build_rx(oracle)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")    # noqa: E731
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    n, npkt = 70, 150
    wire, hw = guarded_from(r["wire"][:n], offset=1)
    at, ol, state = (torch.full((x,), 7, dtype=i32, device="cuda") for x in (npkt, npkt, n))
    one = dict(code=z(1, u8), bb=z(1, i32), first=z(1, i32), off=z(1, i64), rows=z(KMAX, u8),
               rr=z(RMAX, u8), rev=z(64, u8), rl=z(1, i32), buf=z(64, u8),
               wlen=dev(r["wire_len"][:n]), ad=dev(r["hdr_len"][:n]), grp=dev(r["grp"][:n]),
               idx=dev(r["idx"][:n]))
    p = lambda t: ctypes.c_void_p(t.data_ptr())                           # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = engine.lib.qfec_open_decode_extract_arrivals_mixed(
        engine._h, codeset._h, 0, p(one["code"]), p(one["bb"]), p(one["first"]), npkt, n, p(wire),
        wire.stride(0), p(one["wlen"]), p(one["ad"]), 0, None, 1, p(one["grp"]), p(one["idx"]),
        p(state), p(at), p(one["buf"]), p(one["off"]), p(one["rows"]), p(ol), p(one["buf"]),
        p(one["off"]), p(one["rr"]), None, p(one["rev"]), 64, p(one["rl"]), None, stream)
    assert rc == 0
    assert (host(at) == -1).all() and (host(ol) == -1).all() and (host(state) == -2).all()
    for name in ("rows", "rr", "rev", "rl", "buf"):
        assert (host(one[name]) == 0).all(), name
    hw.check_guards()


def test_mixed_wire_call_limits(engine, oracle, codeset):
    """Call-level -2, before anything is enqueued: a set with a code of k + m > 255, a set of
    another context, a NULL array, a misaligned base, a bad stride."""
    import torch
    from quic_amd.fec import FecEngine, FecError
    r, s = build_rx(oracle), build_tx(oracle)
    G = r["G"]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")    # noqa: E731
    u8, i32 = torch.uint8, torch.int32

    def rx(eng=engine, cs=codeset, **kw):
        a = dict(code=dev(r["code"]), bb=dev(r["bb"]), first=dev(r["pkt_first"]),
                 boff=dev(r["blocks_off"]), roff=dev(r["rec_off"]), blocks=z(r["blocks_bytes"], u8),
                 rec=z(r["rec_bytes"], u8), grp=dev(r["grp"][:64]), rows=z((G, cs.kmax), u8))
        a.update(kw)
        eng.open_decode_extract_arrivals_mixed(
            cs, a["code"], a["bb"], a["first"], dev(r["wire"][:64]), dev(r["wire_len"][:64]), 16, 1,
            a["grp"], dev(r["idx"][:64]), None, z(r["npkt"], i32), a["blocks"], a["boff"], a["rows"],
            z(r["npkt"], i32), a["rec"], a["roff"], z((G, cs.rmax), u8), z((G * cs.rmax, 64), u8),
            z(G * cs.rmax, i32))

    def tx(eng=engine, cs=codeset, **kw):
        a = dict(code=dev(s["code"]), bb=dev(s["bb"]), first=dev(s["pkt_first"]),
                 pfirst=dev(s["pay_first"]), doff=dev(s["data_off"]), poff=dev(s["par_off"]),
                 data=z(s["data_bytes"], u8), par=z(s["par_bytes"], u8),
                 pkt=z((s["npkt"], s["pkt_stride"]), u8))
        a.update(kw)
        eng.frame_encode_seal_mixed(
            cs, a["code"], a["bb"], a["first"], a["pfirst"], a["data"], a["doff"], a["par"],
            a["poff"], dev(s["hdr"]), dev(s["hdr_len"]), dev(s["pay"]), dev(s["pay_len"]), 1,
            a["pkt"], z(s["npkt"], i32))

    def refused(call, **kw):
        with pytest.raises(FecError) as e:
            call(**kw)
        assert e.value.rc == -2, kw

    rx()
    tx()
    big = engine.codeset(CODES[:8] + [(250, 6)])
    other = FecEngine(0)
    try:
        refused(rx, cs=big)
        refused(tx, cs=big)
        refused(rx, eng=other)
        refused(tx, eng=other)
        for name in ("bb", "first", "boff", "roff", "rows", "grp"):   # (code sizes the call)
            refused(rx, **{name: None})
        for name in ("bb", "first", "pfirst", "doff", "poff"):
            refused(tx, **{name: None})
        refused(rx, blocks=z(r["blocks_bytes"] + 1, u8)[1:])
        refused(tx, par=z(s["par_bytes"] + 1, u8)[1:])
        refused(tx, pkt=z((s["npkt"], s["pkt_stride"] + 1), u8))        # a stride that is not 4-aligned
    finally:
        big.close()
        other.close()


def test_arrivals_mixed_graph_replay_rewritten(oracle):
    """One linear stream capture after qfec_codeset_reserve, replayed after code, bb, pkt_first,
    the offsets and the ring were rewritten in place to a batch with another code order."""
    import torch
    from quic_amd.fec import FecEngine
    a, b = build_rx(oracle, 0), build_rx(oracle, 1)
    assert a["G"] == b["G"] and a["n"] == b["n"] and a["npkt"] == b["npkt"]
    G, n, npkt = a["G"], a["n"], a["npkt"]
    eng = FecEngine(0)
    cs = eng.codeset(CODES)
    try:
        ref = ref_rx(eng, a)
        cs.reserve(G)
        size = {x: max(a[x], b[x]) for x in ("blocks_bytes", "rec_bytes")}
        names = ("code", "bb", "pkt_first", "blocks_off", "rec_off", "wire", "wire_len", "hdr_len",
                 "pn", "grp", "idx")
        d = {x: dev(a[x]) for x in names}
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")    # noqa: E731
        t = dict(blocks=full((size["blocks_bytes"],), FILL, torch.uint8),
                 rec=full((size["rec_bytes"],), FILL, torch.uint8),
                 rev=full((G * RMAX, a["rev_stride"]), FILL, torch.uint8),
                 rows=full((G, KMAX), ROW_FILL, torch.uint8), open_len=full((npkt,), 7, torch.int32),
                 arr_at=full((npkt,), 7, torch.int32), arr_state=full((n,), 7, torch.int32),
                 rec_rows=full((G, RMAX), ROW_FILL, torch.uint8), status=full((G,), 7, torch.int32),
                 rev_len=full((G * RMAX,), 7, torch.int32), rev_pn=full((G * RMAX,), FILL, torch.uint8))
        fills = {x: int(v.reshape(-1)[0]) for x, v in t.items()}
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            eng.open_decode_extract_arrivals_mixed(
                cs, d["code"], d["bb"], d["pkt_first"], d["wire"], d["wire_len"], d["hdr_len"],
                d["pn"], d["grp"], d["idx"], t["arr_state"], t["arr_at"], t["blocks"],
                d["blocks_off"], t["rows"], t["open_len"], t["rec"], d["rec_off"], t["rec_rows"],
                t["rev"], t["rev_len"], rev_pn_len=t["rev_pn"], status=t["status"],
                stream=s.cuda_stream)
        torch.cuda.synchronize()
        for c in (a, b):
            for x in names:
                d[x].copy_(torch.from_numpy(np.ascontiguousarray(c[x])))
            for x, v in t.items():
                v.fill_(fills[x])
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                gr.replay()
            out = {x: host(v) for x, v in t.items()}
            out["blocks"] = out["blocks"][:c["blocks_bytes"]]
            check_rx(c, out, ref)
    finally:
        cs.close()
        eng.close()


# ---------------------------------------------------------------- sender case
_TX = {}


def build_tx(O, seed=0, shapes=None):
    """The mixed sender batch: the per-shape sender cases' groups interleaved (cached)."""
    from quic_amd import fec
    key = (seed, shapes)
    if key in _TX:
        return _TX[key]
    use = list(range(len(SHAPES))) if shapes is None else [SHAPES.index(s) for s in shapes]
    cases = {ci: A.sender(O, *SHAPES[ci]) for ci in use}
    order = group_order([cases[ci]["G"] if ci in cases else 0 for ci in range(len(SHAPES))], seed) \
        if shapes is None else [(ci, g) for ci in use for g in range(cases[ci]["G"])]
    G = len(order)
    code = np.array([NOCODE if og is None else code_index(*og) for og in order], np.uint8)
    bb = np.array([1352 if og is None else cases[og[0]]["bb"][og[1]] for og in order], np.int32)
    pkt_first, pay_first = fec.mixed_packet_layout(CODES, code)
    npkt, npay = int(pkt_first[-1]), int(pay_first[-1])
    rng = np.random.default_rng(57 + seed)
    data_off, data_bytes = layout(order, bb, lambda k, m: k, rng)
    par_off, par_bytes = layout(order, bb, lambda k, m: m, rng)
    pstride = max(c["pay_stride"] for c in cases.values())
    kstride = max(c["pkt_stride"] for c in cases.values())
    pay = np.zeros((npay, pstride), np.uint8)
    pay_len, pn = np.zeros(npay, np.int32), np.ones(npay, np.uint8)
    hdr, hdr_len = np.zeros((npkt, T.HMAX), np.uint8), np.zeros(npkt, np.int32)
    for g, og in enumerate(order):
        if og is None:
            continue
        (ci, sg), c = og, cases[og[0]]
        k, m = SHAPES[ci]
        q, p = int(pay_first[g]), int(pkt_first[g])
        pay[q:q + k, :c["pay_stride"]] = c["pay"][sg * k:(sg + 1) * k]
        pay_len[q:q + k], pn[q:q + k] = c["pay_len"][sg * k:(sg + 1) * k], c["pn"][sg * k:(sg + 1) * k]
        per = k + m
        hdr[p:p + per], hdr_len[p:p + per] = c["hdr"][sg * per:(sg + 1) * per], c["hdr_len"][sg * per:(sg + 1) * per]
    s = dict(seed=seed, cases=cases, use=use, order=order, G=G, code=code, bb=bb, pkt_first=pkt_first,
             pay_first=pay_first, npkt=npkt, npay=npay, data_off=data_off, data_bytes=data_bytes,
             par_off=par_off, par_bytes=par_bytes, pay=pay, pay_len=pay_len, pn=pn, hdr=hdr,
             hdr_len=hdr_len, pay_stride=pstride, pkt_stride=kstride,
             nocode=[g for g, og in enumerate(order) if og is None])
    _TX[key] = s
    return s


def run_tx(engine, cs, s, bb=None, pay_len=None, pn=None, pay_first=None, npay=None,
           pkt_first=None):
    import torch
    from quic_amd import fec
    data, hd = guarded((s["data_bytes"],))
    par, hp = guarded((s["par_bytes"],))
    pkt, hk = guarded((s["npkt"], s["pkt_stride"]))
    payv, hy = guarded_from(s["pay"][:s["npay"] if npay is None else npay], offset=3)
    plen = torch.full((s["npkt"],), 7, dtype=torch.int32, device="cuda")
    st = torch.full((s["G"],), 7, dtype=torch.int32, device="cuda")
    npay = payv.shape[0]
    engine.frame_encode_seal_mixed(
        cs, dev(s["code"]), dev(s["bb"] if bb is None else bb),
        dev(s["pkt_first"] if pkt_first is None else pkt_first),
        dev(s["pay_first"] if pay_first is None else pay_first), data, dev(s["data_off"]), par,
        dev(s["par_off"]), dev(s["hdr"]), dev(s["hdr_len"]), payv,
        dev((s["pay_len"] if pay_len is None else pay_len)[:npay]),
        dev(s["pn"][:npay]) if pn is None else pn, pkt, plen, status=st)
    out = dict(kernels=fec.last_kernels(), data=host(data), par=host(par), pkt=host(pkt),
               plen=host(plen), status=host(st))
    for h in (hd, hp, hk, hy):
        h.check_guards()
    return out


def ref_tx(engine, s, bb=None, pay_len=None):
    """The parent's route: the ragged framed sender once per code; bb / pay_len: the mixed batch's
    overrides, carried back to each case's own order."""
    ref = {}
    for ci in s["use"]:
        c = s["cases"][ci]
        k = SHAPES[ci][0]
        cb, cl = c["bb"].copy(), c["pay_len"].copy()
        for g, og in enumerate(s["order"]):
            if og is not None and og[0] == ci:
                if bb is not None:
                    cb[og[1]] = bb[g]
                if pay_len is not None:
                    q = int(s["pay_first"][g])
                    cl[og[1] * k:(og[1] + 1) * k] = pay_len[q:q + k]
        ref[ci] = T.run_send(engine, c, bb=cb, pay_len=cl)
    return ref


def check_tx(s, out, ref, skip_groups=()):
    covered = np.zeros(s["npkt"], bool)
    for g, og in enumerate(s["order"]):
        if g in skip_groups:
            continue
        if og is None:
            assert out["status"][g] == -2
            continue
        (ci, sg), c, o = og, s["cases"][og[0]], ref[og[0]]
        k, m = SHAPES[ci]
        per, b = k + m, int(c["bb"][sg])
        tag = f"group {g} = shape {SHAPES[ci]} group {sg}"
        np.testing.assert_array_equal(out["status"][g], o["status"][sg], tag)
        do, co = int(s["data_off"][g]), int(c["data_off"][sg])
        np.testing.assert_array_equal(out["data"][do:do + k * b], o["data"][co:co + k * b], tag)
        po, qo = int(s["par_off"][g]), int(c["par_off"][sg])
        np.testing.assert_array_equal(out["par"][po:po + m * b], o["par"][qo:qo + m * b], tag)
        p = int(s["pkt_first"][g])
        covered[p:p + per] = True
        np.testing.assert_array_equal(out["plen"][p:p + per], o["plen"][sg * per:(sg + 1) * per], tag)
        w = c["pkt_stride"]
        np.testing.assert_array_equal(out["pkt"][p:p + per, :w], o["pkt"][sg * per:(sg + 1) * per], tag)
        assert (out["pkt"][p:p + per, w:] == FILL).all(), tag
    if not skip_groups:
        assert (out["plen"][~covered] == -1).all() and (out["pkt"][~covered] == FILL).all()


# ---------------------------------------------------------------- sender tests
def test_frame_seal_mixed_vs_ragged_per_code(engine, oracle, codeset):
    """Blocks, parity, wire packets, pkt_len and status group by group against the ragged sender
    run per code; the FEC packets of two groups per code against the oracle directly."""
    s = build_tx(oracle)
    out = run_tx(engine, codeset, s)
    names = out["kernels"].split(" + ")
    assert names[:2] == KERNELS_TX[:2] and names[-1] == KERNELS_TX[2], out["kernels"]
    assert "xor_copy_mixed_kernel<encode>" in names and "gf_mixed_kernel<encode>" in names
    check_tx(s, out, ref_tx(engine, s))
    seen = {}
    for g, og in enumerate(s["order"]):
        if og is None or seen.get(og[0], 0) >= 2:
            continue
        seen[og[0]] = seen.get(og[0], 0) + 1
        (ci, sg), c = og, s["cases"][og[0]]
        k, m = SHAPES[ci]
        p, per = int(s["pkt_first"][g]), k + m
        np.testing.assert_array_equal(out["plen"][p:p + per], c["plen"][sg * per:(sg + 1) * per])
        for i in range(per):
            ln = int(out["plen"][p + i])
            np.testing.assert_array_equal(out["pkt"][p + i, :ln], c["pkt"][sg * per + i, :ln])
    assert len(seen) == len(SHAPES)


def test_frame_seal_mixed_rejections(engine, oracle, codeset):
    """A bad length (-3), bb = 0 (-3, in a tile beside other groups) and a framed bb that is no
    multiple of 8 (-1): exactly the ragged sender's results, with exact neighbours."""
    s = build_tx(oracle)
    bb, pl = s["bb"].copy(), s["pay_len"].copy()
    gf = [g for g, og in enumerate(s["order"]) if og is not None and min(SHAPES[og[0]]) > 1]
    g_len = gf[3]
    # a size that is no multiple of 8 and still holds every payload of the group behind its prefix
    slack = lambda g: int(s["bb"][g]) - 2 - int(                                  # noqa: E731
        s["pay_len"][int(s["pay_first"][g]):int(s["pay_first"][g + 1])].max())
    g_odd = next(g for g in gf[30:] if slack(g) >= 4 and s["bb"][g] >= 16)
    # bb = 0 in a tile beside other groups: its first packet shares a tile with its predecessor's
    g_bb0 = next(g for g in gf[10:] if g != g_odd and s["order"][g - 1] is not None and
                 int(s["pkt_first"][g]) // 64 == int(s["pkt_first"][g - 1]) // 64)
    pl[int(s["pay_first"][g_len]) + 1] = 0x4000
    bb[g_bb0] = 0
    bb[g_odd] -= 4
    out = run_tx(engine, codeset, s, bb=bb, pay_len=pl)
    assert out["status"][g_len] == -3 and out["status"][g_bb0] == -3 and out["status"][g_odd] == -1
    for g in (g_len, g_bb0, g_odd):
        k, m = SHAPES[s["order"][g][0]]
        p = int(s["pkt_first"][g])
        assert (out["plen"][p:p + k + m] == -1).all()
    check_tx(s, out, ref_tx(engine, s, bb=bb, pay_len=pl))


def test_frame_seal_mixed_pn_once_for_all(engine, oracle, codeset):
    """pn_len as one value for every packet equals the array that holds it everywhere."""
    import torch
    s = build_tx(oracle)
    one = run_tx(engine, codeset, s, pn=2)
    arr = run_tx(engine, codeset, s, pn=torch.full((s["npay"],), 2, dtype=torch.uint8, device="cuda"))
    for name in ("data", "par", "pkt", "plen", "status"):
        np.testing.assert_array_equal(one[name], arr[name], name)
    per_packet = run_tx(engine, codeset, s)
    assert not np.array_equal(one["data"], per_packet["data"])


def test_frame_seal_mixed_hostile_pay_first(engine, oracle, codeset):
    """A pay_first span one too short, and one that reaches past npay: those groups get -2, none of
    their packets is sealed, nothing of them is written; the neighbours are exact."""
    s = build_tx(oracle)
    g = next(x for x in range(20, s["G"] - 1) if s["order"][x] is not None and
             s["order"][x + 1] is not None)
    first = s["pay_first"].copy()
    first[g + 1] -= 1
    last = [x for x in range(s["G"]) if s["order"][x] is not None and s["pay_first"][x + 1] > s["npay"] - 2]
    out = run_tx(engine, codeset, s, pay_first=first, npay=s["npay"] - 2)
    bad = [g, g + 1] + last
    for x in bad:
        k, m = SHAPES[s["order"][x][0]]
        p, do, po, b = int(s["pkt_first"][x]), int(s["data_off"][x]), int(s["par_off"][x]), int(s["bb"][x])
        assert out["status"][x] == -2
        assert (out["plen"][p:p + k + m] == -1).all() and (out["pkt"][p:p + k + m] == FILL).all()
        assert (out["data"][do:do + k * b] == FILL).all() and (out["par"][po:po + m * b] == FILL).all()
    check_tx(s, out, ref_tx(engine, s), skip_groups=set(bad))


@pytest.mark.parametrize("what", ["short", "descending"])
def test_frame_seal_mixed_hostile_pkt_first(engine, oracle, codeset, what):
    """A malformed pkt_first on the sender.  The two groups around the break get -2 and nothing
    of them is written or sealed.  A span one too short leaves every other group exact.  A
    descending entry makes the seal's search of the tiles around it land on the rejected group, so
    packets of valid groups within a tile of the break may come out unsealed (pkt_len -1, the
    header's rule for a table that is not ascending); every group farther away is exact, and no
    byte outside the guarded buffers is touched."""
    s = build_tx(oracle)
    g = next(x for x in range(20, s["G"] - 1) if s["order"][x] is not None and
             s["order"][x + 1] is not None)
    first = s["pkt_first"].copy()
    near = set()
    if what == "short":
        first[g + 1] -= 1
    else:
        first[g + 1] = first[g] - 5
        lo, hi = (int(first[g]) - 5) // 64 * 64 - 64, (int(s["pkt_first"][g + 2]) + 63) // 64 * 64 + 64
        near = {x for x in range(s["G"]) if s["order"][x] is not None and
                s["pkt_first"][x + 1] > lo and s["pkt_first"][x] < hi}
    out = run_tx(engine, codeset, s, pkt_first=first)
    for x in (g, g + 1):
        k, m = SHAPES[s["order"][x][0]]
        do, po, b = int(s["data_off"][x]), int(s["par_off"][x]), int(s["bb"][x])
        assert out["status"][x] == -2
        assert (out["data"][do:do + k * b] == FILL).all() and (out["par"][po:po + m * b] == FILL).all()
    p0, p1 = int(s["pkt_first"][g]), int(s["pkt_first"][g + 2])
    assert (out["plen"][p0:p1] == -1).all() and (out["pkt"][p0:p1] == FILL).all()
    ref = ref_tx(engine, s)
    check_tx(s, out, ref, skip_groups={g, g + 1} | near)
    assert len(near) < 40
    for x in near - {g, g + 1}:                      # sealed exactly, or not at all
        (ci, sg), c = s["order"][x], s["cases"][s["order"][x][0]]
        per, p = sum(SHAPES[ci]), int(s["pkt_first"][x])
        assert out["status"][x] == ref[ci]["status"][sg]
        for i in range(per):
            if out["plen"][p + i] == -1:
                assert (out["pkt"][p + i] == FILL).all()
            else:
                assert out["plen"][p + i] == ref[ci]["plen"][sg * per + i]
                np.testing.assert_array_equal(out["pkt"][p + i, :c["pkt_stride"]],
                                              ref[ci]["pkt"][sg * per + i])


@pytest.mark.parametrize("k,m", [(32, 4), (10, 1), (5, 5)])
def test_frame_seal_mixed_one_code_equals_ragged(engine, oracle, k, m):
    """A set of one code on the ragged sender's own input: byte-identical outputs ((5, 5) passes
    one pn_len for every packet)."""
    import torch
    from quic_amd import fec
    c = A.sender(oracle, k, m)
    ref = T.run_send(engine, c)
    cs = engine.codeset([(k, m)])
    try:
        code = np.zeros(c["G"], np.uint8)
        pkt_first, pay_first = fec.mixed_packet_layout([(k, m)], code)
        data, hd = guarded((c["data_bytes"],))
        par, hp = guarded((c["par_bytes"],))
        pkt, hk = guarded((c["n"], c["pkt_stride"]))
        payv, hy = guarded_from(c["pay"], offset=3)
        plen = torch.full((c["n"],), 7, dtype=torch.int32, device="cuda")
        st = torch.full((c["G"],), 7, dtype=torch.int32, device="cuda")
        engine.frame_encode_seal_mixed(
            cs, dev(code), dev(c["bb"]), dev(pkt_first), dev(pay_first), data, dev(c["data_off"]),
            par, dev(c["par_off"]), dev(c["hdr"]), dev(c["hdr_len"]), payv, dev(c["pay_len"]),
            T.pn_arg(c), pkt, plen, status=st)
        got = dict(data=host(data), par=host(par), pkt=host(pkt), plen=host(plen), status=host(st))
        for h in (hd, hp, hk, hy):
            h.check_guards()
        for name, v in got.items():
            np.testing.assert_array_equal(v, ref[name], name)
    finally:
        cs.close()


def test_frame_seal_mixed_graph_replay(oracle):
    """A captured sender, replayed after the batch was rewritten in place to another order."""
    import torch
    from quic_amd.fec import FecEngine
    a, b = build_tx(oracle, 0), build_tx(oracle, 1)
    assert a["G"] == b["G"] and a["npkt"] == b["npkt"] and not np.array_equal(a["code"], b["code"])
    eng = FecEngine(0)
    cs = eng.codeset(CODES)
    try:
        ref = ref_tx(eng, a)
        cs.reserve(a["G"])
        names = ("code", "bb", "pkt_first", "pay_first", "data_off", "par_off", "hdr", "hdr_len",
                 "pay", "pay_len", "pn")
        d = {x: dev(a[x]) for x in names}
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")    # noqa: E731
        t = dict(data=full((max(a["data_bytes"], b["data_bytes"]),), FILL, torch.uint8),
                 par=full((max(a["par_bytes"], b["par_bytes"]),), FILL, torch.uint8),
                 pkt=full((a["npkt"], a["pkt_stride"]), FILL, torch.uint8),
                 plen=full((a["npkt"],), 7, torch.int32), status=full((a["G"],), 7, torch.int32))
        fills = {x: int(v.reshape(-1)[0]) for x, v in t.items()}
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            eng.frame_encode_seal_mixed(
                cs, d["code"], d["bb"], d["pkt_first"], d["pay_first"], t["data"], d["data_off"],
                t["par"], d["par_off"], d["hdr"], d["hdr_len"], d["pay"], d["pay_len"], d["pn"],
                t["pkt"], t["plen"], status=t["status"], stream=st.cuda_stream)
        torch.cuda.synchronize()
        for c in (a, b):
            for x in names:
                d[x].copy_(torch.from_numpy(np.ascontiguousarray(c[x])))
            for x, v in t.items():
                v.fill_(fills[x])
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                gr.replay()
            check_tx(c, {x: host(v) for x, v in t.items()}, ref)
    finally:
        cs.close()
        eng.close()


def test_mixed_wire_end_to_end(engine, oracle, codeset):
    """The mixed sender's packets, shuffled, with one data packet of every group lost (two where
    the code recovers two) and as many FEC packets kept, through the mixed receiver: every lost
    payload comes back."""
    from quic_amd import fec
    s = build_tx(oracle)
    tx = run_tx(engine, codeset, s)
    rng = np.random.default_rng(5)
    keep, lost = [], {}
    for g, og in enumerate(s["order"]):
        if og is None:
            continue
        k, m = SHAPES[og[0]]
        lost[g] = sorted(int(x) for x in rng.choice(k, min(2, k, m), replace=False))
        keep += [(g, i) for i in range(k + len(lost[g])) if i not in lost[g]]
    keep = [keep[i] for i in rng.permutation(len(keep))]
    n = len(keep)
    grp = np.array([g for g, _ in keep], np.int32)
    idx = np.array([i for _, i in keep], np.uint8)
    at = s["pkt_first"][grp] + idx
    wire, wlen, ad = tx["pkt"][at], tx["plen"][at], s["hdr_len"][at]
    assert (wlen >= 0).all()
    pn = np.ones(n, np.uint8)
    for a, (g, i) in enumerate(keep):
        if i < SHAPES[s["order"][g][0]][0]:
            pn[a] = s["pn"][int(s["pay_first"][g]) + i]
    bb = fec.arrivals_rx_block_bytes_mixed(CODES, s["code"], grp, idx, wlen, ad)
    np.testing.assert_array_equal(np.delete(bb, s["nocode"]), np.delete(s["bb"], s["nocode"]))
    r = dict(G=s["G"], code=s["code"], bb=bb, pkt_first=s["pkt_first"], npkt=s["npkt"], n=n,
             wire=np.ascontiguousarray(wire), wire_len=wlen, hdr_len=ad, pn=pn, grp=grp, idx=idx,
             blocks_off=s["data_off"], blocks_bytes=s["data_bytes"], pkt_stride=s["pkt_stride"],
             rev_stride=A.REV_STRIDE)
    r["rec_off"], r["rec_bytes"] = layout(s["order"], bb, lambda k, m: min(k, m), rng)
    out = run_rx(engine, codeset, r)
    for g, xs in lost.items():
        assert out["status"][g] == 0, g
        assert [int(x) for x in out["rec_rows"][g, :len(xs)]] == xs
        q0 = int(s["pay_first"][g])
        for j, x in enumerate(xs):
            q = g * RMAX + j
            ln = int(s["pay_len"][q0 + x])
            assert out["rev_len"][q] == ln
            np.testing.assert_array_equal(out["rev"][q, :ln], s["pay"][q0 + x, :ln])
            assert out["rev_pn"][q] == {1: 1, 2: 2, 4: 0, 6: 2}[int(s["pn"][q0 + x])]
