"""GPU: ragged packet protection (qfec_seal_groups_batch_ragged, qfec_encode_seal_groups_
batch_ragged, qfec_open_decode_batch_ragged and the two host forms) against the oracle, group
by group: per group a ragged call does what the uniform call with block_bytes = bb[g] does.

One wave handles 64 consecutive packets, so the shapes put several groups of different size
into one tile, let groups straddle two tiles and end in a partial tile.  The case builders
(build_case, build_open_case) run on the CPU and are cached; tests/test_pp_ragged_abi.py
checks their construction without a GPU."""
import numpy as np
import pytest

from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_pp import _expected_open_decode

pytestmark = pytest.mark.gpu

HMAX = 20            # header bytes per packet, at most
# (k, m): (G, the block sizes the groups draw from)
SEAL_SHAPES = {
    (10, 1): (13, [1352, 1350, 1000, 48, 8, 3, 2056]),
    (2, 2): (40, [8, 16, 24, 1352]),
    (5, 5): (14, [1352, 1344, 520, 8]),
    (32, 4): (5, [1352, 64, 1350, 8, 1352]),        # in this order
    (10, 20): (5, [1352, 8, 1352, 264, 40]),
}
OPEN_SHAPES = dict(SEAL_SHAPES)
OPEN_SHAPES[(250, 5)] = (2, [1352, 40])             # k + m = 255, the k > 64 loops of the assemble
# host forms: enough groups for several chunks at the smallest host_chunk_mb (1 MiB)
HOST_G = {(10, 1): 84, (5, 5): 112, (32, 4): 30}


def up16(v):
    return (v + 15) & ~15


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def draw_sizes(k, m, G, pool):
    """G sizes from the pool, each at least once; shuffled unless the pool names every group."""
    bbs = [int(pool[i % len(pool)]) for i in range(G)]
    if G != len(pool):
        np.random.default_rng(100 * k + m).shuffle(bbs)
    return bbs


def packed_gaps(nblk, bbs, rng):
    """Offsets of groups of nblk blocks: multiples of 16, a gap of 16, 32 or 48 bytes after
    every group; and the buffer size."""
    off, run = [], 0
    for b in bbs:
        off.append(run)
        run = up16(run + nblk * b) + 16 * int(rng.integers(1, 4))
    return np.array(off, np.int64), run


_CASES = {}


def build_case(O, k, m, bbs):
    """One sender batch and what the oracle says about it (cached, read-only).
    data / par_given: packed buffers (par_given: the oracle's parity array of every group, the
    encode's -1 groups included: XOR row, zero rows).  par_exp: what the ragged encode leaves
    in a buffer of FILL.  pkt / plen: every packet sealed from pt_len bytes; pkt_whole /
    plen_whole: from whole blocks.  rej [G]: the groups the encode rejects (status -1)."""
    key = (k, m, tuple(bbs))
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(7919 * k + 31 * m + len(bbs))
    G, per = len(bbs), k + m
    n = G * per
    stride = (HMAX + 12 + max(bbs) + 8 + 3) // 4 * 4        # room for a plaintext of bb + 5
    c = dict(k=k, m=m, G=G, per=per, n=n, rmax=min(k, m), stride=stride,
             bb=np.array(bbs, np.int32), bbs=list(bbs))
    c["data_off"], c["data_bytes"] = packed_gaps(k, bbs, rng)
    c["par_off"], c["par_bytes"] = packed_gaps(m, bbs, rng)
    c["rec_off"], c["rec_bytes"] = packed_gaps(c["rmax"], bbs, rng)
    c["data"] = np.full(c["data_bytes"], 0x11, np.uint8)
    c["par_given"] = np.full(c["par_bytes"], FILL, np.uint8)
    c["par_exp"] = np.full(c["par_bytes"], FILL, np.uint8)
    c["hdr"] = rng.integers(0, 256, (n, HMAX), dtype=np.uint8)
    c["hdr_len"] = rng.integers(9, HMAX + 1, n).astype(np.int32)
    c["pt_len"] = np.zeros(n, np.int32)
    c["rej"] = np.zeros(G, bool)
    c["blocks"] = []                                         # per group: data [k][bb]
    for name in ("pkt", "pkt_whole"):
        c[name] = np.zeros((n, stride), np.uint8)
    c["plen"], c["plen_whole"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for g, bb in enumerate(bbs):
        p0 = g * per
        data = rng.integers(0, 256, (k, bb), dtype=np.uint8)
        ptl = np.full(per, bb, np.int32)
        ptl[:k] = rng.integers(max(0, bb - 300), bb + 1, k)
        for i in range(k):
            data[i, ptl[i]:] = 0                             # a data block is its payload, padded
        par, rc = O.encode_batch(k, m, bb, data[None])
        assert rc in (0, -1) and (rc == -1) == (m > 1 and k > 1 and bb % 8 != 0)
        c["rej"][g] = rc != 0
        do, po = int(c["data_off"][g]), int(c["par_off"][g])
        c["data"][do:do + k * bb] = data.ravel()
        c["par_given"][po:po + m * bb] = par[0].ravel()
        nwritten = m if rc == 0 else 1                       # -1: the XOR parity alone
        c["par_exp"][po:po + nwritten * bb] = par[0][:nwritten].ravel()
        c["pt_len"][p0:p0 + per] = ptl
        c["blocks"].append(data)
        rows_pt = np.concatenate([data, par[0]])
        sl = slice(p0, p0 + per)
        c["pkt"][sl], c["plen"][sl] = O.null_seal_batch(c["hdr"][sl], c["hdr_len"][sl], rows_pt,
                                                        ptl, stride)
        c["pkt_whole"][sl], c["plen_whole"][sl] = O.null_seal_batch(
            c["hdr"][sl], c["hdr_len"][sl], rows_pt, np.full(per, bb, np.int32), stride)
    assert (c["plen"] >= 0).all() and (c["plen_whole"] >= 0).all()
    _CASES[key] = c
    return c


def seal_case(O, k, m):
    G, pool = SEAL_SHAPES[(k, m)]
    return build_case(O, k, m, draw_sizes(k, m, G, pool))


def group_kinds(k, m, bbs):
    """What happens to each group's packets, by construction.  Kinds: clean (nothing lost),
    loss1 (one data packet lost), nofec (a data packet and every FEC packet lost), tagfail (a
    data packet lost and the first FEC packet tampered), toolong (a data packet whose
    plaintext is longer than bb), mod8 (m > 1, bb % 8 != 0, one data packet lost).  A batch
    of fewer than four groups ((250, 5)) combines kinds in one group, and has no group without
    a loss.  mod8 exists only where the sizes hold one that is no multiple of 8 ((32, 4)'s
    1350); such a group gets no other kind with m > 1, since any loss there ends in -1."""
    G = len(bbs)
    if G < 4:
        return [{"tagfail", "toolong"}, {"nofec"}][:G]
    gf = m > 1 and k > 1
    kinds = [set() for _ in bbs]
    odd = [g for g in range(G) if gf and bbs[g] % 8]
    for j, g in enumerate(odd):
        kinds[g] = {"mod8"} if j == 0 else {"clean"}
    order = ["clean", "nofec", "tagfail", "toolong", "loss1"]
    free = [g for g in range(G) if not kinds[g]]
    for i, g in enumerate(free):
        kinds[g] = {order[i % len(order)]}
    return kinds


def required_kinds(k, m, bbs):
    need = {"nofec", "tagfail", "toolong"}
    if len(bbs) >= 4:
        need.add("clean")
    if m > 1 and k > 1 and any(b % 8 for b in bbs):
        need.add("mod8")
    return need


_OPEN = {}


def build_open_case(O, k, m, bbs):
    """A receiver batch built from build_case's wire packets, and the oracle's open -> decode
    of every group (tests/test_gpu_pp.py's _expected_open_decode with G = 1 and that group's
    bb).  The constructed properties are asserted here, on the CPU."""
    key = (k, m, tuple(bbs))
    if key in _OPEN:
        return _OPEN[key]
    s = build_case(O, k, m, bbs)
    rng = np.random.default_rng(104729 * k + 17 * m + len(bbs))
    G, per, n, rmax, stride = s["G"], s["per"], s["n"], s["rmax"], s["stride"]
    c = dict(s)
    pkt, pkt_len = s["pkt"].copy(), s["plen"].copy()
    kinds = group_kinds(k, m, bbs)
    assert set().union(*kinds) >= required_kinds(k, m, bbs)
    lost, tampered, toolong = {}, {}, {}
    for g, bb in enumerate(bbs):
        p0, ks = g * per, kinds[g]
        if ks & {"loss1", "mod8", "nofec", "tagfail"}:
            x = int(rng.integers(k))
            lost[g] = x
            pkt_len[p0 + x] = -1
        if "nofec" in ks:
            pkt_len[p0 + k:p0 + per] = -1
        if "tagfail" in ks:
            p = p0 + k                                       # the first FEC packet, by length
            pkt[p, s["hdr_len"][p] + 12 + int(rng.integers(bb))] ^= 0x40
            tampered[g] = p
        if "toolong" in ks:
            y = int(rng.choice([i for i in range(k) if i != lost.get(g)]))
            p = p0 + y
            long_pt = rng.integers(0, 256, (1, bb + 5), dtype=np.uint8)
            row, ln = O.null_seal_batch(s["hdr"][p:p + 1], s["hdr_len"][p:p + 1], long_pt,
                                        np.array([bb + 5], np.int32), stride)
            assert ln[0] == s["hdr_len"][p] + 12 + bb + 5
            pkt[p], pkt_len[p] = row[0], ln[0]
            toolong[g] = y
    c.update(wire=pkt, wire_len=pkt_len, kinds=kinds)
    c["open_len"] = np.zeros(n, np.int32)
    c["rows"] = np.zeros((G, k), np.uint8)
    c["blocks_exp"] = np.full(s["data_bytes"], FILL, np.uint8)     # gaps and 255 slots: the fill
    # The open streams a plaintext into its slot before the packet's tag is known (as the
    # uniform call, whose header calls the bytes of a slot tagged 255 unspecified): a slot that
    # ends up tagged 255 after a packet that passed the length checks was streamed into it (its
    # own data packet, or the FEC packet the length checks alone match to the hole) holds that
    # packet's bytes.  Only those slots are exempt; every other 255 slot keeps the fill.
    c["blocks_any"] = np.zeros(s["data_bytes"], bool)
    c["rec_exp"] = np.full(s["rec_bytes"], FILL, np.uint8)
    c["rec_rows"] = np.full((G, rmax), 255, np.uint8)
    c["status"] = np.zeros(G, np.int32)
    for g, bb in enumerate(bbs):
        sl = slice(g * per, (g + 1) * per)
        ol, blocks, rows, ok, rec, rr, st = _expected_open_decode(
            O, k, m, bb, 1, pkt[sl], pkt_len[sl], s["hdr_len"][sl])
        c["open_len"][sl], c["rows"][g], c["status"][g] = ol, rows[0], st[0]
        do, ro = int(s["data_off"][g]), int(s["rec_off"][g])
        pl = pkt_len[sl] - s["hdr_len"][sl] - 12             # plaintext bytes by the lengths alone
        len_ok = (pkt_len[sl] >= 0) & (pl >= 0) & (pl <= bb)
        holes = [i for i in range(k) if not len_ok[i]]
        pre = set(holes[:int(len_ok[k:].sum())])             # holes an FEC packet is streamed into
        for i in range(k):
            if rows[0, i] != 255:
                c["blocks_exp"][do + i * bb:do + (i + 1) * bb] = blocks[0, i]
            elif len_ok[i] or i in pre:
                c["blocks_any"][do + i * bb:do + (i + 1) * bb] = True
        if st[0] == 0:
            c["rec_rows"][g] = rr[0]
            for j in range(rmax):
                if rr[0, j] != 255:
                    # every recovered block is the lost data block
                    assert np.array_equal(rec[0, j], s["blocks"][g][rr[0, j]])
                    c["rec_exp"][ro + j * bb:ro + (j + 1) * bb] = rec[0, j]
        # the kinds did what they were built for
        ks = kinds[g]
        if ks == {"clean"}:
            assert st[0] == 0 and (rr[0] == 255).all() and (ol >= 0).all()
        if "loss1" in ks:
            assert st[0] == 0 and rr[0, 0] == lost[g]
        if "nofec" in ks:
            assert st[0] == -3 and rows[0, lost[g]] == 255
        if "mod8" in ks:
            assert st[0] == -1 and bb % 8 != 0
        if "toolong" in ks:
            assert ol[toolong[g]] == -1
        if "tagfail" in ks:
            assert ol[k] == -1
            if m > 1:       # the length checks alone match FEC packet 0; the tags, packet 1
                assert st[0] == 0 and rows[0, min(lost[g], toolong.get(g, k))] == k + 1
            else:
                assert st[0] == -3
    assert 3 * int((c["status"] == 0).sum()) >= G, c["status"]
    _OPEN[key] = c
    return c


def open_case(O, k, m):
    G, pool = OPEN_SHAPES[(k, m)]
    return build_open_case(O, k, m, draw_sizes(k, m, G, pool))


# ---------------------------------------------------------------- device runs
def run_seal(engine, c, encode, whole, pt_len=None, bb=None, fill=0):
    """One ragged seal into guarded buffers; returns the results and the guard handles."""
    import torch
    k, m, G, n = c["k"], c["m"], c["G"], c["n"]
    if encode:
        par, hpar = guarded((c["par_bytes"],))
    else:
        par, hpar = guarded_from(c["par_given"])
    pkt, hpkt = guarded((n, c["stride"]), fill=fill)
    plen = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda") if encode else None
    ptl = None if whole else dev(c["pt_len"] if pt_len is None else pt_len)
    engine.seal_groups_ragged(k, m, dev(c["bb"] if bb is None else bb), dev(c["data"]),
                              dev(c["data_off"]), par, dev(c["par_off"]), dev(c["hdr"]),
                              dev(c["hdr_len"]), ptl, pkt, plen, encode=encode, status=st)
    from quic_amd import fec
    out = dict(kernels=fec.last_kernels(), pkt=host(pkt), plen=host(plen), par=host(par),
               status=None if st is None else host(st))
    hpkt.check_guards()
    hpar.check_guards()
    return out


def run_open(engine, c, bb=None, stream=None):
    import torch
    k, m, G, n, rmax = c["k"], c["m"], c["G"], c["n"], c["rmax"]
    blocks, hb = guarded((c["data_bytes"],))
    rec, hr = guarded((c["rec_bytes"],))
    t = dict(rows=torch.full((G, k), 9, dtype=torch.uint8, device="cuda"),
             open_len=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
             rec_rows=torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda"),
             status=torch.full((G,), 7, dtype=torch.int32, device="cuda"))
    engine.open_decode_ragged(k, m, dev(c["bb"] if bb is None else bb), dev(c["wire"]),
                              dev(c["wire_len"]), dev(c["hdr_len"]), blocks, dev(c["data_off"]),
                              t["rows"], t["open_len"], rec, dev(c["rec_off"]), t["rec_rows"],
                              status=t["status"])
    from quic_amd import fec
    out = dict(kernels=fec.last_kernels(), blocks=host(blocks), rec=host(rec))
    out.update({name: host(v) for name, v in t.items()})
    hb.check_guards()
    hr.check_guards()
    return out


def used_mask(c, rec_rows, status):
    """Bytes of the packed rec buffer that hold a recovered block / that a status-0 group
    leaves unwritten (entries past its erasure count); gaps are in neither."""
    used = np.zeros(c["rec_bytes"], bool)
    spare = np.zeros(c["rec_bytes"], bool)
    for g, bb in enumerate(c["bbs"]):
        ro = int(c["rec_off"][g])
        for j in range(c["rmax"]):
            if status[g] == 0:
                (used if rec_rows[g, j] != 255 else spare)[ro + j * bb:ro + (j + 1) * bb] = True
    return used, spare


def gap_mask(c, off_name, nblk, total):
    gaps = np.ones(total, bool)
    for g, bb in enumerate(c["bbs"]):
        o = int(c[off_name][g])
        gaps[o:o + nblk * bb] = False
    return gaps


def check_open(c, out):
    np.testing.assert_array_equal(out["open_len"], c["open_len"])
    np.testing.assert_array_equal(out["rows"], c["rows"])
    # filled slots hold the plaintexts, zero-padded; gaps and slots tagged 255 keep the fill
    # (but for the slots a packet with a failing tag was streamed into, build_open_case)
    cmp = ~c["blocks_any"]
    np.testing.assert_array_equal(out["blocks"][cmp], c["blocks_exp"][cmp])
    np.testing.assert_array_equal(out["status"], c["status"])
    np.testing.assert_array_equal(out["rec_rows"], c["rec_rows"])
    used, spare = used_mask(c, c["rec_rows"], c["status"])
    # every recovered block equals the lost data block (rec_exp holds them, build_open_case)
    np.testing.assert_array_equal(out["rec"][used], c["rec_exp"][used])
    assert (out["rec"][spare] == FILL).all()
    assert (out["rec"][gap_mask(c, "rec_off", c["rmax"], c["rec_bytes"])] == FILL).all()


# ---------------------------------------------------------------- 1. seal vs oracle
@pytest.mark.parametrize("whole", [False, True], ids=["pt_len", "whole_blocks"])
@pytest.mark.parametrize("encode", [False, True], ids=["parity_given", "encode"])
@pytest.mark.parametrize("k,m", sorted(SEAL_SHAPES))
def test_seal_ragged_vs_oracle(engine, oracle, k, m, encode, whole):
    """Packets, pkt_len, parity and status bit-exact with the oracle's per-group encode and
    per-packet NullEncrypter.  encode: a group the encode rejects (m > 1, bb % 8 != 0) has
    status -1, its XOR parity, and none of its packets sealed."""
    c = seal_case(oracle, k, m)
    out = run_seal(engine, c, encode, whole)
    exp = (c["pkt_whole"] if whole else c["pkt"]).copy()
    elen = (c["plen_whole"] if whole else c["plen"]).copy()
    if encode:
        for g in np.flatnonzero(c["rej"]):
            exp[g * c["per"]:(g + 1) * c["per"]] = 0
            elen[g * c["per"]:(g + 1) * c["per"]] = -1
        np.testing.assert_array_equal(out["status"], np.where(c["rej"], -1, 0))
        np.testing.assert_array_equal(out["par"], c["par_exp"])
    else:
        np.testing.assert_array_equal(out["par"], c["par_given"])
    np.testing.assert_array_equal(out["plen"], elen)
    np.testing.assert_array_equal(out["pkt"], exp)


# ---------------------------------------------------------------- 2. open -> decode vs oracle
@pytest.mark.parametrize("k,m", sorted(OPEN_SHAPES))
def test_open_decode_ragged_vs_oracle(engine, oracle, k, m):
    """open_len, rows, filled blocks, status, rec_rows and the recovered blocks against the
    oracle's NullDecrypter and decode of every group; the kinds of group each case holds by
    construction are group_kinds' (asserted in build_open_case)."""
    c = open_case(oracle, k, m)
    out = run_open(engine, c)
    check_open(c, out)
    assert 3 * int((out["status"] == 0).sum()) >= c["G"]


# ---------------------------------------------------------------- 3. ragged equals uniform
@pytest.mark.parametrize("k,m,G", [(10, 1, 13), (32, 4, 5)])
def test_pp_ragged_equals_uniform(engine, oracle, k, m, G):
    """Every bb[g] = 1352: packets, lengths, parity, open_len, rows, filled blocks, rec,
    rec_rows and status are byte-identical to seal_groups / open_decode on the same inputs."""
    import torch
    bb = 1352
    c = build_open_case(oracle, k, m, [bb] * G)
    n, rmax, per = c["n"], c["rmax"], c["per"]
    out = run_seal(engine, c, True, False)
    data = np.stack(c["blocks"])
    u_par = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    u_pkt = torch.zeros((n, c["stride"]), dtype=torch.uint8, device="cuda")
    u_len = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    engine.seal_groups(k, m, bb, dev(data), u_par, dev(c["hdr"]), dev(c["hdr_len"]),
                       dev(c["pt_len"]), u_pkt, u_len, encode=True)
    np.testing.assert_array_equal(out["pkt"], host(u_pkt))
    np.testing.assert_array_equal(out["plen"], host(u_len))
    for g in range(G):
        po = int(c["par_off"][g])
        np.testing.assert_array_equal(out["par"][po:po + m * bb], host(u_par)[g].ravel())
    ro = run_open(engine, c)
    u = dict(blocks=torch.full((G, k, bb), FILL, dtype=torch.uint8, device="cuda"),
             rows=torch.full((G, k), 9, dtype=torch.uint8, device="cuda"),
             open_len=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
             rec=torch.full((G, rmax, bb), FILL, dtype=torch.uint8, device="cuda"),
             rec_rows=torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda"),
             status=torch.full((G,), 7, dtype=torch.int32, device="cuda"))
    engine.open_decode(k, m, bb, dev(c["wire"]), dev(c["wire_len"]), dev(c["hdr_len"]),
                       u["blocks"], u["rows"], u["open_len"], u["rec"], u["rec_rows"], u["status"])
    u = {name: host(v) for name, v in u.items()}
    for name in ("open_len", "rows", "rec_rows", "status"):
        np.testing.assert_array_equal(ro[name], u[name], err_msg=name)
    for g in range(G):
        do, rc = int(c["data_off"][g]), int(c["rec_off"][g])
        for i in np.flatnonzero(u["rows"][g] != 255):
            np.testing.assert_array_equal(ro["blocks"][do + i * bb:do + (i + 1) * bb],
                                          u["blocks"][g, i])
        for j in np.flatnonzero(u["rec_rows"][g] != 255):
            np.testing.assert_array_equal(ro["rec"][rc + j * bb:rc + (j + 1) * bb],
                                          u["rec"][g, j])


# ---------------------------------------------------------------- 4. nothing else is written
@pytest.mark.parametrize("k,m", [(10, 1), (5, 5)])
def test_pp_ragged_writes_nothing_else(engine, oracle, k, m):
    """Packed buffers with 16-48-byte gaps and guard regions, everything pre-filled: gaps,
    guards (checked in run_seal / run_open), slots tagged 255 and rejected packets' rows keep
    the fill.  One group has bb = 0: its packets get length -1, on the open its rows are 255,
    its status -3 and its rec_rows 255, and its neighbours are as without it.  One packet of
    another group has a pt_len of bb + 1: rejected, nothing written."""
    c = open_case(oracle, k, m)
    per, z = c["per"], 3
    big = (z + 2) * per + 1                                  # a data packet two groups on
    bb0 = c["bb"].copy()
    bb0[z] = 0
    pt_len = c["pt_len"].copy()
    pt_len[big] = c["bbs"][z + 2] + 1
    out = run_seal(engine, c, True, False, pt_len=pt_len, bb=bb0, fill=FILL)
    elen = c["plen"].copy()
    elen[z * per:(z + 1) * per] = -1
    elen[big] = -1
    for g in np.flatnonzero(c["rej"]):
        elen[g * per:(g + 1) * per] = -1
    exp = np.full_like(c["pkt"], FILL)
    for p in np.flatnonzero(elen >= 0):
        exp[p, :elen[p]] = c["pkt"][p, :elen[p]]
    np.testing.assert_array_equal(out["plen"], elen)
    np.testing.assert_array_equal(out["pkt"], exp)
    par_exp = c["par_exp"].copy()
    po = int(c["par_off"][z])
    par_exp[po:po + m * c["bbs"][z]] = FILL                  # the skipped group's parity region
    np.testing.assert_array_equal(out["par"], par_exp)
    keep = np.arange(c["G"]) != z
    np.testing.assert_array_equal(out["status"][keep], np.where(c["rej"], -1, 0)[keep])
    # open: the same batch with group z skipped
    e = dict(c)
    for name in ("open_len", "rows", "blocks_exp", "blocks_any", "rec_exp", "rec_rows", "status"):
        e[name] = c[name].copy()
    e["open_len"][z * per:(z + 1) * per] = -1
    e["rows"][z], e["rec_rows"][z], e["status"][z] = 255, 255, -3
    do = int(c["data_off"][z])
    e["blocks_exp"][do:do + k * c["bbs"][z]] = FILL
    e["blocks_any"][do:do + k * c["bbs"][z]] = False         # nothing of it is written at all
    check_open(e, run_open(engine, c, bb=bb0))


# ---------------------------------------------------------------- 5. names and limits
def test_pp_ragged_kernel_names_and_limits(engine, oracle):
    """qfec_last_kernels names the ragged kernels and none of the uniform grouped ones; the
    call-level limits return -2 with nothing written."""
    import ctypes
    import torch
    from quic_amd.fec import FecError
    c = open_case(oracle, 5, 5)
    names = run_seal(engine, c, True, False)["kernels"].split(" + ")
    assert "null_seal_kernel<ragged>" in names and "gf_ragged_kernel<encode>" in names
    assert not {"null_seal_kernel<groups>", "null_seal_kernel"} & set(names)
    names = run_seal(engine, c, False, False)["kernels"].split(" + ")
    assert names == ["null_seal_kernel<ragged>"]
    names = run_open(engine, c)["kernels"].split(" + ")
    assert {"open_group_kernel<ragged>", "open_assemble_kernel<ragged>",
            "gf_ragged_kernel<decode>"} <= set(names)
    assert not {"open_group_kernel", "open_assemble_kernel"} & set(names)

    L, h = engine.lib, engine._h
    vp = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731

    def seal(k, m, pkt_stride=1400, null=None, encode=False):
        n = k + m
        t = dict(bb=dev(np.array([1352], np.int32)), off=dev(np.zeros(1, np.int64)),
                 data=torch.zeros(k * 1352, dtype=torch.uint8, device="cuda"),
                 par=torch.zeros(m * 1352, dtype=torch.uint8, device="cuda"),
                 pkt=torch.full((n, pkt_stride + 8), FILL, dtype=torch.uint8, device="cuda"),
                 plen=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                 st=torch.full((1,), 7, dtype=torch.int32, device="cuda"))
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        args = [h, k, m, 1, a["bb"], a["data"], a["off"], a["par"], a["off"], None, 0, None, 0,
                None, a["pkt"], pkt_stride, a["plen"]]
        if encode:
            rc = L.qfec_encode_seal_groups_batch_ragged(*args, a["st"], None)
        else:
            rc = L.qfec_seal_groups_batch_ragged(*args, None)
        assert (host(t["pkt"]) == FILL).all() and (host(t["plen"]) == 7).all()
        assert (host(t["st"]) == 7).all() and (host(t["par"]) == 0).all()
        return rc

    for encode in (False, True):
        assert seal(250, 7, encode=encode) == -2             # k + m = 257
        assert seal(10, 1, pkt_stride=1401, encode=encode) == -2     # an odd pkt_stride
        for null in ("bb", "data", "par", "pkt", "plen", "off"):
            assert seal(10, 1, null=null, encode=encode) == -2, null

    def opn(k, m, null=None, pkt_stride=1400):
        n, rmax = k + m, min(k, m)
        t = dict(bb=dev(np.array([1352], np.int32)), off=dev(np.zeros(1, np.int64)),
                 pkt=torch.zeros((n, pkt_stride), dtype=torch.uint8, device="cuda"),
                 plen=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                 blocks=torch.full((k * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rows=torch.full((k,), 9, dtype=torch.uint8, device="cuda"),
                 ol=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                 rec=torch.full((rmax * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rr=torch.full((rmax,), 9, dtype=torch.uint8, device="cuda"),
                 st=torch.full((1,), 7, dtype=torch.int32, device="cuda"))
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        rc = L.qfec_open_decode_batch_ragged(h, k, m, 1, a["bb"], a["pkt"], pkt_stride, a["plen"],
                                             None, 16, a["blocks"], a["off"], a["rows"], a["ol"],
                                             a["rec"], a["off"], a["rr"], a["st"], None)
        if rc:
            for name, fill in (("blocks", FILL), ("rows", 9), ("ol", 7), ("rec", FILL), ("rr", 9),
                               ("st", 7)):
                assert (host(t[name]) == fill).all(), name
        return rc

    assert opn(250, 5) == 0                                  # k + m = 255: the largest group
    assert opn(250, 6) == -2                                 # k + m = 256
    for null in ("bb", "pkt", "plen", "blocks", "off", "rows", "ol", "rec", "rr"):
        assert opn(10, 1, null=null) == -2, null
    # the wrapper raises on the same limits
    t = torch.zeros(257 * 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(FecError) as ei:
        engine.seal_groups_ragged(250, 7, dev(np.array([8], np.int32)), t,
                                  dev(np.zeros(1, np.int64)), t, dev(np.zeros(1, np.int64)),
                                  None, 0, None, torch.zeros((257, 32), dtype=torch.uint8,
                                                             device="cuda"),
                                  torch.zeros(257, dtype=torch.int32, device="cuda"))
    assert ei.value.rc == -2


# ---------------------------------------------------------------- 6. host variants
@pytest.mark.parametrize("chunk", [0, 1], ids=["one_chunk", "many_chunks"])
@pytest.mark.parametrize("k,m", sorted(HOST_G))
def test_pp_ragged_host_variants(oracle, k, m, chunk):
    """qfec_encode_seal_groups_batch_ragged_host / qfec_open_decode_batch_ragged_host against
    the device calls and the oracle, in one chunk and with host_chunk_mb = 1 (several chunks:
    the packet rows of every batch here exceed 1 MiB).  h_pkt rows come back whole, zeros past their
    lengths and in rejected rows; a pre-filled h_rec keeps the caller's bytes where nothing is
    recovered."""
    import torch
    from quic_amd import fec
    G, pool = HOST_G[(k, m)], SEAL_SHAPES[(k, m)][1]
    c = build_open_case(oracle, k, m, draw_sizes(k, m, G, pool))
    n, rmax = c["n"], c["rmax"]
    eng = fec.FecEngine(0)
    try:
        if chunk:
            eng.set_option("host_chunk_mb", 1)
        dseal = run_seal(eng, c, True, False)
        dopen = run_open(eng, c)
        h_pkt = torch.full((n, c["stride"]), FILL, dtype=torch.uint8).pin_memory()
        h_len = torch.full((n,), 7, dtype=torch.int32).pin_memory()
        h_st = torch.full((G,), 7, dtype=torch.int32).pin_memory()
        fec.encode_seal_groups_ragged_host_into(
            eng, k, m, torch.from_numpy(c["bb"]), torch.from_numpy(c["data"]).pin_memory(),
            torch.from_numpy(c["data_off"]), torch.from_numpy(c["hdr"]).pin_memory(),
            torch.from_numpy(c["hdr_len"]), torch.from_numpy(c["pt_len"]), h_pkt, h_len, h_st)
        assert "null_seal_kernel<ragged>" in fec.last_kernels()
        np.testing.assert_array_equal(h_len.numpy(), dseal["plen"])
        np.testing.assert_array_equal(h_st.numpy(), dseal["status"])
        np.testing.assert_array_equal(h_pkt.numpy(), dseal["pkt"])      # zeros past each length
        elen = np.where(np.repeat(c["rej"], c["per"]), -1, c["plen"])
        np.testing.assert_array_equal(h_len.numpy(), elen)
        past = np.arange(c["stride"])[None, :] >= np.maximum(elen, 0)[:, None]
        assert (h_pkt.numpy()[past] == 0).all()
        # receiver: h_rec laid out by the caller, pre-filled
        h_rec = torch.full((c["rec_bytes"],), FILL, dtype=torch.uint8).pin_memory()
        h_rr = torch.full((G, rmax), 9, dtype=torch.uint8).pin_memory()
        h_st = torch.full((G,), 7, dtype=torch.int32).pin_memory()
        h_ol = torch.full((n,), 7, dtype=torch.int32).pin_memory()
        fec.open_decode_ragged_host_into(
            eng, k, m, torch.from_numpy(c["bb"]), torch.from_numpy(c["wire"]).pin_memory(),
            torch.from_numpy(c["wire_len"]), torch.from_numpy(c["hdr_len"]), h_rec,
            torch.from_numpy(c["rec_off"]), h_rr, h_st, h_ol)
        assert "open_group_kernel<ragged>" in fec.last_kernels()
        for name, got in (("open_len", h_ol), ("status", h_st), ("rec_rows", h_rr)):
            np.testing.assert_array_equal(got.numpy(), dopen[name], err_msg=name)
            np.testing.assert_array_equal(got.numpy(), c[name], err_msg=name)
        used, spare = used_mask(c, c["rec_rows"], c["status"])
        rec = h_rec.numpy()
        np.testing.assert_array_equal(rec[used], dopen["rec"][used])
        np.testing.assert_array_equal(rec[used], c["rec_exp"][used])
        assert (rec[spare] == FILL).all()
        assert (rec[gap_mask(c, "rec_off", rmax, c["rec_bytes"])] == FILL).all()
        # descending offsets are refused before anything is staged
        bad_off = torch.from_numpy(c["rec_off"][::-1].copy())
        with pytest.raises((fec.FecError, ValueError)):
            fec.open_decode_ragged_host_into(
                eng, k, m, torch.from_numpy(c["bb"]), torch.from_numpy(c["wire"]),
                torch.from_numpy(c["wire_len"]), torch.from_numpy(c["hdr_len"]), h_rec, bad_off,
                h_rr, h_st, h_ol)
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. graph capture
def test_pp_ragged_open_decode_graph_capture(oracle):
    """A ragged open -> decode captured into a HIP graph after qfec_reserve with the largest
    bb, replayed twice: the eager result each time, no allocation during the capture."""
    import torch
    from quic_amd.fec import FecEngine
    k, m = 32, 4
    c = open_case(oracle, k, m)
    G, n, rmax = c["G"], c["n"], c["rmax"]
    eng = FecEngine(0)
    try:
        eager = run_open(eng, c)
        check_open(c, eager)
        eng.reserve(k, m, int(c["bb"].max()), G)
        bb, wire, wlen, hlen = dev(c["bb"]), dev(c["wire"]), dev(c["wire_len"]), dev(c["hdr_len"])
        boff, roff = dev(c["data_off"]), dev(c["rec_off"])
        t = dict(blocks=torch.full((c["data_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                 rec=torch.full((c["rec_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                 rows=torch.full((G, k), 9, dtype=torch.uint8, device="cuda"),
                 open_len=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                 rec_rows=torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda"),
                 status=torch.full((G,), 7, dtype=torch.int32, device="cuda"))
        fills = dict(blocks=FILL, rec=FILL, rows=9, open_len=7, rec_rows=9, status=7)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.open_decode_ragged(k, m, bb, wire, wlen, hlen, t["blocks"], boff, t["rows"],
                                   t["open_len"], t["rec"], roff, t["rec_rows"],
                                   status=t["status"], stream=s.cuda_stream)
        torch.cuda.synchronize()
        for _ in range(2):
            for name, v in t.items():
                v.fill_(fills[name])
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            got = {name: host(v) for name, v in t.items()}
            check_open(c, got)
            for name in got:
                np.testing.assert_array_equal(got[name], eager[name], err_msg=name)
    finally:
        eng.close()
