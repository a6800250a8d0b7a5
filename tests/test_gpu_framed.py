"""GPU: the framed protected paths (qfec_frame_encode_seal_groups_batch_ragged,
qfec_open_decode_extract_batch_ragged and the two kernels on their own) against
tests/ref_framing.py, the oracle codec and the oracle's NullEncrypter / NullDecrypter.
Everything is bit-exact.

The shapes are the ragged protection tests': one wave handles 64 consecutive packets, so
several groups of different size share a tile, groups straddle two tiles and the last tile is
partial.  The case builders run on the CPU and are cached; tests/test_framed_abi.py checks
their construction without a GPU."""
import numpy as np
import pytest

from tests import ref_framing as R
from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_pp_ragged import dev, host, packed_gaps

pytestmark = pytest.mark.gpu

SHAPES = {(10, 1): 13, (2, 2): 40, (5, 5): 14, (32, 4): 5, (10, 20): 5}
LENS = [1350, 1349, 1346, 1343, 1000, 46, 7, 6, 1, 0]     # 1346: no padding, 1343: 7 bytes
HDR_LENS = [0, 13, 16]
HMAX = 16
PN = [1, 2, 4, 6]
PN_ALL = {(5, 5): 4}                 # this shape passes one pn_len for every packet
PAY_STRIDE = {(10, 1): 1351, (2, 2): 1400, (5, 5): 1351, (32, 4): 1400, (10, 20): 1351}
BASE = 1000                          # packet number of a group's first packet (tests.ref_framing)
# receiver: what happens to group g's packets, g mod len(KINDS); every shape has G >= 5
KINDS = ["loss", "tagfail", "unrec", "nofec", "tamper", "toolong", "clean", "loss2"]


def up8(v):
    return (v + 7) & ~7


_SEND = {}


def build_send(O, k, m, G, lens=None, stride=None):
    """One sender batch and what the reference says about it (cached, read-only): payload rows
    pay [G*k][stride] with lengths pay_len and pn, the framed blocks (ref_framing.prefix,
    zero-padded to bb = roundup8(max(len + 2))), the oracle's parity, and every wire packet:
    data packet = null_seal(hdr, payload), FEC packet = null_seal(hdr, parity block)."""
    key = (k, m, G, None if lens is None else tuple(lens), stride)
    if key in _SEND:
        return _SEND[key]
    rng = np.random.default_rng(3571 * k + 13 * m + G)
    per, n, rmax = k + m, G * (k + m), min(k, m)
    stride = PAY_STRIDE[(k, m)] if stride is None else stride
    if lens is None:
        lens = np.zeros(G * k, np.int32)
        for g in range(G):
            # the group's longest payload walks through LENS; the others take every length
            # that fits in turn, so each shape holds all of LENS and a tile mixes them
            top = LENS[7 * g % len(LENS)]
            pool = [v for v in LENS if v <= top]
            for i in range(k):
                want = LENS[(g * k + i) % len(LENS)]
                lens[g * k + i] = want if want <= top else rng.choice(pool)
            lens[g * k + int(rng.integers(k))] = top
    lens = np.asarray(lens, np.int32)
    pn = rng.choice(PN, G * k).astype(np.uint8)
    if (k, m) in PN_ALL:
        pn[:] = PN_ALL[(k, m)]
    bbs = [up8(int(lens[g * k:(g + 1) * k].max()) + 2) for g in range(G)]
    c = dict(k=k, m=m, G=G, per=per, n=n, rmax=rmax, pay_stride=stride, pay_len=lens, pn=pn,
             bb=np.array(bbs, np.int32), bbs=bbs)
    c["pkt_stride"] = (HMAX + 12 + max(bbs) + 8 + 3) // 4 * 4
    c["data_off"], c["data_bytes"] = packed_gaps(k, bbs, rng)
    c["par_off"], c["par_bytes"] = packed_gaps(m, bbs, rng)
    c["pay"] = rng.integers(0, 256, (G * k, stride), dtype=np.uint8)
    c["hdr"] = rng.integers(0, 256, (n, HMAX), dtype=np.uint8)
    c["hdr_len"] = rng.choice(HDR_LENS, n).astype(np.int32)
    c["data_exp"] = np.full(c["data_bytes"], FILL, np.uint8)
    c["par_exp"] = np.full(c["par_bytes"], FILL, np.uint8)
    c["pkt"] = np.zeros((n, c["pkt_stride"]), np.uint8)
    c["plen"] = np.zeros(n, np.int32)
    c["payloads"], c["parity"] = [], []
    for g, bb in enumerate(bbs):
        rows_pt = np.zeros((per, bb), np.uint8)
        ptl = np.full(per, bb, np.int32)
        blocks = np.zeros((k, bb), np.uint8)
        pls = []
        for i in range(k):
            q = g * k + i
            payload = c["pay"][q, :lens[q]].tobytes()
            pls.append(payload)
            pre = R.prefix(payload, int(pn[q]))
            blocks[i, :len(pre)] = np.frombuffer(pre, np.uint8)
            rows_pt[i, :lens[q]] = c["pay"][q, :lens[q]]
            ptl[i] = lens[q]
        par, rc = O.encode_batch(k, m, bb, blocks[None])
        assert rc == 0
        # the block size and the parity are the reference group layer's (getRedundancyPackets)
        red, rrc = R.redundancy(O, k, m, BASE, [(BASE + i, pls[i], int(pn[g * k + i]))
                                                for i in range(k)])
        assert rrc == 0 and all(len(d) == bb for _, d, _ in red)
        for pnum, d, _ in red:
            assert d == par[0, pnum - BASE - k].tobytes()
        rows_pt[k:] = par[0]
        do, po = int(c["data_off"][g]), int(c["par_off"][g])
        c["data_exp"][do:do + k * bb] = blocks.ravel()
        c["par_exp"][po:po + m * bb] = par[0].ravel()
        sl = slice(g * per, (g + 1) * per)
        c["pkt"][sl], c["plen"][sl] = O.null_seal_batch(c["hdr"][sl], c["hdr_len"][sl], rows_pt,
                                                        ptl, c["pkt_stride"])
        c["payloads"].append(pls)
        c["parity"].append(par[0])
    assert (c["plen"] >= 0).all()
    _SEND[key] = c
    return c


def send_case(O, k, m):
    return build_send(O, k, m, SHAPES[(k, m)])


def group_kind(g, k, m):
    kind = KINDS[g % len(KINDS)]
    if kind == "loss2" and min(k, m) < 2:
        kind = "loss"
    return kind


_RECV = {}


def build_recv(O, k, m, G, framed_rx_block_bytes):
    """A receiver batch made of build_send's wire packets, and what the reference does with
    it: the oracle's NullDecrypter on every packet, the group layer's placement (a data packet
    stored behind its prefix, quic_fec_group.cc:178-183; holes filled with the opened FEC packets,
    ascending), the oracle's decode, and ref_framing.revive's payloads.  bb[g] is
    framed_rx_block_bytes' (quic_amd.fec), taken before the 'toolong' packet is put in.
    Kinds (group_kind): loss / loss2 (data packets lost; loss also drops FEC packet 0 when
    m > 1), tagfail (a data packet lost and the first FEC packet tampered, so the assemble
    re-matches), unrec (a data packet and every FEC packet lost: not recoverable), nofec (no FEC
    packet received, nothing lost: bb is not rounded and the status is 0), tamper (a data packet
    tampered), toolong (a data packet whose plaintext is bb - 1 long: rejected), clean."""
    from tests.test_gpu_parity import expected_recovered
    key = (k, m, G)
    if key in _RECV:
        return _RECV[key]
    s = build_send(O, k, m, G)
    rng = np.random.default_rng(9176 * k + 5 * m + G)
    per, n, rmax, stride = s["per"], s["n"], s["rmax"], s["pkt_stride"]
    c = dict(s)
    wire, wlen = s["pkt"].copy(), s["plen"].copy()
    kinds = [group_kind(g, k, m) for g in range(G)]
    lost = {g: [] for g in range(G)}
    for g in range(G):
        p0, kind = g * per, kinds[g]
        if kind in ("loss", "tagfail", "unrec"):
            lost[g] = [int(rng.integers(k))]
        if kind == "loss2":
            lost[g] = sorted(int(x) for x in rng.choice(k, 2, replace=False))
        for x in lost[g]:
            wlen[p0 + x] = -1
        if kind == "loss" and m > 1:
            wlen[p0 + k] = -1
        if kind in ("unrec", "nofec"):
            wlen[p0 + k:p0 + per] = -1
        if kind == "tagfail":
            p = p0 + k
            wire[p, s["hdr_len"][p] + 12 + int(rng.integers(s["bbs"][g]))] ^= 0x40
        if kind == "tamper":
            x = int(np.argmax(s["pay_len"][g * k:(g + 1) * k]))      # a packet with a payload
            p = p0 + x
            wire[p, s["hdr_len"][p] + int(rng.integers(12 + max(1, s["pay_len"][g * k + x])))] ^= 1
            lost[g] = [x]
    bb = np.asarray(framed_rx_block_bytes(k, m, wlen, s["hdr_len"]), np.int32)
    toolong = {}
    for g in range(G):
        if kinds[g] == "toolong":
            x = int(rng.integers(k))
            p = g * per + x
            ln = int(bb[g]) - 1
            pt = rng.integers(0, 256, (1, ln), dtype=np.uint8)
            row, rl = O.null_seal_batch(s["hdr"][p:p + 1], s["hdr_len"][p:p + 1], pt,
                                        np.array([ln], np.int32), stride)
            assert rl[0] == s["hdr_len"][p] + 12 + ln
            wire[p], wlen[p] = row[0], rl[0]
            toolong[g] = x
            lost[g] = [x]
    bbs = [int(b) for b in bb]
    c.update(wire=wire, wire_len=wlen, kinds=kinds, lost=lost, rbb=bb, rbbs=bbs)
    c["pn_rx"] = np.ones(n, np.uint8)
    for g in range(G):
        c["pn_rx"][g * per:g * per + k] = s["pn"][g * k:(g + 1) * k]
    c["blocks_off"], c["blocks_bytes"] = packed_gaps(k, bbs, rng)
    c["rec_off"], c["rec_bytes"] = packed_gaps(rmax, bbs, rng)
    c["rev_stride"] = 1351
    c["open_len"] = np.full(n, -1, np.int32)
    c["rows"] = np.full((G, k), 255, np.uint8)
    c["blocks_exp"] = np.full(c["blocks_bytes"], FILL, np.uint8)
    c["blocks_any"] = np.zeros(c["blocks_bytes"], bool)      # see tests/test_gpu_pp_ragged.py
    c["rec_exp"] = np.full(c["rec_bytes"], FILL, np.uint8)
    c["rec_rows"] = np.full((G, rmax), 255, np.uint8)
    c["status"] = np.full(G, -3, np.int32)
    c["rev_exp"] = np.full((G * rmax, c["rev_stride"]), FILL, np.uint8)
    c["rev_len"] = np.full(G * rmax, -1, np.int32)
    c["rev_pn"] = np.full(G * rmax, FILL, np.uint8)
    rcv = wlen >= 0
    plain, res = O.null_open_batch(wire, np.where(rcv, wlen, s["hdr_len"]), s["hdr_len"],
                                   (max(bbs) + 12 + 3) // 4 * 4 + 64)
    for g, b in enumerate(bbs):
        p0 = g * per
        lim = np.array([b - 2] * k + [b] * m)
        pl = wlen[p0:p0 + per] - s["hdr_len"][p0:p0 + per] - 12
        len_ok = rcv[p0:p0 + per] & (pl >= 0) & (pl <= lim)
        ol = np.where(len_ok & (res[p0:p0 + per] >= 0), res[p0:p0 + per], -1).astype(np.int32)
        c["open_len"][p0:p0 + per] = ol
        blocks = np.zeros((k, b), np.uint8)
        rows = np.full(k, 255, np.uint8)
        stored = []                                          # the group layer's received list
        avail = [j for j in range(m) if ol[k + j] >= 0]
        h = 0
        for i in range(k):
            if ol[i] >= 0:
                pre = R.prefix(plain[p0 + i, :ol[i]].tobytes(), int(c["pn_rx"][p0 + i]))
                rows[i] = i
                blocks[i, :len(pre)] = np.frombuffer(pre, np.uint8)
                stored.append((BASE + i, pre))
            elif h < len(avail):
                j = avail[h]
                h += 1
                rows[i] = k + j
                blocks[i, :ol[k + j]] = plain[p0 + k + j, :ol[k + j]]
        stored += [(BASE + k + j, plain[p0 + k + j, :ol[k + j]].tobytes()) for j in avail]
        c["rows"][g] = rows
        do, ro = int(c["blocks_off"][g]), int(c["rec_off"][g])
        holes = [i for i in range(k) if not len_ok[i]]
        pre_set = set(holes[:int(len_ok[k:].sum())])
        for i in range(k):
            if rows[i] != 255:
                c["blocks_exp"][do + i * b:do + (i + 1) * b] = blocks[i]
            elif len_ok[i] or i in pre_set:
                c["blocks_any"][do + i * b:do + (i + 1) * b] = True
        if (rows != 255).all():
            b_or, r_or, s_or = O.decode_batch(k, m, b, blocks[None], rows[None])
            rec, rr = expected_recovered(k, m, b, rows[None], b_or, r_or, s_or)
            c["status"][g] = s_or[0]
            if s_or[0] == 0:
                c["rec_rows"][g] = rr[0]
                revived, rrc = R.revive(O, k, m, BASE, stored)
                assert rrc == 0
                by_pn = {pnum: (pay, pnl) for pnum, pay, pnl in revived}
                for j in range(rmax):
                    if rr[0, j] == 255:
                        continue
                    c["rec_exp"][ro + j * b:ro + (j + 1) * b] = rec[0, j]
                    pay, pnl = by_pn[BASE + int(rr[0, j])]
                    q = g * rmax + j
                    c["rev_exp"][q, :len(pay)] = np.frombuffer(pay, np.uint8)
                    c["rev_len"][q], c["rev_pn"][q] = len(pay), pnl
                    if kinds[g] != "toolong":                # the revived packet is the lost one
                        x = int(rr[0, j])
                        assert pay == s["payloads"][g][x]
                        assert pnl == {1: 1, 2: 2, 4: 0, 6: 2}[int(s["pn"][g * k + x])]
        # the kinds did what they were built for
        kind, st, rr = kinds[g], c["status"][g], c["rec_rows"][g]
        if kind in ("loss", "loss2", "tamper", "toolong"):
            assert st == 0 and [int(x) for x in rr[:len(lost[g])]] == lost[g], (kind, g)
            assert ol[lost[g][0]] == -1
        if kind == "tagfail":
            assert ol[k] == -1 and st == (0 if m > 1 else -3)
            if m > 1:
                assert rows[lost[g][0]] == k + 1             # by length FEC 0, by tag FEC 1
        if kind == "unrec":
            assert st == -3 and rows[lost[g][0]] == 255
        if kind == "nofec":
            assert st == 0 and (rr == 255).all() and (ol[:k] >= 0).all()
            assert b == int(s["pay_len"][g * k:(g + 1) * k].max()) + 2
        if kind == "clean":
            assert st == 0 and (rr == 255).all() and (ol >= 0).all() and b == s["bbs"][g]
    assert any(b % 8 for g, b in enumerate(bbs) if kinds[g] == "nofec")
    assert (c["rev_len"] >= 0).sum() >= 3
    _RECV[key] = c
    return c


def recv_case(O, k, m):
    from quic_amd import fec
    return build_recv(O, k, m, SHAPES[(k, m)], fec.framed_rx_block_bytes)


# ---------------------------------------------------------------- device runs
def pn_arg(c, key="pn"):
    """The pn_len argument: the array, or the one value where every packet has it."""
    a = c[key]
    if (c["k"], c["m"]) in PN_ALL and key == "pn":
        return int(a[0])
    return dev(a)


def run_send(engine, c, bb=None, pay=None, pay_len=None, alone=False):
    """frame -> encode -> seal (or the frame alone) into guarded, gapped buffers."""
    import torch
    from quic_amd import fec
    k, m, G, n = c["k"], c["m"], c["G"], c["n"]
    data, hdata = guarded((c["data_bytes"],))
    payv, hpay = guarded_from(c["pay"] if pay is None else pay, offset=3)
    bbv = dev(c["bb"] if bb is None else bb)
    plv = dev(c["pay_len"] if pay_len is None else pay_len)
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    if alone:
        engine.frame_blocks_ragged(k, bbv, payv, plv, pn_arg(c), data, dev(c["data_off"]),
                                   status=st)
        out = dict(kernels=fec.last_kernels(), data=host(data), status=host(st))
        hdata.check_guards()
        return out
    par, hpar = guarded((c["par_bytes"],))
    pkt, hpkt = guarded((n, c["pkt_stride"]))
    plen = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    engine.frame_encode_seal_ragged(k, m, bbv, data, dev(c["data_off"]), par, dev(c["par_off"]),
                                    dev(c["hdr"]), dev(c["hdr_len"]), payv, plv, pn_arg(c), pkt,
                                    plen, status=st)
    out = dict(kernels=fec.last_kernels(), data=host(data), par=host(par), pkt=host(pkt),
               plen=host(plen), status=host(st))
    for h in (hdata, hpar, hpkt, hpay):
        h.check_guards()
    return out


def recv_tensors(c):
    import torch
    G, k, n, rmax = c["G"], c["k"], c["n"], c["rmax"]
    return dict(rows=torch.full((G, k), 9, dtype=torch.uint8, device="cuda"),
                open_len=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                rec_rows=torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda"),
                status=torch.full((G,), 7, dtype=torch.int32, device="cuda"),
                rev_len=torch.full((G * rmax,), 7, dtype=torch.int32, device="cuda"),
                rev_pn=torch.full((G * rmax,), FILL, dtype=torch.uint8, device="cuda"))


def call_recv(engine, c, a, blocks, rec, rev, t, stream=None):
    engine.open_decode_extract_ragged(
        c["k"], c["m"], a["bb"], a["wire"], a["wire_len"], a["hdr_len"], a["pn"], blocks,
        a["blocks_off"], t["rows"], t["open_len"], rec, a["rec_off"], t["rec_rows"], rev,
        t["rev_len"], rev_pn_len=t["rev_pn"], status=t["status"], stream=stream)


def recv_args(c):
    # the PN_ALL shape passes its one pn_len for every packet on the receiver too: only the data
    # packets' prefixes are written from it, and every data packet of that shape has that value
    pn = PN_ALL.get((c["k"], c["m"]))
    return dict(bb=dev(c["rbb"]), wire=dev(c["wire"]), wire_len=dev(c["wire_len"]),
                hdr_len=dev(c["hdr_len"]), pn=dev(c["pn_rx"]) if pn is None else pn,
                blocks_off=dev(c["blocks_off"]), rec_off=dev(c["rec_off"]))


def run_recv(engine, c):
    from quic_amd import fec
    blocks, hb = guarded((c["blocks_bytes"],))
    rec, hr = guarded((c["rec_bytes"],))
    rev, hv = guarded((c["G"] * c["rmax"], c["rev_stride"]), offset=5)
    t = recv_tensors(c)
    call_recv(engine, c, recv_args(c), blocks, rec, rev, t)
    out = dict(kernels=fec.last_kernels(), blocks=host(blocks), rec=host(rec), rev=host(rev))
    out.update({name: host(v) for name, v in t.items()})
    for h in (hb, hr, hv):
        h.check_guards()
    return out


def check_recv(c, out):
    np.testing.assert_array_equal(out["open_len"], c["open_len"])
    np.testing.assert_array_equal(out["rows"], c["rows"])
    cmp = ~c["blocks_any"]
    np.testing.assert_array_equal(out["blocks"][cmp], c["blocks_exp"][cmp])
    np.testing.assert_array_equal(out["status"], c["status"])
    np.testing.assert_array_equal(out["rec_rows"], c["rec_rows"])
    # rec: the recovered blocks; the unused entries of a status-0 group and the gaps keep the
    # fill (the rec bytes of a group with another status are unspecified, as in the ragged call)
    used = np.zeros(c["rec_bytes"], bool)
    free = np.zeros(c["rec_bytes"], bool)
    for g, b in enumerate(c["rbbs"]):
        o = int(c["rec_off"][g])
        if c["status"][g] != 0:
            free[o:o + c["rmax"] * b] = True
        for j in range(c["rmax"]):
            if c["rec_rows"][g, j] != 255:
                used[o + j * b:o + (j + 1) * b] = True
    np.testing.assert_array_equal(out["rec"][used], c["rec_exp"][used])
    assert (out["rec"][~used & ~free] == FILL).all()
    # revived payloads; a row past its length, and a row with rev_len -1, keep the guard value
    np.testing.assert_array_equal(out["rev_len"], c["rev_len"])
    np.testing.assert_array_equal(out["rev_pn"], c["rev_pn"])
    np.testing.assert_array_equal(out["rev"], c["rev_exp"])


# ---------------------------------------------------------------- 1. sender
@pytest.mark.parametrize("k,m", sorted(SHAPES))
def test_frame_encode_seal_vs_reference(engine, oracle, k, m):
    """Blocks = ref_framing.prefix zero-padded, parity = the oracle's, data packet =
    null_seal(hdr, payload) with no prefix on the wire, FEC packet = null_seal(hdr, parity
    block); pkt_len, status, gaps and guard bytes.  The frame kernel alone writes the same
    blocks."""
    c = send_case(oracle, k, m)
    out = run_send(engine, c)
    np.testing.assert_array_equal(out["status"], np.zeros(c["G"], np.int32))
    np.testing.assert_array_equal(out["data"], c["data_exp"])
    np.testing.assert_array_equal(out["par"], c["par_exp"])
    np.testing.assert_array_equal(out["plen"], c["plen"])
    exp = np.full_like(c["pkt"], FILL)
    for p in range(c["n"]):
        exp[p, :c["plen"][p]] = c["pkt"][p, :c["plen"][p]]
    np.testing.assert_array_equal(out["pkt"], exp)
    alone = run_send(engine, c, alone=True)
    np.testing.assert_array_equal(alone["data"], c["data_exp"])
    np.testing.assert_array_equal(alone["status"], np.zeros(c["G"], np.int32))


# ---------------------------------------------------------------- 2. receiver
@pytest.mark.parametrize("k,m", sorted(SHAPES))
def test_open_decode_extract_vs_reference(engine, oracle, k, m):
    """open_len, rows, the placed blocks (prefix included), rec, rec_rows and status against
    the oracle's open, the group layer's placement and the oracle's decode; rev, rev_len and
    rev_pn_len against ref_framing.revive for every lost data packet."""
    c = recv_case(oracle, k, m)
    check_recv(c, run_recv(engine, c))


# ---------------------------------------------------------------- 3. the group layer
@pytest.mark.parametrize("k,m", [(5, 5), (10, 1)])
def test_wire_compatible_with_group_layer(engine, oracle, k, m):
    """One group through the device calls and through qfec_group_update_sent /
    qfec_group_redundancy and qfec_group_update_received / qfec_group_revived: those parity
    blocks are the FEC packets' plaintexts, those revived packets are rev."""
    from quic_amd import fec_group as F
    c = recv_case(oracle, k, m)
    sent = run_send(engine, c)
    got = run_recv(engine, c)
    g = c["kinds"].index("loss")
    per, rmax, p0 = c["per"], c["rmax"], g * c["per"]
    F.set_fec_overrides(k, m)
    try:
        s = F.QuicFecGroup(BASE, F.FEC_5_5)
        for i in range(k):
            s.UpdateSentList(2, BASE + i, int(c["pn"][g * k + i]), c["payloads"][g][i])
        red, st = s.getRedundancyPackets()
        assert st == 0 and len(red) == m
        for pnum, d, _ in red:
            p = p0 + (pnum - BASE)
            hl = int(c["hdr_len"][p])
            assert bytes(sent["pkt"][p, hl + 12:sent["plen"][p]]) == d
        r = F.QuicFecGroup(BASE, F.FEC_5_5)
        for i in range(per):
            if c["open_len"][p0 + i] < 0:
                continue
            p = p0 + i
            hl = int(c["hdr_len"][p])
            pt = bytes(c["wire"][p, hl + 12:c["wire_len"][p]])
            assert r.UpdateReceivedList(2, BASE + i, int(c["pn_rx"][p]), pt, i >= k)
        rev, rst = r.getRevivedPackets()
    finally:
        F.set_fec_overrides(0, 0)
    assert rst == 0 and len(rev) == len(c["lost"][g]) > 0
    for pnum, pay, pnl in rev:
        j = [int(x) for x in got["rec_rows"][g]].index(pnum - BASE)
        q = g * rmax + j
        assert got["rev_len"][q] == len(pay) and got["rev_pn"][q] == pnl
        assert bytes(got["rev"][q, :len(pay)]) == pay


# ---------------------------------------------------------------- 4. rejection
def test_sender_rejects_groups(engine, oracle):
    """A group with a length of bb - 1, one with a length of 0x4000 (the stride is large enough)
    and one with bb[g] = 0: status -3, every pkt_len -1, nothing of them written; their
    neighbours are exact."""
    k, m, G = 5, 5, 7
    stride = 0x4008
    rng = np.random.default_rng(5)
    lens = rng.choice([46, 7, 6, 1, 0, 1000], G * k).astype(np.int32)
    lens[3 * k + 2] = 0x3fff                                  # the largest length there is
    lens[k] = 1000
    c = build_send(oracle, k, m, G, lens=lens, stride=stride)
    assert c["bbs"][3] == 16392
    bb, pl = c["bb"].copy(), c["pay_len"].copy()
    bb[1] = int(pl[k:2 * k].max()) + 1                         # its longest payload is bb - 1
    pl[3 * k + 2] = 0x4000
    bb[5] = 0
    bad = [1, 3, 5]
    out = run_send(engine, c, bb=bb, pay_len=pl)
    est = np.zeros(G, np.int32)
    est[bad] = -3
    np.testing.assert_array_equal(out["status"], est)
    elen, epkt = c["plen"].copy(), np.full_like(c["pkt"], FILL)
    dexp, pexp = c["data_exp"].copy(), c["par_exp"].copy()
    for g in bad:
        elen[g * c["per"]:(g + 1) * c["per"]] = -1
        do, po = int(c["data_off"][g]), int(c["par_off"][g])
        dexp[do:do + k * c["bbs"][g]] = FILL
        pexp[po:po + m * c["bbs"][g]] = FILL
    for p in np.flatnonzero(elen >= 0):
        epkt[p, :elen[p]] = c["pkt"][p, :elen[p]]
    np.testing.assert_array_equal(out["plen"], elen)
    np.testing.assert_array_equal(out["pkt"], epkt)
    np.testing.assert_array_equal(out["data"], dexp)
    np.testing.assert_array_equal(out["par"], pexp)
    alone = run_send(engine, c, bb=bb, pay_len=pl, alone=True)
    np.testing.assert_array_equal(alone["status"], est)
    np.testing.assert_array_equal(alone["data"], dexp)


def test_receiver_length_limits(engine, oracle):
    """A data packet whose plaintext is bb - 1 long is rejected (the 'toolong' groups), while an
    FEC packet's plaintext of bb bytes is accepted."""
    c = recv_case(oracle, 5, 5)
    out = run_recv(engine, c)
    gs = [g for g in range(c["G"]) if c["kinds"][g] == "toolong"]
    assert gs
    for g in gs:
        p0, x = g * c["per"], c["lost"][g][0]
        hl = c["hdr_len"][p0:p0 + c["per"]]
        assert c["wire_len"][p0 + x] - hl[x] - 12 == c["rbbs"][g] - 1
        assert out["open_len"][p0 + x] == -1
        assert out["open_len"][p0 + c["k"]] == c["rbbs"][g]   # an FEC packet: the whole block
        assert out["status"][g] == 0


# ---------------------------------------------------------------- 5. the clamp
def test_extract_clamps_to_block(engine, oracle):
    """A recovered block whose prefix claims more than bb - 2 bytes is extracted at bb - 2 bytes
    (the reference reads past the block there): a hand-made block through the bare ragged codec,
    then qfec_extract_revived_batch_ragged alone."""
    import torch
    k, m, bb, G = 4, 2, 64, 2
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, (G, k, bb), dtype=np.uint8)
    data[0, 1, :2] = [0xff, 0x7f]                              # len 0x3fff, pn bits 1
    data[1, 2, :2] = [bb - 1, 0x80]                            # len bb - 1, pn bits 2
    bbv = dev(np.full(G, bb, np.int32))
    doff = dev(np.arange(G, dtype=np.int64) * k * bb)
    poff = dev(np.arange(G, dtype=np.int64) * m * bb)
    par = torch.zeros(G * m * bb, dtype=torch.uint8, device="cuda")
    assert engine.encode_ragged(k, m, bbv, dev(data.ravel()), doff, par, poff) == 0
    blocks, rows = data.copy(), np.tile(np.arange(k, dtype=np.uint8), (G, 1))
    parh = host(par).reshape(G, m, bb)
    for g, x in ((0, 1), (1, 2)):
        blocks[g, x], rows[g, x] = parh[g, 0], k
    rec = torch.full((G * m * bb,), FILL, dtype=torch.uint8, device="cuda")
    rr = torch.full((G, m), 9, dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    engine.decode_ragged_recovered(k, m, bbv, dev(blocks.ravel()), doff, dev(rows), rec, poff, rr,
                                   status=st)
    rev, hv = guarded((G * m, 100), offset=1)
    rl = torch.full((G * m,), 7, dtype=torch.int32, device="cuda")
    rp = torch.full((G * m,), FILL, dtype=torch.uint8, device="cuda")
    engine.extract_revived_ragged(k, m, bbv, rec, poff, rr, st, rev, rl, rp)
    from quic_amd import fec
    assert fec.last_kernels() == "extract_revived_kernel"
    hv.check_guards()
    np.testing.assert_array_equal(host(rl), [bb - 2, -1, bb - 2, -1])
    np.testing.assert_array_equal(host(rp), [1, FILL, 2, FILL])
    exp = np.full((G * m, 100), FILL, np.uint8)
    exp[0, :bb - 2], exp[2, :bb - 2] = data[0, 1, 2:], data[1, 2, 2:]
    np.testing.assert_array_equal(host(rev), exp)
    # a row too short for the payload: -1 and nothing written
    rev2, hv2 = guarded((G * m, bb - 3))
    engine.extract_revived_ragged(k, m, bbv, rec, poff, rr, None, rev2, rl, None)
    hv2.check_guards()
    assert (host(rl) == -1).all() and (host(rev2) == FILL).all()


# ---------------------------------------------------------------- 6. names and limits
def test_framed_kernel_names_and_limits(engine, oracle):
    import ctypes
    import torch
    c = recv_case(oracle, 5, 5)
    names = run_send(engine, c)["kernels"].split(" + ")
    assert names[0] == "frame_blocks_kernel" and names[-1] == "null_seal_kernel<framed>"
    assert "gf_ragged_kernel<encode>" in names
    assert run_send(engine, c, alone=True)["kernels"] == "frame_blocks_kernel"
    names = run_recv(engine, c)["kernels"].split(" + ")
    assert names[:2] == ["open_group_kernel<framed>", "open_assemble_kernel<framed>"]
    assert names[-1] == "extract_revived_kernel" and "gf_ragged_kernel<decode>" in names

    L, h = engine.lib, engine._h
    vp = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731

    def send(k, m, null=None, pkt_stride=1400, pay_stride=1351):
        n = k + m
        t = dict(bb=dev(np.array([1352], np.int32)), off=dev(np.zeros(1, np.int64)),
                 data=torch.full((k * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 par=torch.full((m * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 pay=torch.zeros((k, 1351), dtype=torch.uint8, device="cuda"),
                 pl=torch.full((k,), 100, dtype=torch.int32, device="cuda"),
                 pkt=torch.full((n, pkt_stride + 8), FILL, dtype=torch.uint8, device="cuda"),
                 plen=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                 st=torch.full((1,), 7, dtype=torch.int32, device="cuda"))
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        rc = L.qfec_frame_encode_seal_groups_batch_ragged(
            h, k, m, 1, a["bb"], a["data"], a["off"], a["par"], a["off"], None, 0, None, 0,
            a["pay"], pay_stride, a["pl"], None, 1, a["pkt"], pkt_stride, a["plen"], a["st"], None)
        if rc:
            for name, fill in (("data", FILL), ("par", FILL), ("pkt", FILL), ("plen", 7),
                               ("st", 7)):
                assert (host(t[name]) == fill).all(), name
        return rc

    assert send(10, 1) == 0
    assert send(250, 7) == -2                                # k + m = 257
    assert send(10, 1, pkt_stride=1401) == -2
    assert send(10, 1, pay_stride=-1) == -2
    for null in ("bb", "off", "data", "par", "pay", "pl", "pkt", "plen"):
        assert send(10, 1, null=null) == -2, null

    def recv(k, m, null=None, rev_stride=1351):
        n, rmax = k + m, min(k, m)
        t = dict(bb=dev(np.array([1352], np.int32)), off=dev(np.zeros(1, np.int64)),
                 pkt=torch.zeros((n, 1400), dtype=torch.uint8, device="cuda"),
                 plen=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                 blocks=torch.full((k * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rows=torch.full((k,), 9, dtype=torch.uint8, device="cuda"),
                 ol=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
                 rec=torch.full((rmax * 1352,), FILL, dtype=torch.uint8, device="cuda"),
                 rr=torch.full((rmax,), 9, dtype=torch.uint8, device="cuda"),
                 st=torch.full((1,), 7, dtype=torch.int32, device="cuda"),
                 rev=torch.full((rmax, 1351), FILL, dtype=torch.uint8, device="cuda"),
                 rl=torch.full((rmax,), 7, dtype=torch.int32, device="cuda"))
        a = {name: (None if name == null else vp(v)) for name, v in t.items()}
        rc = L.qfec_open_decode_extract_batch_ragged(
            h, k, m, 1, a["bb"], a["pkt"], 1400, a["plen"], None, 16, None, 1, a["blocks"],
            a["off"], a["rows"], a["ol"], a["rec"], a["off"], a["rr"], a["st"], a["rev"],
            rev_stride, a["rl"], None, None)
        if rc:
            for name, fill in (("blocks", FILL), ("rows", 9), ("ol", 7), ("rec", FILL), ("rr", 9),
                               ("st", 7), ("rev", FILL), ("rl", 7)):
                assert (host(t[name]) == fill).all(), name
        return rc

    assert recv(250, 5) == 0                                 # k + m = 255
    assert recv(250, 6) == -2
    assert recv(10, 1, rev_stride=-1) == -2
    for null in ("bb", "pkt", "plen", "blocks", "off", "rows", "ol", "rec", "rr", "rev", "rl"):
        assert recv(10, 1, null=null) == -2, null


# ---------------------------------------------------------------- 7. graph capture
def test_open_decode_extract_graph_capture(oracle):
    """qfec_open_decode_extract_batch_ragged captured into a HIP graph after qfec_reserve and
    replayed twice: the eager result each time."""
    import torch
    from quic_amd.fec import FecEngine
    k, m = 32, 4
    c = recv_case(oracle, k, m)
    eng = FecEngine(0)
    try:
        eager = run_recv(eng, c)
        check_recv(c, eager)
        eng.reserve(k, m, int(c["rbb"].max()), c["G"])
        a = recv_args(c)
        t = recv_tensors(c)
        fills = dict(rows=9, open_len=7, rec_rows=9, status=7, rev_len=7, rev_pn=FILL)
        bufs = dict(blocks=torch.full((c["blocks_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                    rec=torch.full((c["rec_bytes"],), FILL, dtype=torch.uint8, device="cuda"),
                    rev=torch.full((c["G"] * c["rmax"], c["rev_stride"]), FILL,
                                   dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call_recv(eng, c, a, bufs["blocks"], bufs["rec"], bufs["rev"], t,
                      stream=s.cuda_stream)
        torch.cuda.synchronize()
        for _ in range(2):
            for name, v in t.items():
                v.fill_(fills[name])
            for v in bufs.values():
                v.fill_(FILL)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            got = {name: host(v) for name, v in {**t, **bufs}.items()}
            check_recv(c, got)
            for name in got:
                if name == "rec":
                    continue                                 # checked by check_recv
                keep = ~c["blocks_any"] if name == "blocks" else slice(None)
                np.testing.assert_array_equal(got[name][keep], eager[name][keep], err_msg=name)
    finally:
        eng.close()
