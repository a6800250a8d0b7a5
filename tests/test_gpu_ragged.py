"""Ragged batches on the GPU: groups that share (k, m) but carry their own block_bytes, in one
launch (qfec_*_batch_ragged*), against the CPU oracle called once per group with that group's
block size.  Bit-exact.  Every output buffer is pre-filled with a poison byte: the gaps between
groups, a tail canary, every rec entry past a group's erasure count and the regions of groups
with a negative status must still hold it afterwards.  Run with -m gpu."""
import random

import numpy as np
import pytest

from quic_amd import fec
from quic_amd import fec_group as F
from tests import ref_framing as R

pytestmark = pytest.mark.gpu

POISON = 0xA5
# s = bb / 8 = 1, 2, 3 (byte-wise), 4, 5, 13, 65 (17 words), 169 (43 words, partial last word),
# 257 (65 words: a second tile with one live lane), 258
GF_SIZES = [8, 16, 24, 32, 40, 104, 520, 1352, 2056, 2064]
XOR_EXTRA = [1, 7, 15, 17, 1350]
KINDS = ["none", "r1", "rmax", "parity_only", "ooo", "malformed"]


def up16(v):
    return (v + 15) & ~15


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def packed(n, bbs):
    """Offsets of groups of n blocks, 16-byte aligned, with a further 16-byte gap after every
    other group, and the buffer size including a 64-byte tail canary."""
    off, run = [], 0
    for g, b in enumerate(bbs):
        off.append(run)
        run = up16(run + n * b) + (16 if g % 2 == 0 else 0)
    return np.array(off, np.int64), run + 64


def sizes_for(k, m, G, rng):
    pool = GF_SIZES + (XOR_EXTRA if (m == 1 or k <= 1) else [])
    if G == 1:
        return [1352]
    bbs = [pool[i % len(pool)] for i in range(G)] if G >= len(pool) else \
        [pool[i] for i in rng.choice(len(pool), G, replace=False)]
    bbs = [int(b) for b in bbs]
    rng.shuffle(bbs)
    return bbs


def receive_rows(rng, k, m, kind):
    """Row tags of one group's receive set (slot i holds the block with row rows[i])."""
    rmax = min(k, m)
    if k == 1:
        return [0] if kind in ("none", "parity_only") else [1 + int(rng.integers(m))]
    rows = list(range(k))
    if kind == "none":
        return rows
    if kind == "parity_only":            # only parity packets dropped: nothing to recover
        rng.shuffle(rows)
        return rows
    if kind == "malformed":              # the same recovery row twice
        a, b = sorted(rng.choice(k, 2, replace=False))
        rows[a] = rows[b] = k + int(rng.integers(m))
        return rows
    r = 1 if (kind == "r1" or m == 1) else rmax if kind == "rmax" else min(2, rmax)
    lost = sorted(int(x) for x in rng.choice(k, r, replace=False))
    par = sorted(int(x) for x in rng.choice(min(m, 256 - k), r, replace=False))   # tags are u8
    if kind == "ooo":                    # parity rows received out of order
        par = par[::-1]
    for x, y in zip(lost, par):
        rows[x] = k + y
    if kind == "ooo":
        rng.shuffle(rows)
    return rows


_CASES = {}


def build_case(O, k, m, bbs, kinds, seed):
    """One batch and everything the oracle says about it (cached: computed once, read-only)."""
    key = (k, m, tuple(bbs), tuple(kinds), seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed)
    G, rmax = len(bbs), min(k, m)
    c = dict(k=k, m=m, G=G, rmax=rmax, bb=np.array(bbs, np.int32))
    c["data_off"], c["data_bytes"] = packed(k, bbs)
    c["par_off"], c["par_bytes"] = packed(m, bbs)
    c["rec_off"], c["rec_bytes"] = packed(rmax, bbs)
    c["data"] = np.full(c["data_bytes"], 0x11, np.uint8)
    c["blocks"] = np.full(c["data_bytes"], 0x22, np.uint8)
    c["rows"] = np.zeros((G, k), np.uint8)
    c["par_exp"] = np.full(c["par_bytes"], POISON, np.uint8)
    c["rec_exp"] = np.full(c["rec_bytes"], POISON, np.uint8)
    c["enc_status"] = np.zeros(G, np.int32)
    c["dec_status"] = np.zeros(G, np.int32)
    c["rec_rows"] = np.full((G, rmax), 255, np.uint8)
    c["nrec"] = np.zeros(G, np.int64)
    for g, bb in enumerate(bbs):
        data = rng.integers(0, 256, size=(k, bb), dtype=np.uint8)
        par, rc = O.encode_ptrs(k, m, bb, list(data))
        do, po, ro = int(c["data_off"][g]), int(c["par_off"][g]), int(c["rec_off"][g])
        c["data"][do:do + k * bb] = data.ravel()
        c["enc_status"][g] = rc
        nwritten = m if rc == 0 else 1          # -1: the XOR parity only (cauchy_256.cpp:1519-1534)
        c["par_exp"][po:po + nwritten * bb] = par[:nwritten].ravel()
        kind = kinds[g % len(kinds)]
        if kind == "malformed" and (m == 1 or k < 2):
            kind = "r1"                         # no -3 exists for m = 1 / k = 1
        rows = receive_rows(rng, k, m, kind)
        sent = np.concatenate([data, par])
        blocks = sent[rows]
        c["blocks"][do:do + k * bb] = blocks.ravel()
        c["rows"][g] = rows
        if kind == "malformed":
            c["dec_status"][g] = -1 if bb % 8 else -3
            continue
        arrs, rows2, drc = O.decode_blocks(k, m, bb, list(blocks), rows)
        c["dec_status"][g] = drc
        if drc != 0:
            continue
        rec = []
        if k <= 1:
            if rows[0] != 0:
                rec = [(0, blocks[0])]
        else:
            slots = [i for i in range(k) if rows[i] >= k]
            for sl in (slots[:1] if m == 1 else slots):
                if rows2[sl] < k:
                    rec.append((rows2[sl], arrs[sl]))
        assert [x for x, _ in rec] == sorted(x for x, _ in rec)
        for j, (x, blk) in enumerate(rec):
            np.testing.assert_array_equal(blk, data[x])      # the oracle recovered the data
            c["rec_rows"][g][j] = x
            c["rec_exp"][ro + j * bb:ro + (j + 1) * bb] = blk
        c["nrec"][g] = len(rec)
    _CASES[key] = c
    return c


def mixed_case(O, k, m, G):
    rng = np.random.default_rng(1000 * k + 10 * m + G)
    return build_case(O, k, m, sizes_for(k, m, G, rng), KINDS, seed=7 * k + m + G)


def run_device(engine, c, what="both"):
    import torch
    k, m, G = c["k"], c["m"], c["G"]
    bb = dev(c["bb"])
    out = {}
    if what in ("both", "encode"):
        par = torch.full((c["par_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        out["enc_rc"] = engine.encode_ragged(k, m, bb, dev(c["data"]), dev(c["data_off"]), par,
                                             dev(c["par_off"]), status=st)
        out["enc_kernels"] = fec.last_kernels()
        out["par"], out["enc_status"] = host(par), host(st)
    if what in ("both", "decode"):
        rec = torch.full((c["rec_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        blocks, rows = dev(c["blocks"]), dev(c["rows"])
        engine.decode_ragged_recovered(k, m, bb, blocks, dev(c["data_off"]), rows, rec,
                                       dev(c["rec_off"]), rr, status=st)
        out["dec_kernels"] = fec.last_kernels()
        out["rec"], out["rec_rows"], out["dec_status"] = host(rec), host(rr), host(st)
        np.testing.assert_array_equal(host(blocks), c["blocks"])     # inputs untouched
        np.testing.assert_array_equal(host(rows), c["rows"])
    return out


def check(c, out):
    if "par" in out:
        np.testing.assert_array_equal(out["enc_status"], c["enc_status"])
        np.testing.assert_array_equal(out["par"], c["par_exp"])
    if "rec" in out:
        np.testing.assert_array_equal(out["dec_status"], c["dec_status"])
        np.testing.assert_array_equal(out["rec_rows"], c["rec_rows"])
        np.testing.assert_array_equal(out["rec"], c["rec_exp"])


CODES = [(10, 1), (3, 2), (5, 5), (32, 4), (10, 20), (1, 3)]


@pytest.mark.parametrize("G", [1, 7, 203])
@pytest.mark.parametrize("k,m", CODES)
def test_ragged_vs_oracle(engine, oracle, k, m, G):
    c = mixed_case(oracle, k, m, G)
    if G == 203:
        assert set(c["bb"].tolist()) >= set(GF_SIZES)
        assert (c["dec_status"] == -3).any() == (m > 1 and k > 1)
    out = run_device(engine, c)
    assert out["enc_rc"] == 0
    check(c, out)


def test_ragged_250_5(engine, oracle):
    c = mixed_case(oracle, 250, 5, 12)
    assert set(c["bb"].tolist()) == set(GF_SIZES)
    out = run_device(engine, c)
    assert out["enc_rc"] == 0
    check(c, out)


def test_ragged_status_minus_one(engine, oracle):
    """(5, 5) with two groups of 1350 bytes: encode status -1 for exactly those two, their first
    parity block holds the XOR of their data and nothing else of them is written; on decode the
    same two report -1 and leave their rec regions poisoned.  The others match the oracle."""
    bbs = [1352, 1350, 520, 104, 1350, 2056, 40]
    c = build_case(oracle, 5, 5, bbs, ["r1", "rmax", "ooo"], seed=55)
    assert c["enc_status"].tolist() == [0, -1, 0, 0, -1, 0, 0]
    assert c["dec_status"].tolist() == [0, -1, 0, 0, -1, 0, 0]
    for g in (1, 4):
        do, po, bb = int(c["data_off"][g]), int(c["par_off"][g]), 1350
        x = np.bitwise_xor.reduce(c["data"][do:do + 5 * bb].reshape(5, bb), axis=0)
        np.testing.assert_array_equal(c["par_exp"][po:po + bb], x)
        assert (c["par_exp"][po + bb:po + 5 * bb] == POISON).all()
    out = run_device(engine, c)
    assert out["enc_rc"] == 0                      # the call succeeds; the groups carry the -1
    check(c, out)
    # a group of that size that lost nothing still has status 0 (cauchy_256.cpp:1287-1289)
    c2 = build_case(oracle, 5, 5, [1350, 1352], ["none"], seed=56)
    assert c2["dec_status"].tolist() == [0, 0]
    check(c2, run_device(engine, c2, "decode"))


def test_ragged_k_plus_m_over_256(engine, oracle):
    """m > 1 and k + m > 256: as qfec_encode_batch, every group gets its XOR parity and the call
    returns -1; the decode reports -1 for the groups that hold a recovery block."""
    c = build_case(oracle, 250, 7, [16, 24, 1352], ["r1", "none"], seed=3)
    assert c["enc_status"].tolist() == [-1, -1, -1] and c["dec_status"].tolist() == [-1, 0, -1]
    out = run_device(engine, c)
    assert out["enc_rc"] == -1
    check(c, out)


def test_ragged_equals_uniform(engine, oracle):
    """Every bb[g] = 1352 with (32, 4): the same bytes as qfec_encode_batch /
    qfec_decode_batch_recovered."""
    import torch
    k, m, bb, G = 32, 4, 1352, 7
    c = build_case(oracle, k, m, [bb] * G, KINDS, seed=99)
    out = run_device(engine, c)
    check(c, out)
    data = np.stack([c["data"][o:o + k * bb].reshape(k, bb) for o in c["data_off"]])
    blocks = np.stack([c["blocks"][o:o + k * bb].reshape(k, bb) for o in c["data_off"]])
    par = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    assert engine.encode(k, m, bb, dev(data), par) == 0
    rec = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    rr = torch.zeros((G, m), dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    engine.decode_recovered(k, m, bb, dev(blocks), dev(c["rows"]), rec, rr, status=st)
    par, rec = host(par), host(rec)
    np.testing.assert_array_equal(host(st), out["dec_status"])
    np.testing.assert_array_equal(host(rr), out["rec_rows"])
    for g in range(G):
        po, ro = int(c["par_off"][g]), int(c["rec_off"][g])
        np.testing.assert_array_equal(out["par"][po:po + m * bb], par[g].ravel())
        n = int(c["nrec"][g])              # entries past the count are unspecified in the uniform API
        np.testing.assert_array_equal(out["rec"][ro:ro + n * bb], rec[g][:n].ravel())


def test_ragged_kernel_names(engine, oracle):
    """last_kernels() names the ragged kernels, and a uniform call right after still names its
    usual kernel: the uniform dispatch is untouched."""
    import torch
    k, m, bb, G = 32, 4, 1352, 7
    data = torch.zeros((G, k, bb), dtype=torch.uint8, device="cuda")
    par = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    rows = dev(np.tile(np.arange(k, dtype=np.uint8), (G, 1)))
    rec = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    rr = torch.zeros((G, m), dtype=torch.uint8, device="cuda")
    engine.encode(k, m, bb, data, par)
    enc_before = fec.last_kernels()
    engine.decode_recovered(k, m, bb, data, rows, rec, rr)
    dec_before = fec.last_kernels()
    assert "ragged" not in enc_before + dec_before
    out = run_device(engine, mixed_case(oracle, k, m, 7))
    assert "gf_ragged_kernel<encode>" in out["enc_kernels"]
    assert "gf_ragged_kernel<decode>" in out["dec_kernels"]
    assert "gf_ragged_kernel" in fec.last_grids()
    engine.encode(k, m, bb, data, par)
    assert fec.last_kernels() == enc_before
    engine.decode_recovered(k, m, bb, data, rows, rec, rr)
    assert fec.last_kernels() == dec_before
    out = run_device(engine, mixed_case(oracle, 10, 1, 7))
    assert "xor_ragged_kernel" in out["enc_kernels"] and "gf_" not in out["enc_kernels"]
    assert "xor_ragged_kernel" in out["dec_kernels"] and "gf_" not in out["dec_kernels"]
    torch.cuda.synchronize()


@pytest.mark.parametrize("k,m", [(32, 4), (10, 1), (10, 20)])
def test_ragged_host_variants(oracle, k, m):
    """The same mixed batch through the host entry points with 1 MiB chunks (at least 3 of
    them): the results equal the device path's, which equal the oracle's."""
    import torch
    from quic_amd.fec import FecEngine
    c = mixed_case(oracle, k, m, 203)
    G, rmax = c["G"], c["rmax"]
    assert int(c["data_bytes"]) > 3 << 20 or (k, m) != (32, 4)
    eng = FecEngine(0)
    try:
        eng.set_option("host_chunk_mb", 1)
        dv = run_device(eng, c)
        check(c, dv)
        par = torch.full((int(c["par_bytes"]),), POISON, dtype=torch.uint8)
        est = torch.full((G,), 7, dtype=torch.int32)
        bb_h = torch.from_numpy(c["bb"])
        rc = fec.encode_ragged_host_into(eng, k, m, bb_h, torch.from_numpy(c["data"]),
                                         torch.from_numpy(c["data_off"]), par,
                                         torch.from_numpy(c["par_off"]), est)
        assert rc == 0
        assert "ragged_kernel" in fec.last_kernels()
        np.testing.assert_array_equal(par.numpy(), dv["par"])
        np.testing.assert_array_equal(est.numpy(), dv["enc_status"])
        rec = torch.full((int(c["rec_bytes"]),), POISON, dtype=torch.uint8)
        rr = torch.full((G, rmax), 9, dtype=torch.uint8)
        dst = torch.full((G,), 7, dtype=torch.int32)
        fec.decode_ragged_recovered_host_into(eng, k, m, bb_h, torch.from_numpy(c["blocks"]),
                                              torch.from_numpy(c["data_off"]),
                                              torch.from_numpy(c["rows"]), rec,
                                              torch.from_numpy(c["rec_off"]), rr, dst)
        np.testing.assert_array_equal(rec.numpy(), dv["rec"])
        np.testing.assert_array_equal(rr.numpy(), dv["rec_rows"])
        np.testing.assert_array_equal(dst.numpy(), dv["dec_status"])
        # descending offsets are refused, nothing is written
        with pytest.raises(fec.FecError):
            fec.encode_ragged_host_into(eng, k, m, bb_h[:2].contiguous(),
                                        torch.from_numpy(c["data"]),
                                        torch.from_numpy(c["data_off"][:2][::-1].copy()), par,
                                        torch.from_numpy(c["par_off"][:2].copy()), None)
        np.testing.assert_array_equal(par.numpy(), dv["par"])
    finally:
        eng.close()


def test_ragged_decode_graph_capture(oracle):
    """One ragged decode captured into a HIP graph after qfec_reserve with the largest bb and
    replayed twice: equal results, no allocation during the capture."""
    import torch
    from quic_amd.fec import FecEngine
    k, m = 32, 4
    c = mixed_case(oracle, k, m, 7)
    G = c["G"]
    eng = FecEngine(0)
    try:
        eng.reserve(k, m, int(c["bb"].max()), G)
        bb, blocks, rows = dev(c["bb"]), dev(c["blocks"]), dev(c["rows"])
        boff, roff = dev(c["data_off"]), dev(c["rec_off"])
        rec = torch.full((int(c["rec_bytes"]),), POISON, dtype=torch.uint8, device="cuda")
        rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.decode_ragged_recovered(k, m, bb, blocks, boff, rows, rec, roff, rr, status=st,
                                        stream=s.cuda_stream)
        torch.cuda.synchronize()
        results = []
        for _ in range(2):
            rec.fill_(POISON)
            rr.fill_(9)
            st.fill_(7)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            results.append(dict(rec=host(rec), rec_rows=host(rr), dec_status=host(st)))
        for r in results:
            check(c, r)
        for key in results[0]:
            np.testing.assert_array_equal(results[0][key], results[1][key])
    finally:
        eng.close()


# ------------------------------------------------------------------ the batching queue
def _queue_groups(seed):
    """40 FEC_10_10 sender groups whose largest payload differs per group (40 .. 1350)."""
    rnd = random.Random(seed)
    out = []
    for gi in range(40):
        base = 5000 + gi * 32
        top = rnd.randrange(40, 1351)
        lens = [rnd.randrange(40, top + 1) for _ in range(10)]
        lens[rnd.randrange(10)] = top
        sent = [(base + i, bytes(rnd.getrandbits(8) for _ in range(n)), rnd.choice([1, 2, 4, 6]))
                for i, n in enumerate(lens)]
        out.append((base, sent, F.block_bytes(top + 2)))
    return out


def _sender(base, sent):
    s = F.QuicFecGroup(base, F.FEC_10_10)
    for pn, p, pl in sent:
        s.UpdateSentList(2, pn, pl, p)
    return s


def _receiver(base, sent, par, drop):
    r = F.QuicFecGroup(base, F.FEC_10_10)
    for i, (pn, p, pl) in enumerate(sent):
        if i not in drop:
            r.UpdateReceivedList(2, pn, pl, p, False)
    for pn, d, pl in par:
        r.UpdateFec(2, pn, pl, d)
    assert r.CanRevive()
    return r


def _ragged_launches(name):
    grids = fec.load().qfec_last_grids().decode().split()
    return sum(1 for gr in grids if gr.startswith(name + "="))


@pytest.mark.parametrize("ragged", [True, False])
def test_queue_ragged_buckets(engine, oracle, ragged):
    """40 groups with at least 10 distinct block sizes: with set_ragged(True) one flush is one
    ragged launch, and the packets equal the per-group getRedundancyPackets() /
    getRevivedPackets() path on a second, identical set of groups; with ragged off the same
    input still works as before."""
    F.set_fec_overrides(0, 0)
    k, m = 10, 10
    groups = _queue_groups(17)
    assert len({bb for _, _, bb in groups}) >= 10
    batch = F.FecBatch(engine, max_groups=1000, max_delay_us=10**9)
    if ragged:
        batch.set_ragged(True)
    senders = []
    for base, sent, _ in groups:
        s = _sender(base, sent)
        assert batch.add_encode(s) == 0
        senders.append(s)
    if ragged:
        with pytest.raises(ValueError):
            batch.set_ragged(False)              # not while groups are queued
    assert batch.pending() == 40
    assert batch.flush() == 40 and batch.pending() == 0
    if ragged:
        assert "gf_ragged_kernel<encode>" in fec.last_kernels()
        assert _ragged_launches("gf_ragged_kernel") == 1
    else:
        assert "ragged" not in fec.last_kernels()
    rnd = random.Random(23)
    receivers, expected = [], []
    for (base, sent, _), s in zip(groups, senders):
        par, st = s.getRedundancyPackets()
        par2, st2 = _sender(base, sent).getRedundancyPackets()      # per-group path
        assert st == st2 == 0
        assert par == par2
        assert par == R.redundancy(oracle, k, m, base, sent)[0]
        drop = set(rnd.sample(range(k), rnd.randrange(1, 6)))
        r = _receiver(base, sent, par, drop)
        assert batch.add_decode(r) == 0
        receivers.append(r)
        expected.append(_receiver(base, sent, par, drop).getRevivedPackets())
    assert batch.flush() == 40
    if ragged:
        assert "gf_ragged_kernel<decode>" in fec.last_kernels()
        assert _ragged_launches("gf_ragged_kernel") == 1
    for r, (rev2, st2) in zip(receivers, expected):
        rev, st = r.getRevivedPackets()
        assert st == st2 == 0
        assert rev == rev2 and len(rev) > 0
