"""Byte offsets that need more than 31 and more than 32 bits.  Ordinary in-bounds calls whose
buffers pass 2^32 bytes: a product or an offset that a kernel computes in 32 bits lands inside
the same allocation and shows as a wrong byte or a touched poison byte.

  ragged calls through gaps      a dozen small groups at explicit offsets around 2^31 and 2^32
  packet protection via strides  4,200 packets with a row stride of 2^20 + 4 bytes
  dense uniform batches          the smallest group count at which a buffer passes 2^32 by two
                                 groups, per kernel family

Everything is compared with the CPU oracle, bit-exact; whole buffers are compared on the device.
Run with -m gpu."""
import numpy as np
import pytest

from quic_amd import fec, synth
from tests import test_gpu_pp as PP
from tests import test_gpu_ragged as RG
from tests.guarded import FILL
from tests.test_gpu_parity import dev, expected_recovered, host, tuned_engine  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = RG.POISON
B31, B32 = 2**31, 2**32


def up16(v):
    return (v + 15) & ~15


# ------------------------------------------------------------------ B1: ragged through gaps
RAGGED_BYTES = B32 + 2**29          # every data / parity / rec buffer

# (bb, bb for m = 1 or k = 1, receive-set kind, place) of the 12 groups.  A group cannot both
# straddle a boundary and start at it in one buffer, so there are two layouts: in "straddle"
# the groups placed at 2^31 and 2^32 lie across them, in "exact" they start there.
RAGGED_GROUPS = [
    (1352, 1352, "r1", "zero"),
    (2056, 2056, "rmax", "at31"),
    (1352, 1350, "ooo", "at32"),
    (24, 24, "rmax", "low"),               # 2^20
    (8, 8, "ooo", "below31"),              # 2^31 - 2^16
    (1352, 1, "none", "between"),          # 2^31 + 2^30 + 4112
    (2056, 2056, "r1", "past32"),          # 2^32 + 2^28
    (8, 1, "malformed", "bad3"),           # 2^32 + 2^27: status -3 where the code has one
    (1350, 1350, "r1", "bad1"),            # 2^32 + 2^27 + 2^20: status -1 for m > 1
    (24, 8, "parity_only", "past31"),      # 2^31 + 2^20
    (2056, 2056, "rmax", "end"),           # the last bytes of the buffer
    (1352, 1352, "rmax", "second"),        # right behind group 0, one 16-byte gap
]
RAGGED_CODES = [(10, 1), (32, 4), (5, 5), (1, 3)]


def ragged_offsets(nblk, bbs, layout):
    """The offset of every group in a buffer of nblk blocks per group (multiples of 16)."""
    off = []
    for bb, (_, _, _, place) in zip(bbs, RAGGED_GROUPS):
        size = nblk * bb
        across = up16(size // 2) if layout == "straddle" else 0
        off.append({
            "zero": 0, "second": up16(nblk * bbs[0]) + 16, "low": 2**20, "below31": B31 - 2**16,
            "at31": B31 - across, "past31": B31 + 2**20, "between": B31 + 2**30 + 4112,
            "at32": B32 - across, "bad3": B32 + 2**27, "bad1": B32 + 2**27 + 2**20,
            "past32": B32 + 2**28, "end": (RAGGED_BYTES - size) & ~15,
        }[place])
    off = np.array(off, np.int64)
    assert (off % 16 == 0).all()
    order = np.argsort(off)                      # no overlap, nothing past the end
    ends = off[order] + nblk * np.array(bbs, np.int64)[order]
    assert (ends[:-1] <= off[order][1:]).all() and ends[-1] <= RAGGED_BYTES
    return off


def place_on_device(regions):
    """A poison-filled buffer of RAGGED_BYTES with the (offset, bytes) regions copied in."""
    import torch
    buf = torch.full((RAGGED_BYTES,), POISON, dtype=torch.uint8, device="cuda")
    for off, a in regions:
        buf[off:off + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf


@pytest.mark.parametrize("layout", ["straddle", "exact"])
@pytest.mark.parametrize("k,m", RAGGED_CODES)
def test_ragged_offsets_past_4gib(engine, oracle, k, m, layout):
    """qfec_encode_batch_ragged / qfec_decode_batch_ragged_recovered with explicit 64-bit
    offsets: in each of the data, parity and rec buffers (2^32 + 2^29 bytes, poisoned) one group
    at 0, one across (or exactly at) 2^31, one across (or at) 2^32, one at 2^32 + 2^28, one at
    the buffer's very end, others between.  The oracle's bytes per group are assembled on the
    device and whole buffers compared, so every gap byte is checked; a malformed group (-3) and
    a bb % 8 != 0 group (-1) lie past 2^32 and keep their poison."""
    import torch
    small = m == 1 or k <= 1
    bbs = [(b1 if small else b) for b, b1, _, _ in RAGGED_GROUPS]
    kinds = [kd for _, _, kd, _ in RAGGED_GROUPS]
    G, rmax = len(bbs), min(k, m)
    c = RG.build_case(oracle, k, m, bbs, kinds, seed=31 * k + m)
    if not small:
        assert c["dec_status"][7] == -3 and c["dec_status"][8] == -1 and c["enc_status"][8] == -1
    assert (np.delete(c["dec_status"], [7, 8]) == 0).all()
    offs = {n: ragged_offsets(n_blk, bbs, layout)
            for n, n_blk in (("data", k), ("par", m), ("rec", rmax))}
    for n_blk, off in ((k, offs["data"]), (m, offs["par"]), (rmax, offs["rec"])):
        if layout == "exact":                    # the placement the test is about
            assert off[1] == B31 and off[2] == B32
        else:
            assert off[1] < B31 < off[1] + n_blk * bbs[1] and off[2] < B32 < off[2] + n_blk * bbs[2]
        assert (off >= B32).sum() >= 4 and ((off > B31) & (off < B32)).sum() >= 2
        assert off[10] + n_blk * bbs[10] > RAGGED_BYTES - 16

    def regions(packed, packed_off, nblk, where):
        return [(int(where[g]), packed[int(packed_off[g]):int(packed_off[g]) + nblk * bbs[g]])
                for g in range(G)]
    d_bb = dev(c["bb"])
    d_off = {n: dev(o) for n, o in offs.items()}
    data = place_on_device(regions(c["data"], c["data_off"], k, offs["data"]))
    par = torch.full((RAGGED_BYTES,), POISON, dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    assert engine.encode_ragged(k, m, d_bb, data, d_off["data"], par, d_off["par"], status=st) == 0
    kernels = fec.last_kernels()
    assert ("copy_ragged_kernel" if k == 1 else "xor_ragged_kernel" if m == 1
            else "gf_ragged_kernel<encode>") in kernels
    np.testing.assert_array_equal(host(st), c["enc_status"])
    exp = place_on_device(regions(c["par_exp"], c["par_off"], m, offs["par"]))
    assert torch.equal(par, exp)
    del par
    exp = place_on_device(regions(c["data"], c["data_off"], k, offs["data"]))
    assert torch.equal(data, exp)                # the input is unchanged
    del data, exp

    blocks = place_on_device(regions(c["blocks"], c["data_off"], k, offs["data"]))
    rows = dev(c["rows"])
    rec = torch.full((RAGGED_BYTES,), POISON, dtype=torch.uint8, device="cuda")
    rr = torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda")
    st.fill_(7)
    engine.decode_ragged_recovered(k, m, d_bb, blocks, d_off["data"], rows, rec, d_off["rec"], rr,
                                   status=st)
    kernels = fec.last_kernels()
    assert ("copy_ragged_kernel" if k == 1 else "xor_ragged_kernel" if m == 1
            else "gf_ragged_kernel<decode>") in kernels
    np.testing.assert_array_equal(host(st), c["dec_status"])
    np.testing.assert_array_equal(host(rr), c["rec_rows"])
    np.testing.assert_array_equal(host(rows), c["rows"])
    exp = place_on_device(regions(c["rec_exp"], c["rec_off"], rmax, offs["rec"]))
    assert torch.equal(rec, exp)
    del rec
    exp = place_on_device(regions(c["blocks"], c["data_off"], k, offs["data"]))
    assert torch.equal(blocks, exp)
    del blocks, exp
    torch.cuda.empty_cache()


# ------------------------------------------------- B2: packet protection through strides
PP_STRIDE = 2**20 + 4               # 4-byte aligned, 4 mod 16: row p starts at phase 4 p mod 16
PP_N = 4200                         # row offsets pass 2^31 at packet 2,048, 2^32 at 4,096
PP_COMPACT = 1380                   # 16 + 12 + 1352: the oracle's stride
PP_EDGES = [2047, 2048, 2049, 4095, 4096, 4097]


def strided(n, small=None):
    """[n][PP_STRIDE] on the device, poisoned; `small` [n][w] copied into its first columns."""
    import torch
    t = torch.full((n, PP_STRIDE), POISON, dtype=torch.uint8, device="cuda")
    if small is not None:
        t[:, :small.shape[1]].copy_(dev(small))
    return t


def over_poison(exp, written):
    """The oracle's rows (zeros where it wrote nothing) with the poison where it wrote nothing:
    row i was written up to written[i] bytes."""
    cols = np.arange(exp.shape[1])[None, :]
    return np.where(cols < np.maximum(written, 0)[:, None], exp, POISON).astype(np.uint8)


def rest_is_poison(t, width):
    return bool((t[:, width:] == POISON).all())


def test_null_seal_open_strides_past_4gib(engine, oracle):
    """qfec_null_seal_batch with pt_stride = out_stride = 2^20 + 4 and qfec_null_open_batch with
    pkt_stride = out_stride = 2^20 + 4 over 4,200 packets (4.4 GB per buffer): rows 2,048 and
    4,096 are the first past 2^31 and 2^32.  The oracle runs with compact strides; the first
    1,380 columns must equal it and everything else must still be poison."""
    import torch
    assert (PP_N - 1) * PP_STRIDE > B32 and 2047 * PP_STRIDE < B31 < 2048 * PP_STRIDE
    assert 4095 * PP_STRIDE < B32 < 4096 * PP_STRIDE and PP_STRIDE % 16 == 4
    rng = np.random.default_rng(2048)
    n, AS, S = PP_N, 16, 1352
    near = sorted({e + d for e in PP_EDGES for d in (-1, 0, 1)})      # 2,046 .. 2,050, 4,094 ..
    ad = rng.integers(0, 256, (n, AS), dtype=np.uint8)
    pt = rng.integers(0, 256, (n, S), dtype=np.uint8)
    ad_len = rng.integers(0, AS + 1, n).astype(np.int32)
    pt_len = rng.choice(np.array([0, 1, 15, 16, 17, S, 700, 1351], np.int32), n)
    pt_len[near], ad_len[near] = S, AS                                  # full length at the edges
    assert set(pt_len.tolist()) >= {0, 1, 15, 16, 17, S}
    exp, eres = oracle.null_seal_batch(ad, ad_len, pt, pt_len, PP_COMPACT)
    assert (eres == ad_len + 12 + pt_len).all()
    d_pt = strided(n, pt)
    out = strided(n)
    out_len = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    engine.null_seal(dev(ad), dev(ad_len), d_pt, dev(pt_len), out, out_len)
    assert "null_seal_kernel" in fec.last_kernels()
    assert d_pt.stride(0) == out.stride(0) == PP_STRIDE
    np.testing.assert_array_equal(host(out_len), eres)
    np.testing.assert_array_equal(host(out[:, :PP_COMPACT].contiguous()), over_poison(exp, eres))
    assert rest_is_poison(out, PP_COMPACT)
    assert torch.equal(d_pt[:, :S], dev(pt)) and rest_is_poison(d_pt, S)    # input unchanged

    # open: tampered and short packets on both sides of the two boundaries
    pkt = exp.copy()
    pkt_len = eres.copy()
    tampered = np.array([2046, 2050, 4094, 4098] + rng.choice(n, 200, replace=False).tolist())
    short = np.array([2045, 2051, 4093, 4099] + rng.choice(n, 100, replace=False).tolist())
    tampered = np.setdiff1d(tampered, PP_EDGES + short.tolist())
    short = np.setdiff1d(short, PP_EDGES)
    for i in tampered:
        pkt[i, ad_len[i] + int(rng.integers(0, pkt_len[i] - ad_len[i]))] ^= 1 << int(rng.integers(8))
    pkt_len[short] = ad_len[short] + rng.integers(0, 12, len(short)).astype(np.int32)
    exp_o, eres_o = oracle.null_open_batch(pkt, pkt_len, ad_len, PP_COMPACT)
    assert (eres_o[tampered] == -1).all() and (eres_o[short] == -1).all()
    assert (eres_o[PP_EDGES] == S).all()
    out[:, :PP_COMPACT].copy_(dev(pkt))                                  # the wire packets
    d_pt.fill_(POISON)                                                   # now the open's output
    len_o = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    engine.null_open(out, dev(pkt_len), dev(ad_len), d_pt, len_o)
    assert "null_open_kernel" in fec.last_kernels()
    np.testing.assert_array_equal(host(len_o), eres_o)
    # the output receives the ciphertext (pkt_len - ad_len bytes), then the plaintext over it
    np.testing.assert_array_equal(host(d_pt[:, :PP_COMPACT].contiguous()),
                                  over_poison(exp_o, pkt_len - ad_len))
    assert rest_is_poison(d_pt, PP_COMPACT)
    assert torch.equal(out[:, :PP_COMPACT], dev(pkt)) and rest_is_poison(out, PP_COMPACT)
    del out, d_pt
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k,m", [(10, 1), (5, 5)])
def test_grouped_seal_open_strides_past_4gib(engine, oracle, k, m):
    """qfec_seal_groups_batch and qfec_open_decode_batch with pkt_stride = 2^20 + 4 and at least
    4,200 packets: packet p = g (k + m) + i lies p strides into the buffer."""
    import torch
    bb = 1352
    per = k + m
    G = -(-PP_N // per)
    n = G * per
    assert n >= PP_N and (n - 1) * PP_STRIDE > B32
    rng = np.random.default_rng(k * 1000 + m)
    data, parity, pt_len, hdr, hdr_len, exp, eres = PP._group_packets(oracle, k, m, bb, G, rng)
    W = exp.shape[1]
    pkt = strided(n)
    pkt_len = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    engine.seal_groups(k, m, bb, dev(data), dev(parity), dev(hdr), dev(hdr_len), dev(pt_len),
                       pkt, pkt_len)
    assert "null_seal_kernel<groups>" in fec.last_kernels()
    np.testing.assert_array_equal(host(pkt_len), eres)
    np.testing.assert_array_equal(host(pkt[:, :W].contiguous()), over_poison(exp, eres))
    assert rest_is_poison(pkt, W)

    # receiver: lost and tampered packets (both sides of the boundaries among them), one
    # group that cannot be recovered
    wire, wire_len = exp.copy(), eres.copy()
    q = 0.4 * m / per
    lost = rng.random(n) < 0.7 * q
    lost[PP_EDGES] = False
    wire_len[lost] = -1
    bad = np.flatnonzero(~lost & (rng.random(n) < 0.3 * q)).tolist() + [2046, 4098]
    bad = np.setdiff1d(bad, PP_EDGES + np.flatnonzero(lost).tolist())
    for p in bad:
        wire[p, hdr_len[p] + int(rng.integers(0, 12 + pt_len[p]))] ^= 1 << int(rng.integers(0, 8))
    wire_len[0] = -1
    wire_len[k:per] = -1
    open_len, blocks, rows, ok, rec, rec_rows, status = PP._expected_open_decode(
        oracle, k, m, bb, G, wire, wire_len, hdr_len)
    assert not ok[0] and ok.sum() >= G // 3
    assert (open_len[PP_EDGES] >= 0).all() and (open_len[bad] == -1).all()
    pkt[:, :W].copy_(dev(wire))
    rmax = min(k, m)
    d_blocks = torch.zeros((G, k, bb), dtype=torch.uint8, device="cuda")
    d_rows = torch.zeros((G, k), dtype=torch.uint8, device="cuda")
    d_ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_rec = torch.zeros((G, rmax, bb), dtype=torch.uint8, device="cuda")
    d_rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
    d_st = torch.full((G,), 99, dtype=torch.int32, device="cuda")
    engine.open_decode(k, m, bb, pkt, dev(wire_len), dev(hdr_len), d_blocks, d_rows, d_ol, d_rec,
                       d_rr, d_st)
    assert "open_group_kernel" in fec.last_kernels()
    np.testing.assert_array_equal(host(d_ol), open_len)
    np.testing.assert_array_equal(host(d_rows), rows)
    filled = rows != 255
    np.testing.assert_array_equal(host(d_blocks)[filled], blocks[filled])
    np.testing.assert_array_equal(host(d_st), status)
    np.testing.assert_array_equal(host(d_rr)[ok], rec_rows[ok])
    used = rec_rows != 255
    np.testing.assert_array_equal(host(d_rec)[used], rec[used])
    assert torch.equal(pkt[:, :W], dev(wire)) and rest_is_poison(pkt, W)     # input unchanged
    del pkt
    torch.cuda.empty_cache()


# ------------------------------------------------------------ B4: dense uniform batches
# (id, k, m, bb, blocks per group of the buffer that must pass 2^32, encode kernel, decode
#  kernel, layouts, options)
DENSE = [
    ("xor_dma", 10, 1, 1352, 10, "xor_dma_kernel<encode>", "xor_dma_kernel<decode",
     ("recovered", "outofplace", "inplace"), {}),
    ("xor_flat", 10, 1, 1350, 10, "xor_flat_kernel<encode>", "xor_flat_kernel<decode>",
     ("outofplace", "inplace"), {}),
    ("ring_psyn_10_20", 10, 20, 1352, 10, "gf_ring_kernel<encode", "gf_psyn_kernel<decode",
     ("recovered",), {}),
    ("ring_psyn_5_5", 5, 5, 1352, 5, "gf_ring_kernel<encode", "gf_psyn_kernel<decode",
     ("recovered",), {}),
    ("stream_250_5", 250, 5, 1352, 250, "gf_stream_kernel<encode", "gf_stream_kernel<decode",
     ("recovered", "inplace"), {"stream_static": 0}),
    ("stream_17_12", 17, 12, 1352, 17, "gf_stream_kernel<encode", "gf_stream_kernel<decode",
     ("recovered", "inplace"), {}),
    ("apply_6_3", 6, 3, 4096, 6, "gf_apply_kernel<encode", "gf_apply_kernel<decode",
     ("recovered", "inplace"), {}),
    ("bsyn_32_4", 32, 4, 1352, 32, "gf_ring_kernel<encode", "gf_bsyn_kernel<decode",
     ("outofplace", "inplace"), {}),
]


def dense_groups(nblk, bb):
    """The smallest group count at which a buffer of nblk blocks per group passes 2^32 bytes by
    at least two groups."""
    return B32 // (nblk * bb) + 3


def boundary_samples(G, group_bytes):
    """Groups to compare with the oracle byte for byte: the first and last two; in every buffer
    (its bytes per group in `group_bytes`) the group that holds byte 2^31 and the one that holds
    byte 2^32, with both neighbours; and the aliases of the last two groups, the groups that
    hold byte (offset mod 2^32) and (offset mod 2^31) of those groups' first bytes."""
    s = {0, 1, G - 2, G - 1}
    for gsz in group_bytes:
        for edge in (B31, B32):
            if G * gsz > edge:
                g = edge // gsz
                s |= {g - 1, g, g + 1}
        for g in (G - 2, G - 1):
            for mod in (B32, B31):
                if g * gsz >= mod:
                    s.add((g * gsz) % mod // gsz)
    return sorted(g for g in s if 0 <= g < G)


def recovered_equal_originals(got, rows_in, rows_out, data, k, what):
    """Every slot tagged as a recovery block holds its original, batch-wide on the device, in
    slices of groups that bound the gathered temporaries to about 1 GiB."""
    import torch
    G, bb = data.shape[0], data.shape[2]
    step = max(1, (1 << 30) // (k * bb))
    for a in range(0, G, step):
        b = min(G, a + step)
        mask = rows_in[a:b] >= k
        ro = rows_out[a:b].long()
        assert bool((ro[mask] < k).all()), (what, a)
        gi = torch.arange(a, b, device="cuda")[:, None].expand(b - a, k)
        assert torch.equal(got[a:b][mask], data[gi[mask], ro[mask]]), (what, a)
        if what == "inplace":       # the other slots still hold the blocks they were given
            keep = ~mask
            assert torch.equal(got[a:b][keep], data[gi[keep], ro[keep]]), (what, a)
        elif what == "outofplace":  # the other slots were not written
            assert bool((got[a:b][~mask] == FILL).all()), (what, a)


@pytest.mark.parametrize("case", DENSE, ids=[c[0] for c in DENSE])
def test_dense_batch_past_4gib(tuned_engine, oracle, case):  # noqa: F811
    """One uniform batch per kernel family whose data / blocks (and `out`, parity or rec, as the
    shape gives) pass 2^32 bytes: encode, lose r blocks per group, decode in the layouts named.
    Batch-wide on the device: status 0, every recovered block equals its original, untouched
    slots keep their bytes, the m = 1 parity is the XOR of the data.  Byte-exact against the
    oracle on the groups around byte 2^31 and 2^32 of every buffer and on the aliases of the
    last groups (boundary_samples): where a truncated load or store would show."""
    import torch
    name, k, m, bb, nblk, enc_kernel, dec_kernel, layouts, opts = case
    engine = tuned_engine
    for opt, v in opts.items():
        engine.set_option(opt, v)
    G = dense_groups(nblk, bb)
    rmax = min(k, m)
    r = max(1, rmax // 2)
    assert (G - 2) * nblk * bb >= B32 > (G - 3) * nblk * bb
    data = torch.empty((G, k, bb), dtype=torch.uint8, device="cuda")
    fec.synth_fill(data, seed=4100 + k + m)
    parity = torch.full((G, m, bb), FILL, dtype=torch.uint8, device="cuda")
    assert engine.encode(k, m, bb, data, parity) == 0
    assert enc_kernel in fec.last_kernels(), fec.last_kernels()
    if m == 1:
        acc = data[:, 0].clone()
        for x in range(1, k):
            acc ^= data[:, x]
        assert torch.equal(parity[:, 0], acc)
        del acc
    rows, src = synth.loss_patterns(k, m, r, G, 4200 + k, shuffle=True)
    rows_d = dev(rows)
    blocks = torch.empty((G, k, bb), dtype=torch.uint8, device="cuda")
    fec.synth_gather(data, parity, dev(src), blocks, k, m, bb)

    group_bytes = [k * bb, m * bb] + ([rmax * bb] if "recovered" in layouts else [])
    sample = boundary_samples(G, group_bytes)
    assert {0, 1, G - 2, G - 1, B31 // (k * bb), B32 // (k * bb)} <= set(sample)
    sample_d = torch.tensor(sample, device="cuda")
    d_np = host(data[sample_d])
    np.testing.assert_array_equal(
        d_np[-1].ravel(), synth.stream_bytes(4100 + k + m, (G - 1) * k * bb, k * bb))
    p_or, _ = oracle.encode_batch(k, m, bb, d_np)
    np.testing.assert_array_equal(host(parity[sample_d]), p_or)
    recv = synth.assemble_received(d_np, p_or, src[sample])
    np.testing.assert_array_equal(host(blocks[sample_d]), recv)
    b_or, r_or, s_or = oracle.decode_batch(k, m, bb, recv, rows[sample])
    assert (s_or == 0).all()
    slot_mask = rows[sample] >= k

    for layout in layouts:                       # in place last: it overwrites the blocks
        st = torch.full((G,), 9, dtype=torch.int32, device="cuda")
        if layout == "recovered":
            rec = torch.full((G, rmax, bb), FILL, dtype=torch.uint8, device="cuda")
            rr = torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda")
            engine.decode_recovered(k, m, bb, blocks, rows_d, rec, rr, status=st)
            kern = fec.last_kernels()
            got = rr != 255
            assert bool((got.sum(dim=1) == r).all())
            step = max(1, (1 << 30) // (rmax * bb))
            for a in range(0, G, step):
                b = min(G, a + step)
                gi = torch.arange(a, b, device="cuda")[:, None].expand(b - a, rmax)[got[a:b]]
                assert torch.equal(rec[a:b][got[a:b]], data[gi, rr[a:b].long()[got[a:b]]]), a
            exp, exp_rows = expected_recovered(k, m, bb, rows[sample], b_or, r_or, s_or)
            np.testing.assert_array_equal(host(rr[sample_d]), exp_rows)
            np.testing.assert_array_equal(host(rec[sample_d])[exp_rows != 255],
                                          exp[exp_rows != 255])
            del rec, rr
        elif layout == "outofplace":
            out = torch.full((G, k, bb), FILL, dtype=torch.uint8, device="cuda")
            ro = torch.full((G, k), 9, dtype=torch.uint8, device="cuda")
            engine.decode(k, m, bb, blocks, rows_d, out=out, rows_out=ro, status=st)
            kern = fec.last_kernels()
            recovered_equal_originals(out, rows_d, ro, data, k, layout)
            np.testing.assert_array_equal(host(ro[sample_d]), r_or)
            o = host(out[sample_d])
            np.testing.assert_array_equal(o[slot_mask], b_or[slot_mask])
            assert (o[~slot_mask] == FILL).all()
            del out, ro
        else:
            rio = rows_d.clone()
            engine.decode(k, m, bb, blocks, rio, status=st)
            kern = fec.last_kernels()
            recovered_equal_originals(blocks, rows_d, rio, data, k, layout)
            np.testing.assert_array_equal(host(rio[sample_d]), r_or)
            np.testing.assert_array_equal(host(blocks[sample_d]), b_or)
        assert dec_kernel in kern, (layout, kern)
        assert int(st.abs().max()) == 0, layout
        if layout != "inplace":                  # the inputs are read only
            np.testing.assert_array_equal(host(blocks[sample_d]), recv)
            assert torch.equal(rows_d, dev(rows))
    del data, parity, blocks
    torch.cuda.empty_cache()
