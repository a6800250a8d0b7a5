"""GPU: the uniform entry points at misaligned pointers, every buffer between guard bytes.

include/quic_fec.h promises nothing about the alignment of d_data / d_blocks, d_parity / d_out /
d_rec or the row-tag arrays, and the library picks kernels and store variants from the low bits
of those pointers (fec_api.cpp encode_impl / decode_impl, xor_dma_ok, xor_unit, launch_gf_stream's
wide stores, launch_gf_psyn's wide stores, launch_decode_prep's lane kernel).  Each shape here
runs encode, both slot-layout decodes and decode_recovered at a set of (in, out, rows) byte
offsets past a 16-byte boundary.  Every buffer comes from tests/guarded.py: outputs start as the
fill byte, so bytes a call must not write are asserted to still hold it, and the guards on both
sides of every input and output are checked after every call.  Bit-exact against the CPU oracle.
The packet-protection calls run the same way at output bases 0, 4 and 12 with a row stride that
is 4 mod 16.  Run with -m gpu."""
import numpy as np
import pytest

from quic_amd import fec, synth
from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_parity import expected_recovered

pytestmark = pytest.mark.gpu

# (in, out, rows): offsets of data / blocks, of parity / out / rec, of rows_in and rows_out /
# rec_rows.  In place, out = in
TRIPLES = [(0, 0, 0), (0, 8, 0), (0, 4, 0), (0, 1, 1), (8, 0, 2), (8, 8, 3), (4, 12, 0),
           (1, 0, 1), (1, 1, 0), (0, 0, 1), (0, 0, 2)]

# (k, m, bb, G): the smallest shape of each rung of the dispatch
SHAPES = [
    (1, 3, 64, 5),                                                     # k <= 1
    (4, 1, 1352, 5), (4, 1, 100, 5), (3, 1, 7, 5), (3, 1, 3, 5),       # m = 1
    (10, 1, 1350, 5), (64, 1, 1352, 3),
    (32, 4, 1352, 5), (5, 5, 1352, 5), (10, 10, 1352, 5),              # compiled codes
    (10, 20, 1352, 5), (15, 15, 1352, 5), (128, 16, 9008, 2),
    (128, 16, 9008, 3),          # with 2 groups none is left that loses blocks and decodes
    (250, 5, 1352, 3), (12, 10, 1352, 5), (6, 3, 4096, 5),             # run-time codes
    (20, 12, 4096, 3), (9, 4, 40, 5),
    (4, 2, 100, 5), (250, 7, 16, 3),                                   # status -1
]

# the same cases with the wide stores switched the other way
OPTION_CASES = [
    ((5, 5, 1352, 5), {"ring_wide": 0}), ((15, 15, 1352, 5), {"psyn_wide": 2}),
    ((5, 5, 1352, 5), {"stream_static": 0}),
]
OPTION_TRIPLES = [(0, 4, 0), (0, 8, 0)]

# kernels that read their input through 16-byte LDS DMA: launched only for 16-byte aligned input
DMA_KERNELS = ("gf_ring", "gf_stream", "gf_dcol", "gf_bsyn", "gf_psyn", "xor_dma")


def dev(a):
    """A device copy (of a writable copy: the cached references are read-only)."""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def shape_id(s):
    return "k%dm%dbb%dg%d" % s


def triple_id(t):
    return "in%d-out%d-rows%d" % t


@pytest.fixture
def fresh_engine():
    """A fresh engine (own context) for the cases that change launch options."""
    eng = fec.FecEngine(0)
    yield eng
    eng.close()


_refs = {}


def reference(oracle, k, m, bb, G):
    """Inputs and expected results of one shape, computed once (read-only).  Group 0 has no
    loss; the last group of a supported m > 1 code names one parity row twice (status -3, left
    as it was: the reference's result for it is not defined, so the oracle decodes the other
    groups only)."""
    key = (k, m, bb, G)
    if key in _refs:
        return _refs[key]
    data = synth.group_data(7300 + 5 * k + m + bb, k, bb, G)
    p_or, rc_or = oracle.encode_batch(k, m, bb, data)
    rows, src = synth.loss_patterns(k, m, min(k, m), G, 17 + k + bb, shuffle=True)
    rows[0] = np.arange(k, dtype=rows.dtype)
    src[0] = np.arange(k, dtype=src.dtype)
    supported = k + m <= 256 and bb % 8 == 0
    malformed = k >= 2 and m >= 2 and supported
    if malformed:
        par = np.flatnonzero(rows[-1] >= k)
        assert par.size >= 2
        rows[-1, par[1]] = rows[-1, par[0]]
        src[-1, par[1]] = src[-1, par[0]]
    recv = synth.assemble_received(data, p_or, src)
    ok = np.ones(G, bool)
    ok[-1] = not malformed
    b_exp, r_exp = recv.copy(), rows.copy()
    s_exp = np.full(G, -3, np.int32)
    b_exp[ok], r_exp[ok], s_exp[ok] = oracle.decode_batch(k, m, bb, recv[ok], rows[ok])
    exp, exp_rows = expected_recovered(k, m, bb, rows, b_exp, r_exp, s_exp)
    if supported or m == 1 or k <= 1:
        assert s_exp[0] == 0 and (s_exp[1:G - 1] == 0).all()
    else:
        assert s_exp[0] == 0 and (s_exp[1:] == -1).all()
    par_exp = p_or
    if rc_or != 0:                       # -1: the XOR parity in block 0 and nothing else
        par_exp = np.full_like(p_or, FILL)
        par_exp[:, 0] = p_or[:, 0]
    _refs[key] = dict(data=data, par_exp=par_exp, rc=rc_or, rows=rows, recv=recv, b_exp=b_exp,
                      r_exp=r_exp, s_exp=s_exp, exp=exp, exp_rows=exp_rows)
    for v in _refs[key].values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _refs[key]


def status_buf(G):
    import torch
    st, h = guarded((G,), dtype=torch.int32)
    st.fill_(7)
    return st, h


def unchanged(pairs):
    """Inputs of a call that is not in place: payload and guards as they were."""
    for (h, a) in pairs:
        np.testing.assert_array_equal(h.host(), a)
        h.check_guards()


def run_plain(engine, ref, k, m, bb, G):
    """The four calls on tensors straight from the torch allocator: the kernels they launch."""
    import torch
    rmax = min(k, m)
    names = []
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")   # noqa: E731
    st = torch.zeros(G, dtype=torch.int32, device="cuda")
    engine.encode(k, m, bb, dev(ref["data"]), z(G, m, bb))
    names.append(fec.last_kernels())
    engine.decode(k, m, bb, dev(ref["recv"]), dev(ref["rows"]), status=st)
    names.append(fec.last_kernels())
    engine.decode(k, m, bb, dev(ref["recv"]), dev(ref["rows"]), out=z(G, k, bb),
                  rows_out=z(G, k), status=st)
    names.append(fec.last_kernels())
    engine.decode_recovered(k, m, bb, dev(ref["recv"]), dev(ref["rows"]), z(G, rmax, bb),
                            z(G, rmax), status=st)
    names.append(fec.last_kernels())
    torch.cuda.synchronize()
    return tuple(names)


def run_case(engine, oracle, shape, triple):
    """Encode, decode in place, decode out of place and decode_recovered at one offset triple;
    returns the kernels the four calls launched."""
    k, m, bb, G = shape
    o_in, o_out, o_rows = triple
    ref = reference(oracle, k, m, bb, G)
    rows, recv, s_exp = ref["rows"], ref["recv"], ref["s_exp"]
    rmax = min(k, m)
    failed = s_exp != 0
    names = []

    # ---- encode
    d, hd = guarded_from(ref["data"], o_in)
    p, hp = guarded((G, m, bb), o_out)
    rc = engine.encode(k, m, bb, d, p)
    names.append(fec.last_kernels())
    assert rc == ref["rc"]
    np.testing.assert_array_equal(hp.host(), ref["par_exp"])
    hp.check_guards()
    unchanged([(hd, ref["data"])])

    # ---- slot layout, in place
    b, hb = guarded_from(recv, o_in)
    r, hr = guarded_from(rows, o_rows)
    st, hst = status_buf(G)
    assert engine.decode(k, m, bb, b, r, status=st) == 0
    names.append(fec.last_kernels())
    np.testing.assert_array_equal(hst.host(), s_exp)
    np.testing.assert_array_equal(hr.host(), ref["r_exp"])
    np.testing.assert_array_equal(hb.host(), ref["b_exp"])
    for h in (hb, hr, hst):
        h.check_guards()

    # ---- slot layout, out of place: the recovered slots and nothing else
    b, hb = guarded_from(recv, o_in)
    r, hr = guarded_from(rows, o_rows)
    out, ho = guarded((G, k, bb), o_out)
    ro, hro = guarded((G, k), o_rows)
    st, hst = status_buf(G)
    assert engine.decode(k, m, bb, b, r, out=out, rows_out=ro, status=st) == 0
    names.append(fec.last_kernels())
    np.testing.assert_array_equal(hst.host(), s_exp)
    np.testing.assert_array_equal(hro.host(), ref["r_exp"])
    written = (ref["r_exp"] != rows) & (k > 1)     # k <= 1 only retags the block it was given
    assert not written[failed].any()
    got = ho.host()
    np.testing.assert_array_equal(got[written], ref["b_exp"][written])
    assert (got[~written] == FILL).all()
    for h in (ho, hro, hst):
        h.check_guards()
    unchanged([(hb, recv), (hr, rows)])

    # ---- recovered-blocks layout
    rec, hrec = guarded((G, rmax, bb), o_out)
    rr, hrr = guarded((G, rmax), o_rows)
    st, hst = status_buf(G)
    assert engine.decode_recovered(k, m, bb, b, r, rec, rr, status=st) == 0
    names.append(fec.last_kernels())
    np.testing.assert_array_equal(hst.host(), s_exp)
    np.testing.assert_array_equal(hrr.host(), ref["exp_rows"])   # 255 past the erasure count
    used = ref["exp_rows"] != 255
    got = hrec.host()
    np.testing.assert_array_equal(got[used], ref["exp"][used])
    assert (got[failed] == FILL).all()             # status -1 / -3: nothing recovered
    for h in (hrec, hrr, hst):
        h.check_guards()
    unchanged([(hb, recv), (hr, rows)])

    # ---- the gates did flip (the launchers' own checks)
    names = tuple(names)
    if o_in % 16:
        for n in names:
            assert not any(x in n for x in DMA_KERNELS), (n, triple)
    if m == 1 and o_out % 8:
        for n in (names[0], names[2], names[3]):   # in place, out = in
            assert "xor_dma" not in n, (n, triple)
    return names


@pytest.mark.parametrize("triple", TRIPLES, ids=triple_id)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_uniform_calls_at_offsets(engine, oracle, shape, triple):
    names = run_case(engine, oracle, shape, triple)
    print(shape_id(shape), triple_id(triple), names)
    if triple == (0, 0, 0):     # the guards do not change the path
        assert names == run_plain(engine, reference(oracle, *shape), *shape)


@pytest.mark.parametrize("triple", OPTION_TRIPLES, ids=triple_id)
@pytest.mark.parametrize("case", OPTION_CASES,
                         ids=lambda c: shape_id(c[0]) + "-" + ",".join(f"{o}={v}" for o, v in c[1].items()))
def test_uniform_calls_at_offsets_with_options(fresh_engine, oracle, case, triple):
    shape, opts = case
    for name, v in opts.items():
        fresh_engine.set_option(name, v)
    names = run_case(fresh_engine, oracle, shape, triple)
    print(shape_id(shape), opts, triple_id(triple), names)


# ------------------------------------------------------------------ packet protection
PP_SHAPES = [(10, 1, 1352, 7), (5, 5, 1352, 4)]
PP_OFFSETS = [0, 4, 12]
PP_STRIDE = 1380                 # 4 mod 16: successive rows take all four dword phases
EDGE_LENS = [0, 1, 15, 16, 17]


def rows_written(exp, nbytes):
    """Rows that started as the fill byte and whose first nbytes[i] bytes were written as exp."""
    col = np.arange(exp.shape[1])[None, :]
    return np.where(col < np.maximum(nbytes, 0)[:, None], exp, FILL).astype(np.uint8)


_pp = {}


def pp_case(oracle, k, m, bb, G, hdr_max):
    """A batch of G groups as packets p = g * (k + m) + i: data blocks (each its payload,
    zero-padded), parity, per-packet header and plaintext lengths that include 0, 1, 15, 16, 17
    and the whole block, headers in rows of 21 bytes (an odd stride), and the oracle's sealed
    packets in rows of 1380 bytes.  hdr_max 21: some packets do not fit their row."""
    key = (k, m, bb, G, hdr_max)
    if key in _pp:
        return _pp[key]
    rng = np.random.default_rng(31 * k + m + hdr_max)
    per, n = k + m, G * (k + m)
    pt_len = rng.integers(0, bb + 1, (G, per)).astype(np.int32)
    pt_len.reshape(n)[:12] = EDGE_LENS + [bb] + EDGE_LENS[::-1] + [bb]
    pt_len.reshape(n)[-3:] = bb
    pt_len[:, k:] = bb                   # an FEC packet carries its whole parity block
    data = rng.integers(0, 256, (G, k, bb), dtype=np.uint8)
    for g in range(G):
        for i in range(k):
            data[g, i, pt_len[g, i]:] = 0
    parity, rc = oracle.encode_batch(k, m, bb, data)
    assert rc == 0
    hdr = rng.integers(0, 256, (n, 21), dtype=np.uint8)
    hdr_len = rng.integers(0, hdr_max + 1, n).astype(np.int32)
    hdr_len[:12] = [16, 0, 1, 15, 17, 16, 0, 1, 15, 16, 17, 0]
    hdr_len[-3:] = [hdr_max, 16, hdr_max]
    hdr_len = np.minimum(hdr_len, hdr_max)
    rows_pt = np.concatenate([data, parity], axis=1).reshape(n, bb)
    pkt, plen = oracle.null_seal_batch(hdr, hdr_len, rows_pt, pt_len.reshape(n), PP_STRIDE)
    fits = hdr_len + 12 + pt_len.reshape(n) <= PP_STRIDE
    assert ((plen >= 0) == fits).all() and (fits.all() == (hdr_max <= 16))
    _pp[key] = dict(data=data, parity=parity, pt_len=pt_len.reshape(n), hdr=hdr, hdr_len=hdr_len,
                    rows_pt=rows_pt, pkt=pkt, plen=plen)
    return _pp[key]


@pytest.mark.parametrize("offset", PP_OFFSETS)
@pytest.mark.parametrize("shape", PP_SHAPES, ids=shape_id)
def test_null_seal_at_offsets(engine, oracle, shape, offset):
    """qfec_null_seal_batch: AD and plaintext rows at odd strides (21 and bb + 1), the output
    rows 1380 apart from a base 0, 4 or 12 past a 16-byte boundary.  A sealed row holds the
    oracle's bytes up to out_len and the fill byte after; a packet that does not fit leaves its
    row alone."""
    import torch
    k, m, bb, G = shape
    c = pp_case(oracle, k, m, bb, G, 21)
    n = G * (k + m)
    pt = np.zeros((n, bb + 1), np.uint8)
    pt[:, :bb] = c["rows_pt"]
    ad, had = guarded_from(c["hdr"], 1)
    d_pt, hpt = guarded_from(pt, 3)
    out, ho = guarded((n, PP_STRIDE), offset)
    out_len, hl = guarded((n,), dtype=torch.int32)
    engine.null_seal(ad, dev(c["hdr_len"]), d_pt, dev(c["pt_len"]), out, out_len)
    assert (c["plen"] < 0).sum() >= 2
    np.testing.assert_array_equal(hl.host(), c["plen"])
    np.testing.assert_array_equal(ho.host(), rows_written(c["pkt"], c["plen"]))
    for h in (ho, hl):
        h.check_guards()
    unchanged([(had, c["hdr"]), (hpt, pt)])


@pytest.mark.parametrize("offset", PP_OFFSETS)
@pytest.mark.parametrize("shape", PP_SHAPES, ids=shape_id)
def test_null_open_at_offsets(engine, oracle, shape, offset):
    """qfec_null_open_batch on sealed packets (some tampered, some cut short, some whose
    ciphertext exceeds the output row): the output row holds what the reference's output buffer
    holds -- the ciphertext copy, its start overwritten by the plaintext when accepted -- over
    the ciphertext's length, and the fill byte after; nothing where the ciphertext does not fit."""
    import torch
    k, m, bb, G = shape
    c = pp_case(oracle, k, m, bb, G, 21)
    n = G * (k + m)
    rng = np.random.default_rng(offset + k)
    pkt, ad_len = c["pkt"].copy(), c["hdr_len"]
    pkt_len = np.where(c["plen"] < 0, ad_len + 5, c["plen"]).astype(np.int32)   # 5 < 12: rejected
    for i in rng.choice(n, 5, replace=False):
        if pkt_len[i] > ad_len[i]:
            pkt[i, ad_len[i] + int(rng.integers(0, pkt_len[i] - ad_len[i]))] ^= 0x20
    o_stride = 1348              # 4 mod 16; ciphertexts of more than 1348 bytes do not fit
    exp, eres = oracle.null_open_batch(pkt, pkt_len, ad_len, o_stride)
    cl = pkt_len - ad_len
    copied = np.where(cl <= o_stride, cl, 0)
    assert (cl > o_stride).sum() >= 2 and (eres[cl > o_stride] == -1).all()
    assert (eres >= 0).sum() >= n // 4 and (eres < 0).sum() >= 5
    d_pkt, hp = guarded_from(pkt, offset)
    out, ho = guarded((n, o_stride), offset)
    out_len, hl = guarded((n,), dtype=torch.int32)
    engine.null_open(d_pkt, dev(pkt_len), dev(ad_len), out, out_len)
    np.testing.assert_array_equal(hl.host(), eres)
    np.testing.assert_array_equal(ho.host(), rows_written(exp, copied))
    for h in (ho, hl):
        h.check_guards()
    unchanged([(hp, pkt)])


@pytest.mark.parametrize("offset", PP_OFFSETS)
@pytest.mark.parametrize("shape", PP_SHAPES, ids=shape_id)
def test_seal_groups_at_offsets(engine, oracle, shape, offset):
    """qfec_seal_groups_batch: every data and FEC packet of each group, plaintext lengths from
    0 to the whole block; rows as in test_null_seal_at_offsets."""
    import torch
    k, m, bb, G = shape
    c = pp_case(oracle, k, m, bb, G, 21)
    n = G * (k + m)
    d, hd = guarded_from(c["data"])
    par, hpar = guarded_from(c["parity"])
    hdr, hh = guarded_from(c["hdr"], 1)
    pkt, hp = guarded((n, PP_STRIDE), offset)
    pkt_len, hl = guarded((n,), dtype=torch.int32)
    engine.seal_groups(k, m, bb, d, par, hdr, dev(c["hdr_len"]), dev(c["pt_len"]), pkt, pkt_len)
    assert (c["plen"] < 0).sum() >= 2
    np.testing.assert_array_equal(hl.host(), c["plen"])
    np.testing.assert_array_equal(hp.host(), rows_written(c["pkt"], c["plen"]))
    for h in (hp, hl):
        h.check_guards()
    unchanged([(hd, c["data"]), (hpar, c["parity"]), (hh, c["hdr"])])


@pytest.mark.parametrize("offset", PP_OFFSETS)
@pytest.mark.parametrize("shape", PP_SHAPES, ids=shape_id)
def test_open_decode_at_offsets(engine, oracle, shape, offset):
    """qfec_open_decode_batch with the wire packets 1380 apart from a base 0, 4 or 12 past a
    16-byte boundary: lost and tampered packets, one group that cannot be recovered.  Every
    filled slot of d_blocks is the plaintext zero-padded up to block_bytes (the header's words)
    and nothing beyond the slot is written; every output sits between guards."""
    import torch
    from tests.test_gpu_pp import _expected_open_decode
    k, m, bb, G = shape
    c = pp_case(oracle, k, m, bb, G, 16)
    per, n, rmax = k + m, G * (k + m), min(k, m)
    rng = np.random.default_rng(100 + offset + k)
    pkt, pkt_len, hdr_len = c["pkt"].copy(), c["plen"].copy(), c["hdr_len"]
    for g in range(1, G):                              # lose up to m packets of each group
        lost = rng.choice(per, int(rng.integers(1, m + 1)), replace=False)
        pkt_len[g * per + lost] = -1
    p = per + k - 1                                     # group 1: one more, rejected by its tag
    if pkt_len[p] < 0:
        pkt_len[p] = c["plen"][p]
    pkt[p, hdr_len[p] + 3] ^= 0x04
    pkt_len[0] = -1                                     # group 0: a data packet lost and
    pkt_len[k:per] = -1                                 # no FEC packet left to replace it
    open_len, blocks, rows, ok, rec, rec_rows, status = _expected_open_decode(
        oracle, k, m, bb, G, pkt, pkt_len, hdr_len)
    assert not ok[0] and status[0] == -3 and (status[ok] == 0).all() and open_len[p] == -1
    d_pkt, hp = guarded_from(pkt, offset)
    d_blocks, hb = guarded((G, k, bb))
    d_rows, hr = guarded((G, k))
    d_ol, hol = guarded((n,), dtype=torch.int32)
    d_rec, hrec = guarded((G, rmax, bb))
    d_rr, hrr = guarded((G, rmax))
    d_st, hst = guarded((G,), dtype=torch.int32)
    engine.open_decode(k, m, bb, d_pkt, dev(pkt_len), dev(hdr_len), d_blocks, d_rows, d_ol,
                       d_rec, d_rr, d_st)
    np.testing.assert_array_equal(hol.host(), open_len)
    np.testing.assert_array_equal(hr.host(), rows)
    filled = rows != 255
    np.testing.assert_array_equal(hb.host()[filled], blocks[filled])   # zero-padded up to bb
    np.testing.assert_array_equal(hst.host(), status)
    np.testing.assert_array_equal(hrr.host(), rec_rows)                 # all 255 where not ok
    used = rec_rows != 255
    np.testing.assert_array_equal(hrec.host()[used], rec[used])
    for g, j in zip(*np.nonzero(used)):
        np.testing.assert_array_equal(rec[g, j], c["data"][g, rec_rows[g, j]])
    for h in (hb, hr, hol, hrec, hrr, hst):
        h.check_guards()
    unchanged([(hp, pkt)])


# ------------------------------------------------------------------ ragged batches
@pytest.mark.parametrize("which", ["d_data", "d_parity", "d_blocks", "d_rec"])
def test_ragged_misaligned_base_refused(engine, which):
    """The ragged calls do state a requirement (include/quic_fec.h: the base pointers must be
    16-byte aligned): a base 8 past a 16-byte boundary is refused with -2 before anything is
    launched, and the poisoned outputs are untouched."""
    import torch
    k, m, G = 4, 2, 3
    bbs = np.array([1352, 40, 104], np.int32)
    d_off, p_off, r_off, totals = fec.ragged_layout(k, m, bbs)
    off = {w: 8 if w == which else 0 for w in ("d_data", "d_parity", "d_blocks", "d_rec")}
    rows, hrows = guarded_from(np.tile(np.array([0, 1, 4, 5], np.uint8), (G, 1)))
    st, hst = guarded((G,), dtype=torch.int32)
    if which in ("d_data", "d_parity"):
        a, ha = guarded((int(totals[0]),), off["d_data"])
        o, ho = guarded((int(totals[1]),), off["d_parity"])
        with pytest.raises(fec.FecError) as e:
            engine.encode_ragged(k, m, dev(bbs), a, dev(d_off), o, dev(p_off), status=st)
        outs = (ho, hst)
    else:
        a, ha = guarded((int(totals[0]),), off["d_blocks"])
        o, ho = guarded((int(totals[2]),), off["d_rec"])
        rr, hrr = guarded((G, 2))
        with pytest.raises(fec.FecError) as e:
            engine.decode_ragged_recovered(k, m, dev(bbs), a, dev(d_off), rows, o, dev(r_off), rr,
                                           status=st)
        outs = (ho, hrr, hst)
    assert e.value.rc == -2 and "16-byte aligned" in str(e.value)
    for h in outs:
        assert (h.host().view(np.uint8) == FILL).all()
    for h in outs + (ha, hrows):
        h.check_guards()
