"""The run-time kernels at the edges of the (k, m) domain, bit-exact against the CPU oracle.

The library serves every code with 1 <= k <= 255 and k + m <= 256 through gf_stream, gf_apply,
gf_ragged and the three general decode preps; m > 1 with k + m > 256 answers -1.  The shapes
here are the smallest that reach each threshold of that dispatch: the prep selection (k <= 64,
k % 4, rmax <= 4, rmax <= 16), the encode chunking (4 / 8 / 16 outputs, then chunks of 8 past
m = 16), the decode chunking, row tags up to 255 at k + m = 256, and the launch shapes of
decode_prep_kernel that hold 2 or 1 groups per workgroup.  Every output sits between guard
bytes.  Run with -m gpu."""
import numpy as np
import pytest

from quic_amd import fec, synth
from tests import test_gpu_ragged as RG
from tests.test_gpu_parity import check_decodes, gpu_encode, parity_written
from tests.test_gpu_parity import tuned_engine  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 68, 127, 128, 129, 200, 254, 255]
MS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 64]


def ms_of(k, band=True):
    """The m of one k: the thresholds that are legal, the largest legal m (row tags up to 255)
    and, with `band`, the first m past it (k + m = 257: -1)."""
    ms = {m for m in MS if m <= 256 - k} | {256 - k}
    if band and 257 - k > 1:
        ms.add(257 - k)
    return sorted(ms)


GRID = [(k, m) for k in KS for m in ms_of(k)]
assert len(GRID) == 422, len(GRID)         # a literal: an edit cannot silently drop shapes
assert sum(k + m == 257 for k, m in GRID) == 24 and sum(k + m == 256 for k, m in GRID) == 24

CORNER_KM = [2, 9, 17, 64, 65, 128]
CORNERS = [(k, m) for k in CORNER_KM for m in CORNER_KM if k + m <= 256] + \
    [(254, 2), (2, 254), (200, 56)]
assert len(CORNERS) == 39, len(CORNERS)
CORNER_KS = sorted({k for k, _ in CORNERS})


def receive_sets(k, m):
    """Row tags [6][k] of hand-built receive sets: no loss; the last data row lost, the last
    parity row in its place; rmax losses standing on the last rmax parity rows; rmax losses on
    the first parity rows in descending arrival; two sets with a random loss count in
    [0, rmax]; the odd sets in shuffled arrival order.  A row tag is one byte, so at
    k + m = 257 the last parity row cannot arrive: the sets use the first 256 - k."""
    mp = min(m, 256 - k)
    rmax = min(k, mp)
    rng = np.random.default_rng(1000 * k + m)

    def lose(lost, par):
        keep = [x for x in range(k) if x not in set(lost)]
        return keep + [k + y for y in par]
    sets = [
        list(range(k)),
        lose([k - 1], [mp - 1]),
        lose(range(k - rmax, k), range(mp - rmax, mp)),
        lose(range(rmax), range(rmax - 1, -1, -1)),
    ]
    for _ in range(2):
        r = int(rng.integers(0, rmax + 1))
        sets.append(lose(sorted(rng.choice(k, r, replace=False)),
                         sorted(rng.choice(mp, r, replace=False))))
    rows = np.array(sets, np.uint8)
    for g in range(1, len(rows), 2):
        rows[g] = rows[g][rng.permutation(k)]
    return rows


_refs = {}


def reference(oracle, k, m, bb, pick=None):
    """One shape's data, the oracle's parity and the received blocks of its receive sets
    (the sets `pick`, or all six), built once (read-only)."""
    key = (k, m, bb, pick)
    if key not in _refs:
        rows = receive_sets(k, m)
        if pick is not None:
            rows = rows[list(pick)]
        data = synth.group_data(6100 + 3 * k + m, k, bb, len(rows))
        p_or, rc_or = oracle.encode_batch(k, m, bb, data)
        assert rc_or == (-1 if (k > 1 and m > 1 and k + m > 256) else 0)
        recv = synth.assemble_received(data, p_or, rows.astype(np.int16))
        for a in (data, p_or, rows, recv):
            a.setflags(write=False)
        _refs[key] = (data, p_or, rc_or, rows, recv)
    return _refs[key]


def run_shape(engine, oracle, k, m, bb, enc_kernel, dec_kernel, never=None, pick=None):
    """Encode and every decode layout of one shape against the oracle.  enc_kernel /
    dec_kernel: what a legal code with k > 1 and m > 1 must launch (the others run the XOR and
    k = 1 kernels, and k + m > 256 only writes the XOR parity and the status)."""
    data, p_or, rc_or, rows, recv = reference(oracle, k, m, bb, pick)
    general = k > 1 and m > 1 and k + m <= 256
    p_gpu, rc = gpu_encode(engine, k, m, bb, data)
    kernels = fec.last_kernels()
    assert rc == rc_or, (k, m)
    np.testing.assert_array_equal(p_gpu, parity_written(p_or, rc_or), err_msg=f"k={k} m={m}")
    if general:
        assert enc_kernel in kernels, (k, m, kernels)
    assert never is None or never not in kernels, (k, m, kernels)
    s_or = check_decodes(engine, oracle, k, m, bb, recv, rows, dec_kernel if general else "")
    assert never is None or never not in fec.last_kernels(), (k, m, fec.last_kernels())
    lossy = (rows >= k).any(axis=1)
    if k > 1 and m > 1 and k + m > 256:
        assert s_or.tolist() == [-1 if x else 0 for x in lossy], (k, m)
    else:
        assert (s_or == 0).all(), (k, m)


# ------------------------------------------------------------------ B.2: the paths
@pytest.mark.parametrize("k", KS)
def test_stream(engine, oracle, k):
    """gf_stream, default options, 24-byte blocks: three 8-byte sub-rows, and with odd k every
    other group starts 8 bytes off a 16-byte boundary.  Never gf_apply."""
    for m in ms_of(k):
        run_shape(engine, oracle, k, m, 24, "gf_stream_kernel<encode", "gf_stream_kernel<decode",
                  never="gf_apply")


@pytest.mark.parametrize("k", KS)
def test_apply_small(tuned_engine, oracle, k):  # noqa: F811
    """The same shapes through gf_apply (stream = 0)."""
    tuned_engine.set_option("stream", 0)
    for m in ms_of(k):
        run_shape(tuned_engine, oracle, k, m, 24, "gf_apply_kernel<encode",
                  "gf_apply_kernel<decode", never="gf_stream")


@pytest.mark.parametrize("k", CORNER_KS)
def test_apply_2056(engine, oracle, k):
    """Default options at the first block size past gf_stream's 2048 bytes: gf_apply with 257
    words per sub-row (a second tile with one live lane), 3 groups."""
    for m in [m for kk, m in CORNERS if kk == k]:
        run_shape(engine, oracle, k, m, 2056, "gf_apply_kernel<encode", "gf_apply_kernel<decode",
                  never="gf_stream", pick=(1, 2, 3))


RAGGED_SIZES = [8, 24, 40, 104, 16, 2056]


@pytest.mark.parametrize("k", KS)
def test_ragged(engine, oracle, k):
    """encode_ragged / decode_ragged_recovered with six block sizes in one launch, every kind
    of receive set; the kinds rotate with k + m, so every size meets every kind over the grid.
    The poison checks are those of tests/test_gpu_ragged.py."""
    for m in ms_of(k, band=False):
        s = (k + m) % len(RG.KINDS)
        c = RG.build_case(oracle, k, m, RAGGED_SIZES, RG.KINDS[s:] + RG.KINDS[:s], seed=31 * k + m)
        out = RG.run_device(engine, c)
        assert out["enc_rc"] == 0, (k, m)
        assert (c["enc_status"] == 0).all() and (c["dec_status"] == 0).sum() >= 5
        try:
            RG.check(c, out)
        except AssertionError as e:
            raise AssertionError(f"k={k} m={m}: {e}") from None


@pytest.mark.parametrize("k", CORNER_KS)
def test_dropin(oracle, k):
    """cauchy_256_encode / cauchy_256_decode, the reference's own call surface: one group of
    24-byte blocks per call, a full-loss and a one-loss receive set."""
    assert fec.cauchy_256_init() == 0
    bb = 24
    for m in [m for kk, m in CORNERS if kk == k]:
        data, p_or, rc_or, rows, recv = reference(oracle, k, m, bb)
        par = np.full(m * bb, 0x5A, np.uint8)
        assert fec.cauchy_256_encode(k, m, list(data[0]), par, bb) == rc_or == 0
        np.testing.assert_array_equal(par.reshape(m, bb), p_or[0], err_msg=f"k={k} m={m}")
        for g in (1, 3):
            blocks = [b.copy() for b in recv[g]]
            exp, exp_rows, exp_rc = oracle.decode_blocks(k, m, bb, blocks, rows[g])
            blk = fec.make_blocks(blocks, rows[g])
            assert fec.cauchy_256_decode(k, m, blk, bb) == exp_rc == 0
            assert [blk[i].row for i in range(k)] == exp_rows, (k, m, g)
            np.testing.assert_array_equal(np.stack(blocks), np.stack(exp), err_msg=f"k={k} m={m}")
            for i in range(k):                   # and the blocks are the data
                np.testing.assert_array_equal(blocks[i], data[g][blk[i].row])


# ------------------------------------------------------------------ B.3: prep selection
# Recorded strings, read off launch_decode_prep: the lane prep needs rmax <= 4, k <= 64 and
# k % 4 == 0; the wide prep k <= 64 and rmax <= 16; decode_prep_kernel takes the rest.
PREP_AT = {
    (64, 4): "decode_prep_lane_kernel", (60, 3): "decode_prep_lane_kernel",
    (4, 4): "decode_prep_lane_kernel",
    (63, 4): "decode_prep_wide_kernel", (64, 5): "decode_prep_wide_kernel",
    (64, 16): "decode_prep_wide_kernel", (16, 64): "decode_prep_wide_kernel",
    (65, 4): "decode_prep_kernel", (68, 4): "decode_prep_kernel", (64, 17): "decode_prep_kernel",
    (65, 16): "decode_prep_kernel", (17, 17): "decode_prep_kernel",
}


@pytest.mark.parametrize("k,m", sorted(PREP_AT))
def test_prep_selection_boundaries(engine, oracle, k, m):
    """Each side of every threshold of the prep selection.  The receive sets lose data row
    k - 1 (set 1) and row 0 (set 3): bit k - 1 and bit 0 of the 64-bit presence mask."""
    rows = receive_sets(k, m)
    assert k - 1 not in rows[1] and 0 not in rows[3]
    prep = PREP_AT[(k, m)] + " + "
    data, p_or, rc_or, rows, recv = reference(oracle, k, m, 24)
    s_or = check_decodes(engine, oracle, k, m, 24, recv, rows, prep)
    print((k, m), fec.last_kernels())
    assert fec.last_kernels() == prep + "gf_stream_kernel<decode,s>"
    assert (s_or == 0).all()


# ------------------------------------------------------------------ B.4: large-r launches
# decode_prep_kernel's LDS is 768 + m k + nwv (1280 + 2 rmax^2) (each term rounded up to 16)
# for nwv groups per workgroup, halved from 4 until it fits 64 KiB: 4 up to r = 81 for
# k = m = r, 2 up to r = 111, then 1.  Workgroups for 8 groups:
PREP_GRID = {(81, 81): 2, (82, 82): 4, (111, 111): 4, (100, 156): 4, (156, 100): 4,
             (112, 112): 8, (127, 129): 8, (128, 128): 8}


def prep_groups_per_workgroup(k, m):
    def up16(v):
        return (v + 15) & ~15
    rmax = min(k, m)
    nwv = 4
    while nwv > 1 and 768 + up16(m * k) + nwv * up16(1280 + 2 * rmax * rmax) > 64 * 1024:
        nwv >>= 1
    return nwv


@pytest.mark.parametrize("bb", [8, 24])
@pytest.mark.parametrize("k,m", sorted(PREP_GRID))
def test_prep_large_r(engine, oracle, k, m, bb):
    """The 2-wave and 1-wave launches of decode_prep_kernel (up to 51,200 bytes of LDS, 16
    apply chunks per group): 8 groups with rmax, rmax - 1 and 1 losses."""
    G, rmax = 8, min(k, m)
    assert PREP_GRID[(k, m)] == G // prep_groups_per_workgroup(k, m)
    data = synth.group_data(7300 + k + m, k, bb, G)
    p_or, rc_or = oracle.encode_batch(k, m, bb, data)
    p_gpu, rc = gpu_encode(engine, k, m, bb, data)
    assert rc == rc_or == 0
    np.testing.assert_array_equal(p_gpu, p_or)
    for r in (rmax, rmax - 1, 1):
        rows, src = synth.loss_patterns(k, m, r, G, 17 + r + bb, shuffle=True)
        recv = synth.assemble_received(data, p_or, src)
        s_or = check_decodes(engine, oracle, k, m, bb, recv, rows,
                             "decode_prep_kernel + gf_stream_kernel<decode")
        assert (s_or == 0).all()
        print((k, m, bb, r), fec.last_grids())
        assert fec.last_grids()["decode_prep_kernel"] == PREP_GRID[(k, m)]
