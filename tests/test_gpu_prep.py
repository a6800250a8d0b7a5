"""Every decode prep kernel (quic_amd/csrc/decode_prep.hip) against the same receive sets.

The five preps state the reference's bookkeeping once, so each is pinned here on the sets the
others see: the valid ones bit-exact with the oracle in every layout, the malformed ones
against the contract of DESIGN.md section 3.6 (status -3, the group left as it was).  The
shapes are the smallest that reach each kernel: the compiled paths exist only at these block
sizes.  Run with -m gpu."""
import numpy as np
import pytest

from quic_amd import fec, synth
from tests.guarded import FILL, guarded, guarded_from
from tests.test_gpu_parity import check_decodes, dev, gpu_decode, host, status_buf
from tests.test_gpu_parity import tuned_engine  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GROUPS = 24

# ((k, m, bb), options, offset of the row tags past a 16-byte boundary, the prep that runs).
# The names end in " + ": the prep is followed by its apply kernel, and decode_prep_kernel is a
# prefix of decode_prep_kernel<syndrome>.
B, P, D = (32, 4, 1352), (10, 10, 1352), (128, 16, 9008)
VARIANTS = [
    (B, {}, 0, "decode_prep_bsyn_kernel + "),
    (B, {"bsyn": 0}, 0, "decode_prep_lane_kernel + "),
    (B, {"bsyn": 0, "prep_lane": 0}, 0, "decode_prep_kernel + "),
    (B, {"bsyn": 0}, 1, "decode_prep_wide_kernel + "),      # the lane kernel reads dwords
    (P, {}, 0, "decode_prep_psyn_kernel + "),
    (P, {"psyn": 0}, 0, "decode_prep_wide_kernel + "),
    (P, {"psyn": 0, "prep_lane": 0}, 0, "decode_prep_kernel + "),
    (D, {}, 0, "decode_prep_kernel<syndrome> + "),
    (D, {"dcol": 0}, 0, "decode_prep_kernel + "),
]


def variant_id(v):
    (k, m, bb), opts, off, prep = v
    return "-".join([f"k{k}m{m}"] + [f"{o}={x}" for o, x in opts.items()] +
                    ([f"rows+{off}"] if off else []) + [prep[len("decode_prep_"):-3]])


def receive_sets(k, m, groups=GROUPS):
    """(valid, malformed): row tags [n][k] of hand-built receive sets of a (k, m) code.  Valid:
    no loss; one loss at the first / last / a middle row with the first / last / a middle
    parity row; rmax losses, leading and trailing; parity rows in descending arrival order; a
    repeated data row; random losses up to `groups` sets; every odd set in shuffled arrival
    order.  Malformed: a repeated parity row (singular), a tag >= k + m, and for k > m more
    recovery tags than the code corrects."""
    rmax = min(k, m)
    rng = np.random.default_rng(1000 * k + m)

    def lose(lost, par):
        keep = [x for x in range(k) if x not in set(lost)]
        return keep + [k + y for y in par]
    sets = [
        list(range(k)),
        lose([0], [0]), lose([k - 1], [m - 1]), lose([k // 2], [m // 2]),
        lose([0], [m - 1]), lose([k - 1], [0]),
        lose(list(range(rmax)), list(range(rmax))),
        lose(list(range(k - rmax, k)), list(range(m - rmax, m))),
        lose([1, 4], [m - 1, 0]),                       # descending arrival
        lose(list(range(rmax)), list(range(m - 1, m - 1 - rmax, -1))),
    ]
    dup = list(range(k))                                # row 6 twice, row 5 missing, parity row 2
    dup[5] = 6
    dup[k - 3] = k + 2
    sets.append(dup)
    while len(sets) < groups:
        r = int(rng.integers(1, rmax + 1))
        sets.append(lose(sorted(rng.choice(k, r, replace=False)),
                         sorted(rng.choice(m, r, replace=False))))
    valid = np.array(sets, np.uint8)
    for g in range(1, groups, 2):
        valid[g] = valid[g][rng.permutation(k)]
    bad = [lose([2, 3], [1, 1]), lose([4], [0])]
    bad[1][-1] = k + m + 3
    if k > m:
        bad.append(lose(list(range(rmax + 1)), list(range(m)) + [0]))
    return valid, np.array(bad, np.uint8)


_refs = {}


def reference(oracle, k, m, bb):
    """The shape's receive sets and received blocks, built once (read-only)."""
    if (k, m, bb) not in _refs:
        valid, bad = receive_sets(k, m)
        rows = np.concatenate([valid, bad])
        data = synth.group_data(4200 + k + m, k, bb, len(rows))
        p_or, rc = oracle.encode_batch(k, m, bb, data)
        assert rc == 0
        # a tag >= k + m has no block of its own: any block stands in for it
        src = np.where(rows < k + m, rows, 0).astype(np.int16)
        recv = synth.assemble_received(data, p_or, src)
        for a in (rows, recv):
            a.setflags(write=False)
        _refs[(k, m, bb)] = (rows, recv, len(valid))
    return _refs[(k, m, bb)]


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
def test_prep_receive_sets(tuned_engine, oracle, variant):  # noqa: F811
    """One prep kernel on the shared receive sets.  Valid sets: status, rows_out, blocks in
    place and out of place, rec and rec_rows are the oracle's (check_decodes).  Malformed sets
    (the reference's behaviour is undefined there, so they are not given to the oracle):
    status -3, rows and blocks byte-identical to the input, nothing recovered in any layout,
    guards intact."""
    (k, m, bb), opts, off, prep = variant
    engine = tuned_engine
    for name, v in opts.items():
        engine.set_option(name, v)
    rows, recv, nv = reference(oracle, k, m, bb)
    s_or = check_decodes(engine, oracle, k, m, bb, recv[:nv], rows[:nv], prep, rows_offset=off)
    assert fec.last_kernels().startswith(prep), fec.last_kernels()
    assert (s_or == 0).all()

    brows, brecv = rows[nv:], recv[nv:]
    nb = len(brows)
    for inplace in (True, False):
        b, rr, st = gpu_decode(engine, k, m, bb, brecv, brows, inplace=inplace, rows_offset=off)
        assert fec.last_kernels().startswith(prep), fec.last_kernels()
        assert st.tolist() == [-3] * nb
        np.testing.assert_array_equal(rr, brows)
        if inplace:
            np.testing.assert_array_equal(b, brecv)
        else:                                           # no slot of `out` was written
            assert (b[brows >= k] == FILL).all()
    rmax = min(k, m)
    rec, hrec = guarded((nb, rmax, bb))
    rec_rows, hrr = guarded((nb, rmax))
    st, hst = status_buf(nb)
    d_recv = dev(brecv)
    engine.decode_recovered(k, m, bb, d_recv, guarded_from(brows, off)[0], rec, rec_rows,
                            status=st)
    assert fec.last_kernels().startswith(prep), fec.last_kernels()
    for h in (hrec, hrr, hst):
        h.check_guards()
    assert host(st).tolist() == [-3] * nb
    assert (host(rec_rows) == 255).all()
    assert (host(rec) == FILL).all()
    np.testing.assert_array_equal(host(d_recv), brecv)
