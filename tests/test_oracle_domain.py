"""The CPU oracle against the reference codec over the whole (k, m) domain.

Every GPU test compares with oracle/fec_oracle.c, so the oracle itself is pinned here at every
code the library accepts: the 32,640 legal pairs (k >= 1, m >= 1, k + m <= 256) and the band
(k, 257 - k), k = 2..255, where an encode writes the XOR parity and returns -1 and a decode
that holds a recovery block returns -1.  tests/golden/ref_domain.json holds what the compiled
reference produced (tests/golden/gen_ref_domain.py), folded into one SHA-256 per m and one per
k; this module recomputes the folds with the oracle alone.  Where oracle/_ref is built, a fold
that differs is followed up array against array and the first differing (k, m) is named.

Per pair: 8-byte blocks, 2 groups.  The data of every pair of one m is one seeded stream
(seed 77000 + m): pair k takes bytes [8 k (k - 1), 8 k (k + 1)), which is
synth.group_data(77000 + m, k, 8, 2, first_group=k - 1).  Group 0 loses r = min(k, m, 256 - k)
data rows (256 - k: a row tag is one byte, so in the band the last parity row cannot arrive),
group 1 loses r // 2; both receive a random r-subset of the parity rows in shuffled arrival
order, drawn from numpy's default_rng([k, m]).
"""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from quic_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_domain.json")
BB, GROUPS, SEED = 8, 2, 77000
M_ALL = range(1, 256)
M_RANGES = [(a, min(a + 15, 255)) for a in range(1, 256, 16)]


def ks_of(m):
    """The k of every pair of this m, ascending: the legal ones, then the band's."""
    return list(range(1, 257 - m)) + ([257 - m] if 2 <= m <= 255 else [])


def ms_of(k):
    return list(range(1, 257 - k)) + ([257 - k] if 2 <= k <= 255 else [])


def stream_of(m):
    """The data of every pair of m, in one call."""
    kmax = ks_of(m)[-1]
    return synth.stream_bytes(SEED + m, 0, BB * kmax * (kmax + 1))


def pair_inputs(k, m, stream=None):
    """(data [2][k][8], rows [2][k] uint8) of one pair."""
    if stream is None:
        data = synth.group_data(SEED + m, k, BB, GROUPS, first_group=k - 1)
    else:
        data = stream[BB * k * (k - 1):BB * k * (k + 1)].reshape(GROUPS, k, BB)
    rng = np.random.default_rng([k, m])
    r = min(k, m, 256 - k)
    rows = np.empty((GROUPS, k), np.uint8)
    for g, lost in enumerate((r, r // 2)):
        keep = np.sort(rng.permutation(k)[lost:])
        par = np.sort(rng.permutation(min(m, 256 - k))[:lost]) + k
        rows[g] = np.concatenate([keep, par])[rng.permutation(k)]
    return data, rows


def run_pair(O, k, m, data, rows, use_ref=False):
    """(encode rc, parity, decode status, rows_out, decoded blocks) from one codec."""
    par, rc = O.encode_batch(k, m, BB, data, use_ref=use_ref)
    recv = synth.assemble_received(data, par, rows.astype(np.int16))
    blocks, rows_out, status = O.decode_batch(k, m, BB, recv, rows, use_ref=use_ref)
    return np.int32(rc), par, status.astype(np.int32), rows_out, blocks


def pair_digest(result):
    h = hashlib.sha256()
    for a in result:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.digest()


_digests = {}          # (m, codec) -> {k: digest}, computed once
_pool = None


def digests_of(O, m, use_ref=False):
    """The digest of every pair of m.  Nearly all of the sweep's time is the oracle's own
    arithmetic (190 s on one core against 2 s of numpy), and its calls release the
    interpreter lock and share only read-only tables, so the pairs of one m run on up to 8
    threads.  The reference keeps to one thread."""
    global _pool
    key = (m, use_ref)
    if key not in _digests:
        stream = stream_of(m)

        def one(k):
            return pair_digest(run_pair(O, k, m, *pair_inputs(k, m, stream), use_ref))
        ks = ks_of(m)
        if use_ref:
            ds = [one(k) for k in ks]
        else:
            if _pool is None:
                _pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
            ds = list(_pool.map(one, ks[::-1]))[::-1]     # the long pairs (large k) first
        _digests[key] = dict(zip(ks, ds))
    return _digests[key]


def fold_m(O, m, use_ref=False):
    d = digests_of(O, m, use_ref)
    return hashlib.sha256(b"".join(d[k] for k in ks_of(m))).hexdigest()


def fold_k(O, k, use_ref=False):
    return hashlib.sha256(b"".join(digests_of(O, m, use_ref)[k] for m in ms_of(k))).hexdigest()


def first_difference(O, pairs):
    """Array against array with the compiled reference: the first pair that differs."""
    names = ("encode rc", "parity", "status", "rows_out", "blocks")
    for k, m in pairs:
        data, rows = pair_inputs(k, m)
        got, ref = run_pair(O, k, m, data, rows), run_pair(O, k, m, data, rows, use_ref=True)
        for name, a, b in zip(names, got, ref):
            if not np.array_equal(a, b):
                return f"first difference from the reference at (k={k}, m={m}): {name}"
    return "the oracle equals the compiled reference here: ref_domain.json is stale"


def explain(O, pairs):
    if not O.ref_available():
        return "oracle/_ref is not built: no array comparison"
    return first_difference(O, pairs)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_domain_size(recorded):
    assert sum(len(ks_of(m)) for m in M_ALL) == 32640 + 254
    assert sum(len(ms_of(k)) for k in M_ALL) == 32640 + 254
    assert {(k, m) for m in M_ALL for k in ks_of(m)} == {(k, m) for k in M_ALL for m in ms_of(k)}
    assert recorded["pairs"] == 32640 + 254
    assert (recorded["block_bytes"], recorded["groups"], recorded["seed_base"]) == (BB, GROUPS, SEED)
    assert sorted(map(int, recorded["by_m"])) == list(M_ALL)
    assert sorted(map(int, recorded["by_k"])) == list(M_ALL)


@pytest.mark.parametrize("m_lo,m_hi", M_RANGES, ids=[f"m{a}-{b}" for a, b in M_RANGES])
def test_oracle_folds_by_m(oracle, recorded, m_lo, m_hi):
    """Every pair of every m in the range: the fold over ascending k is the reference's."""
    for m in range(m_lo, m_hi + 1):
        if fold_m(oracle, m) != recorded["by_m"][str(m)]:
            pytest.fail(f"m = {m}: the oracle's fold over k = {ks_of(m)[0]}..{ks_of(m)[-1]} is not "
                        f"the recorded one; " + explain(oracle, [(k, m) for k in ks_of(m)]))


def test_oracle_folds_by_k(oracle, recorded):
    """The same pair digests folded per k over ascending m: with the per-m folds, a mismatch
    localises to a row/column crossing.  Covers all 32,894 pairs whatever ran before."""
    assert sum(len(digests_of(oracle, m)) for m in M_ALL) == 32640 + 254
    bad = [k for k in M_ALL if fold_k(oracle, k) != recorded["by_k"][str(k)]]
    if bad:
        k = bad[0]
        pytest.fail(f"k = {bad}: the oracle's fold over m is not the recorded one; " +
                    explain(oracle, [(k, m) for m in ms_of(k)]))
