"""xor_dma_kernel (m = 1, the headline path) with many groups per wave: every ring shape
xor_slots x xor_waves the library accepts, at group sizes from one DMA instruction to the
largest xor_plan admits, on a grid of ONE workgroup, so a wave streams up to 61 groups back to
back.  Only then do the counted wait WAIT = (NSLOT - 1) * (NDMA + R) and the slot rotation
ua = (u + NSLOT - 1) % NSLOT run: on the default grid every wave of a small batch gets one
group and the loop body that issues group i + NSLOT - 1 before waiting for group i is never
reached.  Encode, both slot-layout decodes and the recovered-blocks decode, guarded buffers,
bit-exact against the CPU oracle.  Run with -m gpu."""
import numpy as np
import pytest

from quic_amd import fec, synth
from tests.test_gpu_parity import check_decodes, gpu_encode, tuned_engine  # noqa: F401

# (k, bb) at m = 1 -> NDMA = ceil(k * bb / 1024) DMA instructions per group
SHAPES = [
    (2, 8),        # NDMA 1, one 16-byte group: every lane's piece is clamped to offset 0
    (6, 8),        # NDMA 1; the tag address g * 6 takes every phase mod 4
    (64, 8),       # NDMA 1; all 64 lanes hold a row tag
    (4, 1352),     # NDMA 6
    (10, 1352),    # NDMA 14 (workload A)
    (16, 1280),    # NDMA 20: 20,480 B, the largest group xor_plan admits
    (65, 16),      # NDMA 2; k > 64: m1_prep_kernel + the eidx variant
    (255, 64),     # NDMA 16; k > 64
]
SLOTS = [2, 3, 4]
WAVES = [1, 2, 3, 4]
# 61: with 4 waves each wave streams 15 or 16 groups (steady state and drain for NSLOT = 4);
# 5: some waves hold 2 groups, some 1, fewer than there are slots (prologue and tail only); 1
GROUPS = [61, 5, 1]
ROWS_OFFSETS = [0, 1, 3]      # the dword-granular tag DMA and its `& 3` re-alignment
KINDS = ["none", "lose_first", "none_shuffled", "lose_last", "lose_random",
         "lose_first_shuffled", "lose_last_shuffled", "lose_random_shuffled"]
KIND_SEED = 3


def ndma_of(k, bb):
    return (k * bb + 1023) // 1024


def plan_fits(k, bb, slots, waves):
    """xor_plan's conditions (quic_amd/csrc/xor_dma.hip), restated: the group is whole 16-byte
    units of 8-byte blocks in at most 20 DMA instructions; the ring (per wave and slot NDMA KiB
    of data and an 80-byte tag window, plus 64 flag bytes per wave) fits 160 KiB of LDS; the
    groups in flight fit the 6-bit vmcnt."""
    gb = k * bb
    if bb % 8 or gb % 16 or gb < 16:
        return False
    ndma = ndma_of(k, bb)
    lds = waves * slots * (ndma * 1024 + 80) + waves * 64
    return lds <= 160 * 1024 and (slots - 1) * (ndma + 1) <= 63 and ndma <= 20


def call_uses_dma(kind, k, fits):
    """Which calls of a fitting plan run xor_dma_kernel: the encode and the slot-layout decode
    for any k (k > 64 reads eidx), the recovered-blocks decode only fused (k <= 64; for k > 64
    the library writes the recovered layout with xor_flat_kernel)."""
    return fits and (kind != "decode_recovered" or k <= 64)


def kinds_for(G):
    """The receive-set kind of every group: drawn, not cycled, so no wave's stride (1 .. 4
    waves) sees a fixed period of them; half of the groups lost nothing."""
    rng = np.random.default_rng(KIND_SEED + G)
    if G == 1:
        return ["lose_random_shuffled"]
    none = [kd for kd in KINDS if kd.startswith("none")]
    lose = [kd for kd in KINDS if kd.startswith("lose")]
    kinds = [str(rng.choice(none if rng.random() < 0.5 else lose)) for _ in range(G)]
    kinds[:min(G, len(KINDS))] = rng.permutation(KINDS)[:min(G, len(KINDS))].tolist()
    return kinds


def receive_rows(rng, k, kind):
    rows = np.arange(k)
    if kind.startswith("lose"):
        lost = {"first": 0, "last": k - 1, "random": int(rng.integers(k))}[kind.split("_")[1]]
        rows[lost] = k                     # the parity block in the lost row's slot
    if kind.endswith("shuffled"):
        rows = rows[rng.permutation(k)]
    return rows


_CASES = {}


def ring_case(O, k, bb, G):
    """(data, parity, recv, rows) of one batch; computed once, read-only."""
    key = (k, bb, G)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * k + bb + G)
        data = synth.group_data(7000 + k + bb + G, k, bb, G)
        p_or, rc = O.encode_batch(k, 1, bb, data)
        assert rc == 0
        rows = np.stack([receive_rows(rng, k, kd) for kd in kinds_for(G)])
        recv = synth.assemble_received(data, p_or, rows.astype(np.int16))
        _CASES[key] = (data, p_or, recv, rows.astype(np.uint8))
    return _CASES[key]


def test_sweep_fit_count():
    """How many (shape, slots, waves) combinations of the sweep run xor_dma_kernel: a literal,
    so an edit cannot silently turn the sweep into fallbacks.  NDMA 1, 1, 1, 2 and 6 fit every
    ring; NDMA 14 up to 11 wave-slots, NDMA 16 up to 9, NDMA 20 up to 7 (LDS); the vmcnt
    bound (NSLOT - 1) * (NDMA + 1) <= 63 is met with equality by 4 slots at NDMA 20."""
    fit = {(k, bb): sum(plan_fits(k, bb, s, w) for s in SLOTS for w in WAVES) for k, bb in SHAPES}
    assert [ndma_of(k, bb) for k, bb in SHAPES] == [1, 1, 1, 6, 14, 20, 2, 16]
    assert list(fit.values()) == [12, 12, 12, 12, 9, 6, 12, 9]
    assert sum(fit.values()) == 84
    assert not plan_fits(16, 1280, 4, 2) and plan_fits(16, 1280, 4, 1)     # LDS; vmcnt 63
    assert not plan_fits(17, 1280, 2, 1)                                   # NDMA 21


def test_receive_sets_alternate():
    """In the 61-group batch every wave's stream (1 .. 4 waves: groups w, w + W, ...) goes from
    a group with nothing to write to a writing one and back, and every kind occurs."""
    kinds = kinds_for(61)
    assert set(kinds) == set(KINDS)
    writes = [kd.startswith("lose") for kd in kinds]
    for W in WAVES:
        for w in range(W):
            s = writes[w::W]
            steps = set(zip(s, s[1:]))
            assert (False, True) in steps and (True, False) in steps, (W, w)
    assert len(kinds_for(5)) == 5 and not all(kd.startswith("lose") for kd in kinds_for(5))


class Recording:
    """The engine, noting what every call launched."""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def _call(self, kind, *a, **kw):
        rc = getattr(self.eng, kind)(*a, **kw)
        self.calls.append((kind, fec.last_kernels(), fec.last_grids()))
        return rc

    def encode(self, *a, **kw):
        return self._call("encode", *a, **kw)

    def decode(self, *a, **kw):
        return self._call("decode", *a, **kw)

    def decode_recovered(self, *a, **kw):
        return self._call("decode_recovered", *a, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("k,bb", SHAPES)
def test_xor_ring_many_groups_per_wave(tuned_engine, oracle, k, bb, slots):  # noqa: F811
    """One workgroup of 1 .. 4 waves streams 61, 5 and 1 groups through a ring of `slots` slots:
    encode, the slot-layout decode in and out of place and the recovered-blocks decode, with the
    row tags at byte phases 0, 1 and 3, every buffer between guards, against the oracle.  Every
    call must have run xor_dma_kernel exactly when its plan fits (a plan that does not fit gives
    the same bytes through the fallback), on a grid of 1."""
    engine = tuned_engine
    engine.set_option("xor_wg", 1 << 20)       # the grid cap becomes one workgroup
    engine.set_option("xor_slots", slots)
    for waves in WAVES:
        engine.set_option("xor_waves", waves)
        fits = plan_fits(k, bb, slots, waves)
        for G in GROUPS:
            data, p_or, recv, rows = ring_case(oracle, k, bb, G)
            rec = Recording(engine)
            p_gpu, rc = gpu_encode(rec, k, 1, bb, data)
            assert rc == 0
            np.testing.assert_array_equal(p_gpu, p_or)
            dec = "xor_dma_kernel<decode" if fits and k <= 64 else "m1_prep_kernel"
            for off in ROWS_OFFSETS:
                s_or = check_decodes(rec, oracle, k, 1, bb, recv, rows, dec, rows_offset=off)
                assert (s_or == 0).all()
            assert [c[0] for c in rec.calls] == ["encode"] + ["decode", "decode",
                                                              "decode_recovered"] * 3
            for kind, kernels, grids in rec.calls:
                what = (k, bb, slots, waves, G, kind, kernels, grids)
                dma = call_uses_dma(kind, k, fits)
                assert ("xor_dma_kernel" in kernels) == dma, what
                assert ("xor_dma_kernel" in grids) == dma, what
                if dma:
                    assert grids["xor_dma_kernel"] == 1, what
