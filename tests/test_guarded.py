"""The guard helper of the GPU tests (tests/guarded.py) on the CPU: the layout it promises, and
that check_guards() does notice a byte written just outside the payload."""
import numpy as np
import pytest

from tests.guarded import FILL, GUARD, guarded, guarded_from


@pytest.mark.parametrize("offset", [0, 1, 4, 8, 12, 15])
def test_layout_and_untouched_buffer_passes(offset):
    v, h = guarded((3, 5, 7), offset=offset, device="cpu")
    assert v.shape == (3, 5, 7) and v.is_contiguous()
    assert v.data_ptr() % 16 == offset
    assert h.buf.data_ptr() % 16 == 0
    assert h.buf.numel() == GUARD + offset + 105 + GUARD
    assert (h.host() == FILL).all() and (h.buf.numpy() == FILL).all()
    h.check_guards()
    a = np.arange(105, dtype=np.uint8).reshape(3, 5, 7)
    h.load(a)
    assert np.array_equal(h.host(), a)
    v[2, 4, 6] = 9          # the payload's own last byte is not a guard
    v[0, 0, 0] = 9
    h.check_guards()
    assert (h.buf.numpy()[:h.lo] == FILL).all() and (h.buf.numpy()[h.hi:] == FILL).all()


@pytest.mark.parametrize("offset", [0, 1, 8])
def test_byte_before_payload_is_caught(offset):
    v, h = guarded((4, 6), offset=offset, device="cpu")
    h.buf[h.lo - 1] = 0
    with pytest.raises(AssertionError, match="payload offset -1 "):
        h.check_guards()


@pytest.mark.parametrize("offset", [0, 1, 8])
def test_byte_past_payload_is_caught(offset):
    v, h = guarded((4, 6), offset=offset, device="cpu")
    h.buf[h.hi] = 0
    with pytest.raises(AssertionError, match="payload offset 24 "):
        h.check_guards()


def test_first_and_last_guard_bytes_are_checked():
    for at in (0, -1):
        v, h = guarded((2,), device="cpu")
        h.buf[at] = FILL ^ 1
        with pytest.raises(AssertionError):
            h.check_guards()


def test_other_fill_and_int32_payload():
    import torch
    v, h = guarded((5,), fill=0x3C, device="cpu", dtype=torch.int32)
    assert v.dtype == torch.int32 and v.data_ptr() % 16 == 0
    assert (h.host() == 0x3C3C3C3C).all()
    h.load(np.array([0, -1, -3, 7, 1 << 30], np.int32))
    assert h.host().tolist() == [0, -1, -3, 7, 1 << 30]
    h.check_guards()
    h.buf[h.hi + 3] = 0
    with pytest.raises(AssertionError, match="payload offset 23 "):
        h.check_guards()
    w, g = guarded_from(np.array([[1, 2], [3, 4]], np.uint8), offset=4, device="cpu")
    assert w.tolist() == [[1, 2], [3, 4]] and w.data_ptr() % 16 == 4
    g.check_guards()
