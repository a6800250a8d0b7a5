"""Guarded test buffers: a payload between two runs of guard bytes, at a chosen byte offset
past a 16-byte boundary, everything pre-filled with one poison byte.

    [256 guard bytes][offset pad][payload][256 guard bytes]

A kernel that stores before or past the buffer it was given changes a guard byte, and
check_guards() names the first such byte relative to the payload; payload bytes the kernel
does not write keep the poison, so a test can assert that they were left alone."""
import numpy as np

GUARD = 256
FILL = 0xA5


class Guarded:
    """Handle of one guarded buffer: `view` is the payload tensor."""

    def __init__(self, buf, lo, hi, fill, view):
        self.buf, self.lo, self.hi, self.fill, self.view = buf, lo, hi, fill, view

    def load(self, a):
        """Copy the ndarray `a` (the payload's shape and item size) into the payload."""
        import torch
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:          # torch.from_numpy wants a writable array
            a = a.copy()
        assert a.nbytes == self.hi - self.lo, (a.nbytes, self.hi - self.lo)
        src = torch.from_numpy(a.reshape(-1).view(np.uint8))
        self.buf[self.lo:self.hi].copy_(src)
        return self.view

    def host(self):
        """The payload as an ndarray (after a device synchronise)."""
        if self.buf.is_cuda:
            import torch
            torch.cuda.synchronize()
        return self.view.cpu().numpy()

    def check_guards(self):
        """Every byte outside the payload still holds the fill byte."""
        if self.buf.is_cuda:
            import torch
            torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        outside = np.ones(b.size, bool)
        outside[self.lo:self.hi] = False
        bad = np.flatnonzero(outside & (b != self.fill))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(
                f"guard byte at payload offset {i - self.lo} (payload is {self.hi - self.lo} "
                f"bytes) holds 0x{int(b[i]):02x}, not the fill 0x{self.fill:02x}; "
                f"{bad.size} guard bytes changed")


def guarded(shape, offset=0, fill=FILL, device="cuda", dtype=None):
    """(view, handle): a contiguous tensor of `shape` (uint8, or `dtype`) whose data_ptr() is
    `offset` bytes past a 16-byte boundary, inside a buffer of guard bytes; every byte, payload
    included, holds `fill`."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    item = torch.empty(0, dtype=dtype).element_size()
    assert 0 <= offset < 16 and offset % item == 0, (offset, item)
    shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    lo, hi = GUARD + offset, GUARD + offset + nbytes
    buf = torch.full((hi + GUARD,), fill, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[lo:hi].view(dtype).view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == offset
    return view, Guarded(buf, lo, hi, fill, view)


def guarded_from(a, offset=0, fill=FILL, device="cuda"):
    """A guarded copy of the uint8 / int32 ndarray `a`: (view, handle)."""
    import torch
    a = np.ascontiguousarray(a)
    dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}[a.dtype]
    v, h = guarded(a.shape, offset, fill, device, dtype)
    h.load(a)
    return v, h
