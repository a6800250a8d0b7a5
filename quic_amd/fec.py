"""Python front-end of the MI355X FEC engine (ctypes over libquic_fec.so).

Mirrors the reference codec interface (net/quic/core/libcat/cauchy_256.h):
`cauchy_256_init`, `cauchy_256_encode`, `cauchy_256_decode`, `Block`, with the same
argument meaning, return codes and in-place decode semantics, plus the batched
engine (`FecEngine`) that the GPU path is built for.  Every byte of parity or
recovered data is computed by the gfx950 kernels; nothing here computes on the CPU.

Device buffers are torch tensors (uint8, contiguous, on a ROCm device): torch is
used only for memory and streams.
"""
import ctypes
import weakref

import numpy as np

from ._lib import Block, FecError, load

CAUCHY_256_VERSION = 2
_u8p = ctypes.POINTER(ctypes.c_uint8)


# ----------------------------------------------------------------- reference ABI
def _cauchy_256_init(expected_version):
    """cauchy_256.h:47.  0 on success, -1 on a version mismatch (what the reference
    code returns), negative on GPU bring-up failure."""
    return load()._cauchy_256_init(expected_version)


def cauchy_256_init():
    return _cauchy_256_init(CAUCHY_256_VERSION)


def _as_u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(_u8p)


def _vp(a):
    """void* of a numpy array; None stays None (a null pointer)."""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def cauchy_256_encode(k, m, data_ptrs, recovery_blocks, block_bytes):
    """cauchy_256.h:78.  data_ptrs: sequence of k uint8 arrays (block_bytes each);
    recovery_blocks: writable uint8 array of m*block_bytes bytes (filled in place).
    Returns the reference's return code."""
    keep = [_as_u8(d) for d in data_ptrs]
    arr = (_u8p * max(len(keep), 1))(*[p for _, p in keep])
    if not (isinstance(recovery_blocks, np.ndarray) and recovery_blocks.dtype == np.uint8
            and recovery_blocks.flags.c_contiguous):
        raise TypeError("recovery_blocks must be a C-contiguous uint8 numpy array")
    return load().cauchy_256_encode(k, m, arr, _vp(recovery_blocks), block_bytes)


def make_blocks(arrays, rows):
    """Build a `Block[]` over caller-owned uint8 arrays (decoded in place)."""
    blocks = (Block * max(len(arrays), 1))()
    for i, (a, r) in enumerate(zip(arrays, rows)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
            raise TypeError("blocks must be C-contiguous uint8 numpy arrays")
        blocks[i].data = a.ctypes.data_as(_u8p)
        blocks[i].row = int(r)
    return blocks


def cauchy_256_decode(k, m, blocks, block_bytes):
    """cauchy_256.h:103.  `blocks` is a Block array from make_blocks(); data and row
    fields are updated in place.  Returns the reference's return code."""
    return load().cauchy_256_decode(k, m, blocks, block_bytes)


def cauchy_matrix(k, m):
    """Rows 1..m-1 of the Cauchy matrix the reference uses, (m-1) x k."""
    out = np.zeros((m - 1, k), np.uint8)
    rc = load().qfec_cauchy_matrix(k, m, _vp(out))
    if rc:
        raise ValueError(f"no Cauchy matrix for k={k} m={m}")
    return out


# ------------------------------------------------------------------ batch engine
# Every wrapper below checks all of its arguments (_check, then _ptr where a pointer is taken)
# before the library is touched (_call).
_HOST_KIND = "host buffers must be contiguous CPU tensors (pinned for full speed)"


def _check(t, name, dtype, shape, host=False, rows=False, optional=False):
    """One array argument: a tensor of `dtype` (a torch dtype's name) and exactly `shape`, None
    in `shape` standing for any extent (of a host buffer: any extent > 0).  An int (one value
    for every row) passes here and is refused where a pointer is taken of it (_ptr); so does
    None for an `optional` host array and for any device array (the library answers for a
    missing one).  The library copies whole rows into and out of a host buffer, so a short one
    would be overrun and a wrong dtype misread: a host buffer must be a contiguous CPU tensor
    (TypeError), and its dtype or shape is a ValueError.  A device tensor's kind, placement and
    contiguity are checked where its pointer is taken; its dtype or shape is a TypeError, but
    for the dense per-row arrays (`rows`: one entry or row per packet, payload or revived
    block), whose row count is a ValueError."""
    if isinstance(t, int) or (t is None and (optional or not host)):
        return
    import torch
    if host and (not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_contiguous()):
        raise TypeError(f"{name}: {_HOST_KIND}")
    dtype = getattr(torch, dtype)
    if t.dtype != dtype:
        raise (ValueError if host else TypeError)(f"{name}: dtype {t.dtype}, expected {dtype}")
    if t.dim() != len(shape) or any(got != want if want is not None else host and got <= 0
                                    for got, want in zip(t.shape, shape)):
        raise (ValueError if host or rows else TypeError)(
            f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")


def _ptr(t, host=False):
    """void* of a tensor argument on its side of the bus; None stays None."""
    if t is None:
        return None
    import torch
    if host:
        if not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_contiguous():
            raise TypeError(_HOST_KIND)
    else:
        if not isinstance(t, torch.Tensor):
            raise TypeError("device buffers must be torch tensors")
        if not t.is_cuda or t.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32,
                                           torch.int64):
            raise TypeError("device buffers must be integer tensors on a ROCm device")
        if not t.is_contiguous():
            raise ValueError("device buffers must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _ptr_or_all(v, host=False):
    """(array pointer, scalar) of a per-row argument (a length, a pn_len): a tensor, or an int
    meaning the same value for every row."""
    if isinstance(v, int):
        return None, v
    return _ptr(v, host), 0


def _stride(t):
    """Row stride of an optional row array (0 without one)."""
    return 0 if t is None else t.stride(0)


def _call(name, engine, *args, reference_rc=False):
    """Call the library's `name` on the engine's context.  Returns its code; a non-zero one
    raises FecError, but for the encodes (`reference_rc`), which hand the reference's -1
    (unsupported parameters) to the caller and raise below it."""
    rc = getattr(engine.lib, name)(engine._h, *args)
    if rc < -1 if reference_rc else rc:
        raise FecError(rc, name)
    return rc


def _stream(stream, like):
    if stream is not None:
        return ctypes.c_void_p(int(stream))
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(like.device).cuda_stream)


def _groups(bb, **offs):
    """G of a ragged device call: bb int32 [G] and its offset arrays int64 [G]."""
    _check(bb, "bb", "int32", (None,))
    for name, off in offs.items():
        _check(off, name, "int64", (bb.shape[0],))
    return bb.shape[0]


def _mixed_groups(code, bb, status, **offs):
    """G of a mixed-code device call: code uint8 [G], then bb, the offsets and status as in the
    ragged calls."""
    import torch
    if not isinstance(code, torch.Tensor):
        raise TypeError("code: a uint8 device tensor [G]")
    _check(code, "code", "uint8", (None,))
    G = code.shape[0]
    _check(bb, "bb", "int32", (G,))
    for name, off in offs.items():
        _check(off, name, "int64", (G,))
    _check(status, "status", "int32", (G,))
    return G


def _codes(codes):
    """(k, m) pairs -> the two int32 arrays the library takes."""
    pairs = [(int(k), int(m)) for k, m in codes]
    return (pairs, np.array([k for k, _ in pairs], np.int32),
            np.array([m for _, m in pairs], np.int32))


class CodeSet:
    """The codes of a mixed-code batch (qfec_codeset): built once per engine, immutable.
    codes[i] = (k, m); kmax, mmax and rmax (the largest min(k, m)) size the row arrays."""

    def __init__(self, engine, codes):
        self.codes, k, m = _codes(codes)
        self.engine = engine
        h = ctypes.c_void_p()
        rc = engine.lib.qfec_codeset_create(engine._h, len(self.codes), _vp(k), _vp(m),
                                            ctypes.byref(h))
        if rc:
            raise FecError(rc, "qfec_codeset_create")
        self._h = h
        d = [ctypes.c_int() for _ in range(3)]
        engine.lib.qfec_codeset_dims(h, *[ctypes.byref(x) for x in d])
        self.kmax, self.mmax, self.rmax = (x.value for x in d)

    def reserve(self, groups):
        """Size both decode workspaces for `groups` groups (qfec_codeset_reserve)."""
        rc = self.engine.lib.qfec_codeset_reserve(self._h, groups)
        if rc:
            raise FecError(rc, "qfec_codeset_reserve")

    def close(self):
        if getattr(self, "_h", None):
            self.engine.lib.qfec_codeset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr_tables(bb, status, **tables):
    """G of a pointer-table call: every table (tensor, n) is int64 [G][n]; bb is an int or
    int32 [G], status None or int32 [G]."""
    import torch
    G = None
    for name, (t, n) in tables.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a pointer table must be an int64 device tensor")
        G = t.shape[0] if G is None and t.dim() else G
        _check(t, name, "int64", (G, n))
    if isinstance(bb, bool) or not isinstance(bb, int):
        if not isinstance(bb, torch.Tensor):
            raise TypeError("bb: an int or an int32 device tensor")
        _check(bb, "bb", "int32", (G,))
    _check(status, "status", "int32", (G,))
    return G


def block_ptrs(tensor, byte_offsets):
    """The int64 device tensor tensor.data_ptr() + byte_offsets: the addresses of blocks that
    start `byte_offsets` (any integer array or tensor, any shape) bytes into `tensor`, as the
    pointer-table calls take them.  The caller keeps `tensor` alive while they are used."""
    import torch
    off = torch.as_tensor(byte_offsets, dtype=torch.int64)
    return (off + tensor.data_ptr()).to(tensor.device)


class FecEngine:
    """One per GPU: owns a qfec_ctx (coefficient tables, decode workspace, staging)."""

    def __init__(self, device=0):
        self.lib = load()
        self.device = device
        h = ctypes.c_void_p()
        rc = self.lib.qfec_ctx_create(device, ctypes.byref(h))
        if rc:
            raise FecError(rc, "qfec_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            for ref in getattr(self, "_windows", []):   # a window is destroyed before its context
                win = ref()
                if win is not None:
                    win.close()
            self.lib.qfec_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """Launch-shape option of this engine's context (qfec_ctx_set_option)."""
        rc = self.lib.qfec_ctx_set_option(self._h, name.encode(), int(value))
        if rc:
            raise FecError(rc, f"qfec_ctx_set_option({name})")

    def get_option(self, name):
        v = ctypes.c_int()
        rc = self.lib.qfec_ctx_get_option(self._h, name.encode(), ctypes.byref(v))
        if rc:
            raise FecError(rc, f"qfec_ctx_get_option({name})")
        return v.value

    def reserve(self, k, m, block_bytes, groups):
        _call("qfec_reserve", self, k, m, block_bytes, groups)

    # device-resident batch calls (enqueue only)
    def encode(self, k, m, block_bytes, data, parity, stream=None):
        """data [G][k][bb] -> parity [G][m][bb] (torch uint8 on the device).  Returns
        0 or -1 (the reference's unsupported-parameter code)."""
        return _call("qfec_encode_batch", self, k, m, block_bytes, data.shape[0], _ptr(data),
                     _ptr(parity), _stream(stream, data), reference_rc=True)

    def decode(self, k, m, block_bytes, blocks, rows_in, out=None, rows_out=None, status=None,
               stream=None):
        """blocks [G][k][bb], rows_in [G][k] uint8.  out defaults to blocks (in place),
        rows_out to rows_in.  status: optional int32 [G]."""
        out = blocks if out is None else out
        rows_out = rows_in if rows_out is None else rows_out
        return _call("qfec_decode_batch", self, k, m, block_bytes, blocks.shape[0], _ptr(blocks),
                     _ptr(rows_in), _ptr(out), _ptr(rows_out), _ptr(status),
                     _stream(stream, blocks))

    def decode_recovered(self, k, m, block_bytes, blocks, rows_in, rec, rec_rows, status=None,
                         stream=None):
        """Recovered-blocks layout: rec [G][min(k,m)][bb], rec_rows [G][min(k,m)] uint8
        (data row of each recovered block, ascending; 255 = unused).  blocks / rows_in are
        not modified."""
        return _call("qfec_decode_batch_recovered", self, k, m, block_bytes, blocks.shape[0],
                     _ptr(blocks), _ptr(rows_in), _ptr(rec), _ptr(rec_rows), _ptr(status),
                     _stream(stream, blocks))

    # ragged batches: one (k, m), a block size per group (packed layout, include/quic_fec.h)
    def encode_ragged(self, k, m, bb, data, data_off, parity, par_off, status=None, stream=None):
        """Group g: data + data_off[g] holds [k][bb[g]], parity + par_off[g] receives
        [m][bb[g]].  bb int32 [G], offsets int64 [G] (bytes, multiples of 16), data / parity
        flat uint8, all on the device; status: optional int32 [G] (per-group 0 / -1).  Returns
        0 or -1 (k + m > 256 with m > 1)."""
        G = _groups(bb, data_off=data_off, par_off=par_off)
        return _call("qfec_encode_batch_ragged", self, k, m, G, _ptr(bb), _ptr(data),
                     _ptr(data_off), _ptr(parity), _ptr(par_off), _ptr(status),
                     _stream(stream, data), reference_rc=True)

    def decode_ragged_recovered(self, k, m, bb, blocks, blocks_off, rows_in, rec, rec_off,
                                rec_rows, status=None, stream=None):
        """Recovered-blocks layout per group: rec + rec_off[g] receives up to
        [min(k,m)][bb[g]], rec_rows [G][min(k,m)] the restored data rows (255 = unused).
        blocks / rows_in [G][k] are not modified."""
        G = _groups(bb, blocks_off=blocks_off, rec_off=rec_off)
        return _call("qfec_decode_batch_ragged_recovered", self, k, m, G, _ptr(bb), _ptr(blocks),
                     _ptr(blocks_off), _ptr(rows_in), _ptr(rec), _ptr(rec_off), _ptr(rec_rows),
                     _ptr(status), _stream(stream, blocks))

    # mixed-code batches: a (k, m) per group through a code set (include/quic_fec.h)
    def codeset(self, codes):
        """A CodeSet of this engine for `codes`, a sequence of 1 to 32 (k, m) pairs; a group
        names its code by its index in the sequence.  Close it before the engine."""
        return CodeSet(self, codes)

    def encode_mixed(self, cs, code, bb, data, data_off, parity, par_off, status=None,
                     stream=None):
        """Group g has code cs.codes[code[g]] = (k_g, m_g): data + data_off[g] holds
        [k_g][bb[g]], parity + par_off[g] receives [m_g][bb[g]].  code uint8 [G], bb int32 [G],
        offsets int64 [G] (bytes, multiples of 16), data / parity flat uint8, all on the device;
        status: optional int32 [G] (per group 0, -1, or -2 for a code index outside the set).
        Returns 0: every rejection is per group."""
        G = _mixed_groups(code, bb, status, data_off=data_off, par_off=par_off)
        return _call("qfec_encode_batch_mixed", self, cs._h, G, _ptr(code), _ptr(bb), _ptr(data),
                     _ptr(data_off), _ptr(parity), _ptr(par_off), _ptr(status),
                     _stream(stream, data))

    def decode_mixed_recovered(self, cs, code, bb, blocks, blocks_off, rows_in, rec, rec_off,
                               rec_rows, status=None, stream=None):
        """Recovered-blocks layout per group: rec + rec_off[g] receives up to
        [min(k_g, m_g)][bb[g]].  rows_in is uint8 [G][cs.kmax] (the first k_g tags of a row are
        read), rec_rows uint8 [G][cs.rmax] (255 = unused, up to the set's rmax).  blocks /
        rows_in are not modified."""
        G = _mixed_groups(code, bb, status, blocks_off=blocks_off, rec_off=rec_off)
        _check(rows_in, "rows_in", "uint8", (G, cs.kmax))
        _check(rec_rows, "rec_rows", "uint8", (G, cs.rmax))
        return _call("qfec_decode_batch_mixed_recovered", self, cs._h, G, _ptr(code), _ptr(bb),
                     _ptr(blocks), _ptr(blocks_off), _ptr(rows_in), _ptr(rec), _ptr(rec_off),
                     _ptr(rec_rows), _ptr(status), _stream(stream, blocks))

    # pointer-table batches: every block at a device address of its own (include/quic_fec.h)
    def encode_ptrs(self, k, m, bb, data_ptrs, parity_ptrs, status=None, stream=None):
        """Group g: its data blocks lie at the addresses data_ptrs[g] (int64 [G][k]), parity
        block y is written at parity_ptrs[g][y] (int64 [G][m]); see block_ptrs().  bb: int32 [G]
        device tensor, or an int for every group; status: optional int32 [G].  The library cannot
        check the addresses.  Returns 0 or -1 (k + m > 256 with m > 1)."""
        G = _ptr_tables(bb, status, data_ptrs=(data_ptrs, k), parity_ptrs=(parity_ptrs, m))
        d_bb, bb_all = _ptr_or_all(bb)
        return _call("qfec_encode_batch_ptrs", self, k, m, G, d_bb, bb_all, _ptr(data_ptrs),
                     _ptr(parity_ptrs), _ptr(status), _stream(stream, data_ptrs),
                     reference_rc=True)

    def decode_ptrs_recovered(self, k, m, bb, block_ptrs, rows_in, rec_ptrs, rec_rows,
                              status=None, stream=None):
        """Recovered-blocks layout over addresses: the received blocks lie at block_ptrs[g]
        (int64 [G][k]), recovered block j is written at rec_ptrs[g][j] (int64 [G][min(k,m)]) and
        its data row to rec_rows [G][min(k,m)] (255 = unused; such rec_ptrs entries are never
        dereferenced).  rows_in uint8 [G][k]; bb and status as in encode_ptrs."""
        rmax = min(k, m)
        G = _ptr_tables(bb, status, block_ptrs=(block_ptrs, k), rec_ptrs=(rec_ptrs, rmax))
        _check(rows_in, "rows_in", "uint8", (G, k))
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        d_bb, bb_all = _ptr_or_all(bb)
        return _call("qfec_decode_batch_ptrs_recovered", self, k, m, G, d_bb, bb_all,
                     _ptr(block_ptrs), _ptr(rows_in), _ptr(rec_ptrs), _ptr(rec_rows),
                     _ptr(status), _stream(stream, block_ptrs))

    # packet protection next to the codec (NullEncrypter / NullDecrypter, pp_null.hip)
    def null_seal(self, ad, ad_len, pt, pt_len, out, out_len, stream=None):
        """NullEncrypter::EncryptPacket over n packets: ad [n][ad_stride], pt [n][pt_stride]
        -> out [n][out_stride] = AD || tag12 || PT; out_len int32 [n] (-1: does not fit).
        ad_len / pt_len: int32 [n] tensors or ints (null_encrypter.cc:23-43)."""
        n = out.shape[0]
        a, a_all = _ptr_or_all(ad_len)
        p, p_all = _ptr_or_all(pt_len)
        _call("qfec_null_seal_batch", self, n, _ptr(ad), ad.stride(0) if n else 0, a, a_all,
              _ptr(pt), pt.stride(0) if n else 0, p, p_all, _ptr(out), out.stride(0),
              _ptr(out_len), _stream(stream, out))

    def null_open(self, pkt, pkt_len, ad_len, out, out_len, stream=None):
        """NullDecrypter::DecryptPacket over n wire packets pkt [n][pkt_stride] (first ad_len
        bytes = associated data) -> plaintext in out [n][out_stride], out_len int32 [n]
        (-1: rejected)."""
        p, p_all = _ptr_or_all(pkt_len)
        a, a_all = _ptr_or_all(ad_len)
        _call("qfec_null_open_batch", self, pkt.shape[0], _ptr(pkt), pkt.stride(0), p, p_all, a,
              a_all, _ptr(out), out.stride(0), _ptr(out_len), _stream(stream, pkt))

    def encode_seal(self, k, m, block_bytes, data, parity, hdr, hdr_len, pkt, pkt_len,
                    stream=None):
        """SerializeFec on the device: encode data [G][k][bb] into parity [G][m][bb], then
        seal FEC packet g*m+i = hdr[g*m+i][:hdr_len] || tag12 || parity[g][i] into
        pkt [G*m][pkt_stride]; pkt_len int32 [G*m]."""
        h, h_all = _ptr_or_all(hdr_len)
        _call("qfec_encode_seal_batch", self, k, m, block_bytes, data.shape[0], _ptr(data),
              _ptr(parity), _ptr(hdr), hdr.stride(0), h, h_all, _ptr(pkt), pkt.stride(0),
              _ptr(pkt_len), _stream(stream, data))

    def seal_groups(self, k, m, block_bytes, data, parity, hdr, hdr_len, pt_len, pkt, pkt_len,
                    encode=False, stream=None):
        """Seal every packet of each group in one launch: packet p = g*(k+m)+i =
        hdr[p][:hdr_len] || tag12 || (data[g][i] if i < k else parity[g][i-k])[:pt_len] into
        pkt [G*(k+m)][pkt_stride]; pkt_len int32 [G*(k+m)].  encode=True first encodes data
        into parity (qfec_encode_seal_groups_batch)."""
        h, h_all = _ptr_or_all(hdr_len)
        p, p_all = _ptr_or_all(pt_len)
        _call("qfec_encode_seal_groups_batch" if encode else "qfec_seal_groups_batch", self, k, m,
              block_bytes, data.shape[0], _ptr(data), _ptr(parity), _ptr(hdr), hdr.stride(0), h,
              h_all, p, p_all, _ptr(pkt), pkt.stride(0), _ptr(pkt_len), _stream(stream, data))

    def open_decode(self, k, m, block_bytes, pkt, pkt_len, ad_len, blocks, rows, open_len, rec,
                    rec_rows, status=None, stream=None):
        """Receiver: open every wire packet pkt [G*(k+m)][stride] (pkt_len int32, < 0 = not
        received), place the plaintexts into blocks [G][k][bb] / rows [G][k], then the
        recovered-layout decode into rec / rec_rows / status.  open_len int32 [G*(k+m)]."""
        a, a_all = _ptr_or_all(ad_len)
        _call("qfec_open_decode_batch", self, k, m, block_bytes, blocks.shape[0], _ptr(pkt),
              pkt.stride(0), _ptr(pkt_len), a, a_all, _ptr(blocks), _ptr(rows), _ptr(open_len),
              _ptr(rec), _ptr(rec_rows), _ptr(status), _stream(stream, pkt))

    # ragged packet protection: the two calls above over the packed layout, a block size per
    # group (include/quic_fec.h, "Ragged packet protection")
    def seal_groups_ragged(self, k, m, bb, data, data_off, parity, par_off, hdr, hdr_len, pt_len,
                           pkt, pkt_len, encode=False, status=None, stream=None):
        """seal_groups with a block size per group: packet p = g*(k+m)+i takes its plaintext
        from block i of data + data_off[g] ([k][bb[g]]) for i < k, else block i-k of parity +
        par_off[g].  bb int32 [G], offsets int64 [G], data / parity flat uint8; hdr, pkt,
        pkt_len dense by packet as in seal_groups; pt_len int32 [G*(k+m)] or None (whole
        blocks).  encode=True first encodes into parity (status: optional int32 [G], -1 for
        the groups the encode rejects, none of whose packets is sealed)."""
        G = _groups(bb, data_off=data_off, par_off=par_off)
        n = G * (k + m)
        _check(hdr, "hdr", "uint8", (n, None), rows=True)
        _check(hdr_len, "hdr_len", "int32", (n,), rows=True)
        _check(pt_len, "pt_len", "int32", (n,), rows=True)
        _check(pkt, "pkt", "uint8", (n, None), rows=True)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(status, "status", "int32", (G,))
        if isinstance(pt_len, int):
            raise TypeError("pt_len: an int32 [G*(k+m)] tensor, or None for whole blocks")
        h, h_all = _ptr_or_all(hdr_len)
        args = (k, m, G, _ptr(bb), _ptr(data), _ptr(data_off), _ptr(parity), _ptr(par_off),
                _ptr(hdr), _stride(hdr), h, h_all, _ptr(pt_len), _ptr(pkt), pkt.stride(0),
                _ptr(pkt_len))
        if encode:
            _call("qfec_encode_seal_groups_batch_ragged", self, *args, _ptr(status),
                  _stream(stream, data))
        else:
            if status is not None:
                raise ValueError("status is the encode's: pass it with encode=True")
            _call("qfec_seal_groups_batch_ragged", self, *args, _stream(stream, data))

    def open_decode_ragged(self, k, m, bb, pkt, pkt_len, ad_len, blocks, blocks_off, rows,
                           open_len, rec, rec_off, rec_rows, status=None, stream=None):
        """open_decode with a block size per group: blocks + blocks_off[g] receives
        [k][bb[g]], rec + rec_off[g] up to [min(k,m)][bb[g]] (flat uint8, offsets int64 [G]);
        pkt, pkt_len, open_len dense by packet, rows [G][k], rec_rows [G][min(k,m)]."""
        G = _groups(bb, blocks_off=blocks_off, rec_off=rec_off)
        n = G * (k + m)
        _check(pkt, "pkt", "uint8", (n, None), rows=True)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(ad_len, "ad_len", "int32", (n,), rows=True)
        _check(open_len, "open_len", "int32", (n,), rows=True)
        _check(rows, "rows", "uint8", (G, k))
        _check(rec_rows, "rec_rows", "uint8", (G, min(k, m)))
        _check(status, "status", "int32", (G,))
        a, a_all = _ptr_or_all(ad_len)
        _call("qfec_open_decode_batch_ragged", self, k, m, G, _ptr(bb), _ptr(pkt), pkt.stride(0),
              _ptr(pkt_len), a, a_all, _ptr(blocks), _ptr(blocks_off), _ptr(rows), _ptr(open_len),
              _ptr(rec), _ptr(rec_off), _ptr(rec_rows), _ptr(status), _stream(stream, pkt))

    # framed groups: QuicFecGroup's wire format around the ragged protected calls
    # (include/quic_fec.h, "Framed groups")
    def frame_blocks_ragged(self, k, bb, pay, pay_len, pn_len, data, data_off, status=None,
                            stream=None):
        """Blocks from payload rows: block (g, i) at data + data_off[g] + i*bb[g] becomes
        prefix || pay[g*k+i][:pay_len] || zeros.  pay uint8 [G*k][stride], pay_len int32 [G*k],
        pn_len uint8 [G*k] or an int; status: optional int32 [G] (-3 for a rejected group, of
        which nothing is written)."""
        G = _groups(bb, data_off=data_off)
        _check(pay, "pay", "uint8", (G * k, None), rows=True)
        _check(pay_len, "pay_len", "int32", (G * k,), rows=True)
        _check(pn_len, "pn_len", "uint8", (G * k,), rows=True)
        _check(status, "status", "int32", (G,))
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_frame_blocks_batch_ragged", self, k, G, _ptr(bb), _ptr(pay), pay.stride(0),
              _ptr(pay_len), pn, pn_all, _ptr(data), _ptr(data_off), _ptr(status),
              _stream(stream, data))

    def extract_revived_ragged(self, k, m, bb, rec, rec_off, rec_rows, status, rev, rev_len,
                               rev_pn_len=None, stream=None):
        """Revived payloads from recovered blocks: rev [G*rmax][stride] row g*rmax+j receives the
        payload of recovered block j of group g, rev_len int32 [G*rmax] its length (-1: no such
        block, or longer than the row), rev_pn_len uint8 [G*rmax] the prefix's top two bits.
        status: int32 [G] or None (every group taken as decoded)."""
        G = _groups(bb, rec_off=rec_off)
        rmax = min(k, m)
        _check(rev, "rev", "uint8", (G * rmax, None), rows=True)
        _check(rev_len, "rev_len", "int32", (G * rmax,), rows=True)
        _check(rev_pn_len, "rev_pn_len", "uint8", (G * rmax,), rows=True)
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        _check(status, "status", "int32", (G,))
        _call("qfec_extract_revived_batch_ragged", self, k, m, G, _ptr(bb), _ptr(rec),
              _ptr(rec_off), _ptr(rec_rows), _ptr(status), _ptr(rev), rev.stride(0),
              _ptr(rev_len), _ptr(rev_pn_len), _stream(stream, rec))

    def frame_encode_seal_ragged(self, k, m, bb, data, data_off, parity, par_off, hdr, hdr_len,
                                 pay, pay_len, pn_len, pkt, pkt_len, status=None, stream=None):
        """Sender: payload rows in, wire packets of the reference's format out.  Frames the
        blocks into data (an output), encodes into parity, seals data packet p = g*(k+m)+i as
        hdr[p] || tag12 || payload and FEC packet p as hdr[p] || tag12 || parity block.  pay,
        pay_len, pn_len as in frame_blocks_ragged; hdr, pkt, pkt_len dense by packet as in
        seal_groups_ragged; status: optional int32 [G] (0, -1 encode rejected, -3 framing
        rejected)."""
        G = _groups(bb, data_off=data_off, par_off=par_off)
        n = G * (k + m)
        _check(hdr, "hdr", "uint8", (n, None), rows=True)
        _check(hdr_len, "hdr_len", "int32", (n,), rows=True)
        _check(pkt, "pkt", "uint8", (n, None), rows=True)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(pay, "pay", "uint8", (G * k, None), rows=True)
        _check(pay_len, "pay_len", "int32", (G * k,), rows=True)
        _check(pn_len, "pn_len", "uint8", (G * k,), rows=True)
        _check(status, "status", "int32", (G,))
        h, h_all = _ptr_or_all(hdr_len)
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_frame_encode_seal_groups_batch_ragged", self, k, m, G, _ptr(bb), _ptr(data),
              _ptr(data_off), _ptr(parity), _ptr(par_off), _ptr(hdr), _stride(hdr), h, h_all,
              _ptr(pay), pay.stride(0), _ptr(pay_len), pn, pn_all, _ptr(pkt), pkt.stride(0),
              _ptr(pkt_len), _ptr(status), _stream(stream, data))

    def open_decode_extract_ragged(self, k, m, bb, pkt, pkt_len, ad_len, pn_len, blocks,
                                   blocks_off, rows, open_len, rec, rec_off, rec_rows, rev,
                                   rev_len, rev_pn_len=None, status=None, stream=None):
        """Receiver: wire packets in, revived payloads out.  open_decode_ragged with a data
        packet's plaintext placed behind its prefix (pn_len uint8 [G*(k+m)] or an int), then
        extract_revived_ragged into rev / rev_len / rev_pn_len."""
        G = _groups(bb, blocks_off=blocks_off, rec_off=rec_off)
        n, rmax = G * (k + m), min(k, m)
        _check(pkt, "pkt", "uint8", (n, None), rows=True)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(ad_len, "ad_len", "int32", (n,), rows=True)
        _check(open_len, "open_len", "int32", (n,), rows=True)
        _check(pn_len, "pn_len", "uint8", (n,), rows=True)
        _check(rev, "rev", "uint8", (G * rmax, None), rows=True)
        _check(rev_len, "rev_len", "int32", (G * rmax,), rows=True)
        _check(rev_pn_len, "rev_pn_len", "uint8", (G * rmax,), rows=True)
        _check(rows, "rows", "uint8", (G, k))
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        _check(status, "status", "int32", (G,))
        a, a_all = _ptr_or_all(ad_len)
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_open_decode_extract_batch_ragged", self, k, m, G, _ptr(bb), _ptr(pkt),
              pkt.stride(0), _ptr(pkt_len), a, a_all, pn, pn_all, _ptr(blocks), _ptr(blocks_off),
              _ptr(rows), _ptr(open_len), _ptr(rec), _ptr(rec_off), _ptr(rec_rows), _ptr(status),
              _ptr(rev), rev.stride(0), _ptr(rev_len), _ptr(rev_pn_len), _stream(stream, pkt))

    def open_decode_extract_arrivals_ragged(self, k, m, bb, pkt, pkt_len, ad_len, pn_len,
                                            arr_group, arr_index, arr_state, arr_at, blocks,
                                            blocks_off, rows, open_len, rec, rec_off, rec_rows,
                                            rev, rev_len, rev_pn_len=None, status=None,
                                            stream=None):
        """Receiver over packets in arrival order (include/quic_fec.h, "Arrival-order
        receiver"): pkt uint8 [n][stride], pkt_len int32 [n], ad_len int32 [n] or an int, pn_len
        uint8 [n] or an int are per arrival; arr_group int32 [n] and arr_index uint8 [n] tag each
        arrival with its group in this batch and packet_number - fec_group.  arr_state int32 [n]
        or None receives each arrival's fate (its plaintext length, or ARR_REJECTED /
        ARR_IGNORED / ARR_DUPLICATE / ARR_LATE), arr_at int32 [G*(k+m)] the arrival accepted for
        each slot (-1: none).  Everything else is open_decode_extract_ragged's on the accepted
        packets placed by slot."""
        G = _groups(bb, blocks_off=blocks_off, rec_off=rec_off)
        _check(pkt, "pkt", "uint8", (None, None), rows=True)
        n, slots, rmax = pkt.shape[0], G * (k + m), min(k, m)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(ad_len, "ad_len", "int32", (n,), rows=True)
        _check(pn_len, "pn_len", "uint8", (n,), rows=True)
        _check(arr_group, "arr_group", "int32", (n,), rows=True)
        _check(arr_index, "arr_index", "uint8", (n,), rows=True)
        _check(arr_state, "arr_state", "int32", (n,), rows=True)
        _check(arr_at, "arr_at", "int32", (slots,), rows=True)
        _check(open_len, "open_len", "int32", (slots,), rows=True)
        _check(rev, "rev", "uint8", (G * rmax, None), rows=True)
        _check(rev_len, "rev_len", "int32", (G * rmax,), rows=True)
        _check(rev_pn_len, "rev_pn_len", "uint8", (G * rmax,), rows=True)
        _check(rows, "rows", "uint8", (G, k))
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        _check(status, "status", "int32", (G,))
        a, a_all = _ptr_or_all(ad_len)
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_open_decode_extract_arrivals_ragged", self, k, m, G, _ptr(bb), n, _ptr(pkt),
              pkt.stride(0), _ptr(pkt_len), a, a_all, pn, pn_all, _ptr(arr_group),
              _ptr(arr_index), _ptr(arr_state), _ptr(arr_at), _ptr(blocks), _ptr(blocks_off),
              _ptr(rows), _ptr(open_len), _ptr(rec), _ptr(rec_off), _ptr(rec_rows), _ptr(status),
              _ptr(rev), rev.stride(0), _ptr(rev_len), _ptr(rev_pn_len), _stream(stream, pkt))

    def rxwin(self, k, m, groups, hold_stride):
        """A receiver window on this engine (include/quic_fec.h, "Receiver window"): `groups`
        group places of one (k, m) whose state stays on the device from push to push."""
        return RxWindow(self, k, m, groups, hold_stride)

    # mixed-code wire path (include/quic_fec.h, "Mixed-code wire path")
    def frame_encode_seal_mixed(self, cs, code, bb, pkt_first, pay_first, data, data_off, parity,
                                par_off, hdr, hdr_len, pay, pay_len, pn_len, pkt, pkt_len,
                                status=None, stream=None):
        """frame_encode_seal_ragged with a code per group: group g has cs.codes[code[g]], its
        packets are rows pkt_first[g] .. of hdr / pkt / pkt_len (npkt rows), its payloads rows
        pay_first[g] .. of pay / pay_len / pn_len (npay rows); pkt_first, pay_first int32 [G+1]
        device tensors (mixed_packet_layout).  status: optional int32 [G] (0, -1, -3, or -2 for a
        group without a code or with a span that does not fit)."""
        G = _mixed_groups(code, bb, status, data_off=data_off, par_off=par_off)
        _check(pkt_first, "pkt_first", "int32", (G + 1,))
        _check(pay_first, "pay_first", "int32", (G + 1,))
        _check(pkt, "pkt", "uint8", (None, None), rows=True)
        _check(pay, "pay", "uint8", (None, None), rows=True)
        npkt, npay = pkt.shape[0], pay.shape[0]
        _check(hdr, "hdr", "uint8", (npkt, None), rows=True)
        _check(hdr_len, "hdr_len", "int32", (npkt,), rows=True)
        _check(pkt_len, "pkt_len", "int32", (npkt,), rows=True)
        _check(pay_len, "pay_len", "int32", (npay,), rows=True)
        _check(pn_len, "pn_len", "uint8", (npay,), rows=True)
        h, h_all = _ptr_or_all(hdr_len)
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_frame_encode_seal_groups_batch_mixed", self, cs._h, G, _ptr(code), _ptr(bb),
              _ptr(pkt_first), _ptr(pay_first), npkt, npay, _ptr(data), _ptr(data_off),
              _ptr(parity), _ptr(par_off), _ptr(hdr), _stride(hdr), h, h_all, _ptr(pay),
              pay.stride(0), _ptr(pay_len), pn, pn_all, _ptr(pkt), pkt.stride(0), _ptr(pkt_len),
              _ptr(status), _stream(stream, data))

    def open_decode_extract_arrivals_mixed(self, cs, code, bb, pkt_first, pkt, pkt_len, ad_len,
                                           pn_len, arr_group, arr_index, arr_state, arr_at,
                                           blocks, blocks_off, rows, open_len, rec, rec_off,
                                           rec_rows, rev, rev_len, rev_pn_len=None, status=None,
                                           stream=None):
        """open_decode_extract_arrivals_ragged with a code per group: the slot of arrival a is
        pkt_first[g] + arr_index[a] (pkt_first int32 [G+1]); arr_at and open_len are int32 [npkt]
        (npkt = arr_at's length), rows uint8 [G][cs.kmax], rec_rows uint8 [G][cs.rmax], rev /
        rev_len / rev_pn_len hold G * cs.rmax rows.  Arrivals of a group without a code or with
        a span that does not fit are ARR_IGNORED and the group's status is -2."""
        G = _mixed_groups(code, bb, status, blocks_off=blocks_off, rec_off=rec_off)
        _check(pkt_first, "pkt_first", "int32", (G + 1,))
        import torch
        if not isinstance(arr_at, torch.Tensor) or not isinstance(pkt, torch.Tensor):
            raise TypeError("pkt and arr_at: device tensors (their lengths are n and npkt)")
        _check(pkt, "pkt", "uint8", (None, None), rows=True)
        _check(arr_at, "arr_at", "int32", (None,), rows=True)
        n, npkt, rmax = pkt.shape[0], arr_at.shape[0], cs.rmax
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(ad_len, "ad_len", "int32", (n,), rows=True)
        _check(pn_len, "pn_len", "uint8", (n,), rows=True)
        _check(arr_group, "arr_group", "int32", (n,), rows=True)
        _check(arr_index, "arr_index", "uint8", (n,), rows=True)
        _check(arr_state, "arr_state", "int32", (n,), rows=True)
        _check(open_len, "open_len", "int32", (npkt,), rows=True)
        _check(rev, "rev", "uint8", (G * rmax, None), rows=True)
        _check(rev_len, "rev_len", "int32", (G * rmax,), rows=True)
        _check(rev_pn_len, "rev_pn_len", "uint8", (G * rmax,), rows=True)
        _check(rows, "rows", "uint8", (G, cs.kmax))
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        a, a_all = _ptr_or_all(ad_len)
        pn, pn_all = _ptr_or_all(pn_len)
        _call("qfec_open_decode_extract_arrivals_mixed", self, cs._h, G, _ptr(code), _ptr(bb),
              _ptr(pkt_first), npkt, n, _ptr(pkt), pkt.stride(0), _ptr(pkt_len), a, a_all, pn,
              pn_all, _ptr(arr_group), _ptr(arr_index), _ptr(arr_state), _ptr(arr_at),
              _ptr(blocks), _ptr(blocks_off), _ptr(rows), _ptr(open_len), _ptr(rec),
              _ptr(rec_off), _ptr(rec_rows), _ptr(status), _ptr(rev), rev.stride(0),
              _ptr(rev_len), _ptr(rev_pn_len), _stream(stream, pkt))

    # host-pointer batch calls (synchronous; include H2D/D2H)
    def encode_host(self, k, m, block_bytes, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        G = data.shape[0]
        parity = np.zeros((G, m, block_bytes), np.uint8)
        rc = _call("qfec_encode_batch_host", self, k, m, block_bytes, G, _vp(data), _vp(parity),
                   reference_rc=True)
        return parity, rc

    def decode_host(self, k, m, block_bytes, blocks, rows):
        blocks = np.array(blocks, dtype=np.uint8, order="C", copy=True)
        rows = np.array(rows, dtype=np.uint8, order="C", copy=True)
        G = blocks.shape[0]
        status = np.zeros(G, np.int32)
        _call("qfec_decode_batch_host", self, k, m, block_bytes, G, _vp(blocks), _vp(rows),
              _vp(status))
        return blocks, rows, status


class RxWindow:
    """FecEngine.rxwin: the arrival-order receiver with its state kept between calls (qfec_rxwin).
    push feeds one ring read; a group delivers in the push that brings its k-th packet, with
    status WIN_OPEN before and WIN_DELIVERED after; release returns places to empty.  The engine
    must outlive the window."""

    def __init__(self, engine, k, m, groups, hold_stride):
        self.engine, self.k, self.m = engine, int(k), int(m)
        self.groups, self.hold_stride = int(groups), int(hold_stride)
        h = ctypes.c_void_p()
        rc = engine.lib.qfec_rxwin_create(engine._h, self.k, self.m, self.groups,
                                          self.hold_stride, ctypes.byref(h))
        if rc:
            raise FecError(rc, "qfec_rxwin_create")
        self._h = h
        if not hasattr(engine, "_windows"):
            engine._windows = []
        engine._windows.append(weakref.ref(self))

    def _call(self, name, *args):
        rc = getattr(self.engine.lib, name)(self._h, *args)
        if rc:
            raise FecError(rc, name)

    def push(self, bb, pkt, pkt_len, ad_len, pn_len, arr_group, arr_index, arr_state, rec,
             rec_off, rec_rows, rev, rev_len, rev_pn_len=None, status=None, stream=None):
        """One ring in arrival order: bb int32 [groups] (this push's block size per group); pkt
        uint8 [n][stride], pkt_len int32 [n], ad_len int32 [n] or an int, pn_len uint8 [n] or an
        int, arr_group int32 [n] and arr_index uint8 [n] per arrival, as
        open_decode_extract_arrivals_ragged takes them; arr_state int32 [n] or None.  rec (packed,
        rec_off int64 [groups]), rec_rows uint8 [groups][rmax], rev uint8 [groups*rmax][stride],
        rev_len int32 and rev_pn_len uint8 [groups*rmax], status int32 [groups] receive the
        groups that complete in this push."""
        G, k, m = self.groups, self.k, self.m
        _check(bb, "bb", "int32", (G,))
        _check(rec_off, "rec_off", "int64", (G,))
        _check(pkt, "pkt", "uint8", (None, None), rows=True)
        n, rmax = pkt.shape[0], min(k, m)
        _check(pkt_len, "pkt_len", "int32", (n,), rows=True)
        _check(ad_len, "ad_len", "int32", (n,), rows=True)
        _check(pn_len, "pn_len", "uint8", (n,), rows=True)
        _check(arr_group, "arr_group", "int32", (n,), rows=True)
        _check(arr_index, "arr_index", "uint8", (n,), rows=True)
        _check(arr_state, "arr_state", "int32", (n,), rows=True)
        _check(rev, "rev", "uint8", (G * rmax, None), rows=True)
        _check(rev_len, "rev_len", "int32", (G * rmax,), rows=True)
        _check(rev_pn_len, "rev_pn_len", "uint8", (G * rmax,), rows=True)
        _check(rec_rows, "rec_rows", "uint8", (G, rmax))
        _check(status, "status", "int32", (G,))
        a, a_all = _ptr_or_all(ad_len)
        pn, pn_all = _ptr_or_all(pn_len)
        self._call("qfec_rxwin_push", _ptr(bb), n, _ptr(pkt) if n else None, pkt.stride(0),
                   _ptr(pkt_len), a, a_all, pn, pn_all, _ptr(arr_group), _ptr(arr_index),
                   _ptr(arr_state), _ptr(rec), _ptr(rec_off), _ptr(rec_rows), _ptr(status),
                   _ptr(rev), rev.stride(0), _ptr(rev_len), _ptr(rev_pn_len), _stream(stream, rec))

    def release(self, groups=None, stream=None):
        """The listed group places (int32 device tensor [count]) back to empty; None: all."""
        import torch
        if groups is None:
            s = ctypes.c_void_p(int(stream)) if stream is not None else ctypes.c_void_p(
                torch.cuda.current_stream(self.engine.device).cuda_stream)
            return self._call("qfec_rxwin_release", 0, None, s)
        if not isinstance(groups, torch.Tensor):
            raise TypeError("groups: an int32 device tensor [count], or None for every group")
        _check(groups, "groups", "int32", (None,))
        self._call("qfec_rxwin_release", groups.shape[0], _ptr(groups), _stream(stream, groups))

    def close(self):
        if getattr(self, "_h", None):
            self.engine.lib.qfec_rxwin_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_kernels():
    """Kernels the calling thread's last engine call launched (qfec_last_kernels)."""
    v = load().qfec_last_kernels()
    return v.decode() if v else ""


def last_grids():
    """{kernel: workgroups} of the persistent kernels the calling thread's last engine call
    launched (qfec_last_grids)."""
    v = load().qfec_last_grids()
    out = {}
    for item in (v.decode() if v else "").split():
        name, _, grid = item.partition("=")
        out[name] = int(grid)
    return out


def encode_host_into(engine, k, m, block_bytes, data_h, parity_h):
    """Host-pointer encode on caller-owned CPU tensors (pinned memory recommended):
    H2D, kernels and D2H pipelined in chunks inside the library.  Returns 0 / -1."""
    G = data_h.shape[0]
    _check(data_h, "data", "uint8", (G, k, block_bytes), host=True)
    _check(parity_h, "parity", "uint8", (G, m, block_bytes), host=True)
    return _call("qfec_encode_batch_host", engine, k, m, block_bytes, G, _ptr(data_h, True),
                 _ptr(parity_h, True), reference_rc=True)


def decode_host_into(engine, k, m, block_bytes, blocks_h, rows_h, status_h=None):
    """Host-pointer in-place decode on caller-owned CPU tensors (cauchy_256_decode
    semantics per group)."""
    G = blocks_h.shape[0]
    _check(blocks_h, "blocks", "uint8", (G, k, block_bytes), host=True)
    _check(rows_h, "rows", "uint8", (G, k), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_decode_batch_host", engine, k, m, block_bytes, G, _ptr(blocks_h, True),
                 _ptr(rows_h, True), _ptr(status_h, True))


def encode_seal_groups_host_into(engine, k, m, block_bytes, data_h, hdr_h, hdr_len, pt_len,
                                 pkt_h, pkt_len_h):
    """Sender, host to host (qfec_encode_seal_groups_batch_host): data [G][k][bb] and
    headers hdr [G*(k+m)][hdr_stride] (or None) -> every packet sealed into pkt
    [G*(k+m)][pkt_stride], pkt_len int32 [G*(k+m)].  Returns 0 / -1."""
    G = data_h.shape[0]
    n = G * (k + m)
    _check(data_h, "data", "uint8", (G, k, block_bytes), host=True)
    _check(hdr_h, "hdr", "uint8", (n, None), host=True, optional=True)
    _check(hdr_len, "hdr_len", "int32", (n,), host=True)
    _check(pt_len, "pt_len", "int32", (n,), host=True)
    _check(pkt_h, "pkt", "uint8", (n, None), host=True)
    _check(pkt_len_h, "pkt_len", "int32", (n,), host=True)
    h, h_all = _ptr_or_all(hdr_len, True)
    p, p_all = _ptr_or_all(pt_len, True)
    return _call("qfec_encode_seal_groups_batch_host", engine, k, m, block_bytes, G,
                 _ptr(data_h, True), _ptr(hdr_h, True), _stride(hdr_h), h, h_all, p, p_all,
                 _ptr(pkt_h, True), pkt_h.stride(0), _ptr(pkt_len_h, True), reference_rc=True)


def open_decode_host_into(engine, k, m, block_bytes, pkt_h, pkt_len_h, ad_len, rec_h,
                          rec_rows_h, status_h=None, open_len_h=None):
    """Receiver, host to host (qfec_open_decode_batch_host): wire packets pkt
    [G*(k+m)][stride], pkt_len int32 (< 0: not received) -> rec [G][min(k,m)][bb],
    rec_rows, status [G], open_len [G*(k+m)]."""
    G = rec_h.shape[0]
    n, rmax = G * (k + m), min(k, m)
    _check(pkt_h, "pkt", "uint8", (n, None), host=True)
    _check(pkt_len_h, "pkt_len", "int32", (n,), host=True)
    _check(ad_len, "ad_len", "int32", (n,), host=True)
    _check(rec_h, "rec", "uint8", (G, rmax, block_bytes), host=True)
    _check(rec_rows_h, "rec_rows", "uint8", (G, rmax), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    _check(open_len_h, "open_len", "int32", (n,), host=True, optional=True)
    a, a_all = _ptr_or_all(ad_len, True)
    return _call("qfec_open_decode_batch_host", engine, k, m, block_bytes, G, _ptr(pkt_h, True),
                 pkt_h.stride(0), _ptr(pkt_len_h, True), a, a_all, _ptr(rec_h, True),
                 _ptr(rec_rows_h, True), _ptr(status_h, True), _ptr(open_len_h, True))


def decode_recovered_host_into(engine, k, m, block_bytes, blocks_h, rows_h, rec_h, rec_rows_h,
                               status_h=None):
    """Host-pointer decode returning only the recovered blocks (CPU tensors)."""
    G, rmax = blocks_h.shape[0], min(k, m)
    _check(blocks_h, "blocks", "uint8", (G, k, block_bytes), host=True)
    _check(rows_h, "rows", "uint8", (G, k), host=True)
    _check(rec_h, "rec", "uint8", (G, rmax, block_bytes), host=True)
    _check(rec_rows_h, "rec_rows", "uint8", (G, rmax), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_decode_batch_recovered_host", engine, k, m, block_bytes, G,
                 _ptr(blocks_h, True), _ptr(rows_h, True), _ptr(rec_h, True),
                 _ptr(rec_rows_h, True), _ptr(status_h, True))


def _layout(name, k, m, G, *arrays):
    """One of the packed-layout calls (host only) over G groups: `arrays` are its numpy arrays
    ahead of the three offset arrays int64 [G] and the three totals, which are returned behind
    the call's code."""
    offs = [np.zeros(G, np.int64) for _ in range(3)]
    totals = np.zeros(3, np.int64)
    rc = getattr(load(), name)(k, m, G, *[_vp(a) for a in arrays + tuple(offs)], _vp(totals))
    return rc, offs, tuple(int(t) for t in totals)


def ragged_layout(k, m, bb):
    """The packed layout of groups with block sizes `bb` (qfec_ragged_layout; host only):
    (data_off, par_off, rec_off, totals), int64 arrays [G] of byte offsets (multiples of 16)
    and the three buffer sizes.  ValueError for a size < 1 or an overflow."""
    bb = np.ascontiguousarray(bb, dtype=np.int32)
    if bb.ndim != 1:
        raise ValueError("bb must be one-dimensional")
    rc, offs, totals = _layout("qfec_ragged_layout", k, m, bb.shape[0], bb)
    if rc:
        raise ValueError(f"qfec_ragged_layout: rc={rc} (k={k} m={m}, a size < 1 or overflow)")
    return offs[0], offs[1], offs[2], totals


def mixed_layout(codes, code, bb):
    """The packed layout of a mixed-code batch (qfec_mixed_layout; host only): group g has
    codes[code[g]] = (k_g, m_g) and block size bb[g].  Returns (data_off, par_off, rec_off,
    totals) as ragged_layout.  ValueError for a code index outside `codes`, a size < 1, a bad
    set or an overflow."""
    pairs, k, m = _codes(codes)
    code = np.ascontiguousarray(code, dtype=np.uint8)
    bb = np.ascontiguousarray(bb, dtype=np.int32)
    if code.ndim != 1 or bb.shape != code.shape:
        raise ValueError("code and bb must be one-dimensional and of one length")
    G = code.shape[0]
    offs = [np.zeros(G, np.int64) for _ in range(3)]
    totals = np.zeros(3, np.int64)
    rc = load().qfec_mixed_layout(len(pairs), _vp(k), _vp(m), G, _vp(code), _vp(bb),
                                  *[_vp(o) for o in offs], _vp(totals))
    if rc:
        raise ValueError(f"qfec_mixed_layout: rc={rc} (a code index outside the set, a size < 1, "
                         "a bad set or overflow)")
    return offs[0], offs[1], offs[2], tuple(int(t) for t in totals)


def framed_layout(k, m, pay_len):
    """The block sizes and the packed layout of framed groups (qfec_framed_layout; host only):
    pay_len int32 [G*k] -> (bb, data_off, par_off, rec_off, totals) with
    bb[g] = roundup8(max(pay_len of group g) + 2).  ValueError for a length outside
    [0, 0x3fff]."""
    pay_len = np.ascontiguousarray(pay_len, dtype=np.int32).reshape(-1)
    if pay_len.size % k:
        raise ValueError("pay_len must hold k lengths per group")
    G = pay_len.size // k
    bb = np.zeros(G, np.int32)
    rc, offs, totals = _layout("qfec_framed_layout", k, m, G, pay_len, bb)
    if rc:
        raise ValueError(f"qfec_framed_layout: rc={rc} (k={k} m={m}, a length outside "
                         "[0, 0x3fff] or overflow)")
    return bb, offs[0], offs[1], offs[2], totals


def framed_rx_block_bytes(k, m, pkt_len, ad_len):
    """The block size the reference's receiver gives each group (qfec_framed_rx_block_bytes;
    host only): pkt_len int32 [G*(k+m)] (< 0: not received), ad_len an int32 array of the same
    shape or an int -> bb int32 [G], the largest stored packet (a data packet's plaintext + 2, an
    FEC packet's plaintext), 0 for a group that received nothing."""
    pkt_len = np.ascontiguousarray(pkt_len, dtype=np.int32).reshape(-1)
    if pkt_len.size % (k + m):
        raise ValueError("pkt_len must hold k + m lengths per group")
    G = pkt_len.size // (k + m)
    if isinstance(ad_len, (int, np.integer)):
        ad_len, a_all = None, int(ad_len)
    else:
        ad_len, a_all = np.ascontiguousarray(ad_len, dtype=np.int32).reshape(-1), 0
        if ad_len.size != pkt_len.size:
            raise ValueError("ad_len must hold one length per packet")
    bb = np.zeros(G, np.int32)
    rc = load().qfec_framed_rx_block_bytes(k, m, G, _vp(pkt_len), _vp(ad_len), a_all, _vp(bb))
    if rc:
        raise ValueError(f"qfec_framed_rx_block_bytes: rc={rc} (k={k} m={m})")
    return bb


# what open_decode_extract_arrivals_ragged's arr_state says of an arrival that was not accepted
ARR_REJECTED, ARR_IGNORED, ARR_DUPLICATE, ARR_LATE = -1, -2, -3, -4


def arrivals_rx_block_bytes(k, m, groups, arr_group, arr_index, pkt_len, ad_len):
    """framed_rx_block_bytes for packets in arrival order (qfec_arrivals_rx_block_bytes; host
    only): arr_group int32 [n], arr_index uint8 [n], pkt_len int32 [n], ad_len an int32 array [n]
    or an int -> bb int32 [groups], the largest stored packet among each group's first k distinct
    arrivals, 0 for a group of which nothing arrived.  Tags outside the batch are skipped."""
    arr_group = np.ascontiguousarray(arr_group, dtype=np.int32).reshape(-1)
    arr_index = np.ascontiguousarray(arr_index, dtype=np.uint8).reshape(-1)
    pkt_len = np.ascontiguousarray(pkt_len, dtype=np.int32).reshape(-1)
    n = pkt_len.size
    if arr_group.size != n or arr_index.size != n:
        raise ValueError("arr_group, arr_index and pkt_len must hold one entry per arrival")
    if isinstance(ad_len, (int, np.integer)):
        ad_len, a_all = None, int(ad_len)
    else:
        ad_len, a_all = np.ascontiguousarray(ad_len, dtype=np.int32).reshape(-1), 0
        if ad_len.size != n:
            raise ValueError("ad_len must hold one length per arrival")
    bb = np.zeros(groups, np.int32)
    rc = load().qfec_arrivals_rx_block_bytes(k, m, groups, n, _vp(arr_group), _vp(arr_index),
                                             _vp(pkt_len), _vp(ad_len), a_all, _vp(bb))
    if rc:
        raise ValueError(f"qfec_arrivals_rx_block_bytes: rc={rc} (k={k} m={m} groups={groups})")
    return bb


# RxWindow.push's status of a group that does not complete in the push
WIN_OPEN, WIN_DELIVERED = -3, -5


def rxwin_bytes(k, m, groups, hold_stride):
    """Bytes of a receiver window's own device allocation (qfec_rxwin_bytes; host only)."""
    out = ctypes.c_longlong()
    rc = load().qfec_rxwin_bytes(k, m, groups, hold_stride, ctypes.byref(out))
    if rc:
        raise ValueError(f"qfec_rxwin_bytes: rc={rc} (k={k} m={m} groups={groups} "
                         f"hold_stride={hold_stride})")
    return out.value


def arrivals_rx_block_bytes_carry(k, m, groups, arr_group, arr_index, pkt_len, ad_len, seen, bb):
    """arrivals_rx_block_bytes fed in pieces (qfec_arrivals_rx_block_bytes_carry; host only):
    seen uint8 [groups][32] and bb int32 [groups] are C-contiguous numpy arrays updated in place
    (from zeros: a stream's pieces give what the one-shot helper gives over the whole stream; the
    caller zeroes a group's row of both when it releases it).  Returns bb."""
    arr_group = np.ascontiguousarray(arr_group, dtype=np.int32).reshape(-1)
    arr_index = np.ascontiguousarray(arr_index, dtype=np.uint8).reshape(-1)
    pkt_len = np.ascontiguousarray(pkt_len, dtype=np.int32).reshape(-1)
    n = pkt_len.size
    if arr_group.size != n or arr_index.size != n:
        raise ValueError("arr_group, arr_index and pkt_len must hold one entry per arrival")
    if isinstance(ad_len, (int, np.integer)):
        ad_len, a_all = None, int(ad_len)
    else:
        ad_len, a_all = np.ascontiguousarray(ad_len, dtype=np.int32).reshape(-1), 0
        if ad_len.size != n:
            raise ValueError("ad_len must hold one length per arrival")
    for name, arr, dtype, shape in (("seen", seen, np.uint8, (groups, 32)),
                                    ("bb", bb, np.int32, (groups,))):
        if not (isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.shape == shape
                and arr.flags.c_contiguous and arr.flags.writeable):
            raise ValueError(f"{name}: a writable C-contiguous {np.dtype(dtype).name} array "
                             f"{shape}")
    rc = load().qfec_arrivals_rx_block_bytes_carry(k, m, groups, n, _vp(arr_group),
                                                   _vp(arr_index), _vp(pkt_len), _vp(ad_len),
                                                   a_all, _vp(seen), _vp(bb))
    if rc:
        raise ValueError(f"qfec_arrivals_rx_block_bytes_carry: rc={rc} (k={k} m={m} "
                         f"groups={groups})")
    return bb


def mixed_packet_layout(codes, code):
    """The packet geometry of a mixed-code batch (qfec_mixed_packet_layout; host only): code
    uint8 [G] -> (pkt_first, pay_first), int32 [G+1] prefix tables: group g's wire packets and
    slots are pkt_first[g] .. pkt_first[g] + k_g + m_g - 1, its payload rows pay_first[g] ..
    pay_first[g] + k_g - 1.  A group with code[g] >= len(codes) gets an empty span in both.
    ValueError for a bad set or a total above INT32_MAX."""
    pairs, k, m = _codes(codes)
    code = np.ascontiguousarray(code, dtype=np.uint8)
    if code.ndim != 1:
        raise ValueError("code must be one-dimensional")
    G = code.shape[0]
    pkt_first, pay_first = np.zeros(G + 1, np.int32), np.zeros(G + 1, np.int32)
    rc = load().qfec_mixed_packet_layout(len(pairs), _vp(k), _vp(m), G, _vp(code),
                                         _vp(pkt_first), _vp(pay_first))
    if rc:
        raise ValueError(f"qfec_mixed_packet_layout: rc={rc} (a bad set, or more than INT32_MAX "
                         "packets)")
    return pkt_first, pay_first


def framed_layout_mixed(codes, code, pay_len, pay_first=None):
    """framed_layout with a code per group (qfec_framed_layout_mixed; host only): pay_len int32
    [npay] holds group g's k_g lengths at pay_first[g] (None: the dense table of
    mixed_packet_layout) -> (bb, data_off, par_off, rec_off, totals) with bb[g] =
    roundup8(max(the group's lengths) + 2) and mixed_layout's offsets.  ValueError for a length
    outside [0, 0x3fff], a span outside pay_len, or a code index outside the set."""
    pairs, k, m = _codes(codes)
    code = np.ascontiguousarray(code, dtype=np.uint8)
    pay_len = np.ascontiguousarray(pay_len, dtype=np.int32).reshape(-1)
    if code.ndim != 1:
        raise ValueError("code must be one-dimensional")
    G = code.shape[0]
    if pay_first is not None:
        pay_first = np.ascontiguousarray(pay_first, dtype=np.int32)
        if pay_first.shape != (G + 1,):
            raise ValueError("pay_first must hold G + 1 entries")
    bb = np.zeros(G, np.int32)
    offs = [np.zeros(G, np.int64) for _ in range(3)]
    totals = np.zeros(3, np.int64)
    rc = load().qfec_framed_layout_mixed(len(pairs), _vp(k), _vp(m), G, _vp(code), _vp(pay_first),
                                         pay_len.size, _vp(pay_len), _vp(bb),
                                         *[_vp(o) for o in offs], _vp(totals))
    if rc:
        raise ValueError(f"qfec_framed_layout_mixed: rc={rc} (a length outside [0, 0x3fff], a "
                         "span outside pay_len, a code index outside the set or overflow)")
    return bb, offs[0], offs[1], offs[2], tuple(int(t) for t in totals)


def arrivals_rx_block_bytes_mixed(codes, code, arr_group, arr_index, pkt_len, ad_len):
    """arrivals_rx_block_bytes with the k and k + m of each arrival's own group
    (qfec_arrivals_rx_block_bytes_mixed; host only): code uint8 [G] -> bb int32 [G].  Arrivals
    tagged to a group without a code are skipped."""
    pairs, k, m = _codes(codes)
    code = np.ascontiguousarray(code, dtype=np.uint8)
    if code.ndim != 1:
        raise ValueError("code must be one-dimensional")
    arr_group = np.ascontiguousarray(arr_group, dtype=np.int32).reshape(-1)
    arr_index = np.ascontiguousarray(arr_index, dtype=np.uint8).reshape(-1)
    pkt_len = np.ascontiguousarray(pkt_len, dtype=np.int32).reshape(-1)
    n = pkt_len.size
    if arr_group.size != n or arr_index.size != n:
        raise ValueError("arr_group, arr_index and pkt_len must hold one entry per arrival")
    if isinstance(ad_len, (int, np.integer)):
        ad_len, a_all = None, int(ad_len)
    else:
        ad_len, a_all = np.ascontiguousarray(ad_len, dtype=np.int32).reshape(-1), 0
        if ad_len.size != n:
            raise ValueError("ad_len must hold one length per arrival")
    bb = np.zeros(code.shape[0], np.int32)
    rc = load().qfec_arrivals_rx_block_bytes_mixed(len(pairs), _vp(k), _vp(m), code.shape[0],
                                                   _vp(code), n, _vp(arr_group), _vp(arr_index),
                                                   _vp(pkt_len), _vp(ad_len), a_all, _vp(bb))
    if rc:
        raise ValueError(f"qfec_arrivals_rx_block_bytes_mixed: rc={rc} (a bad set, or a code "
                         "with k + m > 255)")
    return bb


def _hcheck_ragged_one(n_blocks, bb_h, buf_h, off_h, name):
    """One packed host buffer of a ragged call: bb int32 [G] (every size >= 1), offsets int64
    [G] (non-negative multiples of 16), a flat uint8 buffer that holds every group the offsets
    name (n_blocks blocks each)."""
    import torch
    G = bb_h.shape[0] if isinstance(bb_h, torch.Tensor) and bb_h.dim() == 1 else None
    _check(bb_h, "bb", "int32", (G,), host=True)
    _check(off_h, f"{name}_off", "int64", (G,), host=True)
    _check(buf_h, name, "uint8", (None,), host=True)
    if int(bb_h.min()) < 1:
        raise ValueError("bb: every block size must be >= 1")
    if int(off_h.min()) < 0 or int((off_h % 16).max()) != 0:
        raise ValueError(f"{name}_off: offsets must be non-negative multiples of 16")
    if int((off_h + n_blocks * bb_h.to(torch.int64)).max()) > buf_h.numel():
        raise ValueError(f"{name}: buffer of {buf_h.numel()} bytes is too short for its groups")
    return G


def _hcheck_ragged(k, nout, bb_h, in_h, in_off_h, out_h, out_off_h):
    """Host arguments of a ragged codec call: its input and its output buffer."""
    G = _hcheck_ragged_one(k, bb_h, in_h, in_off_h, "in")
    _hcheck_ragged_one(nout, bb_h, out_h, out_off_h, "out")
    return G


def encode_ragged_host_into(engine, k, m, bb_h, data_h, data_off_h, parity_h, par_off_h,
                            status_h=None):
    """Host-pointer ragged encode on caller-owned CPU tensors (qfec_encode_batch_ragged_host):
    bb int32 [G], offsets int64 [G] (ascending, as ragged_layout gives them), data / parity flat
    uint8.  Returns 0 / -1."""
    G = _hcheck_ragged(k, m, bb_h, data_h, data_off_h, parity_h, par_off_h)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_encode_batch_ragged_host", engine, k, m, G, _ptr(bb_h, True),
                 _ptr(data_h, True), _ptr(data_off_h, True), _ptr(parity_h, True),
                 _ptr(par_off_h, True), _ptr(status_h, True), reference_rc=True)


def decode_ragged_recovered_host_into(engine, k, m, bb_h, blocks_h, blocks_off_h, rows_h, rec_h,
                                      rec_off_h, rec_rows_h, status_h=None):
    """Host-pointer ragged decode returning only the recovered blocks
    (qfec_decode_batch_ragged_recovered_host); rows [G][k], rec_rows [G][min(k,m)]."""
    rmax = min(k, m)
    G = _hcheck_ragged(k, rmax, bb_h, blocks_h, blocks_off_h, rec_h, rec_off_h)
    _check(rows_h, "rows", "uint8", (G, k), host=True)
    _check(rec_rows_h, "rec_rows", "uint8", (G, rmax), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_decode_batch_ragged_recovered_host", engine, k, m, G, _ptr(bb_h, True),
                 _ptr(blocks_h, True), _ptr(blocks_off_h, True), _ptr(rows_h, True),
                 _ptr(rec_h, True), _ptr(rec_off_h, True), _ptr(rec_rows_h, True),
                 _ptr(status_h, True))


def _hcheck_mixed(cs, code_h, bb_h, bufs):
    """Host arguments of a mixed-code call: code uint8 [G], bb int32 [G] (every size >= 1), and
    per packed buffer (name, tensor, offsets, blocks per code): offsets int64 [G], non-negative
    multiples of 16, inside the flat uint8 buffer.  A group whose code index names no code of
    the set holds no blocks."""
    import torch
    G = code_h.shape[0] if isinstance(code_h, torch.Tensor) and code_h.dim() == 1 else None
    _check(code_h, "code", "uint8", (G,), host=True)
    _check(bb_h, "bb", "int32", (G,), host=True)
    if int(bb_h.min()) < 1:
        raise ValueError("bb: every block size must be >= 1")
    for name, buf_h, off_h, per_code in bufs:
        _check(off_h, f"{name}_off", "int64", (G,), host=True)
        _check(buf_h, name, "uint8", (None,), host=True)
        if int(off_h.min()) < 0 or int((off_h % 16).max()) != 0:
            raise ValueError(f"{name}_off: offsets must be non-negative multiples of 16")
        counts = torch.tensor(list(per_code) + [0] * (256 - len(per_code)), dtype=torch.int64)
        if int((off_h + counts[code_h.long()] * bb_h.to(torch.int64)).max()) > buf_h.numel():
            raise ValueError(f"{name}: buffer of {buf_h.numel()} bytes is too short for its groups")
    return G


def encode_mixed_host_into(engine, cs, code_h, bb_h, data_h, data_off_h, parity_h, par_off_h,
                           status_h=None):
    """Host-pointer mixed-code encode on caller-owned CPU tensors (qfec_encode_batch_mixed_host):
    code uint8 [G], bb int32 [G], offsets int64 [G] (ascending, as mixed_layout gives them),
    data / parity flat uint8.  Returns 0: every rejection is per group."""
    G = _hcheck_mixed(cs, code_h, bb_h, [("data", data_h, data_off_h, [k for k, _ in cs.codes]),
                                         ("parity", parity_h, par_off_h, [m for _, m in cs.codes])])
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_encode_batch_mixed_host", engine, cs._h, G, _ptr(code_h, True),
                 _ptr(bb_h, True), _ptr(data_h, True), _ptr(data_off_h, True),
                 _ptr(parity_h, True), _ptr(par_off_h, True), _ptr(status_h, True))


def decode_mixed_recovered_host_into(engine, cs, code_h, bb_h, blocks_h, blocks_off_h, rows_h,
                                     rec_h, rec_off_h, rec_rows_h, status_h=None):
    """Host-pointer mixed-code decode returning only the recovered blocks
    (qfec_decode_batch_mixed_recovered_host); rows [G][cs.kmax], rec_rows [G][cs.rmax]."""
    G = _hcheck_mixed(cs, code_h, bb_h, [("blocks", blocks_h, blocks_off_h, [k for k, _ in cs.codes]),
                                         ("rec", rec_h, rec_off_h, [min(c) for c in cs.codes])])
    _check(rows_h, "rows", "uint8", (G, cs.kmax), host=True)
    _check(rec_rows_h, "rec_rows", "uint8", (G, cs.rmax), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    return _call("qfec_decode_batch_mixed_recovered_host", engine, cs._h, G, _ptr(code_h, True),
                 _ptr(bb_h, True), _ptr(blocks_h, True), _ptr(blocks_off_h, True),
                 _ptr(rows_h, True), _ptr(rec_h, True), _ptr(rec_off_h, True),
                 _ptr(rec_rows_h, True), _ptr(status_h, True))


def encode_seal_groups_ragged_host_into(engine, k, m, bb_h, data_h, data_off_h, hdr_h, hdr_len,
                                        pt_len, pkt_h, pkt_len_h, status_h=None):
    """Sender, host to host, a block size per group (qfec_encode_seal_groups_batch_ragged_host):
    bb int32 [G], data flat uint8 with offsets int64 [G] (ascending, as ragged_layout gives
    them); hdr [G*(k+m)][hdr_stride] (or None), pkt [G*(k+m)][pkt_stride], pkt_len int32
    [G*(k+m)], pt_len int32 [G*(k+m)] or None (whole blocks); status: optional int32 [G]."""
    G = _hcheck_ragged_one(k, bb_h, data_h, data_off_h, "data")
    n = G * (k + m)
    _check(hdr_h, "hdr", "uint8", (n, None), host=True, optional=True)
    _check(hdr_len, "hdr_len", "int32", (n,), host=True)
    _check(pt_len, "pt_len", "int32", (n,), host=True, optional=True)
    _check(pkt_h, "pkt", "uint8", (n, None), host=True)
    _check(pkt_len_h, "pkt_len", "int32", (n,), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    h, h_all = _ptr_or_all(hdr_len, True)
    return _call("qfec_encode_seal_groups_batch_ragged_host", engine, k, m, G, _ptr(bb_h, True),
                 _ptr(data_h, True), _ptr(data_off_h, True), _ptr(hdr_h, True), _stride(hdr_h), h,
                 h_all, _ptr(pt_len, True), _ptr(pkt_h, True), pkt_h.stride(0),
                 _ptr(pkt_len_h, True), _ptr(status_h, True))


def open_decode_ragged_host_into(engine, k, m, bb_h, pkt_h, pkt_len_h, ad_len, rec_h, rec_off_h,
                                 rec_rows_h, status_h=None, open_len_h=None):
    """Receiver, host to host, a block size per group (qfec_open_decode_batch_ragged_host):
    wire packets pkt [G*(k+m)][stride], pkt_len int32 (< 0: not received) -> rec (flat uint8,
    group g's up to [min(k,m)][bb[g]] at rec_off[g]; bytes not written keep their values),
    rec_rows [G][min(k,m)], status [G], open_len [G*(k+m)]."""
    rmax = min(k, m)
    G = _hcheck_ragged_one(rmax, bb_h, rec_h, rec_off_h, "rec")
    n = G * (k + m)
    _check(pkt_h, "pkt", "uint8", (n, None), host=True)
    _check(pkt_len_h, "pkt_len", "int32", (n,), host=True)
    _check(ad_len, "ad_len", "int32", (n,), host=True)
    _check(rec_rows_h, "rec_rows", "uint8", (G, rmax), host=True)
    _check(status_h, "status", "int32", (G,), host=True, optional=True)
    _check(open_len_h, "open_len", "int32", (n,), host=True, optional=True)
    a, a_all = _ptr_or_all(ad_len, True)
    return _call("qfec_open_decode_batch_ragged_host", engine, k, m, G, _ptr(bb_h, True),
                 _ptr(pkt_h, True), pkt_h.stride(0), _ptr(pkt_len_h, True), a, a_all,
                 _ptr(rec_h, True), _ptr(rec_off_h, True), _ptr(rec_rows_h, True),
                 _ptr(status_h, True), _ptr(open_len_h, True))


def synth_fill(t, seed, byte_offset=0, stream=None):
    """Fill a device tensor with the seeded splitmix64 stream (quic_amd.synth)."""
    rc = load().qfec_synth_fill(_ptr(t), t.numel() * t.element_size(), seed, byte_offset,
                                _stream(stream, t))
    if rc:
        raise FecError(rc, "qfec_synth_fill")


def synth_gather(data, parity, src, blocks, k, m, block_bytes, stream=None):
    """blocks[g][i] = sent block src[g][i] of group g (device-side receive-set build)."""
    rc = load().qfec_synth_gather(_ptr(data), _ptr(parity), _ptr(src), _ptr(blocks), k, m,
                                  block_bytes, data.shape[0], _stream(stream, data))
    if rc:
        raise FecError(rc, "qfec_synth_gather")
