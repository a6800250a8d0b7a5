#!/usr/bin/env python3
"""What the launchers launch: one line per engine call over a matrix of shapes, pointer
alignments, options and group counts.

    QFEC_LIB_PATH=<a build of libquic_fec.so> python3 tools/launch_matrix.py > matrix.txt

Per case: one engine, the options set, then one encode, one recovered-layout decode and one
slot-layout in-place decode on zeroed buffers; each prints qfec_last_kernels() and
qfec_last_grids().  No assertions: the output is for diffing against another build's.  Under
`rocprofv3 --kernel-trace --output-format csv -- python3 tools/launch_matrix.py` the trace adds
the kernel names, grids, workgroup sizes and LDS bytes the device saw; a torch fill before each
call separates the calls there.  tools/launch_matrix_reduce.py folds the two into the text that
profiles/launch_matrix/ keeps from the last launcher change.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from quic_amd import fec  # noqa: E402

COMPILED = [(32, 4), (5, 5), (10, 10), (10, 15), (10, 20), (15, 15), (250, 5)]
SHAPES = [(k, m, 1352) for k, m in COMPILED] + [
    (10, 6, 1352), (12, 12, 1352), (20, 9, 1352), (10, 20, 264), (40, 24, 1352),
    (17, 6, 136), (3, 2, 8), (16, 8, 9008), (128, 16, 9008), (10, 1, 1352), (1, 3, 1352)]

# tests/test_gpu_parity.py: OPTION_SETS, then test_reference_presets_stream's opts, then three more
OPTIONS = [
    {},
    {"xor_slots": 3, "xor_waves": 3}, {"xor_slots": 4, "xor_waves": 2}, {"xor_waves": 1},
    {"dma": 0}, {"stream": 0}, {"stream": 0, "pd": 1}, {"stream": 0, "pd": 3},
    {"stream": 0, "flat": 0}, {"enc_rc": 4}, {"enc_rc": 2}, {"prep_lane": 0},
    {"stream_ring": 36}, {"host_chunk_mb": 1, "host_min_groups": 1}, {"const_enc": 0},
    {"stream_static": 0}, {"bsyn": 0}, {"bsyn_depth": 5}, {"bsyn_depth": 7}, {"ring_split": 0},
    {"dcol": 0}, {"dcol_depth": 8}, {"psyn": 0},
    {"ring_wg": 0, "bsyn_wg": 0, "dcol_wg": 0, "stream_wg": 0},
    {"ring_wg": 3, "bsyn_wg": 5, "psyn_wg": 2, "dcol_wg": 1, "xor_wg": 3, "stream_wg": 2},
    {"stream_grid": 1}, {"psyn": 0, "stream_grid": 1}, {"ring_wide": 0},
    {"ring_wide": 0, "stream_grid": 1}, {"psyn_wide": 2}, {"psyn_wide": 0, "stream_grid": 1},
    {"psyn_wide": 0}, {"ring_wide": 0, "ring_split": 0}, {"const_enc": 0, "stream_static": 0},
]
G_SMALL = 11


def buf(shape, offset):
    """A zeroed uint8 device tensor whose pointer is `offset` bytes past an aligned one."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    return flat[offset:offset + n].view(*shape)


def run_case(k, m, bb, G, offset, opts):
    print("k=%d m=%d bb=%d G=%d offset=%d opts=%s" % (
        k, m, bb, G, offset, ",".join("%s=%d" % kv for kv in opts.items()) or "default"))
    eng = fec.FecEngine(0)
    for name, v in opts.items():
        eng.set_option(name, v)
    rmax = min(k, m)
    data, blocks = buf((G, k, bb), offset), buf((G, k, bb), offset)
    parity = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    rows = torch.zeros((G, k), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((G, rmax, bb), dtype=torch.uint8, device="cuda")
    rec_rows = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
    status = torch.zeros(G, dtype=torch.int32, device="cuda")

    def call(tag, f):
        status.zero_()   # a kernel of torch's between two calls' kernels in a trace
        try:
            rc = f()
        except fec.FecError as e:
            rc = "error %d" % e.rc
        grids = ",".join("%s=%d" % kv for kv in fec.last_grids().items())
        print("  %-9s rc=%s kernels=[%s] grids=[%s]" % (tag, rc, fec.last_kernels(), grids))

    call("encode", lambda: eng.encode(k, m, bb, data, parity))
    call("recovered", lambda: eng.decode_recovered(k, m, bb, blocks, rows, rec, rec_rows, status))
    call("in-place", lambda: eng.decode(k, m, bb, blocks, rows, status=status))
    torch.cuda.synchronize()
    eng.close()


def main():
    for (k, m, bb) in SHAPES:
        for offset in (0, 8):
            for opts in OPTIONS:
                run_case(k, m, bb, G_SMALL, offset, opts)
            # enough groups for every persistent grid to reach its cap: the *_wg defaults show
            run_case(k, m, bb, 512 if bb == 9008 else 8192, offset, {})


if __name__ == "__main__":
    main()
