#!/usr/bin/env python3
"""What the launchers launch: one line per engine call over a matrix of shapes, pointer
alignments, options and group counts.

    QFEC_LIB_PATH=<a build of libquic_fec.so> python3 tools/launch_matrix.py > matrix.txt

Per case: one engine, the options set, then one encode, one recovered-layout decode and one
slot-layout in-place decode on zeroed buffers; each prints qfec_last_kernels() and
qfec_last_grids().  Then, for EXTRA_SHAPES at 11 groups under default options: the ragged
encode and decode, the grouped seals and the open-decode (uniform and ragged; the opens read
what the seals wrote), the framed paths, one push into a receiver window and its release, and
every host form at host_chunk_mb = 1.  No assertions: the output is
for diffing against another build's.  Under
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
# the other entry points: m = 1, a preset, config B, k = 1
EXTRA_SHAPES = [(10, 1), (5, 5), (32, 4), (1, 3)]
# block sizes of the ragged calls' 11 groups: 12 is no multiple of 8 (the encode rejects it)
RAGGED_BB = [1352, 264, 8, 136, 1352, 520, 12, 1352, 72, 1000, 1352]
HDR = 16   # header bytes per packet


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

    call = lambda tag, f: report(tag, f, status)
    call("encode", lambda: eng.encode(k, m, bb, data, parity))
    call("recovered", lambda: eng.decode_recovered(k, m, bb, blocks, rows, rec, rec_rows, status))
    call("in-place", lambda: eng.decode(k, m, bb, blocks, rows, status=status))
    torch.cuda.synchronize()
    eng.close()


def report(tag, f, separator):
    separator.zero_()   # a kernel of torch's between two calls' kernels in a trace
    try:
        rc = f()
    except fec.FecError as e:
        rc = "error %d" % e.rc
    grids = ",".join("%s=%d" % kv for kv in fec.last_grids().items())
    print("  %-9s rc=%s kernels=[%s] grids=[%s]" % (tag, rc, fec.last_kernels(), grids))


def run_extra(k, m):
    """The ragged, packet-protection and host entry points, G_SMALL groups, default options."""
    G, bb, np_, rmax = G_SMALL, 1352, k + m, min(k, m)
    n, stride = G * np_, HDR + 12 + bb
    print("k=%d m=%d bb=%d G=%d offset=0 opts=extra" % (k, m, bb, G))
    eng = fec.FecEngine(0)
    eng.set_option("host_chunk_mb", 1)
    sep = torch.zeros(G, dtype=torch.int32, device="cuda")
    bbs = torch.tensor(RAGGED_BB, dtype=torch.int32)
    d_off, p_off, r_off, totals = (torch.from_numpy(a) if hasattr(a, "shape") else a
                                   for a in fec.ragged_layout(k, m, bbs.numpy()))

    def side(dev):
        """One set of buffers, on the device or the host."""
        z = lambda shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
        return dict(
            data=z((G, k, bb)), parity=z((G, m, bb)), blocks=z((G, k, bb)), rows=z((G, k)),
            rec=z((G, rmax, bb)), rec_rows=z((G, rmax)), status=z(G, torch.int32),
            hdr=z((n, HDR)), pkt=z((n, stride)), pkt_len=z(n, torch.int32),
            open_len=z(n, torch.int32), bb=bbs.to(dev), d_off=d_off.to(dev), p_off=p_off.to(dev),
            r_off=r_off.to(dev), rdata=z(totals[0] + 16), rparity=z(totals[1] + 16),
            rblocks=z(totals[0] + 16), rrec=z(totals[2] + 16))
    d, h = side("cuda"), side("cpu")
    call = lambda tag, f: report(tag, f, sep)
    call("r-encode", lambda: eng.encode_ragged(k, m, d["bb"], d["rdata"], d["d_off"], d["rparity"],
                                               d["p_off"], d["status"]))
    call("r-decode", lambda: eng.decode_ragged_recovered(
        k, m, d["bb"], d["rblocks"], d["d_off"], d["rows"], d["rrec"], d["r_off"], d["rec_rows"],
        d["status"]))
    for enc in (False, True):
        call("seal" + "+e" * enc, lambda: eng.seal_groups(
            k, m, bb, d["data"], d["parity"], d["hdr"], HDR, bb, d["pkt"], d["pkt_len"], encode=enc))
    call("open", lambda: eng.open_decode(k, m, bb, d["pkt"], d["pkt_len"], HDR, d["blocks"],
                                         d["rows"], d["open_len"], d["rec"], d["rec_rows"],
                                         d["status"]))
    for enc in (False, True):
        call("r-seal" + "+e" * enc, lambda: eng.seal_groups_ragged(
            k, m, d["bb"], d["rdata"], d["d_off"], d["rparity"], d["p_off"], d["hdr"], HDR, None,
            d["pkt"], d["pkt_len"], encode=enc, status=d["status"] if enc else None))
    call("r-open", lambda: eng.open_decode_ragged(
        k, m, d["bb"], d["pkt"], d["pkt_len"], HDR, d["rblocks"], d["d_off"], d["rows"],
        d["open_len"], d["rrec"], d["r_off"], d["rec_rows"], d["status"]))
    # the framed paths: payloads of RAGGED_BB[g] - 2 bytes (the group of 12 frames, and the encode
    # rejects it), the frame alone, frame + encode + seal, open + decode + extract, the extract
    pay = torch.zeros((G * k, bb), dtype=torch.uint8, device="cuda")
    pay_len = (bbs.repeat_interleave(k) - 2).to("cuda")
    rev = torch.zeros((G * rmax, bb), dtype=torch.uint8, device="cuda")
    rev_len = torch.zeros(G * rmax, dtype=torch.int32, device="cuda")
    call("f-frame", lambda: eng.frame_blocks_ragged(k, d["bb"], pay, pay_len, 1, d["rdata"],
                                                    d["d_off"], d["status"]))
    call("f-seal", lambda: eng.frame_encode_seal_ragged(
        k, m, d["bb"], d["rdata"], d["d_off"], d["rparity"], d["p_off"], d["hdr"], HDR, pay,
        pay_len, 1, d["pkt"], d["pkt_len"], status=d["status"]))
    call("f-open", lambda: eng.open_decode_extract_ragged(
        k, m, d["bb"], d["pkt"], d["pkt_len"], HDR, 1, d["rblocks"], d["d_off"], d["rows"],
        d["open_len"], d["rrec"], d["r_off"], d["rec_rows"], rev, rev_len, status=d["status"]))
    call("f-extract", lambda: eng.extract_revived_ragged(
        k, m, d["bb"], d["rrec"], d["r_off"], d["rec_rows"], d["status"], rev, rev_len))
    # the receiver window: the framed seal's packets as one in-order ring, then a release
    win = eng.rxwin(k, m, G, 1360)
    tags = torch.arange(n, device="cuda")
    grp, idx = (tags // np_).to(torch.int32), (tags % np_).to(torch.uint8)
    state = torch.zeros(n, dtype=torch.int32, device="cuda")
    call("w-push", lambda: win.push(d["bb"], d["pkt"], d["pkt_len"], HDR, 1, grp, idx, state,
                                    d["rrec"], d["r_off"], d["rec_rows"], rev, rev_len,
                                    status=d["status"]))
    call("w-release", lambda: win.release())
    win.close()
    call("h-encode", lambda: fec.encode_host_into(eng, k, m, bb, h["data"], h["parity"]))
    call("h-decode", lambda: fec.decode_host_into(eng, k, m, bb, h["blocks"], h["rows"], h["status"]))
    call("h-recov", lambda: fec.decode_recovered_host_into(
        eng, k, m, bb, h["blocks"], h["rows"], h["rec"], h["rec_rows"], h["status"]))
    call("h-seal", lambda: fec.encode_seal_groups_host_into(
        eng, k, m, bb, h["data"], h["hdr"], HDR, bb, h["pkt"], h["pkt_len"]))
    call("h-open", lambda: fec.open_decode_host_into(
        eng, k, m, bb, h["pkt"], h["pkt_len"], HDR, h["rec"], h["rec_rows"], h["status"],
        h["open_len"]))
    call("h-r-enc", lambda: fec.encode_ragged_host_into(
        eng, k, m, h["bb"], h["rdata"], h["d_off"], h["rparity"], h["p_off"], h["status"]))
    call("h-r-dec", lambda: fec.decode_ragged_recovered_host_into(
        eng, k, m, h["bb"], h["rblocks"], h["d_off"], h["rows"], h["rrec"], h["r_off"],
        h["rec_rows"], h["status"]))
    call("h-r-seal", lambda: fec.encode_seal_groups_ragged_host_into(
        eng, k, m, h["bb"], h["rdata"], h["d_off"], h["hdr"], HDR, None, h["pkt"], h["pkt_len"],
        h["status"]))
    call("h-r-open", lambda: fec.open_decode_ragged_host_into(
        eng, k, m, h["bb"], h["pkt"], h["pkt_len"], HDR, h["rrec"], h["r_off"], h["rec_rows"],
        h["status"], h["open_len"]))
    torch.cuda.synchronize()
    eng.close()


def main():
    if "--extra-only" in sys.argv[1:]:   # the other entry points alone
        for (k, m) in EXTRA_SHAPES:
            run_extra(k, m)
        return
    for (k, m, bb) in SHAPES:
        for offset in (0, 8):
            for opts in OPTIONS:
                run_case(k, m, bb, G_SMALL, offset, opts)
            # enough groups for every persistent grid to reach its cap: the *_wg defaults show
            run_case(k, m, bb, 512 if bb == 9008 else 8192, offset, {})
    for (k, m) in EXTRA_SHAPES:
        run_extra(k, m)


if __name__ == "__main__":
    main()
