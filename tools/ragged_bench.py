#!/usr/bin/env python3
"""Ragged batches against what the uniform entry points can do with the same groups.

Device-resident.  Every call is bracketed by the library's kernel timing events
(qfec_set_timing_events: first kernel start to last kernel end, as bench.py's roofline pass), so
a figure is kernel time, not enqueue time; the wall clock of the whole sequence (enqueue to
synchronise) is reported next to it, because the launch count is what the ragged path removes.
Warm-up, then the median of --reps repetitions, the variants alternating inside one repetition.

Workload (seeded): --groups groups of (32, 4) and of (10, 1); per group bb = 1352 with
probability 0.7, otherwise uniform over the multiples of 8 in [48, 1352].
  ragged    one qfec_encode_batch_ragged / qfec_decode_batch_ragged_recovered call
  buckets   the groups pre-sorted into per-bb uniform buffers (not timed) and one
            qfec_encode_batch / qfec_decode_batch_recovered per bucket: sum of the event times
Reference point: the ragged path with every bb = 1352 against the uniform compiled path.
Outputs of the two paths are compared byte for byte at the timed size before anything is timed.

--pp: the same workload through the protected paths, wire packets at both ends (whole-block
plaintexts, 16-byte headers; the receiver loses `losses` data packets per group):
  ragged    one qfec_encode_seal_groups_batch_ragged / qfec_open_decode_batch_ragged call
  buckets   one qfec_encode_seal_groups_batch / qfec_open_decode_batch per distinct bb
and every bb = 1352 against the one uniform call: the price of run-time shapes.

--framed: the price of framing on the device, on the mixed workload with
payload lengths bb - 2 down to bb - 9:
  framed    qfec_frame_encode_seal_groups_batch_ragged / qfec_open_decode_extract_batch_ragged
  unframed  qfec_encode_seal_groups_batch_ragged / qfec_open_decode_batch_ragged on the same
            (already framed) blocks
The parity of the two routes is compared byte for byte first (the wire data packets differ on
purpose: the framed ones carry no prefix).  The difference is set against the bytes the frame and
extract kernels move.

--arrivals: the arrival-order receiver on the --framed workload:
  slot      qfec_open_decode_extract_batch_ragged, every received packet at its slot
  arrivals  qfec_open_decode_extract_arrivals_ragged on the same packets as an in-order,
            duplicate-free ring (gathered once, not timed) with a (group, index) tag each
  two_read  the same call with the option arr_optimistic = 0: no data packet is placed by the
            open pass, the assemble reads every accepted packet a second time
  shuffled  the arrivals call on the same ring shuffled, with 5 % of its packets twice
The outputs of slot and arrivals are compared byte for byte first; the shuffled ring must revive
every lost payload.  The time ratio is set against the ratio of the bytes the two routes move.

--ptrs: the pointer-table batches against the packed ragged calls, the
same groups, data rows 0 .. r-1 lost:
  packed     qfec_encode_batch_ragged / qfec_decode_batch_ragged_recovered
  identity   qfec_encode_batch_ptrs / qfec_decode_batch_ptrs_recovered with tables that point into
             the same packed buffers
  scattered  the pointer form with every block placed on its own in a seeded random order, at
             16-byte aligned addresses (the receive set names the surviving data blocks and the
             parity blocks where they lie)
  unaligned  the same at addresses of every residue mod 16
The outputs of all four are compared byte for byte first.

--mixed-wire: the mixed-code wire path on the --mixed workload (the six
presets drawn uniformly, the size mix, two losses per group, an in-order ring), sender and
receiver, at 1,024 groups and at --groups:
  mixed   one qfec_frame_encode_seal_groups_batch_mixed / qfec_open_decode_extract_arrivals_mixed
  sorted  the same groups and arrivals pre-split by code (not timed), one ragged call per code
and the one-code (32, 4) set against the ragged call on identical input.  Wire packets, pkt_len,
arr_state, open_len, status, rec_rows and the revived payloads of the routes are compared byte
for byte first.
--window: the receiver window on the --arrivals workload's in-order ring:
  one_shot   qfec_open_decode_extract_arrivals_ragged over the whole ring
  window_P   the ring pushed into a window of --groups places in P = 1, 4 and 16 pieces (the sum
             of the pushes' times; the release between repetitions is not timed)
  empty      one push of no arrivals: the fixed cost of a push over all places
and a window of 4,096 places fed rings of about 16k packets.  arr_state, status, rec_rows, the
recovered blocks and the revived payloads are compared with the one-shot call's first.
--mixed: the mixed-code batches against the ragged calls, two losses per
group (data rows 0 and 1):
  mixed   one qfec_encode_batch_mixed / qfec_decode_batch_mixed_recovered call over groups drawn
          uniformly from the six presets (5,5) (10,10) (10,15) (10,20) (15,15) (250,5)
  sorted  the same groups pre-sorted by code into one packed buffer per code (not timed) and one
          qfec_encode_batch_ragged / qfec_decode_batch_ragged_recovered per code
at --groups groups (a) and at 1,024, the queue's scale (b); and a set of the one code (32, 4)
against the ragged call on identical input (c): the price of the per-group look-ups.  Outputs
are compared byte for byte first.

  python tools/ragged_bench.py --out profiles/ragged/ragged_bench.json
  python tools/ragged_bench.py --mixed --out profiles/ragged/mixed_bench.json
  python tools/ragged_bench.py --mixed-wire --out profiles/ragged/mixed_wire_bench.json
  python tools/ragged_bench.py --ptrs --out profiles/ragged/ptrs_bench.json
  python tools/ragged_bench.py --pp --out profiles/ragged/ragged_pp_bench.json
  python tools/ragged_bench.py --framed --out profiles/ragged/framed_bench.json
  python tools/ragged_bench.py --arrivals --out profiles/ragged/arrivals_bench.json
  python tools/ragged_bench.py --window --out profiles/ragged/window_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def draw_sizes(G, seed):
    rng = np.random.default_rng(seed)
    bb = np.full(G, 1352, np.int32)
    short = rng.random(G) >= 0.7
    bb[short] = 8 * rng.integers(6, 170, size=int(short.sum()))     # 48 .. 1352
    return bb


def views(flat, offs, sizes):
    return [flat[int(o):int(o) + int(n)] for o, n in zip(offs, sizes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--codes", default=None,
                    help="space-separated k,m,losses triples (default: 32,4,2 10,1,1; with "
                         "--ptrs also 10,10,5)")
    ap.add_argument("--pp", action="store_true",
                    help="the protected paths: ragged encode + seal and open -> decode against "
                         "one uniform protected call per distinct bb")
    ap.add_argument("--framed", action="store_true",
                    help="the framed protected paths against the unframed ragged ones")
    ap.add_argument("--arrivals", action="store_true",
                    help="the arrival-order receiver against the slot-order framed receiver")
    ap.add_argument("--window", action="store_true",
                    help="the receiver window (ring pushed whole, in 4 and in 16 pieces) against "
                         "the one-shot arrivals call; and a 4,096-group window fed 16k-packet rings")
    ap.add_argument("--ptrs", action="store_true",
                    help="the pointer-table batches against the packed ragged calls")
    ap.add_argument("--mixed", action="store_true",
                    help="the mixed-code batches against one ragged call per code")
    ap.add_argument("--mixed-wire", action="store_true",
                    help="the mixed-code wire path (framed sender, arrival-order receiver) against "
                         "one ragged call per code")
    ap.add_argument("--variants", default=None,
                    help="--arrivals: comma-separated subset of slot,arrivals,two_read,shuffled "
                         "to time (for a kernel trace of one route)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.codes is None:
        args.codes = "32,4,2 10,1,1" + (" 10,10,5" if args.ptrs else "")

    import torch
    from bench import DeviceEvents
    from quic_amd import _lib, fec
    if not torch.cuda.is_available():
        sys.exit("ragged_bench needs a GPU")
    lib = _lib.load()
    eng = fec.FecEngine(0)
    results = []

    def timed(ev, i, fn):
        lib.qfec_set_timing_events(ev.ev[2 * i], ev.ev[2 * i + 1])
        fn()
        lib.qfec_set_timing_events(None, None)

    def run_config(k, m, r, bb, label):
        G = len(bb)
        rmax = min(k, m)
        d_off, p_off, r_off, tot = fec.ragged_layout(k, m, bb)
        data = torch.empty(tot[0], dtype=torch.uint8, device="cuda")
        fec.synth_fill(data, seed=args.seed)
        par = torch.zeros(tot[1], dtype=torch.uint8, device="cuda")
        rec = torch.zeros(tot[2], dtype=torch.uint8, device="cuda")
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        # receive set: slot i < r holds parity row i (data rows 0 .. r-1 lost)
        rows_np = np.tile(np.arange(k, dtype=np.uint8), (G, 1))
        rows_np[:, :r] = k + np.arange(r, dtype=np.uint8)
        rows = torch.from_numpy(rows_np).cuda()
        rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
        st = torch.zeros(G, dtype=torch.int32, device="cuda")

        assert eng.encode_ragged(k, m, bb_d, data, d_off_d, par, p_off_d) == 0
        blocks = data.clone()
        torch._foreach_copy_(views(blocks, d_off, r * bb.astype(np.int64)),
                             views(par, p_off, r * bb.astype(np.int64)))
        eng.decode_ragged_recovered(k, m, bb_d, blocks, d_off_d, rows, rec, r_off_d, rr, status=st)
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0
        kern = {"ragged_encode": None, "ragged_decode": fec.last_kernels()}

        # the parent's route: per-bb buckets, gathered once (not timed)
        buckets = []
        for b in np.unique(bb):
            idx = np.nonzero(bb == b)[0]
            b = int(b)
            Gb = len(idx)
            bd = torch.stack(views(data, d_off[idx], [k * b] * Gb)).view(Gb, k, b)
            bbk = torch.stack(views(blocks, d_off[idx], [k * b] * Gb)).view(Gb, k, b)
            buckets.append(dict(
                bb=b, G=Gb, idx=idx, data=bd, blocks=bbk, rows=rows[torch.from_numpy(idx).cuda()],
                par=torch.zeros((Gb, m, b), dtype=torch.uint8, device="cuda"),
                rec=torch.zeros((Gb, rmax, b), dtype=torch.uint8, device="cuda"),
                rr=torch.zeros((Gb, rmax), dtype=torch.uint8, device="cuda"),
                st=torch.zeros(Gb, dtype=torch.int32, device="cuda")))
        nb = len(buckets)

        def bucket_encode(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.encode(k, m, B["bb"], B["data"], B["par"])
                timed(ev, base + i, f) if ev else f()

        def bucket_decode(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.decode_recovered(k, m, B["bb"], B["blocks"], B["rows"], B["rec"],
                                                 B["rr"], status=B["st"])
                timed(ev, base + i, f) if ev else f()

        def ragged_encode():
            eng.encode_ragged(k, m, bb_d, data, d_off_d, par, p_off_d)

        def ragged_decode():
            eng.decode_ragged_recovered(k, m, bb_d, blocks, d_off_d, rows, rec, r_off_d, rr,
                                        status=st)

        # same bytes from both paths, at the timed size
        bucket_encode()
        bucket_decode()
        torch.cuda.synchronize()
        for B in buckets:
            idx, b, Gb = B["idx"], B["bb"], B["G"]
            assert torch.equal(torch.stack(views(par, p_off[idx], [m * b] * Gb)).view(Gb, m, b),
                               B["par"]), "parity differs between the paths"
            assert torch.equal(torch.stack(views(rec, r_off[idx], [r * b] * Gb)).view(Gb, r, b),
                               B["rec"][:, :r]), "recovered blocks differ between the paths"
            assert torch.equal(torch.stack(views(rec, r_off[idx], [r * b] * Gb)).view(Gb, r, b),
                               B["data"][:, :r]), "recovered blocks are not the lost data"
        ragged_encode()
        kern["ragged_encode"] = fec.last_kernels()

        # events: [0] ragged enc, [1] ragged dec, [2 .. 2+nb) bucket enc, then bucket dec
        ev = DeviceEvents(2 * (2 + 2 * nb))
        t = {x: [] for x in ("ragged_encode", "ragged_decode", "bucket_encode", "bucket_decode")}
        wall = {x: [] for x in t}

        def walled(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)

        for rep in range(args.warmup + args.reps):
            order = [("ragged_encode", lambda: timed(ev, 0, ragged_encode)),
                     ("bucket_encode", lambda: bucket_encode(ev, 2)),
                     ("ragged_decode", lambda: timed(ev, 1, ragged_decode)),
                     ("bucket_decode", lambda: bucket_decode(ev, 2 + nb))]
            if rep % 2:
                order = [order[1], order[0], order[3], order[2]]
            for name, fn in order:
                walled(name, fn)
            if rep < args.warmup:
                for x in wall:
                    wall[x].clear()
                continue
            t["ragged_encode"].append(ev.elapsed_ms(0, 1))
            t["ragged_decode"].append(ev.elapsed_ms(2, 3))
            t["bucket_encode"].append(sum(ev.elapsed_ms(2 * (2 + i), 2 * (2 + i) + 1)
                                          for i in range(nb)))
            t["bucket_decode"].append(sum(ev.elapsed_ms(2 * (2 + nb + i), 2 * (2 + nb + i) + 1)
                                          for i in range(nb)))
        ev.close()
        total = int(bb.astype(np.int64).sum())
        nbytes = {"encode": (k + m) * total, "decode": (k + r) * total}
        line = dict(config=label, k=k, m=m, losses=r, groups=G, distinct_bb=nb,
                    uniform_launches_per_phase=nb, reps=args.reps, kernels=kern,
                    bytes_moved=nbytes)
        for name, v in t.items():
            med = statistics.median(v)
            by = nbytes["encode" if name.endswith("encode") else "decode"]
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(v), 4),
                              kernel_ms_max=round(max(v), 4),
                              wall_ms_median=round(statistics.median(wall[name]), 4),
                              GBps=round(by / (med * 1e-3) / 1e9, 1),
                              hbm_fraction=round(by / (med * 1e-3) / HBM_BYTES_PER_S, 4))
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_pp(k, m, r, bb, label):
        """--pp: the protected paths.  Sender: encode + seal of every packet (whole-block
        plaintexts, 16-byte headers); receiver: open -> decode with data packets 0 .. r-1 of
        every group lost.  ragged: one qfec_encode_seal_groups_batch_ragged /
        qfec_open_decode_batch_ragged call; buckets: one qfec_encode_seal_groups_batch /
        qfec_open_decode_batch per distinct bb on pre-gathered buffers."""
        G, per, rmax, H = len(bb), k + m, min(k, m), 16
        n = G * per
        stride = H + 12 + int(bb.max())
        assert stride % 4 == 0
        d_off, p_off, r_off, tot = fec.ragged_layout(k, m, bb)
        data = torch.empty(tot[0], dtype=torch.uint8, device="cuda")
        fec.synth_fill(data, seed=args.seed)
        par = torch.zeros(tot[1], dtype=torch.uint8, device="cuda")
        rec = torch.zeros(tot[2], dtype=torch.uint8, device="cuda")
        blocks = torch.zeros(tot[0], dtype=torch.uint8, device="cuda")
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        hdr = torch.randint(0, 256, (n, H), dtype=torch.uint8, device="cuda")
        pkt = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        pkt_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        est = torch.zeros(G, dtype=torch.int32, device="cuda")
        rows = torch.zeros((G, k), dtype=torch.uint8, device="cuda")
        ol = torch.zeros(n, dtype=torch.int32, device="cuda")
        rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
        st = torch.zeros(G, dtype=torch.int32, device="cuda")

        def ragged_seal():
            eng.seal_groups_ragged(k, m, bb_d, data, d_off_d, par, p_off_d, hdr, H, None, pkt,
                                   pkt_len, encode=True, status=est)

        ragged_seal()
        kern = {"ragged_seal": fec.last_kernels()}
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0 and int(pkt_len.min()) >= H + 12
        wire_len = pkt_len.clone().view(G, per)
        wire_len[:, :r] = -1                                  # data packets 0 .. r-1 lost
        wire_len = wire_len.view(n)

        def ragged_open():
            eng.open_decode_ragged(k, m, bb_d, pkt, wire_len, H, blocks, d_off_d, rows, ol, rec,
                                   r_off_d, rr, status=st)

        ragged_open()
        kern["ragged_open"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0

        buckets = []
        for b in np.unique(bb):
            idx = np.nonzero(bb == b)[0]
            b, Gb = int(b), len(idx)
            pidx = torch.from_numpy((idx[:, None] * per + np.arange(per)[None, :]).ravel()).cuda()
            bs = H + 12 + b
            buckets.append(dict(
                bb=b, G=Gb, idx=idx, pidx=pidx,
                data=torch.stack(views(data, d_off[idx], [k * b] * Gb)).view(Gb, k, b),
                hdr=hdr[pidx].contiguous(),
                wire=pkt[pidx][:, :bs].contiguous(), wire_len=wire_len[pidx].contiguous(),
                par=torch.zeros((Gb, m, b), dtype=torch.uint8, device="cuda"),
                pkt=torch.zeros((Gb * per, bs), dtype=torch.uint8, device="cuda"),
                pkt_len=torch.zeros(Gb * per, dtype=torch.int32, device="cuda"),
                blocks=torch.zeros((Gb, k, b), dtype=torch.uint8, device="cuda"),
                rows=torch.zeros((Gb, k), dtype=torch.uint8, device="cuda"),
                ol=torch.zeros(Gb * per, dtype=torch.int32, device="cuda"),
                rec=torch.zeros((Gb, rmax, b), dtype=torch.uint8, device="cuda"),
                rr=torch.zeros((Gb, rmax), dtype=torch.uint8, device="cuda"),
                st=torch.zeros(Gb, dtype=torch.int32, device="cuda")))
        nb = len(buckets)

        def bucket_seal(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.seal_groups(k, m, B["bb"], B["data"], B["par"], B["hdr"], H,
                                            B["bb"], B["pkt"], B["pkt_len"], encode=True)
                timed(ev, base + i, f) if ev else f()

        def bucket_open(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.open_decode(k, m, B["bb"], B["wire"], B["wire_len"], H,
                                            B["blocks"], B["rows"], B["ol"], B["rec"], B["rr"],
                                            status=B["st"])
                timed(ev, base + i, f) if ev else f()

        # the same bytes from both paths, at the timed size
        bucket_seal()
        kern["bucket_seal"] = fec.last_kernels()
        bucket_open()
        kern["bucket_open"] = fec.last_kernels()
        torch.cuda.synchronize()
        for B in buckets:
            idx, b, Gb = B["idx"], B["bb"], B["G"]
            assert torch.equal(B["pkt"], B["wire"]), "sealed packets differ between the paths"
            assert torch.equal(B["pkt_len"], pkt_len[B["pidx"]]), "packet lengths differ"
            assert torch.equal(B["ol"], ol[B["pidx"]]), "open lengths differ"
            got = torch.stack(views(rec, r_off[idx], [r * b] * Gb)).view(Gb, r, b)
            assert torch.equal(got, B["rec"][:, :r]), "recovered blocks differ between the paths"
            assert torch.equal(got, B["data"][:, :r]), "recovered blocks are not the lost data"

        ev = DeviceEvents(2 * (2 + 2 * nb))
        t = {x: [] for x in ("ragged_seal", "ragged_open", "bucket_seal", "bucket_open")}
        wall = {x: [] for x in t}

        def walled(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)

        for rep in range(args.warmup + args.reps):
            order = [("ragged_seal", lambda: timed(ev, 0, ragged_seal)),
                     ("bucket_seal", lambda: bucket_seal(ev, 2)),
                     ("ragged_open", lambda: timed(ev, 1, ragged_open)),
                     ("bucket_open", lambda: bucket_open(ev, 2 + nb))]
            if rep % 2:
                order = [order[1], order[0], order[3], order[2]]
            for name, fn in order:
                walled(name, fn)
            if rep < args.warmup:
                for x in wall:
                    wall[x].clear()
                continue
            t["ragged_seal"].append(ev.elapsed_ms(0, 1))
            t["ragged_open"].append(ev.elapsed_ms(2, 3))
            t["bucket_seal"].append(sum(ev.elapsed_ms(2 * (2 + i), 2 * (2 + i) + 1)
                                        for i in range(nb)))
            t["bucket_open"].append(sum(ev.elapsed_ms(2 * (2 + nb + i), 2 * (2 + nb + i) + 1)
                                        for i in range(nb)))
        ev.close()
        total = int(bb.astype(np.int64).sum())
        # wire bytes: every packet sealed / every received packet opened
        nbytes = {"seal": per * (total + G * (H + 12)), "open": (per - r) * (total + G * (H + 12))}
        line = dict(config=label, mode="pp", k=k, m=m, losses=r, groups=G, packets=n,
                    distinct_bb=nb, uniform_calls_per_phase=nb, reps=args.reps, kernels=kern,
                    wire_bytes=nbytes)
        for name, v in t.items():
            med = statistics.median(v)
            by = nbytes["seal" if name.endswith("seal") else "open"]
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(v), 4),
                              kernel_ms_max=round(max(v), 4),
                              wall_ms_median=round(statistics.median(wall[name]), 4),
                              wire_GBps=round(by / (med * 1e-3) / 1e9, 1))
        for ph in ("seal", "open"):
            line[f"{ph}_kernel_speedup_vs_buckets"] = round(
                line[f"bucket_{ph}"]["kernel_ms_median"] / line[f"ragged_{ph}"]["kernel_ms_median"], 3)
            line[f"{ph}_wall_speedup_vs_buckets"] = round(
                line[f"bucket_{ph}"]["wall_ms_median"] / line[f"ragged_{ph}"]["wall_ms_median"], 3)
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_framed(k, m, r, bb, label):
        """--framed: frame -> encode -> seal against encode -> seal, and open -> decode ->
        extract against open -> decode, the same groups, data packets 0 .. r-1 lost."""
        G, per, rmax, H = len(bb), k + m, min(k, m), 16
        n = G * per
        stride = H + 12 + int(bb.max())
        pay_stride = int(bb.max())
        rng = np.random.default_rng(args.seed + 1)
        lens = (np.repeat(bb, k) - 2 - rng.integers(0, 8, G * k)).astype(np.int32)
        fbb, d_off, p_off, r_off, tot = fec.framed_layout(k, m, lens)
        assert np.array_equal(fbb, bb)
        pay = torch.empty((G * k, pay_stride), dtype=torch.uint8, device="cuda")
        fec.synth_fill(pay, seed=args.seed)
        lens_d = torch.from_numpy(lens).cuda()
        data = torch.zeros(tot[0], dtype=torch.uint8, device="cuda")
        par = {x: torch.zeros(tot[1], dtype=torch.uint8, device="cuda") for x in "fu"}
        rec = {x: torch.zeros(tot[2], dtype=torch.uint8, device="cuda") for x in "fu"}
        blocks = torch.zeros(tot[0], dtype=torch.uint8, device="cuda")
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        hdr = torch.randint(0, 256, (n, H), dtype=torch.uint8, device="cuda")
        pkt = {x: torch.zeros((n, stride), dtype=torch.uint8, device="cuda") for x in "fu"}
        plen = {x: torch.zeros(n, dtype=torch.int32, device="cuda") for x in "fu"}
        est = torch.zeros(G, dtype=torch.int32, device="cuda")
        rows = torch.zeros((G, k), dtype=torch.uint8, device="cuda")
        ol = torch.zeros(n, dtype=torch.int32, device="cuda")
        rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
        st = torch.zeros(G, dtype=torch.int32, device="cuda")
        rev = torch.zeros((G * rmax, pay_stride), dtype=torch.uint8, device="cuda")
        rev_len = torch.zeros(G * rmax, dtype=torch.int32, device="cuda")
        rev_pn = torch.zeros(G * rmax, dtype=torch.uint8, device="cuda")

        def framed_seal():
            eng.frame_encode_seal_ragged(k, m, bb_d, data, d_off_d, par["f"], p_off_d, hdr, H, pay,
                                         lens_d, 1, pkt["f"], plen["f"], status=est)

        def unframed_seal():
            eng.seal_groups_ragged(k, m, bb_d, data, d_off_d, par["u"], p_off_d, hdr, H, None,
                                   pkt["u"], plen["u"], encode=True, status=est)

        framed_seal()
        kern = {"framed_seal": fec.last_kernels()}
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0
        unframed_seal()                                       # on the blocks the frame wrote
        kern["unframed_seal"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert torch.equal(par["f"], par["u"]), "parity differs between the routes"
        wl = {}
        for x in "fu":
            w = plen[x].clone().view(G, per)
            w[:, :r] = -1
            wl[x] = w.view(n)

        def framed_open():
            eng.open_decode_extract_ragged(k, m, bb_d, pkt["f"], wl["f"], H, 1, blocks, d_off_d,
                                           rows, ol, rec["f"], r_off_d, rr, rev, rev_len,
                                           rev_pn_len=rev_pn, status=st)

        def unframed_open():
            eng.open_decode_ragged(k, m, bb_d, pkt["u"], wl["u"], H, blocks, d_off_d, rows, ol,
                                   rec["u"], r_off_d, rr, status=st)

        framed_open()
        kern["framed_open"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0
        lost = torch.arange(G, device="cuda")[:, None] * k + torch.arange(r, device="cuda")[None, :]
        got = rev_len.view(G, rmax)[:, :r]
        assert torch.equal(got, lens_d[lost]), "revived lengths are not the lost payloads'"
        cols = torch.arange(pay_stride, device="cuda")[None, None, :]
        mask = cols < got[:, :, None]
        assert torch.equal(rev.view(G, rmax, pay_stride)[:, :r][mask], pay[lost][mask]), \
            "revived payloads are not the lost ones"
        unframed_open()
        kern["unframed_open"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(st.abs().max()) == 0 and torch.equal(rec["f"], rec["u"])

        names = ["framed_seal", "unframed_seal", "framed_open", "unframed_open"]
        fns = dict(framed_seal=framed_seal, unframed_seal=unframed_seal, framed_open=framed_open,
                   unframed_open=unframed_open)
        ev = DeviceEvents(2 * len(names))
        t = {x: [] for x in names}
        for rep_i in range(args.warmup + args.reps):
            order = names if rep_i % 2 == 0 else [names[1], names[0], names[3], names[2]]
            for name in order:
                timed(ev, names.index(name), fns[name])
            torch.cuda.synchronize()
            if rep_i >= args.warmup:
                for i, name in enumerate(names):
                    t[name].append(ev.elapsed_ms(2 * i, 2 * i + 1))
        ev.close()
        total = int(bb.astype(np.int64).sum())
        frame_bytes = int(lens.astype(np.int64).sum()) + k * total
        extract_bytes = 2 * r * total
        line = dict(config=label, mode="framed", k=k, m=m, losses=r, groups=G, packets=n,
                    reps=args.reps, kernels=kern,
                    wire_bytes={"seal": per * (total + G * (H + 12)),
                                "open": (per - r) * (total + G * (H + 12))},
                    frame_kernel_bytes=frame_bytes, extract_kernel_bytes=extract_bytes)
        for name in names:
            med = statistics.median(t[name])
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(t[name]), 4),
                              kernel_ms_max=round(max(t[name]), 4))
        for ph, extra in (("seal", frame_bytes), ("open", extract_bytes)):
            f, u = line[f"framed_{ph}"]["kernel_ms_median"], line[f"unframed_{ph}"]["kernel_ms_median"]
            line[f"{ph}_framing_ms"] = round(f - u, 4)
            line[f"{ph}_framed_over_unframed"] = round(f / u, 3)
            # what the extra bytes alone would cost at the unframed route's own byte rate
            base = line["wire_bytes"][ph] * 2
            line[f"{ph}_byte_ratio"] = round((base + extra) / base, 3)
            line[f"{ph}_framing_GBps"] = round(extra / max(f - u, 1e-6) / 1e6, 1)
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_arrivals(k, m, r, bb, label):
        """--arrivals: the framed receiver by slot against the arrivals call on the same received
        packets as a ring, data packets 0 .. r-1 of every group lost."""
        G, per, rmax, H = len(bb), k + m, min(k, m), 16
        n = G * per
        stride = H + 12 + int(bb.max())
        pay_stride = int(bb.max())
        rng = np.random.default_rng(args.seed + 1)
        lens = (np.repeat(bb, k) - 2 - rng.integers(0, 8, G * k)).astype(np.int32)
        fbb, d_off, p_off, r_off, tot = fec.framed_layout(k, m, lens)
        assert np.array_equal(fbb, bb)
        pay = torch.empty((G * k, pay_stride), dtype=torch.uint8, device="cuda")
        fec.synth_fill(pay, seed=args.seed)
        lens_d = torch.from_numpy(lens).cuda()
        data = torch.zeros(tot[0], dtype=torch.uint8, device="cuda")
        par = torch.zeros(tot[1], dtype=torch.uint8, device="cuda")
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        hdr = torch.randint(0, 256, (n, H), dtype=torch.uint8, device="cuda")
        pkt = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        plen = torch.zeros(n, dtype=torch.int32, device="cuda")
        est = torch.zeros(G, dtype=torch.int32, device="cuda")
        eng.frame_encode_seal_ragged(k, m, bb_d, data, d_off_d, par, p_off_d, hdr, H, pay, lens_d,
                                     1, pkt, plen, status=est)
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0
        del data, par, hdr
        wl = plen.clone().view(G, per)
        wl[:, :r] = -1
        wl = wl.view(n)

        def outputs():
            return dict(blocks=torch.zeros(tot[0], dtype=torch.uint8, device="cuda"),
                        rec=torch.zeros(tot[2], dtype=torch.uint8, device="cuda"),
                        rows=torch.zeros((G, k), dtype=torch.uint8, device="cuda"),
                        ol=torch.zeros(n, dtype=torch.int32, device="cuda"),
                        rr=torch.zeros((G, rmax), dtype=torch.uint8, device="cuda"),
                        st=torch.zeros(G, dtype=torch.int32, device="cuda"),
                        rev=torch.zeros((G * rmax, pay_stride), dtype=torch.uint8, device="cuda"),
                        rev_len=torch.zeros(G * rmax, dtype=torch.int32, device="cuda"),
                        rev_pn=torch.zeros(G * rmax, dtype=torch.uint8, device="cuda"))

        # the rings (gathered once, not timed): the received packets in slot order, and the same
        # packets shuffled with 5 % of them twice
        recv = torch.nonzero(wl >= 0).view(-1)
        dup = recv[torch.from_numpy(rng.choice(recv.numel(), recv.numel() // 20,
                                               replace=False)).cuda()]
        mixed_src = torch.cat([recv, dup])[torch.from_numpy(
            rng.permutation(recv.numel() + dup.numel())).cuda()]

        def ring_of(src):
            return dict(n=src.numel(), pkt=pkt[src].contiguous(), len=plen[src].contiguous(),
                        grp=(src // per).to(torch.int32), idx=(src % per).to(torch.uint8),
                        state=torch.zeros(src.numel(), dtype=torch.int32, device="cuda"),
                        at=torch.zeros(n, dtype=torch.int32, device="cuda"))

        rings = dict(arrivals=ring_of(recv), shuffled=ring_of(mixed_src))
        out = dict(slot=outputs(), arrivals=outputs())
        out["shuffled"] = out["arrivals"]

        def slot():
            o = out["slot"]
            eng.open_decode_extract_ragged(k, m, bb_d, pkt, wl, H, 1, o["blocks"], d_off_d,
                                           o["rows"], o["ol"], o["rec"], r_off_d, o["rr"], o["rev"],
                                           o["rev_len"], rev_pn_len=o["rev_pn"], status=o["st"])

        def arrivals_call(name, optimistic=1):
            R, o = rings[name], out[name]
            eng.set_option("arr_optimistic", optimistic)
            eng.open_decode_extract_arrivals_ragged(
                k, m, bb_d, R["pkt"], R["len"], H, 1, R["grp"], R["idx"], R["state"], R["at"],
                o["blocks"], d_off_d, o["rows"], o["ol"], o["rec"], r_off_d, o["rr"], o["rev"],
                o["rev_len"], rev_pn_len=o["rev_pn"], status=o["st"])
            eng.set_option("arr_optimistic", 1)

        def revives_lost(o):
            lost = torch.arange(G, device="cuda")[:, None] * k + \
                torch.arange(r, device="cuda")[None, :]
            got = o["rev_len"].view(G, rmax)[:, :r]
            cols = torch.arange(pay_stride, device="cuda")[None, None, :]
            mask = cols < got[:, :, None]
            return int(o["st"].abs().max()) == 0 and torch.equal(got, lens_d[lost]) and \
                torch.equal(o["rev"].view(G, rmax, pay_stride)[:, :r][mask], pay[lost][mask])

        kern = {}
        slot()
        kern["slot"] = fec.last_kernels()
        arrivals_call("arrivals")
        kern["arrivals"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert revives_lost(out["slot"]), "the slot route does not revive the lost payloads"
        a, b = out["slot"], out["arrivals"]

        def same_as_slot():
            for name in ("blocks", "rec", "rows", "rr", "st", "rev", "rev_len", "rev_pn"):
                assert torch.equal(a[name], b[name]), f"{name} differs between the routes"
            # open_len: the arrivals route marks the FEC packets behind the k-th as late
            taken = rings["arrivals"]["at"] >= 0
            assert torch.equal(a["ol"][taken], b["ol"][taken]) and int(b["ol"][~taken].max()) == -1

        same_as_slot()
        states = rings["arrivals"]["state"]
        accepted = int((states >= 0).sum())
        assert accepted == G * k and int((states == -4).sum()) == recv.numel() - G * k
        # plaintext bytes the assemble reads: every accepted packet's, or (optimistic) those of
        # the accepted FEC packets alone
        second_read2 = int(states[states >= 0].sum())
        second_read = int(states[(states >= 0) & (rings["arrivals"]["idx"] >= k)].sum())
        for o in b.values():
            o.zero_()
        arrivals_call("arrivals", 0)
        kern["two_read"] = fec.last_kernels()
        torch.cuda.synchronize()
        same_as_slot()
        arrivals_call("shuffled")
        torch.cuda.synchronize()
        assert revives_lost(out["shuffled"]), "the shuffled ring does not revive the lost payloads"
        sh = rings["shuffled"]["state"]
        shuffled = dict(arrivals=rings["shuffled"]["n"], accepted=int((sh >= 0).sum()),
                        duplicate=int((sh == -3).sum()), late=int((sh == -4).sum()),
                        revived=int((out["shuffled"]["rev_len"] >= 0).sum()),
                        accepted_plaintext_bytes=int(sh[sh >= 0].sum()))

        names = ["slot", "arrivals", "two_read", "shuffled"]
        timed_names = args.variants.split(",") if args.variants else names
        assert set(timed_names) <= set(names)
        fns = dict(slot=slot, arrivals=lambda: arrivals_call("arrivals"),
                   two_read=lambda: arrivals_call("arrivals", 0),
                   shuffled=lambda: arrivals_call("shuffled"))
        ev = DeviceEvents(2 * len(names))
        t = {x: [] for x in names}
        for rep_i in range(args.warmup + args.reps):
            order = names if rep_i % 2 == 0 else [names[2], names[1], names[0], names[3]]
            for name in order:
                if name in timed_names:
                    timed(ev, names.index(name), fns[name])
            torch.cuda.synchronize()
            if rep_i >= args.warmup:
                for i, name in enumerate(names):
                    t[name].append(ev.elapsed_ms(2 * i, 2 * i + 1) if name in timed_names else 0.0)
        ev.close()
        # bytes each route moves, from the shapes: T = the blocks' bytes of one block per group
        T = int(bb.astype(np.int64).sum())
        wire = int(plen[recv].to(torch.int64).sum())
        after_open = (k + r) * T + 2 * r * T                  # decode in + out, extract in + out
        slot_bytes = wire + k * T + after_open                # every received packet read, k placed
        nr = rings["arrivals"]["n"]
        tags = 5 * nr
        # arr_at: init, read and write per slot, one atomic per opened arrival; arr_state written,
        # read and looked up per arrival
        tables2 = 12 * n + 8 * nr + 12 * nr
        # the pre-pass: its table initialised and read per slot, lengths and tags read per
        # arrival, one atomic per data arrival, one look-up per data arrival in the open pass
        tables = tables2 + 8 * n + 13 * nr + 12 * (k - r) * G
        arr_bytes = wire + tags + tables + second_read + k * T + after_open
        arr2_bytes = wire + tags + tables2 + second_read2 + k * T + after_open
        line = dict(config=label, mode="arrivals", k=k, m=m, losses=r, groups=G, packets=n,
                    reps=args.reps, kernels=kern, ring_packets=nr,
                    bytes_moved=dict(slot=slot_bytes, arrivals=arr_bytes, two_read=arr2_bytes,
                                     tag_bytes=tags, table_bytes=tables,
                                     table_bytes_two_read=tables2,
                                     second_read_bytes=second_read,
                                     second_read_bytes_two_read=second_read2),
                    shuffled_ring=shuffled)
        for name in names:
            med = statistics.median(t[name])
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(t[name]), 4),
                              kernel_ms_max=round(max(t[name]), 4))
        if args.variants:                                     # a trace run: no ratios
            results.append(line)
            print(json.dumps(line), flush=True)
            return
        line["arrivals_over_slot"] = round(line["arrivals"]["kernel_ms_median"] /
                                           line["slot"]["kernel_ms_median"], 3)
        line["byte_ratio"] = round(arr_bytes / slot_bytes, 3)
        line["two_read_over_slot"] = round(line["two_read"]["kernel_ms_median"] /
                                           line["slot"]["kernel_ms_median"], 3)
        line["two_read_byte_ratio"] = round(arr2_bytes / slot_bytes, 3)
        line["shuffled_over_arrivals"] = round(line["shuffled"]["kernel_ms_median"] /
                                               line["arrivals"]["kernel_ms_median"], 3)
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_window(k, m, r, bb, label, piece_counts, with_empty=True):
        """--window: the receiver window fed the in-order ring of --arrivals whole and in pieces,
        against the one-shot arrivals call over the same ring, data packets 0 .. r-1 of every group
        lost.  A route's time is the sum over its pushes, each between its own pair of timing
        events; the release that empties the window between repetitions is not timed.  `empty`:
        one push of no arrivals into the emptied window, the fixed cost of a push."""
        G, per, rmax, H = len(bb), k + m, min(k, m), 16
        n = G * per
        stride = H + 12 + int(bb.max())
        pay_stride = int(bb.max())
        hold = (int(bb.max()) + 15) // 16 * 16
        rng = np.random.default_rng(args.seed + 1)
        lens = (np.repeat(bb, k) - 2 - rng.integers(0, 8, G * k)).astype(np.int32)
        fbb, d_off, p_off, r_off, tot = fec.framed_layout(k, m, lens)
        assert np.array_equal(fbb, bb)
        pay = torch.empty((G * k, pay_stride), dtype=torch.uint8, device="cuda")
        fec.synth_fill(pay, seed=args.seed)
        lens_d = torch.from_numpy(lens).cuda()
        data = torch.zeros(tot[0], dtype=torch.uint8, device="cuda")
        par = torch.zeros(tot[1], dtype=torch.uint8, device="cuda")
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        hdr = torch.randint(0, 256, (n, H), dtype=torch.uint8, device="cuda")
        pkt = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        plen = torch.zeros(n, dtype=torch.int32, device="cuda")
        est = torch.zeros(G, dtype=torch.int32, device="cuda")
        eng.frame_encode_seal_ragged(k, m, bb_d, data, d_off_d, par, p_off_d, hdr, H, pay, lens_d,
                                     1, pkt, plen, status=est)
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0
        del data, par, hdr, pay
        wl = plen.clone().view(G, per)
        wl[:, :r] = -1
        recv = torch.nonzero(wl.view(n) >= 0).view(-1)
        nr = recv.numel()
        R = dict(pkt=pkt[recv].contiguous(), len=plen[recv].contiguous(),
                 grp=(recv // per).to(torch.int32), idx=(recv % per).to(torch.uint8),
                 state=torch.zeros(nr, dtype=torch.int32, device="cuda"))
        wire = int(R["len"].to(torch.int64).sum())
        del pkt

        def outputs():
            return dict(rec=torch.zeros(tot[2], dtype=torch.uint8, device="cuda"),
                        rr=torch.zeros((G, rmax), dtype=torch.uint8, device="cuda"),
                        st=torch.zeros(G, dtype=torch.int32, device="cuda"),
                        rev=torch.zeros((G * rmax, pay_stride), dtype=torch.uint8, device="cuda"),
                        rev_len=torch.zeros(G * rmax, dtype=torch.int32, device="cuda"),
                        rev_pn=torch.zeros(G * rmax, dtype=torch.uint8, device="cuda"))

        one, o = outputs(), outputs()
        one.update(blocks=torch.zeros(tot[0], dtype=torch.uint8, device="cuda"),
                   rows=torch.zeros((G, k), dtype=torch.uint8, device="cuda"),
                   ol=torch.zeros(n, dtype=torch.int32, device="cuda"),
                   at=torch.zeros(n, dtype=torch.int32, device="cuda"),
                   state=torch.zeros(nr, dtype=torch.int32, device="cuda"))

        def one_shot():
            eng.open_decode_extract_arrivals_ragged(
                k, m, bb_d, R["pkt"], R["len"], H, 1, R["grp"], R["idx"], one["state"], one["at"],
                one["blocks"], d_off_d, one["rows"], one["ol"], one["rec"], r_off_d, one["rr"],
                one["rev"], one["rev_len"], rev_pn_len=one["rev_pn"], status=one["st"])

        win = eng.rxwin(k, m, G, hold)

        def push(a, b):
            win.push(bb_d, R["pkt"][a:b], R["len"][a:b], H, 1, R["grp"][a:b], R["idx"][a:b],
                     R["state"][a:b], o["rec"], r_off_d, o["rr"], o["rev"], o["rev_len"],
                     rev_pn_len=o["rev_pn"], status=o["st"])

        def cuts_of(P):
            return [nr * i // P for i in range(P + 1)]

        one_shot()
        kern = dict(one_shot=fec.last_kernels())
        torch.cuda.synchronize()
        # outputs first: a group's status, rec_rows, rev_len and rev_pn_len are what the push that
        # completes it wrote (a later push overwrites them with the delivered values, so they are
        # gathered push by push here); rec and rev bytes are written once
        for P in piece_counts:
            for t_ in o.values():
                t_.zero_()
            win.release()
            acc = dict(rr=torch.full_like(o["rr"], 255), rev_len=torch.full_like(o["rev_len"], -1),
                       rev_pn=torch.zeros_like(o["rev_pn"]),
                       st=torch.full_like(o["st"], fec.WIN_OPEN))
            cuts = cuts_of(P)
            for a, b in zip(cuts[:-1], cuts[1:]):
                push(a, b)
                done = (o["st"] != fec.WIN_OPEN) & (o["st"] != fec.WIN_DELIVERED)
                acc["st"] = torch.where(done, o["st"], acc["st"])
                acc["rr"] = torch.where(done[:, None], o["rr"], acc["rr"])
                dq = done.repeat_interleave(rmax)
                acc["rev_len"] = torch.where(dq, o["rev_len"], acc["rev_len"])
                acc["rev_pn"] = torch.where(dq, o["rev_pn"], acc["rev_pn"])
            kern[f"window_{P}"] = fec.last_kernels()
            torch.cuda.synchronize()
            assert torch.equal(R["state"], one["state"]), f"arr_state differs, {P} pieces"
            for name in ("st", "rr", "rev_len"):
                assert torch.equal(acc[name], one[name]), f"{name} differs, {P} pieces"
            taken = one["rev_len"] >= 0
            assert torch.equal(acc["rev_pn"][taken], one["rev_pn"][taken])
            for name in ("rec", "rev"):
                assert torch.equal(o[name], one[name]), f"{name} differs, {P} pieces"

        routes = ["one_shot"] + [f"window_{P}" for P in piece_counts] + \
            (["empty"] if with_empty else [])
        first = {}
        pairs = 0
        for name in routes:
            first[name] = pairs
            pairs += int(name.split("_")[1]) if name.startswith("window_") else 1
        ev = DeviceEvents(2 * pairs)

        def run_route(name):
            if name == "one_shot":
                return timed(ev, first[name], one_shot)
            win.release()
            if name == "empty":
                return timed(ev, first[name], lambda: push(0, 0))
            cuts = cuts_of(int(name.split("_")[1]))
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                timed(ev, first[name] + i, lambda: push(a, b))

        t = {x: [] for x in routes}
        for rep_i in range(args.warmup + args.reps):
            for name in (routes if rep_i % 2 == 0 else routes[::-1]):
                run_route(name)
            torch.cuda.synchronize()
            if rep_i >= args.warmup:
                for name in routes:
                    cnt = int(name.split("_")[1]) if name.startswith("window_") else 1
                    t[name].append(sum(ev.elapsed_ms(2 * (first[name] + i), 2 * (first[name] + i) + 1)
                                       for i in range(cnt)))
        ev.close()
        win.close()
        # bytes moved, from the shapes (T = the bytes of one block per group, S = slots)
        T, S = int(bb.astype(np.int64).sum()), n
        after_open = (k + r) * T + 2 * r * T                  # decode in + out, extract in + out
        per_arrival = 5 * nr + 13 * nr + 8 * nr + 12 * nr     # tags; pre-pass; open; state pass
        one_tables = 12 * S + 8 * S + 12 * (k - r) * G
        # one push over all places: init reads the slot states and writes two tables, the assemble
        # reads three tables and the states and writes one, the group's row tags, effective bb,
        # verdict and count; the decode's prep and status passes and the finish read them again
        push_fixed = 12 * S + 20 * S + G * (k + 16) + G * (k + 8 + rmax + 4)
        completing = G * (8 * k + 8 * rmax)                   # pointer tables, written once
        one_bytes = wire + per_arrival + one_tables + k * T + after_open
        line = dict(config=label, mode="window", k=k, m=m, losses=r, groups=G, ring_packets=nr,
                    hold_stride=hold, window_bytes=fec.rxwin_bytes(k, m, G, hold), reps=args.reps,
                    kernels=kern,
                    bytes_moved=dict(one_shot=one_bytes, push_fixed=push_fixed,
                                     hold_rows_written=k * G * hold))
        for name in routes:
            med = statistics.median(t[name])
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(t[name]), 4),
                              kernel_ms_max=round(max(t[name]), 4))
        for P in piece_counts:
            name = f"window_{P}"
            line["bytes_moved"][name] = wire + per_arrival + P * push_fixed + completing + \
                k * G * hold + after_open
            line[name]["pushes"] = P
            line[name]["packets_per_push"] = round(nr / P)
            line[name]["over_one_shot"] = round(line[name]["kernel_ms_median"] /
                                                line["one_shot"]["kernel_ms_median"], 3)
            line[name]["byte_ratio"] = round(line["bytes_moved"][name] / one_bytes, 3)
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_ptrs(k, m, r, bb, label):
        """--ptrs: the packed ragged calls against the pointer form over identity tables and over
        individually placed blocks, data rows 0 .. r-1 of every group lost."""
        G, rmax = len(bb), min(k, m)
        bb64 = bb.astype(np.int64)
        d_off, p_off, r_off, tot = fec.ragged_layout(k, m, bb)
        data = torch.empty(tot[0], dtype=torch.uint8, device="cuda")
        fec.synth_fill(data, seed=args.seed)
        bb_d = torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        rows_np = np.tile(np.arange(k, dtype=np.uint8), (G, 1))
        rows_np[:, :r] = k + np.arange(r, dtype=np.uint8)
        rows = torch.from_numpy(rows_np).cuda()

        def step(n):
            return bb64[:, None] * np.arange(n, dtype=np.int64)[None, :]

        def outputs():
            return dict(par=torch.zeros(tot[1], dtype=torch.uint8, device="cuda"),
                        rec=torch.zeros(tot[2], dtype=torch.uint8, device="cuda"),
                        rr=torch.zeros((G, rmax), dtype=torch.uint8, device="cuda"),
                        est=torch.zeros(G, dtype=torch.int32, device="cuda"),
                        st=torch.zeros(G, dtype=torch.int32, device="cuda"))

        def copy_blocks(src_ptrs, dst_ptrs, sizes):
            # one block per "group": the pointer form's k = 1 encode is a block copy
            n = src_ptrs.numel()
            assert eng.encode_ptrs(1, 1, sizes, src_ptrs.view(n, 1), dst_ptrs.view(n, 1)) == 0

        def placed(n_per_group, seed, residues):
            """Offsets [G][n] of G * n blocks in a seeded random order, every block in a slot of
            its own (its size rounded up to 16, plus 16 when it starts off a 16-byte boundary)."""
            rng = np.random.default_rng(seed)
            sizes = np.repeat(bb64, n_per_group)
            order = rng.permutation(sizes.size)
            res = (np.arange(sizes.size) % 16) if residues else np.zeros(sizes.size, np.int64)
            slot = ((sizes[order] + 15) & ~15) + (16 if residues else 0)
            start = np.concatenate([[0], np.cumsum(slot)[:-1]]) + res
            off = np.empty(sizes.size, np.int64)
            off[order] = start
            return off.reshape(G, n_per_group), int(slot.sum())

        # packed: the baseline and the buffers the identity tables point into
        P = outputs()
        assert eng.encode_ragged(k, m, bb_d, data, d_off_d, P["par"], p_off_d, status=P["est"]) == 0
        kern = {"packed_encode": fec.last_kernels()}
        blocks = data.clone()
        copy_blocks(fec.block_ptrs(P["par"], p_off[:, None] + step(r)),
                    fec.block_ptrs(blocks, d_off[:, None] + step(r)),
                    torch.from_numpy(np.repeat(bb, r)).cuda())
        eng.decode_ragged_recovered(k, m, bb_d, blocks, d_off_d, rows, P["rec"], r_off_d, P["rr"],
                                    status=P["st"])
        kern["packed_decode"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(P["est"].abs().max()) == 0 and int(P["st"].abs().max()) == 0

        routes = {"packed": dict(out=P)}
        I = outputs()
        routes["identity"] = dict(
            out=I, data=fec.block_ptrs(data, d_off[:, None] + step(k)),
            recv=fec.block_ptrs(blocks, d_off[:, None] + step(k)),
            par=fec.block_ptrs(I["par"], p_off[:, None] + step(m)),
            rec=fec.block_ptrs(I["rec"], r_off[:, None] + step(rmax)))
        sizes_k = torch.from_numpy(np.repeat(bb, k)).cuda()
        for name, residues in (("scattered", False), ("unaligned", True)):
            o = outputs()
            offs = {x: placed(n, args.seed + i, residues)
                    for i, (x, n) in enumerate((("data", k), ("par", m), ("rec", rmax)))}
            arena = {x: torch.zeros(offs[x][1] + 32, dtype=torch.uint8, device="cuda") for x in offs}
            tab = {x: fec.block_ptrs(arena[x], offs[x][0]) for x in offs}
            copy_blocks(routes["identity"]["data"], tab["data"], sizes_k)
            recv = tab["data"].clone()
            recv[:, :r] = tab["par"][:, :r]          # the received parity blocks, where they lie
            routes[name] = dict(out=o, data=tab["data"], recv=recv, par=tab["par"], rec=tab["rec"],
                                arena=arena, residues=sorted(set((offs["data"][0] % 16).ravel()
                                                                 .tolist())))

        def encode(name):
            R, o = routes[name], routes[name]["out"]
            if name == "packed":
                eng.encode_ragged(k, m, bb_d, data, d_off_d, o["par"], p_off_d, status=o["est"])
            else:
                eng.encode_ptrs(k, m, bb_d, R["data"], R["par"], status=o["est"])

        def decode(name):
            R, o = routes[name], routes[name]["out"]
            if name == "packed":
                eng.decode_ragged_recovered(k, m, bb_d, blocks, d_off_d, rows, o["rec"], r_off_d,
                                            o["rr"], status=o["st"])
            else:
                eng.decode_ptrs_recovered(k, m, bb_d, R["recv"], rows, R["rec"], o["rr"],
                                          status=o["st"])

        # the same bytes from every route, at the timed size
        names = list(routes)
        for name in names[1:]:
            R, o = routes[name], routes[name]["out"]
            encode(name)
            kern[name + "_encode"] = fec.last_kernels()
            decode(name)
            kern[name + "_decode"] = fec.last_kernels()
            if "arena" in R:                          # gather the placed outputs into the packed form
                copy_blocks(R["par"], fec.block_ptrs(o["par"], p_off[:, None] + step(m)),
                            torch.from_numpy(np.repeat(bb, m)).cuda())
                copy_blocks(R["rec"][:, :r].contiguous(),
                            fec.block_ptrs(o["rec"], r_off[:, None] + step(r)),
                            torch.from_numpy(np.repeat(bb, r)).cuda())
            torch.cuda.synchronize()
            assert torch.equal(o["par"], P["par"]), f"{name}: parity differs from the packed call's"
            assert torch.equal(o["rec"], P["rec"]), f"{name}: recovered blocks differ"
            assert torch.equal(o["rr"], P["rr"]) and torch.equal(o["st"], P["st"]) and \
                torch.equal(o["est"], P["est"]), f"{name}: rows or statuses differ"

        phases = [(ph, name) for ph in ("encode", "decode") for name in names]
        ev = DeviceEvents(2 * len(phases))
        t = {x: [] for x in phases}
        for rep_i in range(args.warmup + args.reps):
            for ph, fn in (("encode", encode), ("decode", decode)):
                rot = rep_i % len(names)               # the routes alternate inside a repetition
                for name in names[rot:] + names[:rot]:
                    timed(ev, phases.index((ph, name)), lambda: fn(name))
            torch.cuda.synchronize()
            if rep_i >= args.warmup:
                for i, x in enumerate(phases):
                    t[x].append(ev.elapsed_ms(2 * i, 2 * i + 1))
        ev.close()
        total = int(bb64.sum())
        nbytes = {"encode": (k + m) * total, "decode": (k + r) * total}
        line = dict(config=label, mode="ptrs", k=k, m=m, losses=r, groups=G,
                    distinct_bb=len(set(bb.tolist())), reps=args.reps, kernels=kern,
                    bytes_moved=nbytes, table_bytes={"encode": 8 * (k + m) * G,
                                                     "decode": 8 * (k + rmax) * G},
                    residues={n: routes[n]["residues"] for n in ("scattered", "unaligned")})
        for ph, name in phases:
            v = t[(ph, name)]
            med = statistics.median(v)
            line[f"{name}_{ph}"] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(v), 4),
                                        kernel_ms_max=round(max(v), 4),
                                        GBps=round(nbytes[ph] / (med * 1e-3) / 1e9, 1))
        for ph in ("encode", "decode"):
            base = line[f"packed_{ph}"]["kernel_ms_median"]
            for name in names[1:]:
                line[f"{name}_{ph}_over_packed"] = round(
                    line[f"{name}_{ph}"]["kernel_ms_median"] / base, 3)
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_mixed(codes, r, G, label):
        """--mixed: one mixed call against one ragged call per code on the same groups, data rows
        0 .. r-1 of every group lost."""
        rng = np.random.default_rng(args.seed + 7)
        nc = len(codes)
        code = rng.integers(0, nc, G).astype(np.uint8)
        bb = draw_sizes(G, args.seed)
        bb64 = bb.astype(np.int64)
        ks = np.array([k for k, _ in codes], np.int64)[code]
        ms = np.array([m for _, m in codes], np.int64)[code]
        cs = eng.codeset(codes)
        kmax, rmax = cs.kmax, cs.rmax
        d_off, p_off, r_off, tot = fec.mixed_layout(codes, code, bb)
        data = torch.empty(tot[0], dtype=torch.uint8, device="cuda")
        fec.synth_fill(data, seed=args.seed)
        par = torch.zeros(tot[1], dtype=torch.uint8, device="cuda")
        rec = torch.zeros(tot[2], dtype=torch.uint8, device="cuda")
        code_d, bb_d = torch.from_numpy(code).cuda(), torch.from_numpy(bb).cuda()
        d_off_d, p_off_d, r_off_d = (torch.from_numpy(o).cuda() for o in (d_off, p_off, r_off))
        rows_np = np.tile(np.arange(kmax, dtype=np.int64), (G, 1))
        rows_np[:, :r] = ks[:, None] + np.arange(r)[None, :]
        rows = torch.from_numpy(rows_np.astype(np.uint8)).cuda()
        rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
        est = torch.zeros(G, dtype=torch.int32, device="cuda")
        st = torch.zeros(G, dtype=torch.int32, device="cuda")

        def mixed_encode():
            eng.encode_mixed(cs, code_d, bb_d, data, d_off_d, par, p_off_d, status=est)

        mixed_encode()
        kern = {"mixed_encode": fec.last_kernels()}
        blocks = data.clone()
        torch._foreach_copy_(views(blocks, d_off, r * bb64), views(par, p_off, r * bb64))

        def mixed_decode():
            eng.decode_mixed_recovered(cs, code_d, bb_d, blocks, d_off_d, rows, rec, r_off_d, rr,
                                       status=st)

        mixed_decode()
        kern["mixed_decode"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0 and int(st.abs().max()) == 0

        # the parent's route: the groups sorted by code, one packed buffer per code (not timed)
        def up16(v):
            return (v + 15) & ~15

        buckets = []
        for c, (k, m) in enumerate(codes):
            idx = np.nonzero(code == c)[0]
            if not len(idx):
                continue
            bo = fec.ragged_layout(k, m, bb[idx])
            ix = torch.from_numpy(idx).cuda()
            buckets.append(dict(
                k=k, m=m, idx=idx, bb=bb_d[ix].contiguous(),
                off=[torch.from_numpy(o).cuda() for o in bo[:3]], tot=bo[3],
                data=torch.cat(views(data, d_off[idx], up16(k * bb64[idx]))),
                blocks=torch.cat(views(blocks, d_off[idx], up16(k * bb64[idx]))),
                rows=rows[ix][:, :k].contiguous(),
                par=torch.zeros(bo[3][1], dtype=torch.uint8, device="cuda"),
                rec=torch.zeros(bo[3][2], dtype=torch.uint8, device="cuda"),
                rr=torch.zeros((len(idx), min(k, m)), dtype=torch.uint8, device="cuda"),
                st=torch.zeros(len(idx), dtype=torch.int32, device="cuda")))
        nb = len(buckets)

        def sorted_encode(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.encode_ragged(B["k"], B["m"], B["bb"], B["data"], B["off"][0],
                                              B["par"], B["off"][1])
                timed(ev, base + i, f) if ev else f()

        def sorted_decode(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.decode_ragged_recovered(B["k"], B["m"], B["bb"], B["blocks"],
                                                        B["off"][0], B["rows"], B["rec"],
                                                        B["off"][2], B["rr"], status=B["st"])
                timed(ev, base + i, f) if ev else f()

        # the same bytes from both routes, at the timed size
        sorted_encode()
        kern["sorted_encode"] = fec.last_kernels()
        sorted_decode()
        kern["sorted_decode"] = fec.last_kernels()
        torch.cuda.synchronize()
        for B in buckets:
            idx, k, m = B["idx"], B["k"], B["m"]
            assert torch.equal(torch.cat(views(par, p_off[idx], up16(m * bb64[idx]))), B["par"]), \
                "parity differs between the routes"
            got = torch.cat(views(rec, r_off[idx], r * bb64[idx]))
            want = torch.cat(views(B["rec"], B["off"][2].cpu().numpy(), r * bb64[idx]))
            assert torch.equal(got, want), "recovered blocks differ between the routes"
            assert torch.equal(got, torch.cat(views(data, d_off[idx], r * bb64[idx]))), \
                "recovered blocks are not the lost data"
            assert torch.equal(rr[torch.from_numpy(idx).cuda()][:, :min(k, m)], B["rr"])

        ev = DeviceEvents(2 * (2 + 2 * nb))
        t = {x: [] for x in ("mixed_encode", "mixed_decode", "sorted_encode", "sorted_decode")}
        wall = {x: [] for x in t}

        def walled(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)

        for rep_i in range(args.warmup + args.reps):
            order = [("mixed_encode", lambda: timed(ev, 0, mixed_encode)),
                     ("sorted_encode", lambda: sorted_encode(ev, 2)),
                     ("mixed_decode", lambda: timed(ev, 1, mixed_decode)),
                     ("sorted_decode", lambda: sorted_decode(ev, 2 + nb))]
            if rep_i % 2:
                order = [order[1], order[0], order[3], order[2]]
            for name, fn in order:
                walled(name, fn)
            if rep_i < args.warmup:
                for x in wall:
                    wall[x].clear()
                continue
            t["mixed_encode"].append(ev.elapsed_ms(0, 1))
            t["mixed_decode"].append(ev.elapsed_ms(2, 3))
            t["sorted_encode"].append(sum(ev.elapsed_ms(2 * (2 + i), 2 * (2 + i) + 1)
                                          for i in range(nb)))
            t["sorted_decode"].append(sum(ev.elapsed_ms(2 * (2 + nb + i), 2 * (2 + nb + i) + 1)
                                          for i in range(nb)))
        ev.close()
        nbytes = {"encode": int(((ks + ms) * bb64).sum()), "decode": int(((ks + r) * bb64).sum())}
        line = dict(config=label, mode="mixed", codes=[list(c) for c in codes], losses=r, groups=G,
                    groups_per_code=[int((code == c).sum()) for c in range(nc)],
                    ragged_calls_per_phase=nb, reps=args.reps, kernels=kern, grids=fec.last_grids(),
                    bytes_moved=nbytes)
        for name, v in t.items():
            med = statistics.median(v)
            by = nbytes["encode" if name.endswith("encode") else "decode"]
            line[name] = dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(min(v), 4),
                              kernel_ms_max=round(max(v), 4),
                              wall_ms_median=round(statistics.median(wall[name]), 4),
                              GBps=round(by / (med * 1e-3) / 1e9, 1))
        for ph in ("encode", "decode"):
            for what in ("kernel", "wall"):
                line[f"{ph}_{what}_mixed_over_sorted"] = round(
                    line[f"mixed_{ph}"][f"{what}_ms_median"] /
                    line[f"sorted_{ph}"][f"{what}_ms_median"], 3)
        cs.close()
        results.append(line)
        print(json.dumps(line), flush=True)

    def run_mixed_wire(codes, r, G, label):
        """--mixed-wire: the mixed framed sender and the mixed arrival-order receiver, one call
        each, against one ragged call per code on the same groups pre-split by code (not timed);
        data packets 0 .. r-1 of every group lost, the ring in order."""
        rng = np.random.default_rng(args.seed + 11)
        nc, H = len(codes), 16
        code = rng.integers(0, nc, G).astype(np.uint8)
        bb = draw_sizes(G, args.seed)
        ks = np.array([k for k, _ in codes], np.int64)[code]
        ms = np.array([m for _, m in codes], np.int64)[code]
        pkt_first, pay_first = fec.mixed_packet_layout(codes, code)
        npkt, npay = int(pkt_first[-1]), int(pay_first[-1])
        stride, pay_stride = H + 12 + int(bb.max()), int(bb.max())
        gpay, gpkt = np.repeat(np.arange(G), ks), np.repeat(np.arange(G), ks + ms)
        ipkt = np.arange(npkt) - pkt_first[gpkt]
        lens = (bb[gpay] - 2 - rng.integers(0, 8, npay)).astype(np.int32)
        fbb, d_off, p_off, r_off, tot = fec.framed_layout_mixed(codes, code, lens)
        assert np.array_equal(fbb, bb)
        cs = eng.codeset(codes)
        kmax, rmax = cs.kmax, cs.rmax
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
        zeros = lambda shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        pay = torch.empty((npay, pay_stride), dtype=torch.uint8, device="cuda")
        fec.synth_fill(pay, seed=args.seed)
        hdr = torch.randint(0, 256, (npkt, H), dtype=torch.uint8, device="cuda")
        lens_d, code_d, bb_d = cuda(lens), cuda(code), cuda(bb)
        pf_d, qf_d = cuda(pkt_first), cuda(pay_first)
        d_off_d, p_off_d, r_off_d = cuda(d_off), cuda(p_off), cuda(r_off)
        data, par = zeros(tot[0]), zeros(tot[1])
        pkt, plen, est = zeros((npkt, stride)), zeros(npkt, torch.int32), zeros(G, torch.int32)

        def mixed_send():
            eng.frame_encode_seal_mixed(cs, code_d, bb_d, pf_d, qf_d, data, d_off_d, par, p_off_d,
                                        hdr, H, pay, lens_d, 1, pkt, plen, status=est)

        mixed_send()
        kern = {"mixed_send": fec.last_kernels()}
        torch.cuda.synchronize()
        assert int(est.abs().max()) == 0 and int(plen.min()) > 0
        # the in-order ring: every packet but data packets 0 .. r-1 of each group
        recv = np.flatnonzero(ipkt >= r)
        n = recv.size
        recv_d = cuda(recv)
        ring = dict(pkt=pkt[recv_d].contiguous(), len=plen[recv_d].contiguous(),
                    grp=cuda(gpkt[recv].astype(np.int32)), idx=cuda(ipkt[recv].astype(np.uint8)))

        def outputs(Gx, kx, rx, slots, nx, tot_x):
            return dict(blocks=zeros(tot_x[0]), rec=zeros(tot_x[2]), rows=zeros((Gx, kx)),
                        ol=zeros(slots, torch.int32), at=zeros(slots, torch.int32),
                        state=zeros(nx, torch.int32), rr=zeros((Gx, rx)), st=zeros(Gx, torch.int32),
                        rev=zeros((Gx * rx, pay_stride)), rev_len=zeros(Gx * rx, torch.int32),
                        rev_pn=zeros(Gx * rx))

        o = outputs(G, kmax, rmax, npkt, n, tot)

        def mixed_recv():
            eng.open_decode_extract_arrivals_mixed(
                cs, code_d, bb_d, pf_d, ring["pkt"], ring["len"], H, 1, ring["grp"], ring["idx"],
                o["state"], o["at"], o["blocks"], d_off_d, o["rows"], o["ol"], o["rec"], r_off_d,
                o["rr"], o["rev"], o["rev_len"], rev_pn_len=o["rev_pn"], status=o["st"])

        mixed_recv()
        kern["mixed_recv"] = fec.last_kernels()
        torch.cuda.synchronize()
        assert int(o["st"].abs().max()) == 0
        # every lost payload comes back
        lost = cuda(pay_first[:-1][:, None] + np.arange(r)[None, :])
        got = o["rev_len"].view(G, rmax)[:, :r]
        assert torch.equal(got, lens_d[lost])
        mask = torch.arange(pay_stride, device="cuda")[None, None, :] < got[:, :, None]
        assert torch.equal(o["rev"].view(G, rmax, pay_stride)[:, :r][mask], pay[lost][mask])
        del mask

        # the parent's route: groups and arrivals pre-split by code (not timed)
        buckets = []
        for c, (k, m) in enumerate(codes):
            idx = np.flatnonzero(code == c)
            if not idx.size:
                continue
            Gb, per, rm = idx.size, k + m, min(k, m)
            prow = (pkt_first[idx][:, None] + np.arange(per)[None, :]).ravel()
            qrow = (pay_first[idx][:, None] + np.arange(k)[None, :]).ravel()
            bo = fec.ragged_layout(k, m, bb[idx])
            sel = np.flatnonzero(code[gpkt[recv]] == c)
            renum = np.zeros(G, np.int32)
            renum[idx] = np.arange(Gb)
            sel_d = cuda(sel)
            B = dict(k=k, m=m, idx=idx, G=Gb, prow=cuda(prow), sel=sel_d, bb=cuda(bb[idx]),
                     off=[cuda(x) for x in bo[:3]], data=zeros(bo[3][0]), par=zeros(bo[3][1]),
                     hdr=hdr[cuda(prow)].contiguous(), pay=pay[cuda(qrow)].contiguous(),
                     lens=cuda(lens[qrow]), pkt=zeros((Gb * per, stride)),
                     plen=zeros(Gb * per, torch.int32), est=zeros(Gb, torch.int32),
                     ring=dict(pkt=ring["pkt"][sel_d].contiguous(), len=ring["len"][sel_d].contiguous(),
                               grp=cuda(renum[gpkt[recv][sel]]), idx=ring["idx"][sel_d].contiguous()),
                     o=outputs(Gb, k, rm, Gb * per, sel.size, bo[3]))
            buckets.append(B)
        nb = len(buckets)

        def sorted_send(ev=None, base=0):
            for i, B in enumerate(buckets):
                f = lambda: eng.frame_encode_seal_ragged(                             # noqa: E731
                    B["k"], B["m"], B["bb"], B["data"], B["off"][0], B["par"], B["off"][1], B["hdr"],
                    H, B["pay"], B["lens"], 1, B["pkt"], B["plen"], status=B["est"])
                timed(ev, base + i, f) if ev else f()

        def sorted_recv(ev=None, base=0):
            for i, B in enumerate(buckets):
                R, x = B["ring"], B["o"]
                f = lambda: eng.open_decode_extract_arrivals_ragged(                  # noqa: E731
                    B["k"], B["m"], B["bb"], R["pkt"], R["len"], H, 1, R["grp"], R["idx"], x["state"],
                    x["at"], x["blocks"], B["off"][0], x["rows"], x["ol"], x["rec"], B["off"][2],
                    x["rr"], x["rev"], x["rev_len"], rev_pn_len=x["rev_pn"], status=x["st"])
                timed(ev, base + i, f) if ev else f()

        # the same bytes from both routes, at the timed size
        sorted_send()
        kern["sorted_send"] = fec.last_kernels()
        sorted_recv()
        kern["sorted_recv"] = fec.last_kernels()
        torch.cuda.synchronize()
        for B in buckets:
            ix, x, rm = cuda(B["idx"]), B["o"], min(B["k"], B["m"])
            assert torch.equal(pkt[B["prow"]], B["pkt"]), "wire packets differ between the routes"
            assert torch.equal(plen[B["prow"]], B["plen"]), "pkt_len differs between the routes"
            assert torch.equal(o["state"][B["sel"]], x["state"]), "arr_state differs"
            assert torch.equal(o["ol"][B["prow"]], x["ol"]), "open_len differs"
            assert torch.equal(o["st"][ix], x["st"]) and torch.equal(o["rr"][ix][:, :rm], x["rr"])
            assert torch.equal(o["rev_len"].view(G, rmax)[ix][:, :rm].reshape(-1), x["rev_len"])
            assert torch.equal(o["rev"].view(G, rmax, pay_stride)[ix][:, :rm].reshape(-1, pay_stride),
                               x["rev"]), "revived payloads differ between the routes"

        ev = DeviceEvents(2 * (2 + 2 * nb))
        t = {x: [] for x in ("mixed_send", "mixed_recv", "sorted_send", "sorted_recv")}
        wall = {x: [] for x in t}

        def walled(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)

        for rep_i in range(args.warmup + args.reps):
            order = [("mixed_send", lambda: timed(ev, 0, mixed_send)),
                     ("sorted_send", lambda: sorted_send(ev, 2)),
                     ("mixed_recv", lambda: timed(ev, 1, mixed_recv)),
                     ("sorted_recv", lambda: sorted_recv(ev, 2 + nb))]
            if rep_i % 2:
                order = [order[1], order[0], order[3], order[2]]
            for name, fn in order:
                walled(name, fn)
            if rep_i < args.warmup:
                for x in wall:
                    wall[x].clear()
                continue
            t["mixed_send"].append(ev.elapsed_ms(0, 1))
            t["mixed_recv"].append(ev.elapsed_ms(2, 3))
            t["sorted_send"].append(sum(ev.elapsed_ms(2 * (2 + i), 2 * (2 + i) + 1)
                                        for i in range(nb)))
            t["sorted_recv"].append(sum(ev.elapsed_ms(2 * (2 + nb + i), 2 * (2 + nb + i) + 1)
                                        for i in range(nb)))
        ev.close()
        line = dict(config=label, mode="mixed_wire", codes=[list(c) for c in codes], losses=r,
                    groups=G, packets=npkt, arrivals=int(n),
                    groups_per_code=[int((code == c).sum()) for c in range(nc)],
                    ragged_calls_per_phase=nb, reps=args.reps, kernels=kern)
        for name, v in t.items():
            line[name] = dict(kernel_ms_median=round(statistics.median(v), 4),
                              kernel_ms_min=round(min(v), 4), kernel_ms_max=round(max(v), 4),
                              wall_ms_median=round(statistics.median(wall[name]), 4),
                              wall_ms_min=round(min(wall[name]), 4),
                              wall_ms_max=round(max(wall[name]), 4))
        for ph in ("send", "recv"):
            for what in ("kernel", "wall"):
                line[f"{ph}_{what}_mixed_over_sorted"] = round(
                    line[f"mixed_{ph}"][f"{what}_ms_median"] /
                    line[f"sorted_{ph}"][f"{what}_ms_median"], 3)
        cs.close()
        results.append(line)
        print(json.dumps(line), flush=True)

    G = args.groups
    if args.mixed_wire:
        presets = [(5, 5), (10, 10), (10, 15), (10, 20), (15, 15), (250, 5)]
        run_mixed_wire(presets, 2, 1024, "(a) six presets, 1024 groups")
        run_mixed_wire([(32, 4)], 2, 1024, "(b) one code (32,4), 1024 groups")
        run_mixed_wire(presets, 2, G, f"(c) six presets, {G} groups")
        run_mixed_wire([(32, 4)], 2, G, f"(d) one code (32,4), {G} groups")
        args.codes = ""
    if args.mixed:
        presets = [(5, 5), (10, 10), (10, 15), (10, 20), (15, 15), (250, 5)]
        run_mixed(presets, 2, G, f"(a) six presets, {G} groups")
        run_mixed(presets, 2, 1024, "(b) six presets, 1024 groups")
        run_mixed([(32, 4)], 2, G, f"(c) one code (32,4), {G} groups")
        args.codes = ""
    if args.window:
        for k, m, r in (tuple(int(v) for v in c.split(",")) for c in args.codes.split()):
            run_window(k, m, r, draw_sizes(G, args.seed), f"mixed ({k},{m})", [1, 4, 16])
        # the shape a connection has: a window of 4,096 places, rings of about 16k packets
        small = draw_sizes(4096, args.seed)
        for k, m, r in ((32, 4, 2), (10, 1, 1)):
            pushes = max(1, round(4096 * (k + m - r) / 16384))
            run_window(k, m, r, small, f"4096 places, 16k-packet rings ({k},{m})", [1, pushes])
        args.codes = ""
    mixed = draw_sizes(G, args.seed)
    flat = np.full(G, 1352, np.int32)
    run = run_pp if args.pp else run_config
    for k, m, r in (tuple(int(v) for v in c.split(",")) for c in args.codes.split()):
        if args.ptrs:
            run_ptrs(k, m, r, mixed, f"mixed ({k},{m})")
            continue
        if args.framed or args.arrivals:
            (run_framed if args.framed else run_arrivals)(k, m, r, mixed, f"mixed ({k},{m})")
            continue
        run(k, m, r, mixed, f"mixed ({k},{m})")
        # the price of run-time shapes: every bb = 1352, one bucket = the compiled path (A / B)
        run(k, m, r, flat, f"all-1352 ({k},{m})")
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/ragged_bench.py", seed=args.seed, hbm_peak_Bps=HBM_BYTES_PER_S,
                           timing="qfec_set_timing_events (first kernel start to last kernel end); "
                                  "wall = enqueue to synchronise",
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
