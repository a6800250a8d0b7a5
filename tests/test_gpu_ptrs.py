"""Pointer-table batches on the GPU (qfec_encode_batch_ptrs / qfec_decode_batch_ptrs_recovered):
every input and output block scattered on its own in one guarded arena, in a seeded permuted
order, at least 16 poison bytes between neighbours, start addresses through all 16 residues mod
16.  After the calls the whole arena is compared with an expected image built from the CPU
oracle (tests/test_gpu_ragged.py's cases): bytes outside the blocks the contract says are
written still hold the poison, and so does the trap block that every never-dereferenced table
entry points at.  Bit-exact.  Run with -m gpu; tests/test_ptrs_abi.py checks the construction
on the CPU."""
import numpy as np
import pytest

from quic_amd import fec
from tests import guarded as Gd
from tests.test_gpu_ragged import (CODES, GF_SIZES, KINDS, POISON, XOR_EXTRA, build_case, dev,
                                   host, mixed_case, up16)

pytestmark = pytest.mark.gpu

assert POISON == Gd.FILL
TRAP_BYTES = 64
ALIGNS = ["all", "aligned", "mixed"]


def _residue(align, n, g):
    """Start residue mod 16 of the n-th placed block, which belongs to group g."""
    if align == "all":
        return n % 16
    if align == "aligned":
        return 0
    return 0 if g % 2 == 0 else 1 + 2 * (n % 8)       # mixed: even groups aligned, odd groups odd


def scatter(c, align="all", seed=0, zero=()):
    """Places every block of the case c (build_case) on its own in one arena.  zero: groups whose
    size is passed as 0 (they keep their statuses and rec_rows, which follow from the row tags,
    and nothing of them is read or written).  Returns the offsets, the tables (as offsets into
    the arena, never-dereferenced entries at the trap), the arena's first image and the image
    expected after the encode and the decode."""
    k, m, G, rmax = c["k"], c["m"], c["G"], c["rmax"]
    rng = np.random.default_rng(seed)
    bbs = [int(b) for b in c["bb"]]
    assert all(bbs[g] % 8 == 0 for g in zero)
    blocks = [("trap", -1, 0, TRAP_BYTES)]
    for g, b in enumerate(bbs):
        if g in zero:
            continue
        blocks += [("data", g, i, b) for i in range(k)] + [("recv", g, i, b) for i in range(k)]
        blocks += [("par", g, y, b) for y in range(m)] + [("rec", g, j, b) for j in range(rmax)]
    off, run, seen = {}, 16, set()
    for n, bi in enumerate(rng.permutation(len(blocks))):
        kind, g, i, b = blocks[bi]
        res = _residue(align, n, g)
        start = up16(run) + res
        off[(kind, g, i)] = start
        seen.add(start % 16)
        run = start + b + 16                              # at least 16 poison bytes between
    total = up16(run)
    trap = off[("trap", -1, 0)]
    s = dict(c=c, total=total, trap=trap, off=off, residues=seen, align=align,
             bb=np.array([0 if g in zero else b for g, b in enumerate(bbs)], np.int32))
    image = np.full(total, POISON, np.uint8)
    tabs = {n: np.full((G, w), trap, np.int64)
            for n, w in (("data", k), ("recv", k), ("par", m), ("rec", rmax))}
    writes = []
    for g, b in enumerate(bbs):
        if g in zero:
            continue
        do, po, ro = int(c["data_off"][g]), int(c["par_off"][g]), int(c["rec_off"][g])
        for i in range(k):
            for kind, src in (("data", c["data"]), ("recv", c["blocks"])):
                o = off[(kind, g, i)]
                tabs[kind][g, i] = o
                image[o:o + b] = src[do + i * b:do + (i + 1) * b]
        npar = m if c["enc_status"][g] == 0 else 1     # a rejected group: its first parity only
        for y in range(npar):
            tabs["par"][g, y] = off[("par", g, y)]
            writes.append((off[("par", g, y)], c["par_exp"][po + y * b:po + (y + 1) * b]))
        nrec = int(c["nrec"][g]) if c["dec_status"][g] >= 0 else 0
        for j in range(nrec):
            tabs["rec"][g, j] = off[("rec", g, j)]
            writes.append((off[("rec", g, j)], c["rec_exp"][ro + j * b:ro + (j + 1) * b]))
    exp = image.copy()
    for o, src in writes:
        exp[o:o + len(src)] = src
    enc_status = c["enc_status"].copy()
    for g in zero:                                        # bb = 0: bb % 8 == 0, nothing to reject
        enc_status[g] = -1 if (m > 1 and k > 1 and k + m > 256) else 0
    s.update(image=image, exp=exp, tabs=tabs, enc_status=enc_status)
    return s


class Arena:
    """The scatter s on the device: one guarded buffer and the four address tables."""

    def __init__(self, s):
        self.s = s
        self.view, self.h = Gd.guarded(s["total"])
        self.h.load(s["image"])
        self.tab = {n: fec.block_ptrs(self.view, t) for n, t in s["tabs"].items()}
        self.bb = dev(s["bb"])

    def run(self, engine, what="both", bb=None, stream=None):
        """Encode and / or decode over the tables; returns statuses, rec_rows and kernel names."""
        import torch
        c = self.s["c"]
        k, m, G = c["k"], c["m"], c["G"]
        bb = self.bb if bb is None else bb
        out = {}
        if what in ("both", "encode"):
            st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
            out["enc_rc"] = engine.encode_ptrs(k, m, bb, self.tab["data"], self.tab["par"],
                                               status=st, stream=stream)
            out["enc_kernels"], out["enc_grids"] = fec.last_kernels(), fec.last_grids()
            out["enc_status"] = host(st)
        if what in ("both", "decode"):
            rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8, device="cuda")
            st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
            rows = dev(c["rows"])
            engine.decode_ptrs_recovered(k, m, bb, self.tab["recv"], rows, self.tab["rec"], rr,
                                         status=st, stream=stream)
            out["dec_kernels"], out["dec_grids"] = fec.last_kernels(), fec.last_grids()
            out["rec_rows"], out["dec_status"] = host(rr), host(st)
            np.testing.assert_array_equal(host(rows), c["rows"])
        return out

    def check(self, out, exp=None):
        """Statuses and rec_rows are the oracle's, and the whole arena is the expected image:
        what had to be written is, every other byte (inputs, gaps, the trap, unwritten outputs,
        the guards) is as it was."""
        s, c = self.s, self.s["c"]
        if "enc_status" in out:
            np.testing.assert_array_equal(out["enc_status"], s["enc_status"])
        if "dec_status" in out:
            np.testing.assert_array_equal(out["dec_status"], c["dec_status"])
            np.testing.assert_array_equal(out["rec_rows"], c["rec_rows"])
        got = self.h.host()
        exp = s["exp"] if exp is None else exp
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (f"{bad.size} arena bytes differ, first at {int(bad[0])}: "
                               f"0x{int(got[bad[0]]):02x}, expected 0x{int(exp[bad[0]]):02x}")
        t = s["trap"]
        assert (got[t:t + TRAP_BYTES] == POISON).all()
        self.h.check_guards()


def run_case(engine, c, align, seed=0, zero=()):
    a = Arena(scatter(c, align, seed, zero))
    out = a.run(engine)
    a.check(out)
    return a, out


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("G", [1, 7, 203])
@pytest.mark.parametrize("k,m", CODES)
def test_ptrs_vs_oracle(engine, oracle, k, m, G, align):
    c = mixed_case(oracle, k, m, G)
    if G == 203:
        assert set(c["bb"].tolist()) >= set(GF_SIZES + (XOR_EXTRA if m == 1 or k <= 1 else []))
    a, out = run_case(engine, c, align, seed=G)
    assert out["enc_rc"] == 0
    if align == "all" and G > 1:
        assert a.s["residues"] == set(range(16))


@pytest.mark.parametrize("align", ALIGNS)
def test_ptrs_250_5(engine, oracle, align):
    c = mixed_case(oracle, 250, 5, 12)
    _, out = run_case(engine, c, align, seed=5)
    assert out["enc_rc"] == 0


# ------------------------------------------------------------------ identity and uniform tables
@pytest.mark.parametrize("k,m", [(32, 4), (10, 1), (5, 5), (1, 3)])
def test_ptrs_identity_tables_equal_ragged(engine, oracle, k, m):
    """Tables that point into the packed ragged layout: byte for byte the ragged calls' outputs,
    statuses and rec_rows, including what those calls leave for bb[g] = 0 groups."""
    import torch
    c = mixed_case(oracle, k, m, 23)
    G, rmax = c["G"], c["rmax"]
    bbs = c["bb"].copy()
    zero = [g for g in range(G) if bbs[g] % 8 == 0][1:6:2]
    bbs[zero] = 0
    assert len(zero) == 3
    bb, data, blocks, rows = dev(bbs), dev(c["data"]), dev(c["blocks"]), dev(c["rows"])
    res = {}
    for form in ("ragged", "ptrs"):
        par = torch.full((c["par_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        rec = torch.full((c["rec_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        est = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        dst = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        rr = torch.full((G, rmax), 9, dtype=torch.uint8, device="cuda")
        if form == "ragged":
            engine.encode_ragged(k, m, bb, data, dev(c["data_off"]), par, dev(c["par_off"]),
                                 status=est)
            engine.decode_ragged_recovered(k, m, bb, blocks, dev(c["data_off"]), rows, rec,
                                           dev(c["rec_off"]), rr, status=dst)
        else:
            step = lambda n: c["bb"].astype(np.int64)[:, None] * np.arange(n)[None, :]  # noqa: E731
            engine.encode_ptrs(k, m, bb, fec.block_ptrs(data, c["data_off"][:, None] + step(k)),
                               fec.block_ptrs(par, c["par_off"][:, None] + step(m)), status=est)
            engine.decode_ptrs_recovered(
                k, m, bb, fec.block_ptrs(blocks, c["data_off"][:, None] + step(k)), rows,
                fec.block_ptrs(rec, c["rec_off"][:, None] + step(rmax)), rr, status=dst)
        res[form] = [host(t) for t in (par, rec, est, dst, rr)]
    for a, b in zip(res["ragged"], res["ptrs"]):
        np.testing.assert_array_equal(a, b)
    for g in zero:                                  # nothing of a bb = 0 group is written
        po, ro, b = int(c["par_off"][g]), int(c["rec_off"][g]), int(c["bb"][g])
        assert (res["ptrs"][0][po:po + m * b] == POISON).all()
        assert (res["ptrs"][1][ro:ro + rmax * b] == POISON).all()


@pytest.mark.parametrize("k,m,bb", [(32, 4, 1352), (10, 1, 1350)])
def test_ptrs_uniform_size(engine, oracle, k, m, bb):
    """d_bb == NULL with bb_all: the bytes of qfec_encode_batch / qfec_decode_batch_recovered."""
    import torch
    G = 7
    c = build_case(oracle, k, m, [bb] * G, KINDS, seed=99)
    a = Arena(scatter(c, "all", seed=3))
    out = a.run(engine, bb=bb)
    a.check(out)
    data = np.stack([c["data"][o:o + k * bb].reshape(k, bb) for o in c["data_off"]])
    blocks = np.stack([c["blocks"][o:o + k * bb].reshape(k, bb) for o in c["data_off"]])
    par = torch.zeros((G, m, bb), dtype=torch.uint8, device="cuda")
    assert engine.encode(k, m, bb, dev(data), par) == 0
    rmax = c["rmax"]
    rec = torch.zeros((G, rmax, bb), dtype=torch.uint8, device="cuda")
    rr = torch.zeros((G, rmax), dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    engine.decode_recovered(k, m, bb, dev(blocks), dev(c["rows"]), rec, rr, status=st)
    np.testing.assert_array_equal(host(st), out["dec_status"])
    np.testing.assert_array_equal(host(rr), out["rec_rows"])
    got, par, rec = a.h.host(), host(par), host(rec)
    for g in range(G):
        for y in range(m):
            o = a.s["off"][("par", g, y)]
            np.testing.assert_array_equal(got[o:o + bb], par[g, y])
        for j in range(int(c["nrec"][g])):
            o = a.s["off"][("rec", g, j)]
            np.testing.assert_array_equal(got[o:o + bb], rec[g, j])


def test_ptrs_uniform_size_not_multiple_of_8(engine, oracle):
    """bb_all = 1350 with m > 1: every group is rejected by the encode (XOR parity in its first
    parity block) and every group holding a recovery block has decode status -1."""
    c = build_case(oracle, 5, 5, [1350] * 5, ["r1", "none", "rmax"], seed=12)
    assert c["enc_status"].tolist() == [-1] * 5 and c["dec_status"].tolist() == [-1, 0, -1, -1, 0]
    a = Arena(scatter(c, "all", seed=4))
    out = a.run(engine, bb=1350)
    a.check(out)
    assert "ptrs_decode_status_kernel" in out["dec_kernels"]


def test_ptrs_shared_blocks(engine, oracle):
    """Two groups whose tables name the same data blocks give the same parity."""
    k, m = 32, 4
    c = build_case(oracle, k, m, [1352, 1352, 520], ["none"], seed=21)
    s = scatter(c, "all", seed=6)
    s["tabs"]["data"][1] = s["tabs"]["data"][0]
    b = 1352
    for y in range(m):
        o0, o1 = s["off"][("par", 0, y)], s["off"][("par", 1, y)]
        s["exp"][o1:o1 + b] = s["exp"][o0:o0 + b]
    a = Arena(s)
    a.check(a.run(engine, "encode"))


# ------------------------------------------------------------------ statuses
def test_ptrs_never_dereferenced_entries(engine, oracle):
    """One batch with every kind of entry the contract says is never dereferenced, all at the
    trap block: rec entries past the erasure count, every rec entry of a -1 and of a -3 group,
    parity entries 1 .. m-1 of a rejected group, every entry of a bb = 0 group."""
    bbs = [1352, 1350, 520, 104, 1350, 2056, 40, 1352, 24]
    c = build_case(oracle, 5, 5, bbs, ["r1", "rmax", "malformed", "none"], seed=55)
    assert c["enc_status"].tolist() == [0, -1, 0, 0, -1, 0, 0, 0, 0]
    assert sorted(set(c["dec_status"].tolist())) == [-3, -1, 0]
    s = scatter(c, "all", seed=8, zero=(3, 7))
    trap, t = s["trap"], s["tabs"]
    assert (t["par"][1, 1:] == trap).all() and t["par"][1, 0] != trap
    assert all((t[n][[3, 7]] == trap).all() for n in t)
    neg = np.flatnonzero(c["dec_status"] < 0)
    assert (t["rec"][neg] == trap).all()
    assert (t["rec"][0, 1:] == trap).all() and t["rec"][0, 0] != trap     # r1: one erasure
    a = Arena(s)
    a.check(a.run(engine))


def test_ptrs_status_minus_one_and_three_beside_healthy(engine, oracle):
    bbs = [1352, 1350, 520, 104, 1350, 2056, 40]
    c = build_case(oracle, 5, 5, bbs, ["r1", "rmax", "ooo"], seed=55)
    assert c["enc_status"].tolist() == [0, -1, 0, 0, -1, 0, 0]
    assert c["dec_status"].tolist() == [0, -1, 0, 0, -1, 0, 0]
    run_case(engine, c, "mixed", seed=9)
    c3 = build_case(oracle, 32, 4, [1352, 520, 2064, 40], ["malformed", "r1"], seed=31)
    assert c3["dec_status"].tolist() == [-3, 0, -3, 0]
    run_case(engine, c3, "all", seed=10)


def test_ptrs_k_plus_m_over_256(engine, oracle):
    """m > 1 and k + m > 256 as the ragged encode treats it: every group's XOR parity in its
    first parity block, the call returns -1; the decode reports -1 where a recovery block is
    held."""
    c = build_case(oracle, 250, 7, [16, 24, 1352], ["r1", "none"], seed=3)
    assert c["enc_status"].tolist() == [-1, -1, -1] and c["dec_status"].tolist() == [-1, 0, -1]
    _, out = run_case(engine, c, "all", seed=11)
    assert out["enc_rc"] == -1
    assert out["enc_kernels"] == "xor_ptrs_kernel"


# ------------------------------------------------------------------ names, graphs, -2
def test_ptrs_kernel_names_and_grids(engine, oracle):
    _, out = run_case(engine, mixed_case(oracle, 32, 4, 7), "mixed")
    assert out["enc_kernels"] == "xor_ptrs_kernel + gf_ptrs_kernel<encode>"
    assert out["dec_kernels"].endswith("gf_ptrs_kernel<decode>")
    assert "ragged_decode_status_kernel" in out["dec_kernels"]
    assert "ragged_kernel<" not in out["enc_kernels"] + out["dec_kernels"]
    # 7 groups x 1 chunk of 4 outputs: 2 workgroups of 4 waves
    assert out["enc_grids"] == {"xor_ptrs_kernel": 2, "gf_ptrs_kernel": 2}
    assert out["dec_grids"]["gf_ptrs_kernel"] == 2
    _, out = run_case(engine, mixed_case(oracle, 10, 1, 7), "mixed")
    assert out["enc_kernels"] == "xor_ptrs_kernel"
    assert out["dec_kernels"].endswith("xor_ptrs_kernel") and "gf_" not in out["dec_kernels"]
    _, out = run_case(engine, mixed_case(oracle, 1, 3, 7), "all")
    assert out["enc_kernels"] == out["dec_kernels"] == "copy_ptrs_kernel"
    _, out = run_case(engine, mixed_case(oracle, 10, 20, 7), "all")     # 5 chunks of 4 outputs
    assert out["enc_grids"]["gf_ptrs_kernel"] == 9


def test_ptrs_decode_graph_capture_tables_rewritten(oracle):
    """One captured decode replayed twice, the block table rewritten in place in between so that
    it names other blocks (a second copy of the receive sets, the groups rotated by one): each
    replay equals the eager result for its table."""
    import torch
    from quic_amd.fec import FecEngine
    k, m, G = 32, 4, 6
    c = build_case(oracle, k, m, [1352] * G, ["r1", "rmax", "ooo"], seed=77)
    s = scatter(c, "all", seed=13)
    eng = FecEngine(0)
    try:
        eng.reserve(k, m, 1352, G)
        a = Arena(s)
        # the second table: group g decodes the receive set of group g + 1 (rows rotated too)
        rot = np.roll(np.arange(G), -1)
        tab2 = fec.block_ptrs(a.view, s["tabs"]["recv"][rot])
        rows = [dev(c["rows"]), dev(c["rows"][rot])]
        tabs = [a.tab["recv"].clone(), tab2]
        # rec entries: every group may recover up to rmax blocks under either table
        rec_all = np.array([[s["off"][("rec", g, j)] for j in range(c["rmax"])] for g in range(G)])
        rec_tab = fec.block_ptrs(a.view, rec_all)
        rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        table, rows_in = tabs[0].clone(), rows[0].clone()

        def reset():
            a.h.load(s["image"])
            rr.fill_(9)
            st.fill_(7)
            torch.cuda.synchronize()

        def result():
            return a.h.host().copy(), host(rr).copy(), host(st).copy()

        eager = []
        for t, r in zip(tabs, rows):
            reset()
            eng.decode_ptrs_recovered(k, m, 1352, t, r, rec_tab, rr, status=st)
            eager.append(result())
        assert (eager[0][0] != eager[1][0]).any()
        reset()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.decode_ptrs_recovered(k, m, 1352, table, rows_in, rec_tab, rr, status=st,
                                      stream=stream.cuda_stream)
        torch.cuda.synchronize()
        for t, r, want in zip(tabs, rows, eager):
            reset()
            table.copy_(t)
            rows_in.copy_(r)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                graph.replay()
            for x, y in zip(result(), want):
                np.testing.assert_array_equal(x, y)
            a.h.check_guards()
        # and the first table's result is the oracle's
        exp = s["image"].copy()
        for g in range(G):
            ro = int(c["rec_off"][g])
            for j in range(int(c["nrec"][g])):
                o = s["off"][("rec", g, j)]
                exp[o:o + 1352] = c["rec_exp"][ro + j * 1352:ro + (j + 1) * 1352]
        np.testing.assert_array_equal(eager[0][0], exp)
        np.testing.assert_array_equal(eager[0][1], c["rec_rows"])
    finally:
        eng.close()


def test_ptrs_call_level_minus_two(engine):
    import ctypes
    import torch
    L, h = engine.lib, engine._h
    k, m, G = 5, 2, 3
    buf = torch.zeros(G * (2 * k + 2 * m) * 64, dtype=torch.uint8, device="cuda")
    tin = fec.block_ptrs(buf, np.arange(G * k).reshape(G, k) * 64)
    tout = fec.block_ptrs(buf, (G * k + np.arange(G * m).reshape(G, m)) * 64)
    rows = torch.zeros((G, k), dtype=torch.uint8, device="cuda")
    rr = torch.zeros((G, m), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    enc, dec = L.qfec_encode_batch_ptrs, L.qfec_decode_batch_ptrs_recovered
    assert enc(h, k, m, G, None, 64, None, p(tout), None, None) == -2    # a NULL table
    assert enc(h, k, m, G, None, 64, p(tin), None, None, None) == -2
    assert enc(h, k, m, -1, None, 64, p(tin), p(tout), None, None) == -2  # groups < 0
    assert enc(h, k, m, G, None, 0, p(tin), p(tout), None, None) == -2   # no d_bb, bb_all = 0
    assert dec(h, k, m, G, None, 64, None, p(rows), p(tout), p(rr), None, None) == -2
    assert dec(h, k, m, G, None, 64, p(tin), p(rows), None, p(rr), None, None) == -2
    assert dec(h, k, m, -1, None, 64, p(tin), p(rows), p(tout), p(rr), None, None) == -2
    assert dec(h, k, m, G, None, 0, p(tin), p(rows), p(tout), p(rr), None, None) == -2
    assert dec(h, k, m, G, None, 64, p(tin), None, p(tout), p(rr), None, None) == -2
    # more (group, chunk) units than 32 bits count: refused before anything is enqueued
    assert enc(h, k, 8, 1 << 30, None, 64, p(tin), p(tout), None, None) == -2
    assert b"units" in L.qfec_last_error()
    with pytest.raises(fec.FecError):
        engine.encode_ptrs(k, m, 0, tin, tout)
    torch.cuda.synchronize()
    assert int(buf.max()) == 0
    # and a valid call with the same tables works
    assert engine.encode_ptrs(k, m, 64, tin, tout) == 0
    torch.cuda.synchronize()
