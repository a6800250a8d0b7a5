"""Mixed-code batches on the GPU: every group names its own (k, m) through an index into a code
set (qfec_*_batch_mixed*), in one call, against the CPU oracle called once per group with that
group's (k, m, bb).  Bit-exact.  Output buffers are pre-filled with a poison byte: the gaps
between groups, a tail canary, every rec entry past a group's erasure count and the regions of
groups with a negative status (but the XOR parity block of an encode -1) must still hold it
afterwards; row tags past a group's k hold poison on input.  Run with -m gpu.

tests/test_mixed_abi.py checks the construction of these cases on the CPU."""
import numpy as np
import pytest

from quic_amd import fec
from tests.test_gpu_ragged import (GF_SIZES, KINDS, POISON, XOR_EXTRA, dev, host, receive_rows,
                                   up16)
from tests import test_gpu_ragged as RG

pytestmark = pytest.mark.gpu

# k + m = 257 is the -1 band
CODES = [(10, 1), (1, 3), (2, 2), (3, 2), (5, 5), (32, 4), (10, 20), (250, 5), (250, 7)]
PER_CODE = 8                      # 72 groups, then the special ones
ROW_POISON = 0xEE                 # row tags past k_g, and every tag of a group without a code
# the cached-cenc path of the prep: these matrices do not fit in LDS beside one wave's scratch
BIG_CODES = [(128, 128), (120, 120), (100, 100), (128, 16)]


def kinds_of(k, m):
    """The receive-set kinds a code can carry (a row tag is 8 bits: with k + m > 256 neither
    every parity row nor min(k, m) of them can be tagged)."""
    if k + m > 256:
        return ["none", "r1", "parity_only", "ooo"]
    return KINDS


def group_specs(codes, per_code, seed, special=True):
    """(code index, bb, kind) per group: every code per_code times, its kinds and sizes cycling,
    plus (special) two m > 1 groups with bb % 8 != 0, one with bb = 0, one with code = ncodes and
    one with code = 255; then a seeded shuffle, so the four waves of a workgroup hold different
    codes."""
    specs = []
    for ci, (k, m) in enumerate(codes):
        pool = GF_SIZES + (XOR_EXTRA if (m == 1 or k <= 1) else [])
        kinds = kinds_of(k, m)
        for j in range(per_code):
            specs.append((ci, pool[(3 * ci + j) % len(pool)], kinds[j % len(kinds)]))
    if special:
        gf = [ci for ci, (k, m) in enumerate(codes) if k > 1 and m > 1 and k + m <= 256]
        specs += [(gf[0], 1350, "r1"), (gf[-1], 20, "malformed"), (gf[len(gf) // 2], 0, "none"),
                  (len(codes), 64, "none"), (255, 64, "none")]
    rng = np.random.default_rng(seed)
    return [specs[i] for i in rng.permutation(len(specs))]


_CASES = {}


def build_mixed(O, codes, specs, seed):
    """One mixed batch and everything the oracle says about it (cached, read-only)."""
    key = (tuple(codes), tuple(specs), seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed)
    G, nc = len(specs), len(codes)
    kmax = max(k for k, _ in codes)
    rmax = max(min(k, m) for k, m in codes)
    c = dict(codes=list(codes), G=G, kmax=kmax, rmax=rmax, specs=list(specs),
             code=np.array([s[0] for s in specs], np.uint8),
             bb=np.array([s[1] for s in specs], np.int32))

    def counts(ci):   # blocks in, parity, recovered; a group without a code gets a small region
        return (codes[ci][0], codes[ci][1], min(codes[ci])) if ci < nc else (2, 2, 2)

    off = {n: [] for n in ("data", "par", "rec")}
    run = dict(data=0, par=0, rec=0)
    for g, (ci, bb, _) in enumerate(specs):
        for n, cnt in zip(("data", "par", "rec"), counts(ci)):
            off[n].append(run[n])
            run[n] = up16(run[n] + cnt * max(bb, 16)) + (16 if g % 2 == 0 else 0)
    for n in off:
        c[n + "_off"] = np.array(off[n], np.int64)
        c[n + "_bytes"] = run[n] + 64
    c["data"] = np.full(c["data_bytes"], 0x11, np.uint8)
    c["blocks"] = np.full(c["data_bytes"], 0x22, np.uint8)
    c["rows"] = np.full((G, kmax), ROW_POISON, np.uint8)
    c["par_exp"] = np.full(c["par_bytes"], POISON, np.uint8)
    c["rec_exp"] = np.full(c["rec_bytes"], POISON, np.uint8)
    c["enc_status"] = np.zeros(G, np.int32)
    c["dec_status"] = np.zeros(G, np.int32)
    c["rec_rows"] = np.full((G, rmax), 255, np.uint8)
    c["nrec"] = np.zeros(G, np.int64)
    c["kind"] = [s[2] for s in specs]
    c["decodable"] = np.zeros(G, bool)       # built to be decoded: the oracle must say 0
    for g, (ci, bb, kind) in enumerate(specs):
        if ci >= nc:
            c["enc_status"][g] = c["dec_status"][g] = -2
            continue
        k, m = codes[ci]
        if bb < 1:                           # skipped: nothing read or written, status 0
            c["rows"][g, :k] = np.arange(k)
            continue
        data = rng.integers(0, 256, size=(k, bb), dtype=np.uint8)
        par, rc = O.encode_ptrs(k, m, bb, list(data))
        do, po, ro = (int(c[n + "_off"][g]) for n in ("data", "par", "rec"))
        c["data"][do:do + k * bb] = data.ravel()
        c["enc_status"][g] = rc
        nwritten = m if rc == 0 else 1       # -1: the XOR parity only (cauchy_256.cpp:1519-1534)
        c["par_exp"][po:po + nwritten * bb] = par[:nwritten].ravel()
        if kind == "malformed" and (m == 1 or k < 2):
            kind = c["kind"][g] = "r1"       # no -3 exists for m = 1 / k = 1
        rows = receive_rows(rng, k, m, kind)
        blocks = np.concatenate([data, par])[rows]
        c["blocks"][do:do + k * bb] = blocks.ravel()
        c["rows"][g, :k] = rows
        if kind == "malformed":
            c["dec_status"][g] = -1 if (bb % 8 or k + m > 256) else -3
            continue
        arrs, rows2, drc = O.decode_blocks(k, m, bb, list(blocks), rows)
        c["dec_status"][g] = drc
        c["decodable"][g] = not (m > 1 and k > 1 and (bb % 8 or k + m > 256))
        if drc != 0:
            continue
        rec = []
        if k <= 1:
            if rows[0] != 0:
                rec = [(0, blocks[0])]
        else:
            slots = [i for i in range(k) if rows[i] >= k]
            for sl in (slots[:1] if m == 1 else slots):
                if rows2[sl] < k:
                    rec.append((rows2[sl], arrs[sl]))
        assert [x for x, _ in rec] == sorted(x for x, _ in rec)
        for j, (x, blk) in enumerate(rec):
            np.testing.assert_array_equal(blk, data[x])      # the oracle recovered the data
            c["rec_rows"][g][j] = x
            c["rec_exp"][ro + j * bb:ro + (j + 1) * bb] = blk
        c["nrec"][g] = len(rec)
    _CASES[key] = c
    return c


def main_case(O, seed=1):
    return build_mixed(O, CODES, group_specs(CODES, PER_CODE, seed), seed)


def run_mixed(engine, cs, c, what="both"):
    import torch
    G = c["G"]
    code, bb = dev(c["code"]), dev(c["bb"])
    out = {}
    if what in ("both", "encode"):
        par = torch.full((c["par_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        out["enc_rc"] = engine.encode_mixed(cs, code, bb, dev(c["data"]), dev(c["data_off"]), par,
                                            dev(c["par_off"]), status=st)
        out["enc_kernels"] = fec.last_kernels()
        out["par"], out["enc_status"] = host(par), host(st)
    if what in ("both", "decode"):
        rec = torch.full((c["rec_bytes"],), POISON, dtype=torch.uint8, device="cuda")
        rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        blocks, rows = dev(c["blocks"]), dev(c["rows"])
        out["dec_rc"] = engine.decode_mixed_recovered(cs, code, bb, blocks, dev(c["data_off"]),
                                                      rows, rec, dev(c["rec_off"]), rr, status=st)
        out["dec_kernels"] = fec.last_kernels()
        out["rec"], out["rec_rows"], out["dec_status"] = host(rec), host(rr), host(st)
        np.testing.assert_array_equal(host(blocks), c["blocks"])     # inputs untouched
        np.testing.assert_array_equal(host(rows), c["rows"])
    return out


def check(c, out):
    """Status, rec_rows (255 up to the set's rmax) and every byte, gaps and canary included."""
    if "par" in out:
        np.testing.assert_array_equal(out["enc_status"], c["enc_status"])
        np.testing.assert_array_equal(out["par"], c["par_exp"])
    if "rec" in out:
        np.testing.assert_array_equal(out["dec_status"], c["dec_status"])
        np.testing.assert_array_equal(out["rec_rows"], c["rec_rows"])
        np.testing.assert_array_equal(out["rec"], c["rec_exp"])


@pytest.fixture(scope="module")
def codeset(engine):
    cs = engine.codeset(CODES)
    yield cs
    cs.close()


def test_mixed_vs_oracle(engine, oracle, codeset):
    c = main_case(oracle)
    assert (codeset.kmax, codeset.mmax, codeset.rmax) == (250, 20, 10)
    assert c["G"] == 77 and (c["enc_status"] == -2).sum() == 2
    out = run_mixed(engine, codeset, c)
    assert out["enc_rc"] == 0 and out["dec_rc"] == 0       # every rejection is per group
    check(c, out)
    for names in (out["enc_kernels"], out["dec_kernels"]):
        assert "ragged" not in names and "ptrs" not in names
    assert "gf_mixed_kernel<encode>" in out["enc_kernels"]
    assert "xor_copy_mixed_kernel<encode>" in out["enc_kernels"]
    assert "gf_mixed_kernel<decode>" in out["dec_kernels"]
    assert "decode_prep_mixed_kernel" in out["dec_kernels"]
    assert "<cached>" not in out["dec_kernels"]             # this set's matrices sit in LDS
    assert "xor_copy_mixed_kernel<decode>" in out["dec_kernels"]
    assert "gf_mixed_kernel" in fec.last_grids()


def test_mixed_without_status(engine, oracle, codeset):
    """status may be NULL: the same bytes."""
    import torch
    c = main_case(oracle)
    code, bb = dev(c["code"]), dev(c["bb"])
    par = torch.full((c["par_bytes"],), POISON, dtype=torch.uint8, device="cuda")
    engine.encode_mixed(codeset, code, bb, dev(c["data"]), dev(c["data_off"]), par,
                        dev(c["par_off"]))
    rec = torch.full((c["rec_bytes"],), POISON, dtype=torch.uint8, device="cuda")
    rr = torch.full((c["G"], c["rmax"]), 9, dtype=torch.uint8, device="cuda")
    engine.decode_mixed_recovered(codeset, code, bb, dev(c["blocks"]), dev(c["data_off"]),
                                  dev(c["rows"]), rec, dev(c["rec_off"]), rr)
    np.testing.assert_array_equal(host(par), c["par_exp"])
    np.testing.assert_array_equal(host(rec), c["rec_exp"])
    np.testing.assert_array_equal(host(rr), c["rec_rows"])


@pytest.mark.parametrize("k,m", [(32, 4), (10, 1)])
def test_one_code_set_equals_ragged(engine, oracle, k, m):
    """A set of one code: the same bytes as qfec_encode_batch_ragged /
    qfec_decode_batch_ragged_recovered on identical input."""
    c = RG.mixed_case(oracle, k, m, 7)
    rg = RG.run_device(engine, c)
    RG.check(c, rg)
    cs = engine.codeset([(k, m)])
    try:
        assert (cs.kmax, cs.mmax, cs.rmax) == (k, m, min(k, m))
        c2 = dict(c, code=np.zeros(c["G"], np.uint8))
        out = run_mixed(engine, cs, c2)
    finally:
        cs.close()
    for key in ("par", "enc_status", "rec", "rec_rows", "dec_status"):
        np.testing.assert_array_equal(out[key], rg[key])


def test_mixed_empty_and_single(engine, oracle, codeset):
    import torch
    c = main_case(oracle)
    # G = 0 through the C entry points (torch gives an empty tensor a null pointer, and a NULL
    # array is -2 whatever the group count): nothing is launched, nothing is written
    buf = torch.full((64,), POISON, dtype=torch.uint8, device="cuda")
    t8 = torch.zeros(16, dtype=torch.uint8, device="cuda")
    t32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    t64 = torch.zeros(2, dtype=torch.int64, device="cuda")
    p, L = fec._ptr, engine.lib
    assert L.qfec_encode_batch_mixed(engine._h, codeset._h, 0, p(t8), p(t32), p(buf), p(t64),
                                     p(buf), p(t64), p(t32), None) == 0
    assert fec.last_kernels() == ""
    assert L.qfec_decode_batch_mixed_recovered(engine._h, codeset._h, 0, p(t8), p(t32), p(buf),
                                               p(t64), p(t8), p(buf), p(t64), p(t8), None,
                                               None) == 0
    assert fec.last_kernels() == "" and (host(buf) == POISON).all()
    # G = 1: the first (32, 4) group with two losses of the main batch, alone
    g = next(i for i, s in enumerate(c["specs"]) if s[0] == CODES.index((32, 4)) and s[2] == "ooo")
    one = build_mixed(oracle, CODES, [c["specs"][g]], 5)
    assert one["nrec"][0] == 2
    check(one, run_mixed(engine, codeset, one))


def test_mixed_unit_limit(engine, codeset):
    """More than 2^31 - 1 (group, chunk) units is -2 before anything is enqueued or allocated:
    the arrays are never read, so tiny ones stand in for them."""
    import torch
    t8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
    t32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    t64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = fec._ptr
    L = engine.lib
    # (10, 20): 5 chunks of 4 parity rows, 3 chunks of 4 recovered blocks
    for nchunk, dec in ((5, False), (3, True)):
        G = (2 ** 31 - 1) // nchunk + 1
        if dec:
            rc = L.qfec_decode_batch_mixed_recovered(engine._h, codeset._h, G, p(t8), p(t32),
                                                     p(t8), p(t64), p(t8), p(t8), p(t64), p(t8),
                                                     None, None)
        else:
            rc = L.qfec_encode_batch_mixed(engine._h, codeset._h, G, p(t8), p(t32), p(t8), p(t64),
                                           p(t8), p(t64), None, None)
        assert rc == -2 and b"units" in L.qfec_last_error()
    assert L.qfec_encode_batch_mixed(engine._h, codeset._h, -1, p(t8), p(t32), p(t8), p(t64), p(t8),
                                     p(t64), None, None) == -2
    # misaligned base
    assert L.qfec_encode_batch_mixed(engine._h, codeset._h, 1, p(t8), p(t32), p(t8[8:]), p(t64),
                                     p(t8), p(t64), None, None) == -2
    torch.cuda.synchronize()


def test_codeset_errors(engine, codeset):
    from quic_amd.fec import FecEngine
    for bad in ([], [(5, 5)] * 33, [(0, 3)], [(256, 1)], [(5, 0)], [(5, 5), (10, -1)]):
        with pytest.raises(fec.FecError) as e:
            engine.codeset(bad)
        assert e.value.rc == -2
    cs = engine.codeset([(5, 5)] * 32)                    # 32 codes, duplicates: allowed
    cs.close()
    cs = engine.codeset([(45, 255), (255, 1000)])   # k + m > 256 is a per-group matter
    assert (cs.kmax, cs.mmax, cs.rmax) == (255, 1000, 255)
    cs.close()
    other = FecEngine(0)
    try:                                                   # a set of another context
        import torch
        t8 = torch.zeros(64, dtype=torch.uint8, device="cuda")
        t32 = torch.zeros(16, dtype=torch.int32, device="cuda")
        t64 = torch.zeros(8, dtype=torch.int64, device="cuda")
        with pytest.raises(fec.FecError) as e:
            other.encode_mixed(codeset, t8[:1], t32[:1], t8, t64[:1], t8, t64[:1])
        assert e.value.rc == -2
    finally:
        other.close()


def test_mixed_graph_replay_rewritten(oracle):
    """One capture (encode and decode) after qfec_codeset_reserve, replayed twice; between the
    replays code, bb, the offsets, rows and data are rewritten in place with another batch.  Both
    replays are exact."""
    import torch
    from quic_amd.fec import FecEngine
    a, b = main_case(oracle, 1), main_case(oracle, 2)
    assert a["G"] == b["G"] and not np.array_equal(a["code"], b["code"])
    G = a["G"]
    size = {n: max(a[n + "_bytes"], b[n + "_bytes"]) for n in ("data", "par", "rec")}
    eng = FecEngine(0)
    cs = eng.codeset(CODES)
    try:
        cs.reserve(G)

        def padded(c, name, n):
            x = np.full(size[n], POISON, np.uint8)
            x[:len(c[name])] = c[name]
            return x

        d = dict(code=dev(a["code"]), bb=dev(a["bb"]), data=dev(padded(a, "data", "data")),
                 blocks=dev(padded(a, "blocks", "data")), rows=dev(a["rows"]),
                 data_off=dev(a["data_off"]), par_off=dev(a["par_off"]), rec_off=dev(a["rec_off"]))
        par = torch.full((size["par"],), POISON, dtype=torch.uint8, device="cuda")
        rec = torch.full((size["rec"],), POISON, dtype=torch.uint8, device="cuda")
        rr = torch.full((G, a["rmax"]), 9, dtype=torch.uint8, device="cuda")
        est = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        dst = torch.full((G,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            eng.encode_mixed(cs, d["code"], d["bb"], d["data"], d["data_off"], par, d["par_off"],
                             status=est, stream=s.cuda_stream)
            eng.decode_mixed_recovered(cs, d["code"], d["bb"], d["blocks"], d["data_off"],
                                       d["rows"], rec, d["rec_off"], rr, status=dst,
                                       stream=s.cuda_stream)
        torch.cuda.synchronize()
        for c in (a, b):
            for name in ("code", "bb", "rows", "data_off", "par_off", "rec_off"):
                d[name].copy_(torch.from_numpy(c[name]))
            d["data"].copy_(torch.from_numpy(padded(c, "data", "data")))
            d["blocks"].copy_(torch.from_numpy(padded(c, "blocks", "data")))
            for t, v in ((par, POISON), (rec, POISON), (rr, 9), (est, 7), (dst, 7)):
                t.fill_(v)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                gr.replay()
            got = dict(par=host(par), rec=host(rec), rec_rows=host(rr), enc_status=host(est),
                       dec_status=host(dst))
            exp = dict(c, par_exp=padded(c, "par_exp", "par"), rec_exp=padded(c, "rec_exp", "rec"))
            check(exp, got)
    finally:
        cs.close()
        eng.close()


def host_case(O):
    """The main batch for the host forms, which refuse a size < 1: its bb = 0 group gets 8."""
    specs = [s if s[1] > 0 else (s[0], 8, s[2]) for s in group_specs(CODES, PER_CODE, 1)]
    return build_mixed(O, CODES, specs, 1)


def test_mixed_host_forms(oracle):
    """The same batch through the host entry points with 1 MiB chunks (several of them, a few
    groups each): the oracle's bytes, the poison everywhere else."""
    import torch
    from quic_amd.fec import FecEngine
    c = host_case(oracle)
    G = c["G"]
    assert int(c["data_bytes"]) > 2 << 20          # at least three chunks
    eng = FecEngine(0)
    cs = eng.codeset(CODES)
    try:
        eng.set_option("host_chunk_mb", 1)
        code_h, bb_h = torch.from_numpy(c["code"]), torch.from_numpy(c["bb"])
        par = torch.full((int(c["par_bytes"]),), POISON, dtype=torch.uint8)
        est = torch.full((G,), 7, dtype=torch.int32)
        assert fec.encode_mixed_host_into(eng, cs, code_h, bb_h, torch.from_numpy(c["data"]),
                                          torch.from_numpy(c["data_off"]), par,
                                          torch.from_numpy(c["par_off"]), est) == 0
        assert "gf_mixed_kernel<encode>" in fec.last_kernels()
        rec = torch.full((int(c["rec_bytes"]),), POISON, dtype=torch.uint8)
        rr = torch.full((G, c["rmax"]), 9, dtype=torch.uint8)
        dst = torch.full((G,), 7, dtype=torch.int32)
        fec.decode_mixed_recovered_host_into(eng, cs, code_h, bb_h, torch.from_numpy(c["blocks"]),
                                             torch.from_numpy(c["data_off"]),
                                             torch.from_numpy(c["rows"]), rec,
                                             torch.from_numpy(c["rec_off"]), rr, dst)
        assert "ragged" not in fec.last_kernels()
        check(c, dict(par=par.numpy(), enc_status=est.numpy(), rec=rec.numpy(),
                      rec_rows=rr.numpy(), dec_status=dst.numpy()))
        # descending offsets are refused, nothing is written
        with pytest.raises(fec.FecError):
            fec.encode_mixed_host_into(eng, cs, code_h[:2].contiguous(), bb_h[:2].contiguous(),
                                       torch.from_numpy(c["data"]),
                                       torch.from_numpy(c["data_off"][:2][::-1].copy()), par,
                                       torch.from_numpy(c["par_off"][:2].copy()), None)
        np.testing.assert_array_equal(par.numpy(), c["par_exp"])
    finally:
        cs.close()
        eng.close()


def test_queue_mixed_bucket(engine, oracle):
    """qfec_batch_set_mixed: 12 groups of three presets, max_groups = 6.  The flush happens at the
    sixth group whatever its code, as one mixed encode; redundancy and revived packets equal
    those of the same groups run through the group layer with the CPU codec."""
    import random
    from quic_amd import fec_group as F
    from tests import ref_framing as R
    F.set_fec_overrides(0, 0)
    confs = [F.FEC_5_5, F.FEC_10_10, F.FEC_10_20]
    rnd = random.Random(31)
    groups = []
    for gi in range(12):
        conf = confs[rnd.randrange(3)] if gi >= 3 else confs[gi]
        k = F.k_from_conf(conf)
        base = 7000 + gi * 64
        top = rnd.randrange(40, 1351)
        lens = [rnd.randrange(40, top + 1) for _ in range(k)]
        lens[rnd.randrange(k)] = top
        sent = [(base + i, bytes(rnd.getrandbits(8) for _ in range(n)), rnd.choice([1, 2, 4, 6]))
                for i, n in enumerate(lens)]
        groups.append((conf, base, sent))
    assert len({c for c, _, _ in groups[:6]}) == 3 and len({c for c, _, _ in groups[6:]}) >= 2

    def sender(conf, base, sent):
        s = F.QuicFecGroup(base, conf)
        for pn, p, pl in sent:
            s.UpdateSentList(2, pn, pl, p)
        return s

    def receiver(conf, base, sent, par, drop):
        r = F.QuicFecGroup(base, conf)
        for i, (pn, p, pl) in enumerate(sent):
            if i not in drop:
                r.UpdateReceivedList(2, pn, pl, p, False)
        for pn, d, pl in par:
            r.UpdateFec(2, pn, pl, d)
        assert r.CanRevive()
        return r

    batch = F.FecBatch(engine, max_groups=6, max_delay_us=10**9)
    batch.set_mixed(True)
    senders = []
    for gi, (conf, base, sent) in enumerate(groups):
        s = sender(conf, base, sent)
        done = batch.add_encode(s)
        senders.append(s)
        assert done == (6 if gi % 6 == 5 else 0)           # the sixth group, whatever its code
        if done:
            names = fec.last_kernels()
            assert names.count("gf_mixed_kernel<encode>") == 1 and "ragged" not in names
            assert "gf_mixed_kernel" in fec.last_grids()
        else:
            with pytest.raises(ValueError):
                batch.set_mixed(False)                     # not while groups are queued
    assert batch.pending() == 0
    receivers, expected = [], []
    for (conf, base, sent), s in zip(groups, senders):
        k, m = F.k_from_conf(conf), F.m_from_conf(conf)
        par, st = s.getRedundancyPackets()
        assert st == 0 and par == R.redundancy(oracle, k, m, base, sent)[0]   # the CPU codec's
        drop = set(rnd.sample(range(k), rnd.randrange(1, 4)))
        r = receiver(conf, base, sent, par, drop)
        assert batch.add_decode(r) in (0, 6)
        receivers.append(r)
        expected.append((drop, sent))
    assert batch.pending() == 0 and "gf_mixed_kernel<decode>" in fec.last_kernels()
    for r, (drop, sent) in zip(receivers, expected):
        rev, st = r.getRevivedPackets()
        assert st == 0
        assert sorted((pn, p) for pn, p, _ in rev) == sorted((sent[i][0], sent[i][1]) for i in drop)


@pytest.mark.parametrize("codes,cached", [([(128, 16), (100, 100)], False), (BIG_CODES, True)])
def test_mixed_large_matrices(engine, oracle, codes, cached):
    """Sets with large encode matrices on a dozen groups of 104 bytes: (128, 16) with (100, 100)
    still fits in LDS beside the solve's scratch; BIG_CODES does not, and the prep reads the
    matrices through the cache."""
    kinds = ["r1", "rmax", "ooo", "malformed", "none", "parity_only"]
    specs = [(i % len(codes), 104, kinds[(i + i // len(codes)) % len(kinds)]) for i in range(12)]
    c = build_mixed(oracle, codes, specs, 11)
    assert (c["dec_status"] == -3).any() and c["nrec"].max() >= 100
    cs = engine.codeset(codes)
    try:
        out = run_mixed(engine, cs, c)
    finally:
        cs.close()
    check(c, out)
    assert ("decode_prep_mixed_kernel<cached>" in out["dec_kernels"]) == cached
