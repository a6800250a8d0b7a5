"""CPU: the ragged packet-protection entry points exist (library, header, ctypes table), their
Python wrappers check their arrays before any call, and the cases tests/test_gpu_pp_ragged.py
runs on the GPU are what they claim to be (built from the oracle alone)."""
import os
import re
import subprocess

import pytest

from quic_amd import _lib, fec
from tests import test_gpu_pp_ragged as T
from tests.test_ragged_layout import CTX, assert_call, recording_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qfec_seal_groups_batch_ragged", "qfec_encode_seal_groups_batch_ragged",
           "qfec_open_decode_batch_ragged", "qfec_encode_seal_groups_batch_ragged_host",
           "qfec_open_decode_batch_ragged_host"]


def test_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "quic_fec.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^QFEC_API\s+[\w\s\*]*?\b(\w+)\s*\(", text, re.M))
    for s in SYMBOLS:
        assert s in exported, s
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    # the header documents the kernel names qfec_last_kernels reports for them
    for name in ("null_seal_kernel<ragged>", "open_group_kernel<ragged>",
                 "open_assemble_kernel<ragged>"):
        assert name in text, name


def test_null_context_is_minus_two():
    L = _lib.load()
    seal = (10, 1, 0, None, None, None, None, None, None, 0, None, 0, None, None, 1400, None)
    assert L.qfec_seal_groups_batch_ragged(None, *seal, None) == -2
    assert L.qfec_encode_seal_groups_batch_ragged(None, *seal, None, None) == -2
    assert L.qfec_open_decode_batch_ragged(None, 10, 1, 0, None, None, 1400, None, None, 16, None,
                                           None, None, None, None, None, None, None, None) == -2
    assert L.qfec_encode_seal_groups_batch_ragged_host(None, 10, 1, 0, None, None, None, None, 0,
                                                       None, 0, None, None, 1400, None, None) == -2
    assert L.qfec_open_decode_batch_ragged_host(None, 10, 1, 0, None, None, 1400, None, None, 16,
                                                None, None, None, None, None) == -2


def test_wrappers_check_arrays_before_the_call():
    """dtype, rows and G consistent across bb, the offsets and the per-packet arrays: the
    engine is never touched (None), so a wrong argument cannot reach the library."""
    import torch
    k, m, G = 10, 1, 3
    n, rmax = G * (k + m), 1
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    TE, VE = TypeError, ValueError
    bb = torch.full((G,), 1352, dtype=i32)
    off = torch.arange(G, dtype=i64) * 16000
    buf = torch.zeros(G * 16000, dtype=u8)
    hdr, pkt = torch.zeros((n, 20), dtype=u8), torch.zeros((n, 1400), dtype=u8)
    lens = torch.zeros(n, dtype=i32)
    seal = fec.FecEngine.seal_groups_ragged
    good = dict(bb=bb, data_off=off, par_off=off, hdr=hdr, hdr_len=lens, pt_len=lens, pkt=pkt,
                pkt_len=lens)
    # device forms: a wrong dtype or a wrong exact shape is a TypeError, a per-packet array
    # with another number of rows a ValueError
    bad = [(dict(bb=bb.to(i64)), TE), (dict(data_off=off[:-1]), TE),
           (dict(par_off=off.to(i32)), TE), (dict(pkt=pkt[:-1]), VE),
           (dict(pkt_len=lens[:-1]), VE), (dict(pkt_len=lens.to(i64)), TE),
           (dict(pt_len=torch.zeros(n + 1, dtype=i32)), VE), (dict(pt_len=1352), TE),
           (dict(hdr=hdr[:-2]), VE), (dict(hdr_len=lens.to(torch.int16)), TE),
           (dict(pkt=pkt.to(torch.int8)), TE)]
    for b, exc in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(exc) as e:
            seal(None, k, m, a["bb"], buf, a["data_off"], buf, a["par_off"], a["hdr"],
                 a["hdr_len"], a["pt_len"], a["pkt"], a["pkt_len"], encode=True)
        assert e.type is exc, b
    opn = fec.FecEngine.open_decode_ragged
    good = dict(bb=bb, pkt=pkt, pkt_len=lens, ad_len=16, boff=off, rows=torch.zeros((G, k), dtype=u8),
                ol=lens, roff=off, rr=torch.zeros((G, rmax), dtype=u8),
                st=torch.zeros(G, dtype=i32))
    bad = [(dict(bb=bb[:-1]), TE), (dict(boff=off.to(i32)), TE), (dict(roff=off[1:]), TE),
           (dict(pkt=pkt[:-1]), VE), (dict(pkt_len=lens.to(i64)), TE), (dict(ad_len=lens[:-1]), VE),
           (dict(ol=lens[:-1]), VE), (dict(rows=torch.zeros((G, k + 1), dtype=u8)), TE),
           (dict(rr=torch.zeros((G + 1, rmax), dtype=u8)), TE),
           (dict(st=torch.zeros(G, dtype=i64)), TE)]
    for b, exc in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(exc) as e:
            opn(None, k, m, a["bb"], a["pkt"], a["pkt_len"], a["ad_len"], buf, a["boff"],
                a["rows"], a["ol"], buf, a["roff"], a["rr"], status=a["st"])
        assert e.type is exc, b
    # host forms: every wrong dtype, shape or value of a contiguous CPU tensor is a ValueError
    st = torch.zeros(G, dtype=i32)
    good = dict(bb=bb, data=buf, off=off, hdr=hdr, hdr_len=16, pt_len=lens, pkt=pkt, plen=lens,
                st=st)
    bad = [dict(bb=bb.to(i64)), dict(off=off[:-1]), dict(off=off + 8), dict(data=buf[:100]),
           dict(bb=torch.zeros(G, dtype=i32)), dict(pkt=pkt[:-1]), dict(plen=lens.to(i64)),
           dict(pt_len=lens[:-1]), dict(hdr=hdr.to(torch.int8)), dict(st=st[:-1])]
    for b in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(ValueError) as e:
            fec.encode_seal_groups_ragged_host_into(None, k, m, a["bb"], a["data"], a["off"],
                                                    a["hdr"], a["hdr_len"], a["pt_len"], a["pkt"],
                                                    a["plen"], a["st"])
        assert e.type is ValueError, b
    rr = torch.zeros((G, rmax), dtype=u8)
    good = dict(bb=bb, pkt=pkt, plen=lens, ad_len=16, rec=buf, roff=off, rr=rr, st=st, ol=lens)
    bad = [dict(bb=bb[:-1]), dict(roff=off.to(i32)), dict(roff=-off - 16), dict(rec=buf[:1000]),
           dict(pkt=pkt[:-1]), dict(plen=lens[:-1]), dict(ad_len=lens.to(i64)),
           dict(rr=torch.zeros((G, rmax + 1), dtype=u8)), dict(st=st.to(i64)), dict(ol=lens[:-1])]
    for b in bad:
        a = dict(good)
        a.update(b)
        with pytest.raises(ValueError) as e:
            fec.open_decode_ragged_host_into(None, k, m, a["bb"], a["pkt"], a["plen"], a["ad_len"],
                                             a["rec"], a["roff"], a["rr"], a["st"], a["ol"])
        assert e.type is ValueError, b
    # a buffer of the wrong kind is a TypeError: non-contiguous rows, an int where only an array
    # or None is taken
    with pytest.raises(TypeError) as e:
        fec.open_decode_ragged_host_into(None, k, m, bb, pkt[:, :1396], lens, 16, buf, off, rr, st,
                                         lens)
    assert e.type is TypeError
    with pytest.raises(TypeError) as e:
        fec.encode_seal_groups_ragged_host_into(None, k, m, bb, buf, off, hdr, 16, 1352, pkt, lens,
                                                st)
    assert e.type is TypeError


def test_host_wrappers_marshal_in_header_order():
    """The two ragged protected host wrappers hand the library what include/quic_fec.h declares,
    in its order; an absent optional array is a null pointer, an absent header a stride of 0."""
    import torch
    k, m, G = 2, 1, 2
    n, rmax = G * (k + m), 1
    u8, i32 = torch.uint8, torch.int32
    eng = recording_engine()
    d_off, _, r_off, tot = fec.ragged_layout(k, m, [8, 24])
    bb = torch.tensor([8, 24], dtype=i32)
    data, d_off = torch.zeros(tot[0], dtype=u8), torch.from_numpy(d_off)
    rec, r_off = torch.zeros(tot[2], dtype=u8), torch.from_numpy(r_off)
    hdr, pkt = torch.zeros((n, 20), dtype=u8), torch.zeros((n, 48), dtype=u8)
    hl, pl, kl, ol = (torch.zeros(n, dtype=i32) for _ in range(4))
    rr, st = torch.zeros((G, rmax), dtype=u8), torch.zeros(G, dtype=i32)
    rag = dict(ctx=CTX, k=k, m=m, groups=G, h_bb=bb)

    assert fec.encode_seal_groups_ragged_host_into(eng, k, m, bb, data, d_off, hdr, hl, pl, pkt,
                                                   kl, st) == 0
    assert_call(eng, "qfec_encode_seal_groups_batch_ragged_host", **rag, h_data=data,
                h_data_off=d_off, h_hdr=hdr, hdr_stride=20, h_hdr_len=hl, hdr_len_all=0,
                h_pt_len=pl, h_pkt=pkt, pkt_stride=48, h_pkt_len=kl, h_status=st)
    fec.encode_seal_groups_ragged_host_into(eng, k, m, bb, data, d_off, None, 0, None, pkt, kl)
    assert_call(eng, "qfec_encode_seal_groups_batch_ragged_host", **rag, h_data=data,
                h_data_off=d_off, h_hdr=None, hdr_stride=0, h_hdr_len=None, hdr_len_all=0,
                h_pt_len=None, h_pkt=pkt, pkt_stride=48, h_pkt_len=kl, h_status=None)
    assert fec.open_decode_ragged_host_into(eng, k, m, bb, pkt, kl, 13, rec, r_off, rr) == 0
    assert_call(eng, "qfec_open_decode_batch_ragged_host", **rag, h_pkt=pkt, pkt_stride=48,
                h_pkt_len=kl, h_ad_len=None, ad_len_all=13, h_rec=rec, h_rec_off=r_off,
                h_rec_rows=rr, h_status=None, h_open_len=None)
    fec.open_decode_ragged_host_into(eng, k, m, bb, pkt, kl, hl, rec, r_off, rr, st, ol)
    assert_call(eng, "qfec_open_decode_batch_ragged_host", **rag, h_pkt=pkt, pkt_stride=48,
                h_pkt_len=kl, h_ad_len=hl, ad_len_all=0, h_rec=rec, h_rec_off=r_off,
                h_rec_rows=rr, h_status=st, h_open_len=ol)


@pytest.mark.parametrize("k,m", sorted(T.OPEN_SHAPES))
def test_gpu_cases_hold_every_kind(oracle, k, m):
    """The receiver batches of the GPU tests, from the oracle alone: every kind of group the
    case must hold is there by construction (build_open_case asserts each kind's outcome and
    that every recovered block is the lost data block), and at least a third of the groups
    decode with status 0 for the seeds chosen."""
    c = T.open_case(oracle, k, m)
    G, pool = T.OPEN_SHAPES[(k, m)]
    assert c["G"] == G and set(c["bbs"]) == set(pool) and c["n"] == G * (k + m)
    have = set().union(*c["kinds"])
    assert have >= T.required_kinds(k, m, c["bbs"])
    assert 3 * int((c["status"] == 0).sum()) >= G
    assert (c["status"] == -3).any() and (c["open_len"] == -1).any()
    if (k, m) == (32, 4):
        assert c["bbs"] == [1352, 64, 1350, 8, 1352] and (c["status"] == -1).sum() == 1
    # a tile (64 consecutive packets) holds groups of different sizes, and groups straddle tiles
    per = k + m
    if G > 2:
        first_tile = {c["bbs"][p // per] for p in range(min(64, c["n"]))}
        assert len(first_tile) > 1
    if 64 % per:
        assert any((g * per) // 64 != ((g + 1) * per - 1) // 64 for g in range(G))
    assert c["n"] % 64 != 0                                  # the last tile is partial


@pytest.mark.parametrize("k,m", sorted(T.HOST_G))
def test_host_cases_need_several_chunks(oracle, k, m):
    """The host tests cut their batch into several chunks at host_chunk_mb = 1."""
    G, pool = T.HOST_G[(k, m)], T.SEAL_SHAPES[(k, m)][1]
    bbs = T.draw_sizes(k, m, G, pool)
    stride = (T.HMAX + 12 + max(bbs) + 8 + 3) // 4 * 4
    assert G * (k + m) * stride > 1 << 20        # the packet rows alone exceed one chunk
