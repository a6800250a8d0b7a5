"""GPU (for the device tensors only; no kernel is launched): what the device wrappers hand to the
library, recorded by a stand-in engine and compared with include/quic_fec.h's parameter order,
and the argument errors the five receiver entry points share."""
import ctypes

import pytest

from quic_amd import fec
from tests.test_ragged_layout import CTX, assert_call, header_params, recording_engine

STREAM = 0x51


def _receiver_args(k, m, device):
    """A good argument set of every receiver form for G = 2 groups of (k, m), bb = 8, by the
    header's parameter names without their d_ / h_ prefix."""
    import torch
    G, bb = 2, 8
    n, rmax = G * (k + m), min(k, m)
    b_off, _, r_off, tot = fec.ragged_layout(k, m, [bb] * G)

    def z(shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device=device)
    i32 = torch.int32
    return dict(k=k, m=m, block_bytes=bb, groups=G,
                bb=torch.full((G,), bb, dtype=i32, device=device), pkt=z((n, 48)), pkt_stride=48,
                pkt_len=z(n, i32), ad_len=None, ad_len_all=16, pn_len=None, pn_len_all=1,
                blocks=z(tot[0]),
                blocks_off=torch.from_numpy(b_off).to(device), rows=z((G, k)), open_len=z(n, i32),
                rec=z(tot[2]), rec_off=torch.from_numpy(r_off).to(device), rec_rows=z((G, rmax)),
                status=z(G, i32), rev=z((G * rmax, 16)), rev_stride=16, rev_len=z(G * rmax, i32),
                rev_pn_len=z(G * rmax), stream=None)


def _call(eng, symbol, args):
    """Call `symbol` of the real library with `args` in the header's order."""
    vals = []
    for name in header_params(symbol):
        v = eng._h if name == "ctx" else args[name[2:] if name[:2] in ("d_", "h_") else name]
        vals.append(ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v)
    return getattr(eng.lib, symbol)(*vals)


@pytest.mark.gpu
def test_device_wrappers_marshal_and_receiver_argument_errors(engine):
    import torch
    k, m, bb, G = 2, 1, 8, 2
    n, rmax = G * (k + m), 1
    u8, i32 = torch.uint8, torch.int32

    def z(shape, dtype=u8):
        return torch.zeros(shape, dtype=dtype, device="cuda")
    eng = recording_engine()
    d_off, p_off, r_off, tot = (torch.from_numpy(a).cuda() if hasattr(a, "dtype") else a
                                for a in fec.ragged_layout(k, m, [bb] * G))
    bbt = torch.full((G,), bb, dtype=i32, device="cuda")
    data, par, rec = z(tot[0]), z(tot[1]), z(tot[2])
    rows, rr, st = z((G, k)), z((G, rmax)), z(G, i32)
    hdr, pkt, pay, rev = z((n, 20)), z((n, 48)), z((G * k, 12)), z((G * rmax, 16))
    hl, pl, kl, al, ol = (z(n, i32) for _ in range(5))
    yl, pn, npn = z(G * k, i32), z(G * k), z(n)
    rl, rpn = z(G * rmax, i32), z(G * rmax)
    udata, upar, urec = z((G, k, bb)), z((G, m, bb)), z((G, rmax, bb))
    rag = dict(ctx=CTX, k=k, m=m, groups=G, d_bb=bbt, stream=STREAM)
    uni = dict(ctx=CTX, k=k, m=m, block_bytes=bb, groups=G, stream=STREAM)
    hdr_arr = dict(d_hdr=hdr, hdr_stride=20, d_hdr_len=hl, hdr_len_all=0)
    hdr_none = dict(d_hdr=None, hdr_stride=0, d_hdr_len=None, hdr_len_all=0)
    pkt_out = dict(d_pkt=pkt, pkt_stride=48, d_pkt_len=kl)

    assert eng.encode_ragged(k, m, bbt, data, d_off, par, p_off, stream=STREAM) == 0
    assert_call(eng, "qfec_encode_batch_ragged", **rag, d_data=data, d_data_off=d_off,
                d_parity=par, d_par_off=p_off, d_status=None)
    assert eng.decode_ragged_recovered(k, m, bbt, data, d_off, rows, rec, r_off, rr, st,
                                       stream=STREAM) == 0
    assert_call(eng, "qfec_decode_batch_ragged_recovered", **rag, d_blocks=data,
                d_blocks_off=d_off, d_rows_in=rows, d_rec=rec, d_rec_off=r_off, d_rec_rows=rr,
                d_status=st)

    seal = dict(d_data=data, d_data_off=d_off, d_parity=par, d_par_off=p_off)
    eng.seal_groups_ragged(k, m, bbt, data, d_off, par, p_off, hdr, hl, pl, pkt, kl, stream=STREAM)
    assert_call(eng, "qfec_seal_groups_batch_ragged", **rag, **seal, **hdr_arr, d_pt_len=pl,
                **pkt_out)
    eng.seal_groups_ragged(k, m, bbt, data, d_off, par, p_off, None, 0, None, pkt, kl,
                           encode=True, status=st, stream=STREAM)
    assert_call(eng, "qfec_encode_seal_groups_batch_ragged", **rag, **seal, **hdr_none,
                d_pt_len=None, **pkt_out, d_status=st)
    with pytest.raises(ValueError) as e:       # status is the encode's
        eng.seal_groups_ragged(k, m, bbt, data, d_off, par, p_off, hdr, hl, pl, pkt, kl, status=st,
                               stream=STREAM)
    assert e.type is ValueError and eng.lib.calls == []

    recv = dict(d_pkt=pkt, pkt_stride=48, d_pkt_len=kl, d_blocks=data, d_blocks_off=d_off,
                d_rows=rows, d_open_len=ol, d_rec=rec, d_rec_off=r_off, d_rec_rows=rr)
    eng.open_decode_ragged(k, m, bbt, pkt, kl, 13, data, d_off, rows, ol, rec, r_off, rr,
                           stream=STREAM)
    assert_call(eng, "qfec_open_decode_batch_ragged", **rag, **recv, d_ad_len=None, ad_len_all=13,
                d_status=None)
    eng.open_decode_ragged(k, m, bbt, pkt, kl, al, data, d_off, rows, ol, rec, r_off, rr, status=st,
                           stream=STREAM)
    assert_call(eng, "qfec_open_decode_batch_ragged", **rag, **recv, d_ad_len=al, ad_len_all=0,
                d_status=st)

    frag = dict(rag)
    del frag["m"]
    eng.frame_blocks_ragged(k, bbt, pay, yl, pn, data, d_off, stream=STREAM)
    assert_call(eng, "qfec_frame_blocks_batch_ragged", **frag, d_pay=pay, pay_stride=12,
                d_pay_len=yl, d_pn_len=pn, pn_len_all=0, d_data=data, d_data_off=d_off,
                d_status=None)
    eng.frame_blocks_ragged(k, bbt, pay, yl, 2, data, d_off, status=st, stream=STREAM)
    assert_call(eng, "qfec_frame_blocks_batch_ragged", **frag, d_pay=pay, pay_stride=12,
                d_pay_len=yl, d_pn_len=None, pn_len_all=2, d_data=data, d_data_off=d_off,
                d_status=st)
    eng.extract_revived_ragged(k, m, bbt, rec, r_off, rr, None, rev, rl, stream=STREAM)
    assert_call(eng, "qfec_extract_revived_batch_ragged", **rag, d_rec=rec, d_rec_off=r_off,
                d_rec_rows=rr, d_status=None, d_rev=rev, rev_stride=16, d_rev_len=rl,
                d_rev_pn_len=None)
    eng.extract_revived_ragged(k, m, bbt, rec, r_off, rr, st, rev, rl, rpn, stream=STREAM)
    assert_call(eng, "qfec_extract_revived_batch_ragged", **rag, d_rec=rec, d_rec_off=r_off,
                d_rec_rows=rr, d_status=st, d_rev=rev, rev_stride=16, d_rev_len=rl,
                d_rev_pn_len=rpn)
    eng.frame_encode_seal_ragged(k, m, bbt, data, d_off, par, p_off, hdr, hl, pay, yl, pn, pkt, kl,
                                 status=st, stream=STREAM)
    assert_call(eng, "qfec_frame_encode_seal_groups_batch_ragged", **rag, **seal, **hdr_arr,
                d_pay=pay, pay_stride=12, d_pay_len=yl, d_pn_len=pn, pn_len_all=0, **pkt_out,
                d_status=st)
    eng.frame_encode_seal_ragged(k, m, bbt, data, d_off, par, p_off, None, 0, pay, yl, 4, pkt, kl,
                                 stream=STREAM)
    assert_call(eng, "qfec_frame_encode_seal_groups_batch_ragged", **rag, **seal, **hdr_none,
                d_pay=pay, pay_stride=12, d_pay_len=yl, d_pn_len=None, pn_len_all=4, **pkt_out,
                d_status=None)
    eng.open_decode_extract_ragged(k, m, bbt, pkt, kl, al, npn, data, d_off, rows, ol, rec, r_off,
                                   rr, rev, rl, rev_pn_len=rpn, status=st, stream=STREAM)
    assert_call(eng, "qfec_open_decode_extract_batch_ragged", **rag, **recv, d_ad_len=al,
                ad_len_all=0, d_pn_len=npn, pn_len_all=0, d_status=st, d_rev=rev, rev_stride=16,
                d_rev_len=rl, d_rev_pn_len=rpn)
    eng.open_decode_extract_ragged(k, m, bbt, pkt, kl, 13, 1, data, d_off, rows, ol, rec, r_off,
                                   rr, rev, rl, stream=STREAM)
    assert_call(eng, "qfec_open_decode_extract_batch_ragged", **rag, **recv, d_ad_len=None,
                ad_len_all=13, d_pn_len=None, pn_len_all=1, d_status=None, d_rev=rev,
                rev_stride=16, d_rev_len=rl, d_rev_pn_len=None)

    useal = dict(d_data=udata, d_parity=upar, **hdr_arr, **pkt_out)
    eng.seal_groups(k, m, bb, udata, upar, hdr, hl, pl, pkt, kl, stream=STREAM)
    assert_call(eng, "qfec_seal_groups_batch", **uni, **useal, d_pt_len=pl, pt_len_all=0)
    eng.seal_groups(k, m, bb, udata, upar, hdr, hl, 7, pkt, kl, encode=True, stream=STREAM)
    assert_call(eng, "qfec_encode_seal_groups_batch", **uni, **useal, d_pt_len=None, pt_len_all=7)
    eng.open_decode(k, m, bb, pkt, kl, 13, udata, rows, ol, urec, rr, stream=STREAM)
    assert_call(eng, "qfec_open_decode_batch", **uni, d_pkt=pkt, pkt_stride=48, d_pkt_len=kl,
                d_ad_len=None, ad_len_all=13, d_blocks=udata, d_rows=rows, d_open_len=ol,
                d_rec=urec, d_rec_rows=rr, d_status=None)
    eng.open_decode(k, m, bb, pkt, kl, al, udata, rows, ol, urec, rr, status=st, stream=STREAM)
    assert_call(eng, "qfec_open_decode_batch", **uni, d_pkt=pkt, pkt_stride=48, d_pkt_len=kl,
                d_ad_len=al, ad_len_all=0, d_blocks=udata, d_rows=rows, d_open_len=ol,
                d_rec=urec, d_rec_rows=rr, d_status=st)

    # the receiver's argument errors, with the real library: -2 and one text in all five forms,
    # before anything is launched (an empty encode first empties the thread's kernel record)
    forms = [("qfec_open_decode_batch", "cuda"), ("qfec_open_decode_batch_host", "cpu"),
             ("qfec_open_decode_batch_ragged", "cuda"),
             ("qfec_open_decode_batch_ragged_host", "cpu"),
             ("qfec_open_decode_extract_batch_ragged", "cuda")]
    good = {dev: _receiver_args(k, m, dev) for dev in ("cuda", "cpu")}
    wide = {dev: _receiver_args(255, 1, dev) for dev in ("cuda", "cpu")}
    assert engine.lib.qfec_encode_batch(engine._h, k, m, bb, 0, None, None, None) == 0
    assert fec.last_kernels() == ""
    errors = [(wide, {}, "k + m > 255 (row tag 255 marks an unfilled slot)"),
              (good, dict(pkt_stride=0), "bad pkt_stride"),
              (good, dict(pkt_len=None), "null buffer"),
              (good, dict(ad_len=None, ad_len_all=-1), "bad ad_len_all")]
    for args, change, text in errors:
        for symbol, dev in forms:
            assert _call(engine, symbol, dict(args[dev], **change)) == -2, (symbol, text)
            assert engine.lib.qfec_last_error().decode() == text, symbol
            assert fec.last_kernels() == "", symbol
    # with no group each form keeps its own rule: the uniform device form still checks k + m
    # and ad_len_all, the host forms k + m (the ragged one its arrays too) and then return 0,
    # the ragged device forms check everything
    none = [("qfec_open_decode_batch", wide, {}, -2),
            ("qfec_open_decode_batch", good, dict(ad_len_all=-1), -2),
            ("qfec_open_decode_batch_host", wide, {}, -2),
            ("qfec_open_decode_batch_host", good,
             dict(pkt_stride=0, pkt_len=None, ad_len_all=-1), 0),
            ("qfec_open_decode_batch_ragged_host", wide, {}, -2),
            ("qfec_open_decode_batch_ragged_host", good, dict(pkt_len=None), -2),
            ("qfec_open_decode_batch_ragged_host", good, dict(pkt_stride=0, ad_len_all=-1), 0),
            ("qfec_open_decode_batch_ragged", good, dict(pkt_stride=0), -2),
            ("qfec_open_decode_extract_batch_ragged", good, dict(ad_len_all=-1), -2)]
    for symbol, args, change, rc in none:
        assert _call(engine, symbol, dict(args[dict(forms)[symbol]], groups=0, **change)) == rc, \
            (symbol, change)
        assert fec.last_kernels() == "", symbol
