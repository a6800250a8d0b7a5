// fec_host.cpp — the host-pointer entry points of libquic_fec.so (qfec_*_host).
//
// Each entry point checks its arguments, declares the arrays it stages on the device once
// (a StageList, fec_host_plan.h) and hands the one pipeline below its kernels.  Sizes, chunks
// and the carve of the staging come from that list (fec_host_plan.cpp, plain C++ checked on
// the CPU); this file holds the HIP calls.
#include <algorithm>

#include "fec_host_plan.h"
#include "fec_internal.h"
#include "pp_null.h"

using namespace qfec;

namespace {

// Host-pointer batches, chunked and pipelined: chunk i's H2D (s_in), kernels (stream)
// and D2H (s_out) are ordered by events, and NB staging buffers rotate, so the copy-in of
// chunk i + 1 and the copy-out of chunk i - 1 overlap the kernels of chunk i (PCIe is
// full duplex).  The kernels of all chunks stay on one stream, so the decode workspace is
// never shared by two chunks in flight.
// kernels(n): enqueues the kernels of a chunk of n groups on c->stream; it reads the stages'
// device pointers.  Every copy is derived from the stage list.
template <class K>
int host_pipeline_body(qfec_ctx* c, StageList& L, const Chunks& ch, K&& kernels) {
    if (!c->s_in) {
        QF_HIP(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
        QF_HIP(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
        for (int b = 0; b < qfec_ctx::NB; ++b) {
            QF_HIP(hipEventCreateWithFlags(&c->ev_in[b], hipEventDisableTiming));
            QF_HIP(hipEventCreateWithFlags(&c->ev_done[b], hipEventDisableTiming));
            QF_HIP(hipEventCreateWithFlags(&c->ev_out[b], hipEventDisableTiming));
        }
    }
    const size_t bytes = staging_bytes(L, ch);
    for (int b = 0; b < qfec_ctx::NB; ++b) QF_HIP(c->pbuf[b].ensure(bytes));
    for (long long i = 0; i < ch.count(); ++i) {
        const long long g0 = ch.begin(i), n = ch.begin(i + 1) - g0;
        const int b = (int)(i % qfec_ctx::NB);
        if (i >= qfec_ctx::NB) QF_HIP(hipStreamWaitEvent(c->s_in, c->ev_out[b], 0));
        stage_carve(L, g0, n, (uint8_t*)c->pbuf[b].p);
        for (int j = 0; j < L.n; ++j) {
            const Stage& s = L.s[j];
            if (s.present && s.src)
                QF_HIP(hipMemcpyAsync(s.dev, (const uint8_t*)s.src + s.host_at(g0), s.bytes,
                                      hipMemcpyHostToDevice, c->s_in));
        }
        QF_HIP(hipEventRecord(c->ev_in[b], c->s_in));
        QF_HIP(hipStreamWaitEvent(c->stream, c->ev_in[b], 0));
        const int r = kernels(n);
        if (r) return r;
        QF_HIP(hipEventRecord(c->ev_done[b], c->stream));
        QF_HIP(hipStreamWaitEvent(c->s_out, c->ev_done[b], 0));
        for (int j = 0; j < L.n; ++j) {
            const Stage& s = L.s[j];
            if (!s.present || !s.dst) continue;
            uint8_t* dst = (uint8_t*)s.dst + s.host_at(g0);
            if (s.row_width)
                QF_HIP(hipMemcpy2DAsync(dst, s.row_pitch, s.dev, s.row_pitch, s.row_width,
                                        s.bytes / s.row_pitch, hipMemcpyDeviceToHost, c->s_out));
            else
                QF_HIP(hipMemcpyAsync(dst, s.dev, s.bytes, hipMemcpyDeviceToHost, c->s_out));
        }
        QF_HIP(hipEventRecord(c->ev_out[b], c->s_out));
    }
    QF_HIP(hipStreamSynchronize(c->s_out));
    return 0;
}

template <class K>
int host_pipeline(qfec_ctx* c, StageList& L, const Chunks& ch, K&& kernels) {
    // the kernels of every chunk run on the context stream: order them after the last eager
    // use of the decode workspace, and the next use after them
    const int r = with_workspace(c, c->stream,
                                 [&] { return host_pipeline_body(c, L, ch, kernels); });
    // On any error, drain all three streams before returning, so no copy of an earlier chunk
    // still writes into the caller's host buffers after the call has returned.
    if (r)
        for (hipStream_t s : {c->s_in, c->stream, c->s_out})
            if (s) (void)hipStreamSynchronize(s);
    return r;
}

// Uniform batches: chunks of the host_chunk_mb option (64 MiB), and at least the
// host_min_groups option's groups (512).
template <class K>
int host_pipeline_uniform(qfec_ctx* c, StageList& L, long long groups, K&& kernels) {
    Chunks ch;
    ch.groups = groups;
    ch.uniform = uniform_chunk(groups, stage_bytes(L, 0, 1), c->tune.host_chunk_mb,
                               c->tune.host_min_groups);
    return host_pipeline(c, L, ch, kernels);
}

// the stages every ragged form hands its kernels as a RaggedView
struct RaggedStages {
    Stage &bb, &in_rel, &out_rel, &status;
    RaggedStages(StageList& L, const int* h_bb, int* h_status)
        : bb(L.dense(sizeof(int32_t)).in(h_bb)),
          in_rel(L.dense(sizeof(long long))),
          out_rel(L.dense(sizeof(long long))),
          status(L.dense(sizeof(int32_t)).out(h_status)) {}
    RaggedView view() const {
        return {bb.as<int32_t>(), in_rel.as<long long>(), out_rel.as<long long>()};
    }
};

// Ragged batches.  The chunks are cut on group boundaries by bytes (the host_chunk_mb option;
// a chunk holds at least one group): a chunk stages the span of its groups in each packed
// array, and the offsets it hands the kernels (the stages in_rel / out_rel) are relative to
// its first group.  An output span is first filled with the caller's bytes, so the copy back
// returns every byte the kernels did not write (gaps, groups with a negative status, entries
// past a group's erasure count) as it was.
template <class K>
int host_pipeline_ragged(qfec_ctx* c, StageList& L, long long groups, const Stage& in,
                         const Stage& out, RaggedStages& rs, K&& kernels) {
    Chunks ch;
    const char* msg = nullptr;
    const long long target = (long long)std::max(1, c->tune.host_chunk_mb) << 20;
    const int rc = ragged_chunks(L, in, out, groups, target, &ch, &msg);
    if (rc) return fail(rc, msg);
    rs.in_rel.in(ch.in_rel.data());
    rs.out_rel.in(ch.out_rel.data());
    return host_pipeline(c, L, ch, kernels);
}

// One column of qfec_ragged_layout: the packed offsets of a buffer the host forms keep on
// the device (the sender's parity: column 1, the receiver's blocks: column 0).
int device_layout(int k, int m, long long G, const int* bb, int column,
                  std::vector<long long>* off) {
    off->resize((size_t)G);
    long long* col[3] = {nullptr, nullptr, nullptr};
    col[column] = off->data();
    if (qfec_ragged_layout(k, m, G, bb, col[0], col[1], col[2], nullptr) == 0) return 0;
    for (long long g = 0; g < G; ++g)
        if (bb[g] < 1) return fail(-2, "bb[g] < 1");
    return fail(-2, "the packed layout overflows");
}

}  // namespace

extern "C" {

int qfec_decode_batch_recovered_host(qfec_ctx* c, int k, int m, int bb, long long groups,
                                     const unsigned char* h_blocks, const unsigned char* h_rows,
                                     unsigned char* h_rec, unsigned char* h_rec_rows,
                                     int* h_status) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups == 0) return 0;
    if (!h_blocks || !h_rows || !h_rec || !h_rec_rows) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const int rmax = std::min(k, m);
    StageList L;
    Stage& db = L.dense((size_t)k * bb).in(h_blocks);
    Stage& dre = L.dense((size_t)rmax * bb).out(h_rec);
    Stage& dr = L.dense(k).in(h_rows);
    Stage& drr = L.dense(rmax).out(h_rec_rows);
    Stage& ds = L.dense(sizeof(int32_t)).out(h_status);
    return host_pipeline_uniform(c, L, groups, [&](long long n) {
        return decode_impl(c, k, m, bb, n, db.dev, dr.dev, {dre.dev, drr.dev, true},
                           ds.as<int32_t>(), c->stream);
    });
}

// Sender, host memory to host memory: data blocks and packet headers in, every sealed packet
// of each group out (the parity never leaves the device).  Chunked and pipelined as the
// other host batches: H2D of chunk i + 1 and D2H of chunk i - 1 overlap chunk i's encode and
// seal.
int qfec_encode_seal_groups_batch_host(qfec_ctx* c, int k, int m, int bb, long long groups,
                                       const unsigned char* h_data, const unsigned char* h_hdr,
                                       long long hdr_stride, const int* h_hdr_len,
                                       int hdr_len_all, const int* h_pt_len, int pt_len_all,
                                       unsigned char* h_pkt, long long pkt_stride,
                                       int* h_pkt_len) {
    int rc = seal_groups_args(c, k, m, bb, groups, {h_data, h_pkt, h_pkt_len},
                              rows_of(h_hdr, hdr_stride, h_hdr_len, hdr_len_all), h_pt_len,
                              pt_len_all, rows_out_of(h_pkt, pkt_stride, h_pkt_len));
    if (rc) return rc;
    if (groups == 0) return 0;
    if (hdr_stride <= 0 && h_hdr) return fail(-2, "host headers need a row stride > 0");
    if (pkt_stride <= 0) return fail(-2, "host packets need a row stride > 0");
    // the encode's -1 (cauchy_256.cpp:1530-1534): no packet is sealed, as on the device path
    // (the parity rows past P0 would be stale staging bytes sent with valid tags)
    if (encode_p0_only(k, m, bb))
        return fail(-1, "unsupported (k + m > 256 or block_bytes % 8 != 0)");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t np = (size_t)(k + m);   // packets per group
    const size_t len_g = np * sizeof(int32_t);
    StageList L;
    Stage& dd = L.dense((size_t)k * bb).in(h_data);
    Stage& dp = L.dense((size_t)m * bb);
    Stage& dh = L.dense(np * hdr_stride, h_hdr != nullptr).in(h_hdr);
    Stage& dk = L.dense(np * pkt_stride).out(h_pkt);
    Stage& dkl = L.dense(len_g).out(h_pkt_len);
    Stage& dhl = L.dense(len_g, h_hdr_len != nullptr).in(h_hdr_len);
    Stage& dpl = L.dense(len_g, h_pt_len != nullptr).in(h_pt_len);
    return host_pipeline_uniform(c, L, groups, [&](long long n) -> int {
        const int r = encode_impl(c, k, m, bb, n, dd.dev, dp.dev, c->stream);
        if (r) return r;
        // packet rows are copied back whole: zero the staging rows first, so the bytes of
        // a row past its packet are zeros (as the device path leaves them untouched), not
        // an earlier chunk's packets
        QF_HIP(hipMemsetAsync(dk.dev, 0, dk.bytes, c->stream));
        const Rows hdr{dh.dev, dh.dev ? hdr_stride : 0, dhl.as<int32_t>(),
                       dh.dev ? hdr_len_all : 0};
        QF_HIP(launch_null_seal_groups(k, m, bb, n, dd.dev, dp.dev, hdr, dpl.as<int32_t>(),
                                       pt_len_all, {dk.dev, pkt_stride, dkl.as<int32_t>()},
                                       c->stream));
        return 0;
    });
}

// Receiver, host memory to host memory: wire packets in, the recovered blocks (and, if asked,
// each packet's open length) out.  Chunked and pipelined as the other host batches.
int qfec_open_decode_batch_host(qfec_ctx* c, int k, int m, int bb, long long groups,
                                const unsigned char* h_pkt, long long pkt_stride,
                                const int* h_pkt_len, const int* h_ad_len, int ad_len_all,
                                unsigned char* h_rec, unsigned char* h_rec_rows, int* h_status,
                                int* h_open_len) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    // no group: k + m alone is checked, then there is nothing to do
    if (groups == 0) return open_decode_args(k, m, false, {}, 0, nullptr, 0);
    if ((rc = open_decode_args(k, m, true, {h_pkt, h_pkt_len, h_rec, h_rec_rows}, pkt_stride,
                               h_ad_len, ad_len_all)))
        return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t np = (size_t)(k + m);
    const size_t len_g = np * sizeof(int32_t);
    const int rmax = std::min(k, m);
    StageList L;
    Stage& dk = L.dense(np * pkt_stride).in(h_pkt);
    Stage& dkl = L.dense(len_g).in(h_pkt_len);
    Stage& dal = L.dense(len_g, h_ad_len != nullptr).in(h_ad_len);
    Stage& dol = L.dense(len_g).out(h_open_len);
    Stage& db = L.dense((size_t)k * bb);
    Stage& dr = L.dense(k);
    Stage& dre = L.dense((size_t)rmax * bb).out(h_rec);
    Stage& drr = L.dense(rmax).out(h_rec_rows);
    Stage& ds = L.dense(sizeof(int32_t)).out(h_status);
    return host_pipeline_uniform(c, L, groups, [&](long long n) {
        return open_decode_impl(c, k, m, bb, n, {dk.dev, pkt_stride, dkl.as<int32_t>(), 0},
                                {nullptr, 0, dal.as<int32_t>(), ad_len_all}, db.dev, dr.dev,
                                dol.as<int32_t>(), {dre.dev, drr.dev, true}, ds.as<int32_t>(),
                                c->stream);
    });
}

int qfec_encode_batch_host(qfec_ctx* c, int k, int m, int bb, long long groups,
                           const unsigned char* h_data, unsigned char* h_parity) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups == 0) return 0;
    if (!h_data || !h_parity) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    StageList L;
    Stage& dd = L.dense((size_t)k * bb).in(h_data);
    Stage& dp = L.dense((size_t)m * bb).out(h_parity);
    // On the reference's -1 path only P0 is written: copy back only row 0 of each group so
    // the caller's other recovery rows stay untouched.
    if (encode_p0_only(k, m, bb)) dp.rows((size_t)m * bb, bb);
    int result = 0;
    rc = host_pipeline_uniform(c, L, groups, [&](long long n) {
        const int r = encode_impl(c, k, m, bb, n, dd.dev, dp.dev, c->stream);
        if (r < -1) return r;
        if (r) result = r;
        return 0;
    });
    return rc ? rc : result;
}

int qfec_decode_batch_host(qfec_ctx* c, int k, int m, int bb, long long groups,
                           unsigned char* h_blocks, unsigned char* h_rows, int* h_status) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups == 0) return 0;
    if (!h_blocks || !h_rows) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    StageList L;
    Stage& db = L.dense((size_t)k * bb).in(h_blocks).out(h_blocks);
    Stage& dr = L.dense(k).in(h_rows).out(h_rows);
    Stage& ds = L.dense(sizeof(int32_t)).out(h_status);
    return host_pipeline_uniform(c, L, groups, [&](long long n) {
        return decode_impl(c, k, m, bb, n, db.dev, dr.dev, {db.dev, dr.dev, false},
                           ds.as<int32_t>(), c->stream);
    });
}

// ---- ragged batches
int qfec_encode_batch_ragged_host(qfec_ctx* c, int k, int m, long long groups, const int* h_bb,
                                  const unsigned char* h_data, const long long* h_data_off,
                                  unsigned char* h_parity, const long long* h_par_off,
                                  int* h_status) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    if (!h_bb || !h_data || !h_data_off || !h_parity || !h_par_off) return fail(-2, "null buffer");
    if (groups == 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    StageList L{h_bb};
    Stage& dd = L.packed(h_data_off, k).in(h_data);
    Stage& dp = L.packed(h_par_off, m).in(h_parity).out(h_parity);
    RaggedStages rs(L, h_bb, h_status);
    int result = 0;
    rc = host_pipeline_ragged(c, L, groups, dd, dp, rs, [&](long long n) {
        const int r = encode_ragged_impl(c, k, m, n, rs.view(), dd.dev, dp.dev,
                                         rs.status.as<int32_t>(), c->stream);
        if (r < -1) return r;
        if (r) result = r;
        return 0;
    });
    return rc ? rc : result;
}

int qfec_decode_batch_ragged_recovered_host(qfec_ctx* c, int k, int m, long long groups,
                                            const int* h_bb, const unsigned char* h_blocks,
                                            const long long* h_blocks_off,
                                            const unsigned char* h_rows, unsigned char* h_rec,
                                            const long long* h_rec_off,
                                            unsigned char* h_rec_rows, int* h_status) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    if (!h_bb || !h_blocks || !h_blocks_off || !h_rows || !h_rec || !h_rec_off || !h_rec_rows)
        return fail(-2, "null buffer");
    if (groups == 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const int rmax = std::min(k, m);
    StageList L{h_bb};
    Stage& db = L.packed(h_blocks_off, k).in(h_blocks);
    Stage& dre = L.packed(h_rec_off, rmax).in(h_rec).out(h_rec);
    RaggedStages rs(L, h_bb, h_status);
    Stage& dr = L.dense(k).in(h_rows);
    Stage& drr = L.dense(rmax).out(h_rec_rows);
    return host_pipeline_ragged(c, L, groups, db, dre, rs, [&](long long n) {
        return decode_ragged_impl(c, k, m, n, rs.view(), db.dev, dr.dev, dre.dev, drr.dev,
                                  rs.status.as<int32_t>(), c->stream);
    });
}

// ---- mixed-code batches: the ragged host forms with a block count per group, taken from the
// group's code (a group whose code index names no code of the set stages nothing: the device
// gives it status -2)
namespace {
struct MixedCounts {
    std::vector<int> in, par, rec;
    MixedCounts(const qfec_codeset* cs, const unsigned char* code, long long G)
        : in((size_t)G, 0), par((size_t)G, 0), rec((size_t)G, 0) {
        for (long long g = 0; g < G; ++g) {
            if (code[g] >= cs->s.ncodes) continue;
            const int k = cs->k[code[g]], m = cs->m[code[g]];
            in[(size_t)g] = k;
            par[(size_t)g] = m;
            rec[(size_t)g] = std::min(k, m);
        }
    }
};
int mixed_host_preface(qfec_ctx* c, const qfec_codeset* cs, long long groups) {
    if (!c) return fail(-2, "null context");
    if (!cs || cs->ctx != c) return fail(-2, "no code set of this context");
    if (groups < 0) return fail(-2, "groups < 0");
    return 0;
}
}  // namespace

int qfec_encode_batch_mixed_host(qfec_ctx* c, const qfec_codeset* cs, long long groups,
                                 const unsigned char* h_code, const int* h_bb,
                                 const unsigned char* h_data, const long long* h_data_off,
                                 unsigned char* h_parity, const long long* h_par_off,
                                 int* h_status) {
    int rc = mixed_host_preface(c, cs, groups);
    if (rc) return rc;
    if (!h_code || !h_bb || !h_data || !h_data_off || !h_parity || !h_par_off)
        return fail(-2, "null buffer");
    if (groups == 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const MixedCounts n(cs, h_code, groups);
    StageList L{h_bb};
    Stage& dd = L.packed(h_data_off, n.in.data()).in(h_data);
    Stage& dp = L.packed(h_par_off, n.par.data()).in(h_parity).out(h_parity);
    RaggedStages rs(L, h_bb, h_status);
    Stage& dc = L.dense(1).in(h_code);
    return host_pipeline_ragged(c, L, groups, dd, dp, rs, [&](long long g) {
        const RaggedView v = rs.view();
        return encode_mixed_impl(c, cs, g, {dc.dev, v.bb, v.in_off, v.out_off}, dd.dev, dp.dev,
                                 rs.status.as<int32_t>(), c->stream);
    });
}

int qfec_decode_batch_mixed_recovered_host(qfec_ctx* c, const qfec_codeset* cs, long long groups,
                                           const unsigned char* h_code, const int* h_bb,
                                           const unsigned char* h_blocks,
                                           const long long* h_blocks_off,
                                           const unsigned char* h_rows, unsigned char* h_rec,
                                           const long long* h_rec_off, unsigned char* h_rec_rows,
                                           int* h_status) {
    int rc = mixed_host_preface(c, cs, groups);
    if (rc) return rc;
    if (!h_code || !h_bb || !h_blocks || !h_blocks_off || !h_rows || !h_rec || !h_rec_off ||
        !h_rec_rows)
        return fail(-2, "null buffer");
    if (groups == 0) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const MixedCounts n(cs, h_code, groups);
    StageList L{h_bb};
    Stage& db = L.packed(h_blocks_off, n.in.data()).in(h_blocks);
    Stage& dre = L.packed(h_rec_off, n.rec.data()).in(h_rec).out(h_rec);
    RaggedStages rs(L, h_bb, h_status);
    Stage& dc = L.dense(1).in(h_code);
    Stage& dr = L.dense(cs->s.kmax).in(h_rows);
    Stage& drr = L.dense(cs->s.rmax).out(h_rec_rows);
    return host_pipeline_ragged(c, L, groups, db, dre, rs, [&](long long g) {
        const RaggedView v = rs.view();
        return decode_mixed_impl(c, cs, g, {dc.dev, v.bb, v.in_off, v.out_off}, db.dev, dr.dev,
                                 dre.dev, drr.dev, rs.status.as<int32_t>(), c->stream);
    });
}

// Sender, host to host, ragged: qfec_encode_seal_groups_batch_host with a block size per group.
// The parity is laid out on the device and never leaves it.
int qfec_encode_seal_groups_batch_ragged_host(qfec_ctx* c, int k, int m, long long groups,
                                              const int* h_bb, const unsigned char* h_data,
                                              const long long* h_data_off,
                                              const unsigned char* h_hdr, long long hdr_stride,
                                              const int* h_hdr_len, int hdr_len_all,
                                              const int* h_pt_len, unsigned char* h_pkt,
                                              long long pkt_stride, int* h_pkt_len,
                                              int* h_status) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    // (host data is staged, so its own alignment does not matter)
    if (!h_bb || !h_data || !h_data_off) return fail(-2, "null buffer");
    if ((rc = seal_ragged_pkt_args(k, m, rows_of(h_hdr, hdr_stride, h_hdr_len, hdr_len_all),
                                   rows_out_of(h_pkt, pkt_stride, h_pkt_len))))
        return rc;
    if (groups == 0) return 0;
    if (hdr_stride <= 0 && h_hdr) return fail(-2, "host headers need a row stride > 0");
    if (pkt_stride <= 0) return fail(-2, "host packets need a row stride > 0");
    std::vector<long long> par_off;
    if ((rc = device_layout(k, m, groups, h_bb, 1, &par_off))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t np = (size_t)(k + m);
    const size_t len_g = np * sizeof(int32_t);
    StageList L{h_bb};
    Stage& dd = L.packed(h_data_off, k).in(h_data);
    Stage& dp = L.packed(par_off.data(), m);
    RaggedStages rs(L, h_bb, h_status);
    Stage& dh = L.dense(np * hdr_stride, h_hdr != nullptr).in(h_hdr);
    Stage& dk = L.dense(np * pkt_stride).out(h_pkt);
    Stage& dkl = L.dense(len_g).out(h_pkt_len);
    Stage& dhl = L.dense(len_g, h_hdr_len != nullptr).in(h_hdr_len);
    Stage& dpl = L.dense(len_g, h_pt_len != nullptr).in(h_pt_len);
    return host_pipeline_ragged(c, L, groups, dd, dp, rs,
                                [&](long long n) -> int {
        const RaggedView v = rs.view();
        const int r = encode_ragged_impl(c, k, m, n, v, dd.dev, dp.dev, rs.status.as<int32_t>(),
                                         c->stream);
        if (r) return r;
        // rows come back whole: zeros past each packet and in rejected rows
        QF_HIP(hipMemsetAsync(dk.dev, 0, dk.bytes, c->stream));
        const Rows hdr{dh.dev, dh.dev ? hdr_stride : 0, dhl.as<int32_t>(),
                       dh.dev ? hdr_len_all : 0};
        QF_HIP(launch_null_seal_groups_ragged(k, m, n, v, dd.dev, dp.dev, true, hdr,
                                              dpl.as<int32_t>(),
                                              {dk.dev, pkt_stride, dkl.as<int32_t>()}, c->stream));
        return 0;
    });
}

// Receiver, host to host, ragged: qfec_open_decode_batch_host with a block size per group.  The
// blocks are laid out on the device; h_rec is the caller's packed buffer, and the bytes of it
// the call does not write keep the caller's values (staged in, as the ragged host decode).
int qfec_open_decode_batch_ragged_host(qfec_ctx* c, int k, int m, long long groups,
                                       const int* h_bb, const unsigned char* h_pkt,
                                       long long pkt_stride, const int* h_pkt_len,
                                       const int* h_ad_len, int ad_len_all, unsigned char* h_rec,
                                       const long long* h_rec_off, unsigned char* h_rec_rows,
                                       int* h_status, int* h_open_len) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    // no group: the arrays are still asked for, the stride and ad_len_all are not looked at
    const bool none = groups == 0;
    if ((rc = open_decode_args(k, m, true, {h_bb, h_pkt, h_pkt_len, h_rec, h_rec_off, h_rec_rows},
                               none ? 1 : pkt_stride, h_ad_len, none ? 0 : ad_len_all)))
        return rc;
    if (none) return 0;
    std::vector<long long> blk_off;
    if ((rc = device_layout(k, m, groups, h_bb, 0, &blk_off))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t np = (size_t)(k + m);
    const size_t len_g = np * sizeof(int32_t);
    const int rmax = std::min(k, m);
    StageList L{h_bb};
    Stage& db = L.packed(blk_off.data(), k);
    Stage& dre = L.packed(h_rec_off, rmax).in(h_rec).out(h_rec);
    RaggedStages rs(L, h_bb, h_status);
    Stage& dk = L.dense(np * pkt_stride).in(h_pkt);
    Stage& dkl = L.dense(len_g).in(h_pkt_len);
    Stage& dal = L.dense(len_g, h_ad_len != nullptr).in(h_ad_len);
    Stage& dol = L.dense(len_g).out(h_open_len);
    Stage& dr = L.dense(k);
    Stage& drr = L.dense(rmax).out(h_rec_rows);
    return host_pipeline_ragged(c, L, groups, db, dre, rs, [&](long long n) {
        return open_decode_ragged_impl(c, k, m, n, rs.view(),
                                       {dk.dev, pkt_stride, dkl.as<int32_t>(), 0},
                                       {nullptr, 0, dal.as<int32_t>(), ad_len_all}, nullptr, db.dev,
                                       dr.dev, dol.as<int32_t>(), dre.dev, drr.dev,
                                       rs.status.as<int32_t>(), c->stream);
    });
}

}  // extern "C"
