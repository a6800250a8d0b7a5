// fec_api.cpp — host side of libquic_fec.so: the C ABI in include/quic_fec.h, except its
// host-pointer batches (fec_host.cpp).
//
// Owns per-device contexts (stream, coefficient tables, decode workspace, pinned
// staging) and maps the reference's per-group codec calls (cauchy_256.h) and the batched
// calls onto the gfx950 kernels in fec_kernels.hip.  There is no CPU compute path: every
// parity / recovered byte is produced on the GPU; if the device is unusable the calls
// fail with a negative code.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fec_host_plan.h"
#include "fec_internal.h"
#include "gf256.h"
#include "gf_mixed.h"
#include "gf_ptrs.h"
#include "pp_mixed.h"
#include "pp_null.h"

using namespace qfec;

// ------------------------------------------------------------- Cauchy table blob
// quic_amd/data/cauchy_256_tables.bin (tools/gen_cauchy_tables.py) embedded at build time:
// M2[1*254] | M3[2*253] | M4[3*252] | M5[4*251] | M6[5*250] | Y[256] | X[30876]
#ifndef QFEC_TABLES_PATH
#error "QFEC_TABLES_PATH must name quic_amd/data/cauchy_256_tables.bin"
#endif
__asm__(".section .rodata\n"
        ".balign 16\n"
        ".hidden qfec_cauchy_blob\n"
        ".globl qfec_cauchy_blob\n"
        "qfec_cauchy_blob:\n"
        ".incbin \"" QFEC_TABLES_PATH "\"\n"
        ".hidden qfec_cauchy_blob_end\n"
        ".globl qfec_cauchy_blob_end\n"
        "qfec_cauchy_blob_end:\n"
        ".previous\n");
extern "C" const unsigned char qfec_cauchy_blob[];
extern "C" const unsigned char qfec_cauchy_blob_end[];

namespace {

enum {
    T_M2 = 0, T_M3 = T_M2 + 254, T_M4 = T_M3 + 506, T_M5 = T_M4 + 756, T_M6 = T_M5 + 1004,
    T_Y = T_M6 + 1250, T_X = T_Y + 256, T_SIZE = T_X + 30876
};

thread_local std::string g_err;
thread_local std::string g_kernels;   // kernels launched by this thread's last call
thread_local std::string g_grids;     // "name=grid" of its persistent kernels

bool blob_ok() { return (qfec_cauchy_blob_end - qfec_cauchy_blob) == T_SIZE; }

// cauchy_matrix(), cauchy_256.cpp:422-480: rows y = 1..m-1, (m-1) x k.
int cauchy_rows(int k, int m, uint8_t* out) {
    if (m < 2 || k < 1 || k + m > 256) return -1;
    const uint8_t* tb = qfec_cauchy_blob;
    if (m <= 6) {
        static const int base[7] = {0, 0, T_M2, T_M3, T_M4, T_M5, T_M6};
        const int stride = 256 - m;
        for (int y = 1; y < m; ++y)
            for (int x = 0; x < k; ++x) out[(y - 1) * k + x] = tb[base[m] + (y - 1) * stride + x];
        return 0;
    }
    const int n = m - 7;
    const uint8_t* X = tb + T_X + n * 249 - n * (n + 1) / 2;
    const uint8_t* Y = tb + T_Y;
    for (int y = 1; y < m; ++y) {
        const uint8_t G = Y[y - 1];
        out[(y - 1) * k] = qfec::gf_inv(1 ^ G);
        for (int x = 1; x < k; ++x) {
            const uint8_t B = X[x - 1];
            out[(y - 1) * k + x] = qfec::gf_div(B, B ^ G);
        }
    }
    return 0;
}

using qfec::encode_rc;
using qfec::pow2_at_least;
using qfec::stream_encode_rc;
// Output chunk of a decode.  gf_stream decodes in units of 8 recovered blocks: a group with
// at most 8 losses leaves its second unit empty, and empty units read nothing, while one unit
// of 16 accumulators halves the occupancy for every group ((10, 10) at 5 losses: 0.615 ms
// with 16 against 0.544 ms).
int decode_rc(int rmax) { return std::min(pow2_at_least(rmax), 8); }

}  // namespace

int qfec::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int qfec::hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return -100 - (int)e;
}

int qfec::set_device(qfec_ctx* c) {
    g_kernels.clear();
    g_grids.clear();
    qfec::launch_timing().first = true;
    QF_HIP(hipSetDevice(c->device));
    return 0;
}

// Order this call's use of the context's decode workspace after the previous eager use
// (which may have been enqueued on another stream).  Not while `st` is capturing into a
// graph: there the calls of one capture are ordered by the capturing stream itself.
// ws_end records ws_ev on the stream of every eager use, right after its kernels, while that
// stream is still eager; ws_begin waits on it when a use arrives on another stream, whatever
// that previous stream is doing now (it may have started a capture since).  A use on the
// same stream as the last needs no wait (stream order).
int qfec::ws_begin(qfec_ctx* c, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    QF_HIP(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) return 0;
    if (c->ws_used && c->ws_stream != st) QF_HIP(hipStreamWaitEvent(st, c->ws_ev, 0));
    return 0;
}
int qfec::ws_end(qfec_ctx* c, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    QF_HIP(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) return 0;
    // HIP refuses any wait on an event whose stream is capturing at the time of the wait, even
    // if the event was recorded before the capture began.  So the completion event lives on a
    // private stream that never captures: it waits for `st` now, while `st` is eager.
    if (!c->ws_helper) QF_HIP(hipStreamCreateWithFlags(&c->ws_helper, hipStreamNonBlocking));
    QF_HIP(hipEventRecord(c->ws_tmp, st));
    QF_HIP(hipStreamWaitEvent(c->ws_helper, c->ws_tmp, 0));
    QF_HIP(hipEventRecord(c->ws_ev, c->ws_helper));
    c->ws_stream = st;
    c->ws_used = true;
    return 0;
}

namespace {

// The workspace of a call on `st`: the graph workspace while `st` is capturing.
Workspace& ws_for(qfec_ctx* c, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return c->ws_graph;
    return c->ws;
}

// A stream argument is a plain hipStream_t: NULL is HIP's null (default) stream, as
// everywhere in HIP, so calls order with the caller's other work on that stream.
hipStream_t pick(qfec_ctx*, void* s) { return (hipStream_t)s; }

// Encode coefficient table: output o = chunk*rc + j; o == 0 is the all-ones row.
int get_enc_table(qfec_ctx* c, int k, int m, int rc, const uint8_t** out) {
    auto key = std::make_tuple(k, m, rc);
    auto it = c->enc_tab.find(key);
    if (it != c->enc_tab.end()) { *out = (const uint8_t*)it->second->p; return 0; }
    const int rcp = std::max(rc, 4);
    const int nchunk = (m + rc - 1) / rc;
    std::vector<uint8_t> C((size_t)std::max(m - 1, 1) * k);
    if (cauchy_rows(k, m, C.data())) return fail(-1, "no Cauchy matrix for (k, m)");
    std::vector<uint8_t> tab((size_t)nchunk * k * rcp, 0);
    for (int o = 0; o < m; ++o) {
        const int ch = o / rc, j = o % rc;
        for (int x = 0; x < k; ++x)
            tab[((size_t)ch * k + x) * rcp + j] = o == 0 ? 1 : C[(size_t)(o - 1) * k + x];
    }
    auto buf = std::make_unique<DevBuf>();
    QF_HIP(buf->ensure(tab.size()));
    QF_HIP(hipMemcpy(buf->p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    *out = (const uint8_t*)buf->p;
    c->enc_tab.emplace(key, std::move(buf));
    return 0;
}

int get_cenc(qfec_ctx* c, int k, int m, const uint8_t** out) {
    auto key = std::make_pair(k, m);
    auto it = c->cenc_tab.find(key);
    if (it != c->cenc_tab.end()) { *out = (const uint8_t*)it->second->p; return 0; }
    std::vector<uint8_t> t((size_t)m * k, 1);
    if (k + m <= 256 && m >= 2) {
        if (cauchy_rows(k, m, t.data() + k)) return fail(-1, "no Cauchy matrix for (k, m)");
    }
    auto buf = std::make_unique<DevBuf>();
    QF_HIP(buf->ensure(t.size() + 16));   // dword loads of the last row stay in the buffer
    QF_HIP(hipMemcpy(buf->p, t.data(), t.size(), hipMemcpyHostToDevice));
    *out = (const uint8_t*)buf->p;
    c->cenc_tab.emplace(key, std::move(buf));
    return 0;
}

// What a decode of one shape needs, stated once: the dispatch below sizes its workspace from
// it, and qfec_reserve pre-sizes from the same answer.
struct DecodePlan {
    int rmax = 0;                // recovered blocks per group, at most
    int rc = 0, nchunk = 0;      // output chunk of the run-time paths and the chunks of rmax
    long long tab_gstride = 0;   // apply coefficients per group: [nchunk][k][max(rc, 4)]
    // workspace bytes per group
    size_t coef = 0;             // the apply coefficients, or a syndrome table (bsyn:: / psyn::)
    size_t slots = 0;            // output slots (m == 1: the erased slot)
    size_t nout = 0;             // recovered-block count
    size_t scratch = 0;          // slot layout in place with several chunks: [rmax][bb]
    bool cenc = false;           // reads the (k, m) encode matrix
};

DecodePlan decode_plan(int k, int m, int bb) {
    DecodePlan p;
    p.rmax = std::min(k, m);
    if (k <= 1) return p;        // cauchy_256.cpp:1257-1261: no tables at all
    p.slots = p.rmax;
    if (m == 1) return p;        // :1264-1267
    p.rc = decode_rc(p.rmax);
    p.nchunk = (p.rmax + p.rc - 1) / p.rc;
    p.tab_gstride = (long long)p.nchunk * k * std::max(p.rc, 4);
    p.coef = std::max<size_t>({(size_t)p.tab_gstride, (size_t)qfec::bsyn::kBytes,
                               (size_t)qfec::psyn::kBytes});
    p.nout = sizeof(int32_t);
    if (p.nchunk > 1) p.scratch = (size_t)p.rmax * bb;
    p.cenc = true;
    return p;
}

int reserve_workspace(Workspace& W, const DecodePlan& p, long long groups, bool scratch) {
    QF_HIP(W.ensure(W.dcoef, (size_t)groups * p.coef));
    QF_HIP(W.ensure(W.dslots, (size_t)groups * p.slots));
    QF_HIP(W.ensure(W.dnout, (size_t)groups * p.nout));
    if (scratch) QF_HIP(W.ensure(W.dscratch, (size_t)groups * p.scratch));
    return 0;
}

}  // namespace

int qfec::check_common(qfec_ctx* c, int k, int m, int bb, long long groups) {
    if (!c) return fail(-2, "null context");
    if (!blob_ok()) return fail(-2, "embedded Cauchy tables have the wrong size");
    if (k < 1 || m < 1 || bb < 1 || groups < 0) return fail(-2, "bad k / m / block_bytes / groups");
    if (k > 255) return fail(-2, "k > 255 cannot be tagged by an 8-bit row");
    return 0;
}

int qfec::encode_impl(qfec_ctx* c, int k, int m, int bb, long long G, const uint8_t* d_data,
                      uint8_t* d_par, hipStream_t st) {
    if (G == 0) return 0;
    if (k <= 1) {   // cauchy_256.cpp:1508-1516
        QF_HIP(qfec::launch_replicate(d_data, d_par, m, bb, G, st));
        return 0;
    }
    // P0 = XOR of the data (:1519-1523).  For m == 1 that is the whole answer; for
    // m > 1 with unsupported parameters the reference still writes it before
    // returning -1 (:1532-1534).
    if (m == 1 || encode_p0_only(k, m, bb)) {
        QF_HIP(qfec::launch_xor_encode(d_data, d_par, k, bb, G, (long long)m * bb, st, c->tune));
        return m == 1 ? 0 : fail(-1, "unsupported (k + m > 256 or block_bytes % 8 != 0)");
    }
    const bool aligned = ((uintptr_t)d_data & 15) == 0;
    const int rc = stream_encode_rc(k, m, bb, aligned, c->tune);
    const uint8_t* tab = nullptr;
    int rcode = get_enc_table(c, k, m, rc, &tab);
    if (rcode) return rcode;
    const qfec::Apply a{d_data, d_par, tab, nullptr, nullptr, nullptr, k, m, bb, G, rc, 0, 0,
                        (long long)m * bb, st, &c->tune};
    if ((m <= rc || rc == 8) && qfec::gf_stream_supported(k, bb, rc, c->tune) && aligned)
        QF_HIP(qfec::launch_gf_stream(a, false));
    else if (qfec::gf_dcol_supported(k, m, bb, c->tune) && aligned)
        QF_HIP(qfec::launch_gf_dcol_encode(a));
    else
        QF_HIP(qfec::launch_gf_encode(a));
    return 0;
}

// The one decode dispatch: which kernels a (k, m, bb) decode runs, for either layout.  The
// caller holds the workspace bracket (with_workspace).
int qfec::decode_impl(qfec_ctx* c, int k, int m, int bb, long long G, const uint8_t* d_blocks,
                      const uint8_t* d_rows_in, DecodeOut o, int32_t* d_status,
                      hipStream_t st) {
    if (G == 0) return 0;
    const DecodePlan p = decode_plan(k, m, bb);
    const int rmax = p.rmax, rc = p.rc;
    if (k <= 1) {   // cauchy_256.cpp:1257-1261
        if (o.compact)
            QF_HIP(qfec::launch_rec_k1(d_blocks, d_rows_in, o.out, o.rows, d_status, bb, rmax, G,
                                       st));
        else
            QF_HIP(qfec::launch_rows_k1(d_rows_in, o.rows, d_status, G, st));
        return 0;
    }
    Workspace& W = ws_for(c, st);
    int r = reserve_workspace(W, p, G, false);
    if (r) return r;
    if (m == 1) {   // :1264-1267
        QF_HIP(qfec::launch_xor_decode(d_blocks, o.out, d_rows_in, o.rows, d_status,
                                       (uint8_t*)W.dslots.p, k, bb, G, st, c->tune, o.compact));
        return 0;
    }
    const uint8_t* cenc = nullptr;
    if ((r = get_cenc(c, k, m, &cenc))) return r;
    qfec::DecodeWork w{(uint8_t*)W.dcoef.p, (uint8_t*)W.dslots.p, (int32_t*)W.dnout.p};
    // what the layout decides: which row output the prep writes, whether the kernels scatter
    // through the slot table, and the stride between the groups of `out`
    const qfec::PrepIO io{d_rows_in, o.compact ? nullptr : o.rows, o.compact ? o.rows : nullptr,
                          d_status, w};
    qfec::Apply a{d_blocks, o.out, w.coef, cenc, o.compact ? nullptr : w.slots, w.nout, k, m, bb,
                  G, rc, rmax, p.tab_gstride, (long long)(o.compact ? rmax : k) * bb, st, &c->tune};
    const bool aligned = ((uintptr_t)d_blocks & 15) == 0;
    // The compiled codes.  In each, a group's stores follow all of its reads, so the slot
    // layout in place needs no scratch.
    if (qfec::gf_dcol_supported(k, m, bb, c->tune) && rmax <= 16 && aligned) {
        // compiled (128, 16) code: syndromes, then the r x r solve
        QF_HIP(qfec::launch_decode_prep(io, cenc, k, m, bb, rc, rmax, G, st, c->tune, true));
        QF_HIP(qfec::launch_gf_dcol_syndrome(a));
        return 0;
    }
    if (qfec::gf_psyn_supported(k, m, bb, rmax, c->tune) && aligned) {
        // compiled QuicR preset code: syndromes of every parity row, then Gauss-Jordan in place
        QF_HIP(qfec::launch_decode_prep_psyn(io, cenc, k, m, bb, rmax, G, st));
        QF_HIP(qfec::launch_gf_psyn(a));
        return 0;
    }
    if (qfec::gf_bsyn_supported(k, m, bb, rmax, c->tune) && aligned &&
        ((uintptr_t)d_rows_in & 3) == 0) {
        // compiled (32, 4) x 1352 B code (configs B / C): syndromes of every parity row, then
        // the r x r solve.  Its prep reads the row tags as dwords; tags at any other address
        // take the run-time path below (decode_prep_wide_kernel reads them bytewise)
        QF_HIP(qfec::launch_decode_prep_bsyn(io, cenc, k, m, bb, rmax, G, st));
        QF_HIP(qfec::launch_gf_bsyn(a));
        return 0;
    }
    // The run-time codes: the prep's coefficients, applied in chunks of rc recovered blocks.
    QF_HIP(qfec::launch_decode_prep(io, cenc, k, m, bb, rc, rmax, G, st, c->tune));
    if (bb % 8 != 0 || k + m > 256) return 0;   // every group is a no-op or status -1
    // One primitive, the dense decode into a [G][rmax][bb] destination: the compact layout's
    // `out` is one.  The slot layout writes straight into its slots instead (`direct`) where a
    // group's stores follow all of its reads: one chunk, or out of place.  In place with
    // several chunks (units on different waves) a later chunk would read slots an earlier one
    // already overwrote, so it is the dense decode into scratch, then the scatter.
    const bool direct = !o.compact && (p.nchunk == 1 || o.out != d_blocks);
    if (!o.compact && !direct) {
        QF_HIP(W.ensure(W.dscratch, (size_t)G * p.scratch));
        a.out = (uint8_t*)W.dscratch.p;
        a.slots = nullptr;
        a.out_gstride = (long long)rmax * bb;
    }
    if (qfec::gf_stream_supported(k, bb, rc, c->tune) && aligned)
        QF_HIP(qfec::launch_gf_stream(a, true));
    else
        QF_HIP(qfec::launch_gf_decode(a));
    if (a.out != o.out)
        QF_HIP(qfec::launch_scatter_recovered(a.out, o.out, w, k, bb, rmax, G, st));
    return 0;
}

namespace {

// Default context for the single-group drop-ins (created on the caller's current device;
// QFEC_DEVICE names another, read once when the context is first needed).
std::once_flag g_default_once;
qfec_ctx* g_default = nullptr;
int g_default_rc = 0;

int default_ctx(qfec_ctx** out) {
    std::call_once(g_default_once, [] {
        int dev = 0;
        if (const char* e = getenv("QFEC_DEVICE")) dev = atoi(e);
        else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        g_default_rc = qfec_ctx_create(dev, &g_default);
    });
    *out = g_default;
    if (!g_default) return g_default_rc ? g_default_rc : fail(-2, "no default GPU context");
    return 0;
}

}  // namespace

namespace qfec {
LaunchTiming& launch_timing() {
    static thread_local LaunchTiming t;
    return t;
}

void note_kernel(const char* name) {
    // a host-pointer batch launches the same kernels once per chunk: list each once
    const std::string n(name);
    size_t at = 0;
    while ((at = g_kernels.find(n, at)) != std::string::npos) {
        const size_t end = at + n.size();
        if ((at == 0 || g_kernels.compare(at - 3, 3, " + ") == 0) &&
            (end == g_kernels.size() || g_kernels.compare(end, 3, " + ") == 0))
            return;
        at = end;
    }
    if (!g_kernels.empty()) g_kernels += " + ";
    g_kernels += n;
}

void note_grid(const char* name, unsigned grid) {
    if (!g_grids.empty()) g_grids += " ";
    g_grids += std::string(name) + "=" + std::to_string(grid);
}

int resident_blocks(const void* kern, int threads, size_t lds) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t>, int> cache;
    const auto key = std::make_tuple(kern, threads, lds);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, lds) != hipSuccess || n < 1)
        n = 1;
    cache.emplace(key, n);
    return n;
}
}  // namespace qfec

// NullDecrypter on every packet of each group, placement into the receive set, the
// recovered-blocks decode, the unfilled-group status (qfec_open_decode_batch)
int qfec::open_decode_impl(qfec_ctx* c, int k, int m, int bb, long long groups, Rows pkt,
                           Rows ad, uint8_t* d_blocks, uint8_t* d_rows, int32_t* d_open_len,
                           DecodeOut rec, int32_t* d_status, hipStream_t st) {
    QF_HIP(qfec::launch_open_groups(k, m, bb, groups, pkt, ad, d_blocks, d_rows, d_open_len, st));
    int rc = decode_impl(c, k, m, bb, groups, d_blocks, d_rows, rec, d_status, st);
    if (rc) return rc;
    QF_HIP(qfec::launch_open_status(k, std::min(k, m), groups, d_rows, rec.rows, d_status, st));
    return 0;
}

namespace {

// The options of qfec_ctx_set_option / qfec_ctx_get_option: a member of the context's Tune, the
// values it accepts (lo > hi: read only, set does not know the name) and any further rule.
struct Opt {
    const char* name;
    int qfec::Tune::*member;
    int lo, hi;
    bool (*ok)(int) = nullptr;
};
using Tu = qfec::Tune;
const Opt kOptions[] = {
    {"cus", &Tu::cus, 1, 0},
    {"xor_slots", &Tu::xor_slots, 2, 4},       {"xor_waves", &Tu::xor_waves, 1, 4},
    {"dma", &Tu::dma, 0, 1},                   {"stream", &Tu::stream, 0, 1},
    {"stream_ring", &Tu::stream_ring, 4, 36},  {"stream_grid", &Tu::stream_grid, 0, 1 << 20},
    {"const_enc", &Tu::const_enc, 0, 1},       {"stream_static", &Tu::stream_static, 0, 1},
    {"ring_wide", &Tu::ring_wide, 0, 1},       {"psyn_wide", &Tu::psyn_wide, 0, 2},
    {"ring_split", &Tu::ring_split, 0, 1},
    {"dcol", &Tu::dcol, 0, 1},                 {"dcol_grid", &Tu::dcol_grid, 0, 1 << 20},
    {"dcol_depth", &Tu::dcol_depth, 6, 8, [](int v) { return v != 7; }},
    {"bsyn", &Tu::bsyn, 0, 1},
    {"bsyn_depth", &Tu::bsyn_depth, 3, 7, [](int v) { return (v & 1) != 0; }},
    {"psyn", &Tu::psyn, 0, 1},
    {"pd", &Tu::pd, 1, 3},                     {"flat", &Tu::flat, 0, 1},
    {"enc_rc", &Tu::enc_rc, 2, 8, [](int v) { return (v & (v - 1)) == 0; }},
    {"prep_lane", &Tu::prep_lane, 0, 1},
    {"host_chunk_mb", &Tu::host_chunk_mb, 1, 4096},
    {"host_min_groups", &Tu::host_min_groups, 1, 1 << 20},
    {"ring_wg", &Tu::ring_wg, -1, 1 << 20},    {"bsyn_wg", &Tu::bsyn_wg, -1, 1 << 20},
    {"psyn_wg", &Tu::psyn_wg, 0, 1 << 20},     {"dcol_wg", &Tu::dcol_wg, 0, 1 << 20},
    {"stream_wg", &Tu::stream_wg, -1, 1 << 20}, {"xor_wg", &Tu::xor_wg, 0, 1 << 20},
    {"arr_optimistic", &Tu::arr_optimistic, 0, 1},
};

const Opt* find_option(const char* name) {
    for (const Opt& o : kOptions)
        if (strcmp(o.name, name) == 0) return &o;
    return nullptr;
}

}  // namespace

// ======================================================================== C ABI
// (the internal qfec:: functions defined among the entry points keep their C++ linkage)
extern "C" {

int qfec_version(void) { return 1; }

const char* qfec_last_error(void) { return g_err.c_str(); }

const char* qfec_last_kernels(void) { return g_kernels.c_str(); }

const char* qfec_last_grids(void) { return g_grids.c_str(); }

int qfec_set_timing_events(void* start_event, void* stop_event) {
    if (!start_event != !stop_event) return fail(-2, "set both timing events or neither");
    qfec::LaunchTiming& t = qfec::launch_timing();
    t.start = (hipEvent_t)start_event;
    t.stop = (hipEvent_t)stop_event;
    t.first = true;
    return 0;
}

int qfec_ctx_set_option(qfec_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(-2, "null context or option name");
    std::lock_guard<std::mutex> lk(c->mu);
    const Opt* o = find_option(name);
    if (!o || o->lo > o->hi) return fail(-2, std::string("unknown option: ") + name);
    if (value < o->lo || value > o->hi || (o->ok && !o->ok(value)))
        return fail(-2, std::string("option value out of range: ") + name);
    c->tune.*o->member = value;
    return 0;
}

int qfec_ctx_get_option(qfec_ctx* c, const char* name, int* value) {
    if (!c || !name || !value) return fail(-2, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const Opt* o = find_option(name);
    if (!o) return fail(-2, std::string("unknown option: ") + name);
    *value = c->tune.*o->member;
    return 0;
}

int qfec_cauchy_matrix(int k, int m, unsigned char* out) {
    if (!blob_ok()) return fail(-2, "embedded Cauchy tables have the wrong size");
    return cauchy_rows(k, m, out);
}

int qfec_ctx_create(int device, qfec_ctx** out) {
    if (!out) return fail(-2, "null out");
    *out = nullptr;
    int n = 0;
    QF_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(-2, "no such HIP device");
    auto c = std::make_unique<qfec_ctx>();
    c->device = device;
    c->ws_graph.keep = true;
    QF_HIP(hipSetDevice(device));
    int cus = 0;
    QF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    c->tune.cus = cus > 0 ? cus : 256;
    QF_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    QF_HIP(hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming));
    QF_HIP(hipEventCreateWithFlags(&c->ws_tmp, hipEventDisableTiming));
    *out = c.release();
    return 0;
}

void qfec_ctx_destroy(qfec_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // the last use of the workspace may be on any stream the caller used (and may have
    // destroyed since), and a graph replay may still read the graph workspace: wait for the
    // whole device rather than for a stored stream handle
    if (c->ws_used || c->ws_graph.dslots.p) (void)hipDeviceSynchronize();
    for (hipStream_t s : {c->stream, c->s_in, c->s_out})
        if (s) (void)hipStreamSynchronize(s);
    if (c->ws_ev) (void)hipEventDestroy(c->ws_ev);
    if (c->ws_tmp) (void)hipEventDestroy(c->ws_tmp);
    for (int b = 0; b < qfec_ctx::NB; ++b)
        for (hipEvent_t e : {c->ev_in[b], c->ev_done[b], c->ev_out[b]})
            if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {c->stream, c->s_in, c->s_out, c->ws_helper})
        if (s) (void)hipStreamDestroy(s);
    delete c;
}

int qfec_encode_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                      const unsigned char* d_data, unsigned char* d_parity, void* stream) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups && (!d_data || !d_parity)) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    return encode_impl(c, k, m, bb, groups, d_data, d_parity, pick(c, stream));
}

// The two device decodes differ only in where they write (DecodeOut).
static int decode_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                        const unsigned char* d_blocks, const unsigned char* d_rows_in,
                        DecodeOut o, int* d_status, void* stream) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups && (!d_blocks || !d_rows_in || !o.out || !o.rows)) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return decode_impl(c, k, m, bb, groups, d_blocks, d_rows_in, o, (int32_t*)d_status, st);
    });
}

int qfec_decode_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                      const unsigned char* d_blocks, const unsigned char* d_rows_in,
                      unsigned char* d_out, unsigned char* d_rows_out, int* d_status,
                      void* stream) {
    return decode_batch(c, k, m, bb, groups, d_blocks, d_rows_in, {d_out, d_rows_out, false},
                        d_status, stream);
}

int qfec_decode_batch_recovered(qfec_ctx* c, int k, int m, int bb, long long groups,
                                const unsigned char* d_blocks, const unsigned char* d_rows_in,
                                unsigned char* d_rec, unsigned char* d_rec_rows, int* d_status,
                                void* stream) {
    return decode_batch(c, k, m, bb, groups, d_blocks, d_rows_in, {d_rec, d_rec_rows, true},
                        d_status, stream);
}

// ---- packet protection (pp_null.hip; null_encrypter.cc:23-43, null_decrypter.cc)
int qfec_null_seal_batch(qfec_ctx* c, long long n, const unsigned char* d_ad, long long ad_stride,
                         const int* d_ad_len, int ad_len_all, const unsigned char* d_pt,
                         long long pt_stride, const int* d_pt_len, int pt_len_all,
                         unsigned char* d_out, long long out_stride, int* d_out_len,
                         void* stream) {
    if (!c) return fail(-2, "null context");
    if (n < 0 || ad_stride < 0 || pt_stride < 0 || out_stride < 0) return fail(-2, "bad n / stride");
    if (n && (!d_out || !d_out_len || (!d_ad && (d_ad_len || ad_len_all)) || (!d_pt && (d_pt_len || pt_len_all))))
        return fail(-2, "null buffer");
    const RowsOut out = rows_out_of(d_out, out_stride, d_out_len);
    if (!aligned4(out)) return fail(-2, "out / out_stride not 4-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = set_device(c))) return rc;
    QF_HIP(qfec::launch_null_seal(n, rows_of(d_ad, ad_stride, d_ad_len, ad_len_all),
                                  rows_of(d_pt, pt_stride, d_pt_len, pt_len_all), out,
                                  pick(c, stream)));
    return 0;
}

int qfec_null_open_batch(qfec_ctx* c, long long n, const unsigned char* d_pkt, long long pkt_stride,
                         const int* d_pkt_len, int pkt_len_all, const int* d_ad_len,
                         int ad_len_all, unsigned char* d_out, long long out_stride,
                         int* d_out_len, void* stream) {
    if (!c) return fail(-2, "null context");
    if (n < 0 || pkt_stride < 0 || out_stride < 0) return fail(-2, "bad n / stride");
    if (n && (!d_pkt || !d_out || !d_out_len)) return fail(-2, "null buffer");
    const RowsOut out = rows_out_of(d_out, out_stride, d_out_len);
    if (!aligned4(out)) return fail(-2, "out / out_stride not 4-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = set_device(c))) return rc;
    QF_HIP(qfec::launch_null_open(n, rows_of(d_pkt, pkt_stride, d_pkt_len, pkt_len_all),
                                  rows_of(nullptr, 0, d_ad_len, ad_len_all), out,
                                  pick(c, stream)));
    return 0;
}

int qfec_encode_seal_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                           const unsigned char* d_data, unsigned char* d_parity,
                           const unsigned char* d_hdr, long long hdr_stride, const int* d_hdr_len,
                           int hdr_len_all, unsigned char* d_pkt, long long pkt_stride,
                           int* d_pkt_len, void* stream) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (groups && (!d_data || !d_parity || !d_pkt || !d_pkt_len || (!d_hdr && (d_hdr_len || hdr_len_all))))
        return fail(-2, "null buffer");
    if (hdr_stride < 0 || pkt_stride < 0) return fail(-2, "bad stride");
    const RowsOut pkt = rows_out_of(d_pkt, pkt_stride, d_pkt_len);
    if (!aligned4(pkt)) return fail(-2, "pkt / pkt_stride not 4-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    // SerializeFec (quic_packet_creator.cc:935-957): parity packets from the group's encode,
    // each sealed with its packet header as the associated data; packet (g, i) = g * m + i
    if ((rc = encode_impl(c, k, m, bb, groups, d_data, d_parity, st))) return rc;
    QF_HIP(qfec::launch_null_seal(groups * m, rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all),
                                  Rows{d_parity, bb, nullptr, bb}, pkt, st));
    return 0;
}

// Every packet of each group, data and FEC, in one launch (quic_packet_creator.cc:733-736
// seals each data packet, :948-953 each FEC packet); packet (g, i) = g * (k + m) + i.
extern "C++" int qfec::seal_groups_args(qfec_ctx* c, int k, int m, int bb, long long groups,
                                        std::initializer_list<const void*> required, Rows hdr,
                                        const int* pt_len, int pt_len_all, RowsOut pkt) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if (k + m > 256) return fail(-2, "k + m > 256");
    if (groups && (any_null(required) || (!hdr.p && (hdr.len || hdr.len_all))))
        return fail(-2, "null buffer");
    if (hdr.stride < 0 || pkt.stride < 0) return fail(-2, "bad stride");
    if (!pt_len && (pt_len_all < 0 || pt_len_all > bb)) return fail(-2, "pt_len_all outside 0..block_bytes");
    if (!aligned4(pkt)) return fail(-2, "pkt / pkt_stride not 4-byte aligned");
    return 0;
}

// The two device forms: seal alone, or after the encode.
static int seal_groups(qfec_ctx* c, int k, int m, int bb, long long groups,
                       const unsigned char* d_data, unsigned char* d_parity, bool encode, Rows hdr,
                       const int* d_pt_len, int pt_len_all, RowsOut pkt, void* stream) {
    int rc = seal_groups_args(c, k, m, bb, groups, {d_data, d_parity, pkt.p, pkt.len}, hdr,
                              d_pt_len, pt_len_all, pkt);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    if (encode && (rc = encode_impl(c, k, m, bb, groups, d_data, d_parity, st))) return rc;
    QF_HIP(qfec::launch_null_seal_groups(k, m, bb, groups, d_data, d_parity, hdr,
                                         (const int32_t*)d_pt_len, pt_len_all, pkt, st));
    return 0;
}

int qfec_seal_groups_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                           const unsigned char* d_data, const unsigned char* d_parity,
                           const unsigned char* d_hdr, long long hdr_stride, const int* d_hdr_len,
                           int hdr_len_all, const int* d_pt_len, int pt_len_all,
                           unsigned char* d_pkt, long long pkt_stride, int* d_pkt_len, void* stream) {
    return seal_groups(c, k, m, bb, groups, d_data, (unsigned char*)d_parity, false,
                       rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all), d_pt_len, pt_len_all,
                       rows_out_of(d_pkt, pkt_stride, d_pkt_len), stream);
}

int qfec_encode_seal_groups_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                                  const unsigned char* d_data, unsigned char* d_parity,
                                  const unsigned char* d_hdr, long long hdr_stride,
                                  const int* d_hdr_len, int hdr_len_all, const int* d_pt_len,
                                  int pt_len_all, unsigned char* d_pkt, long long pkt_stride,
                                  int* d_pkt_len, void* stream) {
    return seal_groups(c, k, m, bb, groups, d_data, d_parity, true,
                       rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all), d_pt_len, pt_len_all,
                       rows_out_of(d_pkt, pkt_stride, d_pkt_len), stream);
}

extern "C++" int qfec::open_decode_args(int k, int m, bool packets,
                                        std::initializer_list<const void*> required,
                                        long long pkt_stride, const int* ad_len, int ad_len_all) {
    if (k + m > 255) return fail(-2, "k + m > 255 (row tag 255 marks an unfilled slot)");
    if (packets && any_null(required)) return fail(-2, "null buffer");
    if (packets && pkt_stride <= 0) return fail(-2, "bad pkt_stride");
    if (!ad_len && ad_len_all < 0) return fail(-2, "bad ad_len_all");
    return 0;
}

// Receiver: open every packet of each group (quic_framer.cc:657 decrypts before the group
// sees a packet), place the data plaintexts, fill the holes with opened FEC packets, decode.
int qfec_open_decode_batch(qfec_ctx* c, int k, int m, int bb, long long groups,
                           const unsigned char* d_pkt, long long pkt_stride, const int* d_pkt_len,
                           const int* d_ad_len, int ad_len_all, unsigned char* d_blocks,
                           unsigned char* d_rows, int* d_open_len, unsigned char* d_rec,
                           unsigned char* d_rec_rows, int* d_status, void* stream) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    if ((rc = open_decode_args(k, m, groups != 0,
                               {d_pkt, d_pkt_len, d_blocks, d_rows, d_open_len, d_rec, d_rec_rows},
                               pkt_stride, d_ad_len, ad_len_all)))
        return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return open_decode_impl(c, k, m, bb, groups, rows_of(d_pkt, pkt_stride, d_pkt_len, 0),
                                rows_of(nullptr, 0, d_ad_len, ad_len_all), d_blocks, d_rows,
                                (int32_t*)d_open_len, {d_rec, d_rec_rows, true},
                                (int32_t*)d_status, st);
    });
}

// ---- ragged batches: the groups share (k, m), each has its own block_bytes (gf_ragged.hip).
// Nothing here reads d_bb or the offsets back: every per-group decision is the kernels'.
// Output chunk of the ragged kernels: at most 4.  Their loops around the unit leave no room
// for 8 x 8 accumulators (256 VGPRs and scratch at two waves per SIMD: (10, 10) encode 2.57 ms
// against the (32, 4) encode's 0.86 ms for less data); more chunks re-read the group from L2.
static int ragged_rc(int rc) { return std::min(rc, 4); }

// The decode plan of the run-time-shape decodes (ragged and pointer-table).  The prep's tables
// do not depend on the block size: plan and prep with the smallest valid one, the per-group
// size only enters the apply and the status fix-up.
static DecodePlan ragged_decode_plan(int k, int m) {
    DecodePlan p = decode_plan(k, m, 8);
    if (p.rc > ragged_rc(p.rc)) {   // smaller chunks never need more table bytes per group
        p.rc = ragged_rc(p.rc);
        p.nchunk = (p.rmax + p.rc - 1) / p.rc;
        p.tab_gstride = (long long)p.nchunk * k * std::max(p.rc, 4);
    }
    return p;
}

extern "C++" int qfec::encode_ragged_impl(qfec_ctx* c, int k, int m, long long G, RaggedView v,
                                          const uint8_t* d_data, uint8_t* d_par, int32_t* d_status,
                                          hipStream_t st) {
    if (G == 0) return 0;
    if (k <= 1) {   // cauchy_256.cpp:1508-1516
        QF_HIP(qfec::launch_copy_ragged(d_data, d_par, v, nullptr, nullptr, d_status, m, G, false,
                                        st, c->tune));
        return 0;
    }
    if (m == 1 || k + m > 256) {   // :1519-1534, as encode_impl: P0 only
        QF_HIP(qfec::launch_xor_ragged(d_data, d_par, v, nullptr, d_status, k, G, false,
                                       m == 1 ? 0 : 1, st, c->tune));
        return m == 1 ? 0 : fail(-1, "unsupported (k + m > 256)");
    }
    const int rc = ragged_rc(encode_rc(m, c->tune));
    const uint8_t* tab = nullptr;
    int r = get_enc_table(c, k, m, rc, &tab);
    if (r) return r;
    // the groups with bb % 8 != 0: P0 and status -1; every other group: the GF encode
    QF_HIP(qfec::launch_xor_ragged(d_data, d_par, v, nullptr, d_status, k, G, false, 2, st,
                                   c->tune));
    const qfec::Apply a{d_data, d_par, tab, nullptr, nullptr, nullptr, k, m, 0, G, rc, 0, 0, 0, st,
                        &c->tune};
    QF_HIP(qfec::launch_gf_ragged(a, v, (m + rc - 1) / rc, false));
    return 0;
}

// The caller holds the workspace bracket (with_workspace).
extern "C++" int qfec::decode_ragged_impl(qfec_ctx* c, int k, int m, long long G, RaggedView v,
                                          const uint8_t* d_blocks, const uint8_t* d_rows_in,
                                          uint8_t* d_rec, uint8_t* d_rec_rows, int32_t* d_status,
                                          hipStream_t st) {
    if (G == 0) return 0;
    const DecodePlan p = ragged_decode_plan(k, m);
    if (k <= 1) {   // cauchy_256.cpp:1257-1261
        QF_HIP(qfec::launch_copy_ragged(d_blocks, d_rec, v, d_rows_in, d_rec_rows, d_status, m, G,
                                        true, st, c->tune));
        return 0;
    }
    Workspace& W = ws_for(c, st);
    int r = reserve_workspace(W, p, G, false);
    if (r) return r;
    if (m == 1) {   // :1264-1267
        QF_HIP(qfec::launch_m1_prep(d_rows_in, d_rec_rows, d_status, (uint8_t*)W.dslots.p, k, G,
                                    true, st));
        QF_HIP(qfec::launch_xor_ragged(d_blocks, d_rec, v, (const uint8_t*)W.dslots.p, nullptr, k,
                                       G, true, 0, st, c->tune));
        return 0;
    }
    const uint8_t* cenc = nullptr;
    if ((r = get_cenc(c, k, m, &cenc))) return r;
    qfec::DecodeWork w{(uint8_t*)W.dcoef.p, (uint8_t*)W.dslots.p, (int32_t*)W.dnout.p};
    const qfec::PrepIO io{d_rows_in, nullptr, d_rec_rows, d_status, w};
    QF_HIP(qfec::launch_decode_prep(io, cenc, k, m, 8, p.rc, p.rmax, G, st, c->tune));
    if (k + m > 256) return 0;   // every group is a no-op or status -1
    QF_HIP(qfec::launch_ragged_decode_status(v.bb, d_rows_in, d_rec_rows, d_status, w.nout, k,
                                             p.rmax, G, st));
    const qfec::Apply a{d_blocks, d_rec, w.coef, cenc, nullptr, w.nout, k, m, 0, G, p.rc, p.rmax,
                        p.tab_gstride, 0, st, &c->tune};
    QF_HIP(qfec::launch_gf_ragged(a, v, p.nchunk, true));
    return 0;
}

extern "C++" int qfec::ragged_preface(qfec_ctx* c, int k, int m, long long groups) {
    int rc = check_common(c, k, m, 1, groups < 0 ? 0 : groups);
    if (rc) return rc;
    if (groups < 0) return fail(-2, "groups < 0");
    return 0;
}

// The device forms: the packed arrays a and b are read in place, in 16-byte columns.
static int ragged_check(qfec_ctx* c, int k, int m, long long groups, const void* bb,
                        const void* a, const void* a_off, const void* b, const void* b_off) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    if (any_null({bb, a, a_off, b, b_off})) return fail(-2, "null buffer");
    if ((((uintptr_t)a) | (uintptr_t)b) & 15) return fail(-2, "ragged base pointers must be 16-byte aligned");
    return 0;
}

int qfec_encode_batch_ragged(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                             const unsigned char* d_data, const long long* d_data_off,
                             unsigned char* d_parity, const long long* d_par_off, int* d_status,
                             void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_data, d_data_off, d_parity, d_par_off);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    return encode_ragged_impl(c, k, m, groups, {(const int32_t*)d_bb, d_data_off, d_par_off},
                              d_data, d_parity, (int32_t*)d_status, pick(c, stream));
}

int qfec_decode_batch_ragged_recovered(qfec_ctx* c, int k, int m, long long groups,
                                       const int* d_bb, const unsigned char* d_blocks,
                                       const long long* d_blocks_off,
                                       const unsigned char* d_rows_in, unsigned char* d_rec,
                                       const long long* d_rec_off, unsigned char* d_rec_rows,
                                       int* d_status, void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_blocks, d_blocks_off, d_rec, d_rec_off);
    if (rc) return rc;
    if (!d_rows_in || !d_rec_rows) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return decode_ragged_impl(c, k, m, groups, {(const int32_t*)d_bb, d_blocks_off, d_rec_off},
                                  d_blocks, d_rows_in, d_rec, d_rec_rows, (int32_t*)d_status, st);
    });
}

// ---- mixed-code batches: a (k, m) per group through an index into a code set (gf_mixed.hip,
// decode_prep_mixed_kernel).  Every per-group decision, the rejection of a code index
// included, is the kernels': nothing here reads d_code, d_bb or the offsets back.
int qfec_codeset_create(qfec_ctx* c, int ncodes, const int* k, const int* m, qfec_codeset** out) {
    if (!c || !out) return fail(-2, "null context or output");
    if (!blob_ok()) return fail(-2, "embedded Cauchy tables have the wrong size");
    if (ncodes < 1 || ncodes > qfec::kMixedMaxCodes || !k || !m)
        return fail(-2, "a code set holds 1 to 32 codes");
    for (int i = 0; i < ncodes; ++i)
        if (k[i] < 1 || k[i] > 255 || m[i] < 1) return fail(-2, "bad (k, m) in a code set");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = set_device(c);
    if (rc) return rc;
    auto cs = std::make_unique<qfec_codeset>();
    cs->ctx = c;
    cs->k.assign(k, k + ncodes);
    cs->m.assign(m, m + ncodes);
    qfec::MixedSet& s = cs->s;
    s.ncodes = ncodes;
    // One chunk size per direction for the whole set, the largest a code asks for (2 or 4):
    // one GF launch per call, and a code with m = 2 in a set with larger codes runs with two
    // of four accumulator rows idle.
    s.enc_rc = s.dec_rc = 2;
    const auto decodable = [&](int i) { return qfec::mixed_is_gf(k[i], m[i]) && m[i] <= 256 - k[i]; };
    for (int i = 0; i < ncodes; ++i) {
        s.kmax = std::max(s.kmax, k[i]);
        cs->mmax = std::max(cs->mmax, m[i]);
        s.rmax = std::max(s.rmax, std::min(k[i], m[i]));
        cs->any_gf |= qfec::mixed_is_gf(k[i], m[i]);
        if (!decodable(i)) continue;
        s.enc_rc = std::max(s.enc_rc, ragged_rc(encode_rc(m[i], c->tune)));
        s.dec_rc = std::max(s.dec_rc, ragged_decode_plan(k[i], m[i]).rc);
    }
    std::vector<qfec::MixedCode> rec((size_t)ncodes);
    std::vector<const uint8_t*> tabs((size_t)ncodes, nullptr);
    long long enc_bytes = 0;
    for (int i = 0; i < ncodes; ++i) {
        qfec::MixedCode& d = rec[(size_t)i];
        d = {k[i], m[i], 0, 0, 0, nullptr};
        if (!decodable(i)) continue;
        const int rmax = std::min(k[i], m[i]);
        d.enc_nchunk = (m[i] + s.enc_rc - 1) / s.enc_rc;
        d.dec_nchunk = (rmax + s.dec_rc - 1) / s.dec_rc;
        if ((rc = get_enc_table(c, k[i], m[i], s.enc_rc, &tabs[(size_t)i]))) return rc;
        if ((rc = get_cenc(c, k[i], m[i], &d.cenc))) return rc;
        d.enc_off = enc_bytes;
        enc_bytes += (long long)d.enc_nchunk * k[i] * std::max(s.enc_rc, 4);
        s.enc_nchunk = std::max(s.enc_nchunk, d.enc_nchunk);
        s.dec_nchunk = std::max(s.dec_nchunk, d.dec_nchunk);
        s.coef_gstride = std::max(s.coef_gstride,
                                  (long long)d.dec_nchunk * k[i] * std::max(s.dec_rc, 4));
        s.cenc_bytes += (m[i] * k[i] + 15) & ~15;
        s.solve_rmax = std::max(s.solve_rmax, rmax);
    }
    // the tables get_enc_table built, side by side in one buffer of the set
    QF_HIP(cs->enc.ensure((size_t)enc_bytes));
    for (int i = 0; i < ncodes; ++i)
        if (tabs[(size_t)i])
            QF_HIP(hipMemcpy((uint8_t*)cs->enc.p + rec[(size_t)i].enc_off, tabs[(size_t)i],
                             (size_t)rec[(size_t)i].enc_nchunk * k[i] * std::max(s.enc_rc, 4),
                             hipMemcpyDeviceToDevice));
    s.enc_tabs = (const uint8_t*)cs->enc.p;
    QF_HIP(cs->codes.ensure(rec.size() * sizeof(qfec::MixedCode)));
    QF_HIP(hipMemcpy(cs->codes.p, rec.data(), rec.size() * sizeof(qfec::MixedCode),
                     hipMemcpyHostToDevice));
    s.codes = (const qfec::MixedCode*)cs->codes.p;
    *out = cs.release();
    return 0;
}

void qfec_codeset_destroy(qfec_codeset* cs) {
    if (!cs) return;
    if (cs->ctx) (void)hipSetDevice(cs->ctx->device);
    delete cs;
}

int qfec_codeset_dims(const qfec_codeset* cs, int* kmax, int* mmax, int* rmax) {
    if (!cs) return fail(-2, "null code set");
    if (kmax) *kmax = cs->s.kmax;
    if (mmax) *mmax = cs->mmax;
    if (rmax) *rmax = cs->s.rmax;
    return 0;
}

// the decode workspace of `groups` groups of the set
static int mixed_reserve(Workspace& W, const qfec::MixedSet& s, long long groups) {
    QF_HIP(W.ensure(W.dcoef, (size_t)groups * (size_t)s.coef_gstride));
    QF_HIP(W.ensure(W.dslots, (size_t)groups * (size_t)s.rmax));
    QF_HIP(W.ensure(W.dnout, (size_t)groups * sizeof(int32_t)));
    return 0;
}

// The two work arrays of a mixed wire call (pp_mixed.h: eff, ecode) in the workspace's scratch
// buffer, which no mixed decode uses.
static size_t mixed_wire_bytes(long long groups) { return (size_t)groups * (sizeof(int32_t) + 1); }
static void mixed_wire_work(Workspace& W, long long groups, qfec::MixedWire* w) {
    w->eff = (int32_t*)W.dscratch.p;
    w->ecode = (uint8_t*)W.dscratch.p + (size_t)groups * sizeof(int32_t);
}

int qfec_codeset_reserve(qfec_codeset* cs, long long groups) {
    if (!cs || groups < 0) return fail(-2, "null code set or groups < 0");
    qfec_ctx* c = cs->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = set_device(c);
    if (rc) return rc;
    for (Workspace* W : {&c->ws, &c->ws_graph}) {
        if ((rc = mixed_reserve(*W, cs->s, groups))) return rc;
        QF_HIP(W->ensure(W->dscratch, mixed_wire_bytes(groups)));
    }
    return 0;
}

extern "C++" int qfec::encode_mixed_impl(qfec_ctx* c, const qfec_codeset* cs, long long G,
                                         MixedView v, const uint8_t* d_data, uint8_t* d_par,
                                         int32_t* d_status, hipStream_t st) {
    if (G == 0) return 0;
    QF_HIP(qfec::launch_xor_copy_mixed(cs->s, v, d_data, d_par, nullptr, nullptr, d_status, G,
                                       false, st, c->tune));
    QF_HIP(qfec::launch_gf_mixed(cs->s, v, d_data, d_par, nullptr, nullptr, G, false, st, c->tune));
    return 0;
}

// The caller holds the workspace bracket (with_workspace).
extern "C++" int qfec::decode_mixed_impl(qfec_ctx* c, const qfec_codeset* cs, long long G,
                                         MixedView v, const uint8_t* d_blocks,
                                         const uint8_t* d_rows_in, uint8_t* d_rec,
                                         uint8_t* d_rec_rows, int32_t* d_status, hipStream_t st) {
    if (G == 0) return 0;
    const qfec::MixedSet& s = cs->s;
    QF_HIP(qfec::launch_xor_copy_mixed(s, v, d_blocks, d_rec, d_rows_in, d_rec_rows, d_status, G,
                                       true, st, c->tune));
    if (!cs->any_gf) return 0;
    Workspace& W = ws_for(c, st);
    int r = mixed_reserve(W, s, G);
    if (r) return r;
    qfec::DecodeWork w{(uint8_t*)W.dcoef.p, (uint8_t*)W.dslots.p, (int32_t*)W.dnout.p};
    const qfec::PrepIO io{d_rows_in, nullptr, d_rec_rows, d_status, w};
    QF_HIP(qfec::launch_decode_prep_mixed(s, v, io, G, st, c->tune));
    QF_HIP(qfec::launch_gf_mixed(s, v, d_blocks, d_rec, w.coef, w.nout, G, true, st, c->tune));
    return 0;
}

static int mixed_check(qfec_ctx* c, const qfec_codeset* cs, long long groups, int nchunk,
                       std::initializer_list<const void*> arrays, const void* a, const void* b) {
    if (!c) return fail(-2, "null context");
    if (!cs || cs->ctx != c) return fail(-2, "no code set of this context");
    if (groups < 0) return fail(-2, "groups < 0");
    if (any_null(arrays) || !a || !b) return fail(-2, "null buffer");
    if ((((uintptr_t)a) | (uintptr_t)b) & 15) return fail(-2, "mixed base pointers must be 16-byte aligned");
    if (nchunk > 0 && groups > 0x7fffffffLL / nchunk)
        return fail(-2, "groups x output chunks exceed 2^31 - 1 units");
    return 0;
}

int qfec_encode_batch_mixed(qfec_ctx* c, const qfec_codeset* cs, long long groups,
                            const unsigned char* d_code, const int* d_bb,
                            const unsigned char* d_data, const long long* d_data_off,
                            unsigned char* d_parity, const long long* d_par_off, int* d_status,
                            void* stream) {
    int rc = mixed_check(c, cs, groups, cs ? cs->s.enc_nchunk : 0,
                         {d_code, d_bb, d_data_off, d_par_off}, d_data, d_parity);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    return encode_mixed_impl(c, cs, groups, {d_code, (const int32_t*)d_bb, d_data_off, d_par_off},
                             d_data, d_parity, (int32_t*)d_status, pick(c, stream));
}

int qfec_decode_batch_mixed_recovered(qfec_ctx* c, const qfec_codeset* cs, long long groups,
                                      const unsigned char* d_code, const int* d_bb,
                                      const unsigned char* d_blocks,
                                      const long long* d_blocks_off,
                                      const unsigned char* d_rows_in, unsigned char* d_rec,
                                      const long long* d_rec_off, unsigned char* d_rec_rows,
                                      int* d_status, void* stream) {
    int rc = mixed_check(c, cs, groups, cs ? cs->s.dec_nchunk : 0,
                         {d_code, d_bb, d_blocks_off, d_rec_off, d_rows_in, d_rec_rows}, d_blocks,
                         d_rec);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return decode_mixed_impl(c, cs, groups,
                                 {d_code, (const int32_t*)d_bb, d_blocks_off, d_rec_off}, d_blocks,
                                 d_rows_in, d_rec, d_rec_rows, (int32_t*)d_status, st);
    });
}

// ---- pointer-table batches: the ragged batches with every block at an address of its own
// (gf_ptrs.hip).  The same order of cases and the same tables as encode_ragged_impl /
// decode_ragged_impl; the tables' entries cannot be checked and are not read here.
// The m > 1 kernels count (group, chunk) units in 32 bits.
static int ptrs_units_check(long long G, int nchunk) {
    if (G > 0x7fffffffLL / nchunk) return fail(-2, "groups x output chunks exceed 2^31 - 1 units");
    return 0;
}

static int encode_ptrs_impl(qfec_ctx* c, int k, int m, long long G, qfec::PtrsView v,
                            int32_t* d_status, hipStream_t st) {
    if (G == 0) return 0;
    if (k <= 1) {   // cauchy_256.cpp:1508-1516
        QF_HIP(qfec::launch_copy_ptrs(v, nullptr, nullptr, d_status, k, m, G, false, st, c->tune));
        return 0;
    }
    if (m == 1 || k + m > 256) {   // :1519-1534, as encode_impl: P0 only
        QF_HIP(qfec::launch_xor_ptrs(v, nullptr, d_status, k, m, G, false, m == 1 ? 0 : 1, st,
                                     c->tune));
        return m == 1 ? 0 : fail(-1, "unsupported (k + m > 256)");
    }
    const int rc = ragged_rc(encode_rc(m, c->tune));
    int r = ptrs_units_check(G, (m + rc - 1) / rc);
    if (r) return r;
    const uint8_t* tab = nullptr;
    if ((r = get_enc_table(c, k, m, rc, &tab))) return r;
    // the groups with bb % 8 != 0: P0 and status -1; every other group: the GF encode
    QF_HIP(qfec::launch_xor_ptrs(v, nullptr, d_status, k, m, G, false, 2, st, c->tune));
    const qfec::Apply a{nullptr, nullptr, tab, nullptr, nullptr, nullptr, k, m, 0, G, rc, 0, 0, 0,
                        st, &c->tune};
    QF_HIP(qfec::launch_gf_ptrs(a, v, (m + rc - 1) / rc, false));
    return 0;
}

// The caller holds the workspace bracket (with_workspace).
static int decode_ptrs_impl(qfec_ctx* c, int k, int m, long long G, qfec::PtrsView v,
                            const uint8_t* d_rows_in, uint8_t* d_rec_rows, int32_t* d_status,
                            hipStream_t st) {
    if (G == 0) return 0;
    const DecodePlan p = ragged_decode_plan(k, m);
    if (k <= 1) {   // cauchy_256.cpp:1257-1261
        QF_HIP(qfec::launch_copy_ptrs(v, d_rows_in, d_rec_rows, d_status, k, m, G, true, st,
                                      c->tune));
        return 0;
    }
    int r = m == 1 ? 0 : ptrs_units_check(G, p.nchunk);
    if (r) return r;
    Workspace& W = ws_for(c, st);
    if ((r = reserve_workspace(W, p, G, false))) return r;
    if (m == 1) {   // :1264-1267
        QF_HIP(qfec::launch_m1_prep(d_rows_in, d_rec_rows, d_status, (uint8_t*)W.dslots.p, k, G,
                                    true, st));
        QF_HIP(qfec::launch_xor_ptrs(v, (const uint8_t*)W.dslots.p, nullptr, k, 1, G, true, 0, st,
                                     c->tune));
        return 0;
    }
    const uint8_t* cenc = nullptr;
    if ((r = get_cenc(c, k, m, &cenc))) return r;
    qfec::DecodeWork w{(uint8_t*)W.dcoef.p, (uint8_t*)W.dslots.p, (int32_t*)W.dnout.p};
    const qfec::PrepIO io{d_rows_in, nullptr, d_rec_rows, d_status, w};
    QF_HIP(qfec::launch_decode_prep(io, cenc, k, m, 8, p.rc, p.rmax, G, st, c->tune));
    if (k + m > 256) return 0;   // every group is a no-op or status -1
    QF_HIP(qfec::launch_ptrs_decode_status(v, d_rows_in, d_rec_rows, d_status, w.nout, k, p.rmax,
                                           G, st));
    const qfec::Apply a{nullptr, nullptr, w.coef, cenc, nullptr, w.nout, k, m, 0, G, p.rc, p.rmax,
                        p.tab_gstride, 0, st, &c->tune};
    QF_HIP(qfec::launch_gf_ptrs(a, v, p.nchunk, true));
    return 0;
}

static int ptrs_check(qfec_ctx* c, int k, int m, long long groups, const void* bb, int bb_all,
                      const void* in_ptrs, const void* out_ptrs) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    if (any_null({in_ptrs, out_ptrs})) return fail(-2, "null pointer table");
    if (!bb && bb_all < 1) return fail(-2, "bb_all < 1 without d_bb");
    return 0;
}

int qfec_encode_batch_ptrs(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                           int bb_all, const unsigned char* const* d_data_ptrs,
                           unsigned char* const* d_parity_ptrs, int* d_status, void* stream) {
    int rc = ptrs_check(c, k, m, groups, d_bb, bb_all, d_data_ptrs, d_parity_ptrs);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    return encode_ptrs_impl(c, k, m, groups,
                            {(const unsigned long long*)d_data_ptrs,
                             (const unsigned long long*)d_parity_ptrs, (const int32_t*)d_bb, bb_all},
                            (int32_t*)d_status, pick(c, stream));
}

int qfec_decode_batch_ptrs_recovered(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                                     int bb_all, const unsigned char* const* d_block_ptrs,
                                     const unsigned char* d_rows_in,
                                     unsigned char* const* d_rec_ptrs, unsigned char* d_rec_rows,
                                     int* d_status, void* stream) {
    int rc = ptrs_check(c, k, m, groups, d_bb, bb_all, d_block_ptrs, d_rec_ptrs);
    if (rc) return rc;
    if (!d_rows_in || !d_rec_rows) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return decode_ptrs_impl(c, k, m, groups,
                                {(const unsigned long long*)d_block_ptrs,
                                 (const unsigned long long*)d_rec_ptrs, (const int32_t*)d_bb, bb_all},
                                d_rows_in, d_rec_rows, (int32_t*)d_status, st);
    });
}

// ---- ragged packet protection: the protected paths over the packed layout (pp_null.hip's
// ragged kernels around encode_ragged_impl / decode_ragged_impl).  Packets stay dense by
// packet index; only the blocks are packed.
extern "C++" int qfec::seal_ragged_pkt_args(int k, int m, Rows hdr, RowsOut pkt) {
    if (k + m > 256) return fail(-2, "k + m > 256");
    if (!pkt.p || !pkt.len || (!hdr.p && (hdr.len || hdr.len_all))) return fail(-2, "null buffer");
    if (hdr.stride < 0 || pkt.stride < 0) return fail(-2, "bad stride");
    if (!aligned4(pkt)) return fail(-2, "pkt / pkt_stride not 4-byte aligned");
    return 0;
}

// v: the data (in_off) and the parity (out_off)
static int seal_groups_ragged(qfec_ctx* c, int k, int m, long long groups, RaggedView v,
                              const unsigned char* d_data, unsigned char* d_parity, bool encode,
                              Rows hdr, const int* d_pt_len, RowsOut pkt, int* d_status,
                              void* stream) {
    int rc = ragged_check(c, k, m, groups, v.bb, d_data, v.in_off, d_parity, v.out_off);
    if (rc) return rc;
    if ((rc = seal_ragged_pkt_args(k, m, hdr, pkt))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    if (encode &&
        (rc = encode_ragged_impl(c, k, m, groups, v, d_data, d_parity, (int32_t*)d_status, st)))
        return rc;
    QF_HIP(qfec::launch_null_seal_groups_ragged(k, m, groups, v, d_data, d_parity, encode, hdr,
                                                (const int32_t*)d_pt_len, pkt, st));
    return 0;
}

int qfec_seal_groups_batch_ragged(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                                  const unsigned char* d_data, const long long* d_data_off,
                                  const unsigned char* d_parity, const long long* d_par_off,
                                  const unsigned char* d_hdr, long long hdr_stride,
                                  const int* d_hdr_len, int hdr_len_all, const int* d_pt_len,
                                  unsigned char* d_pkt, long long pkt_stride, int* d_pkt_len,
                                  void* stream) {
    return seal_groups_ragged(c, k, m, groups, {(const int32_t*)d_bb, d_data_off, d_par_off},
                              d_data, (unsigned char*)d_parity, false,
                              rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all), d_pt_len,
                              rows_out_of(d_pkt, pkt_stride, d_pkt_len), nullptr, stream);
}

int qfec_encode_seal_groups_batch_ragged(qfec_ctx* c, int k, int m, long long groups,
                                         const int* d_bb, const unsigned char* d_data,
                                         const long long* d_data_off, unsigned char* d_parity,
                                         const long long* d_par_off, const unsigned char* d_hdr,
                                         long long hdr_stride, const int* d_hdr_len,
                                         int hdr_len_all, const int* d_pt_len,
                                         unsigned char* d_pkt, long long pkt_stride,
                                         int* d_pkt_len, int* d_status, void* stream) {
    return seal_groups_ragged(c, k, m, groups, {(const int32_t*)d_bb, d_data_off, d_par_off},
                              d_data, d_parity, true,
                              rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all), d_pt_len,
                              rows_out_of(d_pkt, pkt_stride, d_pkt_len), d_status, stream);
}

// open_decode_impl over the packed layout: open (framed: a data packet's plaintext goes behind
// its prefix) -> ragged recovered decode -> open_status.  The caller holds the workspace bracket.
extern "C++" int qfec::open_decode_ragged_impl(qfec_ctx* c, int k, int m, long long groups,
                                               RaggedView v, Rows pkt, Rows ad, const PnLen* framed,
                                               uint8_t* d_blocks, uint8_t* d_rows,
                                               int32_t* d_open_len, uint8_t* d_rec,
                                               uint8_t* d_rec_rows, int32_t* d_status,
                                               hipStream_t st) {
    if (framed)
        QF_HIP(qfec::launch_open_groups_framed(k, m, groups, v, pkt, ad, framed->pn_len,
                                               framed->pn_len_all, d_blocks, d_rows, d_open_len,
                                               st));
    else
        QF_HIP(qfec::launch_open_groups_ragged(k, m, groups, v, pkt, ad, d_blocks, d_rows,
                                               d_open_len, st));
    int rc = decode_ragged_impl(c, k, m, groups, v, d_blocks, d_rows, d_rec, d_rec_rows, d_status,
                                st);
    if (rc) return rc;
    QF_HIP(qfec::launch_open_status(k, std::min(k, m), groups, d_rows, d_rec_rows, d_status, st));
    return 0;
}

int qfec_open_decode_batch_ragged(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                                  const unsigned char* d_pkt, long long pkt_stride,
                                  const int* d_pkt_len, const int* d_ad_len, int ad_len_all,
                                  unsigned char* d_blocks, const long long* d_blocks_off,
                                  unsigned char* d_rows, int* d_open_len, unsigned char* d_rec,
                                  const long long* d_rec_off, unsigned char* d_rec_rows,
                                  int* d_status, void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_blocks, d_blocks_off, d_rec, d_rec_off);
    if (rc) return rc;
    if ((rc = open_decode_args(k, m, true, {d_pkt, d_pkt_len, d_rows, d_open_len, d_rec_rows},
                               pkt_stride, d_ad_len, ad_len_all)))
        return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        return open_decode_ragged_impl(c, k, m, groups,
                                       {(const int32_t*)d_bb, d_blocks_off, d_rec_off},
                                       rows_of(d_pkt, pkt_stride, d_pkt_len, 0),
                                       rows_of(nullptr, 0, d_ad_len, ad_len_all), nullptr, d_blocks,
                                       d_rows, (int32_t*)d_open_len, d_rec, d_rec_rows,
                                       (int32_t*)d_status, st);
    });
}

// ---- framed groups: QuicFecGroup's wire format around the ragged protected paths (pp_null.hip's
// framed kernels).  Payload rows and revived payloads stay dense by packet; blocks are packed.
// the payload rows a framed sender reads, the revived rows a framed receiver writes
static int framed_rows_args(const unsigned char* d_row, long long stride, const int* d_len,
                            const char* bad_stride) {
    if (!d_row || !d_len) return fail(-2, "null buffer");
    if (stride < 0) return fail(-2, bad_stride);
    return 0;
}

// The per-arrival arguments of the three arrival-order calls and the revived rows they write.
// required: the call's own arrays that may not be null; n_neg, n_big: the call's messages for
// n < 0 and for n, or its slots (slots_big), above INT32_MAX: both index int32 tables.
static int arrivals_args(int k, int m, std::initializer_list<const void*> required,
                         const Arrivals& ar, RowsOut rev, bool slots_big, const char* n_neg,
                         const char* n_big) {
    int rc = open_decode_args(k, m, true, required, ar.pkt.stride, ar.ad.len, ar.ad.len_all);
    if (rc || (rc = framed_rows_args(rev.p, rev.stride, rev.len, "bad rev_stride"))) return rc;
    if (ar.n < 0) return fail(-2, n_neg);
    if (ar.n > INT32_MAX || slots_big) return fail(-2, n_big);
    // nothing of the per-arrival arrays is read when nothing arrived
    if (ar.n > 0 && any_null({ar.pkt.p, ar.pkt.len, ar.arr_group, ar.arr_index}))
        return fail(-2, "null buffer");
    return 0;
}

int qfec_frame_blocks_batch_ragged(qfec_ctx* c, int k, long long groups, const int* d_bb,
                                   const unsigned char* d_pay, long long pay_stride,
                                   const int* d_pay_len, const unsigned char* d_pn_len,
                                   int pn_len_all, unsigned char* d_data,
                                   const long long* d_data_off, int* d_status, void* stream) {
    int rc = ragged_preface(c, k, 1, groups);
    if (rc) return rc;
    if (any_null({d_bb, d_data, d_data_off})) return fail(-2, "null buffer");
    if ((uintptr_t)d_data & 15) return fail(-2, "ragged base pointers must be 16-byte aligned");
    if ((rc = framed_rows_args(d_pay, pay_stride, d_pay_len, "bad pay_stride"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    QF_HIP(qfec::launch_frame_blocks_ragged(
        k, groups, {(const int32_t*)d_bb, d_data_off, nullptr},
        rows_of(d_pay, pay_stride, d_pay_len, 0), d_pn_len, pn_len_all, d_data, nullptr,
        (int32_t*)d_status, pick(c, stream)));
    return 0;
}

int qfec_extract_revived_batch_ragged(qfec_ctx* c, int k, int m, long long groups, const int* d_bb,
                                      const unsigned char* d_rec, const long long* d_rec_off,
                                      const unsigned char* d_rec_rows, const int* d_status,
                                      unsigned char* d_rev, long long rev_stride, int* d_rev_len,
                                      unsigned char* d_rev_pn_len, void* stream) {
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    if (any_null({d_bb, d_rec, d_rec_off, d_rec_rows})) return fail(-2, "null buffer");
    if ((rc = framed_rows_args(d_rev, rev_stride, d_rev_len, "bad rev_stride"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    QF_HIP(qfec::launch_extract_revived(k, m, groups, {(const int32_t*)d_bb, nullptr, d_rec_off},
                                        d_rec, d_rec_rows, (const int32_t*)d_status,
                                        rows_out_of(d_rev, rev_stride, d_rev_len), d_rev_pn_len,
                                        pick(c, stream)));
    return 0;
}

// frame -> ragged encode -> framed seal.  The encode runs with the frame's sizes (0 for a group
// the frame rejected, which every encode kernel skips), kept in the decode workspace's count
// array: the call holds the workspace bracket like a decode.
int qfec_frame_encode_seal_groups_batch_ragged(
    qfec_ctx* c, int k, int m, long long groups, const int* d_bb, unsigned char* d_data,
    const long long* d_data_off, unsigned char* d_parity, const long long* d_par_off,
    const unsigned char* d_hdr, long long hdr_stride, const int* d_hdr_len, int hdr_len_all,
    const unsigned char* d_pay, long long pay_stride, const int* d_pay_len,
    const unsigned char* d_pn_len, int pn_len_all, unsigned char* d_pkt, long long pkt_stride,
    int* d_pkt_len, int* d_status, void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_data, d_data_off, d_parity, d_par_off);
    if (rc) return rc;
    const Rows hdr = rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all);
    const RowsOut pkt = rows_out_of(d_pkt, pkt_stride, d_pkt_len);
    if ((rc = seal_ragged_pkt_args(k, m, hdr, pkt))) return rc;
    if ((rc = framed_rows_args(d_pay, pay_stride, d_pay_len, "bad pay_stride"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    const Rows pay = rows_of(d_pay, pay_stride, d_pay_len, 0);
    return with_workspace(c, st, [&] {
        Workspace& W = ws_for(c, st);
        QF_HIP(W.ensure(W.dnout, (size_t)groups * sizeof(int32_t)));
        int32_t* eff = (int32_t*)W.dnout.p;
        const RaggedView v{(const int32_t*)d_bb, d_data_off, d_par_off};
        QF_HIP(qfec::launch_frame_blocks_ragged(k, groups, v, pay, d_pn_len, pn_len_all, d_data,
                                                eff, nullptr, st));
        const int r = encode_ragged_impl(c, k, m, groups, {eff, d_data_off, d_par_off}, d_data,
                                         d_parity, (int32_t*)d_status, st);
        if (r) return r;
        QF_HIP(qfec::launch_null_seal_framed(k, m, groups, v, pay, d_parity, hdr, pkt,
                                             (int32_t*)d_status, st));
        return 0;
    });
}

// framed open -> ragged recovered decode -> open_status -> extract
int qfec_open_decode_extract_batch_ragged(
    qfec_ctx* c, int k, int m, long long groups, const int* d_bb, const unsigned char* d_pkt,
    long long pkt_stride, const int* d_pkt_len, const int* d_ad_len, int ad_len_all,
    const unsigned char* d_pn_len, int pn_len_all, unsigned char* d_blocks,
    const long long* d_blocks_off, unsigned char* d_rows, int* d_open_len, unsigned char* d_rec,
    const long long* d_rec_off, unsigned char* d_rec_rows, int* d_status, unsigned char* d_rev,
    long long rev_stride, int* d_rev_len, unsigned char* d_rev_pn_len, void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_blocks, d_blocks_off, d_rec, d_rec_off);
    if (rc) return rc;
    if ((rc = open_decode_args(k, m, true, {d_pkt, d_pkt_len, d_rows, d_open_len, d_rec_rows},
                               pkt_stride, d_ad_len, ad_len_all)))
        return rc;
    if ((rc = framed_rows_args(d_rev, rev_stride, d_rev_len, "bad rev_stride"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    if (groups == 0) return 0;
    const hipStream_t st = pick(c, stream);
    const RaggedView v{(const int32_t*)d_bb, d_blocks_off, d_rec_off};
    const PnLen framed{d_pn_len, pn_len_all};
    return with_workspace(c, st, [&] {
        const int r = open_decode_ragged_impl(c, k, m, groups, v,
                                              rows_of(d_pkt, pkt_stride, d_pkt_len, 0),
                                              rows_of(nullptr, 0, d_ad_len, ad_len_all), &framed,
                                              d_blocks, d_rows, (int32_t*)d_open_len, d_rec,
                                              d_rec_rows, (int32_t*)d_status, st);
        if (r) return r;
        QF_HIP(qfec::launch_extract_revived(k, m, groups, v, d_rec, d_rec_rows,
                                            (const int32_t*)d_status,
                                            rows_out_of(d_rev, rev_stride, d_rev_len),
                                            d_rev_pn_len, st));
        return 0;
    });
}

// arrivals open (init -> open -> assemble -> state) -> ragged recovered decode -> open_status ->
// extract: the framed receiver over packets in arrival order.  d_arr_at is the binding table, so
// the call needs no workspace beyond the decode's.
int qfec_open_decode_extract_arrivals_ragged(
    qfec_ctx* c, int k, int m, long long groups, const int* d_bb, long long n,
    const unsigned char* d_pkt, long long pkt_stride, const int* d_pkt_len, const int* d_ad_len,
    int ad_len_all, const unsigned char* d_pn_len, int pn_len_all, const int* d_arr_group,
    const unsigned char* d_arr_index, int* d_arr_state, int* d_arr_at, unsigned char* d_blocks,
    const long long* d_blocks_off, unsigned char* d_rows, int* d_open_len, unsigned char* d_rec,
    const long long* d_rec_off, unsigned char* d_rec_rows, int* d_status, unsigned char* d_rev,
    long long rev_stride, int* d_rev_len, unsigned char* d_rev_pn_len, void* stream) {
    int rc = ragged_check(c, k, m, groups, d_bb, d_blocks, d_blocks_off, d_rec, d_rec_off);
    if (rc) return rc;
    const Arrivals ar{n, {d_pkt, pkt_stride, d_pkt_len, 0}, {nullptr, 0, d_ad_len, ad_len_all},
                      d_pn_len, pn_len_all, d_arr_group, d_arr_index, d_arr_state};
    const RowsOut rev = rows_out_of(d_rev, rev_stride, d_rev_len);
    if ((rc = arrivals_args(k, m, {d_rows, d_open_len, d_rec_rows, d_arr_at}, ar, rev,
                            groups > INT32_MAX / (k + m), "n < 0",
                            "n or groups * (k + m) above INT32_MAX")))
        return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    const RaggedView v{(const int32_t*)d_bb, d_blocks_off, d_rec_off};
    return with_workspace(c, st, [&] {
        QF_HIP(qfec::launch_open_arrivals_framed(k, m, groups, v, ar, (int32_t*)d_arr_at, d_blocks,
                                                 d_rows, (int32_t*)d_open_len,
                                                 c->tune.arr_optimistic != 0, st));
        const int r = decode_ragged_impl(c, k, m, groups, v, d_blocks, d_rows, d_rec, d_rec_rows,
                                         (int32_t*)d_status, st);
        if (r) return r;
        QF_HIP(qfec::launch_open_status(k, std::min(k, m), groups, d_rows, d_rec_rows,
                                        (int32_t*)d_status, st));
        QF_HIP(qfec::launch_extract_revived(k, m, groups, v, d_rec, d_rec_rows,
                                            (const int32_t*)d_status, rev, d_rev_pn_len, st));
        return 0;
    });
}

// ---- receiver window: the arrivals call with its state kept between calls (pp_null.hip's rxwin
// kernels).  bind (init -> pre -> open -> assemble -> state) -> pointer-table decode over the
// window's own tables (every block is a hold row) -> finish -> extract.  Nothing is read back.
struct qfec_rxwin {
    qfec_ctx* ctx = nullptr;
    qfec::RxWin w{};
    qfec::DevBuf buf;   // the window's one allocation (RxwinLayout)
};

int qfec_rxwin_create(qfec_ctx* c, int k, int m, long long groups, int hold_stride,
                      qfec_rxwin** out) {
    if (!out) return fail(-2, "null out");
    *out = nullptr;
    int rc = ragged_preface(c, k, m, groups);
    if (rc) return rc;
    qfec::RxwinLayout L;
    const char* why = "";
    if (qfec::rxwin_layout(k, m, groups, hold_stride, &L, &why)) return fail(-2, why);
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    auto win = std::make_unique<qfec_rxwin>();   // frees its allocation on every early return
    win->ctx = c;
    if (hipError_t e = win->buf.ensure((size_t)std::max(L.total, 256LL))) {
        (void)hipGetLastError();   // the launchers return the last error: leave none behind
        return hip_fail(e, "hipMalloc of the window");
    }
    uint8_t* b = (uint8_t*)win->buf.p;
    win->w = qfec::RxWin{k, m, groups, hold_stride, b + L.hold, (int32_t*)(b + L.slot_state),
                         (int32_t*)(b + L.held), (int32_t*)(b + L.delivered),
                         (int32_t*)(b + L.arr_at), (int32_t*)(b + L.pre_at), b + L.rows,
                         (unsigned long long*)(b + L.blk_ptrs),
                         (unsigned long long*)(b + L.rec_ptrs), (int32_t*)(b + L.eff),
                         (int32_t*)(b + L.verdict)};
    // every slot empty (kSlotEmpty = -1: all-ones bytes), no packet held, nothing delivered
    QF_HIP(hipMemset(b + L.slot_state, 0xff, (size_t)(L.held - L.slot_state)));
    QF_HIP(hipMemset(b + L.held, 0, (size_t)(L.arr_at - L.held)));
    // what a push's decode needs, in both workspaces, so that no push allocates
    const DecodePlan p = ragged_decode_plan(k, m);
    for (Workspace* W : {&c->ws, &c->ws_graph})
        if ((rc = reserve_workspace(*W, p, groups, false))) return rc;
    if (p.cenc) {
        const uint8_t* t;
        if ((rc = get_cenc(c, k, m, &t))) return rc;
    }
    QF_HIP(hipDeviceSynchronize());
    *out = win.release();
    return 0;
}

void qfec_rxwin_destroy(qfec_rxwin* win) {
    if (!win) return;
    {
        std::lock_guard<std::mutex> lk(win->ctx->mu);
        (void)hipSetDevice(win->ctx->device);
        (void)hipDeviceSynchronize();   // a push or a graph replay may still use the rows
    }
    delete win;
}

int qfec_rxwin_release(qfec_rxwin* win, long long count, const int* d_groups, void* stream) {
    if (!win) return fail(-2, "null window");
    if (count < 0) return fail(-2, "count < 0");
    if (d_groups && count > INT32_MAX / (win->w.k + win->w.m))
        return fail(-2, "count * (k + m) above INT32_MAX");
    qfec_ctx* c = win->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = set_device(c);
    if (rc) return rc;
    QF_HIP(qfec::launch_rxwin_release(win->w, count, (const int32_t*)d_groups, pick(c, stream)));
    return 0;
}

int qfec_rxwin_push(qfec_rxwin* win, const int* d_bb, long long n, const unsigned char* d_pkt,
                    long long pkt_stride, const int* d_pkt_len, const int* d_ad_len,
                    int ad_len_all, const unsigned char* d_pn_len, int pn_len_all,
                    const int* d_arr_group, const unsigned char* d_arr_index, int* d_arr_state,
                    unsigned char* d_rec, const long long* d_rec_off, unsigned char* d_rec_rows,
                    int* d_status, unsigned char* d_rev, long long rev_stride, int* d_rev_len,
                    unsigned char* d_rev_pn_len, void* stream) {
    if (!win) return fail(-2, "null window");
    qfec_ctx* c = win->ctx;
    const qfec::RxWin& w = win->w;
    int rc;
    if (any_null({d_bb, d_rec, d_rec_off, d_rec_rows})) return fail(-2, "null buffer");
    if ((uintptr_t)d_rec & 15) return fail(-2, "ragged base pointers must be 16-byte aligned");
    const Arrivals ar{n, {d_pkt, pkt_stride, d_pkt_len, 0}, {nullptr, 0, d_ad_len, ad_len_all},
                      d_pn_len, pn_len_all, d_arr_group, d_arr_index, d_arr_state};
    const RowsOut rev = rows_out_of(d_rev, rev_stride, d_rev_len);
    if ((rc = arrivals_args(w.k, w.m, {}, ar, rev, false, "n < 0", "n above INT32_MAX"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        QF_HIP(qfec::launch_rxwin_bind(w, (const int32_t*)d_bb, ar, d_rec, d_rec_off,
                                       c->tune.arr_optimistic != 0, st));
        const int r = decode_ptrs_impl(c, w.k, w.m, w.groups, {w.blk_ptrs, w.rec_ptrs, w.eff, 0},
                                       w.rows, d_rec_rows, (int32_t*)d_status, st);
        if (r) return r;
        QF_HIP(qfec::launch_rxwin_finish(w, d_rec_rows, (int32_t*)d_status, st));
        QF_HIP(qfec::launch_extract_revived(w.k, w.m, w.groups, {w.eff, nullptr, d_rec_off}, d_rec,
                                            d_rec_rows, (const int32_t*)d_status, rev,
                                            d_rev_pn_len, st));
        return 0;
    });
}

// ---- mixed-code wire path: the two calls above with a (k, m) per group (pp_mixed.h).  Nothing
// here reads d_code, d_bb, the offsets or the prefix tables back: the plan kernel decides every
// group, and npkt / npay size the grids.
// The limits both directions add to mixed_check's.  The k + m limit of the set stands here; the
// shared packet-argument helpers below (seal_ragged_pkt_args, open_decode_args) are therefore
// called with the smallest code, (1, 1), which passes their own k + m check, for the rest of
// what they check: the packet arrays, strides and lengths.
static int mixed_wire_check(const qfec_codeset* cs, long long npkt, long long npay) {
    for (size_t i = 0; i < cs->k.size(); ++i)
        if (cs->k[i] + cs->m[i] > 255)
            return fail(-2, "a code of the set has k + m > 255 (the wire's group-offset byte)");
    if (npkt < 0 || npkt > INT32_MAX || npay < 0 || npay > INT32_MAX)
        return fail(-2, "npkt or npay outside [0, INT32_MAX]");
    return 0;
}

// plan -> frame -> mixed encode with the plan's codes and sizes -> framed seal
int qfec_frame_encode_seal_groups_batch_mixed(
    qfec_ctx* c, const qfec_codeset* cs, long long groups, const unsigned char* d_code,
    const int* d_bb, const int* d_pkt_first, const int* d_pay_first, long long npkt,
    long long npay, unsigned char* d_data, const long long* d_data_off, unsigned char* d_parity,
    const long long* d_par_off, const unsigned char* d_hdr, long long hdr_stride,
    const int* d_hdr_len, int hdr_len_all, const unsigned char* d_pay, long long pay_stride,
    const int* d_pay_len, const unsigned char* d_pn_len, int pn_len_all, unsigned char* d_pkt,
    long long pkt_stride, int* d_pkt_len, int* d_status, void* stream) {
    int rc = mixed_check(c, cs, groups, cs ? cs->s.enc_nchunk : 0,
                         {d_code, d_bb, d_data_off, d_par_off, d_pkt_first, d_pay_first}, d_data,
                         d_parity);
    if (rc) return rc;
    if ((rc = mixed_wire_check(cs, npkt, npay))) return rc;
    const Rows hdr = rows_of(d_hdr, hdr_stride, d_hdr_len, hdr_len_all);
    const RowsOut pkt = rows_out_of(d_pkt, pkt_stride, d_pkt_len);
    if ((rc = seal_ragged_pkt_args(1, 1, hdr, pkt))) return rc;
    if ((rc = framed_rows_args(d_pay, pay_stride, d_pay_len, "bad pay_stride"))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    const Rows pay = rows_of(d_pay, pay_stride, d_pay_len, 0);
    return with_workspace(c, st, [&] {
        Workspace& W = ws_for(c, st);
        QF_HIP(W.ensure(W.dscratch, mixed_wire_bytes(groups)));
        qfec::MixedWire w{d_code, (const int32_t*)d_bb, (const int32_t*)d_pkt_first,
                          (const int32_t*)d_pay_first, npkt, npay, nullptr, nullptr};
        mixed_wire_work(W, groups, &w);
        QF_HIP(qfec::launch_mixed_wire_plan(cs->s, groups, w, &pay, st));
        QF_HIP(qfec::launch_frame_blocks_mixed(cs->s, groups, w, pay, d_pn_len, pn_len_all, d_data,
                                               d_data_off, st));
        const int r = encode_mixed_impl(c, cs, groups, {w.ecode, w.eff, d_data_off, d_par_off},
                                        d_data, d_parity, (int32_t*)d_status, st);
        if (r) return r;
        QF_HIP(qfec::launch_null_seal_mixed(cs->s, groups, w, pay, d_parity, d_par_off, hdr, pkt,
                                            (int32_t*)d_status, st));
        return 0;
    });
}

// plan -> arrivals open (init -> pre -> open -> assemble -> state) -> mixed recovered decode with
// the plan's codes and sizes -> open_status -> extract
int qfec_open_decode_extract_arrivals_mixed(
    qfec_ctx* c, const qfec_codeset* cs, long long groups, const unsigned char* d_code,
    const int* d_bb, const int* d_pkt_first, long long npkt, long long n,
    const unsigned char* d_pkt, long long pkt_stride, const int* d_pkt_len, const int* d_ad_len,
    int ad_len_all, const unsigned char* d_pn_len, int pn_len_all, const int* d_arr_group,
    const unsigned char* d_arr_index, int* d_arr_state, int* d_arr_at, unsigned char* d_blocks,
    const long long* d_blocks_off, unsigned char* d_rows, int* d_open_len, unsigned char* d_rec,
    const long long* d_rec_off, unsigned char* d_rec_rows, int* d_status, unsigned char* d_rev,
    long long rev_stride, int* d_rev_len, unsigned char* d_rev_pn_len, void* stream) {
    int rc = mixed_check(c, cs, groups, cs ? cs->s.dec_nchunk : 0,
                         {d_code, d_bb, d_blocks_off, d_rec_off, d_pkt_first}, d_blocks, d_rec);
    if (rc) return rc;
    if ((rc = mixed_wire_check(cs, npkt, 0))) return rc;
    const Arrivals ar{n, {d_pkt, pkt_stride, d_pkt_len, 0}, {nullptr, 0, d_ad_len, ad_len_all},
                      d_pn_len, pn_len_all, d_arr_group, d_arr_index, d_arr_state};
    const RowsOut rev = rows_out_of(d_rev, rev_stride, d_rev_len);
    const char* n_msg = "n outside [0, INT32_MAX]";
    if ((rc = arrivals_args(1, 1, {d_rows, d_open_len, d_rec_rows, d_arr_at}, ar, rev, false, n_msg,
                            n_msg)))
        return rc;
    if (groups > 0x7fffffffLL / cs->s.rmax) return fail(-2, "groups * rmax above INT32_MAX");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const hipStream_t st = pick(c, stream);
    return with_workspace(c, st, [&] {
        Workspace& W = ws_for(c, st);
        QF_HIP(W.ensure(W.dscratch, mixed_wire_bytes(groups)));
        qfec::MixedWire w{d_code, (const int32_t*)d_bb, (const int32_t*)d_pkt_first, nullptr, npkt,
                          0, nullptr, nullptr};
        mixed_wire_work(W, groups, &w);
        QF_HIP(qfec::launch_mixed_wire_plan(cs->s, groups, w, nullptr, st));
        QF_HIP(qfec::launch_open_arrivals_mixed(cs->s, groups, w, d_blocks_off, ar,
                                                (int32_t*)d_arr_at, d_blocks, d_rows,
                                                (int32_t*)d_open_len,
                                                c->tune.arr_optimistic != 0, st));
        const int r = decode_mixed_impl(c, cs, groups, {w.ecode, w.eff, d_blocks_off, d_rec_off},
                                        d_blocks, d_rows, d_rec, d_rec_rows, (int32_t*)d_status,
                                        st);
        if (r) return r;
        QF_HIP(qfec::launch_open_status_mixed(cs->s, groups, w, d_rows, d_rec_rows,
                                              (int32_t*)d_status, st));
        QF_HIP(qfec::launch_extract_revived_mixed(cs->s, groups, w, d_rec, d_rec_off, d_rec_rows,
                                                  (const int32_t*)d_status, rev, d_rev_pn_len,
                                                  st));
        return 0;
    });
}

int qfec_synth_fill(void* d_dst, unsigned long long bytes, unsigned long long seed,
                    unsigned long long byte_offset, void* stream) {
    qfec::TimingMute mute;
    QF_HIP(qfec::launch_synth_fill((uint8_t*)d_dst, bytes, seed, byte_offset,
                                   (hipStream_t)stream));
    return 0;
}

int qfec_synth_gather(const unsigned char* d_data, const unsigned char* d_parity,
                      const short* d_src, unsigned char* d_blocks, int k, int m, int bb,
                      long long groups, void* stream) {
    qfec::TimingMute mute;
    QF_HIP(qfec::launch_synth_gather(d_data, d_parity, (const int16_t*)d_src, d_blocks, k, m, bb,
                                     groups, (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------- single-group drop-ins
int _cauchy_256_init(int expected_version) {
    if (expected_version != CAUCHY_256_VERSION) return -1;   // cauchy_256.cpp:389-398
    qfec_ctx* c;
    return default_ctx(&c);
}

int cauchy_256_encode(int k, int m, const unsigned char* data_ptrs[], void* recovery_blocks,
                      int block_bytes) {
    qfec_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    if ((rc = check_common(c, k, m, block_bytes, 1))) return rc;
    if (!data_ptrs || !recovery_blocks) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t bb = (size_t)block_bytes;
    const size_t in_bytes = (size_t)k * bb, out_bytes = (size_t)m * bb;
    QF_HIP(c->h_stage.ensure(in_bytes + out_bytes));
    QF_HIP(c->d_stage.ensure(in_bytes + out_bytes));
    uint8_t* hs = (uint8_t*)c->h_stage.p;
    for (int x = 0; x < k; ++x) memcpy(hs + x * bb, data_ptrs[x], bb);
    uint8_t* dd = (uint8_t*)c->d_stage.p;
    QF_HIP(hipMemcpyAsync(dd, hs, in_bytes, hipMemcpyHostToDevice, c->stream));
    // outputs the reference leaves untouched (the -1 paths) keep the caller's bytes
    QF_HIP(hipMemcpyAsync(dd + in_bytes, recovery_blocks, out_bytes, hipMemcpyHostToDevice,
                          c->stream));
    if (m > 1 && k > 1 && k + m <= 256 && bb % 8 == 0)   // :1554 zeroes rows 1..m-1
        QF_HIP(hipMemsetAsync(dd + in_bytes, 0, out_bytes, c->stream));
    rc = encode_impl(c, k, m, block_bytes, 1, dd, dd + in_bytes, c->stream);
    if (rc < -1) return rc;
    QF_HIP(hipMemcpyAsync(hs + in_bytes, dd + in_bytes, out_bytes, hipMemcpyDeviceToHost,
                          c->stream));
    QF_HIP(hipStreamSynchronize(c->stream));
    memcpy(recovery_blocks, hs + in_bytes, out_bytes);
    return rc;
}

int cauchy_256_decode(int k, int m, Block* blocks, int block_bytes) {
    qfec_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    if ((rc = check_common(c, k, m, block_bytes, 1))) return rc;
    if (!blocks) return fail(-2, "null buffer");
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    const size_t bb = (size_t)block_bytes;
    const size_t data_bytes = (size_t)k * bb;
    QF_HIP(c->h_stage.ensure(data_bytes + 256 + 16));
    QF_HIP(c->d_stage.ensure(data_bytes + 256 + 16));
    uint8_t* hs = (uint8_t*)c->h_stage.p;
    uint8_t* hr = hs + data_bytes;
    int32_t* hst = (int32_t*)(((uintptr_t)(hr + 256) + 3) & ~(uintptr_t)3);
    for (int x = 0; x < k; ++x) {
        memcpy(hs + x * bb, blocks[x].data, bb);
        hr[x] = blocks[x].row;
    }
    uint8_t* dd = (uint8_t*)c->d_stage.p;
    uint8_t* dr = dd + data_bytes;
    int32_t* dst = (int32_t*)(((uintptr_t)(dr + 256) + 3) & ~(uintptr_t)3);
    QF_HIP(hipMemcpyAsync(dd, hs, data_bytes + 256, hipMemcpyHostToDevice, c->stream));
    rc = with_workspace(c, c->stream, [&] {
        return decode_impl(c, k, m, block_bytes, 1, dd, dr, {dd, dr, false}, dst, c->stream);
    });
    if (rc) return rc;
    QF_HIP(hipMemcpyAsync(hs, dd, data_bytes + k, hipMemcpyDeviceToHost, c->stream));
    QF_HIP(hipMemcpyAsync(hst, dst, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    QF_HIP(hipStreamSynchronize(c->stream));
    for (int x = 0; x < k; ++x) {
        if (blocks[x].row >= k || hr[x] != blocks[x].row)   // only recovery slots change
            memcpy(blocks[x].data, hs + x * bb, bb);
        blocks[x].row = hr[x];
    }
    return *hst;
}

int qfec_reserve(qfec_ctx* c, int k, int m, int bb, long long groups) {
    int rc = check_common(c, k, m, bb, groups);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = set_device(c))) return rc;
    // both workspaces: the eager one and the one calls captured into a graph use
    const DecodePlan p = decode_plan(k, m, bb);
    for (Workspace* W : {&c->ws, &c->ws_graph}) {
        if ((rc = reserve_workspace(*W, p, groups, true))) return rc;
        // the framed sender's per-group sizes (any k, m)
        QF_HIP(W->ensure(W->dnout, (size_t)groups * sizeof(int32_t)));
    }
    if (m > 1 && k > 1 && k + m <= 256) {
        const uint8_t* t;
        if ((rc = get_enc_table(c, k, m, stream_encode_rc(k, m, bb, true, c->tune), &t))) return rc;
        // the ragged encode's table (chunks of at most 4 outputs)
        if ((rc = get_enc_table(c, k, m, ragged_rc(encode_rc(m, c->tune)), &t))) return rc;
    }
    if (p.cenc) {
        const uint8_t* t;
        if ((rc = get_cenc(c, k, m, &t))) return rc;
    }
    return 0;
}

}  // extern "C"
