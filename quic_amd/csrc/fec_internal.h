// fec_internal.h — what fec_api.cpp (contexts, dispatch, the device-pointer ABI) and
// fec_host.cpp (the host-pointer ABI) share.  Library-internal: hidden visibility, not in
// include/.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/quic_fec.h"
#include "fec_kernels.h"
#include "gf_mixed.h"

namespace qfec {

int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define QF_HIP(expr)                                   \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return qfec::hip_fail(_e, #expr); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= n) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) n = bytes;
        return e;
    }
};

struct HostBuf {
    void* p = nullptr;
    size_t n = 0;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= n) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
        hipError_t e = hipHostMalloc(&p, bytes, 0);
        if (e == hipSuccess) n = bytes;
        return e;
    }
};

// One decode workspace: the prep's per-group tables and the in-place scratch.
struct Workspace {
    DevBuf dcoef, dslots, dnout, dscratch;
    // graph workspace: a buffer outgrown by a later capture is kept (not freed) until the
    // context is destroyed, since the graphs captured before still name it
    bool keep = false;
    std::vector<std::unique_ptr<DevBuf>> retired;
    hipError_t ensure(DevBuf& b, size_t bytes) {
        if (bytes <= b.n) return hipSuccess;
        if (keep && b.p) {
            auto old = std::make_unique<DevBuf>();
            std::swap(old->p, b.p);
            std::swap(old->n, b.n);
            retired.push_back(std::move(old));
        }
        return b.ensure(bytes);
    }
};

}  // namespace qfec

struct qfec_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    qfec::Tune tune;
    // Decode workspaces.  Eager calls share `ws`; they may enqueue on any stream: every
    // eager use records ws_ev after its kernels, and a use on another stream waits for it, so
    // eager uses are ordered across streams (ws_begin / ws_end).  Calls captured into a graph
    // use `ws_graph` instead, so a replay (on whatever stream it is launched) never shares
    // tables with an eager call; graphs captured on one context share ws_graph, so their
    // replays must be ordered with each other (include/quic_fec.h).
    hipEvent_t ws_ev = nullptr;      // on ws_helper, after the last eager use
    hipEvent_t ws_tmp = nullptr;     // on the last eager use's stream
    hipStream_t ws_helper = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    // encode coefficient tables keyed by (k, m, rc): [nchunk][k][rcp]; decode cenc by (k, m)
    std::map<std::tuple<int, int, int>, std::unique_ptr<qfec::DevBuf>> enc_tab;
    std::map<std::pair<int, int>, std::unique_ptr<qfec::DevBuf>> cenc_tab;
    qfec::Workspace ws, ws_graph;
    qfec::HostBuf h_stage;
    qfec::DevBuf d_stage;
    // host-pointer batches: copy-in / copy-out streams around `stream` (compute), NB
    // rotating device staging buffers so H2D, kernels and D2H of successive chunks overlap
    static constexpr int NB = 3;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[NB] = {}, ev_done[NB] = {}, ev_out[NB] = {};
    qfec::DevBuf pbuf[NB];
    std::mutex mu;   // one caller at a time per context (the reference is single-threaded)
};

// A code set (qfec_codeset_create): the codes of a mixed-code batch.
struct qfec_codeset {
    qfec_ctx* ctx = nullptr;
    int mmax = 0;
    bool any_gf = false;      // a code with k > 1 and m > 1: the decode runs the prep
    std::vector<int> k, m;    // the codes, for the host forms' block counts
    qfec::MixedSet s{};
    qfec::DevBuf codes;       // MixedCode [ncodes]; the matrices it names are the context's
    qfec::DevBuf enc;         // the codes' encode tables, copies of the context's
};

namespace qfec {

int set_device(qfec_ctx* c);
int ws_begin(qfec_ctx* c, hipStream_t st);
int ws_end(qfec_ctx* c, hipStream_t st);

// The bracket of one C entry point whose kernels on `st` use the decode workspace: applied
// once per call, around everything the call enqueues.  ws_end runs whenever ws_begin
// succeeded, also when the body fails after it has enqueued work.
template <class F>
int with_workspace(qfec_ctx* c, hipStream_t st, F&& body) {
    int r = ws_begin(c, st);
    if (r) return r;
    r = body();
    const int r2 = ws_end(c, st);
    return r ? r : r2;
}

// ---- argument checks every form of a call shares (the device forms add their pointer
// alignment rules)
int check_common(qfec_ctx* c, int k, int m, int bb, long long groups);
// the preface of every ragged form: no block_bytes, and groups < 0 has its own message
int ragged_preface(qfec_ctx* c, int k, int m, long long groups);
inline bool any_null(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return true;
    return false;
}
// The C entry points build their packet arrays (Rows / RowsOut, fec_kernels.h) once, from
// their `const int*` / `unsigned char*` arguments; nothing below them casts.
inline Rows rows_of(const unsigned char* p, long long stride, const int* len, int len_all) {
    return {p, stride, (const int32_t*)len, len_all};
}
inline RowsOut rows_out_of(unsigned char* p, long long stride, int* len) {
    return {p, stride, (int32_t*)len};
}
// what the seal and open kernels ask of the rows they write (each call site has its message)
inline bool aligned4(RowsOut r) { return ((((uintptr_t)r.p) | (uintptr_t)r.stride) & 3) == 0; }
// qfec_[encode_]seal_groups_batch[_host]; `required`: the arrays this form cannot do without
int seal_groups_args(qfec_ctx* c, int k, int m, int bb, long long groups,
                     std::initializer_list<const void*> required, Rows hdr, const int* pt_len,
                     int pt_len_all, RowsOut pkt);
// the packet side of the ragged seals, after the form's own checks of the block arrays
int seal_ragged_pkt_args(int k, int m, Rows hdr, RowsOut pkt);
// The receiver's arguments, every form of open-decode, after the form's preface; `required`: the
// arrays this form cannot do without.  `packets` false: k + m and ad_len_all alone, for a call
// with no group whose form then takes null arrays and any stride.
int open_decode_args(int k, int m, bool packets, std::initializer_list<const void*> required,
                     long long pkt_stride, const int* ad_len, int ad_len_all);

// ---- the dispatch: which kernels a call runs on `st` (fec_api.cpp)
// Where a decode writes.  Slot layout (qfec_decode_batch): recovered blocks go back into their
// slots of out [G][k][bb] (which may be the blocks themselves) and rows [G][k] gets every
// slot's row tag.  Compact layout (qfec_decode_batch_recovered): recovered block j of group g
// goes to out + (g * rmax + j) * bb and its data row to rows[g * rmax + j] (ascending, 255
// past the erasure count); blocks and row tags are left as they are.  This is what the
// receiver consumes (getRevivedPackets, quic_fec_group.cc:280-293, only extracts the missing
// packets), and the writes are dense.
struct DecodeOut {
    uint8_t* out;
    uint8_t* rows;
    bool compact;
};

// The encode's -1 (cauchy_256.cpp:1519-1534): only P0, the XOR of the data, is written.
inline bool encode_p0_only(int k, int m, int bb) {
    return m > 1 && k > 1 && (k + m > 256 || bb % 8 != 0);
}
int encode_impl(qfec_ctx* c, int k, int m, int bb, long long G, const uint8_t* d_data,
                uint8_t* d_par, hipStream_t st);
// The decodes: the caller holds the workspace bracket (with_workspace).
int decode_impl(qfec_ctx* c, int k, int m, int bb, long long G, const uint8_t* d_blocks,
                const uint8_t* d_rows_in, DecodeOut o, int32_t* d_status, hipStream_t st);
// pkt: the wire packets; ad: their associated-data lengths; rec: the compact DecodeOut
int open_decode_impl(qfec_ctx* c, int k, int m, int bb, long long groups, Rows pkt, Rows ad,
                     uint8_t* d_blocks, uint8_t* d_rows, int32_t* d_open_len, DecodeOut rec,
                     int32_t* d_status, hipStream_t st);
int encode_ragged_impl(qfec_ctx* c, int k, int m, long long G, RaggedView v, const uint8_t* d_data,
                       uint8_t* d_par, int32_t* d_status, hipStream_t st);
int decode_ragged_impl(qfec_ctx* c, int k, int m, long long G, RaggedView v,
                       const uint8_t* d_blocks, const uint8_t* d_rows_in, uint8_t* d_rec,
                       uint8_t* d_rec_rows, int32_t* d_status, hipStream_t st);
// Mixed-code batches (gf_mixed.h): what the device and the host forms enqueue on `st`.  The
// decode's caller holds the workspace bracket.
int encode_mixed_impl(qfec_ctx* c, const qfec_codeset* cs, long long G, MixedView v,
                      const uint8_t* d_data, uint8_t* d_par, int32_t* d_status, hipStream_t st);
int decode_mixed_impl(qfec_ctx* c, const qfec_codeset* cs, long long G, MixedView v,
                      const uint8_t* d_blocks, const uint8_t* d_rows_in, uint8_t* d_rec,
                      uint8_t* d_rec_rows, int32_t* d_status, hipStream_t st);
// The framing of a framed open: each packet's pn_len, or one value for all (pn_len null).
struct PnLen {
    const uint8_t* pn_len;
    int pn_len_all;
};
// v: the blocks (in_off) and the recovered blocks (out_off); framed: null for the unframed open
int open_decode_ragged_impl(qfec_ctx* c, int k, int m, long long groups, RaggedView v, Rows pkt,
                            Rows ad, const PnLen* framed, uint8_t* d_blocks, uint8_t* d_rows,
                            int32_t* d_open_len, uint8_t* d_rec, uint8_t* d_rec_rows,
                            int32_t* d_status, hipStream_t st);

}  // namespace qfec
