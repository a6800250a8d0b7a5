// fec_kernels.h — launch interface of the gfx950 FEC kernels (internal to libquic_fec.so).
//
// Layouts (all device memory, row-major, bb = block_bytes, s = bb / 8):
//   data     [G][k][bb]   the k data blocks of each packet group
//   parity   [G][m][bb]   encode output (parity block y of group g at (g*m + y)*bb)
//   blocks   [G][k][bb]   decode input: the first k packets received, any order
//   rows     [G][k]       row tag of each received block (data 0..k-1, parity k..k+m-1)
// The bit-sliced code treats every block as 8 sub-rows of s bytes; see DESIGN.md.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <utility>

namespace qfec {

// Per-context launch configuration.  The defaults are the measured best shapes
// (DESIGN.md); qfec_ctx_set_option() changes them for one context only, so no
// environment variable can change what the product launches.
struct Tune {
    int cus = 256;            // compute units of the context's device (filled at create)
    int xor_slots = 2;        // m = 1 LDS ring: group slots per wave (2..4)
    int xor_waves = 3;        //                 waves per workgroup (1..4)
    int dma = 1;              // m = 1: LDS-DMA ring kernel (0: flat register kernel)
    int stream = 1;           // m > 1, small blocks: gf_stream (0: gf_apply)
    int stream_ring = 8;      // gf_stream: 1 KiB ring slots per wave (4..36), + 2 mirrored
    int stream_grid = 0;      // gf_stream: grid cap in workgroups (0: CUs x per-CU fit)
    int stream_static = 1;    // gf_ring: compile-time ring schedule (the codes of compiled_codes.h)
    int ring_wide = 1;        // gf_ring: LDS-staged 8-byte parity stores (the rows' ring_wide)
    int ring_split = 1;       // gf_ring: two units of m / 2 parity rows per group (ring_split rows)
    int psyn_wide = 1;        // gf_psyn wide recovered-block stores: 1 the psyn_wide rows, 2 all
    int const_enc = 1;        // encode kernels specialised for fixed (k, m) where compiled
    int pd = 2;               // gf_apply: register pipeline depth (1..3)
    int flat = 1;             // gf_apply: lane-flat encode
    int enc_rc = 8;           // gf_apply: encode outputs per wave (2, 4, 8)
    int prep_lane = 1;        // decode prep with 4 lanes per group when it applies
    int bsyn = 1;             // compiled syndrome decode gf_bsyn (the Syn::bsyn row of
                              //   compiled_codes.h; 0: the run-time gf_stream decode)
    int bsyn_depth = 3;       // gf_bsyn: blocks in flight per wave (3, 5, 7; 3: 5 waves/SIMD)
    int psyn = 1;             // compiled syndrome decode gf_psyn (the Syn::psyn rows of
                              //   compiled_codes.h; 0: the run-time gf_stream decode)
    int dcol = 1;             // (128, 16) x 9008 B: gf_dcol (one wave per column tile, all 16
                              //   rows; 0: gf_apply)
    int dcol_grid = 0;        // gf_dcol: grid cap in workgroups (0: CUs x per-CU fit)
    int dcol_depth = 6;       // gf_dcol: blocks in flight per wave (6 or 8; two waves per SIMD)
    // Oversubscribed grids: about this many groups (units) per wave, more workgroups than the
    // device holds at once, so the hardware hands the last ones to whichever CU frees first
    // (0: the resident persistent grid, every wave walking groups g0, g0 + W, ...; -1: the
    // measured choice)
    int ring_wg = -1;         // gf_ring encodes (-1: the row's ring_wg in compiled_codes.h)
    int bsyn_wg = -1;         // gf_bsyn decode (-1: 2)
    int psyn_wg = 0;          // gf_psyn decodes
    int stream_wg = -1;       // gf_stream (run-time coefficients: the (250, 5) decode, other shapes;
                              //   -1: 1 for groups of at least 64 KiB, else 0)
    int dcol_wg = 4;          // gf_dcol encode / decode (units = column tiles; D 1909 -> 2000 GiB/s
                              //   over three alternating pairs on a power-limited box)
    int xor_wg = 0;           // xor_dma (m = 1)
    int arr_optimistic = 1;   // arrivals receiver: first-candidate data packets are placed by the
                              //   open pass (0: the assemble reads every accepted packet again)
    int host_chunk_mb = 64;   // host-pointer batches: chunk size
    int host_min_groups = 512;  // host-pointer batches: at least this many groups per chunk
                                //   (capped at 2 GiB of staging per buffer)
};

// Records the name of a kernel a call launched (qfec_last_kernels(), per thread).
void note_kernel(const char* name);
// Records the grid (workgroups) a persistent kernel was launched with (qfec_last_grids(),
// per thread, "name=grid" entries).
void note_grid(const char* name, unsigned grid);

// Workgroups of `kern` one CU holds at once (the runtime's occupancy answer), cached per
// (kernel, threads, LDS bytes); thread-safe.
int resident_blocks(const void* kern, int threads, size_t lds);

// Grid of a persistent kernel whose waves each walk units u0, u0 + W, ... (W = waves in the
// grid): enough workgroups of `waves` waves for one unit per wave, capped at `resident` (the
// workgroups the device holds at once), or, oversubscribed (wg > 0), at about wg units per wave;
// grid_cap > 0 (stream_grid / dcol_grid: tests) overrides both caps.  0 = invalid: a wave's
// units times per_unit (what its 32-bit counters count per unit) must stay below 2^31.
inline unsigned persistent_grid(long long units, int waves, long long resident, int wg,
                                int grid_cap, long long per_unit = 1) {
    const long long want = (units + waves - 1) / waves;
    long long cap = resident;
    if (wg > 0) cap = (units + (long long)waves * wg - 1) / ((long long)waves * wg);
    if (grid_cap > 0) cap = grid_cap;
    const unsigned grid = (unsigned)std::min<long long>(want, cap);
    const long long total = (long long)grid * waves;
    if (grid == 0 || (units + total - 1) / total * per_unit >= (1LL << 31)) return 0;
    return grid;
}

// Workgroups one CU holds of a kernel that needs `lds` bytes each (160 KiB per CU), at most
// `cap` (what the registers or the wave slots allow), at least 1.
inline int lds_blocks_per_cu(size_t lds, int cap = 1 << 30) {
    return std::max(1, std::min((int)((160 * 1024) / lds), cap));
}

// The ragged kernels' grid (gf_ragged.hip).  A different rule from persistent_grid on purpose:
// oversubscribed at about two units per wave once the device is full, but never fewer
// workgroups than the device holds (`resident`) while there are units for them, where
// persistent_grid's wg cap replaces the resident one.
inline unsigned ragged_grid(long long units, long long resident) {
    const long long per_wg = 4;
    const long long all = (units + per_wg - 1) / per_wg;
    const long long two = (units + 2 * per_wg - 1) / (2 * per_wg);
    const long long nb = std::max<long long>(1, std::min(all, std::max(resident, two)));
    return (unsigned)std::min<long long>(nb, 0x7fffffffLL);
}

// Kernel timing hook (qfec_set_timing_events, per thread).  While a stop event is set, each
// engine call records `start` at the start of its first kernel and `stop` at the end of
// every kernel (the last record wins), through hipExtLaunchKernel: the events bracket the
// kernels themselves, not the launch gaps around them, so they agree with rocprofv3.
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
    bool first = true;   // the call's first kernel has not been launched yet
    bool muted = false;  // a helper call (synth) is launching: leave the events alone
};
LaunchTiming& launch_timing();

// Helper entry points (qfec_synth_*) launch under this guard, so a timing bracket armed
// for the engine's next call neither starts nor stops at their kernels.
struct TimingMute {
    TimingMute() { launch_timing().muted = true; }
    ~TimingMute() { launch_timing().muted = false; }
};

// Run-time value -> template argument: calls f(std::integral_constant<int, V>{}) for the V among
// Vs that equals v.  False: v is none of them, f was not called.
template <int... Vs, class F>
inline bool dispatch_value(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// The same for a flag: f(std::true_type{}) or f(std::false_type{}).
template <class F>
inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// Every kernel of the library is launched through this.
template <typename F, typename... Args>
inline void qlaunch(F kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t st,
                    Args... args) {
    LaunchTiming& t = launch_timing();
    hipEvent_t a = nullptr, b = t.muted ? nullptr : t.stop;
    if (b && t.first) {
        a = t.start;
        t.first = false;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, a, b, 0u, args...);
}

// Decode work tables written by the prep kernel and read by the apply kernel.
struct DecodeWork {
    uint8_t* coef;     // [G][nchunk][k][RCP]  bit-sliced GF(256) coefficients
    uint8_t* slots;    // [G][RMAX]            output slot (0..k-1) of recovered block j
    int32_t* nout;     // [G]                  number of recovered blocks in this group
};

// What every decode prep reads and writes (decode_prep.hip).  w.coef is the table its apply
// kernel reads: the coefficients, or the syn:: / bsyn:: / psyn:: table.
struct PrepIO {
    const uint8_t* rows_in;   // [G][k]
    uint8_t* rows_out;        // [G][k], may alias rows_in; null: recovered-blocks layout, then
    uint8_t* rec_rows;        // [G][rmax] gets the data row of recovered block j (ascending),
                              //   255 past the group's erasure count; null in the slot layout
    int32_t* status;          // [G] or null
    DecodeWork w;
};

// What every GF(256) apply launcher takes.  An encode leaves cenc, slots and nout null and
// rmax, tab_gstride 0; its tab is the shared table.  A decode's tab is the prep's per-group
// table (coefficients, or the syn:: / bsyn:: / psyn:: table) at tab + g * tab_gstride; slots
// null: recovered blocks written densely.  The launchers hand the kernels the members as
// scalar arguments; the struct itself is never a kernel argument.
struct Apply {
    const uint8_t* in;
    uint8_t* out;
    const uint8_t* tab;
    const uint8_t* cenc;
    const uint8_t* slots;
    const int32_t* nout;
    int k, m, bb;
    long long groups;
    int rc, rmax;
    long long tab_gstride, out_gstride;
    hipStream_t st;
    const Tune* t;
};

// A packet array: row i at p + i * stride, len[i] bytes of it (len null: len_all for every
// row).  Where only the lengths of a call's rows matter (the associated data of an open is the
// head of its packet), p and stride stay null.
struct Rows {
    const uint8_t* p;
    long long stride;
    const int32_t* len;
    int len_all;
};
// Its writable twin: the lengths are an output too.  p and stride must be 4-byte aligned.
struct RowsOut {
    uint8_t* p;
    long long stride;
    int32_t* len;
};
// The packets of one ring read in arrival order: arrival a is pkt row a
// (pkt.len never null; ad: lengths only), tagged (arr_group[a], arr_index[a]) = (the group's
// index, packet number - fec_group).  pn_len: u8 per arrival, or null: pn_all for all.
// arr_state [n] (may be null) is written: what became of each arrival.  n == 0: no array is read.
struct Arrivals {
    long long n;
    Rows pkt, ad;
    const uint8_t* pn_len;
    int pn_all;
    const int32_t* arr_group;
    const uint8_t* arr_index;
    int32_t* arr_state;
};

// Syndrome table (decode prep in syndrome mode, read by gf_dcol's syndrome decode), one per
// group at coef + g * coef_gstride, k <= 128 and at most 16 parity rows:
namespace syn {
constexpr int kPerm = 0;     // u8[k]  stream order of the slots: the present data rows
                             //        ascending (one slot each), then the extras: recovery
                             //        blocks and repeated data rows, in slot order
constexpr int kMask = 128;   // u32[4] bit x: data row x is in the ascending part
constexpr int kNeed = 144;   // u32    bit y: parity row y was received (a syndrome row)
constexpr int kISlot = 148;  // u8[16] syndrome index i of received parity row y
constexpr int kERow = 164;   // u8[k]  row tag of extra e
constexpr int kSinv = 292;   // u8[16][16] Sinv[j][i]: recovered j = sum_i Sinv[j][i] T_i
constexpr int kRowSlot = 548;  // u8[128] slot holding data row x (255: erased / unchanged group)
constexpr int kYmap = 676;   // u8[16] parity row y_i of syndrome i (recovery blocks, array order)
constexpr int kNExt = 692;   // u32    extras to stream after the rows (0: unchanged group)
constexpr int kBytes = 696;
}  // namespace syn

// Compact syndrome table of the small-block decode (decode_prep_bsyn, read by gf_bsyn), one
// per group at tab + g * kBytes, k <= 64 and at most 4 recovered blocks:
namespace bsyn {
constexpr int kPerm = 0;     // u8[64] stream order of the slots: present data rows ascending
                             //        (first copy of each), then the extras in slot order
constexpr int kMask = 64;    // u32[2] bit x: data row x is in the ascending part
constexpr int kY = 72;       // u8[4]  parity row y_i of recovery block i
constexpr int kSinv = 76;    // u8[4][4] Sinv[j][i]: recovered j = sum_i Sinv[j][i] T_{y_i}
constexpr int kERow = 92;    // u8[64] row tag of extra e (255: no-op, unchanged group)
constexpr int kBytes = 156;
}  // namespace bsyn

// Preset syndrome table (decode_prep_psyn, read by gf_psyn), one per group at
// tab + g * kBytes, k <= 64, m <= 32, at most 16 recovered blocks:
namespace psyn {
constexpr int kPerm = 0;     // u8[64] stream order of the slots: present data rows ascending
                             //        (first copy of each), then the extras in slot order
constexpr int kMask = 64;    // u32[2] bit x: data row x is in the ascending part
constexpr int kYs = 72;      // u8[16] received parity rows, ascending (syndrome slot s)
constexpr int kERow = 88;    // u8[64] row tag of extra e (255: no-op, unchanged group)
constexpr int kCoef = 152;   // u8[16][16] g[p][i]: pivot p's coefficient for slot i
constexpr int kNeed = 408;   // u32    bit y: parity row y enters the solve (received)
constexpr int kBytes = 412;
}  // namespace psyn

// parity[g*out_gstride ..+bb) = XOR of the k blocks of group g (m == 1 encode, and the
// P0 the reference writes before rejecting invalid m > 1 parameters).
hipError_t launch_xor_encode(const uint8_t* data, uint8_t* parity, int k, int bb,
                             long long groups, long long out_gstride, hipStream_t st,
                             const Tune& t);

// m == 1 decode: XOR the k-1 other blocks into the block tagged row >= k.  eidx is a
// [G] byte workspace (erased slot per group).  compact: the recovered block of group g
// goes to out + g * bb and its data row to rows_out[g] (255 = nothing erased).
hipError_t launch_xor_decode(const uint8_t* blocks, uint8_t* out, const uint8_t* rows_in,
                             uint8_t* rows_out, int32_t* status, uint8_t* eidx, int k, int bb,
                             long long groups, hipStream_t st, const Tune& t,
                             bool compact = false);

// The m == 1 decode bookkeeping alone (the ragged decode runs its own XOR after it): eidx [G]
// gets the erased slot (255: nothing erased); compact: rows_out [G] the recovered data row.
hipError_t launch_m1_prep(const uint8_t* rows_in, uint8_t* rows_out, int32_t* status,
                          uint8_t* eidx, int k, long long groups, bool compact, hipStream_t st);

// k <= 1 encode: copy data[0] into each of the m outputs (cauchy_256.cpp:1508-1516).
hipError_t launch_replicate(const uint8_t* data, uint8_t* parity, int m, int bb,
                            long long groups, hipStream_t st);

// k <= 1 decode in the recovered-blocks layout (rec [G][rmax][bb], rec_rows [G][rmax]).
hipError_t launch_rec_k1(const uint8_t* blocks, const uint8_t* rows_in, uint8_t* rec,
                        uint8_t* rec_rows, int32_t* status, int bb, int rmax, long long groups,
                        hipStream_t st);

// k <= 1 decode: row := 0 (cauchy_256.cpp:1257-1261).
hipError_t launch_rows_k1(const uint8_t* rows_in, uint8_t* rows_out, int32_t* status,
                          long long groups, hipStream_t st);

// Bit-sliced GF(256) apply.  Encode: coef is the shared [nchunk][k][RCP] table built
// from the Cauchy matrix (row 0 = ones), outputs are parity rows chunk*RC + j.
hipError_t launch_gf_encode(const Apply& a);
// Its chunk (outputs per wave) for m parity rows: the power of two that holds them, capped
// at enc_rc.
inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int encode_rc(int m, const Tune& t) { return std::min(pow2_at_least(m), t.enc_rc); }

// Decode prep: per group, sort blocks, invert the erasure submatrix in GF(256) and
// emit the r x k recovery coefficients (syndrome: the syn:: table instead).  cenc is the
// [m][k] encode matrix (row 0 = ones).  All preps live in decode_prep.hip.
hipError_t launch_decode_prep(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                              int rc, int rmax, long long groups, hipStream_t st,
                              const Tune& t, bool syndrome = false);

// Decode apply: recovered block j of group g = sum_pos coef[g][..][pos][j] (x) blocks[g][pos],
// written to out[g][slots[g][j]], or densely (slots null: out is [G][rmax][bb]).
hipError_t launch_gf_decode(const Apply& a);

// In-place decode when rmax > rc: the dense apply into scratch [G][rmax][bb], then this
// scatter to the slots.
hipError_t launch_scatter_recovered(const uint8_t* scratch, uint8_t* out, DecodeWork w, int k,
                                   int bb, int rmax, long long groups, hipStream_t st);

// m = 1 LDS-ring XOR kernel (xor_dma.hip).  Requires 16-byte aligned `in`, 8-byte aligned
// `out`/stride and bb % 8 == 0; decode with rows_in != null also does the row bookkeeping.
bool xor_dma_ok(const void* in, const void* out, int k, int bb, long long ogs, const Tune& t);
// compact: recovered-blocks layout (out [G][bb], rows_out [G] = recovered data row).
hipError_t launch_xor_dma(const uint8_t* in, uint8_t* out, const uint8_t* eidx,
                          const uint8_t* rows_in, uint8_t* rows_out, int32_t* status, int k,
                          int bb, long long groups, long long out_gstride, bool decode,
                          hipStream_t st, const Tune& t, bool compact = false);

// Per-wave LDS-ring streaming kernels (gf_stream.hip), bb a multiple of 8 up to 2048, `in`
// 16-byte aligned.  Encode (decode false): the m parity rows of each group; the codes of
// compiled_codes.h run compiled (gf_ring_kernel, or gf_stream_kernel<encode,compiled>) and read
// no table, every other code reads tab, the shared table built for rc = stream_encode_rc().
// Decode: up to rmax recovered blocks per group in chunks of rc (2, 4, 8) from the prep's
// per-group tables, through slots (slot layout) or densely (slots null).
bool gf_stream_supported(int k, int bb, int rc, const Tune& t);
// Encode table rows: gf_apply's chunk (<= 8), or 16 where gf_stream takes 9..16 outputs in
// one unit (m <= 8: one unit of m outputs; more than 16: chunks of 8; compiled codes read no
// table).  aligned: the data pointer is 16-byte aligned (otherwise gf_apply encodes).
int stream_encode_rc(int k, int m, int bb, bool aligned, const Tune& t);
hipError_t launch_gf_stream(const Apply& a, bool decode);


// One wave per column tile computing all 16 rows (gf_dcol.hip): encode of the compiled
// (128, 16) x 9008-byte code, and its syndrome decode from the syn:: table.
bool gf_dcol_supported(int k, int m, int bb, const Tune& t);
hipError_t launch_gf_dcol_encode(const Apply& a);
hipError_t launch_gf_dcol_syndrome(const Apply& a);

// Syndrome decode of the Syn::bsyn code of compiled_codes.h, (32, 4) x 1352 bytes: prep (bsyn:: table, one lane per
// group; reads the row tags as dwords) and the block pass + r x r solve (gf_bsyn.hip).
bool gf_bsyn_supported(int k, int m, int bb, int rmax, const Tune& t);
hipError_t launch_decode_prep_bsyn(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                                   int rmax, long long groups, hipStream_t st);
hipError_t launch_gf_bsyn(const Apply& a);

// Syndrome decode of the Syn::psyn codes of compiled_codes.h (QuicR presets at 1352-byte
// blocks): prep (psyn:: table, 16 lanes per group) and the block pass + in-place Gauss-Jordan
// replay (gf_psyn.hip).
bool gf_psyn_supported(int k, int m, int bb, int rmax, const Tune& t);
hipError_t launch_decode_prep_psyn(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                                   int rmax, long long groups, hipStream_t st);
hipError_t launch_gf_psyn(const Apply& a);

// Ragged batches (gf_ragged.hip): the groups share (k, m), each has its own block size.
// Group g's input blocks are [k][bb[g]] at in + in_off[g] and its outputs [n][bb[g]] at
// out + out_off[g] (byte offsets, multiples of 16; all three arrays in device memory).
// The groups a ragged encode rejects (status -1, XOR parity only, cauchy_256.cpp:1519-1534;
// k + m > 256 is a call-level matter): asked by the encode (xor_ragged_kernel, which writes
// the status) and by the seal that follows it (pp_null.hip, which then seals none of the
// group's packets), so the two cannot disagree.
__host__ __device__ inline bool ragged_encode_rejects(int k, int m, int bb) {
    return m > 1 && k > 1 && (bb & 7) != 0;
}

// The groups the framed sender rejects (status -3, every pkt_len -1, none of its blocks, parity
// or packets written): a payload length that has no 14-bit prefix, exceeds its row or does not
// fit behind the prefix in a block, or a block too small to encode.  len: the group's k payload
// lengths.  Asked by the frame kernel, by the framed seal and for the status (pp_null.hip), so
// the three cannot disagree.
__host__ __device__ inline bool framed_group_rejects(const int32_t* len, int k,
                                                     long long pay_stride, int bb) {
    // no early exit: the lanes of a wave ask for different groups, and a loop every lane runs
    // to its end keeps the control flow uniform (a form that returned at the first bad length
    // let a bb = 0 group through in the framed seal)
    bool bad = bb < 8;
    for (int i = 0; i < k; ++i) {
        const int l = len[i];
        bad |= (l < 0) | (l > 0x3fff) | ((pay_stride != 0) & (l > pay_stride)) | (l > bb - 2);
    }
    return bad;
}

struct RaggedView {
    const int32_t* bb;
    const long long* in_off;
    const long long* out_off;
};
// m > 1, the groups with bb % 8 == 0 (the others are skipped).  Encode: coef is the shared
// [nchunk][k][max(rc, 4)] table; decode: the prep's per-group tables, outputs o < nout[g] in
// the recovered-blocks layout.  rc 2 or 4; a.bb, a.cenc, a.slots and a.out_gstride are not read.
hipError_t launch_gf_ragged(const Apply& a, RaggedView v, int nchunk, bool decode);
// XOR of each group's k blocks.  Encode modes: 0 every group, status 0; 1 every group, status
// -1; 2 only the groups with bb % 8 != 0 (status -1, the rest 0).  Decode: the recovered block
// of the groups with eidx[g] != 255 (m1_prep_kernel's erased slot).
hipError_t launch_xor_ragged(const uint8_t* in, uint8_t* out, RaggedView v, const uint8_t* eidx,
                             int32_t* status, int k, long long groups, bool decode, int mode,
                             hipStream_t st, const Tune& t);
// k <= 1: encode copies the group's block into its m outputs; decode (rmax = 1) copies a block
// not tagged row 0 into rec and writes rec_rows [G].
hipError_t launch_copy_ragged(const uint8_t* in, uint8_t* out, RaggedView v,
                              const uint8_t* rows_in, uint8_t* rec_rows, int32_t* status, int m,
                              long long groups, bool decode, hipStream_t st, const Tune& t);
// After launch_decode_prep with a block size of 8: status -1 and nothing recovered for the
// groups whose own bb % 8 != 0 and that hold a recovery block.
hipError_t launch_ragged_decode_status(const int32_t* bb, const uint8_t* rows_in,
                                       uint8_t* rec_rows, int32_t* status, int32_t* nout, int k,
                                       int rmax, long long groups, hipStream_t st);

// Synthetic workload helpers (bench / tests): splitmix64 stream and receive-set gather.
hipError_t launch_synth_fill(uint8_t* dst, unsigned long long bytes, unsigned long long seed,
                             unsigned long long byte_offset, hipStream_t st);
hipError_t launch_synth_gather(const uint8_t* data, const uint8_t* parity, const int16_t* src,
                               uint8_t* blocks, int k, int m, int bb, long long groups,
                               hipStream_t st);

}  // namespace qfec
