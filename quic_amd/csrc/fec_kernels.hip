// fec_kernels.hip — gfx950 kernels for QuicR packet-group FEC (encode + erasure recover).
//
// The reference codec (libcat cauchy_256, net/quic/core/libcat/cauchy_256.cpp) is a
// bit-sliced Cauchy Reed-Solomon code over GF(2^8): each block of bb bytes is 8 sub-rows
// of s = bb/8 bytes and a GF(256) coefficient c acts on a block through its transposed
// 8x8 bit expansion
//      out[r][j] ^= XOR_{t : bit t of (c * alpha^r)} in[t][j]          (j = byte column)
// i.e. pure byte XORs between sub-rows at the SAME column j.  No multiplications touch
// the data, so the work is HBM-bound byte streaming (no MFMA: nothing here is a
// floating-point contraction).
//
// Kernel set (all wave64, 256-thread workgroups = 4 independent waves):
//   xor_encode / xor_decode   m = 1 XOR parity (cauchy_256.cpp:1519-1528, :486-540)
//   gf_apply<RC>              bit-sliced GF(256) matrix x blocks, RC outputs per wave;
//                             used for encode (Cauchy rows, :1502-1601) and for decode
//                             (per-group recovery rows from the prep kernel)
// The decode preps (per-group GF(256) inverse of the erasure submatrix, replacing
// sort_blocks/eliminate_original/bitmatrix GE, :543-1252) are in decode_prep.hip.
//
// The coefficient of a (output, input) pair is wave-uniform, so it lives in SGPRs and the
// 8x8 expansion is a scalar branch over its two nibbles; the data lane only ever runs
// v_xor / v_bitop3 (3-input XOR).  See DESIGN.md "Kernels" for the derivation of the
// W/Z recurrences used below.
#include "fec_kernels.h"
#include "gf256.h"
#include "gf_bitslice.h"
#include "gf_colword.h"

namespace qfec {

typedef uint64_t u64a __attribute__((aligned(8)));

// ------------------------------------------------------------------ m = 1 XOR paths
// Flat mapping: every lane owns one VS-byte unit (g, q) of one group and issues all k of
// its loads back to back, so a wave keeps k * 64 * VS bytes in flight in a single phase.
// The last unit of a block is shifted back to end at bb (loads stay inside the block) and
// stores only the bytes no other unit owns, so no byte is written twice and an in-place
// decode never reads a byte another lane has already rewritten and then uses it.
//   encode: out = parity + g*out_gstride
//   decode: out = blocks' slot eidx[g] (the slot tagged row >= k); the XOR runs over all
//           k slots — the erased slot's own parity included (cauchy_256.cpp:505-531) —
//           so the loads never wait on eidx, only the store does.
typedef uint32_t u32x4a8 __attribute__((ext_vector_type(4), aligned(8)));

template <int VS> struct Unit;
// Loads and stores are non-temporal: every byte is touched exactly once, and on gfx950
// nt streaming measured +17-23% over the default policy with cold caches
// (tools/microbench).
template <> struct Unit<16> {
    typedef u32x4a8 T;
    static __device__ __forceinline__ T ld(const uint8_t* p) {
        return __builtin_nontemporal_load((const T*)p);
    }
    static __device__ __forceinline__ void st(uint8_t* p, T v) {
        __builtin_nontemporal_store(v, (T*)p);
    }
};
template <> struct Unit<4> {
    typedef uint32_t T;
    static __device__ __forceinline__ T ld(const uint8_t* p) {
        return __builtin_nontemporal_load((const u32ua*)p);
    }
    static __device__ __forceinline__ void st(uint8_t* p, T v) {
        __builtin_nontemporal_store(v, (u32ua*)p);
    }
};

template <int VS, int K, bool DECODE>
__global__ __launch_bounds__(256) void xor_flat_kernel(
    const uint8_t* __restrict__ in, uint8_t* out, const uint8_t* __restrict__ eidx, int k,
    int bb, int nu, unsigned total_units, long long in_gstride, long long out_gstride,
    long long e_stride) {
    typedef typename Unit<VS>::T V;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total_units) return;
    const unsigned g = u / (unsigned)nu;
    const int q = (int)(u - g * (unsigned)nu);
    const int off = min(q * VS, bb - VS);
    const uint8_t* p = in + (long long)g * in_gstride + off;
    int e = 0;
    if (DECODE) e = eidx[g];   // issued beside the data loads
    V acc = Unit<VS>::ld(p);
    if (K) {
#pragma unroll
        for (int x = 1; x < (K ? K : 1); ++x) acc ^= Unit<VS>::ld(p + (long long)x * bb);
    } else {
#pragma unroll 4
        for (int x = 1; x < k; ++x) acc ^= Unit<VS>::ld(p + (long long)x * bb);
    }
    uint8_t* dst = out + (long long)g * out_gstride;
    if (DECODE) {
        if (e == 255) return;   // nothing erased in this group
        dst += (long long)e * e_stride;   // e_stride 0: recovered-blocks layout
    }
    const int own = q * VS;   // first byte this unit owns
    if (own + VS <= bb) {
        Unit<VS>::st(dst + off, acc);
    } else {
        // tail unit: owns bytes [own, bb) = the top (bb - own) bytes of the shifted vector
        const int skip = own - off;
        const uint8_t* b = (const uint8_t*)&acc;
        if (VS == 16 && skip == 8) {
            *(uint64_t*)(dst + own) = ((const uint64_t*)b)[1];
        } else {
            for (int i = skip; i < VS; ++i) dst[off + i] = b[i];
        }
    }
}

// Tiny blocks (bb < 4): one byte per lane.
template <bool DECODE>
__global__ __launch_bounds__(256) void xor_bytes_kernel(
    const uint8_t* __restrict__ in, uint8_t* out, const uint8_t* __restrict__ eidx, int k,
    int bb, long long total, long long in_gstride, long long out_gstride, long long e_stride) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= total) return;
    const long long g = u / bb;
    const int i = (int)(u % bb);
    const uint8_t* p = in + g * in_gstride + i;
    uint8_t acc = 0;
    for (int x = 0; x < k; ++x) acc ^= p[(long long)x * bb];
    uint8_t* dst = out + g * out_gstride;
    if (DECODE) {
        const int e = eidx[g];
        if (e == 255) return;
        dst += (long long)e * e_stride;
    }
    dst[i] = acc;
}

// m = 1 decode bookkeeping (cauchy_decode_m1, cauchy_256.cpp:486-540), one thread per
// group: the erased slot is the first with row >= k; its new row is the first data row
// not tagged by any other slot.  eidx[g] = that slot (255 = nothing erased).  compact:
// rows_out is [G] and receives the recovered data row (255 = nothing erased) instead of
// the rewritten tags.
__global__ __launch_bounds__(256) void m1_prep_kernel(const uint8_t* __restrict__ rows_in,
                                                      uint8_t* rows_out,
                                                      int32_t* __restrict__ status,
                                                      uint8_t* __restrict__ eidx, int k,
                                                      long long groups, int compact) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const uint8_t* rg = rows_in + g * k;
    uint8_t* ro = compact ? nullptr : rows_out + g * k;
    uint64_t seen[4] = {0, 0, 0, 0};
    int e = -1;
    for (int i = 0; i < k; ++i) {
        const int r = rg[i];
        if (r >= k) {
            if (e < 0) { e = i; continue; }
        }
        if (r < k) seen[r >> 6] |= 1ull << (r & 63);
        if (ro && ro != rg) ro[i] = (uint8_t)r;
    }
    if (status) status[g] = 0;
    if (e < 0) {
        eidx[g] = 255;
        if (compact) rows_out[g] = 255;
        return;
    }
    int miss = -1;
    for (int w = 0; w < 4 && miss < 0; ++w) {
        const uint64_t free = ~seen[w];
        if (free) {
            const int b = w * 64 + __ffsll((long long)free) - 1;
            if (b < k) miss = b;
            break;
        }
    }
    const uint8_t nr = miss >= 0 ? (uint8_t)miss : rg[e];
    if (compact) rows_out[g] = nr;
    else ro[e] = nr;
    eidx[g] = (uint8_t)e;
}

__global__ void replicate_kernel(const uint8_t* __restrict__ data, uint8_t* __restrict__ parity,
                                 int m, int bb, long long groups) {
    const long long total = groups * m * (long long)bb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long g = i / ((long long)m * bb);
        const long long b = i % bb;
        parity[i] = data[g * bb + b];   // k = 1: the group holds one block
    }
}

// k <= 1, recovered-blocks layout: a block tagged anything but row 0 is a parity copy of
// data row 0 (cauchy_256.cpp:1508-1516), so it is that row's recovered block.
__global__ void rec_k1_kernel(const uint8_t* __restrict__ blocks, const uint8_t* __restrict__ rows_in,
                              uint8_t* __restrict__ rec, uint8_t* __restrict__ rec_rows,
                              int32_t* __restrict__ status, int bb, int rmax, long long groups) {
    const long long total = groups * (long long)bb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long g = i / bb;
        const long long b = i % bb;
        const bool lost = rows_in[g] != 0;
        if (lost) rec[g * rmax * (long long)bb + b] = blocks[g * (long long)bb + b];
        if (b == 0) {
            rec_rows[g * rmax] = lost ? 0 : 255;
            if (status) status[g] = 0;
        }
    }
}

__global__ void rows_k1_kernel(const uint8_t* __restrict__ rows_in, uint8_t* rows_out,
                               int32_t* __restrict__ status, long long groups) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    rows_out[g] = 0;
    (void)rows_in;
    if (status) status[g] = 0;
}

// Column-word access (col_access / load_raw / store_word): gf_colword.h, shared with the
// ragged kernels.

// Workgroup-size bound per output-chunk width: it caps VGPRs at 512 / ceil(waves / 4), so
// the RC x 8 accumulators never spill (RC 4: 128 VGPR, RC 8: 170, RC 16: 256).
template <int RC> struct ApplyBound { static constexpr int T = RC <= 4 ? 1024 : (RC == 8 ? 640 : 320); };

// One wave = one (group, output chunk, 64-word column tile).  RC outputs per wave.
//   coef:  [(g) * coef_gstride + (chunk * k + pos) * RCP + j]  (RCP = max(4, RC))
//   encode: outputs o = chunk*RC + j < m go to out + g*out_gstride + o*bb
//   decode: outputs o < nout[g] go to out + g*out_gstride + slots[g*rmax + o]*bb
//   FLAT (encode only: the coefficients are the same for every group): the lanes of a wave
//   take consecutive (group, column word) pairs across group boundaries, so no lane idles
//   when a sub-row is not a multiple of 64 words (169-byte sub-rows: 43 words, 67 % of a
//   wave); waves are numbered (lane tile, chunk) with the chunk fastest.
template <int RC, bool DECODE, bool TINY, int PD, bool FLAT = false>
__global__ __launch_bounds__(ApplyBound<RC>::T) void gf_apply_kernel(
    const uint8_t* __restrict__ in, uint8_t* out, const uint8_t* __restrict__ coef,
    const uint8_t* __restrict__ slots, const int32_t* __restrict__ nout, int k, int m, int bb,
    int nw, int ntiles, int nchunk, int rmax, long long coef_gstride, long long out_gstride,
    int total_units, long long flat_lanes = 0) {
    static_assert(!(FLAT && DECODE), "decode coefficients differ per group");
    constexpr int RCP = RC < 4 ? 4 : RC;
    constexpr int NCW = RCP / 4;
    const int lane = threadIdx.x & 63;
    // Units are numbered (group, chunk, tile) with the tile fastest; a workgroup holds 4
    // consecutive units.  The chunks of a group re-read the same input blocks, so the
    // workgroups of one group should share an L2: hardware deals workgroups round-robin
    // to the 8 XCDs (each with its own L2), so logical workgroup l runs as hardware
    // block b with consecutive l on one XCD (a bijection for any grid size).
    const unsigned nbk = gridDim.x, b = blockIdx.x, xcd = b & 7u, q8 = nbk >> 3, r8 = nbk & 7u;
    const unsigned lwg = xcd * q8 + (xcd < r8 ? xcd : r8) + (b >> 3);
    const int unit = (int)lwg * 4 + wave_id();
    if (unit >= total_units) return;
    int g, chunk, c;
    bool live = true;
    if (FLAT) {
        chunk = unit % nchunk;
        long long u = (long long)(unit / nchunk) * 64 + lane;
        live = u < flat_lanes;
        if (!live) u = flat_lanes - 1;
        g = (int)(u / nw);
        c = (int)(u - (long long)g * nw);
    } else {
        const int tile = unit % ntiles;
        const int gc = unit / ntiles;
        chunk = gc % nchunk;
        g = gc / nchunk;
        c = tile * 64 + lane;
    }
    int n = DECODE ? nout[g] : m;
    n = min(n - chunk * RC, RC);
    if (n <= 0) return;
    const int s = bb >> 3;
    const ColAccess ca = col_access<TINY>(c, nw, s);

    const uint8_t* gin = in + (long long)g * k * bb;
    const uint32_t* cw = (const uint32_t*)(coef + (FLAT ? 0 : (long long)g * coef_gstride) +
                                           (long long)chunk * k * RCP);

    uint32_t acc[RC][8];
#pragma unroll
    for (int j = 0; j < RC; ++j)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[j][r] = 0;

    // Software pipeline PD blocks deep: raw words of blocks pos+1 .. pos+PD are in flight
    // while block pos is combined (the realigning shift is applied at use, so the
    // compiler's vmcnt wait lands at the consumer).  The loop is unrolled by PD so every
    // ring slot is a fixed register set.  Loads past the last block are clamped to it.
    uint32_t raw[PD][8];
#pragma unroll
    for (int u = 0; u < PD; ++u) {
        const uint8_t* p = gin + (long long)min(u, k - 1) * bb;
#pragma unroll
        for (int t = 0; t < 8; ++t) raw[u][t] = load_raw<TINY>(p + t * s, ca, s);
    }

#pragma unroll 1
    for (int pos0 = 0; pos0 < k; pos0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const int pos = pos0 + u;
            if (pos < k) {
                WZ v;
#pragma unroll
                for (int t = 0; t < 8; ++t) v.W[t] = TINY ? raw[u][t] : (raw[u][t] >> ca.shift);
                const uint8_t* p = gin + (long long)min(pos + PD, k - 1) * bb;
#pragma unroll
                for (int t = 0; t < 8; ++t) raw[u][t] = load_raw<TINY>(p + t * s, ca, s);
                uint32_t cwv[NCW];
#pragma unroll
                for (int q = 0; q < NCW; ++q) cwv[q] = cw[pos * NCW + q];
                expand_wz(v);
#pragma unroll
                for (int j = 0; j < RC; ++j) {
                    if (j < n) {
                        const uint32_t a = (cwv[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                        apply_nibble<0>(acc[j], a & 15u, v);
                        apply_nibble<4>(acc[j], a >> 4, v);
                    }
                }
            }
        }
    }

    if (!live) return;
#pragma unroll
    for (int j = 0; j < RC; ++j) {
        if (j < n) {
            const int o = chunk * RC + j;
            const int slot = (DECODE && slots) ? slots[(long long)g * rmax + o] : o;
            uint8_t* dst = out + (long long)g * out_gstride + (long long)slot * bb;
#pragma unroll
            for (int r = 0; r < 8; ++r) store_word(dst + r * s, c, ca, acc[j][r]);
        }
    }
}

// In-place decode with more recovered blocks than one wave holds: the chunks write to a
// [G][rmax][bb] scratch, then this copies each recovered block into its slot.
__global__ __launch_bounds__(256) void scatter_recovered_kernel(
    const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
    const uint8_t* __restrict__ slots, const int32_t* __restrict__ nout, int k, int bb,
    int rmax, long long units) {
    const long long u = (long long)blockIdx.x * 4 + wave_id();
    if (u >= units) return;
    const long long g = u / rmax;
    const int o = (int)(u % rmax);
    if (o >= nout[g]) return;
    const int lane = threadIdx.x & 63;
    const uint8_t* from = scratch + u * (long long)bb;
    uint8_t* to = out + (g * k + slots[g * rmax + o]) * (long long)bb;
    for (int q = lane; q < bb; q += 64) to[q] = from[q];
}

// ----------------------------------------------------------------------- synth
__device__ __forceinline__ uint64_t splitmix64_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ void synth_fill_kernel(uint8_t* __restrict__ dst, unsigned long long bytes,
                                  unsigned long long seed, unsigned long long off) {
    // requires off % 8 == 0; word i of dst = stream word off/8 + i
    const unsigned long long nwords = bytes / 8;
    const unsigned long long w0 = off / 8;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < nwords; i += (unsigned long long)gridDim.x * blockDim.x)
        ((uint64_t*)dst)[i] = splitmix64_mix(seed + (w0 + i + 1) * 0x9E3779B97F4A7C15ULL);
    const unsigned long long tail = bytes - nwords * 8;
    if (blockIdx.x == 0 && threadIdx.x < tail) {
        const uint64_t w = splitmix64_mix(seed + (w0 + nwords + 1) * 0x9E3779B97F4A7C15ULL);
        dst[nwords * 8 + threadIdx.x] = (uint8_t)(w >> (8 * threadIdx.x));
    }
}

__global__ __launch_bounds__(256) void synth_gather_kernel(
    const uint8_t* __restrict__ data, const uint8_t* __restrict__ parity,
    const int16_t* __restrict__ src, uint8_t* __restrict__ blocks, int k, int m, int bb,
    long long units) {
    const long long u = (long long)blockIdx.x * 4 + wave_id();
    if (u >= units) return;
    const int lane = threadIdx.x & 63;
    const long long g = u / k;
    const int sidx = src[u];
    const uint8_t* from = sidx < k ? data + (g * k + sidx) * (long long)bb
                                   : parity + (g * m + (sidx - k)) * (long long)bb;
    uint8_t* to = blocks + u * (long long)bb;
    if ((bb & 7) == 0) {
        for (int q = lane; q < bb / 8; q += 64) ((u64a*)to)[q] = ((const u64a*)from)[q];
    } else {
        for (int q = lane; q < bb; q += 64) to[q] = from[q];
    }
}

// ---------------------------------------------------------------------- launchers
static inline unsigned blocks_for_waves(long long waves) { return (unsigned)((waves + 3) / 4); }

// 16-byte units need 8-byte alignment of both buffers and of every block; otherwise
// unaligned 4-byte units; blocks under 4 bytes go bytewise.
static int xor_unit(const void* a, const void* b, long long s1, long long s2, int bb) {
    const uintptr_t al = (uintptr_t)a | (uintptr_t)b | (uintptr_t)s1 | (uintptr_t)s2 |
                         (uintptr_t)bb;
    if (bb >= 16 && (al & 7) == 0) return 16;
    return bb >= 4 ? 4 : 1;
}

template <int VS, bool DECODE>
static void xor_flat_launch(const uint8_t* in, uint8_t* out, const uint8_t* eidx, int k, int bb,
                            long long G, long long igs, long long ogs, hipStream_t st,
                            long long es) {
    const int nu = (bb + VS - 1) / VS;
    const unsigned total = (unsigned)(G * nu);
    const unsigned nb = (total + 255) / 256;
    // k at compile time for configs A and B/C, else at run time
    const auto go = [&](auto KC) {
        qlaunch((xor_flat_kernel<VS, decltype(KC)::value, DECODE>), dim3(nb), dim3(256), 0, st, in,
                out, eidx, k, bb, nu, total, igs, ogs, es);
    };
    if (!dispatch_value<10, 32>(k, go)) go(std::integral_constant<int, 0>{});
}

template <bool DECODE>
static hipError_t xor_any(const uint8_t* in, uint8_t* out, const uint8_t* eidx, int k, int bb,
                          long long G, long long igs, long long ogs, hipStream_t st,
                          const Tune& t, long long es = -1) {
    if (es < 0) es = bb;
    if (G <= 0) return hipSuccess;
    if (es == bb && igs == (long long)k * bb && xor_dma_ok(in, out, k, bb, ogs, t))
        return launch_xor_dma(in, out, eidx, nullptr, nullptr, nullptr, k, bb, G, ogs, DECODE, st,
                              t);
    note_kernel(DECODE ? "xor_flat_kernel<decode>" : "xor_flat_kernel<encode>");
    const int vs = xor_unit(in, out, igs, ogs, bb);
    const long long units = G * ((bb + vs - 1) / vs);
    if (units > 0xffffffffLL) return hipErrorInvalidValue;
    if (vs == 16) xor_flat_launch<16, DECODE>(in, out, eidx, k, bb, G, igs, ogs, st, es);
    else if (vs == 4) xor_flat_launch<4, DECODE>(in, out, eidx, k, bb, G, igs, ogs, st, es);
    else qlaunch((xor_bytes_kernel<DECODE>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st, in, out, eidx, k, bb, units, igs, ogs, es);
    return hipGetLastError();
}

hipError_t launch_xor_encode(const uint8_t* data, uint8_t* parity, int k, int bb,
                             long long groups, long long out_gstride, hipStream_t st,
                             const Tune& t) {
    return xor_any<false>(data, parity, nullptr, k, bb, groups, (long long)k * bb, out_gstride,
                          st, t);
}

hipError_t launch_xor_decode(const uint8_t* blocks, uint8_t* out, const uint8_t* rows_in,
                             uint8_t* rows_out, int32_t* status, uint8_t* eidx, int k, int bb,
                             long long groups, hipStream_t st, const Tune& t, bool compact) {
    if (groups <= 0) return hipSuccess;
    const long long gb = (long long)k * bb;
    const long long ogs = compact ? bb : gb;
    if (k <= 64 && xor_dma_ok(blocks, out, k, bb, ogs, t))
        // single launch: the DMA kernel also does the erased-slot / missing-row bookkeeping
        return launch_xor_dma(blocks, out, nullptr, rows_in, rows_out, status, k, bb, groups, ogs,
                              true, st, t, compact);
    const hipError_t e = launch_m1_prep(rows_in, rows_out, status, eidx, k, groups, compact, st);
    if (e != hipSuccess) return e;
    return xor_any<true>(blocks, out, eidx, k, bb, groups, gb, ogs, st, t, compact ? 0 : bb);
}

hipError_t launch_m1_prep(const uint8_t* rows_in, uint8_t* rows_out, int32_t* status,
                          uint8_t* eidx, int k, long long groups, bool compact, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    note_kernel("m1_prep_kernel");
    qlaunch((m1_prep_kernel), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, rows_in,
            rows_out, status, eidx, k, groups, compact ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_replicate(const uint8_t* data, uint8_t* parity, int m, int bb,
                            long long groups, hipStream_t st) {
    if (groups <= 0 || m <= 0) return hipSuccess;
    const long long total = groups * m * (long long)bb;
    const unsigned nb = (unsigned)std::min<long long>((total + 255) / 256, 65536);
    note_kernel("replicate_kernel");
    qlaunch((replicate_kernel), dim3(nb), dim3(256), 0, st, data, parity, m, bb, groups);
    return hipGetLastError();
}

hipError_t launch_rec_k1(const uint8_t* blocks, const uint8_t* rows_in, uint8_t* rec,
                        uint8_t* rec_rows, int32_t* status, int bb, int rmax, long long groups,
                        hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    const long long total = groups * (long long)bb;
    const unsigned nb = (unsigned)std::min<long long>((total + 255) / 256, 65536);
    note_kernel("rec_k1_kernel");
    qlaunch((rec_k1_kernel), dim3(nb), dim3(256), 0, st, blocks, rows_in, rec, rec_rows, status, bb, rmax, groups);
    return hipGetLastError();
}

hipError_t launch_rows_k1(const uint8_t* rows_in, uint8_t* rows_out, int32_t* status,
                          long long groups, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    note_kernel("rows_k1_kernel");
    qlaunch((rows_k1_kernel), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, rows_in, rows_out, status,
                                                                     groups);
    return hipGetLastError();
}

// nchunk: the chunks of rc outputs (encode: of m, decode: of rmax)
template <bool DECODE>
static hipError_t gf_apply_dispatch(const Apply& a, int nchunk) {
    const Tune& t = *a.t;
    const int bb = a.bb, rc = a.rc;
    const long long groups = a.groups;
    const int s = bb / 8;
    const int nw = (s + 3) / 4;
    const int ntiles = (nw + 63) / 64;
    const bool flat = !DECODE && s >= 4 && t.flat && (nw & 63) != 0;
    const long long flat_lanes = groups * nw;
    const long long units = flat ? nchunk * ((flat_lanes + 63) / 64) : groups * nchunk * ntiles;
    if (units <= 0) return hipSuccess;
    if (units > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned nb = blocks_for_waves(units);
    const unsigned nthr = 256;
    const int tu = (int)units;
    const int pd = t.pd;
    if (pd < 1 || pd > 3) return hipErrorInvalidValue;
    note_kernel(DECODE ? "gf_apply_kernel<decode>"
                       : (flat ? "gf_apply_kernel<encode,flat>" : "gf_apply_kernel<encode>"));
    const auto go = [&](auto kern) {
        qlaunch(kern, dim3(nb), dim3(nthr), 0, a.st, a.in, a.out, a.tab, a.slots, a.nout, a.k, a.m,
                bb, nw, ntiles, nchunk, a.rmax, a.tab_gstride, a.out_gstride, tu, flat_lanes);
    };
    const bool known = dispatch_value<1, 2, 4, 8, 16>(rc, [&](auto RC) {
        constexpr int rcv = decltype(RC)::value;
        if (flat) {
            if constexpr (!DECODE) go(gf_apply_kernel<rcv, false, false, 2, true>);
        } else if (s < 4) {
            go(gf_apply_kernel<rcv, DECODE, true, 1>);
        } else {
            dispatch_value<1, 2, 3>(pd, [&](auto PD) {
                go(gf_apply_kernel<rcv, DECODE, false, decltype(PD)::value>);
            });
        }
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_gf_encode(const Apply& a) {
    return gf_apply_dispatch<false>(a, (a.m + a.rc - 1) / a.rc);
}

hipError_t launch_gf_decode(const Apply& a) {
    return gf_apply_dispatch<true>(a, (a.rmax + a.rc - 1) / a.rc);
}

hipError_t launch_scatter_recovered(const uint8_t* scratch, uint8_t* out, DecodeWork w, int k,
                                   int bb, int rmax, long long groups, hipStream_t st) {
    const long long units = groups * rmax;
    if (units <= 0) return hipSuccess;
    note_kernel("scatter_recovered_kernel");
    qlaunch((scatter_recovered_kernel), dim3(blocks_for_waves(units)), dim3(256), 0, st, scratch, out, w.slots,
                                                                      w.nout, k, bb, rmax,
                                                                      units);
    return hipGetLastError();
}

hipError_t launch_synth_fill(uint8_t* dst, unsigned long long bytes, unsigned long long seed,
                             unsigned long long byte_offset, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (byte_offset % 8) return hipErrorInvalidValue;
    const unsigned long long words = bytes / 8 + 1;
    const unsigned nb = (unsigned)std::min<unsigned long long>((words + 255) / 256, 1u << 16);
    qlaunch((synth_fill_kernel), dim3(nb), dim3(256), 0, st, dst, bytes, seed, byte_offset);
    return hipGetLastError();
}

hipError_t launch_synth_gather(const uint8_t* data, const uint8_t* parity, const int16_t* src,
                               uint8_t* blocks, int k, int m, int bb, long long groups,
                               hipStream_t st) {
    const long long units = groups * k;
    if (units <= 0) return hipSuccess;
    qlaunch((synth_gather_kernel), dim3(blocks_for_waves(units)), dim3(256), 0, st, data, parity, src, blocks, k,
                                                                 m, bb, units);
    return hipGetLastError();
}

}  // namespace qfec
