// gf_bsyn.hip — syndrome decode of a compiled small-block code: BASELINE configs B and C,
// (32 data + 4 parity) x 1352 B blocks, r <= 4 erasures.
//
// The reference decodes in two stages (cauchy_256_decode, cauchy_256.cpp:1269-1420): the
// received originals are eliminated from the recovery rows, then the r x r system over the
// erased rows is solved.  With y_i the parity row of received recovery block R_i:
//   T_y = R_y ^ sum_{present data rows x} C[y][x] D_x      (syndromes, y = 0 .. m - 1)
//   E_j = sum_{i < r} Sinv[j][i] T_{y_i}                    (the r x r solve)
// The recovered bytes are the unique solution, so any exact solver is bit-exact.  Here the
// syndromes of ALL m parity rows are formed with the compile-time Cauchy coefficients of
// row x (cauchy_const.h; the windowed form of gf_bitslice.h, one v_bitop3 per (row,
// sub-row)), exactly the work of the compiled encode: no per-(row, block) coefficient
// loads or scalar nibble dispatch, which cost the run-time decode (gf_stream_kernel<decode>)
// more scalar than vector instructions.  Run-time coefficients remain only in the r x r
// solve (r^2 nibble applies per group against k block steps) and for the rare extra block
// that repeats a data row.
//
// Stream: every wave owns groups g0, g0 + W, ... (no barriers, no cross-wave traffic) and
// streams each group's k received blocks in the order the prep's table gives
// (decode_prep_bsyn_kernel, decode_prep.hip; bsyn:: in fec_kernels.h): the present data
// rows ascending, then the extras (recovery blocks, repeated data rows) in slot order.
// A block is read from wherever its slot lies (bb = 1352 is 8 mod 16: the 16-byte aligned
// envelope of the block is DMA'd, buffer_load_dwordx4 ... lds, and the block is read at the
// 8-byte skew), into a ring of D + 1 block buffers per wave.  The unrolled loop over the k
// data rows consumes the next streamed block only where row x is present (a uniform branch
// per row), so every coefficient stays a compile-time constant.
//
// vmcnt bookkeeping (primitives in gf_counted.h): a block is NPC DMA instructions; a group's stores
// (8 * SPR per recovered block) sit in the count before the waits for the next group's
// blocks 1 .. D - 1.  tests/test_isa.py checks the compiler adds no VMEM instruction or
// vmcnt wait of its own.
#include "cauchy_const.h"
#include "compiled_codes.h"
#include "fec_kernels.h"
#include "gf256.h"
#include "gf_bitslice.h"
#include "gf_counted.h"
#include "gf_winjump.h"

namespace qfec {

// s_waitcnt vmcnt(BASE + 8 * SPR * n) for a wave-uniform n in [0, 4] (the stores of a group
// with n recovered blocks), capped at 63
template <int BASE, int PER>
__device__ __forceinline__ void bsyn_wait_stores(int n) {
    constexpr int W0 = BASE, W1 = BASE + PER > 63 ? 63 : BASE + PER;
    constexpr int W2 = BASE + 2 * PER > 63 ? 63 : BASE + 2 * PER;
    constexpr int W3 = BASE + 3 * PER > 63 ? 63 : BASE + 3 * PER;
    constexpr int W4 = BASE + 4 * PER > 63 ? 63 : BASE + 4 * PER;
    if (n <= 1) {
        if (n <= 0) wait_vmcnt<W0>();
        else wait_vmcnt<W1>();
    } else if (n <= 2) {
        wait_vmcnt<W2>();
    } else {
        if (n == 3) wait_vmcnt<W3>();
        else wait_vmcnt<W4>();
    }
}

constexpr int kBsynWaves = 4;   // waves per workgroup (independent)
constexpr int kBsynRC = 4;      // recovered blocks per group (rmax <= 4)

// KC, MC: the compiled code (k, m); S: sub-row bytes; D: blocks in flight per wave.
// NTS: the recovered blocks are stored non-temporal
template <int KC, int MC, int S, int D, bool NTS = false>
__global__ __launch_bounds__(kBsynWaves * 64) void gf_bsyn_kernel(
    const uint8_t* in, uint8_t* out, const uint8_t* __restrict__ tab,
    const uint8_t* __restrict__ cenc, const uint8_t* __restrict__ slots,
    const int32_t* __restrict__ nout, long long groups, int rmax, long long out_gstride) {
    using SH = SubrowShape<S>;
    constexpr int BB = SH::BB, NW = SH::NW, SPR = SH::SPR;
    constexpr int BUFB = SH::BUFB, NPC = SH::NPC, P1L = SH::P1L;
    constexpr int NB = D + 1;                 // the block being read + D in flight
    constexpr int RC = kBsynRC;
    constexpr int WAITN = (D - 1) * NPC;      // younger than block b + 1 when it is awaited
    static_assert(WAITN <= 63 && D >= 2 && KC >= D, "pipeline depth");
    static_assert(KC <= 64 && MC <= 8 && (KC * BB) % 16 == 0 && BB % 8 == 0 && NB <= 32,
                  "compiled small-block code");
    static_assert(KC % 2 == 0, "register double buffer parity");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int lane = threadIdx.x & 63;
    const int w = wave_id();
    uint8_t* ring = smem + (size_t)w * NB * BUFB;
    const long long W = (long long)gridDim.x * kBsynWaves;
    const long long g0 = (long long)blockIdx.x * kBsynWaves + w;
    if (g0 >= groups) return;
    const int cnt = __builtin_amdgcn_readfirstlane((int)((groups - 1 - g0) / W + 1));
    const int c = lane < NW ? lane : NW - 1;  // idle lanes shadow the last word

    // ---- DMA side: stream block b = position iss_x of group g0 + i * W, the slot the table
    // names there, into ring buffer iss_buf; bit iss_buf of `skew` = its 8-byte skew.  Past
    // the stream's end the last block is re-read (every step issues and waits the same way).
    int iss_buf = 0, iss_x = 0;
    int iss_left = cnt * KC;
    const uint8_t* iss_g = in + g0 * (long long)(KC * BB);
    const uint8_t* iss_t = tab + g0 * (long long)bsyn::kBytes;
    const long long gstride = W * (long long)(KC * BB);
    const long long tstride = W * (long long)bsyn::kBytes;
    uint32_t perm_w = 0, skew = 0;
    auto issue_next = [&]() __attribute__((always_inline)) {
        if ((iss_x & 3) == 0) perm_w = cload_u32(iss_t, bsyn::kPerm + iss_x);
        const int slot = min((int)((perm_w >> (8 * (iss_x & 3))) & 0xFFu), KC - 1);
        const int off = slot * BB;
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)iss_g, 0, 0x7FFFFFFF, 0x00020000);
        uint8_t* dst = ring + iss_buf * BUFB;
        dma16(rs, dst, 16u * (uint32_t)lane, off & ~15);
        if constexpr (NPC == 2)
            if (lane < P1L) dma16(rs, dst + 1024, 1024u + 16u * (uint32_t)lane, off & ~15);
        skew = (off & 15) ? (skew | (1u << iss_buf)) : (skew & ~(1u << iss_buf));
        if (++iss_buf == NB) iss_buf = 0;
        if (--iss_left > 0 && ++iss_x == KC) {
            iss_x = 0;
            iss_g += gstride;
            iss_t += tstride;
        }
    };
    // column word c of the 8 sub-rows of stream block bi: aligned dwords (the buffer start
    // plus the skew is 8-byte aligned, sub-row t is misaligned by the constant (t*S) & 3)
    auto read_block = [&](int bi, uint32_t (&lo)[8], uint32_t (&hi)[8])
                          __attribute__((always_inline)) {
        const int buf = (int)((unsigned)bi % NB);
        uint32_t a = 4u * (uint32_t)c + (uint32_t)(buf * BUFB) + (((skew >> buf) & 1u) << 3);
        asm volatile("" : "+v"(a));   // no hoisting across blocks
        read_subrows<S>(ring + a, lo, hi);
    };

#pragma unroll 1
    for (int u = 0; u < D; ++u) issue_next();
    uint32_t lo0[8], hi0[8], lo1[8], hi1[8];
    wait_vmcnt<WAITN>();
    read_block(0, lo0, hi0);

    int b = 0;        // stream index of the block in (lo0, hi0) / the current block
    int prev_n = -1;  // recovered blocks the previous group stored (-1: no previous group)
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
        const long long g = g0 + (long long)i * W;
        const uint8_t* tb = tab + g * (long long)bsyn::kBytes;
        const uint32_t mlo = cload_u32(tb, bsyn::kMask), mhi = cload_u32(tb, bsyn::kMask + 4);
        const uint32_t ymap = cload_u32(tb, bsyn::kY);
        const int n = min(min(nout[g], rmax), RC);
        const int ne = KC - __builtin_popcount(mlo) - __builtin_popcount(mhi);
        int p = 0;    // blocks of this group consumed
        uint32_t acc[MC][8];
#pragma unroll
        for (int y = 0; y < MC; ++y)
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[y][r] = 0;

        // consume the block in (lo, hi): prefetch block b + D, pull block b + 1 into
        // (nlo, nhi), return block b's realigned words
        auto advance = [&](const uint32_t (&lo)[8], const uint32_t (&hi)[8], uint32_t (&nlo)[8],
                           uint32_t (&nhi)[8], uint32_t (&wv)[8]) __attribute__((always_inline)) {
            issue_next();
            // block b + 1 is position p + 1 of this group (the next group's position 0 when
            // p + 1 == KC, awaited before this group's stores); positions 1 .. D - 1 were
            // DMA'd before the previous group's stores, which are younger
            if (prev_n >= 0 && p + 1 <= D - 1)
                bsyn_wait_stores<WAITN, 8 * SPR>(prev_n);
            else
                wait_vmcnt<WAITN>();
            read_block(b + 1, nlo, nhi);
            ++b;
            ++p;
#pragma unroll
            for (int t = 0; t < 8; ++t) wv[t] = realign_word<S>(lo, hi, t);
        };
        // data row x (compile time): its block, if present, into every syndrome row
        auto row_step = [&](auto xc, uint32_t (&lo)[8], uint32_t (&hi)[8], uint32_t (&nlo)[8],
                            uint32_t (&nhi)[8]) __attribute__((always_inline)) {
            constexpr int x = decltype(xc)::value;
            const uint32_t mw = x < 32 ? mlo : mhi;
            if ((mw >> (x & 31)) & 1u) {
                uint32_t wv[8];
                advance(lo, hi, nlo, nhi, wv);
                Win win;
                win_build(wv, win);
                static_for<MC>([&](auto yc) __attribute__((always_inline)) {
                    constexpr int y = decltype(yc)::value;
                    win_apply<cauchy_coef(MC, y, x)>(acc[y], win);
                });
            } else {
                // row x erased: the block waiting in (lo, hi) is the next present row's
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    nlo[t] = lo[t];
                    nhi[t] = hi[t];
                }
            }
        };
        static_for<KC>([&](auto xc) __attribute__((always_inline)) {
            // accumulators opaque at every block boundary (no cross-block XOR reassociation)
#pragma unroll
            for (int y = 0; y < MC; ++y)
#pragma unroll
                for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(acc[y][r]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(xc)::value % 2 == 0) row_step(xc, lo0, hi0, lo1, hi1);
            else row_step(xc, lo1, hi1, lo0, hi0);
        });

        // extras: a received parity row y adds its block to T_y; a repeated data row adds
        // C[y][row] times its block to every T_y (run-time coefficients, cenc = [m][k])
        auto extra = [&](int e, uint32_t (&lo)[8], uint32_t (&hi)[8], uint32_t (&nlo)[8],
                         uint32_t (&nhi)[8]) __attribute__((always_inline)) {
            WZ v;
            advance(lo, hi, nlo, nhi, v.W8);
            const int row = cload_u8(tb, bsyn::kERow + e);
            if (row >= KC) {
                const int y = row - KC;   // >= MC (255: a no-op extra of an unchanged group)
                static_for<MC>([&](auto yc) __attribute__((always_inline)) {
                    constexpr int yy = decltype(yc)::value;
                    if (y == yy) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) acc[yy][r] ^= v.W[r];
                    }
                });
            } else {
                expand_wz(v);
                static_for<MC>([&](auto yc) __attribute__((always_inline)) {
                    constexpr int yy = decltype(yc)::value;
                    const uint32_t cf = (uint32_t)cload_u8(cenc, yy * KC + row);
                    apply_nibble<0>(acc[yy], cf & 15u, v);
                    apply_nibble<4>(acc[yy], cf >> 4, v);
                });
            }
        };
#pragma unroll 1
        for (int e = 0; e + 1 < ne; e += 2) {
            extra(e, lo0, hi0, lo1, hi1);
            extra(e + 1, lo1, hi1, lo0, hi0);
        }
        if (ne & 1) {
            extra(ne - 1, lo0, hi0, lo1, hi1);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                lo0[t] = lo1[t];
                hi0[t] = hi1[t];
            }
        }

        // ---- E_j = sum_i Sinv[j][i] T_{y_i}, one recovered block at a time, stored as soon
        // as it is formed (8 * SPR store instructions per recovered block)
        asm volatile("" ::: "memory");   // stores stay in issue order among the DMAs
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            uint32_t o[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) o[r] = 0;
            const uint32_t sw = cload_u32(tb, bsyn::kSinv + 4 * j);   // Sinv[j][0..3]
#pragma unroll 1
            for (int ii = 0; ii < n; ++ii) {
                const int y = (int)((ymap >> (8 * ii)) & 0xFFu);
                WZ v;
                static_for<MC>([&](auto yc) __attribute__((always_inline)) {
                    constexpr int yy = decltype(yc)::value;
                    if (y == yy) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) v.W[r] = acc[yy][r];
                    }
                });
                expand_wz(v);
                // the product by two nibble jumps (gf_winjump.h), not two branch trees
                wz_mul_acc_rt(o, v, (sw >> (8 * ii)) & 0xFFu);
            }
            const int oslot = slots ? cload_u8(slots, (int)(g * rmax + j)) : j;
            uint8_t* dst = out + g * out_gstride + (long long)oslot * BB;
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
            // lane offsets from the lane id (not kept live across the block loop)
            const int ln = (int)__lane_id();
            store_subrows<S, NTS ? 2 : 0>(rs, o, subrow_lanes(ln, ln, NW, SH::NWF));
        }
        asm volatile("" ::: "memory");
        prev_n = n;
    }
    wait_vmcnt<0>();
}

// ------------------------------------------------------------------ launchers
namespace {
constexpr int kBsynS = kCompiledS;   // bb = 1352: 1350-byte payloads (BASELINE configs B, C)
}  // namespace

bool gf_bsyn_supported(int k, int m, int bb, int rmax, const Tune& t) {
    return t.bsyn && t.const_enc && rmax <= kBsynRC && find_code(k, m, bb, Syn::bsyn);
}

hipError_t launch_gf_bsyn(const Apply& a) {
    const Tune& t = *a.t;
    const int k = a.k, m = a.m;
    if (a.groups <= 0) return hipSuccess;
    if (!gf_bsyn_supported(k, m, a.bb, a.rmax, t)) return hipErrorInvalidValue;
    if ((((uintptr_t)a.in) & 15) ||
        ((((uintptr_t)a.tab) | (uintptr_t)a.cenc | (uintptr_t)a.slots) & 3))
        return hipErrorInvalidValue;
    using SH = SubrowShape<kBsynS>;
    const int D = t.bsyn_depth;
    if (D != 3 && D != 5 && D != 7) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBsynWaves * (D + 1) * SH::BUFB;
    const int per_cu = lds_blocks_per_cu(lds, 20 / kBsynWaves);
    // oversubscribed: about bwg groups per wave (B decode 0.60-0.61 -> 0.53-0.60 ms, DESIGN.md
    // section 4.5)
    const int bwg = t.bsyn_wg >= 0 ? t.bsyn_wg : 2;
    const unsigned grid =
        persistent_grid(a.groups, kBsynWaves, (long long)t.cus * per_cu, bwg, t.stream_grid, k);
    if (!grid) return hipErrorInvalidValue;
    note_kernel("gf_bsyn_kernel<decode,k32m4>");
    // recovered blocks stored non-temporal (B decode 0.655 -> 0.631 ms)
    with_code(k, m, [&](auto I) {
        constexpr CompiledCode c = kCompiledCodes[decltype(I)::value];
        if constexpr (c.syn == Syn::bsyn)
            dispatch_value<3, 5, 7>(D, [&](auto DV) {
                qlaunch((gf_bsyn_kernel<c.k, c.m, kBsynS, decltype(DV)::value, true>), dim3(grid),
                        dim3(kBsynWaves * 64), lds, a.st, a.in, a.out, a.tab, a.cenc, a.slots,
                        a.nout, a.groups, a.rmax, a.out_gstride);
            });
    });
    return hipGetLastError();
}

}  // namespace qfec
