// gf_psyn.h — the gf_psyn_kernel template and its helpers (see gf_psyn.hip for the method).
// Each instantiation object (gf_psyn_<k><m>.hip) includes this header and compiles one
// preset code's variants, so the codes build in parallel.
#pragma once
#include "cauchy_const.h"
#include "compiled_codes.h"
#include "fec_kernels.h"
#include "gf256.h"
#include "gf_bitslice.h"
#include "gf_counted.h"
#include "gf_winjump.h"

namespace qfec {

namespace {

// f(integral_constant<int, v>) for the run-time v in [LO, HI]: a binary tree of uniform
// branches, so register arrays can be indexed by a wave-uniform value
template <int LO, int HI, class F>
__device__ __forceinline__ void psyn_dispatch(int v, F&& f) {
    if constexpr (LO == HI) {
        f(std::integral_constant<int, LO>{});
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (v <= MID) psyn_dispatch<LO, MID>(v, f);
        else psyn_dispatch<MID + 1, HI>(v, f);
    }
}

constexpr int kPsynWaves = 4;   // waves per workgroup (independent)

// KC, MC: the compiled code (k, m); RC = min(k, m): recovered blocks at most; S: sub-row
// bytes; D: blocks in flight per wave.  Each block is read from LDS when its turn comes (the
// other waves of the SIMD cover the LDS latency; no register prefetch: fewer VGPRs, more
// waves).  The solve's run-time products go through two nibble jumps straight into the slot's
// accumulator (gf_winjump.h wz_mul_acc_rt, one call site per slot); recovered blocks are
// stored non-temporal.  (Measured variants: DESIGN.md section 3.7.)
//
// Per-block bookkeeping is kept scalar-light: one buffer resource per GROUP (its 16-byte
// aligned start, bounded by the end of the input), a block is its slot's byte offset added to
// the lanes' DMA offsets (one VALU); and every group issues at least NSTMIN stores (empty-range
// ones pad a group with fewer than 4 recovered blocks), so the wait for a block DMA'd before
// the previous group's stores is always vmcnt(63): no wait ladder over the store count.
// WIDE: each recovered block is staged in LDS as its contiguous bytes and written as three
// 512-byte runs of 8-byte lanes (3 store instructions instead of 8 x SPR); every group then
// issues exactly 3 x RC stores (empty-range ones pad it), so all its waits are exact
// immediates below 63 instead of the vmcnt(63) that over-waits behind > 63 stores.
constexpr int kPsynStage = 1360;   // per-wave staging buffer (WIDE), after the rings
template <int KC, int MC, int RC, int S, int D, bool WIDE = false>
__global__ __launch_bounds__(kPsynWaves * 64) void gf_psyn_kernel(
    const uint8_t* in, uint8_t* out, const uint8_t* __restrict__ tab,
    const uint8_t* __restrict__ cenc, const uint8_t* __restrict__ slots,
    const int32_t* __restrict__ nout, long long groups, int rmax, long long out_gstride) {
    using SH = SubrowShape<S>;
    constexpr int BB = SH::BB, NW = SH::NW, SPR = SH::SPR;
    constexpr int BUFB = SH::BUFB, NPC = SH::NPC, P1L = SH::P1L;
    constexpr int NB = D + 1;                 // the block being read + D in flight
    constexpr int WAITN = D * NPC;            // younger than block b when it is awaited
    constexpr int NSB = 8 * SPR;              // store instructions per recovered block
    constexpr int NSTMIN = 63 - WAITN;        // stores a group issues at least
    constexpr int NSTW = 3 * RC;              // (WIDE) stores a group issues, exactly
    constexpr int WAIT0 = WIDE ? WAITN + NSTW : 63;   // a block DMA'd before the last stores
    static_assert(WAITN <= 63 && D >= 2 && KC >= D, "pipeline depth");
    static_assert(!WIDE || (S == 169 && WAIT0 <= 63), "wide stores: 1352-byte blocks");
    static_assert(KC <= 64 && MC <= 32 && RC <= 16 && RC <= KC && RC <= MC && BB % 8 == 0 &&
                      NB <= 32 && BUFB <= 2048,
                  "compiled small-block code");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int w = wave_id();
    uint8_t* ring = smem + (size_t)w * NB * BUFB;
    const uint32_t stage =   // (WIDE) this wave's staging buffer (LDS address)
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)(
            smem + (size_t)kPsynWaves * NB * BUFB + (size_t)w * kPsynStage);
    const long long W = (long long)gridDim.x * kPsynWaves;
    const long long g0 = (long long)blockIdx.x * kPsynWaves + w;
    if (g0 >= groups) return;
    const int cnt = __builtin_amdgcn_readfirstlane((int)((groups - 1 - g0) / W + 1));
    constexpr long long GB = (long long)KC * BB;
    const long long in_bytes = groups * GB;
    uint32_t v16 = 16u * (uint32_t)__lane_id();   // the lane's 16 bytes of a DMA instruction
    asm volatile("" : "+v"(v16));

    // ---- DMA side: stream block b = position iss_x of group iss_g, the slot the table names
    // there, into ring buffer iss_buf; bit iss_buf of `skew` = its 8-byte skew.  Past the
    // stream's end the last block is re-read (every step issues and waits the same way).
    int iss_buf = 0, iss_x = 0;
    int iss_left = cnt * KC;
    long long iss_g = g0;
    const uint8_t* iss_t = tab + g0 * (long long)psyn::kBytes;
    const long long tstride = W * (long long)psyn::kBytes;
    uint32_t perm_w = 0, skew = 0;
    int iss_sk = 0;                               // the issued group's start mod 16 (0 or 8)
    __amdgpu_buffer_rsrc_t iss_rs;
    auto group_rsrc = [&]() __attribute__((always_inline)) {
        const long long a = iss_g * GB;
        const long long a16 = a & ~15LL;
        iss_sk = (int)(a & 15);
        iss_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(in + a16), 0,
                                                   (unsigned)min(in_bytes - a16, GB + 32), 0x00020000);
    };
    group_rsrc();
    auto issue_next = [&]() __attribute__((always_inline)) {
        if ((iss_x & 3) == 0) perm_w = cload_u32(iss_t, psyn::kPerm + iss_x);
        const int slot = min((int)((perm_w >> (8 * (iss_x & 3))) & 0xFFu), KC - 1);
        const int off = iss_sk + slot * BB;        // the block's offset from the group's 16-B start
        uint32_t vo = v16 + (uint32_t)(off & ~15);
        uint8_t* dst = ring + iss_buf * BUFB;
        dma16(iss_rs, dst, vo);
        if constexpr (NPC == 2)
            if (__lane_id() < P1L) dma16(iss_rs, dst + 1024, vo + 1024u);
        skew = (off & 8) ? (skew | (1u << iss_buf)) : (skew & ~(1u << iss_buf));
        if (++iss_buf == NB) iss_buf = 0;
        if (--iss_left > 0 && ++iss_x == KC) {
            iss_x = 0;
            iss_g += W;
            iss_t += tstride;
            group_rsrc();
        }
    };

#pragma unroll 1
    for (int u = 0; u < D; ++u) issue_next();
    asm volatile("" ::: "memory");
    // the stores a previous group would have issued (empty range): the first group's
    // blocks 0 .. D - 1 are awaited like every other group's
    {
        const __amdgpu_buffer_rsrc_t none = pad_rsrc(out);
#pragma unroll
        for (int q = 0; q < (WIDE ? NSTW : NSTMIN); ++q) pad_store(none, q);
    }
    asm volatile("" ::: "memory");

    int b = 0;        // stream index of the next block to consume
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
        const long long g = g0 + (long long)i * W;
        const uint8_t* tb = tab + g * (long long)psyn::kBytes;
        const uint32_t mlo = cload_u32(tb, psyn::kMask), mhi = cload_u32(tb, psyn::kMask + 4);
        // the syndrome rows the solve uses (the received parity rows); the others are not
        // accumulated (cauchy_256.cpp:712-795: only received recovery rows enter the system)
        const uint32_t need = cload_u32(tb, psyn::kNeed);
        const int n = min(min(nout[g], rmax), RC);
        const int ne = KC - __builtin_popcount(mlo) - __builtin_popcount(mhi);
        int p = 0;    // blocks of this group consumed
        uint32_t acc[MC][8];
#pragma unroll
        for (int y = 0; y < MC; ++y)
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[y][r] = 0;

        // consume block b: issue block b + D, wait for block b (positions 0 .. D - 1 of a group
        // were DMA'd before the previous group's >= NSTMIN stores), read and realign it
        auto take = [&](uint32_t (&wv)[8]) __attribute__((always_inline)) {
            issue_next();
            if (p < D) wait_vmcnt<WAIT0>();
            else wait_vmcnt<WAITN>();
            const int buf = (int)((unsigned)b % NB);
            uint32_t a = 4u * (uint32_t)min((int)__lane_id(), NW - 1) + (uint32_t)(buf * BUFB) +
                         (((skew >> buf) & 1u) << 3);
            asm volatile("" : "+v"(a));   // no hoisting across blocks
            uint32_t lo[8], hi[8];
            read_subrows<S>(ring + a, lo, hi);
            ++b;
            ++p;
#pragma unroll
            for (int t = 0; t < 8; ++t) wv[t] = realign_word<S>(lo, hi, t);
        };
        // data row x (compile time): its block, if present, into every syndrome row
        static_for<KC>([&](auto xc) __attribute__((always_inline)) {
            constexpr int x = decltype(xc)::value;
            // accumulators opaque at every block boundary (no cross-block XOR reassociation)
#pragma unroll
            for (int y = 0; y < MC; ++y)
#pragma unroll
                for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(acc[y][r]));
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t mw = x < 32 ? mlo : mhi;
            if ((mw >> (x & 31)) & 1u) {
                uint32_t wv[8];
                take(wv);
                Win win;
                win_build(wv, win);
                static_for<MC>([&](auto yc) __attribute__((always_inline)) {
                    constexpr int y = decltype(yc)::value;
                    // a uniform branch per row; the empty asm keeps it a branch (no select)
                    if (__builtin_expect((need >> y) & 1u, 1)) {
                        asm volatile("");
                        win_apply<cauchy_coef(MC, y, x)>(acc[y], win);
                    }
                });
            }
        });

        // extras: a received parity row y adds its block to T_y; a repeated data row adds
        // C[y][row] times its block to every T_y (run-time coefficients, cenc = [m][k],
        // one apply into a temporary, then scattered: this path is rare)
#pragma unroll 1
        for (int e = 0; e < ne; ++e) {
            WZ v;
            take(v.W8);
            const int row = cload_u8(tb, psyn::kERow + e);
            if (row >= KC) {
                const int y = row - KC;   // >= MC (255: a no-op extra of an unchanged group)
                if (y < MC)
                    psyn_dispatch<0, MC - 1>(y, [&](auto yc) __attribute__((always_inline)) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) acc[decltype(yc)::value][r] ^= v.W[r];
                    });
            } else {
                expand_wz(v);
#pragma unroll 1
                for (int yy = 0; yy < MC; ++yy) {
                    if (!((need >> yy) & 1u)) continue;
                    const uint32_t cf = (uint32_t)cload_u8(cenc, yy * KC + row);
                    uint32_t tmp[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        tmp[r] = 0;
                        // opaque zero: the dispatch cases must stay in the loop (folded, they
                        // are loop-invariant and ~70 of them would be hoisted into registers)
                        asm volatile("" : "+v"(tmp[r]));
                    }
                    apply_nibble<0>(tmp, cf & 15u, v);
                    apply_nibble<4>(tmp, cf >> 4, v);
                    psyn_dispatch<0, MC - 1>(yy, [&](auto yc) __attribute__((always_inline)) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) acc[decltype(yc)::value][r] ^= tmp[r];
                    });
                }
            }
        }
        if (n > 0) {
            // ---- T_s <- T_{y_s}: ascending, y_s >= s, so no source is overwritten early
            const uint32_t ys0 = cload_u32(tb, psyn::kYs), ys1 = cload_u32(tb, psyn::kYs + 4);
            const uint32_t ys2 = cload_u32(tb, psyn::kYs + 8), ys3 = cload_u32(tb, psyn::kYs + 12);
            static_for<RC>([&](auto sc) __attribute__((always_inline)) {
                constexpr int s = decltype(sc)::value;
                const uint32_t yw = s < 4 ? ys0 : s < 8 ? ys1 : s < 12 ? ys2 : ys3;
                const int y = (int)((yw >> (8 * (s & 3))) & 0xFFu);
                if (s < n && y != s)
                    psyn_dispatch<s, MC - 1>(y, [&](auto yc) __attribute__((always_inline)) {
                        constexpr int yy = decltype(yc)::value;
                        if constexpr (yy != s) {
#pragma unroll
                            for (int r = 0; r < 8; ++r) acc[s][r] = acc[yy][r];
                        }
                    });
            });
            // ---- Gauss-Jordan replay: the pivot row T_p expanded once (W/Z form), then
            // T_i ^= g[p][i] T_p for every slot by two nibble jumps straight into slot i's
            // accumulator (one call site per slot), g[p][p] = 1 ^ inverse pivot
#pragma unroll 1
            for (int pv = 0; pv < n; ++pv) {
                WZ v;
                psyn_dispatch<0, RC - 1>(pv, [&](auto pc) __attribute__((always_inline)) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v.W[r] = acc[decltype(pc)::value][r];
                });
                const int cb = psyn::kCoef + 16 * pv;
                uint32_t cw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) cw[q] = cload_u32(tb, cb + 4 * q);
                expand_wz(v);
                static_for<RC>([&](auto ic) __attribute__((always_inline)) {
                    constexpr int i = decltype(ic)::value;
                    if (i < n) wz_mul_acc_rt(acc[i], v, (cw[i >> 2] >> (8 * (i & 3))) & 0xFFu);
                });
            }
        }

        // ---- stores: recovered block j (data row e_j) into its output slot, NSB store
        // instructions each, non-temporal; a group with fewer than 4 recovered blocks pads to
        // NSTMIN stores with empty-range ones
        asm volatile("" ::: "memory");   // stores stay in issue order among the DMAs
        if constexpr (WIDE) {
            const int ln = (int)__lane_id();
            const uint32_t ra = stage + 8u * (uint32_t)ln;
            static_for<RC>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value;
                if (j < n) {
                    const int oslot = slots ? (int)((cload_u32(slots, (int)((g * rmax + j) & ~3LL)) >>
                                                     (8 * ((g * rmax + j) & 3))) & 0xFFu)
                                            : j;
                    uint8_t* dst = out + g * out_gstride + (long long)oslot * BB;
                    const __amdgpu_buffer_rsrc_t rs =
                        __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
                    if (ln < NW) stage_block_169(stage, acc[j], ln);
                    store_staged_169<2>(rs, ra, ln);
                }
            });
            // pad to exactly NSTW stores (a rolled loop: the barrier per store, gf_counted.h)
            const __amdgpu_buffer_rsrc_t none = pad_rsrc(out);
#pragma unroll 1
            for (int q = 3 * n; q < NSTW; ++q) {
                pad_store(none, q);
                asm volatile("" ::: "memory");
            }
            asm volatile("" ::: "memory");
            continue;
        }
        static_for<RC>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            if (j < n) {
                const int oslot = slots ? (int)((cload_u32(slots, (int)((g * rmax + j) & ~3LL)) >>
                                                 (8 * ((g * rmax + j) & 3))) & 0xFFu)
                                        : j;
                uint8_t* dst = out + g * out_gstride + (long long)oslot * BB;
                const __amdgpu_buffer_rsrc_t rs =
                    __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
                const int ln = (int)__lane_id();
                store_subrows<S, 2>(rs, acc[j], subrow_lanes(ln, ln, NW, SH::NWF));
            }
        });
        static_assert(4 * NSB >= NSTMIN, "four recovered blocks are enough stores");
        if (n < 4) {
            const __amdgpu_buffer_rsrc_t none = pad_rsrc(out);
#pragma unroll
            for (int q = 0; q < NSTMIN; ++q) pad_store(none, q);
        }
        asm volatile("" ::: "memory");
    }
    wait_vmcnt<0>();
}

}  // namespace

constexpr int kPsynS = kCompiledS;   // bb = 1352: 1350-byte payloads

// One code's kernel: ring depth 5, no register prefetch, solve products by nibble jumps,
// non-temporal stores (the other variants measured slower, 3.7).
// The grid is the workgroups one CU holds at once (the runtime's occupancy answer for this
// kernel, cached per kernel: the codes differ in VGPRs) times the CUs.
// Each Syn::psyn row of compiled_codes.h has its instantiation in its own object
// (gf_psyn_<k><m>.hip), declared here, so no other object compiles a gf_psyn_kernel.
template <int K, int M>
hipError_t psyn_go(const Apply& a, size_t lds, bool wide) {
    const Tune& t = *a.t;
    constexpr int RC = K < M ? K : M;
    const auto kern = wide ? gf_psyn_kernel<K, M, RC, kPsynS, 5, true>
                           : gf_psyn_kernel<K, M, RC, kPsynS, 5, false>;
    const unsigned grid = persistent_grid(
        a.groups, kPsynWaves,
        (long long)t.cus * resident_blocks((const void*)kern, kPsynWaves * 64, lds), t.psyn_wg,
        t.stream_grid, a.k);
    if (!grid) return hipErrorInvalidValue;
    note_grid("gf_psyn_kernel", grid);
    qlaunch(kern, dim3(grid), dim3(kPsynWaves * 64), lds, a.st, a.in, a.out, a.tab, a.cenc,
            a.slots, a.nout, a.groups, a.rmax, a.out_gstride);
    return hipGetLastError();
}
extern template hipError_t psyn_go<5, 5>(const Apply&, size_t, bool);
extern template hipError_t psyn_go<10, 10>(const Apply&, size_t, bool);
extern template hipError_t psyn_go<10, 15>(const Apply&, size_t, bool);
extern template hipError_t psyn_go<10, 20>(const Apply&, size_t, bool);
extern template hipError_t psyn_go<15, 15>(const Apply&, size_t, bool);

}  // namespace qfec
