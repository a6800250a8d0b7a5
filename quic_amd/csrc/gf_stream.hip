// gf_stream.hip — m > 1 encode / decode for groups of small blocks (bb <= 2 KiB, one column
// word of each sub-row per lane): the shape of BASELINE configs B and C ((32 + 4) x 1352 B)
// and of every group whose padded packets are at most 2 KiB.
//
// Same arithmetic as gf_apply_kernel (bit-sliced Cauchy code, cauchy_256.cpp:90-125,
// :1502-1601, W/Z nibble expansion of gf_bitslice.h).  What differs is the memory path.
// Reading 169-byte sub-rows with per-lane dword loads tops out at ~4.5 TB/s on MI355X
// (tools/microbench/b_mem_mb.hip, variants a/e), while 1 KiB global_load_lds_dwordx4 pieces
// of whole groups stream at 6.5-6.8 TB/s read-only (tools/microbench/a_ceiling.hip).
//
// Every wave owns whole groups (g0, g0 + W, ...) and streams them through a private LDS
// ring of R one-KiB slots plus a mirror of the first two (a piece DMA'd into slot s < 2 is
// also DMA'd into slot R + s), so any block that starts inside the ring lies contiguous in
// LDS and is read with fixed offsets.  The wave consumes the blocks of a group in order;
// before block x it tops the ring up with the next pieces of its stream (crossing into its
// next group) and waits, with a counted `s_waitcnt vmcnt`, only for the pieces block x
// covers.  No barriers, no cross-wave traffic.  Lane c takes column word c of the 8
// sub-rows of a block as two aligned dwords and v_alignbyte (sub-row t starts t * s bytes
// into the block), expands W/Z and applies the outputs.  The group's outputs are stored
// when its last block is done, through buffer stores whose out-of-range lanes are
// dropped, so the number of VMEM instructions per group is fixed and the vmcnt
// bookkeeping is exact.
//
// vmcnt bookkeeping: `vm` counts every VMEM instruction the wave issued (DMA pieces, their
// mirror copies, stores); lane s of `vmv` holds the value of `vm` at the last instruction
// that wrote slot s.  VMEM instructions retire in issue order, so waiting for
// vmcnt <= vm - 1 - vmv[slot] retires that piece.  No other VMEM instruction may be
// emitted in the loop (coefficients, nout and slots come through s_load); the ISA check
// in tests/test_isa.py guards that.
//
// Decode: per-group coefficients from the decode prep ([G][1][k][RCP]), outputs go to
// slots[g][j] (or j, recovered-blocks layout) and groups with nout == 0 are skipped.  All of
// a group's blocks are in LDS before any of its stores, so in place is safe.
#include "cauchy_const.h"
#include "compiled_codes.h"
#include "fec_kernels.h"
#include "gf_bitslice.h"
#include "gf_counted.h"
#include "gf_winjump.h"

namespace qfec {

constexpr int kStreamWaves = 4;            // waves per workgroup (independent)
constexpr int kMirror = 2;                 // mirrored slots: a block (<= 2 KiB + 3 B of
                                           // over-read) starting in the ring never wraps

// S = sub-row bytes (bb / 8) at compile time, or 0: s_rt at run time (any s <= 256).
// RC = outputs per group (one chunk: m <= RC for encode, rmax <= RC for decode).
// RCPT = byte stride of a coefficient row in the table (max(4, table rc)).  Encode is
// instantiated with RC = m exactly, so the per-output `j < n` test folds away.
// KC > 0 (encode only): the code is fixed, k = KC and m = RC <= 6, and the coefficients come
// from cauchy_const.h at compile time.  The block loop is then fully unrolled and every
// 8x8 bit expansion folds into its straight-line XORs: no coefficient loads and no scalar
// nibble dispatch (about 9 scalar instructions per nibble in the run-time form).
//
// Units: a group's outputs are cut into nchunk chunks of RC (encode m > 8, decode rmax > 8);
// a unit is one (group, chunk) and streams the whole group (the chunks of one group run on
// neighbouring waves, so the re-reads hit L2).  Groups whose byte offset is 8 mod 16 (odd k
// with bb = 8 mod 16: the reference's (5, 5) and (15, 15) presets at 1352-byte blocks) are
// streamed from the 16-byte boundary below them, their blocks 8 bytes into the stream.
// NJ (decode): each run-time product is two nibble jumps straight into its output's
// accumulator (gf_winjump.h wz_mul_acc_rt) instead of two 16-way uniform branch trees.
// WIDE (compiled encode, S = 169): each output block is assembled in a per-wave LDS staging
// buffer (inline-asm ds ops) and written with 3 dwordx2 stores of contiguous bytes instead
// of 8 x (b32 + b8) sub-row stores (the (5, 5) encode).
constexpr int kStreamStage = 1360;
template <int RC, int S, bool DECODE, int RCPT = (RC < 4 ? 4 : RC), int KC = 0, bool NJ = false,
          bool WIDE = false>
__global__ __launch_bounds__(kStreamWaves * 64) void gf_stream_kernel(
    const uint8_t* in, uint8_t* out, const uint8_t* __restrict__ coef,
    const uint8_t* __restrict__ slots, const int32_t* __restrict__ nout, long long groups,
    int k, int m, int rmax, long long coef_gstride, long long out_gstride, int R, int s_rt,
    int nchunk) {
    static_assert(KC == 0 || (!DECODE && RC >= 2 && RC <= 20 && S > 0),
                  "compile-time codes: encode, m <= 6, fixed block size");
    static_assert(S <= 256, "one column word of each sub-row per lane");
    const int s = S ? S : s_rt;                     // sub-row bytes
    const int BB = 8 * s;
    const int NW = (s + 3) >> 2;                    // column words per sub-row
    const int NWF = s >> 2;                         // full words
    constexpr int NCW = RCPT / 4;
    static_assert(RCPT % 4 == 0 && RCPT >= RC, "coefficient row stride");
    // store instructions per sub-row: b32 (full words) + b16 / b8 (the tail word)
    constexpr int SPR = S ? 1 + ((S >> 1) & 1) + (S & 1) : 3;
    constexpr int SAUX = DECODE ? 0 : 2;   // encode's dense parity stream: nt stores
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // the lane id is recomputed where it is used (lane_here): nothing lane-derived stays live
    // across the block loop (register pressure of the compiled encodes with many outputs)
    const int w = wave_id();
    const int RB = R * 1024;
    uint8_t* ring = smem + (size_t)w * (R + kMirror) * 1024;
    static_assert(!WIDE || (S == 169 && !DECODE), "wide stores: 1352-byte encode blocks");
    const uint32_t stage =   // this wave's staging buffer (LDS address), after every wave's ring
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)(
            smem + (size_t)kStreamWaves * (R + kMirror) * 1024 + (size_t)w * kStreamStage);
    const long long W = (long long)gridDim.x * kStreamWaves;
    const long long g0 = (long long)blockIdx.x * kStreamWaves + w;   // the wave's first unit
    const long long NU = groups * nchunk;
    if (g0 >= NU) return;
    const long long cnt =   // wave-uniform, kept in SGPRs (the division runs on the VALU)
        __builtin_amdgcn_readfirstlane((int)((NU - 1 - g0) / W + 1));   // units of this wave
    if constexpr (KC > 0) k = KC;
    const int gb = k * BB;
    const int skew8 = (gb & 15) ? 8 : 0;               // groups may start 8 mod 16
    const int NP = (gb + skew8 + 1023) >> 10;          // pieces per unit
    // column word of a lane (idle lanes shadow the last word)
    auto col_here = [&]() __attribute__((always_inline)) -> int { return min(lane_here(), NW - 1); };

    // ---- issue side (wave-uniform): next piece iss_p of the stream, into slot iss_slot
    int iss_p = 0, iss_slot = 0;
    int issued = 0;                                    // pieces issued
    int vm = 0;                                        // VMEM instructions issued
    uint32_t vmv = 0;                                  // lane s: vm index of slot s's last write
    // the 16-byte aligned start of unit u's group, and its last 16-byte chunk (clamp)
    // A decode unit without output (a group with nothing lost, or a chunk past its losses) is
    // left out of the stream: its group is not read at all.
    const long long u_end = g0 + cnt * W;              // past the wave's last unit
    auto unit_live = [&](long long u) -> bool {
        if constexpr (!DECODE) return true;
        const long long g = u / nchunk;
        return nout[g] - (int)(u - g * nchunk) * RC > 0;
    };
    long long iss_u = g0;
    while (iss_u < u_end && !unit_live(iss_u)) iss_u += W;
    // The loads go through a buffer resource bounded by the end of the input: the last
    // 16-byte chunk of a group whose size is 8 mod 16 reaches 8 bytes past it, which past the
    // last group of the buffer reads as zeros instead of touching unmapped memory.
    const long long in_bytes = groups * (long long)gb;
    auto unit_src = [&](long long u, int& last, unsigned& nrec) -> const uint8_t* {
        const long long a = (u / nchunk) * (long long)gb;
        const int sk = (int)(a & 15);
        last = (sk + gb - 1) & ~15;
        nrec = (unsigned)min(in_bytes - (a - sk), (long long)gb + 32);
        return in + (a - sk);
    };
    int ilast = 0;
    unsigned inrec = 0;
    const uint8_t* isrc = unit_src(iss_u < u_end ? iss_u : g0, ilast, inrec);

    auto issue_one = [&]() {
        const int lane = lane_here();
        const int off = min(iss_p * 1024 + lane * 16, ilast);   // last piece: clamp inside
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)isrc, 0, inrec, 0x00020000);
        dma16(rs, ring + iss_slot * 1024, (uint32_t)off);
        ++vm;
        if (iss_slot < kMirror) {
            dma16(rs, ring + (R + iss_slot) * 1024, (uint32_t)off);
            ++vm;
        }
        vmv = lane == iss_slot ? (uint32_t)(vm - 1) : vmv;
        ++issued;
        if (++iss_slot == R) iss_slot = 0;
        if (++iss_p == NP) {
            iss_p = 0;
            do {
                iss_u += W;
            } while (iss_u < u_end && !unit_live(iss_u));
            isrc = unit_src(iss_u, ilast, inrec);
        }
    };
    // top the ring up: every piece from `head` on stays, the rest of the R slots refill
    auto fill = [&](int head) {
        while (iss_u < u_end && issued - head < R) issue_one();
    };
    // wait until the block at ring position bp has landed (its last piece retired)
    auto wait_block = [&](uint32_t bp) {
        int sl = (int)((bp + BB - 1) >> 10);
        sl = sl >= R ? sl - R : sl;
        const int idx = __builtin_amdgcn_readlane((int)vmv, sl);
        const int pending = vm - 1 - idx;
        // coarse steps (a smaller count only waits longer): 4 scalar branch levels
        if (pending >= 16) {
            if (pending >= 32) {
                if (pending >= 48) wait_vmcnt<48>();
                else wait_vmcnt<32>();
            } else {
                if (pending >= 24) wait_vmcnt<24>();
                else wait_vmcnt<16>();
            }
        } else {
            wait_vmcnt_upto<0, 15>(pending < 0 ? 0 : pending);
        }
    };
    // column word c of the 8 sub-rows as aligned dword pairs (block starts are 8-byte
    // aligned in the ring: slots are 1 KiB and BB % 8 == 0; sub-row t is misaligned by
    // (t * s) & 3, realigned with v_alignbyte at use).  The block lies contiguous in
    // [bp, bp + BB + 3] thanks to the mirror.
    auto read_block = [&](uint32_t bp, uint32_t (&lo)[8], uint32_t (&hi)[8]) {
        // the lane's byte offset, opaque to the optimiser: in the fully unrolled (KC > 0)
        // form it would otherwise precompute every block's addresses up front
        uint32_t c4 = 4u * (uint32_t)col_here();
        if constexpr (KC > 0) asm volatile("" : "+v"(c4));
        read_subrows<S>(ring + bp + c4, lo, hi, s);
    };
    auto next_pos = [&](uint32_t bp) -> uint32_t {
        bp += BB;
        return bp >= (uint32_t)RB ? bp - (uint32_t)RB : bp;
    };

    // ---- consume side
    int gbase = 0;                                     // first piece of the current group
    int gslot0 = 0;                                    // its slot
#pragma unroll 1
    for (long long i = 0; i < cnt; ++i) {
        const long long u = g0 + i * W;
        const long long g = u / nchunk;
        const int ch = (int)(u - g * nchunk);            // output chunk: outputs ch * RC + j
        const int sk = (int)((g * gb) & 15);             // the group's bytes start sk into its stream
        int n = (DECODE ? nout[g] : m) - ch * RC;
        n = n > RC ? RC : n;
        if (n > 0) {
            const uint32_t* cw = (const uint32_t*)(coef + (DECODE ? g * coef_gstride : 0) +
                                                   (long long)ch * k * RCPT);
            uint32_t acc[RC][8];
#pragma unroll
            for (int j = 0; j < RC; ++j)
#pragma unroll
                for (int r = 0; r < 8; ++r) acc[j][r] = 0;
            // Block x + 1's LDS reads are issued before block x is combined (software
            // pipeline); the ring keeps every piece from block x's first on, so block x's
            // pieces are not refilled while its reads may still be in flight.
            uint32_t bpos = (uint32_t)gslot0 * 1024u + (uint32_t)sk;   // ring position of block x
            uint32_t lo0[8], hi0[8], lo1[8], hi1[8];
            fill(gbase);
            wait_block(bpos);
            read_block(bpos, lo0, hi0);
            // xc: the block index, an int or (KC > 0) an integral_constant
            // run-time coefficients two blocks ahead: the scalar load for block x + 2 is
            // issued while block x is combined, so its latency is hidden
            uint32_t cA[NCW], cB[NCW];
            if constexpr (KC == 0) {
#pragma unroll
                for (int q = 0; q < NCW; ++q) {
                    cA[q] = cw[q];
                    cB[q] = cw[(k > 1 ? 1 : 0) * NCW + q];
                }
            }
            auto step = [&](auto xc, uint32_t (&lo)[8], uint32_t (&hi)[8],
                            uint32_t (&nlo)[8], uint32_t (&nhi)[8], uint32_t (&cc)[NCW]) {
                const int x = xc;
                const uint32_t bn = next_pos(bpos);
                if (x + 1 < k) {
                    fill(gbase + ((sk + x * BB) >> 10));
                    wait_block(bn);
                    read_block(bn, nlo, nhi);
                }
                bpos = bn;
                WZ v;
#pragma unroll
                for (int t = 0; t < 8; ++t) v.W[t] = realign_word<S>(lo, hi, t, s);
                if constexpr (KC > 0) {
                    // windowed form (gf_bitslice.h): one v_bitop3 per (output, sub-row); row 0
                    // is P0, all coefficients 1 (cauchy_256.cpp:1519-1523)
                    Win win;
                    win_build(v.W8, win);
                    static_for<RC>([&](auto jc) __attribute__((always_inline)) {
                        constexpr int j = decltype(jc)::value;
                        win_apply<cauchy_coef(RC, j, decltype(xc)::value)>(acc[j], win);
                    });
                    return;
                }
                uint32_t cwv[NCW];
                const int xn = x + 2 < k ? x + 2 : k - 1;
#pragma unroll
                for (int q = 0; q < NCW; ++q) {
                    cwv[q] = cc[q];
                    cc[q] = cw[xn * NCW + q];
                }
                expand_wz(v);
#pragma unroll
                for (int j = 0; j < RC; ++j) {
                    if (!DECODE && j == 0 && ch == 0) {
                        // encode row 0 is P0, all coefficients 1 (cauchy_256.cpp:1519-1523):
                        // a plain XOR, no scalar nibble dispatch
#pragma unroll
                        for (int r = 0; r < 8; ++r) acc[0][r] ^= v.W[r];
                    } else if (j < n) {
                        const uint32_t cf = (cwv[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                        if constexpr (NJ) {
                            wz_mul_acc_rt(acc[j], v, cf);
                        } else {
                            apply_nibble<0>(acc[j], cf & 15u, v);
                            apply_nibble<4>(acc[j], cf >> 4, v);
                        }
                    }
                }
            };
            if constexpr (KC > 0) {
                // the block loop inline, not through a lambda (the fully unrolled 250-block
                // loop of (250, 5) spills to scratch through one)
                static_for<KC>([&](auto xc) {
                    // the accumulators are opaque at every block boundary: with all
                    // coefficients constant, the XOR reassociation would otherwise flatten the
                    // blocks' sums into one tree and keep every block's W/Z live (~490 VGPRs)
#pragma unroll
                    for (int j = 0; j < RC; ++j)
#pragma unroll
                        for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(acc[j][r]));
                    if constexpr (decltype(xc)::value % 2 == 0)
                        step(xc, lo0, hi0, lo1, hi1, cA);
                    else
                        step(xc, lo1, hi1, lo0, hi0, cB);
                });
            } else {
#pragma unroll 1
                for (int x = 0; x < k; x += 2) {
                    step(x, lo0, hi0, lo1, hi1, cA);
                    if (x + 1 < k) step(x + 1, lo1, hi1, lo0, hi0, cB);
                }
            }
            asm volatile("" ::: "memory");   // stores stay in issue order among the DMAs
            // ---- outputs: fixed instruction count per output (dropped lanes, no branches).
            // Lane offsets 4c (full words) and the tail lane's, sub-row in the scalar offset:
            // two address VGPRs, opaque so they are not hoisted as 8 x RC precomputed ones
            // (subrow_lanes() spelled out: with run-time s its form compiles to other code).
            const int lane = lane_here(), c = min(lane, NW - 1);
            uint32_t vo = lane < NWF ? 4u * (uint32_t)c : kLaneDrop;
            uint32_t vt = lane == NWF && NWF < NW ? 4u * (uint32_t)c : kLaneDrop;
            asm volatile("" : "+v"(vo), "+v"(vt));
            const SubrowLanes sl{vo, vt};
            if constexpr (WIDE) {
                const uint32_t ra = stage + 8u * (uint32_t)lane;
#pragma unroll
                for (int j = 0; j < RC; ++j) {
                    const int jo = ch * RC + j;
                    uint8_t* dst = out + g * out_gstride + (long long)jo * BB;
                    const __amdgpu_buffer_rsrc_t rs =
                        __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
                    if (lane < NW) stage_block_169(stage, acc[j], lane);
                    store_staged_169<SAUX>(rs, ra, lane);
                    vm += 3;
                }
                asm volatile("" ::: "memory");
                gbase += NP;
                gslot0 = (gslot0 + NP) % R;
                continue;
            }
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                if (j < n) {
                    const int jo = ch * RC + j;
                    const int oslot = (DECODE && slots) ? cload_u8(slots, g * rmax + jo) : jo;
                    uint8_t* dst = out + g * out_gstride + (long long)oslot * BB;
                    const __amdgpu_buffer_rsrc_t rs =
                        __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
#pragma unroll
                    for (int r = 0; r < 8; ++r) store_subrow<S, SAUX>(rs, acc[j][r], r, sl, s);
                    vm += 8 * SPR;
                }
            }
            asm volatile("" ::: "memory");
            gbase += NP;                                 // units without output stream nothing
            gslot0 = (gslot0 + NP) % R;
        }
    }
    wait_vmcnt<0>();
}

// ------------------------------------------------------------------ static ring
// gf_ring_kernel: the same stream for one FIXED shape (k = K blocks of 8 * S bytes: the
// BASELINE B/C groups, (32 + 4) x 1352 B), with the whole per-group schedule known at
// compile time.  A group is NP one-KiB pieces; piece n of a wave's stream lands in ring slot
// (phase + n) mod R, phase = the group's first slot (advances by NP mod R per group).
// Before block x's compute the ring holds every piece from block x's first one on and is
// filled up to F(x) = pf(x) + R - 1 (the next group's first pieces included), so the number
// of pieces per step, and the count of VMEM instructions younger than the next block's
// last piece (plus the previous group's fixed-count stores where they sit in between), are
// constants: every wait is an immediate `s_waitcnt vmcnt`, with no run-time bookkeeping.
// The stream's ends are made regular too: the first group finds NST dummy stores (empty
// buffer range) where a previous group's stores would be, and the last group issues
// dummy pieces (a reread of its own last piece) for the group that does not follow.
// No mirror: a block that wraps round the ring end (uniform test) is read with per-lane
// wrapped addresses.
constexpr int kRingWaves = 4;

// SK: the group's bytes start SK bytes into its stream (odd k at 1352-byte blocks: groups
// alternate between 0 and 8 bytes past a 16-byte boundary)
template <int S, int SK = 0>
struct RingShape : SubrowShape<S> {
    static constexpr int R = 8, RB = R * 1024;
    static constexpr int BB = SubrowShape<S>::BB;
    static constexpr int pf(int x) { return (SK + x * BB) >> 10; }             // first piece of block x
    static constexpr int pl(int x) { return (SK + (x + 1) * BB - 1) >> 10; }   // its last piece
};

// Encode only: the coefficients are cauchy_const.h's at compile time, every group stores its RC
// parity rows.  (The rolled run-time-coefficient decode this schedule once carried measured
// slower than gf_stream_kernel's, DESIGN.md section 3.3, and is gone.)
// NT: the parity stores are non-temporal.  SK: see RingShape.
// A group whose size is 8 mod 16 is streamed as GBS = GB + 8 bytes from the 16-byte boundary
// at or below its start; the loads then go through a buffer resource bounded by the end of
// the input (the last group's stream may end 8 bytes past it: those lanes read zeros).
// NCH > 1: a group's MC parity rows are NCH chunks of RC rows, one unit each; unit
// u = NCH * g + ch, and a wave's units u0, u0 + W, ... (W a multiple of NCH) all have chunk
// Y0 / RC = u0 % NCH, so the chunk's rows are compile-time; the NCH units of a group run on
// neighbouring waves, whose reads of the group meet in L2.
template <int K, int S, int RC, int MC, bool NT, int SK, bool WIDE, int NCH = 1, int Y0 = 0>
__device__ __forceinline__ void gf_ring_run(const uint8_t* in, uint8_t* out, long long groups,
                                            long long out_gstride, uint8_t* smem) {
    using SH = RingShape<S, SK>;
    constexpr int R = SH::R, RB = SH::RB, BB = SH::BB, NW = SH::NW;
    constexpr int GB = K * BB;
    constexpr bool SKEW = GB % 16 != 0;
    constexpr int GBS = (GB + 15) / 16 * 16;              // stream bytes per group
    constexpr int NP = (GBS + 1023) / 1024;
    static_assert(SKEW ? GB % 16 == 8 : SK == 0, "groups 0 or 8 bytes off 16");
    // stores per group, fixed: 8 sub-rows x SPR per output, or (WIDE) 3 runs of 512 bytes
    constexpr int NST = WIDE ? RC * 3 : RC * 8 * SH::SPR;
    static_assert(!WIDE || S == 169, "wide stores: 1352-byte blocks");
    constexpr int SAUX = NT ? 2 : 0;                      // the parity stream: nt
    constexpr int FM1 = SH::pf(K - 1) + R - 1 - NP;       // next-group pieces issued early
    static_assert(MC == RC * NCH, "one output per register set");
    static_assert(NCH == 1 || (Y0 % RC == 0 && Y0 < MC), "chunked encode");
    static_assert(FM1 >= SH::pl(0), "block 0 of the next group is prefetched in full");
    static_assert(SH::pf(K - 1) + R - 1 < 2 * NP, "the frontier stays within the next group");
    const int lane = threadIdx.x & 63;
    const int w = wave_id();
    uint8_t* ring = smem + (size_t)w * RB;
    const uint32_t stage =   // (WIDE) this wave's staging buffer (LDS address), after the rings
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)(
            smem + (size_t)kRingWaves * RB + (size_t)w * kStreamStage);
    const long long W = (long long)gridDim.x * kRingWaves / NCH;   // group stride of the wave
    const long long g0 = ((long long)blockIdx.x * kRingWaves + w) / NCH;
    if (g0 >= groups) return;
    const long long cnt =   // wave-uniform, kept in SGPRs (the division runs on the VALU)
        __builtin_amdgcn_readfirstlane((int)((groups - 1 - g0) / W + 1));      // groups of this wave
    const int c = lane < NW ? lane : NW - 1;              // idle lanes shadow the last word
    const long long gstep = W * GB;

    const uint8_t* gsrc = in + g0 * GB - SK;              // current group's stream
    const uint8_t* in_end = in + groups * GB;
    int phase = 0;                                        // ring slot of its piece 0
    long long i = 0;                                      // current group

    // piece p of the stream that starts at src into ring slot `slot`.  The skewed form puts
    // the piece's offset into the descriptor's base (the range check then bounds the piece,
    // and the lane offsets are two loop-invariant VGPRs instead of one per piece)
    const uint32_t v16 = 16u * (uint32_t)lane;
    const uint32_t vlast = min(16u * (uint32_t)lane, (uint32_t)(GBS - 16 - (NP - 1) * 1024));
    // non-temporal loads, but default policy when a group's chunks are read by NCH waves
    // (the sibling's reads then hit the lines in L2)
    constexpr int LAUX = NCH > 1 ? 0 : 2;
    auto dma = [&](const uint8_t* src, int p, int slot) __attribute__((always_inline)) {
        if constexpr (SKEW) {
            const uint8_t* b = src + p * 1024;
            const long long left = in_end - b;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)b, 0, (unsigned)(left < 1024 ? left : 1024), 0x00020000);
            dma16<LAUX>(rs, ring + slot * 1024, p == NP - 1 ? vlast : v16);
        } else {
            const int off = min(p * 1024 + lane * 16, GBS - 16);
            __builtin_amdgcn_global_load_lds(QF_GPTR(src + off), QF_LPTR(ring + slot * 1024), 16,
                                             0, LAUX);
        }
    };

    // piece n of the current group (n >= NP: piece n - NP of the next, or a dummy reread
    // of the current group's last piece when there is no next group)
    auto issue = [&](auto nc) __attribute__((always_inline)) {
        constexpr int n = decltype(nc)::value;
        if constexpr (n < NP) {
            dma(gsrc, n, (phase + n) & (R - 1));
        } else {
            const bool next = i + 1 < cnt;
            dma(next ? gsrc + gstep : gsrc, next ? n - NP : NP - 1, (phase + n) & (R - 1));
        }
    };
    // block x (compile time) at ring byte (phase * 1024 + x * BB) mod RB
    auto read_block = [&](auto xc, uint32_t (&lo)[8], uint32_t (&hi)[8])
                          __attribute__((always_inline)) {
        const int x = xc;
        uint32_t c4 = 4u * (uint32_t)c;
        asm volatile("" : "+v"(c4));   // opaque: addresses are not hoisted across blocks
        uint32_t bp = ((uint32_t)phase * 1024u + (uint32_t)(SK + x * BB)) & (uint32_t)(RB - 1);
        if (bp + (uint32_t)BB + 4u <= (uint32_t)RB) {
            read_subrows<S>(ring + bp + c4, lo, hi);
        } else {
            const uint32_t base = bp + c4;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int o = t * S;
                const uint32_t a0 = base + (uint32_t)(o & ~3);
                lo[t] = *(const uint32_t*)(ring + min(a0, a0 - (uint32_t)RB));
                if (o & 3) {
                    const uint32_t a1 = a0 + 4u;
                    hi[t] = *(const uint32_t*)(ring + min(a1, a1 - (uint32_t)RB));
                } else {
                    hi[t] = 0u;
                }
            }
        }
    };

    // ---- prologue: the first group's early pieces, then the stores a previous group
    // would have issued (dropped: empty range), so every group sees the same VMEM history
    static_for<FM1 + 1>([&](auto nc) __attribute__((always_inline)) { issue(nc); });
    // The waits count VMEM instructions in issue order: the compiler must not move a
    // buffer store across a DMA (it may: they touch different memory).
    asm volatile("" ::: "memory");
    {
        const __amdgpu_buffer_rsrc_t none = pad_rsrc(out);
#pragma unroll
        for (int q = 0; q < NST; ++q) pad_store(none, q);
    }

    uint32_t lo0[8], hi0[8], lo1[8], hi1[8];
#pragma unroll 1
    for (; i < cnt; ++i) {
        const long long g = g0 + i * W;
        uint32_t acc[RC][8];
#pragma unroll
        for (int j = 0; j < RC; ++j)
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[j][r] = 0;
        // block 0: its pieces were issued before the previous group's stores
        wait_vmcnt<(FM1 - SH::pl(0) + NST > 63 ? 63 : FM1 - SH::pl(0) + NST)>();
        read_block(std::integral_constant<int, 0>{}, lo0, hi0);

        auto step = [&](auto xc, uint32_t (&lo)[8], uint32_t (&hi)[8], uint32_t (&nlo)[8],
                        uint32_t (&nhi)[8]) __attribute__((always_inline)) {
            constexpr int x = decltype(xc)::value;
            constexpr int F0 = x == 0 ? FM1 : SH::pf(x - 1) + R - 1;   // frontier before
            constexpr int F1 = SH::pf(x) + R - 1;                       // and after this step
            static_for<F1 - F0>([&](auto qc) __attribute__((always_inline)) {
                issue(std::integral_constant<int, F0 + 1 + decltype(qc)::value>{});
            });
            if constexpr (x + 1 < K) {
                constexpr int pl1 = SH::pl(x + 1);
                constexpr int yng = F1 - pl1 + (pl1 <= FM1 ? NST : 0);
                wait_vmcnt<(yng > 63 ? 63 : yng)>();
                read_block(std::integral_constant<int, x + 1>{}, nlo, nhi);
            }
            WZ v;
#pragma unroll
            for (int t = 0; t < 8; ++t) v.W[t] = realign_word<S>(lo, hi, t);
            Win win;
            win_build(v.W8, win);
            static_for<RC>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value;
                win_apply<cauchy_coef(MC, Y0 + j, x)>(acc[j], win);
            });
        };
        static_for<K>([&](auto xc) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < RC; ++j)
#pragma unroll
                for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(acc[j][r]));
            if constexpr (decltype(xc)::value % 2 == 0) step(xc, lo0, hi0, lo1, hi1);
            else step(xc, lo1, hi1, lo0, hi0);
        });

        // ---- outputs: NST store instructions, kept after the last step's DMAs and before the
        // next group's (issue order)
        asm volatile("" ::: "memory");
        if constexpr (WIDE) {
            const uint32_t ra = stage + 8u * (uint32_t)lane;
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                uint8_t* dst = out + g * out_gstride + (long long)(Y0 + j) * BB;
                const __amdgpu_buffer_rsrc_t rs =
                    __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
                if (lane < NW) stage_block_169(stage, acc[j], lane);
                store_staged_169<SAUX>(rs, ra, lane);
            }
        } else {
            const SubrowLanes sl = subrow_lanes(lane, c, NW, SH::NWF);
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                uint8_t* dst = out + g * out_gstride + (long long)(Y0 + j) * BB;
                const __amdgpu_buffer_rsrc_t rs =
                    __builtin_amdgcn_make_buffer_rsrc(dst, 0, (unsigned)BB, 0x00020000);
#pragma unroll
                for (int r = 0; r < 8; ++r) store_subrow<S, SAUX>(rs, acc[j][r], r, sl);
            }
        }
        asm volatile("" ::: "memory");
        gsrc += gstep;
        phase = (phase + NP) & (R - 1);
    }
    wait_vmcnt<0>();
}

#ifndef QF_RING_SKEW_INLINE
#define QF_RING_SKEW_INLINE __forceinline__
#endif
#ifndef QF_RING_ATTR
#define QF_RING_ATTR
#endif
template <int K, int S, int RC, int MC, bool NT, bool WIDE, int NCH, int Y0>
__device__ QF_RING_SKEW_INLINE void gf_ring_skew(const uint8_t* in, uint8_t* out, long long groups,
                                                 long long out_gstride, uint8_t* smem) {
    if constexpr ((K * 8 * S) % 16 == 0) {
        gf_ring_run<K, S, RC, MC, NT, 0, WIDE, NCH, Y0>(in, out, groups, out_gstride, smem);
    } else {
        // group g starts 8 * (g & 1) bytes past a 16-byte boundary; a wave's groups g0,
        // g0 + W, ... (W = 4 x the grid / NCH, even) all share g0's skew
        const long long g0 = ((long long)blockIdx.x * kRingWaves + wave_id()) / NCH;
        if (g0 & 1)
            gf_ring_run<K, S, RC, MC, NT, 8, WIDE, NCH, Y0>(in, out, groups, out_gstride, smem);
        else
            gf_ring_run<K, S, RC, MC, NT, 0, WIDE, NCH, Y0>(in, out, groups, out_gstride, smem);
    }
}

// NCH: parity-row chunks per group (RC = MC / NCH rows each, chunk = the wave's unit index
// mod NCH).  DECODE is always false: the bench's counter summaries tell encode from decode
// kernels by this template argument's position, so it stays.  The arguments between `out` and
// `groups`, and rmax and coef_gstride, are the common launch signature; the encode reads none.
template <int K, int S, int RC, bool DECODE, int MC, bool NT = true, bool WIDE = false, int NCH = 1>
__global__ __launch_bounds__(kRingWaves * 64) QF_RING_ATTR void gf_ring_kernel(
    const uint8_t* in, uint8_t* out, const uint8_t* __restrict__ coef,
    const uint8_t* __restrict__ slots, const int32_t* __restrict__ nout, long long groups,
    int rmax, long long coef_gstride, long long out_gstride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    static_assert(!DECODE, "the static ring schedule is an encode");
    static_assert(NCH == 1 || NCH == 2, "one or two chunks");
    if constexpr (NCH == 1) {
        gf_ring_skew<K, S, RC, MC, NT, WIDE, 1, 0>(in, out, groups, out_gstride, smem);
    } else {
        if ((blockIdx.x * kRingWaves + wave_id()) & 1)
            gf_ring_skew<K, S, RC, MC, NT, WIDE, 2, RC>(in, out, groups, out_gstride, smem);
        else
            gf_ring_skew<K, S, RC, MC, NT, WIDE, 2, 0>(in, out, groups, out_gstride, smem);
    }
}

// Ring slots the stream needs: before block x's compute the ring keeps every piece from
// block x's first on, and block x + 1 must land in it too.  Blocks x and x + 1 span
// (o + 2 * bb + 1023) / 1024 pieces from block x's head piece, o its start offset in that
// piece; o is a multiple of gcd(bb, 1024), so at most 1024 - gcd(bb, 1024).
int gf_stream_min_ring(int bb) {
    int a = bb, b = 1024;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    const int max_o = 1024 - a;
    return (max_o + 2 * bb + 1023) / 1024;
}

bool gf_stream_supported(int k, int bb, int rc, const Tune& t) {
    if (!t.stream) return false;
    if (bb % 8 != 0 || bb < 8 || bb > 2048) return false;   // s <= 256: a word per lane
    if (rc != 2 && rc != 4 && rc != 8 && rc != 16) return false;
    if ((long long)k * bb < 16) return false;   // groups 8 mod 16 apart stream skewed
    if (t.stream_ring < gf_stream_min_ring(bb)) return false;   // gf_apply instead
    return true;
}

int stream_encode_rc(int k, int m, int bb, bool aligned, const Tune& t) {
    if (m > 8 && m <= 16 && aligned && gf_stream_supported(k, bb, 16, t)) return 16;
    return encode_rc(m, t);
}

#ifndef QF_KERNELS_ONLY   // (register-use experiments compile single instantiations)
hipError_t launch_gf_stream(const Apply& a, bool decode) {
    const Tune& t = *a.t;
    const int k = a.k, m = a.m, bb = a.bb, rc = a.rc;
    const long long groups = a.groups;
    if (groups <= 0) return hipSuccess;
    if (!gf_stream_supported(k, bb, rc, t)) return hipErrorInvalidValue;
    if (((uintptr_t)a.in & 15) != 0 || ((uintptr_t)a.slots & 3) != 0) return hipErrorInvalidValue;
    const int R = t.stream_ring;
    if (R < 4 || R > 36) return hipErrorInvalidValue;
    const int s = bb / 8;
    // the row of a compiled encode (BASELINE configs B/C and the QuicR presets at 1350-byte
    // payloads): the code is fixed at compile time and no table is read
    const CompiledCode* const code =
        !decode && t.const_enc && s == kCompiledS ? find_code(k, m) : nullptr;
    const bool out8 = (((uintptr_t)a.out | (uintptr_t)a.out_gstride) & 7) == 0;
    // wide (LDS-staged 8-byte) parity stores: measured faster only for the (5, 5) encode
    // (0.203 -> 0.180 ms; within +-5 % on the other presets)
    const bool wide_enc = code && code->stream_wide && out8;
    const size_t lds = (size_t)kStreamWaves * ((R + kMirror) * 1024 + (wide_enc ? kStreamStage : 0));
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int per_cu = lds_blocks_per_cu(lds);
    // units: (group, chunk of outputs).  Decode: chunks of rc for rmax > rc.  A compiled encode:
    // one unit.  A table encode: the table is the one stream_encode_rc() asks for (rows of
    // max(4, rc) bytes), and a unit is every output where they fit its rows, else a chunk of 8
    int nchunk = 1, enc_rc = 0;
    if (decode) {
        nchunk = (a.rmax + rc - 1) / rc;
    } else if (!code) {
        enc_rc = stream_encode_rc(k, m, bb, true, t);
        if (std::max(rc, 4) != std::max(enc_rc, 4) || (m > enc_rc && enc_rc != 8))
            return hipErrorInvalidValue;
        if (m > enc_rc) nchunk = (m + 7) / 8;
    }
    const long long units = groups * nchunk;
    // oversubscribed: about swg units per wave ((250, 5) decode 5.02 -> 4.36 ms, DESIGN.md
    // section 4.5); large groups only by default
    const int swg = t.stream_wg >= 0 ? t.stream_wg : ((long long)k * bb >= 65536 ? 1 : 0);
    // the wave's 32-bit piece counter counts cnt * NP pieces
    const unsigned grid =
        persistent_grid(units, kStreamWaves, (long long)t.cus * per_cu, swg, t.stream_grid,
                        ((long long)k * bb + 8 + 1023) / 1024);
    if (!grid) return hipErrorInvalidValue;
    // the static ring schedule is an encode only: a rolled decode on it measured slower than
    // gf_stream's (0.644 vs 0.619 ms on config B)
    if (code && t.stream_static) {
        // compile-time ring schedule (gf_ring_kernel).  Wide (LDS-staged 8-byte) parity stores:
        // 3 store instructions per block instead of 16, so the group's store count stays under
        // the 63 a counted wait can name.  Which rows take them, and which split a group into
        // two units of m / 2 parity rows (half the accumulators per wave, so wide stores fit
        // the registers): compiled_codes.h, DESIGN.md section 3.3
        const bool rsplit = t.ring_split && code->ring_split;
        const bool rwide = t.ring_wide && (rsplit || code->ring_wide) && out8;
        const size_t rlds = (size_t)kRingWaves * (RingShape<kCompiledS>::RB + (rwide ? kStreamStage : 0));
        // oversubscribed: about rwg units per wave; measured faster for some of these encodes
        // (B 0.58 -> 0.55 ms, (10,10) 0.361 -> 0.330; (10,20) and (15,15) no better,
        // DESIGN.md section 4.5)
        const int rwg = t.ring_wg >= 0 ? t.ring_wg : code->ring_wg;
        const unsigned rgrid = persistent_grid(groups * (rsplit ? 2 : 1), kRingWaves,
                                               (long long)t.cus * lds_blocks_per_cu(rlds), rwg,
                                               t.stream_grid);
        if (!rgrid) return hipErrorInvalidValue;
        char name[64];
        snprintf(name, sizeof name, "gf_ring_kernel<encode,k%dm%d%s>", k, m, rsplit ? ",split" : "");
        note_kernel(name);
        const auto go = [&](auto kern) {
            qlaunch(kern, dim3(rgrid), dim3(kRingWaves * 64), rlds, a.st, a.in, a.out, a.tab,
                    a.slots, a.nout, groups, a.rmax, a.tab_gstride, a.out_gstride);
        };
        // nt parity stores (plain: 0.673 vs 0.578 ms on B)
        with_code(k, m, [&](auto I) {
            constexpr CompiledCode c = kCompiledCodes[decltype(I)::value];
            if constexpr (c.ring_split) {
                if (rsplit) {
                    if (rwide) go(gf_ring_kernel<c.k, kCompiledS, c.m / 2, false, c.m, true, true, 2>);
                    else go(gf_ring_kernel<c.k, kCompiledS, c.m / 2, false, c.m, true, false, 2>);
                    return;
                }
            }
            if constexpr (c.ring_wide) {
                if (rwide) {
                    go(gf_ring_kernel<c.k, kCompiledS, c.m, false, c.m, true, true>);
                    return;
                }
            }
            go(gf_ring_kernel<c.k, kCompiledS, c.m, false, c.m, true, false>);
        });
        return hipGetLastError();
    }
    const unsigned threads = kStreamWaves * 64;
    const auto go = [&](auto kern) {
        qlaunch(kern, dim3(grid), dim3(threads), lds, a.st, a.in, a.out, a.tab, a.slots, a.nout,
                groups, k, m, a.rmax, a.tab_gstride, a.out_gstride, R, s, nchunk);
    };
    if (code) {
        // windowed form, every output in one unit
        note_kernel("gf_stream_kernel<encode,compiled>");
        with_code(k, m, [&](auto I) {
            constexpr CompiledCode c = kCompiledCodes[decltype(I)::value];
            if constexpr (c.stream_wide) {
                if (wide_enc) {
                    go(gf_stream_kernel<c.m, kCompiledS, false, c.rcpt(), c.k, false, true>);
                    return;
                }
            }
            go(gf_stream_kernel<c.m, kCompiledS, false, c.rcpt(), c.k>);
        });
        return hipGetLastError();
    }
    // S at compile time for 1352-byte blocks, else s at run time
    bool ok = true;
    dispatch_bool(s == kCompiledS, [&](auto fixed) {
        constexpr int sv = decltype(fixed)::value ? kCompiledS : 0;
        if (decode) {
            // nibble jumps (NJ) where S is fixed
            note_kernel(sv ? "gf_stream_kernel<decode>" : "gf_stream_kernel<decode,s>");
            ok = dispatch_value<2, 4, 8>(rc, [&](auto RC) {
                constexpr int rcv = decltype(RC)::value;
                go(gf_stream_kernel<rcv, sv, true, (rcv <= 4 ? 4 : 8), 0, sv != 0>);
            });
            return;
        }
        note_kernel(sv ? "gf_stream_kernel<encode>" : "gf_stream_kernel<encode,s>");
        if (enc_rc == 16) {   // one unit of up to 16 outputs (table rows of 16)
            go(gf_stream_kernel<16, sv, false, 16, 0>);
            return;
        }
        // one output per register set, RC = m; chunks of 8 (and any other m) run RC = 8
        const auto enc = [&](auto RC) {
            constexpr int rcv = decltype(RC)::value;
            go(gf_stream_kernel<rcv, sv, false, (rcv <= 4 ? 4 : 8), 0>);
        };
        if (!dispatch_value<2, 3, 4, 5, 6, 7, 8>(m, enc)) enc(std::integral_constant<int, 8>{});
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

#endif
}  // namespace qfec
