// gf_ragged_unit.h — what the run-time-shape kernel families share: the packed ragged batches
// (gf_ragged.hip) and the pointer-table batches (gf_ptrs.hip).  The two differ only in where a
// group's blocks lie, so the (group, chunk) unit is written once over a block addressing:
//   PackedIn / PackedOut   block pos at base + pos * bb (the packed layout)
//   TableIn / TableOut     block pos at the address a device table names (gf_ptrs.hip)
#pragma once
#include "fec_kernels.h"
#include "gf256.h"
#include "gf_bitslice.h"
#include "gf_colword.h"

namespace qfec {

// Logical workgroup of hardware block b: consecutive logical workgroups run on one XCD (the
// bijection of gf_apply_kernel), so the chunks of one group share an L2.
__device__ __forceinline__ unsigned xcd_logical_block() {
    const unsigned nbk = gridDim.x, b = blockIdx.x, xcd = b & 7u, q8 = nbk >> 3, r8 = nbk & 7u;
    return xcd * q8 + (xcd < r8 ? xcd : r8) + (b >> 3);
}

// A wave-uniform 64-bit value the compiler may not see as uniform (loaded per group): keep
// it in scalar registers.
__device__ __forceinline__ long long uniform64(long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// Blocks in flight per wave while one is combined, as gf_apply_kernel (PD = 2).
constexpr int kRaggedPD = 2;

// The packed layout: the address of a block follows from its position.
struct PackedIn {
    const uint8_t* gin;
    int bb;
    __device__ __forceinline__ void start(int) {}
    // the address of block `pos`, asked for slot u of the pipeline
    __device__ __forceinline__ const uint8_t* block(int, int pos, int) const {
        return gin + (long long)pos * bb;
    }
};
struct PackedOut {
    uint8_t* gout;
    int bb;
    __device__ __forceinline__ uint8_t* at(int j) const { return gout + (long long)j * bb; }
};

// One (group, chunk) unit: n <= RC outputs over every column tile of the group.
//   cw: the unit's coefficient words, [k][RCP] bytes (RCP = max(4, RC))
//   in.block(u, pos, k): the address of input block pos; the unit asks in the order it loads
//   (slot u = pos % PD, first min(u, k - 1), then min(pos + PD, k - 1) while pos is combined)
//   out.at(j): the address of output j < n
template <int RC, bool TINY, class In, class Out>
__device__ __forceinline__ void ragged_unit(In in, const Out out, const uint32_t* cw, int k,
                                            int bb, int n, int lane) {
    constexpr int RCP = RC < 4 ? 4 : RC;
    constexpr int NCW = RCP / 4;
    constexpr int PD = kRaggedPD;
    const int s = bb >> 3;
    const int nw = (s + 3) >> 2;
    const int ntiles = (nw + 63) >> 6;
#pragma unroll 1
    for (int tile = 0; tile < ntiles; ++tile) {
        const int c = tile * 64 + lane;
        const ColAccess ca = col_access<TINY>(c, nw, s);
        uint32_t acc[RC][8];
#pragma unroll
        for (int j = 0; j < RC; ++j)
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[j][r] = 0;
        in.start(k);
        // two blocks in flight while one is combined, as gf_apply_kernel (PD = 2)
        uint32_t raw[PD][8];
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const uint8_t* p = in.block(u, min(u, k - 1), k);
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
                    for (int t = 0; t < 8; ++t)
                        v.W[t] = TINY ? raw[u][t] : (raw[u][t] >> ca.shift);
                    const uint8_t* p = in.block(u, min(pos + PD, k - 1), k);
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
#pragma unroll
        for (int j = 0; j < RC; ++j) {
            if (j < n) {
                uint8_t* dst = out.at(j);
#pragma unroll
                for (int r = 0; r < 8; ++r) store_word(dst + r * s, c, ca, acc[j][r]);
            }
        }
    }
}

// Register bound (the kernels are launched with 256 threads; the bound only caps VGPRs at
// 512 / ceil(waves / 4) = 168, three waves per SIMD).  The loops around the unit cost registers
// that gf_apply_kernel's straight-line body does not need: at gf_apply's bound for RC 4
// (128 VGPRs) the kernel spilled 232 bytes per lane; at 168 it needs no scratch.  Measured on
// one box, alternating: (32, 4) encode 1.10 -> 0.87 ms, decode 1.01 -> 0.75 ms.  RC 8 does
// not fit under any bound (256 VGPRs and 404 bytes of scratch at two waves), so the ragged
// paths use chunks of at most 4 outputs.
constexpr int kRaggedBound = 640;

// 16 bytes at an 8-byte aligned address (the XOR kernels' wide unit)
typedef uint32_t rg_u32x4a8 __attribute__((ext_vector_type(4), aligned(8)));

// ragged_grid (fec_kernels.h) against the workgroups of `kern` the device holds
inline unsigned ragged_grid_of(const void* kern, long long units, const Tune& t) {
    return ragged_grid(units, (long long)t.cus * resident_blocks(kern, 256, 0));
}

}  // namespace qfec
