// gf_ptrs.hip — pointer-table batches (qfec_*_batch_ptrs*, include/quic_fec.h): the run-time-
// shape kernels of gf_ragged.hip with one change of addressing.  Block pos of group g lies at
// the device address in_ptrs[g * k + pos], output o at out_ptrs[g * ostride + o] (ostride = m for
// an encode, min(k, m) for a decode), anywhere and at any alignment; the group's size is
// bbs[g], or bb_all for every group where bbs is null.  Per-group semantics, unit mapping and
// grids are the ragged kernels' (DESIGN.md sections 3.8 and 3.9):
//   gf_ptrs_kernel    unit = (group, output chunk), chunk fastest; m > 1
//   xor_ptrs_kernel   unit = group; m == 1 and the XOR parity of the groups the reference rejects
//   copy_ptrs_kernel  unit = group; k <= 1
// A table entry is wave-uniform and is dereferenced only where the contract says so: none of a
// group with bb < 1, no parity entry past the first of a rejected group, no recovered-block
// entry at or past the group's erasure count.  Table indices are 64-bit.
#include <algorithm>

#include "gf_ptrs.h"
#include "gf_ragged_unit.h"

namespace qfec {

typedef unsigned long long ptr_t;   // a device address as the tables hold it

// The group's k input addresses, fetched as the unit's block loop goes: slot u holds the address
// of the block that slot loads next, and is refilled (a scalar load) with the one after it when
// that is handed out.  So the address of block pos + 2 * PD is on its way while block pos is
// combined and block pos + PD is being loaded; k reaches 255 and the addresses are never all held.
struct TableIn {
    const ptr_t* tbl;   // in_ptrs + g * k, wave-uniform
    ptr_t held[kRaggedPD];
    __device__ __forceinline__ void start(int k) {
#pragma unroll
        for (int u = 0; u < kRaggedPD; ++u) held[u] = tbl[min(u, k - 1)];
    }
    __device__ __forceinline__ const uint8_t* block(int u, int pos, int k) {
        const ptr_t a = held[u];
        held[u] = tbl[min(pos + kRaggedPD, k - 1)];
        return (const uint8_t*)uniform64((long long)a);
    }
};
// The unit's output addresses, read once per unit.
template <int RC>
struct TableOut {
    uint8_t* p[RC];
    __device__ __forceinline__ uint8_t* at(int j) const { return p[j]; }
};

__device__ __forceinline__ int group_bb(const int32_t* bbs, int bb_all, long long g) {
    return bbs ? __builtin_amdgcn_readfirstlane(bbs[g]) : bb_all;
}

//   coef:   encode: the shared [nchunk][k][RCP] table; decode: + g * coef_gstride
//   encode: outputs o = chunk*RC + j < m; decode: outputs o < nout[g]
// A group with bb % 8 != 0 (or bb < 8) is skipped: its status and XOR parity are the other
// kernels' business.
template <int RC, bool DECODE>
__global__ __launch_bounds__(kRaggedBound) void gf_ptrs_kernel(
    const ptr_t* __restrict__ in_ptrs, const ptr_t* __restrict__ out_ptrs,
    const int32_t* __restrict__ bbs, int bb_all, const uint8_t* __restrict__ coef,
    const int32_t* __restrict__ nout, int k, int m, int ostride, int nchunk,
    long long coef_gstride, long long total_units) {
    constexpr int RCP = RC < 4 ? 4 : RC;
    const int lane = threadIdx.x & 63;
    // 32-bit unit numbers (the launcher caps them at 2^31), as gf_ragged_kernel
    const unsigned stride = gridDim.x * 4u, total = (unsigned)total_units;
#pragma unroll 1
    for (unsigned unit = xcd_logical_block() * 4u + (unsigned)wave_id(); unit < total;
         unit += stride) {
        unsigned gq = unit, chunk = 0;
        if (nchunk > 1) {
            gq = __builtin_amdgcn_readfirstlane(unit / (unsigned)nchunk);
            chunk = unit - gq * (unsigned)nchunk;
        }
        const long long g = gq;
        const int bb = group_bb(bbs, bb_all, g);
        if (bb < 8 || (bb & 7)) continue;
        int n = DECODE ? __builtin_amdgcn_readfirstlane(nout[g]) : m;
        n = min(n - (int)chunk * RC, RC);
        if (n <= 0) continue;
        TableIn bin;
        bin.tbl = in_ptrs + g * k;
        TableOut<RC> bout;
        const ptr_t* po = out_ptrs + g * ostride + (long long)chunk * RC;
#pragma unroll
        for (int j = 0; j < RC; ++j)
            bout.p[j] = j < n ? (uint8_t*)uniform64((long long)po[j]) : nullptr;
        const uint32_t* cw = (const uint32_t*)(coef + (DECODE ? g * coef_gstride : 0) +
                                               (long long)chunk * k * RCP);
        if (bb >= 32) ragged_unit<RC, false>(bin, bout, cw, k, bb, n, lane);
        else ragged_unit<RC, true>(bin, bout, cw, k, bb, n, lane);
    }
}

// ------------------------------------------------------------------ XOR (m == 1)
// Up to 64 of a group's addresses lie one per lane (va: entry base + lane); block x of them as a
// scalar.  v_readlane reads a lane whether or not it is active, so va must have been loaded
// with every lane active: the loops below are uniform, their idle lanes repeat the last unit.
__device__ __forceinline__ const uint8_t* lane_addr(ptr_t va, int x) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)va, x);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(va >> 32), x);
    return (const uint8_t*)(((ptr_t)hi << 32) | lo);
}

// dst unit q = XOR over the k blocks of their unit q, for the `count` units of type U from
// unit `first` on.  va0: the group's first 64 addresses.
template <class U>
__device__ __forceinline__ void xor_units(const ptr_t* tbl, ptr_t va0, uint8_t* dst, int k,
                                          int first, int count, int lane) {
#pragma unroll 1
    for (int q0 = 0; q0 < count; q0 += 64) {
        const int q = first + min(q0 + lane, count - 1);
        U acc = {};
#pragma unroll 1
        for (int base = 0; base < k; base += 64) {
            const ptr_t va = base == 0 ? va0 : tbl[min(base + lane, k - 1)];
            const int nb = min(64, k - base);
            const auto unit_of = [&](int x) {
                return __builtin_nontemporal_load((const U*)lane_addr(va, x) + q);
            };
            // four loads in flight (written out: the lane reads keep the loop from unrolling)
            int x = 0;
            for (; x + 4 <= nb; x += 4) {
                const U a = unit_of(x), b = unit_of(x + 1), c = unit_of(x + 2), d = unit_of(x + 3);
                acc = (U)(acc ^ a ^ b ^ c ^ d);
            }
            for (; x < nb; ++x) acc = (U)(acc ^ unit_of(x));
        }
        if (q0 + lane < count) __builtin_nontemporal_store(acc, (U*)dst + q);
    }
}

// out block of group g = XOR of its k blocks, modes and decode form as xor_ragged_kernel.
// 16-byte units where bb % 8 == 0 and the output and all k inputs are 8-byte aligned (chosen
// per group, wave-uniformly); unaligned 4-byte units otherwise; a byte tail.  Both give the same
// bytes, and no byte outside [ptr, ptr + bb) of a block is touched.
template <bool DECODE>
__global__ __launch_bounds__(256) void xor_ptrs_kernel(
    const ptr_t* __restrict__ in_ptrs, const ptr_t* __restrict__ out_ptrs,
    const int32_t* __restrict__ bbs, int bb_all, const uint8_t* __restrict__ eidx,
    int32_t* __restrict__ status, int k, int ostride, long long groups, int mode) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long g = (long long)xcd_logical_block() * 4 + wave_id(); g < groups; g += stride) {
        const int bb = group_bb(bbs, bb_all, g);
        if (DECODE) {
            if (eidx[g] == 255) continue;
        } else {
            // mode 2 is the m > 1 encode's
            const bool bad = mode == 1 || (mode == 2 && ragged_encode_rejects(k, 2, bb));
            if (status && lane == 0) status[g] = bad ? -1 : 0;
            if (mode == 2 && !bad) continue;
        }
        if (bb < 1) continue;
        const ptr_t* tbl = in_ptrs + g * k;
        uint8_t* dst = (uint8_t*)uniform64((long long)out_ptrs[g * ostride]);
        const ptr_t va0 = tbl[min(lane, k - 1)];
        uint32_t mis = (uint32_t)va0 | (uint32_t)(uintptr_t)dst | (uint32_t)bb;
        for (int base = 64; base < k; base += 64) mis |= (uint32_t)tbl[min(base + lane, k - 1)];
        const bool wide = __builtin_amdgcn_ballot_w64((mis & 7u) != 0) == 0;
        int done;
        if (wide) {
            xor_units<rg_u32x4a8>(tbl, va0, dst, k, 0, bb >> 4, lane);
            done = (bb >> 4) << 4;
        } else {
            xor_units<u32ua>(tbl, va0, dst, k, 0, bb >> 2, lane);
            done = (bb >> 2) << 2;
        }
        xor_units<uint8_t>(tbl, va0, dst, k, done, bb - done, lane);   // at most 8 bytes
    }
}

// ------------------------------------------------------------------ k <= 1
// encode: the group's one block into each of its m outputs; decode: a block tagged anything
// but row 0 is the recovered block (rmax = 1).  As copy_ragged_kernel.
template <bool DECODE>
__global__ __launch_bounds__(256) void copy_ptrs_kernel(
    const ptr_t* __restrict__ in_ptrs, const ptr_t* __restrict__ out_ptrs,
    const int32_t* __restrict__ bbs, int bb_all, const uint8_t* __restrict__ rows_in,
    uint8_t* __restrict__ rec_rows, int32_t* __restrict__ status, int k, int m, int ostride,
    long long groups) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long g = (long long)blockIdx.x * 4 + wave_id(); g < groups; g += stride) {
        const int bb = group_bb(bbs, bb_all, g);
        int copies = m;
        if (DECODE) {
            const bool lost = rows_in[g * k] != 0;
            if (lane == 0) rec_rows[g] = lost ? 0 : 255;
            copies = lost ? 1 : 0;
        }
        if (status && lane == 0) status[g] = 0;
        if (bb < 1 || copies == 0) continue;
        const uint8_t* p = (const uint8_t*)uniform64((long long)in_ptrs[g * k]);
        for (int y = 0; y < copies; ++y) {
            uint8_t* dst = (uint8_t*)uniform64((long long)out_ptrs[g * ostride + y]);
            for (int i = lane; i < bb; i += 64) dst[i] = p[i];
        }
    }
}

// The status fix-up of ragged_decode_status_kernel for a call without a size array: bb_all is
// not a multiple of 8, so every group that holds a recovery block has status -1 and recovers
// nothing.
__global__ __launch_bounds__(256) void ptrs_decode_status_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* __restrict__ rec_rows,
    int32_t* __restrict__ status, int32_t* __restrict__ nout, int k, int rmax, long long groups) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    bool anyrec = false;
    for (int i = 0; i < k; ++i) anyrec |= rows_in[g * k + i] >= k;
    if (!anyrec) return;
    nout[g] = 0;
    for (int j = 0; j < rmax; ++j) rec_rows[g * rmax + j] = 255;
    if (status) status[g] = -1;
}

// ---------------------------------------------------------------------- launchers
hipError_t launch_gf_ptrs(const Apply& a, PtrsView v, int nchunk, bool decode) {
    const long long units = a.groups * nchunk;
    if (units <= 0) return hipSuccess;
    if (units > 0x7fffffffLL) return hipErrorInvalidValue;
    note_kernel(decode ? "gf_ptrs_kernel<decode>" : "gf_ptrs_kernel<encode>");
    const bool known = dispatch_value<2, 4>(a.rc, [&](auto RC) {
        dispatch_bool(decode, [&](auto DEC) {
            const auto kern = gf_ptrs_kernel<decltype(RC)::value, decltype(DEC)::value>;
            const unsigned nb = ragged_grid_of((const void*)kern, units, *a.t);
            note_grid("gf_ptrs_kernel", nb);
            qlaunch(kern, dim3(nb), dim3(256), 0, a.st, v.in, v.out, v.bb, v.bb_all, a.tab, a.nout,
                    a.k, a.m, decode ? a.rmax : a.m, nchunk, a.tab_gstride, units);
        });
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_xor_ptrs(PtrsView v, const uint8_t* eidx, int32_t* status, int k, int ostride,
                           long long groups, bool decode, int mode, hipStream_t st,
                           const Tune& t) {
    if (groups <= 0) return hipSuccess;
    note_kernel("xor_ptrs_kernel");
    dispatch_bool(decode, [&](auto DEC) {
        const auto kern = xor_ptrs_kernel<decltype(DEC)::value>;
        const unsigned nb = ragged_grid_of((const void*)kern, groups, t);
        note_grid("xor_ptrs_kernel", nb);
        qlaunch(kern, dim3(nb), dim3(256), 0, st, v.in, v.out, v.bb, v.bb_all, eidx, status, k,
                ostride, groups, mode);
    });
    return hipGetLastError();
}

hipError_t launch_copy_ptrs(PtrsView v, const uint8_t* rows_in, uint8_t* rec_rows,
                            int32_t* status, int k, int m, long long groups, bool decode,
                            hipStream_t st, const Tune& t) {
    if (groups <= 0) return hipSuccess;
    const unsigned nb = persistent_grid(groups, 4, (long long)t.cus * 16, 0, 0);
    if (!nb) return hipErrorInvalidValue;
    note_kernel("copy_ptrs_kernel");
    dispatch_bool(decode, [&](auto DEC) {
        qlaunch((copy_ptrs_kernel<decltype(DEC)::value>), dim3(nb), dim3(256), 0, st, v.in, v.out,
                v.bb, v.bb_all, rows_in, rec_rows, status, k, m, decode ? 1 : m, groups);
    });
    return hipGetLastError();
}

hipError_t launch_ptrs_decode_status(PtrsView v, const uint8_t* rows_in, uint8_t* rec_rows,
                                     int32_t* status, int32_t* nout, int k, int rmax,
                                     long long groups, hipStream_t st) {
    if (v.bb) return launch_ragged_decode_status(v.bb, rows_in, rec_rows, status, nout, k, rmax,
                                                 groups, st);
    if (groups <= 0 || (v.bb_all & 7) == 0) return hipSuccess;
    note_kernel("ptrs_decode_status_kernel");
    qlaunch((ptrs_decode_status_kernel), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
            rows_in, rec_rows, status, nout, k, rmax, groups);
    return hipGetLastError();
}

}  // namespace qfec
