// gf_ragged.hip — run-time-shape kernels for batches whose groups share (k, m) but carry their
// own block_bytes (qfec_*_batch_ragged*, include/quic_fec.h).
//
// Packed layout: group g's blocks are [n][bb[g]] contiguous at base + off[g] (off a multiple
// of 16, gaps never written).  Per-group semantics are those of the uniform call with
// block_bytes = bb[g]; the bit-sliced code splits a block into 8 sub-rows of bb/8 bytes, so
// the sub-row stride differs per group and a short group cannot be padded to a common size.
//
// Work mapping: persistent, oversubscribed grids.  Wave w walks the
// units w, w + W, ... and loops over the unit's 64-word column tiles, so no unit-start table
// has to be scanned first and nothing depends on the sizes on the host.
//   gf_ragged_kernel   unit = (group, output chunk), chunk fastest; m > 1
//   xor_ragged_kernel  unit = group; m == 1, and the XOR parity of the groups the reference
//                      rejects (cauchy_256.cpp:1519-1534)
//   copy_ragged_kernel unit = group; k <= 1
// All of a unit's shape (bb, offsets, counts) is wave-uniform.  No MFMA: byte XORs only.
#include <algorithm>

#include "gf_ragged_unit.h"

namespace qfec {

//   coef:   encode: the shared [nchunk][k][RCP] table; decode: + g * coef_gstride
//   encode: outputs o = chunk*RC + j < m go to out + out_off[g] + o*bb[g]
//   decode: outputs o < nout[g], same place (the recovered-blocks layout)
// A group with bb % 8 != 0 (or bb < 8) is skipped: its status and XOR parity are the other
// kernels' business.
template <int RC, bool DECODE>
__global__ __launch_bounds__(kRaggedBound) void gf_ragged_kernel(
    const uint8_t* __restrict__ in, const long long* __restrict__ in_off, uint8_t* out,
    const long long* __restrict__ out_off, const int32_t* __restrict__ bbs,
    const uint8_t* __restrict__ coef, const int32_t* __restrict__ nout, int k, int m,
    int nchunk, long long coef_gstride, long long total_units) {
    constexpr int RCP = RC < 4 ? 4 : RC;
    const int lane = threadIdx.x & 63;
    // 32-bit unit numbers (the launcher caps them at 2^31): a 64-bit division has no scalar
    // form and would drag the unit's addresses into vector registers
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
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        if (bb < 8 || (bb & 7)) continue;
        int n = DECODE ? __builtin_amdgcn_readfirstlane(nout[g]) : m;
        n = min(n - (int)chunk * RC, RC);
        if (n <= 0) continue;
        const uint8_t* gin = in + uniform64(in_off[g]);
        uint8_t* gout = out + uniform64(out_off[g]) + (long long)chunk * RC * bb;
        const uint32_t* cw = (const uint32_t*)(coef + (DECODE ? g * coef_gstride : 0) +
                                               (long long)chunk * k * RCP);
        const PackedIn bin{gin, bb};
        const PackedOut bout{gout, bb};
        if (bb >= 32) ragged_unit<RC, false>(bin, bout, cw, k, bb, n, lane);
        else ragged_unit<RC, true>(bin, bout, cw, k, bb, n, lane);
    }
}

// ------------------------------------------------------------------ XOR (m == 1)
// out block of group g = XOR of its k blocks.  16-byte units where bb % 8 == 0 (every block
// then starts 8-byte aligned), unaligned 4-byte units otherwise, and a byte tail.  Every byte
// is touched once: non-temporal, as xor_flat_kernel.
//   encode modes: 0 every group, status 0 (m == 1); 1 every group, status -1 (m > 1 and
//   k + m > 256); 2 only the groups with bb % 8 != 0, status -1 for those and 0 for the rest
//   decode: the group's recovered block, unless eidx[g] == 255 (nothing erased); the XOR
//   runs over all k slots, the recovery block included (cauchy_256.cpp:505-531)
template <bool DECODE>
__global__ __launch_bounds__(256) void xor_ragged_kernel(
    const uint8_t* __restrict__ in, const long long* __restrict__ in_off, uint8_t* out,
    const long long* __restrict__ out_off, const int32_t* __restrict__ bbs,
    const uint8_t* __restrict__ eidx, int32_t* __restrict__ status, int k, long long groups,
    int mode) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long g = (long long)xcd_logical_block() * 4 + wave_id(); g < groups; g += stride) {
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        if (DECODE) {
            if (eidx[g] == 255) continue;
        } else {
            // mode 2 is the m > 1 encode's
            const bool bad = mode == 1 || (mode == 2 && ragged_encode_rejects(k, 2, bb));
            if (status && lane == 0) status[g] = bad ? -1 : 0;
            if (mode == 2 && !bad) continue;
        }
        if (bb < 1) continue;
        const uint8_t* p = in + uniform64(in_off[g]);
        uint8_t* dst = out + uniform64(out_off[g]);
        int done;
        if ((bb & 7) == 0) {
            const int nu = bb >> 4;
            for (int q = lane; q < nu; q += 64) {
                const uint8_t* pq = p + 16 * q;
                rg_u32x4a8 acc = __builtin_nontemporal_load((const rg_u32x4a8*)pq);
#pragma unroll 4
                for (int x = 1; x < k; ++x)
                    acc ^= __builtin_nontemporal_load((const rg_u32x4a8*)(pq + (long long)x * bb));
                __builtin_nontemporal_store(acc, (rg_u32x4a8*)(dst + 16 * q));
            }
            done = nu << 4;
        } else {
            const int nu = bb >> 2;
            for (int q = lane; q < nu; q += 64) {
                const uint8_t* pq = p + 4 * q;
                uint32_t acc = __builtin_nontemporal_load((const u32ua*)pq);
#pragma unroll 4
                for (int x = 1; x < k; ++x)
                    acc ^= __builtin_nontemporal_load((const u32ua*)(pq + (long long)x * bb));
                __builtin_nontemporal_store(acc, (u32ua*)(dst + 4 * q));
            }
            done = nu << 2;
        }
        for (int i = done + lane; i < bb; i += 64) {   // at most 8 bytes
            uint8_t acc = 0;
            for (int x = 0; x < k; ++x) acc ^= p[(long long)x * bb + i];
            dst[i] = acc;
        }
    }
}

// ------------------------------------------------------------------ k <= 1
// encode: the group's one block into each of its m outputs (cauchy_256.cpp:1508-1516).
// decode: a block tagged anything but row 0 is a copy of data row 0, so it is the recovered
// block (rec_k1_kernel); rmax = 1.
template <bool DECODE>
__global__ __launch_bounds__(256) void copy_ragged_kernel(
    const uint8_t* __restrict__ in, const long long* __restrict__ in_off, uint8_t* out,
    const long long* __restrict__ out_off, const int32_t* __restrict__ bbs,
    const uint8_t* __restrict__ rows_in, uint8_t* __restrict__ rec_rows,
    int32_t* __restrict__ status, int m, long long groups) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long g = (long long)blockIdx.x * 4 + wave_id(); g < groups; g += stride) {
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        int copies = m;
        if (DECODE) {
            const bool lost = rows_in[g] != 0;
            if (lane == 0) rec_rows[g] = lost ? 0 : 255;
            copies = lost ? 1 : 0;
        }
        if (status && lane == 0) status[g] = 0;
        const uint8_t* p = in + uniform64(in_off[g]);
        uint8_t* dst = out + uniform64(out_off[g]);
        for (int y = 0; y < copies; ++y)
            for (int i = lane; i < bb; i += 64) dst[(long long)y * bb + i] = p[i];
    }
}

// After the run-time decode prep (run with a block size of 8: its tables do not depend on
// it): a group whose own bb is not a multiple of 8 has status -1 unless it holds no recovery
// block (cauchy_256.cpp:1287-1294), and recovers nothing.
__global__ __launch_bounds__(256) void ragged_decode_status_kernel(
    const int32_t* __restrict__ bbs, const uint8_t* __restrict__ rows_in,
    uint8_t* __restrict__ rec_rows, int32_t* __restrict__ status, int32_t* __restrict__ nout,
    int k, int rmax, long long groups) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    if ((bbs[g] & 7) == 0) return;
    bool anyrec = false;
    for (int i = 0; i < k; ++i) anyrec |= rows_in[g * k + i] >= k;
    if (!anyrec) return;
    nout[g] = 0;
    for (int j = 0; j < rmax; ++j) rec_rows[g * rmax + j] = 255;
    if (status) status[g] = -1;
}

// ---------------------------------------------------------------------- launchers
hipError_t launch_gf_ragged(const Apply& a, RaggedView v, int nchunk, bool decode) {
    const long long units = a.groups * nchunk;
    if (units <= 0) return hipSuccess;
    if (units > 0x7fffffffLL) return hipErrorInvalidValue;
    note_kernel(decode ? "gf_ragged_kernel<decode>" : "gf_ragged_kernel<encode>");
    const bool known = dispatch_value<2, 4>(a.rc, [&](auto RC) {
        dispatch_bool(decode, [&](auto DEC) {
            const auto kern = gf_ragged_kernel<decltype(RC)::value, decltype(DEC)::value>;
            const unsigned nb = ragged_grid_of((const void*)kern, units, *a.t);
            note_grid("gf_ragged_kernel", nb);
            qlaunch(kern, dim3(nb), dim3(256), 0, a.st, a.in, v.in_off, a.out, v.out_off, v.bb,
                    a.tab, a.nout, a.k, a.m, nchunk, a.tab_gstride, units);
        });
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_xor_ragged(const uint8_t* in, uint8_t* out, RaggedView v, const uint8_t* eidx,
                             int32_t* status, int k, long long groups, bool decode, int mode,
                             hipStream_t st, const Tune& t) {
    if (groups <= 0) return hipSuccess;
    note_kernel("xor_ragged_kernel");
    dispatch_bool(decode, [&](auto DEC) {
        const auto kern = xor_ragged_kernel<decltype(DEC)::value>;
        const unsigned nb = ragged_grid_of((const void*)kern, groups, t);
        note_grid("xor_ragged_kernel", nb);
        qlaunch(kern, dim3(nb), dim3(256), 0, st, in, v.in_off, out, v.out_off, v.bb, eidx, status,
                k, groups, mode);
    });
    return hipGetLastError();
}

hipError_t launch_copy_ragged(const uint8_t* in, uint8_t* out, RaggedView v,
                              const uint8_t* rows_in, uint8_t* rec_rows, int32_t* status, int m,
                              long long groups, bool decode, hipStream_t st, const Tune& t) {
    if (groups <= 0) return hipSuccess;
    const unsigned nb = persistent_grid(groups, 4, (long long)t.cus * 16, 0, 0);
    if (!nb) return hipErrorInvalidValue;
    note_kernel("copy_ragged_kernel");
    dispatch_bool(decode, [&](auto DEC) {
        qlaunch((copy_ragged_kernel<decltype(DEC)::value>), dim3(nb), dim3(256), 0, st, in,
                v.in_off, out, v.out_off, v.bb, rows_in, rec_rows, status, m, groups);
    });
    return hipGetLastError();
}

hipError_t launch_ragged_decode_status(const int32_t* bb, const uint8_t* rows_in,
                                       uint8_t* rec_rows, int32_t* status, int32_t* nout, int k,
                                       int rmax, long long groups, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    note_kernel("ragged_decode_status_kernel");
    qlaunch((ragged_decode_status_kernel), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
            st, bb, rows_in, rec_rows, status, nout, k, rmax, groups);
    return hipGetLastError();
}

}  // namespace qfec
