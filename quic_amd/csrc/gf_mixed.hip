// gf_mixed.hip — run-time-shape kernels for batches whose groups each name their own (k, m)
// through an index into a code set (qfec_*_batch_mixed*, include/quic_fec.h; DESIGN.md
// section 3.10).
//
// The packed layout and the per-group semantics are the ragged batches' (gf_ragged.hip) with
// the group's own k and m: group g's k_g blocks are [k_g][bb[g]] at base + off[g].  The unit
// body is ragged_unit (gf_ragged_unit.h), which already takes k, bb, the output count and the
// coefficient pointer as wave-uniform run-time values; what is new here is where they come
// from: the record codes[code[g]] of the set's device table (gf_mixed.h), read once per unit
// into scalar registers.
//   gf_mixed_kernel        unit = (group, output chunk) over groups x the set's largest chunk
//                          count, chunk fastest; a unit past its group's own count, of a group
//                          the code or the size rejects, or of a code without GF work (m == 1,
//                          k <= 1) leaves at once
//   xor_copy_mixed_kernel  unit = group; everything that is not GF work, and every status the
//                          prep does not write
// One output chunk size for the whole set keeps each direction to one GF launch.
#include <algorithm>

#include "gf_mixed.h"
#include "gf_ragged_unit.h"

namespace qfec {

// The record of group g's code in scalar registers; false: code[g] names no code of the set.
struct CodeOf {
    int k, m, nchunk;
    long long enc_off;
};
template <bool DECODE>
__device__ __forceinline__ bool code_of(const MixedCode* __restrict__ codes, int ncodes,
                                        const uint8_t* __restrict__ code, long long g, CodeOf* c) {
    const int ci = __builtin_amdgcn_readfirstlane((int)code[g]);
    if (ci >= ncodes) return false;
    const MixedCode* d = codes + ci;
    c->k = __builtin_amdgcn_readfirstlane(d->k);
    c->m = __builtin_amdgcn_readfirstlane(d->m);
    c->nchunk = __builtin_amdgcn_readfirstlane(DECODE ? d->dec_nchunk : d->enc_nchunk);
    c->enc_off = DECODE ? 0 : uniform64(d->enc_off);
    return true;
}

//   encode: outputs o = chunk*RC + j < m_g go to out + out_off[g] + o*bb[g], from the code's table
//           at coef + enc_off (coef: the set's encode tables)
//   decode: outputs o < nout[g], same place, from the prep's table at coef + g * coef_gstride
template <int RC, bool DECODE>
__global__ __launch_bounds__(kRaggedBound) void gf_mixed_kernel(
    const uint8_t* __restrict__ in, const long long* __restrict__ in_off, uint8_t* out,
    const long long* __restrict__ out_off, const int32_t* __restrict__ bbs,
    const uint8_t* __restrict__ code, const MixedCode* __restrict__ codes, int ncodes,
    const uint8_t* __restrict__ coef, const int32_t* __restrict__ nout, int nchunk,
    long long coef_gstride, long long total_units) {
    constexpr int RCP = RC < 4 ? 4 : RC;
    const int lane = threadIdx.x & 63;
    // 32-bit unit numbers, as gf_ragged_kernel (the launcher caps them at 2^31)
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
        CodeOf c;
        if (!code_of<DECODE>(codes, ncodes, code, g, &c)) continue;
        if ((int)chunk >= c.nchunk) continue;      // also every code without GF work (0 chunks)
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        if (bb < 8 || (bb & 7)) continue;
        int n = DECODE ? __builtin_amdgcn_readfirstlane(nout[g]) : c.m;
        n = min(n - (int)chunk * RC, RC);
        if (n <= 0) continue;
        const uint8_t* gin = in + uniform64(in_off[g]);
        uint8_t* gout = out + uniform64(out_off[g]) + (long long)chunk * RC * bb;
        const uint32_t* cw = (const uint32_t*)(coef + (DECODE ? g * coef_gstride : c.enc_off) +
                                               (long long)chunk * c.k * RCP);
        const PackedIn bin{gin, bb};
        const PackedOut bout{gout, bb};
        if (bb >= 32) ragged_unit<RC, false>(bin, bout, cw, c.k, bb, n, lane);
        else ragged_unit<RC, true>(bin, bout, cw, c.k, bb, n, lane);
    }
}

// dst = XOR of the k blocks [k][bb] at p, by one wave; the units of xor_ragged_kernel: 16 bytes
// where bb % 8 == 0 (every block then starts 8-byte aligned), unaligned dwords otherwise, and a
// byte tail.  Vector loads and stores only.
__device__ __forceinline__ void xor_group(const uint8_t* p, uint8_t* dst, int k, int bb, int lane) {
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

// A wave's LDS operations execute in order: only the compiler has to be kept from reordering.
__device__ __forceinline__ void mixed_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// One wave per group, persistent.
//   encode  code[g] >= ncodes: status -2, nothing else.  k <= 1: the block into each of the m
//           outputs (copy_ragged_kernel).  m == 1: XOR parity.  m > 1: status 0, or -1 with the
//           XOR parity in the first parity block where the code (k + m > 256) or the size
//           (bb % 8 != 0) is rejected (xor_ragged_kernel's modes 1 and 2, per group).
//   decode  code[g] >= ncodes: status -2, rec_rows 255.  k <= 1: copy_ragged_kernel<decode>.
//           m == 1: m1_prep_kernel's bookkeeping (the first slot tagged a row >= k receives the
//           first data row not present, or keeps its tag), then the XOR over all k slots
//           (cauchy_256.cpp:505-531).  m > 1: the prep's.
// rec_rows is written up to the set's rmax; rows are read at g * kmax.
template <bool DECODE>
__global__ __launch_bounds__(256) void xor_copy_mixed_kernel(
    const uint8_t* __restrict__ in, const long long* __restrict__ in_off, uint8_t* out,
    const long long* __restrict__ out_off, const int32_t* __restrict__ bbs,
    const uint8_t* __restrict__ code, const MixedCode* __restrict__ codes, int ncodes,
    const uint8_t* __restrict__ rows_in, uint8_t* __restrict__ rec_rows,
    int32_t* __restrict__ status, int kmax, int rmax, long long groups) {
    __shared__ uint8_t lseen[4][256];
    const int lane = threadIdx.x & 63;
    uint8_t* seen = lseen[wave_id()];
    const long long stride = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long g = (long long)xcd_logical_block() * 4 + wave_id(); g < groups; g += stride) {
        CodeOf c;
        uint8_t* rr = DECODE ? rec_rows + g * rmax : nullptr;
        if (!code_of<true>(codes, ncodes, code, g, &c)) {
            if (status && lane == 0) status[g] = -2;
            if (DECODE)
                for (int j = lane; j < rmax; j += 64) rr[j] = 255;
            continue;
        }
        const int k = c.k, m = c.m;
        if (DECODE && mixed_is_gf(k, m)) continue;
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        const uint8_t* p = in + uniform64(in_off[g]);
        uint8_t* dst = out + uniform64(out_off[g]);
        if (k <= 1) {
            int copies = m;
            if (DECODE) {
                const bool lost = rows_in[g * kmax] != 0;
                for (int j = lane; j < rmax; j += 64) rr[j] = (j == 0 && lost) ? 0 : 255;
                copies = lost ? 1 : 0;
            }
            if (status && lane == 0) status[g] = 0;
            for (int y = 0; y < copies; ++y)
                for (int i = lane; i < bb; i += 64) dst[(long long)y * bb + i] = p[i];
            continue;
        }
        if (DECODE) {   // m == 1
            const uint8_t* rg = rows_in + g * kmax;
            for (int i = lane; i < 256; i += 64) seen[i] = 0;
            mixed_wave_sync();
            int e = -1;
            for (int base = 0; base < k; base += 64) {
                const int i = base + lane;
                const int r = i < k ? rg[i] : 0;
                const unsigned long long msk = __ballot(i < k && r >= k);
                if (e < 0 && msk) e = base + __ffsll((long long)msk) - 1;
                if (i < k && r < k) seen[r] = 1;
            }
            mixed_wave_sync();
            int miss = -1;
            for (int base = 0; base < k && miss < 0; base += 64) {
                const int x = base + lane;
                const unsigned long long msk = __ballot(x < k && !seen[x]);
                if (msk) miss = base + __ffsll((long long)msk) - 1;
            }
            mixed_wave_sync();
            if (status && lane == 0) status[g] = 0;
            for (int j = lane; j < rmax; j += 64)
                rr[j] = (j == 0 && e >= 0) ? (uint8_t)(miss >= 0 ? miss : rg[e]) : (uint8_t)255;
            if (e < 0 || bb < 1) continue;
            xor_group(p, dst, k, bb, lane);
            continue;
        }
        const bool bad = mixed_encode_rejects(k, m, bb);
        if (status && lane == 0) status[g] = bad ? -1 : 0;
        if ((m > 1 && !bad) || bb < 1) continue;
        xor_group(p, dst, k, bb, lane);
    }
}

// ---------------------------------------------------------------------- launchers
hipError_t launch_gf_mixed(const MixedSet& s, MixedView v, const uint8_t* in, uint8_t* out,
                           const uint8_t* coef, const int32_t* nout, long long groups, bool decode,
                           hipStream_t st, const Tune& t) {
    const int nchunk = decode ? s.dec_nchunk : s.enc_nchunk;
    const long long units = groups * nchunk;
    if (units <= 0) return hipSuccess;
    if (units > 0x7fffffffLL) return hipErrorInvalidValue;
    note_kernel(decode ? "gf_mixed_kernel<decode>" : "gf_mixed_kernel<encode>");
    const bool known = dispatch_value<2, 4>(decode ? s.dec_rc : s.enc_rc, [&](auto RC) {
        dispatch_bool(decode, [&](auto DEC) {
            const auto kern = gf_mixed_kernel<decltype(RC)::value, decltype(DEC)::value>;
            const unsigned nb = ragged_grid_of((const void*)kern, units, t);
            note_grid("gf_mixed_kernel", nb);
            qlaunch(kern, dim3(nb), dim3(256), 0, st, in, v.in_off, out, v.out_off, v.bb, v.code,
                    s.codes, s.ncodes, decode ? coef : s.enc_tabs, nout, nchunk, s.coef_gstride,
                    units);
        });
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_xor_copy_mixed(const MixedSet& s, MixedView v, const uint8_t* in, uint8_t* out,
                                 const uint8_t* rows_in, uint8_t* rec_rows, int32_t* status,
                                 long long groups, bool decode, hipStream_t st, const Tune& t) {
    if (groups <= 0) return hipSuccess;
    note_kernel(decode ? "xor_copy_mixed_kernel<decode>" : "xor_copy_mixed_kernel<encode>");
    dispatch_bool(decode, [&](auto DEC) {
        const auto kern = xor_copy_mixed_kernel<decltype(DEC)::value>;
        const unsigned nb = ragged_grid_of((const void*)kern, groups, t);
        note_grid("xor_copy_mixed_kernel", nb);
        qlaunch(kern, dim3(nb), dim3(256), 0, st, in, v.in_off, out, v.out_off, v.bb, v.code,
                s.codes, s.ncodes, rows_in, rec_rows, status, s.kmax, s.rmax, groups);
    });
    return hipGetLastError();
}

}  // namespace qfec
