// gf_colword.h — column-word access of the bit-sliced apply kernels (gf_apply_kernel in
// fec_kernels.hip, the ragged and pointer-table unit in gf_ragged_unit.h).
//
// Word c of sub-row t covers bytes [t*s + 4c, +4); the last word of a sub-row may be partial
// (s % 4 != 0).  Loads of the last word are shifted back inside the sub-row (never past the
// block) and realigned; stores write only the valid bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfec {

typedef uint32_t u32ua __attribute__((aligned(1)));   // unaligned dword (gfx950 unaligned mode)

struct ColAccess {
    int lo;        // byte offset of the dword actually loaded within the sub-row
    int shift;     // right shift (bits) that realigns it
    int nvalid;    // valid bytes of this lane's word (0 = lane idle)
};

template <bool TINY>
__device__ __forceinline__ ColAccess col_access(int c, int nw, int s) {
    ColAccess a;
    const int cc = c < nw ? c : nw - 1;
    const int off = 4 * cc;
    a.nvalid = c < nw ? min(4, s - off) : 0;
    if (!TINY) {
        a.lo = min(off, s - 4);
        a.shift = 8 * (off - a.lo);
    } else {
        a.lo = 0;
        a.shift = 0;
    }
    return a;
}

// TINY = blocks under 32 bytes (s < 4): bytewise, never past the sub-row.  Otherwise the
// raw (unshifted) dword; the caller applies `>> shift`.
template <bool TINY>
__device__ __forceinline__ uint32_t load_raw(const uint8_t* sub, const ColAccess& a, int s) {
    if (!TINY) return *(const u32ua*)(sub + a.lo);
    uint32_t v = 0;
    for (int b = 0; b < 3; ++b)
        if (b < s) v |= (uint32_t)sub[b] << (8 * b);
    return v;
}

__device__ __forceinline__ void store_word(uint8_t* sub, int c, const ColAccess& a, uint32_t v) {
    if (a.nvalid == 4) {
        *(u32ua*)(sub + 4 * c) = v;
    } else if (a.nvalid > 0) {
        for (int b = 0; b < a.nvalid; ++b) sub[4 * c + b] = (uint8_t)(v >> (8 * b));
    }
}

}  // namespace qfec
