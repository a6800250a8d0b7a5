// gf_mixed.h — launch interface of the mixed-code batches (gf_mixed.hip, and the mixed prep in
// decode_prep.hip): every group of a batch names its own (k, m) through an index into a code
// set (qfec_codeset, include/quic_fec.h).  Kept out of fec_kernels.h: only the mixed entry
// points include it, so the uniform, ragged and pointer-table dispatch never sees it.
#pragma once
#include "fec_kernels.h"

namespace qfec {

constexpr int kMixedMaxCodes = 32;   // five configuration bits on the wire

// One code of a set as the kernels read it: a record of a device table that lives as long as
// the set (immutable, so a captured call stays valid).  A unit reads the record of code[g]
// with a wave-uniform index, so the loads are scalar and the table (at most 1 KiB) stays in
// the scalar cache.  The alternative, the records by value in the kernel arguments, is indexed
// at run time too, and the compiler lowers a dynamically indexed by-value array to a private
// copy (scratch), which the run-time-shape kernels have no registers to spare for.
struct MixedCode {
    int32_t k, m;
    int32_t enc_nchunk;   // chunks of the set's encode chunk size over m; 0: no GF encode
                          //   (m == 1, k <= 1 or k + m > 256)
    int32_t dec_nchunk;   // chunks of the set's decode chunk size over min(k, m); 0 likewise
    long long enc_off;    // its encode table [enc_nchunk][k][max(rc, 4)] in the set's buffer
    const uint8_t* cenc;  // [m][k] encode matrix of the decode prep, or null
};

// A set as the launchers take it.
struct MixedSet {
    const MixedCode* codes;   // device, [ncodes]
    // The codes' encode tables, one after the other in one buffer of the set.  The encode kernel
    // takes it as a __restrict__ argument and adds the code's offset, so the coefficient loads
    // are the scalar loads of gf_ragged_kernel; a table address read from the record instead is
    // a pointer of unknown address space, which costs flat loads and their full waits in the
    // block loop.
    const uint8_t* enc_tabs;
    int ncodes;
    int kmax, rmax;           // row strides of rows [G][kmax] and rec_rows / slots [G][rmax]
    int enc_rc, dec_rc;       // output chunk of the whole set (2 or 4), encode and decode
    int enc_nchunk, dec_nchunk;   // the largest chunk count of a code
    long long coef_gstride;   // prep table bytes per group: max of nchunk * k * max(rc, 4)
    int cenc_bytes;           // every decodable code's m * k, each rounded up to 16
    int solve_rmax;           // the largest min(k, m) of a code with k + m <= 256 (the r x r solve)
};

// The packed arrays of a mixed call (device memory).
struct MixedView {
    const uint8_t* code;      // [G] index into the set
    const int32_t* bb;        // [G]
    const long long* in_off;
    const long long* out_off;
};

// The groups the m > 1 encode rejects with status -1 (cauchy_256.cpp:1519-1534): asked by the
// pass that writes their XOR parity and status; the GF kernel skips them by the same rule.
__host__ __device__ inline bool mixed_is_gf(int k, int m) { return k > 1 && m > 1; }
__host__ __device__ inline bool mixed_encode_rejects(int k, int m, int bb) {
    return mixed_is_gf(k, m) && (k + m > 256 || (bb & 7) != 0);
}

// m > 1: unit = (group, chunk) over groups x the set's largest chunk count.  Encode: the
// code's own table; decode: the prep's per-group table, outputs o < nout[g].
hipError_t launch_gf_mixed(const MixedSet& s, MixedView v, const uint8_t* in, uint8_t* out,
                           const uint8_t* coef, const int32_t* nout, long long groups, bool decode,
                           hipStream_t st, const Tune& t);
// Everything else, one wave per group.  Encode: XOR parity of m == 1 and of rejected groups,
// the copies of k <= 1, every group's status (-2 for code[g] >= ncodes).  Decode: the m == 1 and
// k <= 1 groups whole (bookkeeping, rec_rows, status, recovered block), and status -2 with
// rec_rows 255 for code[g] >= ncodes; the m > 1 groups are the prep's.
hipError_t launch_xor_copy_mixed(const MixedSet& s, MixedView v, const uint8_t* in, uint8_t* out,
                                 const uint8_t* rows_in, uint8_t* rec_rows, int32_t* status,
                                 long long groups, bool decode, hipStream_t st, const Tune& t);
// Decode prep of the m > 1 groups (decode_prep.hip): prep_group with the group's own k, m,
// cenc and bb, rows at g * kmax, rec_rows / slots at g * rmax, table at g * coef_gstride.
hipError_t launch_decode_prep_mixed(const MixedSet& s, MixedView v, const PrepIO& io,
                                    long long groups, hipStream_t st, const Tune& t);

}  // namespace qfec
