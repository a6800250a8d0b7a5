// gf_ptrs.h — launch interface of the pointer-table batches (gf_ptrs.hip): the ragged kernels
// (fec_kernels.h) with every block at an address of its own.
#pragma once
#include "fec_kernels.h"

namespace qfec {

// in [G][k] and out [G][m] (encode) or [G][min(k, m)] (decode) are device arrays of device
// addresses; bb [G], or null: every group has bb_all.  Nothing is read back to the host.
struct PtrsView {
    const unsigned long long* in;
    const unsigned long long* out;
    const int32_t* bb;
    int bb_all;
};
// As launch_gf_ragged; a.in and a.out are not read.
hipError_t launch_gf_ptrs(const Apply& a, PtrsView v, int nchunk, bool decode);
// As launch_xor_ragged; group g's output is out[g * ostride].
hipError_t launch_xor_ptrs(PtrsView v, const uint8_t* eidx, int32_t* status, int k, int ostride,
                           long long groups, bool decode, int mode, hipStream_t st,
                           const Tune& t);
// As launch_copy_ragged.
hipError_t launch_copy_ptrs(PtrsView v, const uint8_t* rows_in, uint8_t* rec_rows,
                            int32_t* status, int k, int m, long long groups, bool decode,
                            hipStream_t st, const Tune& t);
// launch_ragged_decode_status over v.bb; without a size array the same fix-up for bb_all.
hipError_t launch_ptrs_decode_status(PtrsView v, const uint8_t* rows_in, uint8_t* rec_rows,
                                     int32_t* status, int32_t* nout, int k, int rmax,
                                     long long groups, hipStream_t st);

}  // namespace qfec
