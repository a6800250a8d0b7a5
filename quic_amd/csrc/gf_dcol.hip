// gf_dcol.hip — launchers of the config D kernels (gf_dcol.h); the kernel instantiations are
// in gf_dcol_<e|d><depth><cache>.hip, one per translation unit.
#include "gf_dcol.h"

namespace qfec {


bool gf_dcol_supported(int k, int m, int bb, const Tune& t) {
    return t.dcol && t.const_enc && k == 128 && m == 16 && bb == 8 * kDcolS;
}

// Ring depth, LDS bytes and grid of either launch.  A CU holds 2 workgroups of 4 waves by
// registers (<= 256 VGPRs), LDS permitting.  Units are column tiles; oversubscribed at about
// dcol_wg units per wave.  False: invalid.
static bool dcol_shape(const Apply& a, int* D, size_t* lds, unsigned* grid) {
    const Tune& t = *a.t;
    *D = t.dcol_depth;
    if (*D != 6 && *D != 8) return false;
    *lds = (size_t)kDcWaves * (*D + 1) * DcShape<kDcolS>::BUFB;
    *grid = persistent_grid(a.groups * DcShape<kDcolS>::NT, kDcWaves,
                            (long long)t.cus * lds_blocks_per_cu(*lds, 2), t.dcol_wg, t.dcol_grid);
    return *grid != 0;
}

hipError_t launch_gf_dcol_encode(const Apply& a) {
    if (a.groups <= 0) return hipSuccess;
    if (!gf_dcol_supported(a.k, a.m, a.bb, *a.t) || ((uintptr_t)a.in & 15) != 0)
        return hipErrorInvalidValue;
    int D;
    size_t lds;
    unsigned grid;
    if (!dcol_shape(a, &D, &lds, &grid)) return hipErrorInvalidValue;
    note_kernel("gf_dcol_kernel<encode,k128m16>");
    note_grid("gf_dcol_kernel<encode>", grid);
    // cached loads and stores: the parity's partial cache lines at tile edges merge in L2
    // instead of going to HBM twice (D encode 20.3 -> 16.5 ms; non-temporal loads too: 21.7
    // ms)
    return D == 8 ? dcol_go<8, false, 3>(a, grid, lds) : dcol_go<6, false, 3>(a, grid, lds);
}

hipError_t launch_gf_dcol_syndrome(const Apply& a) {
    if (a.groups <= 0) return hipSuccess;
    if (!gf_dcol_supported(a.k, a.m, a.bb, *a.t) || a.rmax > 16 || a.tab_gstride < syn::kBytes)
        return hipErrorInvalidValue;
    if ((((uintptr_t)a.in) & 15) || ((((uintptr_t)a.tab) | (uintptr_t)a.tab_gstride |
                                       (uintptr_t)a.cenc | (uintptr_t)a.slots) & 3))
        return hipErrorInvalidValue;
    int D;
    size_t lds;
    unsigned grid;
    if (!dcol_shape(a, &D, &lds, &grid)) return hipErrorInvalidValue;
    note_kernel("gf_dcol_kernel<decode,k128m16>");
    note_grid("gf_dcol_kernel<decode>", grid);
    // decode: non-temporal loads, plain stores (cached loads: 1.011x instead of 1.167x the
    // algorithmic reads, but 18.3 vs 16.9 ms and the next encode over-reads)
    return D == 8 ? dcol_go<8, true, 2>(a, grid, lds) : dcol_go<6, true, 2>(a, grid, lds);
}

}  // namespace qfec
