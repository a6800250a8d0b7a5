// gf_dcol_e63.hip — gf_dcol_kernel<kDcolS, 6, false, 3> (gf_dcol.h), one instantiation per
// translation unit so the D kernels compile in parallel.
#include "gf_dcol.h"

namespace qfec {
template hipError_t dcol_go<6, false, 3>(const Apply&, unsigned, size_t);
}  // namespace qfec
