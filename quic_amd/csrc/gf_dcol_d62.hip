// gf_dcol_d62.hip — gf_dcol_kernel<kDcolS, 6, true, 2> (gf_dcol.h), one instantiation per
// translation unit so the D kernels compile in parallel.
#include "gf_dcol.h"

namespace qfec {
template hipError_t dcol_go<6, true, 2>(const Apply&, unsigned, size_t);
}  // namespace qfec
