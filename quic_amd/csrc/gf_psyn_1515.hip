// gf_psyn_1515.hip — the gf_psyn_kernel variants of FEC_15_15 (gf_psyn.h).
#include "gf_psyn.h"

namespace qfec {
template hipError_t psyn_go<15, 15>(const Apply&, size_t, bool);
}  // namespace qfec
