// gf_psyn_1015.hip — the gf_psyn_kernel variants of FEC_10_15 (gf_psyn.h).
#include "gf_psyn.h"

namespace qfec {
template hipError_t psyn_go<10, 15>(const Apply&, size_t, bool);
}  // namespace qfec
