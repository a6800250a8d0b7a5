// gf_psyn_55.hip — the gf_psyn_kernel variants of FEC_5_5 (gf_psyn.h).
#include "gf_psyn.h"

namespace qfec {
template hipError_t psyn_go<5, 5>(const Apply&, size_t, bool);
}  // namespace qfec
