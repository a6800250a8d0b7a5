// fec_ragged_host.cpp — host-only part of the ragged batches: the packed layout and the
// queue's packing.  Plain C++ (no HIP), so the sanitizer check under tools/ links it alone.
#include "fec_ragged_host.h"

#include <cstring>

#include "../../include/quic_fec.h"

namespace {

// running = roundup16(running + n * bb); false on overflow
bool advance(long long* running, long long n, long long bb) {
    long long bytes, end;
    if (__builtin_mul_overflow(n, bb, &bytes)) return false;
    if (__builtin_add_overflow(*running, bytes, &end)) return false;
    if (__builtin_add_overflow(end, 15LL, &end)) return false;
    *running = end & ~15LL;
    return true;
}

}  // namespace

extern "C" int qfec_ragged_layout(int k, int m, long long groups, const int* bb,
                                  long long* data_off, long long* par_off, long long* rec_off,
                                  long long totals[3]) {
    if (k < 1 || m < 1 || groups < 0 || (groups && !bb)) return -2;
    const long long nblk[3] = {k, m, k < m ? k : m};
    long long* const off[3] = {data_off, par_off, rec_off};
    long long run[3] = {0, 0, 0};
    for (long long g = 0; g < groups; ++g) {
        if (bb[g] < 1) return -2;
        for (int a = 0; a < 3; ++a) {
            if (off[a]) off[a][g] = run[a];
            if (!advance(&run[a], nblk[a], bb[g])) return -2;
        }
    }
    if (totals)
        for (int a = 0; a < 3; ++a) totals[a] = run[a];
    return 0;
}

namespace qfec {

int ragged_pack(int k, int m, bool decode, const std::vector<const unsigned char*>& blocks,
                const std::vector<int>& bb, RaggedPack* p) {
    const size_t G = blocks.size();
    if (bb.size() != G || !p) return -2;
    p->bb = bb;
    p->in_off.assign(G, 0);
    p->out_off.assign(G, 0);
    long long totals[3] = {0, 0, 0};
    const int r = qfec_ragged_layout(k, m, (long long)G, bb.data(), p->in_off.data(),
                                     decode ? nullptr : p->out_off.data(),
                                     decode ? p->out_off.data() : nullptr, totals);
    if (r) return r;
    p->in.resize((size_t)totals[0]);
    p->out.assign((size_t)totals[decode ? 2 : 1], 0);
    for (size_t g = 0; g < G; ++g)
        memcpy(p->in.data() + p->in_off[g], blocks[g], (size_t)k * bb[g]);
    return 0;
}

}  // namespace qfec
