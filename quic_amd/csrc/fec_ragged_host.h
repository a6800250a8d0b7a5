// fec_ragged_host.h — host-only helpers of the ragged batches (no GPU, no HIP): the packed
// layout (qfec_ragged_layout, include/quic_fec.h) and the batching queue's packing of queued
// groups into it.  tools/ragged_pack_check.cpp links these without the rest of the library.
#pragma once
#include <vector>

namespace qfec {

// One flush of a ragged (k, m) bucket, packed for qfec_*_batch_ragged*_host.
struct RaggedPack {
    std::vector<int> bb;                 // [G]
    std::vector<long long> in_off;       // [G] the group's k blocks in `in`
    std::vector<long long> out_off;      // [G] its m parity (encode) / min(k, m) recovered blocks
    std::vector<unsigned char> in, out;  // the packed buffers (`out` zeroed)
};

// Packs G groups: group g's k blocks of bb[g] bytes (blocks[g], contiguous) are copied to
// p->in + p->in_off[g]; p->out is sized for the outputs (decode: min(k, m) blocks per group,
// encode: m) and zeroed.  Returns 0, or -2 for a bad size.
int ragged_pack(int k, int m, bool decode, const std::vector<const unsigned char*>& blocks,
                const std::vector<int>& bb, RaggedPack* p);

}  // namespace qfec
