// fec_host_plan.h — host-only arithmetic of the host-pointer batches (no GPU, no HIP): the
// packed layout (qfec_ragged_layout, include/quic_fec.h), the batching queue's packing of
// queued groups into it, and the staging plan of fec_host.cpp's pipeline: the list of staged
// arrays an entry point declares, the chunks a batch is cut into, and the carve of one chunk's
// staging buffer.  tools/ragged_pack_check.cpp links these without the rest of the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
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

// One array a host-pointer batch stages on the device, stated once.  Its bytes for the groups
// [g0, g0 + n) of a chunk: dense, n * per_group; or packed, the span from group g0's offset to
// the end of the chunk's last group (nblk blocks of bb[g] bytes at off[g]; nblk_g: a count per
// group instead, the mixed-code batches').  `src` is the host
// array copied in before the kernels, `dst` the one copied out after them (both: the caller's
// bytes are staged in, so what the kernels leave unwritten returns as it was; neither: the
// array lives on the device only).  An absent stage is a null device pointer and zero bytes.
struct Stage {
    bool present = true;
    size_t per_group = 0;              // dense
    const long long* off = nullptr;    // packed: [G], ascending
    int nblk = 0;
    const int* nblk_g = nullptr;       // packed: [G] blocks per group, instead of nblk
    const void* src = nullptr;
    void* dst = nullptr;
    size_t row_pitch = 0, row_width = 0;   // copy out only row_width bytes of every row_pitch
    // this chunk's sub-buffer (stage_carve)
    uint8_t* dev = nullptr;
    size_t bytes = 0;

    Stage& in(const void* h) { src = h; return *this; }
    Stage& out(void* h) { dst = h; return *this; }
    Stage& rows(size_t pitch, size_t width) { row_pitch = pitch; row_width = width; return *this; }
    template <class T> T* as() const { return (T*)dev; }
    long long blocks(long long g) const { return nblk_g ? nblk_g[g] : nblk; }
    // where the chunk that starts at group g0 begins in a host array of this stage
    size_t host_at(long long g0) const { return off ? (size_t)off[g0] : (size_t)g0 * per_group; }
};

struct StageList {
    static constexpr int kMax = 16;
    const int* bb = nullptr;   // [G] block sizes, for the packed stages
    Stage s[kMax];
    int n = 0;
    Stage& dense(size_t per_group, bool present = true) {
        Stage& st = add();
        st.present = present;
        st.per_group = present ? per_group : 0;
        return st;
    }
    Stage& packed(const long long* off, int nblk) {
        Stage& st = add();
        st.off = off;
        st.nblk = nblk;
        return st;
    }
    Stage& packed(const long long* off, const int* nblk_g) {
        Stage& st = add();
        st.off = off;
        st.nblk_g = nblk_g;
        return st;
    }
    Stage& add() {
        if (n == kMax) abort();   // a longer list is a bug in the entry point, not an input
        return s[n++];
    }
};

// A batch cut into chunks of whole groups: chunk i = groups [begin(i), begin(i + 1)).
struct Chunks {
    long long groups = 0;
    long long uniform = 0;            // > 0: every chunk holds this many groups, the last the rest
    std::vector<long long> first;     // else: begin(i), and `groups` at the end
    // ragged: [G] offsets relative to the chunk's first group
    std::vector<long long> in_rel, out_rel;
    long long count() const {
        return uniform ? (groups + uniform - 1) / uniform : (long long)first.size() - 1;
    }
    long long begin(long long i) const {
        return uniform ? (i * uniform < groups ? i * uniform : groups) : first[(size_t)i];
    }
};

// Bytes the present stages hold for the groups [g0, g0 + n), without alignment padding.
size_t stage_bytes(const StageList& L, long long g0, long long n);

// Cuts consecutive 256-byte aligned sub-buffers for the groups [g0, g0 + n) out of `base`, in
// declaration order: sets every stage's dev / bytes and returns the bytes used.
size_t stage_carve(StageList& L, long long g0, long long n, uint8_t* base);

// The staging one buffer needs: the largest carve over the chunks.
size_t staging_bytes(StageList& L, const Chunks& ch);

// Uniform batches: host_chunk_mb MiB per chunk, but at least host_min_groups groups (up to
// 2 GiB of staging), and at least one group.
long long uniform_chunk(long long groups, size_t per_group, int host_chunk_mb, int host_min_groups);

// Ragged batches: validates bb and the offsets of the packed stages `in` and `out` (-2 and a
// message), then cuts by bytes on group boundaries (a chunk holds at least one group) and
// fills in_rel / out_rel.
int ragged_chunks(const StageList& L, const Stage& in, const Stage& out, long long groups,
                  long long target_bytes, Chunks* ch, const char** msg);

// The receiver window's one device allocation (qfec_rxwin_create, include/quic_fec.h): byte
// offsets of its sections, each rounded up to 256 bytes, in this order.  With S = groups * (k + m)
// slots and rmax = min(k, m): the hold rows S * hold_stride; the carried state: slot_state int32
// [S], held int32 [G], delivered int32 [G]; the per-push tables: arr_at and pre_at int32 [S], rows
// u8 [G][k], blk_ptrs u64 [G * k], rec_ptrs u64 [G * rmax], eff (the effective bb) and verdict
// int32 [G].  total: their sum, what qfec_rxwin_bytes reports.
struct RxwinLayout {
    long long hold, slot_state, held, delivered, arr_at, pre_at, rows, blk_ptrs, rec_ptrs, eff,
        verdict, total;
};
// 0, or -2 with *why (may be null) naming the limit: k, m < 1, k > 255, groups < 0, k + m > 255,
// groups * (k + m) > INT32_MAX, hold_stride < 16 or not a multiple of 16, a total past 2^62.
int rxwin_layout(int k, int m, long long groups, int hold_stride, RxwinLayout* L,
                 const char** why);

}  // namespace qfec
