// fec_host_plan.cpp — host-only part of the host-pointer batches: the packed layout, the
// queue's packing, and the staging plan (stages, chunks, carve).  Plain C++ (no HIP), so the
// sanitizer check under tools/ links it alone.
#include "fec_host_plan.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

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

// *end = off + n * bb; false on overflow
bool block_end(long long off, long long n, long long bb, long long* end) {
    long long bytes;
    return !__builtin_mul_overflow(n, bb, &bytes) && !__builtin_add_overflow(off, bytes, end);
}

size_t one_stage_bytes(const qfec::StageList& L, const qfec::Stage& s, long long g0, long long n) {
    if (!s.present) return 0;
    if (!s.off) return (size_t)n * s.per_group;
    const long long last = g0 + n - 1;
    return (size_t)(s.off[last] + s.blocks(last) * L.bb[last] - s.off[g0]);
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

// qfec_ragged_layout with the block counts of each group's own code.
extern "C" int qfec_mixed_layout(int ncodes, const int* k, const int* m, long long groups,
                                 const unsigned char* code, const int* bb, long long* data_off,
                                 long long* par_off, long long* rec_off, long long totals[3]) {
    if (ncodes < 1 || ncodes > 32 || !k || !m || groups < 0 || (groups && (!code || !bb)))
        return -2;
    for (int c = 0; c < ncodes; ++c)
        if (k[c] < 1 || k[c] > 255 || m[c] < 1) return -2;
    long long* const off[3] = {data_off, par_off, rec_off};
    long long run[3] = {0, 0, 0};
    for (long long g = 0; g < groups; ++g) {
        if (code[g] >= ncodes || bb[g] < 1) return -2;
        const int kg = k[code[g]], mg = m[code[g]];
        const long long nblk[3] = {kg, mg, kg < mg ? kg : mg};
        for (int a = 0; a < 3; ++a) {
            if (off[a]) off[a][g] = run[a];
            if (!advance(&run[a], nblk[a], bb[g])) return -2;
        }
    }
    if (totals)
        for (int a = 0; a < 3; ++a) totals[a] = run[a];
    return 0;
}

// The block size getRedundancyPackets gives a group (quic_fec_group.cc:344-352): the largest
// prefixed payload, rounded up to 8; then qfec_ragged_layout's offsets.
extern "C" int qfec_framed_layout(int k, int m, long long groups, const int* pay_len, int* bb,
                                  long long* data_off, long long* par_off, long long* rec_off,
                                  long long totals[3]) {
    if (k < 1 || m < 1 || groups < 0 || (groups && (!pay_len || !bb))) return -2;
    for (long long g = 0; g < groups; ++g) {
        int most = 0;
        for (int i = 0; i < k; ++i) {
            const int len = pay_len[g * k + i];
            if (len < 0 || len > 0x3fff) return -2;
            most = std::max(most, len);
        }
        bb[g] = (most + 2 + 7) & ~7;
    }
    return qfec_ragged_layout(k, m, groups, bb, data_off, par_off, rec_off, totals);
}

// The block size getRevivedPackets gives a group (quic_fec_group.cc:264-265): the largest
// packet it stored, a data packet with its 2-byte prefix, an FEC packet as it is.
extern "C" int qfec_framed_rx_block_bytes(int k, int m, long long groups, const int* pkt_len,
                                          const int* ad_len, int ad_len_all, int* bb) {
    if (k < 1 || m < 1 || groups < 0 || (groups && (!pkt_len || !bb))) return -2;
    const long long per = (long long)k + m;
    for (long long g = 0; g < groups; ++g) {
        long long most = 0;
        for (long long i = 0; i < per; ++i) {
            const long long p = g * per + i;
            const long long tl = pkt_len[p], al = ad_len ? ad_len[p] : ad_len_all;
            if (tl < 0 || al < 0 || tl - al < 12) continue;   // not received, or no packet
            most = std::max(most, tl - al - 12 + (i < k ? 2 : 0));
        }
        bb[g] = (int)std::min<long long>(most, 0x7fffffffLL);
    }
    return 0;
}

// The same size for packets that lie in arrival order: QuicFecGroup stores the first copy of an
// index (quic_fec_group.cc:167-169) until it holds k packets (:210-213), so only a group's first
// k distinct arrivals count.  By lengths alone, as above: whether a packet opens is the device's.
extern "C" int qfec_arrivals_rx_block_bytes(int k, int m, long long groups, long long n,
                                            const int* arr_group, const unsigned char* arr_index,
                                            const int* pkt_len, const int* ad_len, int ad_len_all,
                                            int* bb) {
    if (k < 1 || m < 1 || k + m > 255 || groups < 0 || n < 0 || (groups && !bb) ||
        (n && (!arr_group || !arr_index || !pkt_len)))
        return -2;
    const long long per = (long long)k + m;
    long long slots;
    if (__builtin_mul_overflow(groups, per, &slots)) return -2;
    std::vector<unsigned char> seen;
    std::vector<int> held;
    try {
        seen.assign((size_t)slots, 0);
        held.assign((size_t)groups, 0);
    } catch (const std::bad_alloc&) {
        return -2;
    }
    for (long long g = 0; g < groups; ++g) bb[g] = 0;
    for (long long a = 0; a < n; ++a) {
        const long long g = arr_group[a];
        const int i = arr_index[a];
        if (g < 0 || g >= groups || i >= per) continue;   // no packet of this batch
        const long long tl = pkt_len[a], al = ad_len ? ad_len[a] : ad_len_all;
        if (tl < 0 || al < 0 || tl - al < 12) continue;    // no packet
        if (seen[(size_t)(g * per + i)] || held[(size_t)g] >= k) continue;   // duplicate, late
        seen[(size_t)(g * per + i)] = 1;
        ++held[(size_t)g];
        const long long size = tl - al - 12 + (i < k ? 2 : 0);
        bb[g] = (int)std::max<long long>(bb[g], std::min<long long>(size, 0x7fffffffLL));
    }
    return 0;
}

// The same with the state in the caller's hands, so that a stream can be fed in pieces: seen
// [groups][32] is a bitset of the indices counted so far (bit i of a group: byte i / 8, bit
// i % 8), bb [groups] the running maximum over the group's first k distinct indices.  Both are
// in/out; a group's entries are zeroed by the caller when it releases the group.  Over the
// pieces of a stream, from zeroed state, bb ends as qfec_arrivals_rx_block_bytes gives it over
// their concatenation.
extern "C" int qfec_arrivals_rx_block_bytes_carry(int k, int m, long long groups, long long n,
                                                  const int* arr_group,
                                                  const unsigned char* arr_index,
                                                  const int* pkt_len, const int* ad_len,
                                                  int ad_len_all, unsigned char* seen, int* bb) {
    if (k < 1 || m < 1 || k + m > 255 || groups < 0 || n < 0 || (groups && (!bb || !seen)) ||
        (n && (!arr_group || !arr_index || !pkt_len)))
        return -2;
    const int per = k + m;
    for (long long a = 0; a < n; ++a) {
        const long long g = arr_group[a];
        const int i = arr_index[a];
        if (g < 0 || g >= groups || i >= per) continue;   // no packet of this window
        const long long tl = pkt_len[a], al = ad_len ? ad_len[a] : ad_len_all;
        if (tl < 0 || al < 0 || tl - al < 12) continue;    // no packet
        unsigned char* sg = seen + g * 32;
        int held = 0;
        for (int b = 0; b < 32; ++b) held += __builtin_popcount(sg[b]);
        if (((sg[i >> 3] >> (i & 7)) & 1) || held >= k) continue;   // duplicate, late
        sg[i >> 3] = (unsigned char)(sg[i >> 3] | (1u << (i & 7)));
        const long long size = tl - al - 12 + (i < k ? 2 : 0);
        bb[g] = (int)std::max<long long>(bb[g], std::min<long long>(size, 0x7fffffffLL));
    }
    return 0;
}

// ---- the receiver window's allocation
int qfec::rxwin_layout(int k, int m, long long groups, int hold_stride, RxwinLayout* L,
                       const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (k < 1 || m < 1 || groups < 0) return *why = "bad k / m / groups", -2;
    if (k > 255) return *why = "k > 255 cannot be tagged by an 8-bit row", -2;
    if (k + m > 255) return *why = "k + m > 255", -2;
    const long long per = k + m, rmax = std::min(k, m);
    if (groups > 0x7fffffffLL / per) return *why = "groups * (k + m) above INT32_MAX", -2;
    if (hold_stride < 16 || hold_stride % 16)
        return *why = "hold_stride must be a multiple of 16, at least 16", -2;
    const long long S = groups * per;   // < 2^31, so every product below stays under 2^62
    long long at = 0;
    const auto take = [&](long long bytes) {
        const long long here = at;
        at += (bytes + 255) & ~255LL;
        return here;
    };
    L->hold = take(S * hold_stride);
    L->slot_state = take(S * 4);
    L->held = take(groups * 4);
    L->delivered = take(groups * 4);
    L->arr_at = take(S * 4);
    L->pre_at = take(S * 4);
    L->rows = take(groups * k);
    L->blk_ptrs = take(groups * k * 8);
    L->rec_ptrs = take(groups * rmax * 8);
    L->eff = take(groups * 4);
    L->verdict = take(groups * 4);
    L->total = at;
    return 0;
}

extern "C" int qfec_rxwin_bytes(int k, int m, long long groups, int hold_stride,
                                long long* bytes) {
    qfec::RxwinLayout L;
    if (!bytes || qfec::rxwin_layout(k, m, groups, hold_stride, &L, nullptr)) return -2;
    *bytes = L.total;
    return 0;
}

// ---- the packet geometry of a mixed-code batch: with a code per group, packet p no longer
// belongs to group p / (k + m), so the wire calls take two prefix tables.
static bool mixed_codes_ok(int ncodes, const int* k, const int* m) {
    if (ncodes < 1 || ncodes > 32 || !k || !m) return false;
    for (int c = 0; c < ncodes; ++c)
        if (k[c] < 1 || k[c] > 255 || m[c] < 1) return false;
    return true;
}

extern "C" int qfec_mixed_packet_layout(int ncodes, const int* k, const int* m, long long groups,
                                        const unsigned char* code, int* pkt_first,
                                        int* pay_first) {
    if (!mixed_codes_ok(ncodes, k, m) || groups < 0 || (groups && !code)) return -2;
    long long pkt = 0, pay = 0;
    for (long long g = 0; g < groups; ++g) {
        if (pkt_first) pkt_first[g] = (int)pkt;
        if (pay_first) pay_first[g] = (int)pay;
        if (code[g] >= ncodes) continue;   // no code: an empty span in both tables
        pkt += (long long)k[code[g]] + m[code[g]];
        pay += k[code[g]];
        if (pkt > 0x7fffffffLL) return -2;   // pay <= pkt
    }
    if (pkt_first) pkt_first[groups] = (int)pkt;
    if (pay_first) pay_first[groups] = (int)pay;
    return 0;
}

// qfec_framed_layout with each group's own k lengths, at pay_first[g] (null: the dense table
// qfec_mixed_packet_layout gives); then qfec_mixed_layout's offsets.
extern "C" int qfec_framed_layout_mixed(int ncodes, const int* k, const int* m, long long groups,
                                        const unsigned char* code, const int* pay_first,
                                        long long npay, const int* pay_len, int* bb,
                                        long long* data_off, long long* par_off,
                                        long long* rec_off, long long totals[3]) {
    if (!mixed_codes_ok(ncodes, k, m) || groups < 0 || npay < 0 ||
        (groups && (!code || !bb || !pay_len)))
        return -2;
    long long run = 0;
    for (long long g = 0; g < groups; ++g) {
        if (code[g] >= ncodes) return -2;
        const int kg = k[code[g]];
        const long long at = pay_first ? pay_first[g] : run;
        if (at < 0 || at > npay - kg) return -2;   // the group's lengths lie outside pay_len
        run = at + kg;
        int most = 0;
        for (int i = 0; i < kg; ++i) {
            const int len = pay_len[at + i];
            if (len < 0 || len > 0x3fff) return -2;
            most = std::max(most, len);
        }
        bb[g] = (most + 2 + 7) & ~7;
    }
    return qfec_mixed_layout(ncodes, k, m, groups, code, bb, data_off, par_off, rec_off, totals);
}

// qfec_arrivals_rx_block_bytes with k and k + m of the arrival's own group.
extern "C" int qfec_arrivals_rx_block_bytes_mixed(int ncodes, const int* k, const int* m,
                                                  long long groups, const unsigned char* code,
                                                  long long n, const int* arr_group,
                                                  const unsigned char* arr_index,
                                                  const int* pkt_len, const int* ad_len,
                                                  int ad_len_all, int* bb) {
    if (!mixed_codes_ok(ncodes, k, m) || groups < 0 || n < 0 || (groups && (!bb || !code)) ||
        (n && (!arr_group || !arr_index || !pkt_len)))
        return -2;
    for (int c = 0; c < ncodes; ++c)
        if (k[c] + (long long)m[c] > 255) return -2;
    // an index is a byte: 256 slots per group hold every tag
    std::vector<unsigned char> seen;
    std::vector<int> held;
    try {
        if (groups > 0x7fffffffLL) return -2;
        seen.assign((size_t)groups * 256, 0);
        held.assign((size_t)groups, 0);
    } catch (const std::bad_alloc&) {
        return -2;
    }
    for (long long g = 0; g < groups; ++g) bb[g] = 0;
    for (long long a = 0; a < n; ++a) {
        const long long g = arr_group[a];
        const int i = arr_index[a];
        if (g < 0 || g >= groups || code[g] >= ncodes) continue;   // no group, or one without a code
        const int kg = k[code[g]], per = kg + m[code[g]];
        if (i >= per) continue;                                     // no packet of this group
        const long long tl = pkt_len[a], al = ad_len ? ad_len[a] : ad_len_all;
        if (tl < 0 || al < 0 || tl - al < 12) continue;             // no packet
        if (seen[(size_t)(g * 256 + i)] || held[(size_t)g] >= kg) continue;   // duplicate, late
        seen[(size_t)(g * 256 + i)] = 1;
        ++held[(size_t)g];
        const long long size = tl - al - 12 + (i < kg ? 2 : 0);
        bb[g] = (int)std::max<long long>(bb[g], std::min<long long>(size, 0x7fffffffLL));
    }
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

size_t stage_bytes(const StageList& L, long long g0, long long n) {
    size_t sum = 0;
    for (int i = 0; i < L.n; ++i) sum += one_stage_bytes(L, L.s[i], g0, n);
    return sum;
}

size_t stage_carve(StageList& L, long long g0, long long n, uint8_t* base) {
    size_t at = 0;
    for (int i = 0; i < L.n; ++i) {
        Stage& s = L.s[i];
        s.bytes = one_stage_bytes(L, s, g0, n);
        s.dev = s.present && base ? base + at : nullptr;   // no base: sizes only
        if (s.present) at += (s.bytes + 255) & ~(size_t)255;
    }
    return at;
}

size_t staging_bytes(StageList& L, const Chunks& ch) {
    size_t most = 0;
    for (long long i = 0; i < ch.count(); ++i)
        most = std::max(most, stage_carve(L, ch.begin(i), ch.begin(i + 1) - ch.begin(i), nullptr));
    return most;
}

long long uniform_chunk(long long groups, size_t per_group, int host_chunk_mb,
                        int host_min_groups) {
    // at least host_min_groups groups per chunk (up to 2 GiB of staging per buffer): a
    // 64 MiB chunk of D's 1.2 MB groups is 54 groups, too few to fill the device (D at
    // 16,384 groups: 16.1 GiB/s with 64 MiB chunks, 22.9 with 256 MiB, 23.3 with 1 GiB).
    // Both are options, so a caller (and the tests) can still force small chunks.
    const size_t target = (size_t)std::max(1, host_chunk_mb) << 20;
    const long long by_bytes = (long long)(target / per_group);
    const long long floor_g = std::min<long long>(std::max(1, host_min_groups),
                                                  (long long)((2ull << 30) / per_group));
    return std::max<long long>(1, std::min<long long>(groups, std::max(by_bytes, floor_g)));
}

int ragged_chunks(const StageList& L, const Stage& in, const Stage& out, long long G,
                  long long target, Chunks* ch, const char** msg) {
    const int* bb = L.bb;
    long long in_end = 0, out_end = 0;   // ends of group g - 1
    for (long long g = 0; g < G; ++g) {
        if (bb[g] < 1) return *msg = "bb[g] < 1", -2;
        if (in.off[g] < 0 || out.off[g] < 0 || ((in.off[g] | out.off[g]) & 15))
            return *msg = "ragged offsets must be non-negative multiples of 16", -2;
        if ((g && (in.off[g] < in_end || out.off[g] < out_end)) ||
            !block_end(in.off[g], in.blocks(g), bb[g], &in_end) ||
            !block_end(out.off[g], out.blocks(g), bb[g], &out_end))
            return *msg = "host ragged batches need ascending, non-overlapping offsets", -2;
    }
    ch->groups = G;
    ch->in_rel.resize((size_t)G);
    ch->out_rel.resize((size_t)G);
    long long g0 = 0;
    ch->first.push_back(0);
    for (long long g = 0; g < G; ++g) {
        if (g > g0 && (long long)stage_bytes(L, g0, g + 1 - g0) > target) {
            g0 = g;
            ch->first.push_back(g);
        }
        ch->in_rel[(size_t)g] = in.off[g] - in.off[g0];
        ch->out_rel[(size_t)g] = out.off[g] - out.off[g0];
    }
    ch->first.push_back(G);
    return 0;
}

}  // namespace qfec
