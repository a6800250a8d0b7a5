// ragged_pack_check — host-code sanitizer check of the ragged layout, the queue's packing and
// the staging plan of the host-pointer batches.
//
// Stand-alone (its own main, no GPU, no HIP): built from this file and
// quic_amd/csrc/fec_host_plan.cpp with -fsanitize=address,undefined (`make ragged-check`).
// It calls qfec_ragged_layout, qfec::ragged_pack and the planning functions of the host
// pipeline (chunks, stage sizes, carve) on random sizes and checks offsets and bounds, and the
// two helpers of the framed calls (qfec_framed_layout, qfec_framed_rx_block_bytes) on hostile
// inputs: zero groups, every packet absent, the largest length, offsets past 2^40, and the helper
// of the arrival-order receiver (qfec_arrivals_rx_block_bytes): duplicates, more than k arrivals,
// tags outside the batch, no arrival, a tag at the last group; and the layout of the mixed-code
// batches (qfec_mixed_layout): ragged counts per group, hostile code indices, G = 0;
// out-of-bounds copies or overflowing arithmetic abort under the sanitizers.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fec_host_plan.h"
#include "quic_fec.h"

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

static long long up16(long long v) { return (v + 15) & ~15LL; }

static void check_layout(int k, int m, const std::vector<int>& bb) {
    const long long G = (long long)bb.size();
    std::vector<long long> d(G), p(G), r(G);
    long long tot[3] = {-1, -1, -1};
    CHECK(qfec_ragged_layout(k, m, G, bb.data(), d.data(), p.data(), r.data(), tot) == 0);
    const int n[3] = {k, m, k < m ? k : m};
    const std::vector<long long>* off[3] = {&d, &p, &r};
    for (int a = 0; a < 3; ++a) {
        long long run = 0;
        for (long long g = 0; g < G; ++g) {
            CHECK((*off[a])[g] == run);
            CHECK((*off[a])[g] % 16 == 0);
            run = up16(run + (long long)n[a] * bb[g]);
        }
        CHECK(tot[a] == run);
    }
    // any output may be NULL
    CHECK(qfec_ragged_layout(k, m, G, bb.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    long long tot2[3];
    CHECK(qfec_ragged_layout(k, m, G, bb.data(), nullptr, p.data(), nullptr, tot2) == 0);
    CHECK(tot2[0] == tot[0] && tot2[1] == tot[1] && tot2[2] == tot[2]);
}

static void check_pack(int k, int m, bool decode, const std::vector<int>& bb, std::mt19937& rng) {
    const size_t G = bb.size();
    // every group's blocks in an allocation of exactly its size: a copy past it is caught
    std::vector<std::vector<unsigned char>> src(G);
    std::vector<const unsigned char*> ptr(G);
    for (size_t g = 0; g < G; ++g) {
        src[g].resize((size_t)k * bb[g]);
        for (auto& b : src[g]) b = (unsigned char)rng();
        ptr[g] = src[g].data();
    }
    qfec::RaggedPack pk;
    // stale content from an earlier, larger flush must not matter
    pk.in.assign(1 << 16, 0xEE);
    pk.out.assign(1 << 16, 0xEE);
    CHECK(qfec::ragged_pack(k, m, decode, ptr, bb, &pk) == 0);
    CHECK(pk.bb == bb);
    CHECK(pk.in_off.size() == G && pk.out_off.size() == G);
    const int nout = decode ? (k < m ? k : m) : m;
    long long in_end = 0, out_end = 0;
    for (size_t g = 0; g < G; ++g) {
        CHECK(pk.in_off[g] % 16 == 0 && pk.out_off[g] % 16 == 0);
        CHECK(pk.in_off[g] >= in_end && pk.out_off[g] >= out_end);   // ascending, no overlap
        in_end = pk.in_off[g] + (long long)k * bb[g];
        out_end = pk.out_off[g] + (long long)nout * bb[g];
        CHECK(in_end <= (long long)pk.in.size());
        CHECK(out_end <= (long long)pk.out.size());
        CHECK(memcmp(pk.in.data() + pk.in_off[g], src[g].data(), src[g].size()) == 0);
    }
    CHECK((long long)pk.in.size() == up16(in_end));
    CHECK((long long)pk.out.size() == up16(out_end));
    for (unsigned char b : pk.out) CHECK(b == 0);
}

namespace qfec { struct Chunks; struct Stage; struct StageList; }
static void check_carve(qfec::StageList& L, const qfec::Chunks& ch);

// ---- qfec_mixed_layout: the block counts of each group's own code, in arrays of exactly G
// entries; hostile code indices, sizes and sets; G = 0
static void check_mixed_layout(std::mt19937& rng) {
    const int ks[] = {10, 1, 2, 3, 5, 32, 10, 250, 250}, ms[] = {1, 3, 2, 2, 5, 4, 20, 5, 7};
    const int nc = 9;
    for (int rep = 0; rep < 60; ++rep) {
        const long long G = rep == 0 ? 0 : 1 + (long long)(rng() % 200);
        std::vector<unsigned char> code((size_t)G);
        std::vector<int> bb((size_t)G);
        for (auto& c : code) c = (unsigned char)(rng() % nc);
        for (auto& b : bb) b = 1 + (int)(rng() % 2100);
        std::vector<long long> d((size_t)G), p((size_t)G), r((size_t)G);
        long long tot[3] = {-1, -1, -1};
        CHECK(qfec_mixed_layout(nc, ks, ms, G, code.data(), bb.data(), d.data(), p.data(), r.data(),
                                tot) == 0);
        long long run[3] = {0, 0, 0};
        for (long long g = 0; g < G; ++g) {
            const int k = ks[code[(size_t)g]], m = ms[code[(size_t)g]];
            const int n[3] = {k, m, k < m ? k : m};
            const long long got[3] = {d[(size_t)g], p[(size_t)g], r[(size_t)g]};
            for (int a = 0; a < 3; ++a) {
                CHECK(got[a] == run[a] && got[a] % 16 == 0);
                run[a] = up16(run[a] + (long long)n[a] * bb[(size_t)g]);
            }
        }
        CHECK(tot[0] == run[0] && tot[1] == run[1] && tot[2] == run[2]);
        // any output may be NULL
        CHECK(qfec_mixed_layout(nc, ks, ms, G, code.data(), bb.data(), nullptr, nullptr, nullptr,
                                nullptr) == 0);
        if (G == 0) {
            CHECK(qfec_mixed_layout(nc, ks, ms, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    tot) == 0);
            CHECK(tot[0] == 0 && tot[1] == 0 && tot[2] == 0);
            continue;
        }
        // the staging plan over these groups: a block count per group (0 for a group whose code
        // index names no code), random gaps, chunks of a few groups and one group per chunk
        {
            std::vector<int> nin((size_t)G), nout((size_t)G);
            std::vector<long long> in_off((size_t)G), out_off((size_t)G);
            long long ri = 0, ro = 0;
            for (long long g = 0; g < G; ++g) {
                const bool none = rng() % 9 == 0;
                nin[(size_t)g] = none ? 0 : ks[code[(size_t)g]];
                nout[(size_t)g] = none ? 0 : ms[code[(size_t)g]];
                in_off[(size_t)g] = ri += 16 * (rng() % 4);
                out_off[(size_t)g] = ro += 16 * (rng() % 4);
                ri = up16(ri + (long long)nin[(size_t)g] * bb[(size_t)g]);
                ro = up16(ro + (long long)nout[(size_t)g] * bb[(size_t)g]);
            }
            for (long long target : {1LL << 20, 64LL << 10, 1LL}) {
                qfec::StageList L{bb.data()};
                qfec::Stage& in = L.packed(in_off.data(), nin.data());
                qfec::Stage& out = L.packed(out_off.data(), nout.data());
                for (size_t b : {4, 8, 8, 4, 1, 250, 10}) L.dense(b);   // bb .. status, code, rows
                qfec::Chunks ch;
                const char* msg = nullptr;
                CHECK(qfec::ragged_chunks(L, in, out, G, target, &ch, &msg) == 0);
                CHECK(ch.count() >= 1 && ch.begin(0) == 0 && ch.begin(ch.count()) == G);
                if (target == 1) CHECK(ch.count() == G);                // one group per chunk
                for (long long i = 0; i < ch.count(); ++i) {
                    const long long g0 = ch.begin(i), n = ch.begin(i + 1) - g0;
                    CHECK(n >= 1);
                    if (n > 1) CHECK((long long)qfec::stage_bytes(L, g0, n) <= target);
                    const long long last = g0 + n - 1;
                    CHECK((long long)in.off[last] + (long long)nin[(size_t)last] * bb[(size_t)last] -
                              in.off[g0] <= (long long)qfec::stage_bytes(L, g0, n));
                }
                check_carve(L, ch);
            }
            // overlapping by the group's own count: group 0 of 250 blocks, the next 16 bytes on
            if (G >= 2) {
                nin[0] = 250;
                in_off[1] = in_off[0] + 16;
                qfec::StageList L{bb.data()};
                qfec::Stage& in = L.packed(in_off.data(), nin.data());
                qfec::Stage& out = L.packed(out_off.data(), nout.data());
                qfec::Chunks ch;
                const char* msg = nullptr;
                CHECK(qfec::ragged_chunks(L, in, out, G, 1 << 20, &ch, &msg) == -2);
            }
        }
        // one hostile entry at a time; the offset arrays are exactly G long
        const size_t at = (size_t)(rng() % (unsigned)G);
        const unsigned char keep_c = code[at];
        for (int v : {nc, nc + 1, 32, 255}) {
            code[at] = (unsigned char)v;
            CHECK(qfec_mixed_layout(nc, ks, ms, G, code.data(), bb.data(), d.data(), p.data(),
                                    r.data(), tot) == -2);
        }
        code[at] = keep_c;
        const int keep_b = bb[at];
        for (int v : {0, -1, INT_MIN}) {
            bb[at] = v;
            CHECK(qfec_mixed_layout(nc, ks, ms, G, code.data(), bb.data(), d.data(), p.data(),
                                    r.data(), tot) == -2);
        }
        bb[at] = keep_b;
        // a one-code set is qfec_ragged_layout
        std::vector<unsigned char> zero((size_t)G, 0);
        std::vector<long long> d2((size_t)G), p2((size_t)G), r2((size_t)G);
        long long tot2[3];
        const int k1[1] = {ks[rep % nc]}, m1[1] = {ms[rep % nc]};
        CHECK(qfec_mixed_layout(1, k1, m1, G, zero.data(), bb.data(), d.data(), p.data(), r.data(),
                                tot) == 0);
        CHECK(qfec_ragged_layout(k1[0], m1[0], G, bb.data(), d2.data(), p2.data(), r2.data(),
                                 tot2) == 0);
        CHECK(d == d2 && p == p2 && r == r2 && tot[0] == tot2[0] && tot[1] == tot2[1] &&
              tot[2] == tot2[2]);
    }
    // bad sets and arguments
    const unsigned char c0[3] = {0, 0, 0};
    const int b8[3] = {8, 8, 8};
    long long tot[3];
    std::vector<int> k33(33, 5);
    CHECK(qfec_mixed_layout(0, ks, ms, 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(33, k33.data(), k33.data(), 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(32, k33.data(), k33.data(), 1, c0, b8, nullptr, nullptr, nullptr, tot) == 0);
    CHECK(qfec_mixed_layout(-1, ks, ms, 0, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(nc, nullptr, ms, 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(nc, ks, nullptr, 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(nc, ks, ms, -1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(nc, ks, ms, 1, nullptr, b8, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_mixed_layout(nc, ks, ms, 1, c0, nullptr, nullptr, nullptr, nullptr, tot) == -2);
    for (int v : {0, 256, -4, INT_MAX}) {
        const int kb[2] = {5, v}, mb[2] = {5, 5};
        CHECK(qfec_mixed_layout(2, kb, mb, 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    }
    for (int v : {0, -1, INT_MIN}) {
        const int kb[2] = {5, 5}, mb[2] = {5, v};
        CHECK(qfec_mixed_layout(2, kb, mb, 1, c0, b8, nullptr, nullptr, nullptr, tot) == -2);
    }
    // overflow of the running offset: 2^31 - 1 parity blocks of 2^31 - 1 bytes per group
    const int kb[1] = {255}, mb[1] = {INT_MAX}, bmax[3] = {INT_MAX, INT_MAX, INT_MAX};
    CHECK(qfec_mixed_layout(1, kb, mb, 1, c0, bmax, nullptr, nullptr, nullptr, tot) == 0);
    CHECK(qfec_mixed_layout(1, kb, mb, 3, c0, bmax, nullptr, nullptr, nullptr, tot) == -2);
}

// ---- the staging plan of the host-pointer batches (fec_host.cpp declares these lists)
using qfec::Chunks;
using qfec::Stage;
using qfec::StageList;

enum Body { DEC_REC, SEAL, OPEN, ENC, DEC, R_ENC, R_DEC, R_SEAL, R_OPEN, N_BODIES };

// A stage list shaped like the body of one host entry point; `opt`: its optional arrays are
// present.  The ragged shapes name their two packed stages.
static void declare(int body, bool opt, int k, int m, int bb, size_t stride,
                    const long long* in_off, const long long* out_off, StageList& L, Stage** in,
                    Stage** out) {
    const int rmax = k < m ? k : m;
    const size_t np = (size_t)(k + m), len_g = np * 4;
    auto ragged = [&](int n_out) {
        *in = &L.packed(in_off, k);
        *out = &L.packed(out_off, n_out);
        for (size_t b : {4, 8, 8, 4}) L.dense(b);   // bb, in_rel, out_rel, status
    };
    auto seal_pkts = [&] {
        L.dense(np * stride, opt);
        L.dense(np * stride);
        L.dense(len_g);
        L.dense(len_g, opt);
        L.dense(len_g, opt);
    };
    auto open_pkts = [&] {
        L.dense(np * stride);
        L.dense(len_g);
        L.dense(len_g, opt);
        L.dense(len_g);
    };
    switch (body) {
    case DEC_REC:
        for (size_t b : {(size_t)k * bb, (size_t)rmax * bb, (size_t)k, (size_t)rmax, (size_t)4})
            L.dense(b);
        break;
    case SEAL:
        L.dense((size_t)k * bb);
        L.dense((size_t)m * bb);
        seal_pkts();
        break;
    case OPEN:
        open_pkts();
        for (size_t b : {(size_t)k * bb, (size_t)k, (size_t)rmax * bb, (size_t)rmax, (size_t)4})
            L.dense(b);
        break;
    case ENC:
        L.dense((size_t)k * bb);
        L.dense((size_t)m * bb).rows((size_t)m * bb, bb);
        break;
    case DEC:
        for (size_t b : {(size_t)k * bb, (size_t)k, (size_t)4}) L.dense(b);
        break;
    case R_ENC: ragged(m); break;
    case R_DEC:
        ragged(rmax);
        L.dense(k);
        L.dense(rmax);
        break;
    case R_SEAL:
        ragged(m);
        seal_pkts();
        break;
    case R_OPEN:
        ragged(rmax);
        open_pkts();
        L.dense(k);
        L.dense(rmax);
        break;
    }
}

// Every chunk's carve: aligned, disjoint, in declaration order, inside the staging size the
// same list produced.  The block has exactly that size and every sub-buffer is written in
// full, so an overrun is an ASan error.
static void check_carve(StageList& L, const Chunks& ch) {
    const size_t total = qfec::staging_bytes(L, ch);
    std::vector<uint8_t> block(total);
    for (long long i = 0; i < ch.count(); ++i) {
        const long long g0 = ch.begin(i), n = ch.begin(i + 1) - g0;
        CHECK(n >= 1);
        CHECK(qfec::stage_carve(L, g0, n, block.data()) <= total);
        uint8_t* end = block.data();
        for (int j = 0; j < L.n; ++j) {
            const Stage& s = L.s[j];
            if (!s.present) {
                CHECK(!s.dev && s.bytes == 0);
                continue;
            }
            CHECK((s.dev - block.data()) % 256 == 0);
            CHECK(s.dev >= end);
            end = s.dev + s.bytes;
            CHECK(end <= block.data() + total);
            memset(s.dev, 0xA5, s.bytes);
        }
    }
}

static void check_uniform(int k, int m, std::mt19937& rng) {
    for (int body = DEC_REC; body <= DEC; ++body)
        for (int opt = 0; opt < 2; ++opt) {
            StageList L;
            const int bb = 1 + (int)(rng() % 2100);
            declare(body, opt, k, m, bb, 4 * (1 + rng() % 400), nullptr, nullptr, L, nullptr,
                    nullptr);
            Chunks ch;
            const long long G = 1 + rng() % 300;
            ch.groups = G;
            ch.uniform =
                qfec::uniform_chunk(G, qfec::stage_bytes(L, 0, 1), 1, 1 + (int)(rng() % 8));
            CHECK(ch.begin(0) == 0 && ch.begin(ch.count()) == G);
            check_carve(L, ch);
        }
}

static void check_ragged(int k, int m, const std::vector<int>& bb, std::mt19937& rng) {
    const long long G = (long long)bb.size();
    if (G == 0) return;
    for (int body = R_ENC; body < N_BODIES; ++body)
        for (int opt = 0; opt < 2; ++opt)
            for (long long target : {1LL << 20, 64LL << 10}) {
                const int n_out = (body == R_ENC || body == R_SEAL) ? m : (k < m ? k : m);
                // packed offsets with random 16-byte gaps between the groups
                std::vector<long long> in_off(G), out_off(G);
                long long ri = 0, ro = 0;
                for (long long g = 0; g < G; ++g) {
                    in_off[g] = ri += 16 * (rng() % 4);
                    out_off[g] = ro += 16 * (rng() % 4);
                    ri = up16(ri + (long long)k * bb[g]);
                    ro = up16(ro + (long long)n_out * bb[g]);
                }
                StageList L{bb.data()};
                Stage *in = nullptr, *out = nullptr;
                declare(body, opt, k, m, 0, 4 * (1 + rng() % 400), in_off.data(), out_off.data(), L,
                        &in, &out);
                Chunks ch;
                const char* msg = nullptr;
                CHECK(qfec::ragged_chunks(L, *in, *out, G, target, &ch, &msg) == 0);
                CHECK(ch.count() >= 1 && ch.begin(0) == 0 && ch.begin(ch.count()) == G);
                for (long long i = 0; i < ch.count(); ++i) {
                    const long long g0 = ch.begin(i), n = ch.begin(i + 1) - g0;
                    CHECK(n >= 1);
                    if (n > 1) CHECK((long long)qfec::stage_bytes(L, g0, n) <= target);
                    for (long long g = g0; g < g0 + n; ++g) {
                        CHECK(ch.in_rel[g] == in_off[g] - in_off[g0]);
                        CHECK(ch.out_rel[g] == out_off[g] - out_off[g0]);
                    }
                }
                check_carve(L, ch);
            }
}

// ragged_chunks on G groups of (k = 4, m = 2); exact-size inputs, so a read past them is caught
static int chunk_rc(std::vector<int> bb, std::vector<long long> in_off,
                    std::vector<long long> out_off, const char** msg) {
    StageList L{bb.data()};
    Stage& in = L.packed(in_off.data(), 4);
    Stage& out = L.packed(out_off.data(), 2);
    Chunks ch;
    return qfec::ragged_chunks(L, in, out, (long long)bb.size(), 1 << 20, &ch, msg);
}

static void check_plan_errors() {
    const char* msg = nullptr;
    const char* const asc = "host ragged batches need ascending, non-overlapping offsets";
    const char* const mult = "ragged offsets must be non-negative multiples of 16";
    CHECK(chunk_rc({8, 8}, {0, 32}, {0, 16}, &msg) == 0);
    CHECK(chunk_rc({8, 0}, {0, 32}, {0, 16}, &msg) == -2 && !strcmp(msg, "bb[g] < 1"));
    CHECK(chunk_rc({-3, 8}, {0, 32}, {0, 16}, &msg) == -2 && !strcmp(msg, "bb[g] < 1"));
    CHECK(chunk_rc({8, 8}, {-16, 32}, {0, 16}, &msg) == -2 && !strcmp(msg, mult));
    CHECK(chunk_rc({8, 8}, {0, 32}, {0, 24}, &msg) == -2 && !strcmp(msg, mult));
    CHECK(chunk_rc({8, 8}, {32, 0}, {0, 16}, &msg) == -2 && !strcmp(msg, asc));    // descending
    CHECK(chunk_rc({8, 8}, {0, 16}, {0, 16}, &msg) == -2 && !strcmp(msg, asc));    // overlapping
    CHECK(chunk_rc({8, 8}, {0, 32}, {0, 0}, &msg) == -2 && !strcmp(msg, asc));
    const long long top = LLONG_MAX & ~15LL;   // a group there ends past INT64_MAX
    CHECK(chunk_rc({8, 8}, {0, top}, {0, 16}, &msg) == -2 && !strcmp(msg, asc));
    CHECK(chunk_rc({8, 8}, {0, 32}, {top, top}, &msg) == -2 && !strcmp(msg, asc));
    CHECK(chunk_rc({8}, {top}, {0}, &msg) == -2 && !strcmp(msg, asc));
    // the uniform chunk size, by hand from max(1, min(G, max(target / per, min(min_groups,
    // 2 GiB / per)))) at 64 MiB / 512 groups
    CHECK(qfec::uniform_chunk(65536, 48672, 64, 512) == 1378);     // B encode: 67108864 / 48672
    CHECK(qfec::uniform_chunk(16384, 1297152, 64, 512) == 512);    // D encode: 51 by bytes
    CHECK(qfec::uniform_chunk(100, 48672, 64, 512) == 100);
    CHECK(qfec::uniform_chunk(100, 1297152, 64, 512) == 100);
    CHECK(qfec::uniform_chunk(65536, (size_t)3 << 30, 64, 512) == 1);
    CHECK(qfec::uniform_chunk(241, 17550, 1, 1) == 59);            // 1048576 / 17550
}

// ---- the host helpers of the framed calls
static void check_framed(std::mt19937& rng) {
    long long tot[3] = {-1, -1, -1};
    // zero groups: nothing is read
    CHECK(qfec_framed_layout(5, 5, 0, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == 0);
    CHECK(tot[0] == 0 && tot[1] == 0 && tot[2] == 0);
    CHECK(qfec_framed_rx_block_bytes(5, 5, 0, nullptr, nullptr, 0, nullptr) == 0);
    CHECK(qfec_framed_layout(5, 5, 1, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_framed_layout(0, 5, 0, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == -2);
    CHECK(qfec_framed_rx_block_bytes(5, 0, 0, nullptr, nullptr, 0, nullptr) == -2);
    CHECK(qfec_framed_rx_block_bytes(5, 5, -1, nullptr, nullptr, 0, nullptr) == -2);
    // random groups in allocations of exactly their size; any offset array may be NULL
    for (int rep = 0; rep < 50; ++rep) {
        const int k = 1 + (int)(rng() % 40), m = 1 + (int)(rng() % 8);
        const long long G = 1 + (long long)(rng() % 30);
        std::vector<int> len((size_t)(G * k)), bb((size_t)G), want((size_t)G);
        for (long long g = 0; g < G; ++g) {
            int most = 0;
            for (int i = 0; i < k; ++i) {
                const int l = rng() % 7 == 0 ? 0x3fff : (int)(rng() % 1400);
                len[(size_t)(g * k + i)] = l;
                most = l > most ? l : most;
            }
            want[(size_t)g] = (most + 2 + 7) / 8 * 8;
        }
        std::vector<long long> d((size_t)G), r((size_t)G);
        CHECK(qfec_framed_layout(k, m, G, len.data(), bb.data(), d.data(), nullptr, r.data(), tot) == 0);
        CHECK(bb == want);
        std::vector<long long> d2((size_t)G), r2((size_t)G);
        long long tot2[3];
        CHECK(qfec_ragged_layout(k, m, G, bb.data(), d2.data(), nullptr, r2.data(), tot2) == 0);
        CHECK(d == d2 && r == r2 && tot[0] == tot2[0] && tot[1] == tot2[1] && tot[2] == tot2[2]);
        const size_t bad = (size_t)(rng() % (unsigned)(G * k));
        const int keep = len[bad];
        for (int v : {0x4000, -1, INT_MAX, INT_MIN}) {
            len[bad] = v;
            CHECK(qfec_framed_layout(k, m, G, len.data(), bb.data(), nullptr, nullptr, nullptr, nullptr) == -2);
        }
        len[bad] = keep;
        // the receiver's sizes: all absent, then a random receive set with hostile lengths
        const long long per = k + m;
        std::vector<int> pl((size_t)(G * per), -1), ad((size_t)(G * per), 16), rb((size_t)G, 7);
        CHECK(qfec_framed_rx_block_bytes(k, m, G, pl.data(), ad.data(), 0, rb.data()) == 0);
        for (int b : rb) CHECK(b == 0);
        for (long long g = 0; g < G; ++g) {
            long long most = 0;
            for (long long i = 0; i < per; ++i) {
                const size_t p = (size_t)(g * per + i);
                const unsigned pick = rng() % 8;
                ad[p] = pick == 0 ? -3 : (int)(rng() % 20);
                pl[p] = pick == 1 ? -1 : pick == 2 ? INT_MAX : pick == 3 ? ad[p] + 11
                                                    : ad[p] + 12 + (int)(rng() % 1400);
                const long long pt = (long long)pl[p] - ad[p] - 12;
                if (pl[p] >= 0 && ad[p] >= 0 && pt >= 0) {
                    const long long st = pt + (i < k ? 2 : 0);
                    most = st > most ? st : most;
                }
            }
            want[(size_t)g] = (int)(most > INT_MAX ? INT_MAX : most);
        }
        CHECK(qfec_framed_rx_block_bytes(k, m, G, pl.data(), ad.data(), 0, rb.data()) == 0);
        CHECK(rb == want);
    }
    // every length 0x3fff in groups of 255: the data offsets pass 2^40
    {
        const int k = 255, m = 1;
        const long long G = 270000, per_group = ((long long)k * 16392 + 15) & ~15LL;
        std::vector<int> len((size_t)(G * k), 0x3fff), bb((size_t)G);
        std::vector<long long> d((size_t)G);
        CHECK(qfec_framed_layout(k, m, G, len.data(), bb.data(), d.data(), nullptr, nullptr, tot) == 0);
        CHECK(bb[0] == 16392 && bb[(size_t)G - 1] == 16392);
        CHECK(d[(size_t)G - 1] == (G - 1) * per_group && d[(size_t)G - 1] > (1LL << 40));
        CHECK(tot[0] == G * per_group && tot[1] == G * 16400 && tot[2] == G * 16400);
    }
}

// ---- the host helper of the arrival-order receiver, in arrays of exactly n entries
static void check_arrivals(std::mt19937& rng) {
    // n = 0: no array is read, every size is 0; no groups: nothing is written
    {
        std::vector<int> bb(3, 7);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 3, 0, nullptr, nullptr, nullptr, nullptr, 0, bb.data()) == 0);
        CHECK(bb == std::vector<int>(3, 0));
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0);
        const int grp[1] = {0}, len[1] = {40};
        const unsigned char idx[1] = {0};
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 0, 1, grp, idx, len, nullptr, 16, nullptr) == 0);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 1, -1, grp, idx, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, -1, 1, grp, idx, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(0, 5, 1, 1, grp, idx, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(250, 6, 1, 1, grp, idx, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 1, 1, nullptr, idx, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 1, 1, grp, nullptr, len, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 1, 1, grp, idx, nullptr, nullptr, 16, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes(5, 5, 1, 1, grp, idx, len, nullptr, 16, nullptr) == -2);
    }
    // duplicates, more than k arrivals, a tag at the last group, ignored tags: k = 2, m = 2
    {
        //                 dup of (0,0)   late in g0  last group   ignored: g = -1, g = G, i = k+m, 255
        const int grp[] = {0, 0, 0, 0,    0,          2, 2,        -1, 3, 1, 1};
        const unsigned char idx[] = {0, 0, 3, 1,  2,  3, 3,        0, 0, 4, 255};
        const int len[] = {16 + 12 + 10, 16 + 12 + 900, 16 + 12 + 16, 16 + 12 + 500,
                           16 + 12 + 1000, 16 + 12 + 24, 16 + 12 + 999,
                           2000, 2000, 2000, 2000};
        int bb[3] = {7, 7, 7};
        CHECK(qfec_arrivals_rx_block_bytes(2, 2, 3, 11, grp, idx, len, nullptr, 16, bb) == 0);
        // g0: (0, 10 + 2) and FEC (3, 16) are its first k = 2; the duplicate's 900 bytes, data
        // packet 1 and FEC packet 2 come too late.  g1: only ignored tags.  g2: the first copy.
        CHECK(bb[0] == 16 && bb[1] == 0 && bb[2] == 24);
        // a first copy with fewer than 12 bytes behind its AD does not count, its second copy does
        const int grp2[] = {0, 0}, len2[] = {16 + 11, 16 + 12 + 30};
        const unsigned char idx2[] = {1, 1};
        int one[1] = {7};
        CHECK(qfec_arrivals_rx_block_bytes(2, 2, 1, 2, grp2, idx2, len2, nullptr, 16, one) == 0);
        CHECK(one[0] == 32);
    }
    // random streams with hostile tags and lengths against the sequential rule
    for (int rep = 0; rep < 50; ++rep) {
        const int k = 1 + (int)(rng() % 40), m = 1 + (int)(rng() % 8), per = k + m;
        const long long G = 1 + (long long)(rng() % 12);
        const size_t n = rng() % 600;
        std::vector<int> grp(n), len(n), ad(n), bb((size_t)G, 7), want((size_t)G, 0);
        std::vector<unsigned char> idx(n);
        std::vector<std::vector<bool>> seen((size_t)G, std::vector<bool>((size_t)per, false));
        std::vector<int> held((size_t)G, 0);
        for (size_t a = 0; a < n; ++a) {
            const unsigned pick = rng() % 16;
            grp[a] = pick == 0 ? -1 : pick == 1 ? (int)G : pick == 2 ? INT_MIN : pick == 3 ? INT_MAX
                                                                          : (int)(rng() % G);
            if (pick == 4) grp[a] = (int)G - 1;
            idx[a] = (unsigned char)(pick == 5 ? per : pick == 6 ? 255 : rng() % per);
            ad[a] = pick == 7 ? -3 : (int)(rng() % 20);
            len[a] = pick == 8 ? -1 : pick == 9 ? INT_MAX : pick == 10 ? ad[a] + 11
                                                          : ad[a] + 12 + (int)(rng() % 1400);
            const long long g = grp[a], pt = (long long)len[a] - ad[a] - 12;
            if (g < 0 || g >= G || idx[a] >= per) continue;
            if (len[a] < 0 || ad[a] < 0 || pt < 0) continue;
            if (seen[(size_t)g][idx[a]] || held[(size_t)g] >= k) continue;
            seen[(size_t)g][idx[a]] = true;
            ++held[(size_t)g];
            const long long st = pt + (idx[a] < k ? 2 : 0);
            want[(size_t)g] = std::max(want[(size_t)g], (int)std::min<long long>(st, INT_MAX));
        }
        CHECK(qfec_arrivals_rx_block_bytes(k, m, G, (long long)n, grp.data(), idx.data(), len.data(),
                                           ad.data(), 0, bb.data()) == 0);
        CHECK(bb == want);
    }
}

// ---- the running form (qfec_arrivals_rx_block_bytes_carry) and the window's size helper
// (qfec_rxwin_bytes): pieces of hostile random streams in arrays of exactly the piece's entries,
// state arrays of exactly [G][32] and [G], against the one-shot helper over the whole stream;
// duplicates and more than k arrivals across pieces, tags at the last group, n = 0, a release
static void check_arrivals_carry(std::mt19937& rng) {
    {
        std::vector<unsigned char> seen(3 * 32, 0);
        std::vector<int> bb(3, 0);
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 3, 0, nullptr, nullptr, nullptr, nullptr, 0,
                                                 seen.data(), bb.data()) == 0);
        CHECK(bb == std::vector<int>(3, 0) && seen == std::vector<unsigned char>(96, 0));
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 0, 0, nullptr, nullptr, nullptr, nullptr, 0,
                                                 nullptr, nullptr) == 0);
        const int grp[1] = {0}, len[1] = {40};
        const unsigned char idx[1] = {0};
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 0, 1, grp, idx, len, nullptr, 16, nullptr, nullptr) == 0);
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 1, -1, grp, idx, len, nullptr, 16, seen.data(), bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_carry(250, 6, 1, 1, grp, idx, len, nullptr, 16, seen.data(), bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 1, 1, grp, idx, len, nullptr, 16, nullptr, bb.data()) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 1, 1, grp, idx, len, nullptr, 16, seen.data(), nullptr) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_carry(5, 5, 1, 1, nullptr, idx, len, nullptr, 16, seen.data(), bb.data()) == -2);
    }
    // k = 2, m = 2, one arrival per call: a duplicate of a packet counted two calls earlier, a
    // packet late behind k counted ones, a tag at the last group and its last index
    {
        const int grp[] = {0, 2, 0, 0, 0, 2, 3};
        const unsigned char idx[] = {0, 3, 3, 0, 1, 3, 0};
        const int len[] = {28 + 10, 28 + 24, 28 + 16, 28 + 900, 28 + 1000, 28 + 999, 2000};
        std::vector<unsigned char> seen(3 * 32, 0);
        std::vector<int> bb(3, 0);
        for (int a = 0; a < 7; ++a)
            CHECK(qfec_arrivals_rx_block_bytes_carry(2, 2, 3, 1, grp + a, idx + a, len + a, nullptr,
                                                     16, seen.data(), bb.data()) == 0);
        CHECK(bb[0] == 16 && bb[1] == 0 && bb[2] == 24);
        CHECK(seen[0] == 0x09 && seen[64] == 0x08 && seen[32] == 0);
    }
    for (int rep = 0; rep < 50; ++rep) {
        const int k = 1 + (int)(rng() % 60), m = 1 + (int)(rng() % 8), per = k + m;
        const long long G = 1 + (long long)(rng() % 12);
        const size_t n = rng() % 600;
        std::vector<int> grp(n), len(n), ad(n);
        std::vector<unsigned char> idx(n);
        for (size_t a = 0; a < n; ++a) {
            const unsigned pick = rng() % 16;
            grp[a] = pick == 0 ? -1 : pick == 1 ? (int)G : pick == 2 ? INT_MIN : pick == 3 ? INT_MAX
                                                                          : (int)(rng() % G);
            if (pick == 4) grp[a] = (int)G - 1;
            idx[a] = (unsigned char)(pick == 5 ? per : pick == 6 ? 255 : rng() % per);
            ad[a] = pick == 7 ? -3 : (int)(rng() % 20);
            len[a] = pick == 8 ? -1 : pick == 9 ? INT_MAX : pick == 10 ? ad[a] + 11
                                                          : ad[a] + 12 + (int)(rng() % 1400);
        }
        std::vector<int> whole((size_t)G, 7);
        CHECK(qfec_arrivals_rx_block_bytes(k, m, G, (long long)n, grp.data(), idx.data(), len.data(),
                                           ad.data(), 0, whole.data()) == 0);
        // the pieces, each in arrays of its own size (an empty one among them)
        std::vector<unsigned char> seen((size_t)G * 32, 0);
        std::vector<int> bb((size_t)G, 0);
        size_t at = 0, released_at = n;
        const long long rel = (long long)(rng() % G);
        const bool release = rep % 3 == 0;
        while (at < n || at == 0) {
            const size_t take = std::min(n - at, (size_t)(rng() % 97));
            std::vector<int> pg(grp.begin() + at, grp.begin() + at + take),
                pl(len.begin() + at, len.begin() + at + take),
                pa(ad.begin() + at, ad.begin() + at + take);
            std::vector<unsigned char> pi(idx.begin() + at, idx.begin() + at + take);
            CHECK(qfec_arrivals_rx_block_bytes_carry(k, m, G, (long long)take, pg.data(), pi.data(),
                                                     pl.data(), pa.data(), 0, seen.data(),
                                                     bb.data()) == 0);
            at += take;
            if (release && released_at == n && at >= n / 2) {   // one group back to empty
                std::fill(seen.begin() + rel * 32, seen.begin() + rel * 32 + 32, 0);
                bb[(size_t)rel] = 0;
                released_at = at;
            }
            if (n == 0) break;
        }
        if (release && released_at < n) {
            std::vector<int> rest((size_t)G, 7);
            CHECK(qfec_arrivals_rx_block_bytes(k, m, G, (long long)(n - released_at),
                                               grp.data() + released_at, idx.data() + released_at,
                                               len.data() + released_at, ad.data() + released_at, 0,
                                               rest.data()) == 0);
            whole[(size_t)rel] = rest[(size_t)rel];
        } else if (release && n > 0) {
            whole[(size_t)rel] = 0;   // released behind the last arrival
        }
        CHECK(bb == whole);
    }
    long long bytes = -7;
    CHECK(qfec_rxwin_bytes(10, 1, 4096, 1360, &bytes) == 0 && bytes > 4096LL * 11 * 1360);
    CHECK(qfec_rxwin_bytes(2, 2, 0, 16, &bytes) == 0 && bytes == 0);
    CHECK(qfec_rxwin_bytes(127, 128, 8421504, 2147483632, &bytes) == 0 && bytes > 0);   // the largest
    CHECK(qfec_rxwin_bytes(127, 128, 8421505, 16, &bytes) == -2);
    CHECK(qfec_rxwin_bytes(250, 6, 1, 16, &bytes) == -2 && qfec_rxwin_bytes(10, 1, 1, 24, &bytes) == -2);
    CHECK(qfec_rxwin_bytes(10, 1, 1, 16, nullptr) == -2 && qfec_rxwin_bytes(10, 1, -1, 16, &bytes) == -2);
}

// ---- the three host helpers of the mixed-code wire path, in arrays of exactly G, G + 1, npay
// and n entries: empty sets of groups, groups without a code, duplicates, more than k arrivals,
// tags at the last group, n = 0, and random hostile streams against the sequential rule
static void check_mixed_wire(std::mt19937& rng) {
    const int ks[] = {10, 2, 5, 32, 10, 250}, ms[] = {1, 2, 5, 4, 20, 5};
    const int nc = 6;
    long long tot[3];
    // no groups: the tables hold their one entry, nothing else is read or written
    {
        std::vector<int> pf(1, 7), qf(1, 7);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, 0, nullptr, pf.data(), qf.data()) == 0);
        CHECK(pf[0] == 0 && qf[0] == 0);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, 0, nullptr, nullptr, nullptr) == 0);
        CHECK(qfec_framed_layout_mixed(nc, ks, ms, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, tot) == 0);
        CHECK(tot[0] == 0 && tot[1] == 0 && tot[2] == 0);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 0, nullptr, 0, nullptr, nullptr, nullptr,
                                                 nullptr, 0, nullptr) == 0);
        const int grp[1] = {0}, len[1] = {40};
        const unsigned char idx[1] = {0};
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 0, nullptr, 1, grp, idx, len, nullptr, 16,
                                                 nullptr) == 0);
        // argument errors
        const unsigned char c0[1] = {0};
        int b1[1] = {7};
        CHECK(qfec_mixed_packet_layout(0, ks, ms, 0, nullptr, nullptr, nullptr) == -2);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, -1, nullptr, nullptr, nullptr) == -2);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, 1, nullptr, nullptr, nullptr) == -2);
        CHECK(qfec_framed_layout_mixed(nc, ks, ms, 1, c0, nullptr, 10, nullptr, b1, nullptr, nullptr,
                                       nullptr, nullptr) == -2);
        CHECK(qfec_framed_layout_mixed(nc, ks, ms, 1, c0, nullptr, -1, len, b1, nullptr, nullptr,
                                       nullptr, nullptr) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 1, c0, -1, grp, idx, len, nullptr, 16, b1) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 1, nullptr, 1, grp, idx, len, nullptr, 16, b1) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 1, c0, 1, nullptr, idx, len, nullptr, 16, b1) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 1, c0, 1, grp, idx, len, nullptr, 16, nullptr) == -2);
        const int kb[1] = {250}, mb[1] = {6};
        CHECK(qfec_arrivals_rx_block_bytes_mixed(1, kb, mb, 1, c0, 1, grp, idx, len, nullptr, 16, b1) == -2);
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 1, c0, 0, nullptr, nullptr, nullptr, nullptr,
                                                 16, b1) == 0);
        CHECK(b1[0] == 0);
    }
    // duplicates, more than k arrivals, a tag at the last group, a group without a code: codes
    // (2, 2), none, (10, 1)
    {
        const unsigned char code[] = {1, 200, 0};
        //                 dup of (0,0)   late in g0  codeless  last group (k = 10: index 10 is FEC)
        const int grp[] = {0, 0, 0, 0,    0,          1, 1,     2, 2, 2,   -1, 3};
        const unsigned char idx[] = {0, 0, 3, 1,  2,  0, 1,     10, 11, 0, 0, 0};
        const int len[] = {16 + 12 + 10, 16 + 12 + 900, 16 + 12 + 16, 16 + 12 + 500, 16 + 12 + 1000,
                           16 + 12 + 700, 16 + 12 + 700, 16 + 12 + 24, 2000, 16 + 12 + 30, 2000, 2000};
        int bb[3] = {7, 7, 7};
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, 3, code, 12, grp, idx, len, nullptr, 16,
                                                 bb) == 0);
        CHECK(bb[0] == 16 && bb[1] == 0 && bb[2] == 32);    // g2: FEC 24, index 11 ignored, data 30 + 2
        int pf[4], qf[4];
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, 3, code, pf, qf) == 0);
        CHECK(pf[0] == 0 && pf[1] == 4 && pf[2] == 4 && pf[3] == 15);
        CHECK(qf[0] == 0 && qf[1] == 2 && qf[2] == 2 && qf[3] == 12);
        const std::vector<int> lens(12, 100);
        int fb[3];
        CHECK(qfec_framed_layout_mixed(nc, ks, ms, 3, code, qf, 12, lens.data(), fb, nullptr, nullptr,
                                       nullptr, nullptr) == -2);    // the codeless group has no layout
    }
    for (int rep = 0; rep < 60; ++rep) {
        const size_t G = 1 + rng() % 40;
        std::vector<unsigned char> code(G);
        for (auto& c : code) c = (unsigned char)(rng() % 8 == 0 ? 6 + rng() % 250 : rng() % nc);
        std::vector<int> pf(G + 1, -7), qf(G + 1, -7);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, (long long)G, code.data(), pf.data(), qf.data()) == 0);
        long long p = 0, q = 0;
        for (size_t g = 0; g < G; ++g) {
            CHECK(pf[g] == p && qf[g] == q);
            if (code[g] < nc) p += ks[code[g]] + ms[code[g]], q += ks[code[g]];
        }
        CHECK(pf[G] == p && qf[G] == q);
        // framed layout: every group needs a code; lengths in an array of exactly npay entries
        std::vector<unsigned char> good(code);
        for (auto& c : good) c = (unsigned char)(c % nc);
        CHECK(qfec_mixed_packet_layout(nc, ks, ms, (long long)G, good.data(), nullptr, qf.data()) == 0);
        const size_t npay = (size_t)qf[G];
        std::vector<int> len(npay), bb(G, -7), want(G);
        for (auto& l : len) l = (int)(rng() % 8 == 0 ? 0x3fff : rng() % 1400);
        for (size_t g = 0; g < G; ++g) {
            int most = 0;
            for (int i = 0; i < ks[good[g]]; ++i) most = std::max(most, len[(size_t)qf[g] + (size_t)i]);
            want[g] = (most + 2 + 7) & ~7;
        }
        std::vector<long long> d(G), pr(G), r(G), d2(G), p2(G), r2(G);
        long long tot2[3];
        for (const int* table : {(const int*)nullptr, (const int*)qf.data()}) {
            CHECK(qfec_framed_layout_mixed(nc, ks, ms, (long long)G, good.data(), table, (long long)npay,
                                           len.data(), bb.data(), d.data(), pr.data(), r.data(), tot) == 0);
            CHECK(bb == want);
        }
        CHECK(qfec_mixed_layout(nc, ks, ms, (long long)G, good.data(), bb.data(), d2.data(), p2.data(),
                                r2.data(), tot2) == 0);
        CHECK(d == d2 && pr == p2 && r == r2 && tot[0] == tot2[0] && tot[1] == tot2[1] && tot[2] == tot2[2]);
        // hostile: a length outside the prefix, an array one entry short, a table that leaves it
        const size_t at = rng() % npay;
        const int keep = len[at];
        len[at] = rng() % 2 ? -1 : 0x4000;
        CHECK(qfec_framed_layout_mixed(nc, ks, ms, (long long)G, good.data(), nullptr, (long long)npay,
                                       len.data(), bb.data(), nullptr, nullptr, nullptr, nullptr) == -2);
        len[at] = keep;
        {
            std::vector<int> cut(len.begin(), len.end() - 1);
            CHECK(qfec_framed_layout_mixed(nc, ks, ms, (long long)G, good.data(), nullptr,
                                           (long long)npay - 1, cut.data(), bb.data(), nullptr, nullptr,
                                           nullptr, nullptr) == -2);
            std::vector<int> bad(qf);
            bad[rng() % G] = rng() % 2 ? -1 : (int)npay;
            CHECK(qfec_framed_layout_mixed(nc, ks, ms, (long long)G, good.data(), bad.data(),
                                           (long long)npay, len.data(), bb.data(), nullptr, nullptr,
                                           nullptr, nullptr) == -2);
        }
        // arrivals: hostile tags and lengths against the sequential rule with k per group
        const size_t n = rng() % 800;
        std::vector<int> grp(n), wl(n), ad(n), rb(G, 7), rwant(G, 0), held(G, 0);
        std::vector<unsigned char> idx(n);
        std::vector<std::vector<bool>> seen(G, std::vector<bool>(256, false));
        for (size_t a = 0; a < n; ++a) {
            const unsigned pick = rng() % 16;
            grp[a] = pick == 0 ? -1 : pick == 1 ? (int)G : pick == 2 ? INT_MIN : pick == 3 ? INT_MAX
                                                                          : (int)(rng() % G);
            if (pick == 4) grp[a] = (int)G - 1;
            idx[a] = (unsigned char)(pick == 6 ? 255 : pick == 5 ? 254 : rng() % 40);
            ad[a] = pick == 7 ? -3 : (int)(rng() % 20);
            wl[a] = pick == 8 ? -1 : pick == 9 ? INT_MAX : pick == 10 ? ad[a] + 11
                                                         : ad[a] + 12 + (int)(rng() % 1400);
            const long long g = grp[a], pt = (long long)wl[a] - ad[a] - 12;
            if (g < 0 || g >= (long long)G || code[(size_t)g] >= nc) continue;
            const int k = ks[code[(size_t)g]], per = k + ms[code[(size_t)g]];
            if (idx[a] >= per) continue;
            if (wl[a] < 0 || ad[a] < 0 || pt < 0) continue;
            if (seen[(size_t)g][idx[a]] || held[(size_t)g] >= k) continue;
            seen[(size_t)g][idx[a]] = true;
            ++held[(size_t)g];
            const long long st = pt + (idx[a] < k ? 2 : 0);
            rwant[(size_t)g] = std::max(rwant[(size_t)g], (int)std::min<long long>(st, INT_MAX));
        }
        CHECK(qfec_arrivals_rx_block_bytes_mixed(nc, ks, ms, (long long)G, code.data(), (long long)n,
                                                 grp.data(), idx.data(), wl.data(), ad.data(), 0,
                                                 rb.data()) == 0);
        CHECK(rb == rwant);
    }
}

int main() {
    std::mt19937 rng(20240607);
    const int codes[][2] = {{10, 1}, {3, 2}, {5, 5}, {32, 4}, {10, 20}, {1, 3}, {250, 5}, {10, 10}};
    for (auto& c : codes) {
        for (int rep = 0; rep < 40; ++rep) {
            const size_t G = rep == 0 ? 0 : 1 + rng() % 64;
            std::vector<int> bb(G);
            for (auto& b : bb) b = 1 + (int)(rng() % 2100);
            check_layout(c[0], c[1], bb);
            check_pack(c[0], c[1], false, bb, rng);
            check_pack(c[0], c[1], true, bb, rng);
            check_uniform(c[0], c[1], rng);
            check_ragged(c[0], c[1], bb, rng);
        }
    }
    check_plan_errors();
    check_framed(rng);
    check_arrivals(rng);
    check_arrivals_carry(rng);
    check_mixed_layout(rng);
    check_mixed_wire(rng);
    // errors: a size < 1, bad arguments, overflow of the running offset
    {
        const int bad[3] = {8, 0, 8};
        long long tot[3];
        CHECK(qfec_ragged_layout(4, 2, 3, bad, nullptr, nullptr, nullptr, tot) == -2);
        const int neg[1] = {-8};
        CHECK(qfec_ragged_layout(4, 2, 1, neg, nullptr, nullptr, nullptr, tot) == -2);
        CHECK(qfec_ragged_layout(0, 2, 1, bad, nullptr, nullptr, nullptr, tot) == -2);
        CHECK(qfec_ragged_layout(4, 0, 1, bad, nullptr, nullptr, nullptr, tot) == -2);
        CHECK(qfec_ragged_layout(4, 2, -1, bad, nullptr, nullptr, nullptr, tot) == -2);
        CHECK(qfec_ragged_layout(4, 2, 1, nullptr, nullptr, nullptr, nullptr, tot) == -2);
        CHECK(qfec_ragged_layout(4, 2, 0, nullptr, nullptr, nullptr, nullptr, tot) == 0);
        CHECK(tot[0] == 0 && tot[1] == 0 && tot[2] == 0);
        // 2^31 - 1 bytes x 255 blocks x 2^25 groups overflows int64
        const long long G = 1LL << 25;
        std::vector<int> big((size_t)G, 0x7fffffff);
        CHECK(qfec_ragged_layout(255, 1, G, big.data(), nullptr, nullptr, nullptr, tot) == -2);
        qfec::RaggedPack pk;
        std::vector<const unsigned char*> none(2, nullptr);
        CHECK(qfec::ragged_pack(4, 2, false, none, {8}, &pk) == -2);   // sizes disagree
    }
    if (g_fail) {
        fprintf(stderr, "ragged_pack_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("ragged_pack_check: ok\n");
    return 0;
}
