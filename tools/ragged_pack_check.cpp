// ragged_pack_check — host-code sanitizer check of the ragged layout and the queue's packing.
//
// Stand-alone (its own main, no GPU, no HIP): built from this file and
// quic_amd/csrc/fec_ragged_host.cpp with -fsanitize=address,undefined (`make ragged-check`).
// It calls qfec_ragged_layout and qfec::ragged_pack on random sizes and checks offsets and
// bounds; out-of-bounds copies or overflowing arithmetic abort under the sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fec_ragged_host.h"
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
        }
    }
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
