// compiled_codes.h — the (k, m) codes with compiled kernels at 1352-byte blocks (S = 169), one
// row each, and every per-code fact a launcher branches on.  BASELINE configs B/C's (32, 4) and
// the QuicR presets (quic_fec_group.cc:22-82).  The launchers (gf_stream.hip, gf_psyn.hip,
// gf_bsyn.hip) read this table and nothing else: a code's launch shape changes here.
#pragma once
#include <stddef.h>

#include <type_traits>
#include <utility>

namespace qfec {

constexpr int kCompiledS = 169;   // sub-row bytes of every row: bb = 1352, 1350-byte payloads

// compiled syndrome decode of a code: none (the run-time gf_stream decode), gf_bsyn, gf_psyn
enum class Syn { none, bsyn, psyn };

// Every row has the compiled gf_stream encode (gf_stream_kernel<m, 169, false, rcpt(), k>: the
// coefficients of cauchy_const.h, windowed form, every output in one unit) and the gf_ring
// static schedule.  Measurements behind the flags: DESIGN.md sections 3.3, 3.3.2, 3.7, 4.5.
struct CompiledCode {
    int k, m;
    bool stream_wide;   // gf_stream compiled encode: LDS-staged 8-byte parity stores
    bool ring_wide;     // gf_ring, one unit per group: wide parity stores under ring_wide
    bool ring_split;    // gf_ring: two units of m / 2 rows per group under ring_split (wide
                        //   stores then fit the registers, so the split form takes them)
    int ring_wg;        // what ring_wg = -1 resolves to
    Syn syn;
    bool psyn_wide;     // gf_psyn: psyn_wide = 1 takes wide recovered-block stores
    // byte stride of a coefficient row the compiled gf_stream encode is instantiated with
    constexpr int rcpt() const { return m <= 4 ? 4 : (m + 3) / 4 * 4; }
};

inline constexpr CompiledCode kCompiledCodes[] = {
    //  k   m  s.wide r.wide r.split r.wg  syn       p.wide
    {32, 4, false, false, false, 1, Syn::bsyn, false},
    {5, 5, true, true, false, 1, Syn::psyn, true},
    {10, 10, false, true, false, 1, Syn::psyn, true},
    {10, 15, false, true, false, 0, Syn::psyn, false},
    {10, 20, false, false, true, 0, Syn::psyn, false},
    {15, 15, false, true, false, 0, Syn::psyn, false},
    {250, 5, false, true, false, 1, Syn::none, false},
};
constexpr size_t kNumCompiledCodes = sizeof(kCompiledCodes) / sizeof(kCompiledCodes[0]);

constexpr const CompiledCode* find_code(int k, int m) {
    for (const CompiledCode& c : kCompiledCodes)
        if (c.k == k && c.m == m) return &c;
    return nullptr;
}
// the row of (k, m) at block size bb, if its decode is `syn`
constexpr const CompiledCode* find_code(int k, int m, int bb, Syn syn) {
    const CompiledCode* c = bb == 8 * kCompiledS ? find_code(k, m) : nullptr;
    return c && c->syn == syn ? c : nullptr;
}

// f(std::integral_constant<size_t, I>{}) for the row I of (k, m), so kCompiledCodes[I] is a
// constant expression inside f.  False: no such row, f was not called.
template <class F, size_t... Is>
inline bool with_code(int k, int m, F&& f, std::index_sequence<Is...>) {
    return ((kCompiledCodes[Is].k == k && kCompiledCodes[Is].m == m
                 ? (f(std::integral_constant<size_t, Is>{}), true)
                 : false) ||
            ...);
}
template <class F>
inline bool with_code(int k, int m, F&& f) {
    return with_code(k, m, f, std::make_index_sequence<kNumCompiledCodes>{});
}

template <class P>
constexpr bool all_codes(P pred) {
    for (const CompiledCode& c : kCompiledCodes)
        if (!pred(c)) return false;
    return true;
}
static_assert(all_codes([](const CompiledCode& c) { return find_code(c.k, c.m) == &c; }),
              "rows unique");
static_assert(all_codes([](const CompiledCode& c) { return !c.ring_split || c.m % 2 == 0; }),
              "a split row has two units of m / 2 parity rows");
static_assert(all_codes([](const CompiledCode& c) {
                  return c.syn != Syn::psyn ||
                         (c.k <= 64 && c.m <= 32 && (c.k < c.m ? c.k : c.m) <= 16);
              }),
              "gf_psyn_kernel: KC <= 64, MC <= 32, RC = min(k, m) <= 16");
static_assert(all_codes([](const CompiledCode& c) {
                  return c.syn != Syn::bsyn || (c.k % 2 == 0 && c.m <= 8);
              }),
              "gf_bsyn_kernel: KC % 2 == 0, MC <= 8");
static_assert(all_codes([](const CompiledCode& c) { return !c.psyn_wide || c.syn == Syn::psyn; }),
              "psyn_wide is a gf_psyn fact");

}  // namespace qfec
