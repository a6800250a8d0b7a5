// gf_psyn.hip — syndrome decode of the QuicR preset codes at 1350-byte payloads:
// FEC_10_10, FEC_10_15, FEC_10_20, FEC_15_15 (quic_fec_group.cc:22-82), bb = 1352, any
// erasure count up to min(k, m).
//
// The reference decodes in two stages (cauchy_256_decode, cauchy_256.cpp:1269-1420; for
// more than 4 erasures its windowed forms win_original :578-653 and
// win_gaussian_elimination :809-1018): eliminate the received originals from the recovery
// rows, then solve the r x r system over the erased rows.  Here, with y_s the received
// parity rows sorted ascending and e_j the erased data rows ascending:
//   T_y = R_y ^ sum_{present x} C[y][x] D_x          syndromes of ALL m parity rows, with
//                                                    the compile-time coefficients of the
//                                                    preset code (windowed form, one
//                                                    v_bitop3 per (row, sub-row), no
//                                                    scalar dispatch)
//   T_s <- T_{y_s}                                   in place: y_s >= s, ascending
//   Gauss-Jordan on S[s][j] = C[y_s][e_j], replayed on the data in place: for pivot p,
//   T_i ^= g[p][i] * T_p for every slot i (g[p][p] = 1 ^ 1/S'[p][p] normalises the pivot
//   row by linearity), one W/Z expansion of T_p per pivot, r^2 run-time applies per group
//   T_j = E_{e_j}
// For m >= 7 the reference's matrix is C[y][x] = b_x / (b_x + g_y) (cauchy_256.cpp:
// 459-477; row 0, all ones, is g_0 = 0 and b_0 = 1): a column-scaled Cauchy matrix with
// distinct nodes (checked for these codes by tests/test_psyn_prep.py), so every square
// submatrix of it is nonsingular and the elimination needs no pivoting in any row order.
// The recovered bytes are the unique solution, so the result is bit-exact with the
// reference's bit-matrix elimination.  A zero pivot can only come from a malformed receive
// set (a repeated parity row): status -3, group unchanged, as in every other decode here.
//
// Against the run-time decode it replaces (gf_stream_kernel<decode>, k x r run-time applies
// with two scalar nibble dispatches each): (10, 10) at 5 losses goes from 50 run-time
// applies per group to 25, and the other 5 x 10 row contributions are compile-time.
//
// Stream: as gf_bsyn (every wave owns groups g0, g0 + W, ...; a group's k received blocks in
// the order of the prep's table (decode_prep_psyn_kernel, decode_prep.hip; psyn:: in
// fec_kernels.h): present data rows ascending, then the extras in slot order; each
// block's 16-byte aligned envelope DMA'd into a ring of D + 1 block buffers, read at its
// 8-byte skew).  Groups of odd k start 8 bytes off a 16-byte boundary; the block address
// decides the skew.  Loads go through a buffer resource bounded by the end of the input, so
// the envelope of the last block of the buffer reads zeros past it.
//
// vmcnt bookkeeping as in gf_bsyn: a block is NPC DMA instructions; a group's stores
// (8 * SPR per recovered block) sit in the count before the waits for the next group's
// blocks 1 .. D - 1.  tests/test_isa.py checks the compiler adds no VMEM instruction or
// vmcnt wait of its own.
#include "gf_psyn.h"

namespace qfec {

// ------------------------------------------------------------------ launchers
// The codes compiled here are the Syn::psyn rows of compiled_codes.h, at 1352-byte blocks: the
// QuicR presets with m >= 7 (their matrices are column-scaled Cauchy matrices: no pivoting
// needed) and FEC_5_5, whose 5 x 5 matrix (the ones row and CAUCHY_MATRIX_5's rows,
// cauchy_256.cpp:428-442) has every square submatrix nonsingular (checked exhaustively by
// tests/test_psyn_prep.py), so it needs no pivoting either.
bool gf_psyn_supported(int k, int m, int bb, int rmax, const Tune& t) {
    return t.psyn && t.const_enc && rmax <= 16 && find_code(k, m, bb, Syn::psyn);
}

hipError_t launch_gf_psyn(const Apply& a) {
    const Tune& t = *a.t;
    if (a.groups <= 0) return hipSuccess;
    if (!gf_psyn_supported(a.k, a.m, a.bb, a.rmax, t)) return hipErrorInvalidValue;
    if ((((uintptr_t)a.in) & 15) ||
        ((((uintptr_t)a.tab) | (uintptr_t)a.cenc | (uintptr_t)a.slots) & 3))
        return hipErrorInvalidValue;
    using SH = SubrowShape<kPsynS>;
    // wide recovered-block stores: measured faster for (10, 10) (0.370-0.382 -> 0.348-0.356
    // ms) and (5, 5) (0.185 -> 0.156 ms); (15, 15) and (10, 20) unchanged, (10, 15) 0.392 ->
    // 0.410; so psyn_wide = 1 (default) takes them for the rows that say so and psyn_wide = 2
    // for every code; out 8-byte aligned
    const bool wide = (t.psyn_wide == 2 || (t.psyn_wide == 1 && find_code(a.k, a.m)->psyn_wide)) &&
                      ((((uintptr_t)a.out) | (uintptr_t)a.out_gstride) & 7) == 0;
    const size_t lds = (size_t)kPsynWaves * ((5 + 1) * SH::BUFB + (wide ? kPsynStage : 0));   // ring depth 5
    note_kernel("gf_psyn_kernel<decode,preset>");
    hipError_t e = hipErrorInvalidValue;
    with_code(a.k, a.m, [&](auto I) {
        constexpr CompiledCode c = kCompiledCodes[decltype(I)::value];
        if constexpr (c.syn == Syn::psyn) e = psyn_go<c.k, c.m>(a, lds, wide);
    });
    return e;
}

}  // namespace qfec
