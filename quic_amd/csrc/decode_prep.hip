// decode_prep.hip — the prep kernels of every m > 1 decode, and their launchers.
//
// A prep restates the reference's decode bookkeeping per group (cauchy_256_decode,
// net/quic/core/libcat/cauchy_256.cpp: sort_blocks :543-575, the erased rows ascending, the
// recovery blocks in array order receive them, the recovery row rewrite, the status codes)
// and replaces its GF(2) bitmatrix elimination by a GF(256) solve of the r x r erasure
// submatrix S[i][j] = C[y_i][e_j]: since c -> (8x8 expansion) is a ring homomorphism, the
// inverse bitmatrix is the expansion of S^-1, and the recovered data is unique.
//
// Five kernels, by lanes per group and by what the apply kernel reads:
//   decode_prep_kernel       64 lanes  coefficients per (output, input slot), or the syn::
//                                      table (gf_dcol's syndrome decode)
//   decode_prep_wide_kernel  16 lanes  coefficients            (k <= 64, rmax <= 16)
//   decode_prep_lane_kernel   4 lanes  coefficient dwords      (k <= 64, rmax <= 4)
//   decode_prep_bsyn_kernel   1 lane   bsyn:: table            (k <= 64, rmax <= 4)
//   decode_prep_psyn_kernel  16 lanes  psyn:: table            (k <= 64, rmax <= 16)
// The bookkeeping is stated once: stage_gf_and_cenc (LDS tables), classify (the status
// ladder), finish_group (rows, slots, rec_rows, nout, status), scan_tags_serial + invert4
// (lane, bsyn), scan_tags_16 (wide, psyn), write_stream_order (bsyn::, psyn::).  The solves
// differ where the algorithms do: wave-wide pivoting in LDS, 16-lane column-owned pivoting in
// LDS, psyn's row-per-lane elimination without pivoting that records g[p][i], and the 4 x 8
// register form.
//
// Contract of a group that is not decoded (status != 0, or no recovery block): rows, blocks
// and the recovered-blocks outputs are left as they are (rec_rows 255), nout = 0.
#include <algorithm>

#include "fec_kernels.h"
#include "gf256.h"
#include "gf_bitslice.h"
#include "gf_mixed.h"

namespace qfec {

__constant__ GfTables c_gf = make_gf_tables();

// Lanes of one wave exchange data through LDS without barriers: a wave's LDS operations
// execute in order, so wave_sync() only has to stop the compiler from reordering them.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// GF(256) through the exp / log tables in LDS.
struct GfLds {
    const uint8_t* exp;   // 512
    const uint8_t* log;   // 256
    __device__ __forceinline__ int mul(int a, int b) const {
        return (a && b) ? exp[log[a] + log[b]] : 0;
    }
    __device__ __forceinline__ int inv(int a) const { return exp[255 - log[a]]; }
};

// The workgroup's LDS copies of exp / log and of the m x k encode matrix (the inner loops
// read all three at random).  The caller's barrier follows.
__device__ __forceinline__ void stage_gf_and_cenc(uint8_t* gexp, uint8_t* glog, uint8_t* lcenc,
                                                  const uint8_t* __restrict__ cenc, int mk) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) gexp[i] = c_gf.exp[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) glog[i] = c_gf.log[i];
    for (int i = threadIdx.x; i < mk; i += blockDim.x) lcenc[i] = cenc[i];
}

// The status of a group before its solve.  kGo: it has erasures to solve.
constexpr int kGo = 1;
constexpr int kMalformed = -3;   // malformed receive set; also a singular / zero-pivot solve
__device__ __forceinline__ int classify(int nrec, int nera, int rmax, int k, int m, int bb,
                                        bool any_bad_row) {
    if (nrec == 0) return 0;                            // :1287-1289
    if (k + m > 256 || (bb & 7)) return -1;             // :1292-1294
    // more recovery blocks than erased rows or than the code corrects, or a row >= k + m
    if (nrec > rmax || nera < nrec || any_bad_row) return kMalformed;
    return kGo;
}

// A call's row / slot outputs (kernel arguments, the same for every group).
struct PrepOut {
    const uint8_t* rows_in;
    uint8_t* rows_out;    // null: recovered-blocks layout
    uint8_t* rec_rows;    // null: slot layout
    uint8_t* slots;
    int32_t* nout;
    int32_t* status;
    int k, rmax;
    // Strides of the per-group arrays, in entries per group: rows at g * kstride(), rec_rows
    // and slots at g * rstride(), the prep's table at coef + table_at().  A call of one code
    // strides by its own k and rmax; a mixed batch (PrepOutMixed) carries the set's as members.
    __device__ __forceinline__ int kstride() const { return k; }
    __device__ __forceinline__ int rstride() const { return rmax; }
    __device__ __forceinline__ long long table_at(long long g, int nchunk, int k_, int rcp) const {
        return g * (long long)nchunk * k_ * rcp;
    }
};
struct PrepOutMixed : PrepOut {
    int ks, rs;                 // the set's kmax and rmax
    long long tab_gstride;      // the set's table bytes per group
    __device__ __forceinline__ int kstride() const { return ks; }
    __device__ __forceinline__ int rstride() const { return rs; }
    __device__ __forceinline__ long long table_at(long long g, int, int, int) const {
        return g * tab_gstride;
    }
};

// The epilogue of group g, run by the nl lanes that share it (lane = 0 .. nl - 1; nl = 1:
// one lane writes everything).  rg: the group's tags as read; recpos(j) / era(j): the slot
// of recovery block j and the erased row it receives, j < n.  n = 0 leaves the group
// unchanged with status st.
template <class Out, class RecPos, class Era>
__device__ __forceinline__ void finish_group(const Out& o, long long g, int lane, int nl,
                                             const uint8_t* rg, int n, int st, RecPos recpos,
                                             Era era) {
    const uint8_t* rgg = o.rows_in + g * o.kstride();
    uint8_t* ro = o.rows_out ? o.rows_out + g * o.kstride() : nullptr;
    uint8_t* rec = o.rec_rows ? o.rec_rows + g * o.rstride() : nullptr;
    if (ro && ro != rgg)
        for (int i = lane; i < o.k; i += nl) ro[i] = rg[i];
    if (nl > 1) wave_sync();
    for (int j = lane; j < n; j += nl) {
        o.slots[g * o.rstride() + j] = (uint8_t)recpos(j);
        if (ro) ro[recpos(j)] = (uint8_t)era(j);        // :791
    }
    if (rec)
        for (int j = lane; j < o.rmax; j += nl) rec[j] = j < n ? (uint8_t)era(j) : 255;
    if (lane == 0) {
        o.nout[g] = n;
        if (o.status) o.status[g] = st;
    }
}

// ------------------------------------------------------------- one wave per group
// Persistent: each wave walks groups w, w + W, ...  Output, per recovered row e_j:
//   e_j = sum_i Sinv[j][i] * R_i + sum_{x present} (sum_i Sinv[j][i] C[y_i][x]) * D_x
// so one coefficient per (j, input slot) and a single pass over the received blocks; in
// syndrome mode the syn:: table instead (cauchy_256.cpp:1269-1420: the originals are
// eliminated from the recovery rows, T_i = R_i ^ sum_{data slots} C[y_i][row] D_slot, then
// e_j = sum_i Sinv[j][i] T_i).
struct PrepScratch {
    uint8_t* rowl;      // 256
    uint8_t* present;   // 256
    uint8_t* recpos;    // 256: slot of recovery i
    uint8_t* era;       // 256: erased row j
    uint8_t* recidx;    // 256: recovery index of slot (255 = original)
    uint8_t* mat;       // rmax x (2 rmax)
};

// [S | I] -> [I | Sinv] in LDS, the wave's lanes across the columns.  false: singular
__device__ __forceinline__ bool invert_wave(uint8_t* mat, int n, int lane, const GfLds& gf) {
    const int n2 = 2 * n;
    for (int p = 0; p < n; ++p) {
        int piv = -1;
        for (int base = p; base < n && piv < 0; base += 64) {
            const int i = base + lane;
            const unsigned long long msk = __ballot(i < n && mat[i * n2 + p] != 0);
            if (msk) piv = base + __ffsll((long long)msk) - 1;
        }
        if (piv < 0) return false;
        if (piv != p) {
            for (int j = lane; j < n2; j += 64) {
                const uint8_t t = mat[p * n2 + j];
                mat[p * n2 + j] = mat[piv * n2 + j];
                mat[piv * n2 + j] = t;
            }
            wave_sync();
        }
        const int inv = gf.inv(mat[p * n2 + p]);
        wave_sync();
        for (int j = lane; j < n2; j += 64) mat[p * n2 + j] = (uint8_t)gf.mul(mat[p * n2 + j], inv);
        wave_sync();
        for (int i = 0; i < n; ++i) {
            if (i == p) continue;
            const uint8_t f = mat[i * n2 + p];
            wave_sync();
            if (f)
                for (int j = lane; j < n2; j += 64)
                    mat[i * n2 + j] ^= (uint8_t)gf.mul(f, mat[p * n2 + j]);
            wave_sync();
        }
    }
    return true;
}

// The syn:: table of an unchanged group: a stream of k extras in slot order that feeds no
// syndrome row (the apply kernel still reads every group's k blocks); for gf_dcol every row
// position a zero block, no extras.
__device__ __forceinline__ void write_syn_unchanged(uint8_t* tb, int lane, int k) {
    for (int i = lane; i < k; i += 64) tb[syn::kPerm + i] = (uint8_t)i;
    if (lane < 5) ((uint32_t*)(tb + syn::kMask))[lane] = 0;   // mask and need
    for (int x = lane; x < 128; x += 64) tb[syn::kRowSlot + x] = 255;
    if (lane == 0) *(uint32_t*)(tb + syn::kNExt) = 0;
}

// The syn:: table of a group with n erasures (k <= 128; present[x] = a slot of row x + 1).
__device__ __forceinline__ void write_syn_table(uint8_t* tb, int lane, const PrepScratch& sc,
                                                int k, int n) {
    const uint8_t* rowl = sc.rowl;
    const uint8_t* present = sc.present;
    int np = 0;
    for (int base = 0; base < 128; base += 64) {   // present rows ascending
        const int x = base + lane;
        const bool pres = x < k && present[x] != 0;
        const unsigned long long msk = __ballot(pres);
        const int pre = __popcll(msk & ((1ull << lane) - 1));
        if (pres) tb[syn::kPerm + np + pre] = (uint8_t)(present[x] - 1);
        if (lane < 2)
            ((uint32_t*)(tb + syn::kMask))[base / 32 + lane] = (uint32_t)(msk >> (32 * lane));
        np += __popcll(msk);
    }
    int ne = 0;
    for (int base = 0; base < k; base += 64) {     // extras in slot order
        const int i = base + lane;
        const bool ext = i < k && (rowl[i] >= k || present[rowl[i]] != i + 1);
        const unsigned long long msk = __ballot(ext);
        const int pre = __popcll(msk & ((1ull << lane) - 1));
        if (ext) {
            tb[syn::kPerm + np + ne + pre] = (uint8_t)i;
            tb[syn::kERow + ne + pre] = rowl[i];
        }
        ne += __popcll(msk);
    }
    // gf_dcol: the slot of each data row (255: erased), the parity row of each syndrome,
    // the count of extras
    for (int x = lane; x < 128; x += 64)
        tb[syn::kRowSlot + x] = x < k && present[x] ? (uint8_t)(present[x] - 1) : (uint8_t)255;
    if (lane < n) tb[syn::kYmap + lane] = (uint8_t)(rowl[sc.recpos[lane]] - k);
    if (lane == 0) *(uint32_t*)(tb + syn::kNExt) = (uint32_t)ne;
    uint32_t need = 0;
    for (int i = 0; i < n; ++i) need |= 1u << (rowl[sc.recpos[i]] - k);
    if (lane < n) tb[syn::kISlot + rowl[sc.recpos[lane]] - k] = (uint8_t)lane;
    if (lane == 0) *(uint32_t*)(tb + syn::kNeed) = need;
    for (int idx = lane; idx < n * n; idx += 64) {
        const int j = idx / n, i = idx % n;
        tb[syn::kSinv + j * 16 + i] = sc.mat[j * 2 * n + n + i];
    }
}

template <class Out>
__device__ __forceinline__ void prep_group(long long g, int lane, const GfLds& gf,
                                           const PrepScratch& sc, const Out& o,
                                           const uint8_t* cenc, uint8_t* __restrict__ coef, int m,
                                           int bb, int rc, int nchunk, bool syndrome) {
    uint8_t* rowl = sc.rowl;
    uint8_t* present = sc.present;
    uint8_t* recpos = sc.recpos;
    uint8_t* era = sc.era;
    uint8_t* recidx = sc.recidx;
    uint8_t* mat = sc.mat;
    const int k = o.k;
    const int rcp = rc < 4 ? 4 : rc;
    for (int i = lane; i < 256; i += 64) {
        present[i] = 0;
        recidx[i] = 255;
    }
    const uint8_t* rg = o.rows_in + g * o.kstride();
    for (int i = lane; i < k; i += 64) rowl[i] = rg[i];
    wave_sync();
    // present[x] != 0: data row x received; syndrome mode keeps one of its slots + 1
    for (int i = lane; i < k; i += 64)
        if (rowl[i] < k) present[rowl[i]] = syndrome ? (uint8_t)(i + 1) : 1;
    wave_sync();
    // recovery blocks in array order (sort_blocks); bad: one of them tagged row >= k + m
    int nrec = 0;
    bool bad = false;
    for (int base = 0; base < k; base += 64) {
        const int i = base + lane;
        const bool isrec = i < k && rowl[i] >= k;
        const unsigned long long msk = __ballot(isrec);
        const int pre = __popcll(msk & ((1ull << lane) - 1));
        if (isrec) {
            recpos[nrec + pre] = (uint8_t)i;
            recidx[i] = (uint8_t)(nrec + pre);
        }
        bad |= __ballot(isrec && rowl[i] - k >= m) != 0;
        nrec += __popcll(msk);
    }
    // erasures: the first nrec data rows not present, ascending
    int nera = 0;
    for (int base = 0; base < k && nera < nrec; base += 64) {
        const int x = base + lane;
        const bool miss = x < k && !present[x];
        const unsigned long long msk = __ballot(miss);
        const int pre = __popcll(msk & ((1ull << lane) - 1));
        if (miss && nera + pre < nrec) era[nera + pre] = (uint8_t)x;
        nera += __popcll(msk);
    }
    wave_sync();

    int st = classify(nrec, nera, o.rmax, k, m, bb, bad);
    int n = st == kGo ? nrec : 0;
    const int n2 = 2 * n;
    if (n) {
        // [S | I]
        for (int idx = lane; idx < n * n2; idx += 64) {
            const int i = idx / n2, j = idx % n2;
            uint8_t v;
            if (j < n) v = cenc[(rowl[recpos[i]] - k) * k + era[j]];
            else v = (j - n == i) ? 1 : 0;
            mat[i * n2 + j] = v;
        }
        wave_sync();
        if (!invert_wave(mat, n, lane, gf)) {
            st = kMalformed;
            n = 0;
        }
    }
    uint8_t* tb = coef + o.table_at(g, nchunk, k, rcp);   // the group's table
    if (syndrome) {
        if (n) write_syn_table(tb, lane, sc, k, n);
        else write_syn_unchanged(tb, lane, k);
    }
    // recovery coefficients per (output j, input slot pos)
    for (int pos = lane; pos < k && !syndrome; pos += 64) {
        const int ri = recidx[pos];
        for (int j = 0; j < n; ++j) {
            const uint8_t* inv_row = mat + j * n2 + n;   // Sinv[j][*]
            int cval;
            if (ri != 255) {
                cval = inv_row[ri];
            } else {
                const int x = rowl[pos];
                cval = 0;
                for (int i = 0; i < n; ++i)
                    cval ^= gf.mul(inv_row[i], cenc[(rowl[recpos[i]] - k) * k + x]);
            }
            const int ch = j / rc, jj = j % rc;
            tb[((long long)ch * k + pos) * rcp + jj] = (uint8_t)cval;
        }
    }
    finish_group(o, g, lane, 64, rowl, n, st == kGo ? 0 : st,
                 [&](int j) { return recpos[j]; }, [&](int j) { return era[j]; });
}

__global__ __launch_bounds__(256) void decode_prep_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* rows_out, int32_t* __restrict__ status,
    const uint8_t* __restrict__ cenc, uint8_t* __restrict__ coef, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int k, int m,
    int bb, int rc, int rmax, int nchunk, int scratch_bytes, int syndrome) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* gexp = smem;              // 512
    uint8_t* glog = gexp + 512;        // 256
    uint8_t* lcenc = glog + 256;       // m x k
    const int cbytes = (m * k + 15) & ~15;
    stage_gf_and_cenc(gexp, glog, lcenc, cenc, m * k);
    __syncthreads();
    const int nwv = blockDim.x >> 6;
    const int w = wave_id(), lane = threadIdx.x & 63;
    uint8_t* base = lcenc + cbytes + (size_t)w * scratch_bytes;
    const PrepScratch sc{base, base + 256, base + 512, base + 768, base + 1024, base + 1280};
    const GfLds gf{gexp, glog};
    const PrepOut o{rows_in, rows_out, rec_rows, slots, nout, status, k, rmax};
    for (long long g = (long long)blockIdx.x * nwv + w; g < groups;
         g += (long long)gridDim.x * nwv)
        prep_group(g, lane, gf, sc, o, lcenc, coef, m, bb, rc, nchunk, syndrome != 0);
}

// The same prep over a mixed batch (gf_mixed.h): group g's code is codes[code[g]], its k, m and
// encode matrix are read per group, its rows lie at g * kmax, its rec_rows / slots at g * rmax
// (the set's largest) and its table at coef + g * coef_gstride.  Groups whose code has m == 1
// or k <= 1, or names no code of the set, are xor_copy_mixed_kernel's.  The group's own bb
// enters classify, so the status -1 of bb % 8 != 0 needs no fix-up pass.
// LDS: exp / log, the offsets of the codes' matrices, then (stage_cenc) every decodable code's
// m x k matrix, then the per-wave scratch; without stage_cenc (the matrices do not fit beside
// one wave's scratch) cenc is read from memory through the cache.
__global__ __launch_bounds__(256) void decode_prep_mixed_kernel(
    const uint8_t* __restrict__ rows_in, int32_t* __restrict__ status,
    const MixedCode* __restrict__ codes, int ncodes, const uint8_t* __restrict__ code,
    const int32_t* __restrict__ bbs, uint8_t* __restrict__ coef, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int kmax,
    int rmax, int rc, long long coef_gstride, int scratch_bytes, int stage_cenc, int cenc_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* gexp = smem;                       // 512
    uint8_t* glog = gexp + 512;                 // 256
    int32_t* loff = (int32_t*)(glog + 256);     // kMixedMaxCodes offsets into lcenc
    uint8_t* lcenc = (uint8_t*)(loff + kMixedMaxCodes);
    for (int i = threadIdx.x; i < 512; i += blockDim.x) gexp[i] = c_gf.exp[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) glog[i] = c_gf.log[i];
    if (stage_cenc) {
        int at = 0;   // the same running offset in every thread
        for (int c = 0; c < ncodes; ++c) {
            const int mk = codes[c].cenc ? codes[c].m * codes[c].k : 0;
            if (threadIdx.x == 0) loff[c] = at;
            for (int i = threadIdx.x; i < mk; i += blockDim.x) lcenc[at + i] = codes[c].cenc[i];
            at += (mk + 15) & ~15;
        }
    }
    __syncthreads();
    const int nwv = blockDim.x >> 6;
    const int w = wave_id(), lane = threadIdx.x & 63;
    uint8_t* base = lcenc + (stage_cenc ? cenc_bytes : 0) + (size_t)w * scratch_bytes;
    const PrepScratch sc{base, base + 256, base + 512, base + 768, base + 1024, base + 1280};
    const GfLds gf{gexp, glog};
    for (long long g = (long long)blockIdx.x * nwv + w; g < groups;
         g += (long long)gridDim.x * nwv) {
        const int ci = __builtin_amdgcn_readfirstlane((int)code[g]);
        if (ci >= ncodes) continue;
        const int k = __builtin_amdgcn_readfirstlane(codes[ci].k);
        const int m = __builtin_amdgcn_readfirstlane(codes[ci].m);
        if (k <= 1 || m <= 1) continue;
        const int bb = __builtin_amdgcn_readfirstlane(bbs[g]);
        const int rg = min(k, m);
        // a code with k + m > 256 has no matrix: classify answers before one is read
        const uint8_t* cenc = stage_cenc ? lcenc + loff[ci] : codes[ci].cenc;
        const PrepOutMixed o{{rows_in, nullptr, rec_rows, slots, nout, status, k, rg}, kmax, rmax,
                             coef_gstride};
        prep_group(g, lane, gf, sc, o, cenc, coef, m, bb, rc, 0, false);
        for (int j = rg + lane; j < rmax; j += 64) rec_rows[g * rmax + j] = 255;
    }
}

// ------------------------------------------------------------- 16 lanes per group
// The bookkeeping of wide and psyn (k <= 64, at most 16 erasures).  The group's lane l holds
// slots l, l + 16, l + 32, l + 48 (ballots over the group's 16-lane segment `seg` of the
// wave) and entry l of the lists.  A wave holds four groups; the lanes of a group exchange
// data through LDS in program order (one wave: no barrier).
constexpr int kLanes16 = 16;
struct Scan16 {
    uint64_t isrec;     // bit i: slot i holds a recovery block
    uint64_t present;   // bit r: data row r was received
    uint64_t first;     // bit i: slot i holds the first copy of its data row (FIRST only)
    int myrec, myy, myera;   // the l-th recovery slot, its parity row, the l-th erased row
    int n;              // erasures to solve (0: the group stays unchanged)
    int st;             // kGo or the group's status
};

__device__ __forceinline__ uint64_t seg16(uint64_t ballot, int seg) {
    return (ballot >> (kLanes16 * seg)) & 0xFFFFull;
}

// lists[0 .. 2][j], j < n: recpos, y (array order), era, visible to the group's lanes on
// return.  live = false: a group past the batch (n = 0, nothing read).
template <bool FIRST>
__device__ __forceinline__ Scan16 scan_tags_16(const uint8_t* rg, bool live, int l, int seg,
                                               uint8_t (*lists)[16], int k, int m, int bb,
                                               int rmax) {
    Scan16 s{};
    uint64_t isdat = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = kLanes16 * q + l;
        const int r = (live && i < k) ? rg[i] : 0;
        const bool rec = live && i < k && r >= k;
        const bool dat = live && i < k && r < k;
        if (dat) s.present |= 1ull << r;
        s.isrec |= seg16(__ballot(rec), seg) << (kLanes16 * q);
        if (FIRST) isdat |= seg16(__ballot(dat), seg) << (kLanes16 * q);
    }
#pragma unroll
    for (int o = 1; o < kLanes16; o <<= 1) s.present |= __shfl_xor(s.present, o, kLanes16);
    if (FIRST) {
        s.first = isdat;
        if (__popcll(isdat) != __popcll(s.present)) {   // a repeated data row (rare)
            s.first = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = kLanes16 * q + l;
                bool fst = (isdat >> i) & 1;
                if (fst)
                    for (int j = 0; j < i; ++j)
                        if (rg[j] == rg[i]) { fst = false; break; }
                s.first |= seg16(__ballot(fst), seg) << (kLanes16 * q);
            }
        }
    }
    const int nrec = __popcll(s.isrec);
    const uint64_t kmask = k == 64 ? ~0ull : ((1ull << k) - 1);
    const uint64_t missing = ~s.present & kmask;
    s.myrec = s.myera = -1;
    {
        uint64_t a = s.isrec, e = missing;
        for (int j = 0; j < l && a; ++j) a &= a - 1;
        for (int j = 0; j < l && e; ++j) e &= e - 1;
        if (a) s.myrec = __ffsll((long long)a) - 1;
        if (e) s.myera = __ffsll((long long)e) - 1;
    }
    s.myy = s.myrec >= 0 ? rg[s.myrec] - k : 0;
    const bool badrow = l < nrec && s.myy >= m;                 // row >= k + m
    s.st = classify(nrec, __popcll(missing), rmax, k, m, bb, seg16(__ballot(badrow), seg) != 0);
    s.n = s.st == kGo ? nrec : 0;                               // <= rmax <= 16
    if (l < s.n) {
        lists[0][l] = (uint8_t)s.myrec;
        lists[1][l] = (uint8_t)s.myy;
        lists[2][l] = (uint8_t)s.myera;
    }
    wave_sync();
    return s;
}

// Coefficients for small groups with up to 16 erasures (the QuicR presets (5, 5) .. (15, 15)
// at 1350-byte payloads).  The 16 lanes split the slots for the bookkeeping, then the columns
// of [S | I] (lane l owns columns l and l + 16 of the group's n x 2n matrix in LDS) for the
// Gauss-Jordan inverse, then the slots again for the per-slot coefficients.  One wave per
// group runs a chain of wave-wide LDS round trips instead: 270 us for 65,536 (10, 10) groups
// with 5 losses.
__global__ __launch_bounds__(256) void decode_prep_wide_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* rows_out, int32_t* __restrict__ status,
    const uint8_t* __restrict__ cenc, uint8_t* __restrict__ coef, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int k, int m,
    int bb, int rc, int rmax, int nchunk) {
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    constexpr int GPB = 256 / kLanes16;                         // groups per block
    __shared__ uint8_t lrows[GPB][64];
    __shared__ uint8_t lmat[GPB][16][32];                       // [S | I], row-major
    __shared__ uint8_t llist[GPB][3][16];                       // recpos, y, era
    extern __shared__ __attribute__((aligned(16))) uint8_t lcenc[];   // m x k
    stage_gf_and_cenc(gexp, glog, lcenc, cenc, m * k);
    const long long gfirst = (long long)blockIdx.x * GPB;
    const int ng = (int)min((long long)GPB, groups - gfirst);
    for (int i = threadIdx.x; i < ng * k; i += blockDim.x)
        lrows[i / k][i % k] = rows_in[gfirst * k + i];
    __syncthreads();
    const int gl = threadIdx.x / kLanes16, l = threadIdx.x % kLanes16;
    const int seg = (threadIdx.x & 63) / kLanes16;              // the group's 16 lanes in the wave
    if (gl >= ng) return;                                       // whole groups: no barrier below
    const long long g = gfirst + gl;
    const uint8_t* rg = lrows[gl];
    uint8_t (*M)[32] = lmat[gl];
    const uint8_t* lrec = llist[gl][0];
    const uint8_t* ly = llist[gl][1];
    const uint8_t* lera = llist[gl][2];
    const GfLds gf{gexp, glog};
    const Scan16 s = scan_tags_16<false>(rg, true, l, seg, llist[gl], k, m, bb, rmax);
    int n = s.n, st = s.st;
    // ---- [S | I], S[i][j] = C[y_i][e_j]: lane l fills columns l and l + 16
    for (int i = 0; i < n; ++i) {
        const int yi = ly[i];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = l + kLanes16 * h;
            if (c < 2 * n) M[i][c] = c < n ? lcenc[yi * k + lera[c]] : (uint8_t)(c - n == i);
        }
    }
    wave_sync();
    // ---- Gauss-Jordan (the lanes own columns; rows through LDS)
    for (int p = 0; p < n; ++p) {
        int piv = -1;
        for (int i = p; i < n && piv < 0; ++i)
            if (M[i][p]) piv = i;                                 // the same for every lane
        if (piv < 0) {                                            // singular
            st = kMalformed;
            n = 0;
            break;
        }
        if (piv != p) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = l + kLanes16 * h;
                if (c < 2 * n) {
                    const uint8_t t = M[p][c];
                    M[p][c] = M[piv][c];
                    M[piv][c] = t;
                }
            }
            wave_sync();
        }
        const int inv = gf.inv(M[p][p]);
        wave_sync();                                              // every lane read M[p][p]
        int rowp[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = l + kLanes16 * h;
            rowp[h] = c < 2 * n ? gf.mul(M[p][c], inv) : 0;
            if (c < 2 * n) M[p][c] = (uint8_t)rowp[h];
        }
        for (int i = 0; i < n; ++i) {
            if (i == p) continue;
            const int f = M[i][p];                               // before column p changes
            wave_sync();
            if (f) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = l + kLanes16 * h;
                    if (c < 2 * n) M[i][c] ^= (uint8_t)gf.mul(f, rowp[h]);
                }
            }
            wave_sync();
        }
    }
    // ---- coefficients per (output j, input slot pos): recovery slot ri: Sinv[j][ri]; data
    // row x: sum_i Sinv[j][i] C[y_i][x]
    const int rcp = rc < 4 ? 4 : rc;
    uint8_t* tb = coef + g * (long long)nchunk * k * rcp;
    for (int pos = l; pos < k; pos += kLanes16) {
        const bool isr = (s.isrec >> pos) & 1;
        const int ri = isr ? __popcll(s.isrec & ((1ull << pos) - 1)) : -1;
        const int x = rg[pos];
        for (int j = 0; j < n; ++j) {
            int cval;
            if (isr) {
                cval = M[j][n + ri];
            } else {
                cval = 0;
                for (int i = 0; i < n; ++i) cval ^= gf.mul(M[j][n + i], lcenc[ly[i] * k + x]);
            }
            const int ch = j / rc, jj = j % rc;
            tb[((long long)ch * k + pos) * rcp + jj] = (uint8_t)cval;
        }
    }
    const PrepOut o{rows_in, rows_out, rec_rows, slots, nout, status, k, rmax};
    finish_group(o, g, l, kLanes16, rg, n, st == kGo ? 0 : st,
                 [&](int j) { return lrec[j]; }, [&](int j) { return lera[j]; });
}

__device__ __forceinline__ int psyn_byte(const uint32_t (&w)[4], int c) {
    const uint32_t v = c < 4 ? w[0] : c < 8 ? w[1] : c < 12 ? w[2] : w[3];
    return (int)((v >> (8 * (c & 3))) & 0xFFu);
}

// The stream order both compact syndrome tables begin with (bsyn::, psyn::: kPerm at 0, kMask
// at 64, kERow at KEROW), written by the lanes lane, lane + stride, ... of the group.  A
// changed group streams its present rows ascending (first copy of each), then the extras in
// slot order; an unchanged one streams its slots in order as no-op extras (row tag 255).
static_assert(bsyn::kPerm == 0 && psyn::kPerm == 0 && bsyn::kMask == 64 && psyn::kMask == 64,
              "the compact syndrome tables share their head");
template <int KEROW>
__device__ __forceinline__ void write_stream_order(uint8_t* T, int lane, int stride,
                                                   const uint8_t* rg, int k, uint64_t present,
                                                   uint64_t first, bool changed) {
    const uint64_t kmask = k == 64 ? ~0ull : ((1ull << k) - 1);
    const uint64_t extra = ~first & kmask;
    const int np = __popcll(present);
    if (!changed) {
        for (int i = lane; i < k; i += stride) {
            T[i] = (uint8_t)i;
            T[KEROW + i] = 255;
        }
    } else {
        for (int i = lane; i < k; i += stride) {
            const int r = rg[i];
            if ((first >> i) & 1) {
                T[__popcll(present & ((1ull << r) - 1))] = (uint8_t)i;
            } else {
                const int e = __popcll(extra & ((1ull << i) - 1));
                T[np + e] = (uint8_t)i;
                T[KEROW + e] = (uint8_t)r;
            }
        }
    }
    if (lane == 0) {
        *(uint32_t*)(T + 64) = changed ? (uint32_t)present : 0u;
        *(uint32_t*)(T + 68) = changed ? (uint32_t)(present >> 32) : 0u;
    }
}

// The psyn:: table of the compiled QuicR preset codes (gf_psyn.hip): Gauss-Jordan without
// pivoting on S[s][j] = C[y_s][e_j] (received parity rows ascending), recording per pivot p
// the coefficient g[p][i] the kernel applies to T_p for slot i.  k <= 64, m <= 32.  Lane s
// holds row s of S in registers (16 bytes); a pivot row reaches the group's lanes by four
// shuffles, and a row update is n GF(256) products through the LDS log / exp tables.
__global__ __launch_bounds__(256) void decode_prep_psyn_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* rows_out, int32_t* __restrict__ status,
    const uint8_t* __restrict__ cenc, uint8_t* __restrict__ tab, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int k, int m,
    int bb, int rmax) {
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    constexpr int GPB = 256 / kLanes16;                         // groups per block
    __shared__ uint8_t lrows[GPB][64];
    __shared__ uint8_t llist[GPB][3][16];                       // recpos, y (array order), era
    __shared__ __attribute__((aligned(16))) uint8_t ltab[GPB][psyn::kBytes];
    __shared__ uint8_t lsrc[GPB][16];                           // lane of row s
    extern __shared__ __attribute__((aligned(16))) uint8_t lcenc[];   // m x k
    stage_gf_and_cenc(gexp, glog, lcenc, cenc, m * k);
    const long long gfirst = (long long)blockIdx.x * GPB;
    const int ng = (int)min((long long)GPB, groups - gfirst);
    for (int i = threadIdx.x; i < ng * k; i += blockDim.x)
        lrows[i / k][i % k] = rows_in[gfirst * k + i];
    for (int i = threadIdx.x; i < GPB * psyn::kBytes / 4; i += blockDim.x)
        ((uint32_t*)ltab)[i] = 0;
    __syncthreads();
    const int gl = threadIdx.x / kLanes16, l = threadIdx.x % kLanes16;
    const int seg = (threadIdx.x & 63) / kLanes16;              // the group's 16 lanes in the wave
    const int sbase = (threadIdx.x & 63) - l;                   // lane 0 of the group in the wave
    const bool live = gl < ng;
    const long long g = gfirst + gl;
    const uint8_t* rg = lrows[gl];
    const uint8_t* lrec = llist[gl][0];
    const uint8_t* ly = llist[gl][1];
    const uint8_t* lera = llist[gl][2];
    uint8_t* T = ltab[gl];
    const Scan16 s = scan_tags_16<true>(rg, live, l, seg, llist[gl], k, m, bb, rmax);
    int n = s.n, st = s.st;
    const int myy = s.myy;
    // ---- row s of S = C[ys_s][e_j] in lane s (s = the rank of y_l: sorted ascending, ties by
    // array order), packed 4 bytes per dword
    int mys = 0;
    for (int j = 0; j < n; ++j) mys += (ly[j] < myy) || (ly[j] == myy && j < l);
    uint32_t row[4] = {0u, 0u, 0u, 0u};
    if (l < n) {
#pragma unroll
        for (int j = 0; j < 16; ++j)   // compile-time indices: row[] stays in registers
            if (j < n) row[j >> 2] |= (uint32_t)lcenc[myy * k + lera[j]] << (8 * (j & 3));
    }
    // lane l ends up holding row s = mys; the shuffles below address rows by s, so the lane
    // holding row s is found through lsrc
    if (l < n) lsrc[gl][mys] = (uint8_t)l;
    wave_sync();
    const int ok_n = n;
    // ---- Gauss-Jordan without pivoting (every leading minor of a Cauchy submatrix is
    // nonzero); a zero pivot means a repeated parity row
    for (int p = 0; p < ok_n; ++p) {
        const int src = sbase + lsrc[gl][p];
        uint32_t prow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) prow[q] = (uint32_t)__shfl((int)row[q], src, 64);
        const int piv = psyn_byte(prow, p);
        if (piv == 0) {
            st = kMalformed;
            n = 0;
            break;
        }
        const int linv = 255 - glog[piv];                       // log of the inverse pivot
        const int inv = gexp[linv];
        const bool me = mys == p;
        const int f = psyn_byte(row, p);
        // the coefficient the kernel applies to T_p (before this step) for slot mys
        int lg = 0, gco = 0;
        if (me) {
            gco = 1 ^ inv;
            lg = linv;                                          // new row p = inv * row p
        } else if (f) {
            lg = glog[f] + linv;                                // row ^= (f / piv) * row p
            gco = gexp[lg];
        }
        if (lg >= 255) lg -= 255;                               // lg + log(x) < 512: gexp's range
        if (l < ok_n) T[psyn::kCoef + 16 * p + mys] = (uint8_t)gco;
        if (l < ok_n && (me || f)) {
            uint32_t nrow[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                if (c < ok_n) {
                    const int pc = psyn_byte(prow, c);
                    const int prod = pc ? gexp[lg + glog[pc]] : 0;
                    nrow[c >> 2] |= (uint32_t)prod << (8 * (c & 3));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) row[q] = me ? nrow[q] : (row[q] ^ nrow[q]);
        }
    }
    write_stream_order<psyn::kERow>(T, l, kLanes16, rg, k, s.present, s.first, n > 0);
    if (n > 0) {
        if (l < n) T[psyn::kYs + mys] = (uint8_t)myy;
        // the syndrome rows the solve uses: the kernel accumulates only these
        uint32_t need = l < n ? 1u << myy : 0u;
#pragma unroll
        for (int o = 1; o < kLanes16; o <<= 1)
            need |= (uint32_t)__shfl_xor((int)need, o, kLanes16);
        if (l == 0) *(uint32_t*)(T + psyn::kNeed) = need;
    }
    if (live) {
        const PrepOut o{rows_in, rows_out, rec_rows, slots, nout, status, k, rmax};
        finish_group(o, g, l, kLanes16, rg, n, st == kGo ? 0 : st,
                     [&](int j) { return lrec[j]; }, [&](int j) { return lera[j]; });
    }
    __syncthreads();
    // coalesced copy of the block's tables
    uint32_t* dst = (uint32_t*)(tab + gfirst * (long long)psyn::kBytes);
    const int nd = ng * psyn::kBytes / 4;
    for (int d = threadIdx.x; d < nd; d += blockDim.x) dst[d] = ((const uint32_t*)ltab)[d];
}

// ------------------------------------------------------------- one lane's own copy
// lane and bsyn (k <= 64, k % 4 == 0, rmax <= 4): every lane of the group runs the whole
// bookkeeping and the r x r inverse in registers with the log / exp tables in LDS, so a group
// costs a few hundred independent LDS reads instead of a chain of wave-wide LDS round trips
// (one wave per group: ~90 us for 65,536 (32, 4) groups, most of it latency).
// Packed small lists: byte j of recpos / recrow / era = entry j (j < 4).
__device__ __forceinline__ int byte_of(uint32_t v, int j) { return (int)((v >> (8 * j)) & 0xFF); }

struct Scan4 {
    uint64_t present;   // bit r: data row r was received
    uint64_t first;     // bit i: slot i holds the first copy of its data row (FIRST only)
    uint32_t recpos, recrow, era;   // slot and parity row of recovery block j, erased row j
    int n;              // erasures to solve (0: the group stays unchanged)
    int st;             // kGo or the group's status
};

// rg: the group's k tags in LDS, 4-byte aligned (read four at a time)
template <bool FIRST>
__device__ __forceinline__ Scan4 scan_tags_serial(const uint8_t* rg, int k, int m, int bb,
                                                  int rmax) {
    Scan4 s{};
    const uint32_t* rg4 = (const uint32_t*)rg;
    int nrec = 0;
    for (int i4 = 0; i4 < k; i4 += 4) {
        const uint32_t t4 = rg4[i4 >> 2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i4 + u;
            const int r = byte_of(t4, u);
            if (r < k) {
                if (FIRST && !((s.present >> r) & 1)) s.first |= 1ull << i;
                s.present |= 1ull << r;
            } else {
                if (nrec < 4) {
                    s.recpos |= (uint32_t)i << (8 * nrec);
                    s.recrow |= (uint32_t)(r - k < 255 ? r - k : 255) << (8 * nrec);
                }
                ++nrec;
            }
        }
    }
    const uint64_t kmask = k == 64 ? ~0ull : ((1ull << k) - 1);
    uint64_t missing = ~s.present & kmask;
    bool bad = false;                                           // row >= k + m
    for (int i = 0; i < min(nrec, 4); ++i) bad |= byte_of(s.recrow, i) >= m;
    s.st = classify(nrec, __popcll(missing), rmax, k, m, bb, bad);
    s.n = s.st == kGo ? nrec : 0;
    for (int j = 0; j < s.n; ++j) {
        const int e = __ffsll((long long)missing) - 1;
        missing &= missing - 1;
        s.era |= (uint32_t)e << (8 * j);
    }
    return s;
}

// [S | I] -> [I | Sinv], S[i][j] = C[y_i][e_j], Gauss-Jordan fully unrolled over the 4 x 8
// maximum.  false: singular (the elimination still runs to its end, on zeros)
__device__ __forceinline__ bool invert4(uint8_t (&M)[4][8], const Scan4& s, const uint8_t* lcenc,
                                        int k, const GfLds& gf) {
    const int n = s.n;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint8_t v = 0;
            if (i < n && j < n) v = lcenc[byte_of(s.recrow, i) * k + byte_of(s.era, j)];
            else if (i < n && j >= 4) v = (j - 4 == i) ? 1 : 0;
            M[i][j] = v;
        }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (p < n) {
            int piv = -1;
#pragma unroll
            for (int i = 3; i >= p; --i)
                if (i < n && M[i][p] != 0) piv = i;
            if (piv < 0) {
                ok = false;
                piv = p;
            }
#pragma unroll
            for (int i = p + 1; i < 4; ++i) {
                if (i == piv) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint8_t t = M[p][j];
                        M[p][j] = M[i][j];
                        M[i][j] = t;
                    }
                }
            }
            const int inv = M[p][p] ? gf.inv(M[p][p]) : 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) M[p][j] = (uint8_t)gf.mul(M[p][j], inv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i != p && i < n) {
                    const int f = M[i][p];
                    if (f) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) M[i][j] ^= (uint8_t)gf.mul(f, M[p][j]);
                    }
                }
            }
        }
    }
    return ok;
}

// Four lanes per group, each computing the coefficients of every fourth input slot (lane
// q == 0 writes the rest).  A group left unchanged gets no coefficients it could use
// (nout = 0: the apply skips it).
__global__ __launch_bounds__(256) void decode_prep_lane_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* rows_out, int32_t* __restrict__ status,
    const uint8_t* __restrict__ cenc, uint8_t* __restrict__ coef, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int k, int m,
    int bb, int rmax) {
    // LDS: exp/log tables, the m x k encode matrix, the block's row tags [64][k] (loaded
    // coalesced) and its coefficient dwords [64][k + 1] (stored coalesced at the end)
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];
    uint8_t* lcenc = lsm;                                       // m x k (padded to 16)
    constexpr int LPG = 4;                                      // lanes per group
    constexpr int GPB = 256 / LPG;                              // groups per block
    uint8_t* lrows = lsm + ((m * k + 15) & ~15);                // GPB x k
    uint32_t* lcoef = (uint32_t*)(lrows + GPB * k);             // GPB x (k + 1), k % 4 == 0
    stage_gf_and_cenc(gexp, glog, lcenc, cenc, m * k);
    const long long gfirst = (long long)blockIdx.x * GPB;
    const int ng = (int)min((long long)GPB, groups - gfirst);
    {
        const uint32_t* src = (const uint32_t*)(rows_in + gfirst * k);   // 4-byte aligned
        const int nd = ng * k / 4;
#pragma unroll 4
        for (int i = threadIdx.x; i < nd; i += blockDim.x) ((uint32_t*)lrows)[i] = src[i];
    }
    __syncthreads();
    const int gl = threadIdx.x / LPG, q = threadIdx.x % LPG;
    const long long g = gfirst + gl;
    const bool live = gl < ng;
    // every lane runs the body (dead lanes on a copy of group 0's tags, no global writes)
    // so that the block reaches the coalesced coefficient store together
    const uint8_t* rg = lrows + (live ? gl : 0) * k;
    const uint32_t* rg4 = (const uint32_t*)rg;
    uint32_t* mycoef = lcoef + gl * (k + 1);
    const GfLds gf{gexp, glog};
    Scan4 s = scan_tags_serial<false>(rg, k, m, bb, rmax);
    uint8_t M[4][8];
    if (!invert4(M, s, lcenc, k, gf)) {
        s.st = kMalformed;
        s.n = 0;
    }
    const int n = s.n;
    // log of S^-1 (256 = zero)
    int lsi[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (j < n && i < n) ? M[j][4 + i] : 0;
            lsi[j][i] = v ? glog[v] : 256;
        }
    // coefficient dword per input slot: byte j = recovered row j's coefficient
    for (int pos4 = 4 * q; pos4 < k; pos4 += 4 * LPG) {
      const uint32_t t4 = rg4[pos4 >> 2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // four independent lookup chains
        const int pos = pos4 + u;
        int ri = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n && byte_of(s.recpos, i) == pos) ri = i;
        uint32_t cw = 0;
        if (ri >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) {
                    int v = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i == ri) v = M[j][4 + i];
                    cw |= (uint32_t)v << (8 * j);
                }
        } else if (n > 0) {
            const int x = byte_of(t4, u);
            int acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < n) {
                    const int cv = lcenc[byte_of(s.recrow, i) * k + x];
                    if (cv) {
                        const int lc = glog[cv];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n && lsi[j][i] != 256) acc[j] ^= gexp[lsi[j][i] + lc];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) cw |= (uint32_t)acc[j] << (8 * j);
        }
        mycoef[pos] = cw;
      }
    }
    if (live && q == 0) {
        const PrepOut o{rows_in, rows_out, rec_rows, slots, nout, status, k, rmax};
        finish_group(o, g, 0, 1, rg, n, s.st == kGo ? 0 : s.st,
                     [&](int j) { return byte_of(s.recpos, j); },
                     [&](int j) { return byte_of(s.era, j); });
    }
    __syncthreads();
    // coalesced store of the block's coefficient rows [ng][k] dwords
    uint32_t* cdst = (uint32_t*)(coef + gfirst * (long long)k * 4);
    const int nd = ng * k;
#pragma unroll 4
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        const int gg = d / k;
        cdst[d] = lcoef[gg * (k + 1) + (d - gg * k)];
    }
}

// One lane per group: the bsyn:: table of the compiled (32, 4) code (gf_bsyn.hip).
__global__ __launch_bounds__(256) void decode_prep_bsyn_kernel(
    const uint8_t* __restrict__ rows_in, uint8_t* rows_out, int32_t* __restrict__ status,
    const uint8_t* __restrict__ cenc, uint8_t* __restrict__ tab, uint8_t* __restrict__ slots,
    int32_t* __restrict__ nout, uint8_t* __restrict__ rec_rows, long long groups, int k, int m,
    int bb, int rmax) {
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];
    uint8_t* lcenc = lsm;                                    // m x k (padded to 16)
    uint8_t* lrows = lsm + ((m * k + 15) & ~15);             // 256 x k (k % 4 == 0)
    uint8_t* ltab = lrows + 256 * k;                         // 256 x kBytes
    stage_gf_and_cenc(gexp, glog, lcenc, cenc, m * k);
    const long long gfirst = (long long)blockIdx.x * 256;
    const int ng = (int)min(256LL, groups - gfirst);
    {
        const uint32_t* src = (const uint32_t*)(rows_in + gfirst * k);   // 4-byte aligned
        const int nd = ng * k / 4;
        for (int i = threadIdx.x; i < nd; i += blockDim.x) ((uint32_t*)lrows)[i] = src[i];
    }
    __syncthreads();
    const int gl = threadIdx.x;
    const long long g = gfirst + gl;
    const bool live = gl < ng;
    const uint8_t* rg = lrows + (live ? gl : 0) * k;
    uint8_t* T = ltab + gl * bsyn::kBytes;
    const GfLds gf{gexp, glog};
    Scan4 s = scan_tags_serial<true>(rg, k, m, bb, rmax);
    uint8_t M[4][8];
    if (!invert4(M, s, lcenc, k, gf)) {
        s.st = kMalformed;
        s.n = 0;
    }
    const int n = s.n;
    write_stream_order<bsyn::kERow>(T, 0, 1, rg, k, s.present, s.first, n > 0);
    if (n > 0) {
        *(uint32_t*)(T + bsyn::kY) = s.recrow;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t sw = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j < n && i < n) sw |= (uint32_t)M[j][4 + i] << (8 * i);
            *(uint32_t*)(T + bsyn::kSinv + 4 * j) = sw;
        }
    }
    if (live) {
        const PrepOut o{rows_in, rows_out, rec_rows, slots, nout, status, k, rmax};
        finish_group(o, g, 0, 1, rg, n, s.st == kGo ? 0 : s.st,
                     [&](int j) { return byte_of(s.recpos, j); },
                     [&](int j) { return byte_of(s.era, j); });
    }
    __syncthreads();
    // coalesced copy of the block's tables
    uint32_t* dst = (uint32_t*)(tab + gfirst * (long long)bsyn::kBytes);
    const int nd = ng * bsyn::kBytes / 4;
    for (int d = threadIdx.x; d < nd; d += blockDim.x) dst[d] = ((const uint32_t*)ltab)[d];
}

// ---------------------------------------------------------------------- launchers
hipError_t launch_decode_prep(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                              int rc, int rmax, long long groups, hipStream_t st, const Tune& t,
                              bool syndrome) {
    if (groups <= 0) return hipSuccess;
    const DecodeWork& w = io.w;
    if (syndrome && (k > 128 || m > 16 || (long long)((rmax + rc - 1) / rc) * k * std::max(rc, 4) <
                                                 syn::kBytes))
        return hipErrorInvalidValue;
    const size_t cbytes = ((size_t)m * k + 15) & ~(size_t)15;   // the encode matrix in LDS
    if (!syndrome && t.prep_lane && rmax <= 4 && k <= 64 && k % 4 == 0 && (long long)m * k <= 4096 && rc <= 4 &&
        ((((uintptr_t)w.coef) | (uintptr_t)io.rows_in) & 3) == 0) {
        const unsigned nb = (unsigned)((groups + 63) / 64);     // 64 groups x 4 lanes
        const size_t lds = cbytes + 64 * (size_t)k + 64 * (size_t)(k + 1) * 4;
        note_kernel("decode_prep_lane_kernel");
        qlaunch((decode_prep_lane_kernel), dim3(nb), dim3(256), lds, st, io.rows_in, io.rows_out,
                io.status, cenc, w.coef, w.slots, w.nout, io.rec_rows, groups, k, m, bb, rmax);
        return hipGetLastError();
    }
    const int nchunk = (rmax + rc - 1) / rc;
    if (!syndrome && t.prep_lane && k <= 64 && rmax <= 16 && (long long)m * k <= 16384) {
        note_kernel("decode_prep_wide_kernel");
        qlaunch((decode_prep_wide_kernel), dim3((unsigned)((groups + 15) / 16)), dim3(256),
                (uint32_t)cbytes, st, io.rows_in, io.rows_out, io.status, cenc, w.coef, w.slots,
                w.nout, io.rec_rows, groups, k, m, bb, rc, rmax, nchunk);
        return hipGetLastError();
    }
    const int scratch = (int)((1280 + (size_t)rmax * 2 * rmax + 15) & ~(size_t)15);
    const size_t fixed = 768 + cbytes;
    int nwv = 4;
    while (nwv > 1 && fixed + (size_t)nwv * scratch > 64 * 1024) nwv >>= 1;
    const size_t lds = fixed + (size_t)nwv * scratch;
    const unsigned nb = persistent_grid(groups, nwv, (long long)t.cus * 16, 0, 0);
    if (!nb) return hipErrorInvalidValue;
    note_kernel(syndrome ? "decode_prep_kernel<syndrome>" : "decode_prep_kernel");
    note_grid("decode_prep_kernel", nb);
    qlaunch((decode_prep_kernel), dim3(nb), dim3(nwv * 64), lds, st, io.rows_in, io.rows_out,
            io.status, cenc, w.coef, w.slots, w.nout, io.rec_rows, groups, k, m, bb, rc, rmax,
            nchunk, scratch, syndrome ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_decode_prep_mixed(const MixedSet& s, MixedView v, const PrepIO& io,
                                    long long groups, hipStream_t st, const Tune& t) {
    if (groups <= 0) return hipSuccess;
    const DecodeWork& w = io.w;
    const int scratch = (int)((1280 + (size_t)s.solve_rmax * 2 * s.solve_rmax + 15) & ~(size_t)15);
    const size_t head = 768 + kMixedMaxCodes * sizeof(int32_t);
    // the codes' matrices beside at least one wave's scratch, or read through the cache
    const bool stage = head + (size_t)s.cenc_bytes + scratch <= 64 * 1024;
    const size_t fixed = head + (stage ? (size_t)s.cenc_bytes : 0);
    int nwv = 4;
    while (nwv > 1 && fixed + (size_t)nwv * scratch > 64 * 1024) nwv >>= 1;
    const size_t lds = fixed + (size_t)nwv * scratch;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const unsigned nb = persistent_grid(groups, nwv, (long long)t.cus * 16, 0, 0);
    if (!nb) return hipErrorInvalidValue;
    note_kernel(stage ? "decode_prep_mixed_kernel" : "decode_prep_mixed_kernel<cached>");
    note_grid("decode_prep_mixed_kernel", nb);
    qlaunch((decode_prep_mixed_kernel), dim3(nb), dim3(nwv * 64), lds, st, io.rows_in, io.status,
            s.codes, s.ncodes, v.code, v.bb, w.coef, w.slots, w.nout, io.rec_rows, groups, s.kmax,
            s.rmax, s.dec_rc, s.coef_gstride, scratch, stage ? 1 : 0, s.cenc_bytes);
    return hipGetLastError();
}

hipError_t launch_decode_prep_bsyn(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                                   int rmax, long long groups, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    const DecodeWork& w = io.w;
    if (k > 64 || k % 4 != 0 || rmax > 4 || (long long)m * k > 4096 ||
        ((((uintptr_t)w.coef) | (uintptr_t)io.rows_in) & 3))
        return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((groups + 255) / 256);
    const size_t lds = (((size_t)m * k + 15) & ~(size_t)15) + 256 * (size_t)k +
                       256 * (size_t)bsyn::kBytes;
    note_kernel("decode_prep_bsyn_kernel");
    qlaunch((decode_prep_bsyn_kernel), dim3(nb), dim3(256), lds, st, io.rows_in, io.rows_out,
            io.status, cenc, w.coef, w.slots, w.nout, io.rec_rows, groups, k, m, bb, rmax);
    return hipGetLastError();
}

hipError_t launch_decode_prep_psyn(const PrepIO& io, const uint8_t* cenc, int k, int m, int bb,
                                   int rmax, long long groups, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    const DecodeWork& w = io.w;
    if (k > 64 || m > 32 || rmax > 16 || (((uintptr_t)w.coef) & 3))
        return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((groups + 15) / 16);
    note_kernel("decode_prep_psyn_kernel");
    qlaunch((decode_prep_psyn_kernel), dim3(nb), dim3(256),
            (uint32_t)(((size_t)m * k + 15) & ~(size_t)15), st, io.rows_in, io.rows_out,
            io.status, cenc, w.coef, w.slots, w.nout, io.rec_rows, groups, k, m, bb, rmax);
    return hipGetLastError();
}

}  // namespace qfec
