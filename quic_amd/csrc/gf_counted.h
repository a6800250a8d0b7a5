// gf_counted.h — what the counted-vmcnt kernels share (gf_stream / gf_ring, gf_bsyn, gf_psyn,
// gf_dcol).  These kernels keep their own count of the VMEM instructions they issued and wait
// with immediate `s_waitcnt vmcnt(N)`, so the primitives that emit VMEM instructions, and the
// ones that order them, are stated once here: the wait, the buffer -> LDS DMA, the scalar-cache
// table loads, the sub-row read / realign / store of a bit-sliced block, the wide (LDS-staged)
// store and the empty-range padding stores.  Where a helper handles one word, sub-row or store,
// the loop over them stays in the kernel: the kernels' code is sensitive to where the compiler
// first sees those loops, and this way it is what it was when each kernel spelled them out.  tests/test_isa.py checks that the compiler adds no
// VMEM instruction or vmcnt wait of its own to any of them.
//
// Builtins and "v" constraints sit behind __HIP_DEVICE_COMPILE__: in the host pass they would
// void the host stub of the kernel that calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfec {

#define QF_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define QF_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt is 6 bits on gfx9");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n in [LO, HI]: binary dispatch.
template <int LO, int HI>
__device__ __forceinline__ void wait_vmcnt_upto(int n) {
    if constexpr (LO == HI) {
        wait_vmcnt<LO>();
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (n <= MID) wait_vmcnt_upto<LO, MID>(n);
        else wait_vmcnt_upto<MID + 1, HI>(n);
    }
}

// 16 bytes per lane from buffer rs at voff + soff into LDS at lds + 16 * lane (AUX 2: nt).
// Lanes whose offset lies past the buffer's range load zeros.
template <int AUX = 2>
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, uint8_t* lds, uint32_t voff,
                                      int soff = 0) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, QF_LPTR(lds), 16, voff, soff, 0, AUX);
#else
    (void)rs, (void)lds, (void)voff, (void)soff;
#endif
}

// Dword at byte offset o / byte i of a 4-byte-aligned table the kernel never writes, through
// the scalar cache (constant address space): a byte load (global_load_ubyte, or flat_load
// after an integer-to-pointer cast) would be a VMEM instruction outside the vmcnt bookkeeping.
// The index keeps the caller's width (a 32-bit one stays 32-bit scalar arithmetic).
template <class I>
__device__ __forceinline__ uint32_t cload_u32(const uint8_t* base, I o) {
    return ((const __attribute__((address_space(4))) uint32_t*)(base))[o >> 2];
}
template <class I>
__device__ __forceinline__ int cload_u8(const uint8_t* base, I i) {
    return (int)((cload_u32(base, i & ~(I)3) >> (8 * (i & 3))) & 0xFFu);
}

constexpr unsigned kLaneDrop = 0x80000000u;   // buffer offset past any range: lane dropped

// the lane id, recomputed where it is used (v_mbcnt): nothing lane-derived stays live across
// a block loop
__device__ __forceinline__ int lane_here() {
    int l = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
#endif
    return l;
}

// a value made opaque to the optimiser (not hoisted, folded or precomputed across blocks)
__device__ __forceinline__ void opaque_v(uint32_t& x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#else
    (void)x;
#endif
}

// A block of 8 sub-rows of S bytes, one column word of each sub-row per lane, streamed as its
// 16-byte aligned envelope (blocks may start 8 bytes off a 16-byte boundary).
template <int S>
struct SubrowShape {
    static constexpr int BB = 8 * S;
    static constexpr int NW = (S + 3) / 4, NWF = S / 4;        // column words; full words
    static constexpr int SPR = 1 + ((S >> 1) & 1) + (S & 1);   // stores per sub-row
    static constexpr int BUFB = (BB + 8 + 15) / 16 * 16;        // the 16-byte envelope
    static constexpr int NPC = BUFB > 1024 ? 2 : 1;              // DMA instructions per block
    static constexpr int P1L = BUFB > 1024 ? (BUFB - 1024) / 16 : 0;   // lanes of the 2nd
};

// The sub-row helpers take S = sub-row bytes at compile time, or S = 0 and s at run time.
//
// Column word of the 8 sub-rows as aligned dword pairs, L = the lane's word of sub-row 0 (block
// start + 4c, the block start 4-byte aligned): sub-row t is misaligned by (t * s) & 3, realigned
// at use.
template <int S>
__device__ __forceinline__ void read_subrows(const uint8_t* L, uint32_t (&lo)[8],
                                             uint32_t (&hi)[8], int s = S) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int o = t * s;
        const uint32_t* q = (const uint32_t*)(L + (o & ~3));
        lo[t] = q[0];
        hi[t] = (S == 0 || (o & 3)) ? q[1] : 0u;
    }
}

// Word t of them, realigned (v_alignbyte).
template <int S>
__device__ __forceinline__ uint32_t realign_word(const uint32_t (&lo)[8], const uint32_t (&hi)[8],
                                                 int t, int s = S) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int o = t * s;
    return (S == 0 || (o & 3)) ? __builtin_amdgcn_alignbyte(hi[t], lo[t], o & 3) : lo[t];
#else
    return lo[t];
#endif
}
// Lane offsets of the narrow store: 4 * word for the lanes that hold a full word (vo: lane <
// NWF) and for the lane of the tail word (vt: lane NWF when NWF < NW), every other lane dropped.
// Two address VGPRs, opaque so they are not hoisted as one precomputed offset per (output,
// sub-row).
struct SubrowLanes {
    uint32_t vo, vt;
};
__device__ __forceinline__ SubrowLanes subrow_lanes(int lane, int word, int NW, int NWF) {
    SubrowLanes v;
    v.vo = lane < NWF ? 4u * (uint32_t)word : kLaneDrop;
    v.vt = (lane == NWF && NWF < NW) ? 4u * (uint32_t)word : kLaneDrop;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v.vo), "+v"(v.vt));
#endif
    return v;
}

// Sub-row r of a block through buffer rs (the block's BB bytes), fixed instruction count: a b32
// store of the full words, plus b16 / b8 for the 2 or 3 bytes of the tail word (run-time s:
// all three are issued, the ones s does not need dropped).  A block is the 8 sub-rows in order.
template <int S, int AUX>
__device__ __forceinline__ void store_subrow(__amdgpu_buffer_rsrc_t rs, uint32_t vsum, int r,
                                             SubrowLanes v, int s = S) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_buffer_store_b32(vsum, rs, v.vo, r * s, AUX);
    if (S == 0 || (S & 2))
        __builtin_amdgcn_raw_buffer_store_b16((uint16_t)vsum, rs, (s & 2) ? v.vt : kLaneDrop, r * s,
                                              AUX);
    if (S == 0 || (S & 1))
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(vsum >> (8 * (s & 2))), rs,
                                             (s & 1) ? v.vt : kLaneDrop, r * s + (s & 2), AUX);
#else
    (void)rs, (void)vsum, (void)r, (void)v, (void)s;
#endif
}
template <int S, int AUX>
__device__ __forceinline__ void store_subrows(__amdgpu_buffer_rsrc_t rs, const uint32_t (&acc)[8],
                                              SubrowLanes v, int s = S) {
#pragma unroll
    for (int r = 0; r < 8; ++r) store_subrow<S, AUX>(rs, acc[r], r, v, s);
}

// a 64-bit value as the two-dword vector the 8-byte buffer store takes (low dword first)
typedef unsigned qf_u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ qf_u32x2_t qf_u32x2(uint64_t v) {
    qf_u32x2_t r = {(unsigned)v, (unsigned)(v >> 32)};
    return r;
}

// stage_block_169(lds, w, lane): writes one 1352-byte block (8 sub-rows of 169 B) that the wave
// holds bit-sliced (lane c < 43: column word c of each sub-row, bytes 169 t + 4 c ..) to LDS at
// byte address `lds` (8-byte aligned) as its contiguous bytes, with ALIGNED ds_write_b32 only
// (an unaligned one is replayed slowly and measured wrong).  Sub-row t starts a = (t * 169) & 3
// bytes into a dword: lane c writes the dword at 169 t - a + 4 c, built from its own word and
// lane c - 1's (ds_bpermute); lane 0 takes the bytes before the
// sub-row (the previous sub-row's last four, read from its lane 42 into an SGPR).  Sub-rows are
// written in order, so where lane 42's dword runs into the next sub-row, that sub-row's lane 0
// overwrites it with the merged bytes.  Lanes >= 43 must be inactive (exec).  Inline asm with
// its own lgkmcnt waits (as C++ LDS accesses the compiler would first wait for every LDS-DMA in
// flight).
__device__ __forceinline__ void stage_block_169(uint32_t lds, const uint32_t (&w)[8], int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int S = 169;
    const uint32_t qa = lds + 4u * (uint32_t)lane;
    const uint32_t pa = 4u * (uint32_t)(lane - 1);   // lane 0's is replaced below
    uint32_t p[8];   // lane c - 1's word of each sub-row
    asm volatile(
        "ds_bpermute_b32 %0, %8, %9\n\t"
        "ds_bpermute_b32 %1, %8, %10\n\t"
        "ds_bpermute_b32 %2, %8, %11\n\t"
        "ds_bpermute_b32 %3, %8, %12\n\t"
        "ds_bpermute_b32 %4, %8, %13\n\t"
        "ds_bpermute_b32 %5, %8, %14\n\t"
        "ds_bpermute_b32 %6, %8, %15\n\t"
        "ds_bpermute_b32 %7, %8, %16\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3]), "=&v"(p[4]), "=&v"(p[5]),
          "=&v"(p[6]), "=&v"(p[7])
        : "v"(pa), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]),
          "v"(w[7]));
    uint32_t X = 0;   // previous sub-row's bytes 165..168 (wave-uniform)
    const bool l0 = lane == 0;
#define QF_STAGE_T(T)                                                                         \
    {                                                                                         \
        constexpr int a = ((T) * S) & 3;                                                      \
        const uint32_t prev = l0 ? X : p[T];                                                  \
        const uint32_t v = a ? __builtin_amdgcn_alignbyte(w[T], prev, (4 - a) & 3) : w[T];    \
        asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(qa), "v"(v), "n"((T) * S - a)      \
                     : "memory");                                                             \
        if ((T) < 7)                                                                          \
            X = (uint32_t)__builtin_amdgcn_readlane(                                          \
                (int)__builtin_amdgcn_alignbyte(w[T], p[T], 1), 42);                          \
    }
    QF_STAGE_T(0) QF_STAGE_T(1) QF_STAGE_T(2) QF_STAGE_T(3)
    QF_STAGE_T(4) QF_STAGE_T(5) QF_STAGE_T(6) QF_STAGE_T(7)
#undef QF_STAGE_T
#else
    (void)lds, (void)w, (void)lane;
#endif
}

// A staged 1352-byte block (stage_block_169) through buffer rs as 3 dwordx2 stores of contiguous
// bytes instead of 8 x (b32 + b8) sub-row stores: 3 x 512 B read back from the wave's staging
// buffer (1360 bytes: the tail word's 3 extra bytes of a sub-row land on the next sub-row's
// start, overwritten by its later write; the last one's inside the staging pad) and stored as
// contiguous 8-byte lanes (past the block: dropped by the buffer range; the reads past 1360 B
// touch the next wave's buffer or read zeros, unused).  ra = stage + 8 * lane.
template <int AUX>
__device__ __forceinline__ void store_staged_169(__amdgpu_buffer_rsrc_t rs, uint32_t ra,
                                                 int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t v0, v1, v2;
    asm volatile("ds_read_b64 %0, %3\n\t"
                 "ds_read_b64 %1, %3 offset:512\n\t"
                 "ds_read_b64 %2, %3 offset:1024\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2)
                 : "v"(ra)
                 : "memory");
    const uint64_t vv[3] = {v0, v1, v2};
#pragma unroll
    for (int h = 0; h < 3; ++h)
        __builtin_amdgcn_raw_buffer_store_b64(qf_u32x2(vv[h]), rs, 512u * h + 8u * (uint32_t)lane,
                                              0, AUX);
#else
    (void)rs, (void)ra, (void)lane;
#endif
}

// Empty-range stores (nothing is written): they stand where a group's real stores would, so
// every group sees the same VMEM history and its waits stay immediates.  pad_store(none, q) is
// number q of a run, at its own offset so the run is not merged as duplicate stores; none =
// pad_rsrc(out).  Unrolled runs need no more.  A rolled loop also needs a compiler barrier
// after each store: without it the stores of gf_psyn's padding loop were merged into ONE
// instruction, so a group with fewer than RC recovered blocks issued 3 n + 1 stores and the next
// group's vmcnt(WAIT0) could pass before its block had landed in LDS.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pad_rsrc(uint8_t* out) {
    return __builtin_amdgcn_make_buffer_rsrc(out, 0, 0u, 0x00020000);
}
__device__ __forceinline__ void pad_store(__amdgpu_buffer_rsrc_t none, int q) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_buffer_store_b32(0u, none, 0u, 4 * q, 0);
#else
    (void)none, (void)q;
#endif
}

}  // namespace qfec
