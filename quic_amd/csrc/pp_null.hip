// pp_null.hip — packet protection next to the FEC path (SURVEY.md §8 f, rank 4): the
// reference's NullEncrypter / NullDecrypter over batches of packets on the device.
//
// The fork's QuicEncrypter::Create maps kNULL to NullEncrypter and every negotiated AEAD
// (kAESG, kCC20) to MyEncrypter, an identity copy (crypto/quic_encrypter.cc:18-29,
// crypto/none_encrypter.cc EncryptPacket).  NullEncrypter is therefore the only packet
// protection of this reference with arithmetic in it:
//   seal (null_encrypter.cc:23-43):  wire = AD || tag12 || PT,  tag12 = the low 12 bytes
//        (little-endian, quic_utils.cc:175-181) of FNV-1a-128(AD || PT);
//   open (null_decrypter.cc DecryptPacket / ReadHash / ComputeHash): reject short input or
//        a tag that differs from FNV-1a-128(AD || CT[12..]) with its top 32 bits cleared;
//        the output holds a copy of the ciphertext before the check and the plaintext after.
//   FNV-1a-128 (quic_utils.cc:38-56,110-125): h = (h ^ byte) * (2^88 + 315) mod 2^128.
//
// The hash is a serial chain over the bytes of one packet, so one lane owns one packet's
// chain, while the bytes move in wave tiles (tile_stream): a wave's 64 packets stream through
// an 8 KB LDS tile in 128-byte windows.  Per window, 8 global_load_lds_dwordx4 bring 8
// packets x 128 contiguous bytes each (chunk c of packet q at slot c ^ (q & 7), an XOR
// swizzle so the lanes reading their own rows hit distinct banks); lane q hashes its packet's
// valid bytes from LDS and writes each full 16-byte output line (realigned to the output's byte
// phase, zeros past the source) back into the slot it consumed; then 8 coalesced
// global_store_dwordx4 in the same shape.  The two partial output lines at a packet's ends are
// written from registers after the loop.  Then the tag.
//
// The chain: h mod 2^96 (the tag is its low 96 bits) in three 32-bit words, one 64-bit
// multiply-add per word and byte (Fnv below).  Bound: the VALU of the chain and the tile's
// LDS round trips at four to five waves per SIMD.
//
// Grouped forms (the FEC group's view of its packets): every data and FEC packet of G groups
// sealed in one launch, and the receiver's open that writes each data packet's plaintext
// straight into its block slot, followed by one wave per group that fills the holes with the
// opened FEC packets and writes the row tags the decode reads.
//
// Ragged forms of the grouped kernels (a block size per group, the packed layout of
// gf_ragged.hip): the same kernel bodies, tile_stream and chain, instantiated with a row
// lookup that reads bb[g] and the group's byte offset per lane (RaggedRows, RaggedSlots); the
// uniform instantiations (PtRows, UniSlots) carry no run-time branch for them.  A tile that
// mixes block sizes runs its window loop to its longest packet.
//
// Framed forms (QuicFecGroup's wire format): a data packet's block is
// prefix || payload || zeros, its wire packet carries the payload alone.  The same bodies with
// FramedRows (the seal reads payload rows and parity blocks) and FramedSlots (the open places a
// data plaintext two bytes into its slot and writes the prefix), plus the two kernels that only
// move bytes through tile_stream: frame_blocks_kernel (payload rows -> blocks) and
// extract_revived_kernel (recovered blocks -> payload rows).
//
// Mixed forms (a (k, m) per group through a code set; pp_mixed.h): the
// framed sender and the arrival-order receiver over a geometry of two prefix tables.  The
// per-arrival and per-group kernels are one body over a geometry type (UniGeo, MixedGeo); the
// seal takes MixedRows, whose packets find their group by a search of the table
// (mixed_group_of); mixed_wire_plan_kernel decides every group once for all of them.
//
// Receiver window: the arrival-order receiver with its binding state kept
// on the device from call to call: every accepted packet is held in a row of its own, and a group
// that completes is decoded where it lies through pointer tables.  Its pre and open passes are the
// arrival-order kernels over one more slot type (WinSlots); the kernels of the carried state are
// its own (rxwin_*).  Every receiver forms a group's rows by wave_rows, both arrival-order
// assembles accept by wave_accept, and one host sequence (bind_go) launches both.
#include "fec_kernels.h"
#include "pp_null.h"
#include "pp_mixed.h"

namespace qfec {

namespace {

constexpr int kPPThreads = 256;   // one packet per lane
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// FNV-1a-128 modulo 2^96: the tag is the low 96 bits of the hash (quic_utils.cc:175-181,
// null_encrypter.cc:23-43; the decrypter compares the same bits), and arithmetic mod 2^128
// reduces to arithmetic mod 2^96, so bits 96..127 are never formed.  h is three 32-bit words;
// h * P = h * 315 + (h << 88): h * 315 is one 32 x 32 -> 64-bit multiply-add per word
// (v_mad_u64_u32; the low word's high half carries into the next, the top word's product is
// kept mod 2^32), and (h ^ byte) << 88 mod 2^96 is the XORed low byte shifted into bits 24..31
// of the top word.  About 8 VALU per byte, where r02-r06's five 22-bit limbs in carry-save form
// (v_mul_u32_u24 per limb, masks and shifts between) took 17; the chain alone runs 2.4x as
// fast (tools/microbench/fnv_rate.hip).
struct Fnv {
    uint32_t h0, h1, h2;
    // kOffset = 144066263297769815596495629667062367629 (quic_utils.cc:116-118) mod 2^96
    __device__ __forceinline__ void init() {
        h0 = 0x6295C58Du;
        h1 = 0x62B82175u;
        h2 = 0x07BB0142u;
    }
    __device__ __forceinline__ void byte(uint32_t b) {
        const uint32_t x0 = h0 ^ b;
        const uint64_t p0 = (uint64_t)x0 * 315u;
        const uint64_t p1 = (uint64_t)h1 * 315u + (p0 >> 32);
        h2 = h2 * 315u + (uint32_t)(p1 >> 32) + (x0 << 24);
        h0 = (uint32_t)p0;
        h1 = (uint32_t)p1;
    }
    __device__ __forceinline__ void word(uint32_t w) {
        byte(w & 0xFFu);
        byte((w >> 8) & 0xFFu);
        byte((w >> 16) & 0xFFu);
        byte(w >> 24);
    }
    // the low 96 bits of h, little-endian dwords (SerializeUint128Short, quic_utils.cc:175-181)
    __device__ __forceinline__ void tag(uint32_t& t0, uint32_t& t1, uint32_t& t2) const {
        t0 = h0, t1 = h1, t2 = h2;
    }
};

// stores through the global address space (a generic pointer compiles to flat stores, which
// also count on the LDS counter that tile_stream's waits after each ds_read use)
__device__ __forceinline__ void gst32(uint8_t* a, uint32_t v) {
    *(__attribute__((address_space(1))) uint32_t*)(uintptr_t)a = v;
}
__device__ __forceinline__ void gst8(uint8_t* a, uint32_t v) {
    *(__attribute__((address_space(1))) uint8_t*)(uintptr_t)a = (uint8_t)v;
}

// Per-lane byte-stream writer: bytes go out as aligned dword stores; `carry` holds the bytes
// of the current dword not yet stored.  Bytes before `start` are not the writer's: a dword
// that holds some of them is written byte by byte.
struct Sink {
    uint8_t* ptr;
    uint8_t* start;
    uint32_t carry;
    __device__ __forceinline__ void begin(uint8_t* p) {
        ptr = start = p;
        carry = 0;
    }
    __device__ __forceinline__ void store_dw(uint8_t* a, uint32_t v) {   // a 4-byte aligned
        if (a >= start) {
            gst32(a, v);
        } else {
            for (int q = (int)(start - a); q < 4; ++q) gst8(a + q, v >> (8 * q));
        }
    }
    __device__ __forceinline__ void word(uint32_t w) {
        const uint32_t pb = (uint32_t)(uintptr_t)ptr & 3u;
        const uint64_t v = ((uint64_t)w << (8 * pb)) | carry;
        store_dw(ptr - pb, (uint32_t)v);
        carry = (uint32_t)(v >> 32);
        ptr += 4;
    }
    __device__ __forceinline__ void byte(uint32_t b) {
        const uint32_t pb = (uint32_t)(uintptr_t)ptr & 3u;
        carry |= b << (8 * pb);
        ++ptr;
        if (pb == 3) {
            store_dw(ptr - 4, carry);
            carry = 0;
        }
    }
    __device__ __forceinline__ void flush() {
        const uint32_t pb = (uint32_t)(uintptr_t)ptr & 3u;
        uint8_t* a = ptr - pb;
        for (uint32_t q = 0; q < pb; ++q)
            if (a + q >= start) gst8(a + q, carry >> (8 * q));
    }
    // zero bytes up to `end`, then flush
    __device__ __forceinline__ void zeros_to(const uint8_t* end) {
        while (ptr < end && ((uintptr_t)ptr & 3u)) byte(0);
        while (ptr + 4 <= end) word(0);
        while (ptr < end) byte(0);
        flush();
    }
};

// One lane streams p[0 .. len): bytes up to 16-byte alignment, then 64-byte chunks of four
// 16-byte loads with the next chunk in flight while this one is consumed, then the last
// < 64 bytes.  HASH: into h; WRITE: through s.
constexpr int CH = 4;
template <bool HASH, bool WRITE, int CHN = CH, class H>
__device__ __forceinline__ void span(H& h, Sink& s, const uint8_t* p, int len) {
    if (len <= 0) return;
    auto dw = [&](uint32_t w) {
        if constexpr (HASH) h.word(w);
        if constexpr (WRITE) s.word(w);
    };
    auto by = [&](uint32_t b) {
        if constexpr (HASH) h.byte(b);
        if constexpr (WRITE) s.byte(b);
    };
    auto eat = [&](const u32x4& v) {
        dw(v.x);
        dw(v.y);
        dw(v.z);
        dw(v.w);
    };
    const int head = min(len, (int)((16u - ((uintptr_t)p & 15u)) & 15u));
    for (int i = 0; i < head; ++i) by(p[i]);
    const u32x4* q = (const u32x4*)(p + head);
    const int rest = len - head;
    const int nc = rest / (16 * CHN);   // 16 * CHN-byte chunks
    // Line writer for the chunks: 16 source bytes make 4 output dwords d0..d3 (realigned by
    // pb = ptr % 4 bytes with the carry), which land at dword positions di..di+3 of the
    // output's 16-byte lines (di = the dword index of ptr - pb in its line, fixed for the
    // span).  Rotated right by di they fill line L's positions di..3 and line L+1's 0..di-1:
    // line L = (positions < di ? the previous rotation : this one), one 16-byte store; the
    // first line is stored dword by dword from position di (the bytes before it are stored
    // already or are not this writer's), the last partial line by flush_line.
    const uint32_t pb = (uint32_t)(uintptr_t)s.ptr & 3u;
    const uint32_t di = ((uint32_t)((uintptr_t)s.ptr - pb) >> 2) & 3u;
    const uint32_t sh = 4u - pb;
    uint32_t P0 = 0, P1 = 0, P2 = 0, P3 = 0;
    auto eat4 = [&](const u32x4& v, bool first) {
        if constexpr (HASH) {
            h.word(v.x);
            h.word(v.y);
            h.word(v.z);
            h.word(v.w);
        }
        if constexpr (WRITE) {
            uint32_t d0 = v.x, d1 = v.y, d2 = v.z, d3 = v.w, nc4 = 0;
            if (pb) {
                d0 = (v.x << (8 * pb)) | s.carry;
                d1 = __builtin_amdgcn_alignbyte(v.y, v.x, sh);
                d2 = __builtin_amdgcn_alignbyte(v.z, v.y, sh);
                d3 = __builtin_amdgcn_alignbyte(v.w, v.z, sh);
                nc4 = v.w >> (8 * sh);
            }
            // rotate right by di: R[j] = d[(j - di) & 3]
            if (di & 1u) {
                const uint32_t t = d3;
                d3 = d2, d2 = d1, d1 = d0, d0 = t;
            }
            if (di & 2u) {
                uint32_t t = d0;
                d0 = d2, d2 = t;
                t = d1, d1 = d3, d3 = t;
            }
            uint8_t* line = s.ptr - pb - 4 * di;
            if (first) {
                if (di <= 0) s.store_dw(line, d0);
                if (di <= 1) s.store_dw(line + 4, d1);
                if (di <= 2) s.store_dw(line + 8, d2);
                s.store_dw(line + 12, d3);
            } else {
                u32x4 o;
                o.x = di > 0 ? P0 : d0;
                o.y = di > 1 ? P1 : d1;
                o.z = di > 2 ? P2 : d2;
                o.w = d3;
                *(__attribute__((address_space(1))) u32x4*)(uintptr_t)line = o;
            }
            P0 = d0, P1 = d1, P2 = d2, P3 = d3;
            s.carry = nc4;
            s.ptr += 16;
        }
    };
    u32x4 a[CHN], b[CHN];
    if (nc > 0) {
#pragma unroll
        for (int u = 0; u < CHN; ++u) a[u] = __builtin_nontemporal_load(q + u);
    }
    for (int j = 0; j < nc; j += 2) {
        if (j + 1 < nc) {
#pragma unroll
            for (int u = 0; u < CHN; ++u) b[u] = __builtin_nontemporal_load(q + CHN * (j + 1) + u);
        }
        eat4(a[0], j == 0);
#pragma unroll
        for (int u = 1; u < CHN; ++u) eat4(a[u], false);
        if (j + 1 < nc) {
            if (j + 2 < nc) {
#pragma unroll
                for (int u = 0; u < CHN; ++u)
                    a[u] = __builtin_nontemporal_load(q + CHN * (j + 2) + u);
            }
#pragma unroll
            for (int u = 0; u < CHN; ++u) eat4(b[u], false);
        }
    }
    if constexpr (WRITE) {
        // the line the chunks left open: positions 0 .. di - 1 hold P0 .. P(di - 1)
        if (nc > 0) {
            uint8_t* line = s.ptr - pb - 4 * di;
            if (di > 0) s.store_dw(line, P0);
            if (di > 1) s.store_dw(line + 4, P1);
            if (di > 2) s.store_dw(line + 8, P2);
        }
    }
    (void)P3;
    const u32x4* r = q + CHN * nc;
    const int nr = (rest % (16 * CHN)) >> 4;
#pragma unroll 1
    for (int u = 0; u < nr; ++u) eat(__builtin_nontemporal_load(r + u));
    const uint8_t* tb = (const uint8_t*)(r + nr);
    for (int i = 0; i < (rest & 15); ++i) by(tb[i]);
}

__device__ __forceinline__ int len_of(const int32_t* a, int all, long long i) {
    return a ? a[i] : all;
}

// ------------------------------------------------------------------ wave-tiled stream
// The packets of a wave are streamed through an 8 KB LDS tile in 128-byte windows, so that
// both the loads and the stores are coalesced: one wave instruction moves 8 packets x 128
// contiguous bytes (8 lanes per packet, 16 bytes each) instead of 64 packets x 16 bytes, which
// touched 64 cache lines per instruction and cost 1.4x the reads (L2 re-fetches) and 1.55x
// the writes (partial lines) of the one-lane-per-packet streamer (profiles/r05/pp/).  Each lane
// still owns its packet's serial FNV chain.
//   window w of packet q: source chunks 8w .. 8w + 7 (16 bytes each) counted from the source's
//   128-byte aligned line, so that a window is one whole cache line; the tile row of packet q
//   is 128 bytes at q * 128, chunk c at slot c ^ (q & 7) (an XOR swizzle: lanes reading their
//   rows at one chunk index hit distinct banks).
//   1. loads: 8 global_load_lds_dwordx4 (instruction j: packets 8j .. 8j + 7, lane = 8 (q % 8)
//      + slot), each lane's address from its packet's lane by ds_bpermute (all 8 exchanges
//      issued before the first load, so their latency is paid once, not 8 times);
//   2. lane q reads its 8 chunks, hashes the valid bytes, and writes each FULL 16-byte output
//      line (realigned to the output's phase, zeros past the source) back into the slot of the
//      chunk it just consumed; the partial lines at the output's two ends stay in registers;
//   3. stores: 8 global_store_dwordx4 in the same shape (full lines only; exchanges and LDS
//      reads four instructions at a time), plain stores: the
//      next window's vmcnt(0) waits for them too, and non-temporal stores were acknowledged
//      later for the same bytes written (r06: 1.13 -> 0.73 ms for all of A's packets, WRITE_SIZE
//      unchanged).
// After the last window, the two partial end lines are written from registers, whole dwords
// where the output covers them.
// Measured and not kept: 64-byte windows double-buffered, two packets
// per lane, 16-byte aligned windows (each window straddled two lines), and (r06) two window
// buffers with the next window's DMA in flight during the hash (64- and 128-byte windows).
constexpr int kTileBytes = 64 * 128;   // one wave's tile
constexpr int kTilePackets = 64;       // packets per wave (one per lane)

__device__ __forceinline__ uint32_t bperm(uint32_t v, int src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}
__device__ __forceinline__ uint64_t bperm64(uint64_t v, int src_lane) {
    return (uint64_t)bperm((uint32_t)v, src_lane) | ((uint64_t)bperm((uint32_t)(v >> 32), src_lane) << 32);
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// The output line at per-lane dword offset mi (0..4) and byte offset ri (0..3) into the 32
// bytes P || C (the previous chunk, this chunk): dword t = bytes 4 (mi + t) + ri .. + 3, dwords
// past the pair clamped to C[3].  The five dwords it needs are selected by the bits of mi in
// three steps, then realigned by ri.
__device__ __forceinline__ u32x4 line_of(const uint32_t (&P)[4], const uint32_t (&C)[4], int mi,
                                         int ri) {
    // bitwise selects: a conditional between array elements would be folded into one load
    // with a computed index, which puts the array in scratch memory
    const uint32_t A[8] = {P[0], P[1], P[2], P[3], C[0], C[1], C[2], C[3]};
    const uint32_t m0 = 0u - (uint32_t)(mi & 1), m1 = 0u - (uint32_t)((mi >> 1) & 1);
    const uint32_t m2 = 0u - (uint32_t)((mi >> 2) & 1);
    uint32_t B[7], Q[5], V[5];
#pragma unroll
    for (int t = 0; t < 7; ++t) B[t] = (A[t + 1] & m0) | (A[t] & ~m0);
#pragma unroll
    for (int t = 0; t < 5; ++t) Q[t] = (B[t + 2] & m1) | (B[t] & ~m1);
#pragma unroll
    for (int t = 0; t < 5; ++t) V[t] = (A[min(4 + t, 7)] & m2) | (Q[t] & ~m2);
    u32x4 o;
    o.x = __builtin_amdgcn_alignbyte(V[1], V[0], ri);
    o.y = __builtin_amdgcn_alignbyte(V[2], V[1], ri);
    o.z = __builtin_amdgcn_alignbyte(V[3], V[2], ri);
    o.w = __builtin_amdgcn_alignbyte(V[4], V[3], ri);
    return o;
}

// bytes [lo, hi) of the 16-byte line at L (16-byte aligned) from o: dword stores for the
// dwords inside the range, byte stores for the rest
__device__ __forceinline__ void part_line(uint8_t* L, const uint32_t (&o)[4], int lo, int hi) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (lo <= 4 * t && 4 * t + 4 <= hi) {
            gst32(L + 4 * t, o[t]);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo <= 4 * t + b && 4 * t + b < hi) gst8(L + 4 * t + b, o[t] >> (8 * b));
        }
    }
}

// Hash pl source bytes at src into h and write them to dst, followed by zeros up to olen
// bytes (olen == 0: hash only).  Called by every lane of the wave together (wave-uniform
// loop); a lane with pl == 0 and olen == 0 only takes part.  tile: this wave's kTileBytes of
// LDS.  Every memory access of the routine is complete when it returns.  The first window
// starts at the source's 128-byte aligned line: the bytes before src that it loads lie in
// that line (never another page) and are neither hashed nor written.
template <class H>
__device__ void tile_stream(H& h, const uint8_t* src, int pl, uint8_t* dst, int olen,
                            uint8_t* tile) {
    const int lane = (int)__lane_id();
    const uintptr_t sp = (uintptr_t)src;
    const int hoff = pl > 0 ? (int)(sp & 127u) : 0;
    const uint64_t s128 = (uint64_t)(sp - hoff);
    const int cmax = pl > 0 ? (hoff + pl - 1) >> 4 : -1;   // last chunk holding a source byte
    const int send = hoff + pl;                             // source end, chunk coordinates
    // output: stream byte x goes to D + x, D = dst - hoff; 16-byte lines from A0 = D rounded
    // down; the full lines jf .. jl lie inside [dst, dst + olen)
    const uint64_t D = (uint64_t)(uintptr_t)dst - (uint64_t)hoff;
    const int e = (int)(D & 15u);
    const uint64_t A0 = D - (uint64_t)e;
    int jf = 0, jl = -1;
    if (olen > 0) {
        jf = (int)(((uint64_t)(uintptr_t)dst - A0 + 15u) >> 4);
        jl = (int)(((uint64_t)(uintptr_t)dst + (uint64_t)olen - A0) >> 4) - 1;
    }
    // the partial output lines at the two ends: line jf - 1 (when dst is inside it) and line
    // jl + 1 (when the output ends inside it); the same line when the output lies in one line
    const bool hpart = olen > 0 && (uint64_t)(uintptr_t)dst != A0 + 16u * (uint64_t)jf;
    const bool tpart = olen > 0 && (uint64_t)(uintptr_t)dst + (uint64_t)olen != A0 + 16u * (uint64_t)(jl + 1);
    const int last = max(cmax, tpart ? jl + 1 : jl);
    const int nwin_l = last >= 0 ? (last >> 3) + 1 : 0;
    const int nwin = wave_max(nwin_l);
    // line g = stream bytes [16 g - e, 16 g - e + 16): from (previous chunk, this chunk)
    const int mi = (16 - e) >> 2, ri = (16 - e) & 3;
    uint32_t P[4] = {0u, 0u, 0u, 0u};
    uint32_t Hd[4] = {0u, 0u, 0u, 0u}, Tl[4] = {0u, 0u, 0u, 0u};
    const int lq = lane >> 3, pos = lane & 7;
    const int rowoff = lane * 128, sw = lane & 7;
    const uint32_t tb = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)tile;
#pragma unroll 1
    for (int w = 0; w < nwin; ++w) {
        // 1. coalesced loads: instruction j brings packets 8j .. 8j + 7
        {
            uint64_t qs[8];
            int qc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // every exchange first: one wait for all of them
                qs[j] = bperm64(s128, 8 * j + lq);
                qc[j] = (int)bperm((uint32_t)cmax, 8 * j + lq);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int q = 8 * j + lq;
                const int cg = 8 * w + (pos ^ (q & 7));
                if (cg <= qc[j])
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void*)(uintptr_t)(qs[j] + 16u * (uint64_t)cg),
                        (__attribute__((address_space(3))) void*)(tile + 1024 * j), 16, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // 2. this lane's row: hash, full output lines back into the tile, end lines kept
        if (w < nwin_l) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int g = 8 * w + c;
                const uint32_t a = tb + (uint32_t)(rowoff + ((c ^ sw) << 4));
                uint32_t C[4] = {0u, 0u, 0u, 0u};
                if (g <= cmax && 16 * g + 16 > hoff) {   // chunks before the source stay zero
                    u32x4 v;
                    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
                    C[0] = v.x, C[1] = v.y, C[2] = v.z, C[3] = v.w;
                    const int x0 = 16 * g;
                    if (x0 >= hoff && x0 + 16 <= send) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) h.word(C[t]);
                    } else {
                        // a partial chunk: hash its valid bytes, zero the bytes past the source
#pragma unroll 1
                        for (int b = 0; b < 16; ++b) {
                            const int x = x0 + b;
                            if (x >= hoff && x < send) h.byte((C[b >> 2] >> (8 * (b & 3))) & 0xFFu);
                        }
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int keep = min(max(send - (x0 + 4 * t), 0), 4);
                            C[t] = keep >= 4 ? C[t] : keep <= 0 ? 0u : (C[t] & ((1u << (8 * keep)) - 1u));
                        }
                    }
                }
                const bool full = g >= jf && g <= jl;
                const bool hl = hpart && g == jf - 1, tl = tpart && g == jl + 1;
                if (full || hl || tl) {
                    const u32x4 o = line_of(P, C, mi, ri);
                    if (hl) Hd[0] = o.x, Hd[1] = o.y, Hd[2] = o.z, Hd[3] = o.w;
                    if (tl) Tl[0] = o.x, Tl[1] = o.y, Tl[2] = o.z, Tl[3] = o.w;
                    if (full) asm volatile("ds_write_b128 %0, %1" ::"v"(a), "v"(o) : "memory");
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) P[t] = C[t];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // 3. coalesced stores of the full lines: instruction j, packets 8j .. 8j + 7
#pragma unroll
        for (int h4 = 0; h4 < 8; h4 += 4) {   // four instructions at a time: exchanges and
            int qf[4], ql[4];                  // LDS reads issued together, one wait each
            uint64_t qa[4];
            u32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = 8 * (h4 + u) + lq;
                qf[u] = (int)bperm((uint32_t)jf, q);
                ql[u] = (int)bperm((uint32_t)jl, q);
                qa[u] = bperm64(A0, q);
                const uint32_t a = tb + (uint32_t)(q * 128 + ((pos ^ (q & 7)) << 4));
                asm volatile("ds_read_b128 %0, %1" : "=v"(v[u]) : "v"(a) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = 8 * w + pos;
                if (g >= qf[u] && g <= ql[u])
                    *(__attribute__((address_space(1))) u32x4*)(uintptr_t)(qa[u] + 16u * (uint64_t)g) = v[u];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // 4. the partial lines at both ends, from registers
    if (hpart) {
        uint8_t* L = (uint8_t*)(uintptr_t)(A0 + 16u * (uint64_t)(jf - 1));
        part_line(L, Hd, (int)(dst - L), min(16, (int)(dst + olen - L)));
    }
    if (tpart && !(hpart && jl + 1 == jf - 1)) {
        uint8_t* L = (uint8_t*)(uintptr_t)(A0 + 16u * (uint64_t)(jl + 1));
        part_line(L, Tl, max(0, (int)(dst - L)), (int)(dst + olen - L));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// the 12 tag bytes at c against (t0, t1, t2)
__device__ __forceinline__ bool tag_matches(const uint8_t* c, uint32_t t0, uint32_t t1,
                                            uint32_t t2) {
    uint32_t w[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        w[q] = c[4 * q] | (c[4 * q + 1] << 8) | (c[4 * q + 2] << 16) |
               ((uint32_t)c[4 * q + 3] << 24);
    return w[0] == t0 && w[1] == t1 && w[2] == t2;
}

// Plaintext rows: packet p reads b + p * stride (ka == 0), or, grouped, packet
// p = g * (ka + kb) + i reads row (g, i) of a ([G][ka]) for i < ka and row (g, i - ka) of
// b ([G][kb]) otherwise.
struct PtRows {
    const uint8_t* a;
    const uint8_t* b;
    long long stride;
    int ka, kb;
};

__device__ __forceinline__ const uint8_t* pt_row(const PtRows& r, long long p) {
    if (r.ka == 0) return r.b + p * r.stride;
    const int per = r.ka + r.kb;
    const long long g = p / per;
    const int i = (int)(p - g * per);
    return i < r.ka ? r.a + (g * r.ka + i) * r.stride : r.b + (g * r.kb + (i - r.ka)) * r.stride;
}
__device__ __forceinline__ int pt_len_of(const PtRows&, const int32_t* pt_len, int pt_all,
                                         long long p) {
    return len_of(pt_len, pt_all, p);
}
__device__ __forceinline__ bool pt_fits(const PtRows& r, long long, int pl) {
    return r.stride == 0 || pl <= r.stride;
}

// Plaintext rows of a ragged batch: packet p = g * (ka + kb) + i reads block i of group g's
// [ka][bb[g]] at a + a_off[g] for i < ka, block i - ka of its [kb][bb[g]] at b + b_off[g]
// otherwise.  The 64 packets of a wave come from several groups, so g, bb[g] and the offsets
// are per lane.  pt_len == nullptr: every plaintext is its whole block.  A group with
// bb[g] < 1 has no rows, and neither has, when the seal follows the encode (enc), a group
// the encode rejected: none of their packets fits.
struct RaggedRows {
    const uint8_t* a;
    const uint8_t* b;
    const long long* a_off;
    const long long* b_off;
    const int32_t* bb;
    int ka, kb;
    bool enc;
};

__device__ __forceinline__ const uint8_t* pt_row(const RaggedRows& r, long long p) {
    const int per = r.ka + r.kb;
    const long long g = p / per;
    const int i = (int)(p - g * per);
    const long long bb = r.bb[g];
    return i < r.ka ? r.a + r.a_off[g] + i * bb : r.b + r.b_off[g] + (i - r.ka) * bb;
}
__device__ __forceinline__ int pt_len_of(const RaggedRows& r, const int32_t* pt_len, int,
                                         long long p) {
    return pt_len ? pt_len[p] : r.bb[p / (r.ka + r.kb)];
}
__device__ __forceinline__ bool pt_fits(const RaggedRows& r, long long p, int pl) {
    const int bb = r.bb[p / (r.ka + r.kb)];
    return bb >= 1 && pl <= bb && !(r.enc && ragged_encode_rejects(r.ka, r.kb, bb));
}

// Only the framed seal writes a group status.
__device__ __forceinline__ void pt_status(const PtRows&, long long) {}
__device__ __forceinline__ void pt_status(const RaggedRows&, long long) {}

// Rows of the framed sender: packet p = g * (ka + kb) + i reads payload row g * ka + i (pay.len
// bytes of it: the wire packet carries no prefix) for i < ka, parity block i - ka of group g
// (bb[g] bytes) otherwise.  No packet of a group the frame kernel rejected
// (framed_group_rejects) or the encode rejected (ragged_encode_rejects) fits; the first lane of
// a group the frame rejected writes its status, after the encode wrote one for every group.
struct FramedRows {
    Rows pay;
    const uint8_t* par;
    const long long* par_off;
    const int32_t* bb;
    int32_t* status;
    int ka, kb;
};

__device__ __forceinline__ const uint8_t* pt_row(const FramedRows& r, long long p) {
    const int per = r.ka + r.kb;
    const long long g = p / per;
    const int i = (int)(p - g * per);
    return i < r.ka ? r.pay.p + (g * r.ka + i) * r.pay.stride
                    : r.par + r.par_off[g] + (i - r.ka) * (long long)r.bb[g];
}
__device__ __forceinline__ int pt_len_of(const FramedRows& r, const int32_t*, int, long long p) {
    const int per = r.ka + r.kb;
    const long long g = p / per;
    const int i = (int)(p - g * per);
    return i < r.ka ? r.pay.len[g * r.ka + i] : r.bb[g];
}
__device__ __forceinline__ bool framed_rejects(const FramedRows& r, long long g) {
    return framed_group_rejects(r.pay.len + g * r.ka, r.ka, r.pay.stride, r.bb[g]);
}
__device__ __forceinline__ bool pt_fits(const FramedRows& r, long long p, int) {
    const long long g = p / (r.ka + r.kb);
    return !framed_rejects(r, g) && !ragged_encode_rejects(r.ka, r.kb, r.bb[g]);
}
__device__ __forceinline__ void pt_status(const FramedRows& r, long long p) {
    const int per = r.ka + r.kb;
    const long long g = p / per;
    if (r.status && p == g * per && framed_rejects(r, g)) r.status[g] = -3;
}

// Where a packet lies among the rows: the three lookups above find the group of packet p by a
// division, so their place is p itself.
__device__ __forceinline__ long long pt_where(const PtRows&, long long p) { return p; }
__device__ __forceinline__ long long pt_where(const RaggedRows&, long long p) { return p; }
__device__ __forceinline__ long long pt_where(const FramedRows&, long long p) { return p; }

// ------------------------------------------------------------------ mixed geometry
// With a code per group (a code set, gf_mixed.h) packet p no longer belongs to group
// p / (k + m): the groups' spans are a prefix table first [G + 1], and a group's k and m are
// the MixedCode record of its code.  The plan kernel below decides once which groups a call
// runs (ecode[g] = code[g], or 255 for a rejected group) and with which size (eff[g]); every
// other kernel reads those two arrays, so no two of them can disagree about a group.
// The geometry a per-arrival or per-group kernel asks.  find(g, &l) says whether the call runs
// group g and fills the lane's record l; k(l), m(l) and first(l, g), the group's first packet /
// slot, read it; find_wave is find for a group that is the same in every lane of the wave;
// rows(g) is the group's row of the rows array.  Uniform: constants, and an empty record.
struct UniGeo {
    int kk, mm, pp;   // pp = k + m
    // what a kernel takes in its arguments to build the geometry from (two scalars here, so
    // that the uniform kernels keep the argument block they had)
    typedef int A0;
    typedef int A1;
    __device__ __forceinline__ UniGeo(int k, int m) : kk(k), mm(m), pp(k + m) {}
    struct Lane {};
    __device__ __forceinline__ bool find(long long, Lane*) const { return true; }
    __device__ __forceinline__ bool find_wave(long long, Lane*) const { return true; }
    __device__ __forceinline__ int k(const Lane&) const { return kk; }
    __device__ __forceinline__ int m(const Lane&) const { return mm; }
    __device__ __forceinline__ int per(const Lane&) const { return pp; }
    __device__ __forceinline__ long long first(const Lane&, long long g) const { return g * pp; }
    __device__ __forceinline__ long long rows(long long g) const { return g * kk; }
};
// Mixed: the MixedCode record of ecode[g] (255: no group of this call) and first[g].  The loads
// are per lane; the table of records is at most 1 KiB and stays in cache.
struct MixedTabs {
    const MixedCode* codes;
    const uint8_t* ecode;
    const int32_t* pkt_first;
};
struct MixedGeo {
    const MixedCode* codes;
    const uint8_t* ecode;
    const int32_t* pkt_first;
    int kmax;
    typedef MixedTabs A0;
    typedef int A1;
    __host__ __device__ __forceinline__ MixedGeo(const MixedTabs& t, int kmax_)
        : codes(t.codes), ecode(t.ecode), pkt_first(t.pkt_first), kmax(kmax_) {}
    struct Lane {
        int k, m;
        long long first;
    };
    __device__ __forceinline__ bool find(long long g, Lane* l) const {
        const uint32_t ci = ecode[g];
        if (ci == 255) return false;
        *l = {codes[ci].k, codes[ci].m, (long long)pkt_first[g]};
        return true;
    }
    __device__ __forceinline__ bool find_wave(long long g, Lane* l) const {
        const uint32_t ci = (uint32_t)__builtin_amdgcn_readfirstlane((int)ecode[g]);
        if (ci == 255) return false;
        *l = {__builtin_amdgcn_readfirstlane(codes[ci].k),
              __builtin_amdgcn_readfirstlane(codes[ci].m),
              (long long)__builtin_amdgcn_readfirstlane(pkt_first[g])};
        return true;
    }
    __device__ __forceinline__ int k(const Lane& l) const { return l.k; }
    __device__ __forceinline__ int m(const Lane& l) const { return l.m; }
    __device__ __forceinline__ int per(const Lane& l) const { return l.k + l.m; }
    __device__ __forceinline__ long long first(const Lane& l, long long) const { return l.first; }
    __device__ __forceinline__ long long rows(long long g) const { return g * kmax; }
};

// One lane per group: the verdict on group g (pp_mixed.h, launch_mixed_wire_plan).
__global__ __launch_bounds__(kPPThreads) void mixed_wire_plan_kernel(
    long long groups, const MixedCode* __restrict__ codes, int ncodes,
    const uint8_t* __restrict__ code, const int32_t* __restrict__ bbs,
    const int32_t* __restrict__ pkt_first, long long npkt, const int32_t* __restrict__ pay_first,
    long long npay, const int32_t* __restrict__ pay_len, long long pay_stride, int32_t* eff,
    uint8_t* ecode) {
    const long long g = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (g >= groups) return;
    const uint32_t ci = code[g];
    bool ok = ci < (uint32_t)ncodes;
    int k = 0, bb = 0;
    long long p0 = 0;
    if (ok) {
        k = codes[ci].k;
        const long long per = (long long)k + codes[ci].m;
        const long long f0 = pkt_first[g], f1 = pkt_first[g + 1];
        ok = f0 >= 0 && f1 - f0 == per && f0 + per <= npkt;
        if (pay_first) {
            p0 = pay_first[g];
            ok = ok && p0 >= 0 && (long long)pay_first[g + 1] - p0 == k && p0 + k <= npay;
        }
    }
    if (ok) {
        bb = bbs[g];
        if (pay_first && framed_group_rejects(pay_len + p0, k, pay_stride, bb)) bb = 0;
    }
    ecode[g] = ok ? (uint8_t)ci : (uint8_t)255;
    eff[g] = bb;
}

// The group whose span of `first` holds x, for the lanes of one wave whose x are x0 .. x0 + 63
// (x0 from the workgroup index, so that the compiler sees it and the two bounds as uniform):
// the last g in [0, G) with first[g] <= x (empty spans in front of it are passed over).  Two
// searches with wave-uniform indices for x0 and x0 + 63, then each lane's own search between
// the two answers.  Every loop's trip count depends on G and the two uniform answers alone, so
// the lanes never leave a loop apart; every index read lies in [0, G).  A table that is not
// ascending gives some group of the batch; the caller checks x against that group's span.
__device__ __forceinline__ long long mixed_group_of(const int32_t* first, long long G,
                                                    long long x, long long x0) {
    long long b0 = 0, b1 = 0;
    for (long long len = G; len > 1;) {
        const long long half = len >> 1;
        const long long v0 = __builtin_amdgcn_readfirstlane(first[b0 + half]);
        const long long v1 = __builtin_amdgcn_readfirstlane(first[b1 + half]);
        b0 = v0 <= x0 ? b0 + half : b0;
        b1 = v1 <= x0 + 63 ? b1 + half : b1;
        len -= half;
    }
    long long b = b0;
    for (long long len = b1 - b0 + 1; len > 1;) {   // b1 < b0 (a hostile table): no step
        const long long half = len >> 1;
        b = (long long)first[b + half] <= x ? b + half : b;
        len -= half;
    }
    return b;
}

// Rows of the mixed framed sender: FramedRows with the packet's place found by the tables.
struct MixedRows {
    Rows pay;
    const uint8_t* par;
    const long long* par_off;
    const int32_t* eff;
    const uint8_t* ecode;
    const MixedCode* codes;
    const int32_t* pkt_first;
    const int32_t* pay_first;
    long long groups, npkt;
    int32_t* status;
};
// g < 0: the packet lies in no group the call runs
struct MixedAt {
    long long g, pay;   // pay: the payload row of a data packet
    int i, k, m, bb;
};
__device__ __forceinline__ MixedAt pt_where(const MixedRows& r, long long p) {
    MixedAt w{-1, 0, 0, 0, 0, 0};
    if (r.groups <= 0) return w;   // uniform
    const long long g = mixed_group_of(r.pkt_first, r.groups, p, (long long)blockIdx.x * 64);
    const uint32_t ci = r.ecode[g];
    if (ci == 255 || p >= r.npkt) return w;
    const int k = r.codes[ci].k, m = r.codes[ci].m;
    const long long d = p - r.pkt_first[g];
    if (d < 0 || d >= k + m) return w;
    return {g, d < k ? r.pay_first[g] + d : 0, (int)d, k, m, r.eff[g]};
}
__device__ __forceinline__ const uint8_t* pt_row(const MixedRows& r, const MixedAt& w) {
    return w.i < w.k ? r.pay.p + w.pay * r.pay.stride
                     : r.par + r.par_off[w.g] + (w.i - w.k) * (long long)w.bb;
}
__device__ __forceinline__ int pt_len_of(const MixedRows& r, const int32_t*, int,
                                         const MixedAt& w) {
    return w.g < 0 ? -1 : w.i < w.k ? r.pay.len[w.pay] : w.bb;
}
__device__ __forceinline__ bool pt_fits(const MixedRows&, const MixedAt& w, int) {
    return w.g >= 0 && w.bb > 0 && !ragged_encode_rejects(w.k, w.m, w.bb);
}
// eff 0 in a group the plan kept: the frame's rejection
__device__ __forceinline__ void pt_status(const MixedRows& r, const MixedAt& w) {
    if (r.status && w.g >= 0 && w.i == 0 && w.bb == 0) r.status[w.g] = -3;
}

// One wave seals 64 packets (one per lane): the AD through the lane's own streamer (a few
// bytes), the plaintext through the wave's LDS tile (tile_stream), then the tag.  R: where the
// plaintext rows are (PtRows, RaggedRows, FramedRows, MixedRows).
template <class H, class R>
__global__ __launch_bounds__(64) void null_seal_kernel(
    long long n, const uint8_t* __restrict__ ad, long long ad_stride,
    const int32_t* __restrict__ ad_len, int ad_all, R pr, const int32_t* __restrict__ pt_len,
    int pt_all, uint8_t* out, long long out_stride, int32_t* out_len) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    const auto at = pt_where(pr, i);   // asked by every lane of the wave (MixedRows searches)
    bool ok = false;
    int al = 0, pl = 0;
    if (i < n) {
        al = len_of(ad_len, ad_all, i);
        pl = pt_len_of(pr, pt_len, pt_all, at);
        // a row longer than its stride would read the next packet's bytes (or past the buffer
        // for the last one): rejected like a packet that does not fit
        ok = al >= 0 && pl >= 0 && (ad_stride == 0 || al <= ad_stride) &&
             pt_fits(pr, at, pl) && (long long)al + 12 + pl <= out_stride;
        out_len[i] = ok ? al + 12 + pl : -1;
        pt_status(pr, at);
    }
    uint8_t* o = out + (ok ? i : 0) * out_stride;
    H h;
    h.init();
    Sink s, t;
    s.begin(o);
    if (ok) span<true, true, 1>(h, s, ad + i * ad_stride, al);   // a few bytes: 16-byte pieces
    t = s;   // AD's unstored tail bytes; the tag follows them once it is known
    tile_stream(h, ok ? pt_row(pr, at) : nullptr, ok ? pl : 0, o + al + 12, ok ? pl : 0, smem);
    if (!ok) return;
    uint32_t t0, t1, t2;
    h.tag(t0, t1, t2);
    t.word(t0);
    t.word(t1);
    t.word(t2);
    t.flush();
}

template <class H>
__global__ __launch_bounds__(kPPThreads) void null_open_kernel(
    long long n, const uint8_t* __restrict__ pkt, long long pkt_stride,
    const int32_t* __restrict__ pkt_len, int pkt_all, const int32_t* __restrict__ ad_len,
    int ad_all, uint8_t* out, long long out_stride, int32_t* out_len) {
    const long long i = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = pkt + i * pkt_stride;
    const int al = len_of(ad_len, ad_all, i);
    const int tl = len_of(pkt_len, pkt_all, i);
    const int cl = tl - al;   // ciphertext bytes
    // the output receives the ciphertext (reference: before any check)
    const bool copy = al >= 0 && cl >= 0 && cl <= out_stride && (pkt_stride == 0 || tl <= pkt_stride);
    if (!copy) {
        out_len[i] = -1;
        return;
    }
    uint8_t* o = out + i * out_stride;
    const uint8_t* c = p + al;
    int res = -1;
    if (cl >= 12) {
        H h;
        h.init();
        Sink s;
        s.begin(o);
        span<true, false>(h, s, p, al);
        span<true, true>(h, s, c + 12, cl - 12);
        uint32_t t0, t1, t2;
        h.tag(t0, t1, t2);
        if (tag_matches(c, t0, t1, t2)) {
            // accepted: the plaintext, then the last 12 bytes of the ciphertext copy the
            // reference made first (its output buffer holds them past the plaintext)
            for (int q = 0; q < 12; ++q) s.byte(c[cl - 12 + q]);
            s.flush();
            res = cl - 12;
        }
    }
    if (res < 0) {
        // rejected: the ciphertext copy alone, over the plaintext stores of this lane
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        H h;
        Sink s;
        s.begin(o);
        span<false, true>(h, s, c, cl);
        s.flush();
    }
    out_len[i] = res;
}

// The open's length checks alone (the tag is checked later): a packet that fails them is
// rejected whatever its bytes.
// lim: the longest plaintext the packet's slot takes (the slots' limit()).
__device__ __forceinline__ bool open_len_ok(const int32_t* __restrict__ pkt_len,
                                            const int32_t* __restrict__ ad_len, int ad_all,
                                            long long p, int lim, long long pkt_stride) {
    const int tl = pkt_len[p];
    const int al = len_of(ad_len, ad_all, p);
    const int cl = tl - al;
    return tl >= 0 && al >= 0 && cl >= 12 && cl - 12 <= lim && tl <= pkt_stride;
}

// The slot FEC packet i (>= k) of group g is written to by the open, before any tag is known:
// the holes and the available FEC packets as the length checks alone leave them, matched in
// ascending order as open_assemble_kernel matches them (the j-th available FEC packet fills
// the j-th hole); -1 when it fills none.  Where a tag check then changes the match,
// open_assemble_kernel copies the right packet over.
// dlim, flim: the plaintext limits of the group's data and FEC packets.
__device__ int fec_pre_slot(const int32_t* __restrict__ pkt_len,
                            const int32_t* __restrict__ ad_len, int ad_all, long long g, int i,
                            int k, int m, int dlim, int flim, long long pkt_stride) {
    const long long p0 = g * (k + m);
    int j = 0;
#pragma unroll 4
    for (int q = k; q < i; ++q) j += open_len_ok(pkt_len, ad_len, ad_all, p0 + q, flim, pkt_stride) ? 1 : 0;
#pragma unroll 8
    for (int x = 0; x < k; ++x) {
        if (open_len_ok(pkt_len, ad_len, ad_all, p0 + x, dlim, pkt_stride)) continue;
        if (j == 0) return x;
        --j;
    }
    return -1;
}

// Where the receiver's block slots are and how long they are.  Uniform: blocks [G][k][bb].
struct UniSlots {
    int bb;
    __device__ __forceinline__ int size(long long) const { return bb; }
    __device__ __forceinline__ uint8_t* slot(uint8_t* blocks, long long g, int k, int s,
                                             int bb_) const {
        return blocks + (g * k + s) * (long long)bb_;
    }
    // the longest plaintext a slot of size bb_ takes from a data (or FEC) packet, where in
    // the slot it starts, and the framing written in front of it: none
    __device__ __forceinline__ int limit(int bb_, bool) const { return bb_; }
    __device__ __forceinline__ int lead(bool) const { return 0; }
    __device__ __forceinline__ void prefix(uint8_t*, long long, int, int, int, int,
                                           long long) const {}
};
// Ragged: group g's [k][bb[g]] at blocks + off[g].  A wave's 64 packets come from several
// groups, so the size and the offset are per lane.  A group with bb[g] < 1 (and the lanes
// past the last group) get size -1: no packet passes the length checks then (open_len_ok), so
// none of it is written and every row of it is tagged 255.
struct RaggedSlots {
    const int32_t* bb;
    const long long* off;
    long long groups;
    __device__ __forceinline__ int size(long long g) const {
        const int b = g < groups ? bb[g] : -1;
        return b < 1 ? -1 : b;
    }
    __device__ __forceinline__ uint8_t* slot(uint8_t* blocks, long long g, int, int s,
                                             int bb_) const {
        return blocks + off[g] + s * (long long)bb_;
    }
    // the longest plaintext a slot of size bb_ takes from a data (or FEC) packet, where in
    // the slot it starts, and the framing written in front of it: none
    __device__ __forceinline__ int limit(int bb_, bool) const { return bb_; }
    __device__ __forceinline__ int lead(bool) const { return 0; }
    __device__ __forceinline__ void prefix(uint8_t*, long long, int, int, int, int,
                                           long long) const {}
    __device__ __forceinline__ int pad(int bb_) const { return bb_; }
    static constexpr bool kFecPre = false;
};
// the two-byte prefix of a framed data packet's block (little-endian): payload length, pn_len
__device__ __forceinline__ uint32_t frame_prefix(int len, int pn) {
    return (uint32_t)len | ((uint32_t)pn << 14);
}
// Framed (QuicFecGroup's stored packets, quic_fec_group.cc:178-183) over the slots W: a data
// packet's plaintext is a payload: it goes two bytes into its slot, behind the prefix
// len | pn_len << 14 (16 bits, little-endian) that the lane writes itself, so it may be at most
// bb[g] - 2 bytes long.  An FEC packet's plaintext is a whole block, as in RaggedSlots.
// The arrival-order kernels ask two things more of W.  pad(bb_): the length a slot the open pass
// writes is zero-padded to.  kFecPre: whether that pass writes FEC slots before the tags are
// known, too (only where every packet has a slot of its own).
template <class W>
struct Framed {
    W w;
    const uint8_t* pn_len;   // per packet ([G * (k + m)]) or per arrival; null: pn_all
    int pn_all;
    static constexpr bool kFecPre = W::kFecPre;
    __device__ __forceinline__ int size(long long g) const { return w.size(g); }
    __device__ __forceinline__ uint8_t* slot(uint8_t* blocks, long long g, int k, int s,
                                             int bb_) const {
        return w.slot(blocks, g, k, s, bb_);
    }
    __device__ __forceinline__ int pad(int bb_) const { return w.pad(bb_); }
    __device__ __forceinline__ int limit(int bb_, bool data) const {
        return data ? bb_ - 2 : bb_;
    }
    __device__ __forceinline__ int lead(bool data) const { return data ? 2 : 0; }
    // the prefix of a data packet (packet or arrival p) that opened len bytes
    __device__ __forceinline__ uint32_t prefix_of(int len, long long p) const {
        return frame_prefix(len, pn_len ? pn_len[p] : pn_all);
    }
    // data packet i of group g opened len bytes: the prefix in front of them
    __device__ __forceinline__ void prefix(uint8_t* blocks, long long g, int k, int i, int bb_,
                                           int len, long long p) const {
        uint8_t* s = slot(blocks, g, k, i, bb_);
        const uint32_t v = prefix_of(len, p);
        gst8(s, v);
        gst8(s + 1, v >> 8);
    }
};
typedef Framed<RaggedSlots> FramedSlots;
// The receiver window's hold rows: slot s of group g is the row of
// hold_stride bytes at hold + (g * per + s) * hold_stride, whatever this push's bb[g], and it is
// written to its whole length.  A bb[g] below 1 or above hold_stride gives size -1: no packet
// passes the length checks then.  g is a group of the window.
struct HoldRows {
    const int32_t* bb;
    long long hold_stride, groups;
    int per;   // k + m
    static constexpr bool kFecPre = true;
    __device__ __forceinline__ int size(long long g) const {
        const int b = bb[g];
        return b < 1 || b > hold_stride ? -1 : b;
    }
    __device__ __forceinline__ uint8_t* slot(uint8_t* hold, long long g, int, int s, int) const {
        return hold + (g * per + s) * hold_stride;
    }
    __device__ __forceinline__ int pad(int) const { return (int)hold_stride; }
};
typedef Framed<HoldRows> WinSlots;

// Receiver, grouped: packet p = g * (k + m) + i, one wave per 64 packets; a data packet's
// plaintext goes to its block slot, zero-padded to bb, through the wave's LDS tile, and so
// does an FEC packet's, into the hole it fills if the tags change nothing (fec_pre_slot).
// S: the slots (UniSlots, RaggedSlots, FramedSlots).
template <class H, class S>
__global__ __launch_bounds__(64) void open_group_kernel(
    int k, int m, S sl, long long n, const uint8_t* __restrict__ pkt, long long pkt_stride,
    const int32_t* __restrict__ pkt_len, const int32_t* __restrict__ ad_len, int ad_all,
    uint8_t* blocks, int32_t* open_len) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long p = (long long)blockIdx.x * 64 + threadIdx.x;
    const int per = k + m;
    const long long g = p / per;
    const int i = (int)(p - g * per);
    const int bb = sl.size(g);
    const int lim = sl.limit(bb, i < k);   // the longest plaintext this packet's slot takes
    bool ok = false;
    int al = 0, cl = 0;
    if (p < n) {
        const int tl = pkt_len[p];
        al = len_of(ad_len, ad_all, p);
        cl = tl - al;
        ok = tl >= 0 && al >= 0 && cl >= 12 && cl - 12 <= lim && tl <= pkt_stride;
        if (!ok) open_len[p] = -1;
    }
    const uint8_t* pp = pkt + (ok ? p : 0) * pkt_stride;
    const uint8_t* c = pp + al;
    H h;
    h.init();
    Sink s;
    if (ok) span<true, false, 1>(h, s, pp, al);
    const int slot = !ok ? -1 : i < k ? i
                   : fec_pre_slot(pkt_len, ad_len, ad_all, g, i, k, m, sl.limit(bb, true),
                                  sl.limit(bb, false), pkt_stride);
    const int lead = sl.lead(i < k);
    tile_stream(h, ok ? c + 12 : nullptr, ok ? cl - 12 : 0,
                slot >= 0 ? sl.slot(blocks, g, k, slot, bb) + lead : nullptr,
                slot >= 0 ? bb - lead : 0, smem);
    if (!ok) return;
    if (i < k) sl.prefix(blocks, g, k, i, bb, cl - 12, p);
    uint32_t t0, t1, t2;
    h.tag(t0, t1, t2);
    open_len[p] = tag_matches(c, t0, t1, t2) ? cl - 12 : -1;
}

// Block slot dst[0 .. bb) = lead || src[0 .. pl) || zeros, by the whole wave: lead is the two
// prefix bytes `pre` of a data packet's slot (nlead 2) or nothing (nlead 0).  Dword stores where
// the slot and bb allow them; the dwords read then hold at least one byte of lead || src, and
// the bytes in front of src are the packet's own (its tag).
__device__ void wave_place(uint8_t* dst, const uint8_t* src, int pl, int bb, int nlead,
                           uint32_t pre, int lane) {
    const int end = nlead + pl;   // bytes of the slot that are not padding
    if ((((uintptr_t)dst) | (uint32_t)bb) & 3u) {
        for (int o = lane; o < bb; o += 64)
            dst[o] = o < nlead ? (uint8_t)(pre >> (8 * o)) : o < end ? src[o - nlead] : 0;
        return;
    }
    const uint8_t* v0 = src - nlead;   // the slot's byte o is v0[o] for nlead <= o < end
    const uint32_t sh = (uint32_t)(uintptr_t)v0 & 3u;
    const uint32_t* s4 = (const uint32_t*)(v0 - sh);
    for (int u = lane; u < (bb >> 2); u += 64) {
        const int o = 4 * u;
        uint32_t v = 0;
        if (o < end) {
            const uint32_t w0 = s4[u];
            const uint32_t w1 = (sh && o + 4 - (int)sh < end) ? s4[u + 1] : 0u;
            v = sh ? __builtin_amdgcn_alignbyte(w1, w0, sh) : w0;
            if (end - o < 4) v &= (1u << (8 * (end - o))) - 1u;
            if (u == 0 && nlead) v = (v & 0xffff0000u) | (pre & 0xffffu);
        }
        ((uint32_t*)dst)[u] = v;
    }
}

constexpr int kAsmWaves = 4;

// The rows of one group, by its wave (the rule of every receiver here): rows[i] = i where slot i
// is present; the holes, ascending, take the present FEC packets, ascending (row k + j); 255
// where none is left.  present(s): whether slot s of the group holds a packet.  lavail, lhole:
// this wave's LDS rows; afterwards FEC packet lavail[h] fills hole lhole[h] for h below the
// count returned (lhole null: not wanted; the caller waits for its LDS writes).  each(i, row):
// called by the lane that wrote rows[i].
template <class P, class E>
__device__ __forceinline__ int wave_rows(int k, int m, int lane, P present, uint8_t* lavail,
                                         uint8_t* lhole, uint8_t* rows, E each) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int na = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int j = b0 + lane;
        const bool v = j < m && present(k + j);
        const unsigned long long bal = __ballot(v);
        if (v) lavail[na + __popcll(bal & below)] = (uint8_t)j;
        na += __popcll(bal);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes are visible
    __builtin_amdgcn_wave_barrier();
    int nh = 0;
    for (int b0 = 0; b0 < k; b0 += 64) {
        const int i = b0 + lane;
        const bool miss = i < k && !present(i);
        const unsigned long long bal = __ballot(miss);
        const int r = nh + __popcll(bal & below);
        if (i < k) {
            int row = i;
            if (miss) {
                row = r < na ? k + lavail[r] : 255;
                if (lhole && r < na) lhole[r] = (uint8_t)i;
            }
            rows[i] = (uint8_t)row;
            each(i, row);
        }
        nh += __popcll(bal);
    }
    return min(nh, na);
}

// One wave per group: the group's rows (wave_rows) over the packets that opened; with a row 255
// the decode reports the group as malformed, status -3.  The open has already written each FEC
// packet into the hole the length checks alone give it (fec_pre_slot); a pair the tag checks
// changed is copied here.
template <class S>
__global__ __launch_bounds__(kAsmWaves * 64) void open_assemble_kernel(
    int k, int m, S sl, long long groups, const uint8_t* __restrict__ pkt, long long pkt_stride,
    const int32_t* __restrict__ pkt_len, const int32_t* __restrict__ ad_len, int ad_all,
    const int32_t* __restrict__ open_len, uint8_t* blocks, uint8_t* rows) {
    __shared__ uint8_t lavail[kAsmWaves][256], lhole[kAsmWaves][256];
    __shared__ uint8_t prank[kAsmWaves][256], phole[kAsmWaves][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * kAsmWaves + w;
    if (g >= groups) return;   // uniform over the wave; no workgroup barrier below
    const int bb = sl.size(g);
    const int per = k + m;
    const int32_t* ol = open_len + g * per;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int nfill = wave_rows(k, m, lane, [&](int s) { return ol[s] >= 0; }, lavail[w],
                                lhole[w], rows + g * k, [](int, int) {});
    // the match the open wrote by (fec_pre_slot): ranks of the FEC packets and the holes by
    // the length checks alone
    int npa = 0, nph = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int j = b0 + lane;
        const bool v = j < m && open_len_ok(pkt_len, ad_len, ad_all, g * per + k + j,
                                            sl.limit(bb, false), pkt_stride);
        const unsigned long long bal = __ballot(v);
        if (j < m) prank[w][j] = v ? (uint8_t)(npa + __popcll(bal & below)) : (uint8_t)255;
        npa += __popcll(bal);
    }
    for (int b0 = 0; b0 < k; b0 += 64) {
        const int i = b0 + lane;
        const bool miss = i < k && !open_len_ok(pkt_len, ad_len, ad_all, g * per + i,
                                                sl.limit(bb, true), pkt_stride);
        const unsigned long long bal = __ballot(miss);
        if (miss) phole[w][nph + __popcll(bal & below)] = (uint8_t)i;
        nph += __popcll(bal);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    for (int h = 0; h < nfill; ++h) {
        const int j = lavail[w][h], i = lhole[w][h];
        const int pr = prank[w][j];
        if (pr < nph && phole[w][pr] == i) continue;   // written there by the open
        const long long p = g * per + k + j;
        const uint8_t* src = pkt + p * pkt_stride + len_of(ad_len, ad_all, p) + 12;
        wave_place(sl.slot(blocks, g, k, i, bb), src, ol[k + j], bb, 0, 0u, lane);
    }
}

// After the decode: a group with an unfilled slot (row 255) is malformed whatever path
// decoded it (the m = 1 XOR decode takes any row >= k as its parity block): status -3 and no
// recovered rows.  K: the group's k and its rows (UniRowsK; MixedGeo, where a rejected group
// keeps the status -2 the decode gave it).
struct UniRowsK {
    int kk;
    struct Lane {};
    __device__ __forceinline__ bool find(long long, Lane*) const { return true; }
    __device__ __forceinline__ int k(const Lane&) const { return kk; }
    __device__ __forceinline__ long long rows(long long g) const { return g * kk; }
};

template <class K>
__global__ __launch_bounds__(kPPThreads) void open_status_kernel(long long groups, K ge,
                                                                 int rmax,
                                                                 const uint8_t* __restrict__ rows,
                                                                 uint8_t* rec_rows,
                                                                 int32_t* status) {
    const long long g = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (g >= groups) return;
    typename K::Lane gl{};
    if (!ge.find(g, &gl)) return;
    const int k = ge.k(gl);
    const uint8_t* r = rows + ge.rows(g);
    bool unfilled = false;
    for (int i = 0; i < k; ++i) unfilled |= r[i] == 255;
    if (!unfilled) return;
    if (status) status[g] = -3;
    for (int j = 0; j < rmax; ++j) rec_rows[g * rmax + j] = 255;
}

// tile_stream with nothing to hash: the two kernels below only move bytes.
struct NoHash {
    __device__ __forceinline__ void byte(uint32_t) {}
    __device__ __forceinline__ void word(uint32_t) {}
};

// Sender framing (appendLenToPayload, quic_fec_group.cc:109-121, and the padding of
// getRedundancyPackets, :344-352): one lane per data packet q = g * k + i, 64 per wave.  Block
// (g, i) at data + data_off[g] + i * bb[g] becomes prefix || payload || zeros: the payload
// through the wave's tile, two bytes in, the prefix from the lane.  Nothing of a group
// framed_group_rejects names is written.  The group's first lane writes eff[g] (null: not
// wanted) = bb[g], or 0 for a rejected group, the size the encode that follows runs with, and
// status[g] (null: not wanted) = 0 / -3.
__global__ __launch_bounds__(64) __attribute__((flatten)) void frame_blocks_kernel(
    int k, long long n, const uint8_t* __restrict__ pay, long long pay_stride,
    const int32_t* __restrict__ pay_len, const uint8_t* __restrict__ pn_len, int pn_all,
    uint8_t* data, const long long* __restrict__ data_off, const int32_t* __restrict__ bbs,
    int32_t* eff, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long g = q / k;
    const int i = (int)(q - g * k);
    bool ok = false;
    int len = 0, bb = 0;
    if (q < n) {
        bb = bbs[g];
        ok = !framed_group_rejects(pay_len + g * k, k, pay_stride, bb);
        if (i == 0) {
            if (eff) eff[g] = ok ? bb : 0;
            if (status) status[g] = ok ? 0 : -3;
        }
        if (ok) len = pay_len[q];
    }
    uint8_t* blk = ok ? data + data_off[g] + i * (long long)bb : nullptr;
    NoHash h;
    tile_stream(h, ok ? pay + q * pay_stride : nullptr, len, ok ? blk + 2 : nullptr,
                ok ? bb - 2 : 0, smem);
    if (!ok) return;
    const uint32_t v = (uint32_t)len | ((uint32_t)(pn_len ? pn_len[q] : pn_all) << 14);
    gst8(blk, v);
    gst8(blk + 1, v >> 8);
}

// The same over the mixed geometry: one lane per payload row q of [npay], its group found by
// the pay_first table (mixed_group_of), its place checked against the group's span.  The plan
// kernel has asked framed_group_rejects for every group already: eff[g] is bb[g], or 0 for a
// group that is not framed, so the lanes read the verdict where frame_blocks_kernel forms it.
__global__ __launch_bounds__(64) __attribute__((flatten)) void frame_blocks_mixed_kernel(
    long long groups, long long npay, const MixedCode* __restrict__ codes,
    const uint8_t* __restrict__ ecode, const int32_t* __restrict__ eff,
    const int32_t* __restrict__ pay_first, const uint8_t* __restrict__ pay, long long pay_stride,
    const int32_t* __restrict__ pay_len, const uint8_t* __restrict__ pn_len, int pn_all,
    uint8_t* data, const long long* __restrict__ data_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long g = mixed_group_of(pay_first, groups, q, (long long)blockIdx.x * 64);
    bool ok = false;
    int len = 0, bb = 0;
    long long i = 0;
    if (q < npay) {
        const uint32_t ci = ecode[g];
        if (ci != 255) {
            i = q - pay_first[g];
            bb = eff[g];
            ok = i >= 0 && i < codes[ci].k && bb > 0;
        }
        if (ok) len = pay_len[q];
    }
    uint8_t* blk = ok ? data + data_off[g] + i * (long long)bb : nullptr;
    NoHash h;
    tile_stream(h, ok ? pay + q * pay_stride : nullptr, len, ok ? blk + 2 : nullptr,
                ok ? bb - 2 : 0, smem);
    if (!ok) return;
    const uint32_t v = (uint32_t)len | ((uint32_t)(pn_len ? pn_len[q] : pn_all) << 14);
    gst8(blk, v);
    gst8(blk + 1, v >> 8);
}

// Receiver framing (getRevivedPackets, quic_fec_group.cc:287-292): one lane per recovered
// block q = g * rmax + j.  Where rec_rows[q] != 255 and the group's status is 0 (null: every
// group's), the block's prefix v gives len = min(v & 0x3fff, bb[g] - 2) (the reference reads
// past the block there; fec_group.cpp clamps the same way) and pn_len = v >> 14, and exactly
// len bytes go from block + 2 to rev row q.  Every other entry, and a len above rev_stride:
// rev_len -1 and nothing else written.
__global__ __launch_bounds__(64) __attribute__((flatten)) void extract_revived_kernel(
    int rmax, long long n, const uint8_t* __restrict__ rec, const long long* __restrict__ rec_off,
    const int32_t* __restrict__ bbs, const uint8_t* __restrict__ rec_rows,
    const int32_t* __restrict__ status, uint8_t* rev, long long rev_stride, int32_t* rev_len,
    uint8_t* rev_pn_len) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long g = q / rmax;
    const int j = (int)(q - g * rmax);
    bool take = false;
    int len = 0;
    const uint8_t* blk = nullptr;
    if (q < n) {
        const int bb = bbs[g];
        if (rec_rows[q] != 255 && (!status || status[g] == 0) && bb >= 2) {
            blk = rec + rec_off[g] + j * (long long)bb;
            const uint32_t v = blk[0] | ((uint32_t)blk[1] << 8);
            len = min((int)(v & 0x3fffu), bb - 2);
            take = len <= rev_stride;
            if (take && rev_pn_len) rev_pn_len[q] = (uint8_t)(v >> 14);
        }
        rev_len[q] = take ? len : -1;
    }
    if (!take) len = 0;
    NoHash h;
    tile_stream(h, take ? blk + 2 : nullptr, len, take ? rev + q * rev_stride : nullptr, len,
                smem);
}

// ------------------------------------------------------------------ arrival-order receiver
// The framed receiver over packets that lie in arrival order: arrival a
// carries the tag (arr_group[a], arr_index[a]) = (the group's index in the batch, packet number -
// fec_group).  The binding table arr_at [G * (k + m)] is the call's state: arrivals_init_kernel
// sets it to INT32_MAX, every arrival that opens takes the minimum of its slot with its own
// index (open_arrivals_kernel), and one wave per group keeps the k earliest of the group's
// candidates, -1 elsewhere (arrivals_assemble_kernel).  A minimum does not depend on the order
// the lanes run in, and a table is only read by the kernel after the one that writes it.
// The optimistic data write: a second table of the same shape, kept in the open_len output
// until the assemble overwrites it, takes the same minimum over the length checks alone
// (arrivals_pre_kernel), so that a data slot's first candidate is known before any byte is
// hashed.  That arrival streams its plaintext into the slot while it is hashed, as
// open_group_kernel does; the assemble places only what is not in place already, so an
// in-order ring is read once.
constexpr int kArrIgnored = -2, kArrRejected = -1, kArrDuplicate = -3, kArrLate = -4;
constexpr int32_t kArrNone = 0x7fffffff;

// pre_at: null without the optimistic write
__global__ __launch_bounds__(kPPThreads) void arrivals_init_kernel(long long slots,
                                                                   int32_t* arr_at,
                                                                   int32_t* pre_at) {
    const long long p = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (p >= slots) return;
    arr_at[p] = kArrNone;
    if (pre_at) pre_at[p] = kArrNone;
}

// One lane per arrival: an arrival with a tag of this batch that passes the length checks takes
// the minimum of pre_at[g * (k + m) + i] with its own index; a data arrival, or (S::kFecPre) any.
// Ge: the groups' geometry (UniGeo, MixedGeo); S: the framed slots (FramedSlots, WinSlots); here
// and in the kernels below.
template <class Ge, class S>
__global__ __launch_bounds__(kPPThreads) void arrivals_pre_kernel(
    typename Ge::A0 g0, typename Ge::A1 g1, S sl, long long n, long long pkt_stride,
    const int32_t* __restrict__ pkt_len, const int32_t* __restrict__ ad_len, int ad_all,
    const int32_t* __restrict__ arr_group, const uint8_t* __restrict__ arr_index,
    int32_t* pre_at) {
    const Ge ge(g0, g1);
    const long long a = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (a >= n) return;
    const long long g = arr_group[a];
    const int i = arr_index[a];
    typename Ge::Lane gl{};
    if (g < 0 || g >= sl.w.groups || !ge.find(g, &gl)) return;
    if (i >= (S::kFecPre ? ge.per(gl) : ge.k(gl))) return;
    if (open_len_ok(pkt_len, ad_len, ad_all, a, sl.limit(sl.size(g), i < ge.k(gl)), pkt_stride))
        atomicMin(pre_at + ge.first(gl, g) + i, (int32_t)a);
}

// One lane per arrival, 64 per wave: the length checks of the framed open against the tagged
// group's bb (open_len_ok with the framed limits), AD || plaintext hashed through the wave's
// tile, and where the tag matches atomicMin(arr_at[g * (k + m) + i], a).  arr_state (may be
// null) receives the plaintext length of an arrival that opened, kArrRejected or kArrIgnored;
// the two kernels below turn an opened arrival that is not kept into kArrLate / kArrDuplicate.
// pre_at (null: no optimistic write): the arrival that is its slot's first candidate by the
// length checks (arrivals_pre_kernel) streams into the slot before its tag is known, zeros up to
// the slot's pad() behind it, and a data packet's prefix in front; the assemble overwrites the
// slot where another packet is accepted for it.  blocks: what S::slot() takes, the blocks or the
// window's hold rows.
template <class H, class Ge, class S>
__global__ __launch_bounds__(64) void open_arrivals_kernel(
    typename Ge::A0 g0, typename Ge::A1 g1, S sl, long long n, const uint8_t* __restrict__ pkt,
    long long pkt_stride, const int32_t* __restrict__ pkt_len,
    const int32_t* __restrict__ ad_len, int ad_all, const int32_t* __restrict__ arr_group,
    const uint8_t* __restrict__ arr_index, int32_t* arr_state, int32_t* arr_at,
    const int32_t* __restrict__ pre_at, uint8_t* blocks) {
    const Ge ge(g0, g1);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const long long a = (long long)blockIdx.x * 64 + threadIdx.x;
    bool tagged = false, ok = false, place = false;
    long long g = 0;
    typename Ge::Lane gl{};
    int i = 0, al = 0, cl = 0, bb = -1;
    if (a < n) {
        g = arr_group[a];
        i = arr_index[a];
        tagged = g >= 0 && g < sl.w.groups && ge.find(g, &gl) && i < ge.per(gl);
        if (tagged) {
            bb = sl.size(g);
            al = len_of(ad_len, ad_all, a);
            cl = pkt_len[a] - al;
            ok = open_len_ok(pkt_len, ad_len, ad_all, a, sl.limit(bb, i < ge.k(gl)), pkt_stride);
            place = ok && (S::kFecPre || i < ge.k(gl)) && pre_at &&
                    pre_at[ge.first(gl, g) + i] == (int32_t)a;
        }
    }
    const int k = ge.k(gl);
    const int lead = sl.lead(!S::kFecPre || i < k);   // without kFecPre only data is placed
    const uint8_t* pp = pkt + (ok ? a : 0) * pkt_stride;
    const uint8_t* c = pp + al;
    H h;
    h.init();
    Sink s;
    if (ok) span<true, false, 1>(h, s, pp, al);
    tile_stream(h, ok ? c + 12 : nullptr, ok ? cl - 12 : 0,
                place ? sl.slot(blocks, g, k, i, bb) + lead : nullptr,
                place ? sl.pad(bb) - lead : 0, smem);
    if (a >= n) return;
    if (place && lead) sl.prefix(blocks, g, k, i, bb, cl - 12, a);
    bool opened = false;
    if (ok) {
        uint32_t t0, t1, t2;
        h.tag(t0, t1, t2);
        opened = tag_matches(c, t0, t1, t2);
    }
    if (opened) atomicMin(arr_at + ge.first(gl, g) + i, (int32_t)a);
    if (arr_state) arr_state[a] = !tagged ? kArrIgnored : opened ? cl - 12 : kArrRejected;
}

// The acceptance rule (QuicFecGroup takes no packet once it holds k, quic_fec_group.cc:210-213),
// by the group's wave: cand[s] is slot s's candidate of this call, an arrival index; kArrNone or
// a negative value where it has none.  Ranked by arrival index behind the held0 packets the group
// holds already, the candidates below k are accepted.  each(q, s, a, is, acc), called by every
// lane together for q = 0 .. while 64 q < per: slot s = lane + 64 q has the candidate a (is) and
// it is accepted (acc).  cand is not written.
template <class E>
__device__ __forceinline__ void wave_accept(const int32_t* cand, int per, int k, int held0,
                                            int lane, E each) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (64 * q >= per) break;   // uniform: no slot of the group is left
        const int s = lane + 64 * q;
        const int32_t a = s < per ? cand[s] : kArrNone;
        // compared as unsigned, a negative entry lies above kArrNone: it is no candidate, and it
        // is below no candidate
        const bool is = (uint32_t)a < (uint32_t)kArrNone;
        int rank = 0;   // every lane runs the whole loop
        for (int t = 0; t < per; ++t) rank += (uint32_t)cand[t] < (uint32_t)a ? 1 : 0;
        each(q, s, a, is, is && held0 + rank < k);
    }
}

// One wave per group, after the open pass: the group's candidates are the slots whose arr_at
// holds an arrival (the first copy of that index that opened).  The first k by arrival index are
// accepted (wave_accept); the others are late: arr_at -1 and, where arr_state is kept, kArrLate.
// Then what open_assemble_kernel writes for the accepted packets placed by slot: open_len, rows
// (wave_rows over the accepted packets), and every accepted packet's plaintext in its slot, a
// data packet's behind its prefix.  optimistic: on
// entry open_len holds arrivals_pre_kernel's table, and a data slot whose accepted arrival is
// the one named there was written by the open pass.
template <class Ge>
__global__ __launch_bounds__(kAsmWaves * 64) void arrivals_assemble_kernel(
    typename Ge::A0 g0, typename Ge::A1 g1, FramedSlots sl, const uint8_t* __restrict__ pkt,
    long long pkt_stride, const int32_t* __restrict__ pkt_len,
    const int32_t* __restrict__ ad_len, int ad_all, int32_t* arr_state, int32_t* arr_at,
    int32_t* open_len, bool optimistic, uint8_t* blocks, uint8_t* rows) {
    const Ge ge(g0, g1);
    __shared__ int32_t cand[kAsmWaves][256];   // the slot's candidate, then its accepted arrival
    __shared__ uint8_t lavail[kAsmWaves][256], lhole[kAsmWaves][256];
    __shared__ uint8_t inplace[kAsmWaves][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * kAsmWaves + w;
    if (g >= sl.w.groups) return;   // uniform over the wave; no workgroup barrier below
    typename Ge::Lane gl{};
    if (!ge.find_wave(g, &gl)) return;   // the same: one group per wave
    const int k = ge.k(gl), m = ge.m(gl);
    const int bb = sl.size(g);
    const int per = ge.per(gl);
    const long long first = ge.first(gl, g);
    int32_t* at = arr_at + first;
    for (int s = lane; s < per; s += 64) cand[w][s] = at[s];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes are visible
    __builtin_amdgcn_wave_barrier();
    int32_t keep[4] = {-1, -1, -1, -1};
    wave_accept(cand[w], per, k, 0, lane, [&](int q, int, int32_t a, bool is, bool acc) {
        keep[q] = acc ? a : -1;
        if (is && !acc && arr_state) arr_state[a] = kArrLate;
    });
    __builtin_amdgcn_wave_barrier();   // every rank is formed before the table changes
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = lane + 64 * q;
        if (s < per) {
            const int32_t a = keep[q];
            cand[w][s] = a;
            at[s] = a;
            inplace[w][s] = optimistic && a >= 0 && open_len[first + s] == a;
            open_len[first + s] = a < 0 ? -1 : pkt_len[a] - len_of(ad_len, ad_all, a) - 12;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    const int nfill = wave_rows(k, m, lane, [&](int s) { return cand[w][s] >= 0; }, lavail[w],
                                lhole[w], rows + ge.rows(g), [](int, int) {});
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    // the accepted data packets into their own slots, the accepted FEC packets into the holes
    for (int i = 0; i < k; ++i) {
        const int32_t a = __builtin_amdgcn_readfirstlane(cand[w][i]);   // the same in every lane
        if (a < 0 || __builtin_amdgcn_readfirstlane((int)inplace[w][i])) continue;
        const int al = len_of(ad_len, ad_all, a);
        const int pl = pkt_len[a] - al - 12;
        wave_place(sl.slot(blocks, g, k, i, bb), pkt + a * pkt_stride + al + 12, pl, bb, 2,
                   sl.prefix_of(pl, a), lane);
    }
    for (int h = 0; h < nfill; ++h) {
        const int32_t a = __builtin_amdgcn_readfirstlane(cand[w][k + lavail[w][h]]);
        const int al = len_of(ad_len, ad_all, a);
        wave_place(sl.slot(blocks, g, k, lhole[w][h], bb), pkt + a * pkt_stride + al + 12,
                   pkt_len[a] - al - 12, bb, 0, 0u, lane);
    }
}

// One lane per arrival, after the assemble: an arrival that opened (arr_state >= 0) and is not
// the one its slot kept was not the first copy of its index: kArrDuplicate.  (The first copy
// of a slot that was not kept already carries kArrLate.)
// Mixed geometry only, one lane per slot, after the assemble: a slot below npkt that no group of
// the call owns (the clipped span of a rejected group, a gap of the table, the capacity past the
// table's total) still holds the init pass's kArrNone, which no arrival index can equal; it and
// its open_len become -1, as a slot without an accepted arrival has them.  (With the uniform
// geometry every slot belongs to a group and the assemble writes it.)
__global__ __launch_bounds__(kPPThreads) void arrivals_unowned_kernel(long long slots,
                                                                      int32_t* arr_at,
                                                                      int32_t* open_len) {
    const long long p = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (p >= slots) return;
    if (arr_at[p] != kArrNone) return;
    arr_at[p] = -1;
    open_len[p] = -1;
}

// F: a group's first slot (UniFirst, MixedFirst); only an arrival tagged to a group the call
// runs has a state >= 0.
struct UniFirst {
    int per;
    __device__ __forceinline__ long long operator()(long long g) const { return g * per; }
};
struct MixedFirst {
    const int32_t* first;
    __device__ __forceinline__ long long operator()(long long g) const { return first[g]; }
};
template <class F>
__global__ __launch_bounds__(kPPThreads) void arrivals_state_kernel(
    F first, long long n, const int32_t* __restrict__ arr_group,
    const uint8_t* __restrict__ arr_index, const int32_t* __restrict__ arr_at,
    int32_t* arr_state) {
    const long long a = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (a >= n) return;
    if (arr_state[a] < 0) return;
    if (arr_at[first((long long)arr_group[a]) + arr_index[a]] != (int32_t)a)
        arr_state[a] = kArrDuplicate;
}

// ------------------------------------------------------------------ receiver window
// The arrival-order receiver with its state kept on the device between calls (DESIGN.md section
// 6.7; include/quic_fec.h, "Receiver window").  Every slot p = g * (k + m) + i owns a hold row of
// hold_stride bytes and a state: kSlotEmpty, kSlotSeen (a first copy that came late), or the
// plaintext length of the packet it holds.  A push binds its arrivals as the one-shot call does,
// by a minimum over arrival indices, but against the carried state: rxwin_init_kernel gives a
// slot that is not empty the value kWinTaken, below every arrival index, so no arrival of the
// push can win it and all that hit it come out as duplicates.  An accepted packet lies in its own
// row as prefix || payload || zeros (data) or plaintext || zeros (FEC), so the first bb bytes of
// the row are the one-shot call's block for any bb up to hold_stride, and a group that completes
// hands the decode the addresses of its rows: nothing is copied.
constexpr int32_t kSlotEmpty = -1, kSlotSeen = -2;
constexpr int32_t kWinTaken = -1;
constexpr int kWinOpen = -3, kWinDelivered = -5;

// One lane per slot.  pre_at: null without the optimistic write.
__global__ __launch_bounds__(kPPThreads) void rxwin_init_kernel(
    long long slots, const int32_t* __restrict__ slot_state, int32_t* arr_at, int32_t* pre_at) {
    const long long p = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (p >= slots) return;
    const int32_t v = slot_state[p] == kSlotEmpty ? kArrNone : kWinTaken;
    arr_at[p] = v;
    if (pre_at) pre_at[p] = v;
}

// The pre and open passes of a push are arrivals_pre_kernel and open_arrivals_kernel over
// (UniGeo, WinSlots) with the hold rows as blocks (reported as rxwin_pre_kernel and
// rxwin_open_kernel): the length checks run against the bb[g] of this push, a first candidate,
// data or FEC, streams into its hold row, zero-padded to hold_stride, and a slot that is not empty
// holds kWinTaken in both tables: it is never written and never won.

// One wave per group, after the open pass.  The group's candidates of this push are the slots
// whose arr_at holds an arrival; ranked by arrival index behind the packets the group holds
// already (wave_accept), the first k - held are accepted (slot state = the plaintext length), the
// others are late (slot state kSlotSeen, arr_state kArrLate).  An accepted packet that the open
// pass did not write (pre_at names another arrival, or there is no optimistic write) is placed into
// its row from the ring.  A group that reaches k completes: rows (wave_rows)
// over the held slots, block pointer g * k + i = the hold row of the packet in that position, rec
// pointer g * rmax + j = rec + rec_off[g] + j * bb, eff[g] = bb (this push's bb[g]), verdict 0.
// Every other group: eff 0 (the decode then dereferences none of its pointers), identity rows (the
// decode's prep sees a group without a loss) and verdict kWinOpen / kWinDelivered, which
// rxwin_finish_kernel turns into the group's status after the decode.  A completing group that
// holds a packet larger than this push's bb: verdict -3, eff 0.
__global__ __launch_bounds__(kAsmWaves * 64) void rxwin_assemble_kernel(
    int k, int m, WinSlots sl, uint8_t* hold, int32_t* slot_state, int32_t* held,
    int32_t* delivered, const uint8_t* __restrict__ pkt, long long pkt_stride,
    const int32_t* __restrict__ pkt_len, const int32_t* __restrict__ ad_len, int ad_all,
    int32_t* arr_state, int32_t* arr_at, const int32_t* __restrict__ pre_at, uint8_t* rec,
    const long long* __restrict__ rec_off, uint8_t* rows, unsigned long long* blk_ptrs,
    unsigned long long* rec_ptrs, int32_t* eff, int32_t* verdict) {
    __shared__ int32_t cand[kAsmWaves][256];   // the slot's candidate, then what is to be placed
    __shared__ uint8_t isheld[kAsmWaves][256], lavail[kAsmWaves][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * kAsmWaves + w;
    if (g >= sl.w.groups) return;   // uniform over the wave; no workgroup barrier below
    const int per = k + m, rmax = min(k, m);
    const long long first = g * per;
    int32_t* at = arr_at + first;
    int32_t* ss = slot_state + first;
    const int held0 = __builtin_amdgcn_readfirstlane(held[g]);
    const int deliv0 = __builtin_amdgcn_readfirstlane(delivered[g]);
    const int bb = __builtin_amdgcn_readfirstlane(sl.size(g));
    for (int s = lane; s < per; s += 64) cand[w][s] = at[s];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes are visible
    __builtin_amdgcn_wave_barrier();
    int32_t keep[4] = {-1, -1, -1, -1};
    int32_t st[4] = {kSlotEmpty, kSlotEmpty, kSlotEmpty, kSlotEmpty};
    int nacc = 0;
    wave_accept(cand[w], per, k, held0, lane, [&](int q, int s, int32_t a, bool is, bool acc) {
        if (s < per) st[q] = ss[s];
        if (acc) {
            keep[q] = a;
            st[q] = pkt_len[a] - len_of(ad_len, ad_all, a) - 12;
            ss[s] = st[q];
        } else if (is) {
            st[q] = kSlotSeen;
            ss[s] = kSlotSeen;
            if (arr_state) arr_state[a] = kArrLate;
        }
        nacc += __popcll(__ballot(acc));
    });
    __builtin_amdgcn_wave_barrier();   // every rank is formed before the table changes
    bool big = false;                   // a held packet that does not fit this push's bb
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = lane + 64 * q;
        if (s < per) {
            const int32_t a = keep[q];
            at[s] = a;
            // what the open pass wrote already is not placed again
            cand[w][s] = a >= 0 && pre_at && pre_at[first + s] == a ? -1 : a;
            isheld[w][s] = st[q] >= 0;
            big |= st[q] >= 0 && st[q] + sl.lead(s < k) > bb;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    // the accepted packets the open pass did not write, from the ring into their rows
    for (int s = 0; s < per; ++s) {
        const int32_t a = __builtin_amdgcn_readfirstlane(cand[w][s]);   // the same in every lane
        if (a < 0) continue;
        const int al = len_of(ad_len, ad_all, a);
        const int pl = pkt_len[a] - al - 12;
        wave_place(sl.slot(hold, g, k, s, bb), pkt + a * pkt_stride + al + 12, pl, sl.pad(bb),
                   sl.lead(s < k), sl.prefix_of(pl, a), lane);
    }
    const int newheld = held0 + nacc;
    const bool completes = held0 < k && newheld == k;
    const bool toobig = __ballot(big) != 0;
    if (lane == 0) {
        held[g] = newheld;
        if (completes) delivered[g] = 1;
        eff[g] = completes && !toobig ? bb : 0;
        verdict[g] = completes ? (toobig ? -3 : 0) : deliv0 ? kWinDelivered : kWinOpen;
    }
    if (!completes || toobig) {
        for (int i = lane; i < k; i += 64) rows[g * k + i] = (uint8_t)i;
        return;
    }
    // rows over the held slots; the blocks are the hold rows.  (A group that holds k has a held
    // FEC packet for every hole: row is never 255.)
    wave_rows(k, m, lane, [&](int s) { return isheld[w][s] != 0; }, lavail[w], nullptr,
              rows + g * k, [&](int i, int row) {
                  blk_ptrs[g * k + i] = (unsigned long long)(uintptr_t)sl.slot(
                      hold, g, k, row == 255 ? i : row, bb);
              });
    uint8_t* rg = rec + rec_off[g];
    for (int j = lane; j < rmax; j += 64)
        rec_ptrs[g * rmax + j] = (unsigned long long)(uintptr_t)(rg + (long long)j * bb);
}

// One lane per group, after the decode: the decode's prep wrote status 0 and no recovered row
// for a group that did not complete in this push (identity rows); its status is the verdict, and
// its rec_rows are 255 whatever path decoded.  rev_len -1 follows from eff 0 in the extraction.
__global__ __launch_bounds__(kPPThreads) void rxwin_finish_kernel(
    long long groups, int rmax, const int32_t* __restrict__ verdict, uint8_t* rec_rows,
    int32_t* status) {
    const long long g = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    if (g >= groups) return;
    const int v = verdict[g];
    if (v == 0) return;
    if (status) status[g] = v;
    for (int j = 0; j < rmax; ++j) rec_rows[g * rmax + j] = 255;
}

// One lane per slot of the listed groups (list null: of every group): back to empty.
__global__ __launch_bounds__(kPPThreads) void rxwin_release_kernel(
    long long groups, int per, long long count, const int32_t* __restrict__ list,
    int32_t* slot_state, int32_t* held, int32_t* delivered) {
    const long long q = (long long)blockIdx.x * kPPThreads + threadIdx.x;
    const long long e = q / per;
    if (e >= count) return;
    const int s = (int)(q - e * per);
    const long long g = list ? (long long)list[e] : e;
    if (g < 0 || g >= groups) return;
    slot_state[g * per + s] = kSlotEmpty;
    if (s == 0) {
        held[g] = 0;
        delivered[g] = 0;
    }
}

unsigned pp_grid(long long n) {
    return (unsigned)((n + kPPThreads - 1) / kPPThreads);
}

bool pp_grid_ok(long long n) {
    return (n + 63) / 64 <= 0x7fffffffLL;
}

unsigned tile_grid(long long n) {   // one wave (kTilePackets packets) per workgroup
    return (unsigned)((n + kTilePackets - 1) / kTilePackets);
}

}  // namespace


// The three seals: n packets with AD rows ad, the plaintext rows pr (PtRows, RaggedRows).
template <class R>
static hipError_t seal_go(const char* name, long long n, Rows ad, R pr, const int32_t* pt_len,
                          int pt_all, RowsOut out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!pp_grid_ok(n)) return hipErrorInvalidValue;
    note_kernel(name);
    qlaunch((null_seal_kernel<Fnv, R>), dim3(tile_grid(n)), dim3(64), kTileBytes, st, n, ad.p,
            ad.stride, ad.len, ad.len_all, pr, pt_len, pt_all, out.p, out.stride, out.len);
    return hipGetLastError();
}

hipError_t launch_null_seal(long long n, Rows ad, Rows pt, RowsOut out, hipStream_t st) {
    return seal_go("null_seal_kernel", n, ad, PtRows{nullptr, pt.p, pt.stride, 0, 1}, pt.len,
                   pt.len_all, out, st);
}

hipError_t launch_null_seal_groups(int k, int m, int bb, long long groups, const uint8_t* data,
                                   const uint8_t* parity, Rows hdr, const int32_t* pt_len,
                                   int pt_all, RowsOut out, hipStream_t st) {
    return seal_go("null_seal_kernel<groups>", groups * (k + m), hdr,
                   PtRows{data, parity, bb, k, m}, pt_len, pt_all, out, st);
}

hipError_t launch_null_open(long long n, Rows pkt, Rows ad, RowsOut out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!pp_grid_ok(n)) return hipErrorInvalidValue;
    note_kernel("null_open_kernel");
    qlaunch(null_open_kernel<Fnv>, dim3(pp_grid(n)), dim3(kPPThreads), 0, st, n, pkt.p, pkt.stride,
            pkt.len, pkt.len_all, ad.len, ad.len_all, out.p, out.stride, out.len);
    return hipGetLastError();
}

// The two opens: the slots sl (UniSlots, RaggedSlots) of every group's blocks.
template <class S>
static hipError_t open_go(const char* name, int k, int m, long long groups, S sl, Rows pkt,
                          Rows ad, uint8_t* blocks, uint8_t* rows, int32_t* open_len,
                          hipStream_t st) {
    const long long n = groups * (k + m);
    if (n <= 0) return hipSuccess;
    if (k + m > 256 || !pp_grid_ok(n)) return hipErrorInvalidValue;
    const long long wg = (groups + kAsmWaves - 1) / kAsmWaves;
    if (wg > 0x7fffffffLL) return hipErrorInvalidValue;
    note_kernel(name);
    qlaunch((open_group_kernel<Fnv, S>), dim3(tile_grid(n)), dim3(64), kTileBytes, st, k, m, sl, n,
            pkt.p, pkt.stride, pkt.len, ad.len, ad.len_all, blocks, open_len);
    qlaunch(open_assemble_kernel<S>, dim3((unsigned)wg), dim3(kAsmWaves * 64), 0, st, k, m, sl,
            groups, pkt.p, pkt.stride, pkt.len, ad.len, ad.len_all, open_len, blocks, rows);
    return hipGetLastError();
}

hipError_t launch_open_groups(int k, int m, int bb, long long groups, Rows pkt, Rows ad,
                              uint8_t* blocks, uint8_t* rows, int32_t* open_len,
                              hipStream_t st) {
    return open_go("open_group_kernel + open_assemble_kernel", k, m, groups, UniSlots{bb}, pkt, ad,
                   blocks, rows, open_len, st);
}

hipError_t launch_null_seal_groups_ragged(int k, int m, long long groups, RaggedView v,
                                          const uint8_t* data, const uint8_t* parity,
                                          bool after_encode, Rows hdr, const int32_t* pt_len,
                                          RowsOut out, hipStream_t st) {
    return seal_go("null_seal_kernel<ragged>", groups * (k + m), hdr,
                   RaggedRows{data, parity, v.in_off, v.out_off, v.bb, k, m, after_encode}, pt_len,
                   0, out, st);
}

hipError_t launch_open_groups_ragged(int k, int m, long long groups, RaggedView v, Rows pkt,
                                     Rows ad, uint8_t* blocks, uint8_t* rows, int32_t* open_len,
                                     hipStream_t st) {
    return open_go("open_group_kernel<ragged> + open_assemble_kernel<ragged>", k, m, groups,
                   RaggedSlots{v.bb, v.in_off, groups}, pkt, ad, blocks, rows, open_len, st);
}

hipError_t launch_frame_blocks_ragged(int k, long long groups, RaggedView v, Rows pay,
                                      const uint8_t* pn_len, int pn_all, uint8_t* data,
                                      int32_t* eff_bb, int32_t* status, hipStream_t st) {
    const long long n = groups * k;
    if (n <= 0) return hipSuccess;
    if (!pp_grid_ok(n)) return hipErrorInvalidValue;
    note_kernel("frame_blocks_kernel");
    qlaunch(frame_blocks_kernel, dim3(tile_grid(n)), dim3(64), kTileBytes, st, k, n, pay.p,
            pay.stride, pay.len, pn_len, pn_all, data, v.in_off, v.bb, eff_bb, status);
    return hipGetLastError();
}

hipError_t launch_null_seal_framed(int k, int m, long long groups, RaggedView v, Rows pay,
                                   const uint8_t* parity, Rows hdr, RowsOut out, int32_t* status,
                                   hipStream_t st) {
    return seal_go("null_seal_kernel<framed>", groups * (k + m), hdr,
                   FramedRows{pay, parity, v.out_off, v.bb, status, k, m}, nullptr, 0, out, st);
}

hipError_t launch_open_groups_framed(int k, int m, long long groups, RaggedView v, Rows pkt,
                                     Rows ad, const uint8_t* pn_len, int pn_all, uint8_t* blocks,
                                     uint8_t* rows, int32_t* open_len, hipStream_t st) {
    return open_go("open_group_kernel<framed> + open_assemble_kernel<framed>", k, m, groups,
                   FramedSlots{RaggedSlots{v.bb, v.in_off, groups}, pn_len, pn_all}, pkt, ad,
                   blocks, rows, open_len, st);
}

// The binding sequence of every arrival-order receiver, over the geometry Ge (UniGeo, MixedGeo)
// and the framed slots S (FramedSlots, WinSlots): init -> pre -> open -> assemble -> unowned ->
// state.  The pre, open and state kernels are shared and reported under lb's names; init(),
// where there is a slot, and assemble(workgroups), where a group owns one, launch the caller's
// own two kernels.  slots: the length of arr_at; pre_at: the pre-pass table (null: no optimistic
// write); blocks: what S::slot() takes; unowned_len: the open_len of a geometry that leaves slots
// without a group (null: every slot has one).
struct ArrLabels {
    const char *pre, *open, *state;
};
template <class Ge, class S, class F, class Init, class Asm>
static hipError_t bind_go(const ArrLabels& lb, typename Ge::A0 g0, typename Ge::A1 g1, F first,
                          long long groups, long long slots, S sl, const Arrivals& ar,
                          int32_t* arr_at, int32_t* pre_at, uint8_t* blocks, int32_t* unowned_len,
                          Init init, Asm assemble, hipStream_t st) {
    const long long n = ar.n, wg = (groups + kAsmWaves - 1) / kAsmWaves;
    if (n > 0x7fffffffLL || slots > 0x7fffffffLL || wg > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool owned = slots > 0 && groups > 0;
    if (slots > 0) init();
    if (n > 0 && owned && pre_at) {
        note_kernel(lb.pre);
        qlaunch((arrivals_pre_kernel<Ge, S>), dim3(pp_grid(n)), dim3(kPPThreads), 0, st, g0, g1, sl,
                n, ar.pkt.stride, ar.pkt.len, ar.ad.len, ar.ad.len_all, ar.arr_group, ar.arr_index,
                pre_at);
    }
    if (n > 0) {
        note_kernel(lb.open);
        qlaunch((open_arrivals_kernel<Fnv, Ge, S>), dim3(tile_grid(n)), dim3(64), kTileBytes, st,
                g0, g1, sl, n, ar.pkt.p, ar.pkt.stride, ar.pkt.len, ar.ad.len, ar.ad.len_all,
                ar.arr_group, ar.arr_index, ar.arr_state, arr_at,
                (const int32_t*)(owned ? pre_at : nullptr), blocks);
    }
    if (owned) assemble((unsigned)wg);
    if (unowned_len && slots > 0) {
        note_kernel("arrivals_unowned_kernel");
        qlaunch(arrivals_unowned_kernel, dim3(pp_grid(slots)), dim3(kPPThreads), 0, st, slots,
                arr_at, unowned_len);
    }
    if (n > 0 && owned && ar.arr_state) {
        note_kernel(lb.state);
        qlaunch(arrivals_state_kernel<F>, dim3(pp_grid(n)), dim3(kPPThreads), 0, st, first, n,
                ar.arr_group, ar.arr_index, (const int32_t*)arr_at, ar.arr_state);
    }
    return hipGetLastError();
}

// The one-shot open: the pre-pass table lives in open_len until the assemble writes open_len;
// mixed: the kernels' names carry "<mixed>".
template <class Ge, class F>
static hipError_t arrivals_go(bool mixed, typename Ge::A0 g0, typename Ge::A1 g1, F first,
                              long long groups, long long slots, FramedSlots sl,
                              const Arrivals& ar, int32_t* arr_at, uint8_t* blocks, uint8_t* rows,
                              int32_t* open_len, bool optimistic, hipStream_t st) {
    static const ArrLabels uni{"arrivals_pre_kernel", "open_arrivals_kernel",
                               "arrivals_state_kernel"};
    static const ArrLabels mix{"arrivals_pre_kernel<mixed>", "open_arrivals_kernel<mixed>",
                               "arrivals_state_kernel<mixed>"};
    int32_t* pre_at = optimistic ? open_len : nullptr;
    return bind_go<Ge>(
        mixed ? mix : uni, g0, g1, first, groups, slots, sl, ar, arr_at, pre_at, blocks,
        mixed ? open_len : nullptr,
        [&] {
            note_kernel("arrivals_init_kernel");
            qlaunch(arrivals_init_kernel, dim3(pp_grid(slots)), dim3(kPPThreads), 0, st, slots,
                    arr_at, pre_at);
        },
        [&](unsigned wg) {
            note_kernel(mixed ? "arrivals_assemble_kernel<mixed>" : "arrivals_assemble_kernel");
            qlaunch(arrivals_assemble_kernel<Ge>, dim3(wg), dim3(kAsmWaves * 64), 0, st, g0, g1,
                    sl, ar.pkt.p, ar.pkt.stride, ar.pkt.len, ar.ad.len, ar.ad.len_all,
                    ar.arr_state, arr_at, open_len, optimistic, blocks, rows);
        },
        st);
}

hipError_t launch_open_arrivals_framed(int k, int m, long long groups, RaggedView v,
                                       const Arrivals& ar, int32_t* arr_at, uint8_t* blocks,
                                       uint8_t* rows, int32_t* open_len, bool optimistic,
                                       hipStream_t st) {
    if (k + m > 255) return hipErrorInvalidValue;
    return arrivals_go<UniGeo>(
        false, k, m, UniFirst{k + m}, groups, groups * (k + m),
        FramedSlots{RaggedSlots{v.bb, v.in_off, groups}, ar.pn_len, ar.pn_all}, ar, arr_at, blocks,
        rows, open_len, optimistic, st);
}

hipError_t launch_extract_revived(int k, int m, long long groups, RaggedView v, const uint8_t* rec,
                                  const uint8_t* rec_rows, const int32_t* status, RowsOut rev,
                                  uint8_t* rev_pn_len, hipStream_t st) {
    const int rmax = std::min(k, m);
    const long long n = groups * rmax;
    if (n <= 0) return hipSuccess;
    if (!pp_grid_ok(n)) return hipErrorInvalidValue;
    note_kernel("extract_revived_kernel");
    qlaunch(extract_revived_kernel, dim3(tile_grid(n)), dim3(64), kTileBytes, st, rmax, n, rec,
            v.out_off, v.bb, rec_rows, status, rev.p, rev.stride, rev.len, rev_pn_len);
    return hipGetLastError();
}

hipError_t launch_open_status(int k, int rmax, long long groups, const uint8_t* rows,
                              uint8_t* rec_rows, int32_t* status, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    if (!pp_grid_ok(groups)) return hipErrorInvalidValue;
    qlaunch(open_status_kernel<UniRowsK>, dim3(pp_grid(groups)), dim3(kPPThreads), 0, st, groups,
            UniRowsK{k}, rmax, rows, rec_rows, status);
    return hipGetLastError();
}

// ---- the receiver window
hipError_t launch_rxwin_bind(const RxWin& w, const int32_t* bb, const Arrivals& ar, uint8_t* rec,
                             const long long* rec_off, bool optimistic, hipStream_t st) {
    static const ArrLabels lb{"rxwin_pre_kernel", "rxwin_open_kernel", "arrivals_state_kernel"};
    const int per = w.k + w.m;
    const long long slots = w.groups * per;
    if (per > 255) return hipErrorInvalidValue;
    int32_t* pre_at = optimistic && ar.n > 0 ? w.pre_at : nullptr;
    const WinSlots sl{HoldRows{bb, w.hold_stride, w.groups, per}, ar.pn_len, ar.pn_all};
    return bind_go<UniGeo>(
        lb, w.k, w.m, UniFirst{per}, w.groups, slots, sl, ar, w.arr_at, pre_at, w.hold, nullptr,
        [&] {
            note_kernel("rxwin_init_kernel");
            qlaunch(rxwin_init_kernel, dim3(pp_grid(slots)), dim3(kPPThreads), 0, st, slots,
                    (const int32_t*)w.slot_state, w.arr_at, pre_at);
        },
        [&](unsigned wg) {
            note_kernel("rxwin_assemble_kernel");
            qlaunch(rxwin_assemble_kernel, dim3(wg), dim3(kAsmWaves * 64), 0, st, w.k, w.m, sl,
                    w.hold, w.slot_state, w.held, w.delivered, ar.pkt.p, ar.pkt.stride, ar.pkt.len,
                    ar.ad.len, ar.ad.len_all, ar.arr_state, w.arr_at, (const int32_t*)pre_at, rec,
                    rec_off, w.rows, w.blk_ptrs, w.rec_ptrs, w.eff, w.verdict);
        },
        st);
}

hipError_t launch_rxwin_finish(const RxWin& w, uint8_t* rec_rows, int32_t* status,
                               hipStream_t st) {
    if (w.groups <= 0) return hipSuccess;
    note_kernel("rxwin_finish_kernel");
    qlaunch(rxwin_finish_kernel, dim3(pp_grid(w.groups)), dim3(kPPThreads), 0, st, w.groups,
            std::min(w.k, w.m), (const int32_t*)w.verdict, rec_rows, status);
    return hipGetLastError();
}

hipError_t launch_rxwin_release(const RxWin& w, long long count, const int32_t* list,
                                hipStream_t st) {
    const int per = w.k + w.m;
    if (!list) count = w.groups;
    if (count <= 0 || w.groups <= 0) return hipSuccess;
    if (count > 0x7fffffffLL / per || !pp_grid_ok(count * per)) return hipErrorInvalidValue;
    note_kernel("rxwin_release_kernel");
    qlaunch(rxwin_release_kernel, dim3(pp_grid(count * per)), dim3(kPPThreads), 0, st, w.groups,
            per, count, list, w.slot_state, w.held, w.delivered);
    return hipGetLastError();
}

// ---- the mixed-code wire path (pp_mixed.h)
hipError_t launch_mixed_wire_plan(const MixedSet& s, long long groups, MixedWire w,
                                  const Rows* pay, hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    if (!pp_grid_ok(groups)) return hipErrorInvalidValue;
    note_kernel("mixed_wire_plan_kernel");
    qlaunch(mixed_wire_plan_kernel, dim3(pp_grid(groups)), dim3(kPPThreads), 0, st, groups,
            s.codes, s.ncodes, w.code, w.bb, w.pkt_first, w.npkt, pay ? w.pay_first : nullptr,
            w.npay, pay ? pay->len : nullptr, pay ? pay->stride : 0LL, w.eff, w.ecode);
    return hipGetLastError();
}

hipError_t launch_frame_blocks_mixed(const MixedSet& s, long long groups, MixedWire w, Rows pay,
                                     const uint8_t* pn_len, int pn_all, uint8_t* data,
                                     const long long* data_off, hipStream_t st) {
    if (groups <= 0 || w.npay <= 0) return hipSuccess;
    if (!pp_grid_ok(w.npay)) return hipErrorInvalidValue;
    note_kernel("frame_blocks_kernel<mixed>");
    qlaunch(frame_blocks_mixed_kernel, dim3(tile_grid(w.npay)), dim3(64), kTileBytes, st, groups,
            w.npay, s.codes, (const uint8_t*)w.ecode, (const int32_t*)w.eff, w.pay_first, pay.p,
            pay.stride, pay.len, pn_len, pn_all, data, data_off);
    return hipGetLastError();
}

hipError_t launch_null_seal_mixed(const MixedSet& s, long long groups, MixedWire w, Rows pay,
                                  const uint8_t* parity, const long long* par_off, Rows hdr,
                                  RowsOut out, int32_t* status, hipStream_t st) {
    return seal_go("null_seal_kernel<mixed>", w.npkt, hdr,
                   MixedRows{pay, parity, par_off, w.eff, w.ecode, s.codes, w.pkt_first,
                             w.pay_first, groups, w.npkt, status},
                   nullptr, 0, out, st);
}

hipError_t launch_open_arrivals_mixed(const MixedSet& s, long long groups, MixedWire w,
                                      const long long* blocks_off, const Arrivals& ar,
                                      int32_t* arr_at, uint8_t* blocks, uint8_t* rows,
                                      int32_t* open_len, bool optimistic, hipStream_t st) {
    return arrivals_go<MixedGeo>(
        true, MixedTabs{s.codes, w.ecode, w.pkt_first}, s.kmax, MixedFirst{w.pkt_first}, groups,
        w.npkt, FramedSlots{RaggedSlots{w.eff, blocks_off, groups}, ar.pn_len, ar.pn_all}, ar,
        arr_at, blocks, rows, open_len, optimistic, st);
}

hipError_t launch_open_status_mixed(const MixedSet& s, long long groups, MixedWire w,
                                    const uint8_t* rows, uint8_t* rec_rows, int32_t* status,
                                    hipStream_t st) {
    if (groups <= 0) return hipSuccess;
    if (!pp_grid_ok(groups)) return hipErrorInvalidValue;
    note_kernel("open_status_kernel<mixed>");
    qlaunch(open_status_kernel<MixedGeo>, dim3(pp_grid(groups)), dim3(kPPThreads), 0, st, groups,
            MixedGeo(MixedTabs{s.codes, w.ecode, w.pkt_first}, s.kmax), s.rmax, rows, rec_rows, status);
    return hipGetLastError();
}

// extract_revived_kernel reads no k or m: the set's rmax is its row stride, and rec_rows is 255
// from a group's own count on
hipError_t launch_extract_revived_mixed(const MixedSet& s, long long groups, MixedWire w,
                                        const uint8_t* rec, const long long* rec_off,
                                        const uint8_t* rec_rows, const int32_t* status,
                                        RowsOut rev, uint8_t* rev_pn_len, hipStream_t st) {
    const long long n = groups * s.rmax;
    if (n <= 0) return hipSuccess;
    if (!pp_grid_ok(n)) return hipErrorInvalidValue;
    note_kernel("extract_revived_kernel<mixed>");
    qlaunch(extract_revived_kernel, dim3(tile_grid(n)), dim3(64), kTileBytes, st, s.rmax, n, rec,
            rec_off, (const int32_t*)w.eff, rec_rows, status, rev.p, rev.stride, rev.len,
            rev_pn_len);
    return hipGetLastError();
}

}  // namespace qfec
