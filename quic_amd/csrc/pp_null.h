// pp_null.h — launchers of the packet-protection kernels (pp_null.hip) that sit next to the
// FEC codec: the per-packet seal / open, all k + m packets of a group sealed in one launch,
// and the receiver's open -> group assembly that feeds the decode.  Packet arrays travel as
// Rows / RowsOut (fec_kernels.h).
#pragma once
#include "fec_kernels.h"

namespace qfec {

// NullEncrypter seal / NullDecrypter open over n packets.  Open: ad carries only the lengths
// (the associated data is the head of the packet).
hipError_t launch_null_seal(long long n, Rows ad, Rows pt, RowsOut out, hipStream_t st);
hipError_t launch_null_open(long long n, Rows pkt, Rows ad, RowsOut out, hipStream_t st);

// Seal packet p = g * (k + m) + i of every group: AD = hdr row p, PT = data block (g, i) for
// i < k, parity block (g, i - k) otherwise (rows of bb bytes), PT length pt_len[p] (or
// pt_all), wire packet at out row p (quic_packet_creator.cc:733-736 seals every data packet,
// :948-953 every FEC packet).
hipError_t launch_null_seal_groups(int k, int m, int bb, long long groups, const uint8_t* data,
                                   const uint8_t* parity, Rows hdr, const int32_t* pt_len,
                                   int pt_all, RowsOut out, hipStream_t st);

// Receiver: open packet p = g * (k + m) + i (pkt.len[p] < 0: not received; ad: lengths only).
// A data packet's plaintext goes to blocks[g][i], zero-padded to bb; open_len[p] = plaintext
// bytes, or -1 (not received, malformed, longer than bb, or tag mismatch).  Then one wave per
// group builds rows[g][*] (data row i where packet i opened, else the next opened parity
// packet, ascending, whose plaintext it copies into the hole; 255 when none is left) for the
// decode.
hipError_t launch_open_groups(int k, int m, int bb, long long groups, Rows pkt, Rows ad,
                              uint8_t* blocks, uint8_t* rows, int32_t* open_len, hipStream_t st);

// Ragged forms (v.bb [G], byte offsets [G] that are multiples of 16; device arrays, never read
// back): per group what the two launchers above do with bb = v.bb[g].  Packets stay dense by
// packet index.
// Seal: PT of packet (g, i) = block i of data + v.in_off[g] ([k][bb[g]]) for i < k, block
// i - k of parity + v.out_off[g] ([m][bb[g]]) otherwise; pt_len == nullptr: the whole block.
// A packet whose pt_len exceeds bb[g], and every packet of a group with bb[g] < 1, is
// rejected (out.len -1, nothing written); after_encode: so is every packet of a group the
// ragged encode rejected (ragged_encode_rejects).
hipError_t launch_null_seal_groups_ragged(int k, int m, long long groups, RaggedView v,
                                          const uint8_t* data, const uint8_t* parity,
                                          bool after_encode, Rows hdr, const int32_t* pt_len,
                                          RowsOut out, hipStream_t st);
// Open: slot s of group g is blocks + v.in_off[g] + s * bb[g]; rows [G][k] stays dense.  A
// group with bb[g] < 1: every open_len -1, every row 255, nothing written.
hipError_t launch_open_groups_ragged(int k, int m, long long groups, RaggedView v, Rows pkt,
                                     Rows ad, uint8_t* blocks, uint8_t* rows, int32_t* open_len,
                                     hipStream_t st);

// Framed forms (QuicFecGroup's wire format over the ragged layout).  A
// data packet's block is prefix || payload || zeros, prefix = (len | pn_len << 14) & 0xffff,
// little-endian; its wire packet carries the payload alone.  pay: payload row g * k + i, pay.len
// [G * k] (device array, never null).  pn_len: u8 per packet, or null: pn_all for all.
// Frame: block (g, i) at data + v.in_off[g] + i * bb[g].  A group framed_group_rejects names
// (fec_kernels.h) is not written.  eff_bb [G] (may be null) receives bb[g], 0 for a rejected
// group: the sizes the encode after it runs with; status [G] (may be null) 0 / -3.
hipError_t launch_frame_blocks_ragged(int k, long long groups, RaggedView v, Rows pay,
                                      const uint8_t* pn_len, int pn_all, uint8_t* data,
                                      int32_t* eff_bb, int32_t* status, hipStream_t st);
// Seal after the frame and the encode: PT of packet (g, i) = payload row g * k + i for i < k,
// block i - k of parity + v.out_off[g] otherwise.  No packet of a group the frame or the encode
// rejected is sealed (out.len -1); status [G] (may be null) gets -3 for the frame's.
hipError_t launch_null_seal_framed(int k, int m, long long groups, RaggedView v, Rows pay,
                                   const uint8_t* parity, Rows hdr, RowsOut out, int32_t* status,
                                   hipStream_t st);
// launch_open_groups_ragged, but a data packet's plaintext goes to slot + 2 behind its prefix
// (opened length, pn_len [G * (k + m)] or pn_all) and may be at most bb[g] - 2 bytes long.
hipError_t launch_open_groups_framed(int k, int m, long long groups, RaggedView v, Rows pkt,
                                     Rows ad, const uint8_t* pn_len, int pn_all, uint8_t* blocks,
                                     uint8_t* rows, int32_t* open_len, hipStream_t st);
// The framed open over ar.n packets in arrival order (Arrivals, fec_kernels.h; DESIGN.md section
// 6.5).  Per group the first copy of each index that opens is a candidate, the k earliest
// candidates are accepted, and blocks, rows and open_len [G * (k + m)] come out as
// launch_open_groups_framed writes them for the accepted packets placed by slot.  arr_at
// [G * (k + m)]: the arrival accepted for each slot, -1 without one (the call's only table, set up
// again by every call); ar.arr_state: the plaintext length of an accepted arrival, -1 rejected, -2
// ignored tag, -3 duplicate, -4 late.
// optimistic: a data arrival that is its slot's first candidate by the length checks alone (a
// pre-pass finds it; its table lives in open_len until the assemble writes open_len) streams its
// plaintext into the slot during the open pass, so an in-order ring is read once; without it the
// assemble reads every accepted packet a second time.  The outputs are the same either way but
// for the bytes of a slot whose row is 255.
// Five launches (init, pre, open, assemble, state); no pre without optimistic, no state without
// arr_state.
hipError_t launch_open_arrivals_framed(int k, int m, long long groups, RaggedView v,
                                       const Arrivals& ar, int32_t* arr_at, uint8_t* blocks,
                                       uint8_t* rows, int32_t* open_len, bool optimistic,
                                       hipStream_t st);
// After the decode: recovered block (g, j) at rec + v.out_off[g] + j * bb[g] with
// rec_rows[g * rmax + j] != 255 and status[g] == 0 (status null: every group) -> its payload at
// rev row g * rmax + j, rev.len its length (clamped to bb[g] - 2), rev_pn_len (may be null) the
// prefix's top two bits; every other entry, and a payload longer than rev.stride: rev.len -1,
// nothing else written.  rev.p and rev.stride need no alignment.
hipError_t launch_extract_revived(int k, int m, long long groups, RaggedView v, const uint8_t* rec,
                                  const uint8_t* rec_rows, const int32_t* status, RowsOut rev,
                                  uint8_t* rev_pn_len, hipStream_t st);

// The receiver window (include/quic_fec.h, "Receiver window"): the
// arrival-order open against state that stays on the device between calls.  The sections of the
// window's allocation (fec_host_plan.h, RxwinLayout) as device pointers.
struct RxWin {
    int k, m;
    long long groups, hold_stride;
    uint8_t* hold;                            // [groups * (k + m)][hold_stride]
    int32_t *slot_state, *held, *delivered;   // the carried state
    int32_t *arr_at, *pre_at;                 // one push's binding and pre-pass tables
    uint8_t* rows;                            // [groups][k], the decode's rows_in
    unsigned long long *blk_ptrs, *rec_ptrs;  // [groups * k], [groups * min(k, m)]
    int32_t *eff, *verdict;                   // [groups]: the effective bb; 0 or the status to set
};
// One push up to the decode: launch_open_arrivals_framed's sequence with the window's own init and
// assemble kernels; its pre and open passes are the one-shot call's kernels over the hold rows,
// where an FEC packet's first candidate is written optimistically too.
// Afterwards w.rows, w.blk_ptrs, w.rec_ptrs and w.eff are the pointer-table decode's arguments:
// eff[g] = bb[g] for a group that completes in this push, 0 for every other.
hipError_t launch_rxwin_bind(const RxWin& w, const int32_t* bb, const Arrivals& ar, uint8_t* rec,
                             const long long* rec_off, bool optimistic, hipStream_t st);
// After the decode: status (may be null) and rec_rows 255 of the groups that did not complete.
hipError_t launch_rxwin_finish(const RxWin& w, uint8_t* rec_rows, int32_t* status,
                               hipStream_t st);
// list [count] (device, int32) back to empty; list null: every group.
hipError_t launch_rxwin_release(const RxWin& w, long long count, const int32_t* list,
                                hipStream_t st);

// After the decode of an open batch: groups with an unfilled slot get status -3 and no
// recovered rows.
hipError_t launch_open_status(int k, int rmax, long long groups, const uint8_t* rows,
                              uint8_t* rec_rows, int32_t* status, hipStream_t st);

}  // namespace qfec
