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

// After the decode of an open batch: groups with an unfilled slot get status -3 and no
// recovered rows.
hipError_t launch_open_status(int k, int rmax, long long groups, const uint8_t* rows,
                              uint8_t* rec_rows, int32_t* status, hipStream_t st);

}  // namespace qfec
