// pp_mixed.h — launchers of the mixed-code wire path (pp_null.hip's kernels over the mixed
// geometry): the framed sender and the arrival-order receiver with a
// (k, m) per group through a code set.  Kept beside pp_null.h: only the two mixed wire entry
// points include it, so gf_mixed.h stays out of every other dispatch.
#pragma once
#include "gf_mixed.h"

namespace qfec {

// The geometry of one mixed wire call.  The caller's arrays (device memory, never read back) and
// the call's two work arrays, which the plan kernel writes and every later kernel reads in their
// place: a group whose code or span is rejected is decided once, there.
struct MixedWire {
    const uint8_t* code;        // [G] index into the set
    const int32_t* bb;          // [G]
    const int32_t* pkt_first;   // [G + 1] first wire packet / slot of each group
    const int32_t* pay_first;   // [G + 1] first payload row of each group; sender only
    long long npkt, npay;       // capacities of the per-packet and per-payload arrays
    int32_t* eff;               // [G] work: the size group g runs with; 0: the sender's frame
                                //   rejected it (framed_group_rejects), or the group is rejected
    uint8_t* ecode;             // [G] work: code[g], or 255 for a group rejected with status -2
};

// One lane per group: ecode[g] and eff[g].  A group is rejected (ecode 255, eff 0) when code[g]
// >= ncodes, when its pkt_first span is not k_g + m_g wide inside [0, npkt], or (pay non-null:
// the sender) when its pay_first span is not k_g wide inside [0, npay].  Sender: eff[g] = 0 also
// where framed_group_rejects names the group, asked here once for the frame, the seal and the
// status.  Entries of the tables are read at g and g + 1 only.
hipError_t launch_mixed_wire_plan(const MixedSet& s, long long groups, MixedWire w,
                                  const Rows* pay, hipStream_t st);

// launch_frame_blocks_ragged over the mixed geometry: payload row q of [npay] belongs to the
// group whose pay_first span holds it; block (g, i) at data + data_off[g] + i * eff[g].
hipError_t launch_frame_blocks_mixed(const MixedSet& s, long long groups, MixedWire w, Rows pay,
                                     const uint8_t* pn_len, int pn_all, uint8_t* data,
                                     const long long* data_off, hipStream_t st);
// launch_null_seal_framed over the mixed geometry: packet p of [npkt] belongs to the group whose
// pkt_first span holds it; out.len -1 for a packet of no group, of a rejected group, of a group
// the frame or the encode rejected.  status [G] (may be null) gets -3 for the frame's.
hipError_t launch_null_seal_mixed(const MixedSet& s, long long groups, MixedWire w, Rows pay,
                                  const uint8_t* parity, const long long* par_off, Rows hdr,
                                  RowsOut out, int32_t* status, hipStream_t st);
// launch_open_arrivals_framed over the mixed geometry: the slot of arrival a is pkt_first[g] +
// arr_index[a]; arr_at and open_len are [npkt]; rows is [G][kmax].  Arrivals of a rejected group
// are ignored and nothing of the group is written; a last pass (arrivals_unowned_kernel) sets
// arr_at and open_len of every slot below npkt that no kept group owns to -1.
hipError_t launch_open_arrivals_mixed(const MixedSet& s, long long groups, MixedWire w,
                                      const long long* blocks_off, const Arrivals& ar,
                                      int32_t* arr_at, uint8_t* blocks, uint8_t* rows,
                                      int32_t* open_len, bool optimistic, hipStream_t st);
// launch_open_status with the group's own k, rows at g * kmax and rec_rows at g * rmax (the
// set's); a rejected group keeps the decode's -2.
hipError_t launch_open_status_mixed(const MixedSet& s, long long groups, MixedWire w,
                                    const uint8_t* rows, uint8_t* rec_rows, int32_t* status,
                                    hipStream_t st);
// launch_extract_revived with rows g * rmax + j over the set's rmax and the sizes eff.
hipError_t launch_extract_revived_mixed(const MixedSet& s, long long groups, MixedWire w,
                                        const uint8_t* rec, const long long* rec_off,
                                        const uint8_t* rec_rows, const int32_t* status,
                                        RowsOut rev, uint8_t* rev_pn_len, hipStream_t st);

}  // namespace qfec
