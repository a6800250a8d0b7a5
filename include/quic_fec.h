/*
 * quic_fec.h — C ABI of the MI355X-native FEC engine (libquic_fec.so).
 *
 * Drop-in boundary for the QuicR packet-group FEC path.  The reference calls the
 * Longhair codec through three extern "C" entry points
 * (/root/reference/net/quic/core/libcat/cauchy_256.h:47,78,103); this library exports
 * the same three symbols with identical semantics, executed by hand-written gfx950
 * kernels, plus batched device-pointer and host-pointer entry points that process
 * thousands of independent groups per launch.  Plain pointers and sizes only.
 *
 * Return codes (all entry points): 0 = OK; -1 = unsupported parameters, exactly where
 * the reference returns -1 (m > 1 and (k + m > 256 or block_bytes % 8 != 0));
 * <= -2 = errors the reference has no code for (bad arguments, GPU runtime failure;
 * see qfec_last_error()).
 */
#ifndef QUIC_AMD_QUIC_FEC_H
#define QUIC_AMD_QUIC_FEC_H

#ifdef __cplusplus
extern "C" {
#endif

#define CAUCHY_256_VERSION 2

#if defined(QFEC_BUILD)
#define QFEC_API __attribute__((visibility("default")))
#else
#define QFEC_API
#endif

/* Same layout as cauchy_256.h:52-55. */
typedef struct _Block {
    unsigned char *data;
    unsigned char row;
} Block;

/* ---------------------------------------------------------------------------------
 * Single-group drop-ins (host pointers; synchronous).
 * ------------------------------------------------------------------------------- */

/* Replaces _cauchy_256_init (cauchy_256.h:47, cauchy_256.cpp:389-398).  Returns 0 on
 * success and -1 on a version mismatch — what the reference code does (its header
 * comment says otherwise).  Also brings up the default GPU context. */
QFEC_API int _cauchy_256_init(int expected_version);
#ifndef cauchy_256_init
#define cauchy_256_init() _cauchy_256_init(CAUCHY_256_VERSION)
#endif

/* Replaces cauchy_256_encode (cauchy_256.h:78, cauchy_256.cpp:1502-1601): k data blocks
 * (pointer array) -> m recovery blocks stored end to end.  k <= 1 copies data[0] into
 * every output.  For m > 1 with k + m > 256 or block_bytes % 8 != 0 it writes the XOR
 * parity into the first recovery block and returns -1, like the reference. */
QFEC_API int cauchy_256_encode(int k, int m, const unsigned char *data_ptrs[], void *recovery_blocks,
                      int block_bytes);

/* Replaces cauchy_256_decode (cauchy_256.h:103, cauchy_256.cpp:1254-1413): in place.  The
 * i-th block (array order) tagged row >= k receives the i-th smallest missing data row:
 * its data is overwritten with that row's data and its row field rewritten. */
QFEC_API int cauchy_256_decode(int k, int m, Block *blocks, int block_bytes);

/* ---------------------------------------------------------------------------------
 * Batched engine.  Layouts (row-major, bb = block_bytes):
 *   data   [G][k][bb]   parity [G][m][bb]
 *   blocks [G][k][bb]   rows   [G][k]  (u8 row tags, data 0..k-1, parity k..k+m-1)
 *   status [G]          per-group return code of the equivalent cauchy_256_decode call,
 *                       or -3 for a malformed receive set whose reference result is not
 *                       defined (a row tag >= k + m, the same recovery row twice, fewer
 *                       missing data rows than recovery blocks); such a group is left as
 *                       it was
 * The byte buffers of the uniform calls (data, parity, blocks, out, rec and the row-tag arrays)
 * may start at any address, like the reference codec's: the library picks its kernels from the
 * pointers' alignment (16-byte aligned data / blocks and 8-byte aligned outputs take the fastest
 * ones) and the result is the same bytes.  status is an int array, aligned as its type requires.
 * A call writes the bytes this header names and no others.
 * `stream` is a hipStream_t (NULL = HIP's null stream, as everywhere in HIP).  Device
 * entry points only enqueue work on that stream; they do not synchronise.
 *
 * Streams and contexts: a context may be used from several streams.  Its eager decodes
 * share one workspace, so the library orders a decode behind the previous eager decode of
 * the same context when they are enqueued on different streams (an event, not a host
 * wait); calls on one stream are ordered by the stream.  Decodes captured into a HIP graph
 * use a second workspace of the context, so a graph replay, on whatever stream it is
 * launched, never races an eager call.  Graphs captured on one context share that second
 * workspace: replay them in one stream order (or capture on separate contexts), and capture
 * the calls of one context on one stream.  A capture allocates nothing when qfec_reserve
 * covered its batch; a workspace outgrown by a later capture stays allocated until the
 * context is destroyed, so earlier graphs stay valid.  Independent contexts (one per
 * stream, or one per device) share nothing and run concurrently.  Calls on one context are
 * serialised on the host by a mutex (the reference codec is single-threaded per
 * connection).
 * ------------------------------------------------------------------------------- */
typedef struct qfec_ctx qfec_ctx;

QFEC_API int qfec_ctx_create(int device, qfec_ctx **out);
QFEC_API void qfec_ctx_destroy(qfec_ctx *ctx);
/* Launch-shape options of one context (the defaults are the measured best):
 * "xor_slots" 2..4, "xor_waves" 1..4, "dma" 0/1, "stream" 0/1, "stream_ring" 4..36,
 * "stream_grid" 0.., "const_enc" 0/1, "stream_static" 0/1 (gf_ring encodes), "ring_wide" 0/1
 * (their wide parity stores), "dcol" 0/1, "dcol_grid" 0.., "dcol_depth" 6/8, "bsyn" 0/1,
 * "bsyn_depth" 3/5/7, "psyn" 0/1, "psyn_wide" 0..2 (wide recovered-block stores: none,
 * (10, 10), every code), "pd" 1..3, "flat" 0/1, "enc_rc" 2/4/8, "prep_lane" 0/1,
 * "host_chunk_mb" 1..4096, "host_min_groups" 1.., "ring_split" 0/1 ((10, 20) encode in two
 * units), and the grid shares "ring_wg", "bsyn_wg", "stream_wg" (-1 = the measured choice),
 * "psyn_wg", "dcol_wg", "xor_wg" (groups per wave of an oversubscribed grid; 0 = the resident
 * persistent grid), "arr_optimistic" 0/1 (the arrival-order receiver's data
 * write during its open pass).  get also reads "cus" (compute units of the device).  -2 for an unknown name or a value out of range (also for the measured-and-removed
 * variants of earlier versions).  No environment variable changes what the library launches. */
QFEC_API int qfec_ctx_set_option(qfec_ctx *ctx, const char *name, int value);
QFEC_API int qfec_ctx_get_option(qfec_ctx *ctx, const char *name, int *value);
/* Pre-size every per-(k, m) table and both decode workspaces (eager and graph) for up to
 * `groups` groups so that later calls allocate nothing (call it before capturing calls
 * into a HIP graph). */
QFEC_API int qfec_reserve(qfec_ctx *ctx, int k, int m, int block_bytes, long long groups);

QFEC_API int qfec_encode_batch(qfec_ctx *ctx, int k, int m, int block_bytes, long long groups,
                      const unsigned char *d_data, unsigned char *d_parity, void *stream);

/* d_out may equal d_blocks (in place, the reference semantics) or be a separate
 * [G][k][bb] buffer that receives only the recovered blocks.  d_rows_out may equal
 * d_rows_in.  d_status may be NULL. */
QFEC_API int qfec_decode_batch(qfec_ctx *ctx, int k, int m, int block_bytes, long long groups,
                      const unsigned char *d_blocks, const unsigned char *d_rows_in,
                      unsigned char *d_out, unsigned char *d_rows_out, int *d_status,
                      void *stream);

/* Receiver-side decode, recovered-blocks layout.  Same per-group decode as
 * qfec_decode_batch, but d_blocks and d_rows_in are left untouched and only the recovered
 * blocks are written, densely: with rmax = min(k, m), recovered block j of group g goes to
 * d_rec + (g * rmax + j) * block_bytes and the data row it restores to
 * d_rec_rows[g * rmax + j] -- ascending, the order cauchy_256_decode assigns them
 * (cauchy_256.cpp:570-574) -- and 255 past the group's erasure count (the d_rec bytes of
 * such entries are unspecified).  This is what QuicFecGroup::getRevivedPackets consumes
 * (quic_fec_group.cc:280-293).  d_status may be NULL. */
QFEC_API int qfec_decode_batch_recovered(qfec_ctx *ctx, int k, int m, int block_bytes,
                                long long groups, const unsigned char *d_blocks,
                                const unsigned char *d_rows_in, unsigned char *d_rec,
                                unsigned char *d_rec_rows, int *d_status, void *stream);

/* Host-pointer variants: H2D, kernels, D2H, chunked and pipelined; synchronous (pass
 * pinned memory for full PCIe speed).  qfec_decode_batch_host works in place on h_blocks /
 * h_rows like cauchy_256_decode; qfec_decode_batch_recovered_host returns only the
 * recovered blocks, as qfec_decode_batch_recovered does. */
QFEC_API int qfec_encode_batch_host(qfec_ctx *ctx, int k, int m, int block_bytes, long long groups,
                           const unsigned char *h_data, unsigned char *h_parity);
QFEC_API int qfec_decode_batch_host(qfec_ctx *ctx, int k, int m, int block_bytes, long long groups,
                           unsigned char *h_blocks, unsigned char *h_rows, int *h_status);
QFEC_API int qfec_decode_batch_recovered_host(qfec_ctx *ctx, int k, int m, int block_bytes,
                                     long long groups, const unsigned char *h_blocks,
                                     const unsigned char *h_rows, unsigned char *h_rec,
                                     unsigned char *h_rec_rows, int *h_status);

/* ---------------------------------------------------------------------------------
 * Ragged batches: one launch over groups that share (k, m) but each carry their own
 * block_bytes (the group layer fixes block_bytes per group, quic_fec_group.cc:344-352; a
 * short group cannot be zero-padded to a common size, because the sub-row split bb/8 is part
 * of the code and parity is wire-visible).
 *
 * Packed layout: group g's k blocks are [k][bb[g]], contiguous, at base + off[g]; its outputs
 * are [m][bb[g]] (parity) or [min(k,m)][bb[g]] (recovered blocks) at their own base + off[g].
 * Offsets are byte offsets, multiples of 16, in explicit arrays; sizes are the int array
 * bb [G].  The base pointers must be 16-byte aligned.  Gaps between groups are allowed and
 * are never written.  rows [G][k], rec_rows [G][min(k,m)] and status [G] are dense as in the
 * uniform calls.
 *
 * Per-group semantics are exactly those of the uniform call with block_bytes = bb[g], i.e.
 * of cauchy_256_encode / cauchy_256_decode on that group: k <= 1 copies; m == 1 is XOR with
 * any bb >= 1; for m > 1 and bb[g] % 8 != 0 the group's status is -1 (on encode its first
 * parity block still receives the XOR parity, cauchy_256.cpp:1519-1534, and nothing else of
 * that group is written; on decode a group without a recovery block has status 0, :1287-1289);
 * a malformed receive set has status -3 and is left as it was.  rec_rows is 255 past a
 * group's erasure count and the rec bytes of such entries are not written.  Call-level
 * errors follow the uniform calls: with m > 1 and k + m > 256 the encode writes every
 * group's XOR parity and returns -1; a null pointer or groups < 0 returns -2.
 *
 * Workspace, streams, graphs: the device entry points only enqueue on `stream`; they never
 * read d_bb or the offsets back to the host, so a group with bb[g] < 1 is skipped by the
 * kernels rather than reported.  The ragged decode uses the same decode workspace, in the
 * same bracket, as the uniform decodes: everything the paragraph above says about streams,
 * contexts and captured graphs holds for it unchanged.  Its workspace does not depend on
 * the block sizes: qfec_reserve(ctx, k, m, any block_bytes, groups) covers a capture of up
 * to `groups` groups (pass the largest bb; the reserve also loads the encode table of the
 * ragged encode).  In-place and slot-layout ragged decodes do not exist; the recovered layout
 * is what the group layer consumes.
 * ------------------------------------------------------------------------------- */
/* Host helper, no GPU: fills data_off / par_off / rec_off [G] (any may be NULL) with each
 * group's offset in a buffer that packs the groups in order, every group rounded up to 16
 * bytes: k, m and min(k, m) blocks of bb[g] bytes per group.  totals (may be NULL) receives
 * the three buffer sizes (multiples of 16).  -2 on bb[g] < 1, a bad k / m / groups or
 * overflow. */
QFEC_API int qfec_ragged_layout(int k, int m, long long groups, const int *bb,
                                long long *data_off, long long *par_off, long long *rec_off,
                                long long totals[3]);

/* d_parity + d_par_off[g] receives [m][bb[g]].  d_status [G] may be NULL. */
QFEC_API int qfec_encode_batch_ragged(qfec_ctx *ctx, int k, int m, long long groups,
                                      const int *d_bb, const unsigned char *d_data,
                                      const long long *d_data_off, unsigned char *d_parity,
                                      const long long *d_par_off, int *d_status, void *stream);

/* As qfec_decode_batch_recovered: d_blocks and d_rows_in [G][k] are left untouched; recovered
 * block j of group g goes to d_rec + d_rec_off[g] + j * bb[g] and its data row to
 * d_rec_rows[g * min(k,m) + j] (ascending; 255 past the count).  d_status may be NULL. */
QFEC_API int qfec_decode_batch_ragged_recovered(qfec_ctx *ctx, int k, int m, long long groups,
                                                const int *d_bb, const unsigned char *d_blocks,
                                                const long long *d_blocks_off,
                                                const unsigned char *d_rows_in,
                                                unsigned char *d_rec, const long long *d_rec_off,
                                                unsigned char *d_rec_rows, int *d_status,
                                                void *stream);

/* Host-pointer variants: the same arguments in host memory; synchronous; chunked and
 * pipelined like the other host batches.  Chunks are cut on group boundaries by bytes (the
 * "host_chunk_mb" option; "host_min_groups" does not apply, a chunk holds at least one group).
 * The offsets must be ascending and the groups must not overlap (-2 otherwise, and for
 * bb[g] < 1 or an offset that is not a multiple of 16); qfec_ragged_layout produces such
 * offsets.  Bytes of the output buffer the call does not write keep the caller's values. */
QFEC_API int qfec_encode_batch_ragged_host(qfec_ctx *ctx, int k, int m, long long groups,
                                           const int *h_bb, const unsigned char *h_data,
                                           const long long *h_data_off, unsigned char *h_parity,
                                           const long long *h_par_off, int *h_status);
QFEC_API int qfec_decode_batch_ragged_recovered_host(qfec_ctx *ctx, int k, int m,
                                                     long long groups, const int *h_bb,
                                                     const unsigned char *h_blocks,
                                                     const long long *h_blocks_off,
                                                     const unsigned char *h_rows,
                                                     unsigned char *h_rec,
                                                     const long long *h_rec_off,
                                                     unsigned char *h_rec_rows, int *h_status);

/* ---------------------------------------------------------------------------------
 * Mixed-code batches: one launch over groups that each carry their own (k, m) as well as
 * their own block_bytes.  The reference gives every FEC group a configuration of its own
 * (quic_fec_group.cc:84-96) and an adaptive sender changes it with the measured loss
 * (quic_connection.cc:822-966), so one connection produces groups of several codes back to
 * back and a server holds all presets at once.
 *
 * Code set: qfec_codeset_create builds, once, what the kernels need per code (encode table,
 * encode matrix, chunk counts) for up to 32 codes (the wire has five configuration bits).
 * Each (k, m) is whatever qfec_encode_batch_ragged accepts at call level, k <= 1, m == 1 and
 * k + m > 256 included; duplicates are allowed; anything else (ncodes outside 1..32, a NULL
 * array, k < 1, k > 255, m < 1) is -2.  A set belongs to its context and is immutable, so a
 * captured call stays valid; destroy it before the context.  qfec_codeset_dims gives
 * kmax = max k, mmax = max m and rmax = max over codes of min(k, m).
 *
 * Layout: code [G] is a u8 device array, the group's index into the set.  bb [G] and the
 * packed layout are those of the ragged calls with the group's own counts: group g's k_g
 * blocks are [k_g][bb[g]] at base + off[g]; its outputs are [m_g][bb[g]] (parity) or
 * [min(k_g, m_g)][bb[g]] (recovered blocks).  Offsets are multiples of 16, the base pointers
 * are 16-byte aligned, gaps are never written.  rows is [G][kmax]: only the first k_g tags of
 * a row are read.  rec_rows is [G][rmax]: every entry at or past the group's erasure count
 * is 255, up to the set's rmax, so a caller scans it uniformly.  status is [G], may be NULL.
 *
 * Per-group semantics are exactly those of qfec_encode_batch_ragged /
 * qfec_decode_batch_ragged_recovered with that group's (k, m) and bb: k <= 1 copies; m == 1
 * is XOR with any bb >= 1; for m > 1 with bb[g] % 8 != 0 or k + m > 256 the encode gives
 * status -1 with the XOR parity in the first parity block and nothing else written, and the
 * decode follows cauchy_256.cpp:1287-1294 (status 0 without a recovery block, else -1); a
 * malformed receive set has status -3 and is left as it was; a group with bb[g] < 1 is
 * skipped.  A group whose code[g] >= ncodes has status -2 and none of its blocks, rows or
 * outputs is read or written (its rec_rows entries are 255).  Because rejection is per
 * group, the call itself returns 0 in all these cases.
 *
 * Call-level -2, before anything is enqueued: a NULL context, set or array (status excepted),
 * a set of another context, groups < 0, a base pointer that is not 16-byte aligned, and more
 * than 2^31 - 1 (group, output chunk) units (groups x the largest chunk count of a code, in
 * chunks of at most 4 outputs).
 *
 * Enqueue only: the device calls never read code, bb or the offsets back; the kernels read
 * the arrays when they run.  A captured call may therefore be replayed after code, bb,
 * offsets, rows and data were rewritten in place.  The decode uses the decode workspace in
 * the same bracket as every decode; qfec_codeset_reserve(cs, groups) sizes both workspaces,
 * eager and graph, for `groups` groups of the set, so a capture then allocates nothing.
 *
 * Bucket or mix: bucket by (k, m) whenever a bucket fills the device
 * (thousands of groups per code): the per-code calls are then faster in kernel time.  Mix when
 * the traffic spreads a flush of about a thousand groups or fewer over several codes.
 * ------------------------------------------------------------------------------- */
typedef struct qfec_codeset qfec_codeset;
QFEC_API int qfec_codeset_create(qfec_ctx *ctx, int ncodes, const int *k, const int *m,
                                 qfec_codeset **out);
QFEC_API void qfec_codeset_destroy(qfec_codeset *cs);
/* rmax = max over codes of min(k, m); any of the three may be NULL */
QFEC_API int qfec_codeset_dims(const qfec_codeset *cs, int *kmax, int *mmax, int *rmax);
QFEC_API int qfec_codeset_reserve(qfec_codeset *cs, long long groups);

/* Host helper, no GPU: qfec_ragged_layout with the block counts of code[g]: k_g, m_g and
 * min(k_g, m_g) blocks of bb[g] bytes per group, every group rounded up to 16 bytes.  Any of
 * the offset arrays and totals may be NULL.  -2 on code[g] >= ncodes, bb[g] < 1, ncodes
 * outside 1..32, a bad k / m / groups or overflow. */
QFEC_API int qfec_mixed_layout(int ncodes, const int *k, const int *m, long long groups,
                               const unsigned char *code, const int *bb, long long *data_off,
                               long long *par_off, long long *rec_off, long long totals[3]);

/* d_parity + d_par_off[g] receives [m_g][bb[g]].  d_status [G] may be NULL. */
QFEC_API int qfec_encode_batch_mixed(qfec_ctx *ctx, const qfec_codeset *cs, long long groups,
                                     const unsigned char *d_code, const int *d_bb,
                                     const unsigned char *d_data, const long long *d_data_off,
                                     unsigned char *d_parity, const long long *d_par_off,
                                     int *d_status, void *stream);

/* As qfec_decode_batch_ragged_recovered: d_blocks and d_rows_in [G][kmax] are left untouched;
 * recovered block j of group g goes to d_rec + d_rec_off[g] + j * bb[g] and its data row to
 * d_rec_rows[g * rmax + j] (ascending; 255 past the count). */
QFEC_API int qfec_decode_batch_mixed_recovered(qfec_ctx *ctx, const qfec_codeset *cs,
                                               long long groups, const unsigned char *d_code,
                                               const int *d_bb, const unsigned char *d_blocks,
                                               const long long *d_blocks_off,
                                               const unsigned char *d_rows_in,
                                               unsigned char *d_rec, const long long *d_rec_off,
                                               unsigned char *d_rec_rows, int *d_status,
                                               void *stream);

/* Host-pointer variants: the same arguments in host memory; synchronous; chunked and pipelined
 * like qfec_*_batch_ragged*_host, with the block count of each group's own code.  Chunks are cut
 * on group boundaries by bytes ("host_chunk_mb").  The same offset checks apply: ascending,
 * non-overlapping, multiples of 16 (-2 otherwise, and for bb[g] < 1); qfec_mixed_layout
 * produces such offsets.  A group whose code[g] >= ncodes stages nothing and has status -2.
 * Bytes of the output buffer the call does not write keep the caller's values. */
QFEC_API int qfec_encode_batch_mixed_host(qfec_ctx *ctx, const qfec_codeset *cs, long long groups,
                                          const unsigned char *h_code, const int *h_bb,
                                          const unsigned char *h_data,
                                          const long long *h_data_off, unsigned char *h_parity,
                                          const long long *h_par_off, int *h_status);
QFEC_API int qfec_decode_batch_mixed_recovered_host(qfec_ctx *ctx, const qfec_codeset *cs,
                                                    long long groups, const unsigned char *h_code,
                                                    const int *h_bb, const unsigned char *h_blocks,
                                                    const long long *h_blocks_off,
                                                    const unsigned char *h_rows,
                                                    unsigned char *h_rec,
                                                    const long long *h_rec_off,
                                                    unsigned char *h_rec_rows, int *h_status);

/* ---------------------------------------------------------------------------------
 * Pointer-table batches: encode and decode blocks where they lie.  The batched form of the
 * drop-in ABI's one pointer per block (cauchy_256_encode's data_ptrs[], cauchy_256_decode's
 * Block{data,row}[]): the k blocks of a group may lie in k unrelated device buffers (mbufs of a
 * device mempool, ring slots of different sizes, blocks shared between groups), and nothing is
 * packed first.
 *
 * Tables: d_data_ptrs / d_block_ptrs [G*k], d_parity_ptrs [G*m] and d_rec_ptrs [G*min(k,m)] are
 * device arrays of device addresses; entry g*k + pos names block pos of group g (the index is
 * 64-bit).  d_bb [G] is the block size per group, or NULL: every group has bb_all.  rows
 * [G][k], rec_rows [G][min(k,m)] and status [G] are dense as in the uniform calls.
 *
 * Per-group semantics are exactly those of qfec_encode_batch_ragged /
 * qfec_decode_batch_ragged_recovered with block_bytes = bb[g]: k <= 1 copies; m == 1 is XOR
 * with any bb >= 1; for m > 1 and bb[g] % 8 != 0 the status is -1 (the encode writes the XOR
 * parity to the group's first parity block only); a malformed receive set has status -3;
 * rec_rows is 255 past a group's erasure count; with m > 1 and k + m > 256 the encode writes
 * every group's XOR parity to its first parity block and returns -1.
 *
 * Entries that are never dereferenced (a caller may leave anything in them): every entry of a
 * group with bb[g] < 1; parity entries 1 .. m-1 of a group the encode rejects; d_rec_ptrs
 * entries at or past the group's erasure count; every d_rec_ptrs entry of a group with a
 * negative status.
 *
 * Every other entry must be a valid device address of bb[g] bytes.  The library cannot check
 * this and does not try (as the pointer arrays of batched BLAS): a wrong entry is a wild read
 * or write on the device, not an error code.
 *
 * Alignment: a block may start at any address; the result is the same bytes.  No byte outside
 * [ptr, ptr + bb[g]) of any block is read or written.
 *
 * Overlap: input blocks may overlap or be shared between groups.  Output blocks must be
 * distinct from each other and must not overlap any input block of the batch.  In-place decode
 * is not offered (the apply works in output chunks that each re-read the inputs).
 *
 * Call-level -2, before anything is enqueued: the ragged calls' limits (k, m, groups < 0, a
 * null context), a NULL table, d_bb == NULL with bb_all < 1, a null d_rows_in / d_rec_rows, and
 * for m > 1 more than 2^31 - 1 (group, output chunk) units (chunks of at most 4 outputs).
 *
 * Streams, graphs: the calls only enqueue on `stream` and read no device array back.  The
 * decode uses the decode workspace in the same bracket as every decode;
 * qfec_reserve(ctx, k, m, any block_bytes, groups) covers a capture.  A captured call reads the
 * tables when it runs: it may be replayed after the caller rewrote them in place.
 * ------------------------------------------------------------------------------- */
/* Parity block y of group g is written at d_parity_ptrs[g*m + y].  d_status [G] may be NULL. */
QFEC_API int qfec_encode_batch_ptrs(qfec_ctx *ctx, int k, int m, long long groups,
                                    const int *d_bb, int bb_all,
                                    const unsigned char *const *d_data_ptrs,
                                    unsigned char *const *d_parity_ptrs, int *d_status,
                                    void *stream);

/* Recovered-blocks layout: recovered block j of group g is written at
 * d_rec_ptrs[g*min(k,m) + j], its data row to d_rec_rows[g*min(k,m) + j] (ascending; 255 past
 * the count).  The blocks and d_rows_in [G][k] are left untouched.  d_status may be NULL. */
QFEC_API int qfec_decode_batch_ptrs_recovered(qfec_ctx *ctx, int k, int m, long long groups,
                                              const int *d_bb, int bb_all,
                                              const unsigned char *const *d_block_ptrs,
                                              const unsigned char *d_rows_in,
                                              unsigned char *const *d_rec_ptrs,
                                              unsigned char *d_rec_rows, int *d_status,
                                              void *stream);

/* ---------------------------------------------------------------------------------
 * Packet protection next to the FEC path (SURVEY.md §8 f, rank 4).
 *
 * The reference encrypts every packet after serialisation -- the FEC packets right after
 * the encode (QuicPacketCreator::SerializeFec -> QuicFramer::EncryptInPlace,
 * quic_packet_creator.cc:948-953, quic_framer.cc:1921-1939) -- and decrypts before the
 * group sees a packet (quic_framer.cc:657).  In this fork QuicEncrypter::Create yields
 * NullEncrypter for kNULL and an identity copy for every negotiated AEAD
 * (crypto/quic_encrypter.cc:18-29), so NullEncrypter is the packet protection with
 * arithmetic: tag12 = low 12 bytes of FNV-1a-128(AD || PT) (null_encrypter.cc:23-43,
 * quic_utils.cc:38-56,110-125,175-181).
 *
 * Batches of n packets, all device pointers.  Per-packet lengths come from the int32 arrays,
 * or, where an array is NULL, from the `_all` scalar.  d_out and out_stride must be 4-byte
 * aligned.  d_out_len[i] = bytes written for packet i, or -1 where the reference returns
 * false.  A length larger than its row's stride is rejected (-1, nothing written); a stride
 * of 0 (every packet reads the same row) is not checked.
 * ------------------------------------------------------------------------------- */
/* NullEncrypter::EncryptPacket in the EncryptInPlace layout: packet i is
 * AD_i || tag12 || PT_i at d_out + i*out_stride (AD_i at d_ad + i*ad_stride, PT_i at
 * d_pt + i*pt_stride).  -1 (nothing written) when it does not fit in out_stride. */
QFEC_API int qfec_null_seal_batch(qfec_ctx *ctx, long long n, const unsigned char *d_ad,
                                  long long ad_stride, const int *d_ad_len, int ad_len_all,
                                  const unsigned char *d_pt, long long pt_stride,
                                  const int *d_pt_len, int pt_len_all, unsigned char *d_out,
                                  long long out_stride, int *d_out_len, void *stream);
/* NullDecrypter::DecryptPacket: wire packet i at d_pkt + i*pkt_stride (pkt_len bytes, the
 * first ad_len of them the associated data).  The output first receives the ciphertext, as
 * in the reference.  Accepted: the plaintext overwrites its start (the last 12 ciphertext
 * bytes stay behind it) and d_out_len[i] is the plaintext length.  Rejected (ciphertext
 * shorter than 12 bytes or tag mismatch): -1, the output holds the ciphertext copy; -1 with
 * nothing written when the ciphertext exceeds out_stride. */
QFEC_API int qfec_null_open_batch(qfec_ctx *ctx, long long n, const unsigned char *d_pkt,
                                  long long pkt_stride, const int *d_pkt_len, int pkt_len_all,
                                  const int *d_ad_len, int ad_len_all, unsigned char *d_out,
                                  long long out_stride, int *d_out_len, void *stream);
/* Sender side of SerializeFec (quic_packet_creator.cc:935-957): encode the groups into
 * d_parity [G][m][bb] (qfec_encode_batch), then seal parity block (g, i) as FEC packet
 * g*m + i with header g*m + i (d_hdr + (g*m+i)*hdr_stride) as the associated data:
 * d_pkt + (g*m+i)*pkt_stride = header || tag12 || parity.  One call, two launches on one
 * stream; the parity does not leave the device. */
QFEC_API int qfec_encode_seal_batch(qfec_ctx *ctx, int k, int m, int block_bytes,
                                    long long groups, const unsigned char *d_data,
                                    unsigned char *d_parity, const unsigned char *d_hdr,
                                    long long hdr_stride, const int *d_hdr_len, int hdr_len_all,
                                    unsigned char *d_pkt, long long pkt_stride, int *d_pkt_len,
                                    void *stream);

/* Every packet of each group in one launch: the reference seals each data packet
 * (quic_packet_creator.cc:733-736) as well as each FEC packet (:948-953).  Packet
 * p = g*(k+m) + i is sealed with header row p (d_hdr + p*hdr_stride, d_hdr_len[p] or
 * hdr_len_all bytes) as the associated data and, as plaintext, data block (g, i) of d_data
 * [G][k][bb] for i < k or parity block (g, i-k) of d_parity [G][m][bb] otherwise, its first
 * d_pt_len[p] (or pt_len_all <= bb) bytes: d_pkt + p*pkt_stride = header || tag12 || PT,
 * d_pkt_len[p] as in qfec_null_seal_batch.  k + m <= 256. */
QFEC_API int qfec_seal_groups_batch(qfec_ctx *ctx, int k, int m, int block_bytes,
                                    long long groups, const unsigned char *d_data,
                                    const unsigned char *d_parity, const unsigned char *d_hdr,
                                    long long hdr_stride, const int *d_hdr_len, int hdr_len_all,
                                    const int *d_pt_len, int pt_len_all, unsigned char *d_pkt,
                                    long long pkt_stride, int *d_pkt_len, void *stream);
/* qfec_encode_batch into d_parity, then qfec_seal_groups_batch: one call, two launches. */
QFEC_API int qfec_encode_seal_groups_batch(qfec_ctx *ctx, int k, int m, int block_bytes,
                                           long long groups, const unsigned char *d_data,
                                           unsigned char *d_parity, const unsigned char *d_hdr,
                                           long long hdr_stride, const int *d_hdr_len,
                                           int hdr_len_all, const int *d_pt_len, int pt_len_all,
                                           unsigned char *d_pkt, long long pkt_stride,
                                           int *d_pkt_len, void *stream);
/* Receiver side: NullDecrypter::DecryptPacket on every packet of each group (the framer
 * decrypts before the group sees a packet, quic_framer.cc:657), then the group decode.
 * Wire packet p = g*(k+m) + i at d_pkt + p*pkt_stride, d_pkt_len[p] bytes (< 0: not
 * received), the first d_ad_len[p] (or ad_len_all) of them the associated data.
 *   d_open_len [G][k+m]  plaintext bytes of packet p, or -1 (not received, malformed,
 *                        plaintext longer than bb, or tag mismatch)
 *   d_blocks [G][k][bb]  data packet i's plaintext, zero-padded, in slot i; each slot whose
 *                        data packet did not open holds the plaintext of the next opened FEC
 *                        packet (ascending)
 *   d_rows [G][k]        the row tag of each slot (i, or k + j for FEC packet j; 255 when no
 *                        opened FEC packet is left, and the group's status is then -3; the
 *                        bytes of a slot tagged 255 are unspecified)
 * followed by qfec_decode_batch_recovered(d_blocks, d_rows) into d_rec / d_rec_rows /
 * d_status (a group with an unfilled slot: status -3, recovered rows all 255).  Four
 * launches on one stream.  k + m <= 255. */
QFEC_API int qfec_open_decode_batch(qfec_ctx *ctx, int k, int m, int block_bytes,
                                    long long groups, const unsigned char *d_pkt,
                                    long long pkt_stride, const int *d_pkt_len,
                                    const int *d_ad_len, int ad_len_all, unsigned char *d_blocks,
                                    unsigned char *d_rows, int *d_open_len, unsigned char *d_rec,
                                    unsigned char *d_rec_rows, int *d_status, void *stream);

/* Host-pointer variants of the two protected paths: the sender's and the receiver's per-packet
 * work starting and ending in host memory (packets off and onto a socket), chunked and
 * pipelined like qfec_*_batch_host (H2D, kernels and D2H of successive chunks overlap);
 * synchronous; pass pinned memory for full PCIe speed.  Lengths, headers and packets are
 * indexed by packet p = g*(k+m) + i as in the device calls; h_hdr may be NULL (no associated
 * data: h_hdr_len NULL and hdr_len_all 0); h_pkt_len, h_pt_len and h_ad_len are int32 host
 * arrays (NULL where the `_all` scalar applies, except h_pkt_len).  Row strides must be > 0.
 *   qfec_encode_seal_groups_batch_host: data [G][k][bb] -> every packet of each group sealed,
 *     h_pkt [G*(k+m)][pkt_stride], h_pkt_len [G*(k+m)] (qfec_encode_seal_groups_batch); the
 *     bytes of a packet row past h_pkt_len[p] are zero (rows are copied back whole); -1 with
 *     nothing written where the encode returns -1 (m > 1, k > 1 and (k + m > 256 or
 *     block_bytes % 8 != 0));
 *   qfec_open_decode_batch_host: wire packets -> h_rec [G][min(k,m)][bb], h_rec_rows,
 *     h_status [G] (may be NULL) and h_open_len [G*(k+m)] (may be NULL)
 *     (qfec_open_decode_batch). */
QFEC_API int qfec_encode_seal_groups_batch_host(qfec_ctx *ctx, int k, int m, int block_bytes,
                                                long long groups, const unsigned char *h_data,
                                                const unsigned char *h_hdr, long long hdr_stride,
                                                const int *h_hdr_len, int hdr_len_all,
                                                const int *h_pt_len, int pt_len_all,
                                                unsigned char *h_pkt, long long pkt_stride,
                                                int *h_pkt_len);
QFEC_API int qfec_open_decode_batch_host(qfec_ctx *ctx, int k, int m, int block_bytes,
                                         long long groups, const unsigned char *h_pkt,
                                         long long pkt_stride, const int *h_pkt_len,
                                         const int *h_ad_len, int ad_len_all,
                                         unsigned char *h_rec, unsigned char *h_rec_rows,
                                         int *h_status, int *h_open_len);

/* ---------------------------------------------------------------------------------
 * Ragged packet protection: the protected paths above over ragged batches, a block size per
 * group.  Real groups do not share a block_bytes, so a sender or receiver would otherwise make
 * one protected call per distinct size, or run the ragged codec and the per-packet seal / open
 * separately and place the plaintexts by hand.
 *
 * Rule: per group, a ragged call does what the uniform call with block_bytes = bb[g] does to
 * that group.  Only the blocks are packed (the layout of the ragged batches above: group g's
 * blocks [n][bb[g]] at base + off[g], offsets multiples of 16, base pointers 16-byte aligned,
 * gaps never written).  Headers, packets and every per-packet array stay dense by packet
 * index p = g*(k+m) + i with one stride, rows [G][k], rec_rows [G][min(k,m)] and status [G]
 * stay dense, as in the uniform calls.  What the rule fixes:
 *   - d_pt_len == NULL: every packet's plaintext is its whole block, bb[g] bytes (there is no
 *     pt_len_all: no one length fits every group).
 *   - d_pt_len[p] > bb[g] rejects packet p: d_pkt_len[p] = -1 and nothing is written, as a
 *     length beyond its row is rejected by the uniform seal.
 *   - encode + seal, a group whose encode status is -1 (m > 1, k > 1 and bb[g] % 8 != 0; one
 *     predicate asked by the encode and by the seal): none of its k + m packets is sealed,
 *     all of its d_pkt_len entries are -1, its d_status is -1, and its first parity block
 *     holds the XOR parity, exactly as qfec_encode_batch_ragged leaves it.  Every other
 *     group's d_status is 0.  The call itself returns 0.
 *   - bb[g] < 1: the device calls never read d_bb back, so the group is skipped by the
 *     kernels: its packets get d_pkt_len -1 on the seals and d_open_len -1 on the open, and
 *     on the open its rows are 255, its status is -3 and its rec_rows are 255.  Nothing of it
 *     is written and its neighbours are unaffected.  (The host forms read h_bb and return -2.)
 *   - open -> decode: a packet whose plaintext is longer than bb[g] is rejected
 *     (d_open_len -1); the destination of slot s is d_blocks + d_blocks_off[g] + s*bb[g],
 *     zero-padded to bb[g].  A slot tagged 255 is not written, unless a packet that passed
 *     the length checks and then failed its tag had been streamed into it (the open writes
 *     before the tag is known, as in the uniform call: those bytes are unspecified).  The
 *     decode is
 *     qfec_decode_batch_ragged_recovered on what the open placed, and all its per-group
 *     statuses carry over: -1 for m > 1 with bb[g] % 8 != 0 and a recovery block, -3 for a
 *     malformed set (an unfilled slot included).
 *     bb[g] is the caller's.  A receiver takes it from the plaintext length of the group's
 *     FEC packets (an FEC packet's plaintext is a whole block); the reference sizes a group's
 *     recovery by the largest packet it stored (quic_fec_group.cc:264-265).
 *   - call-level limits, -2 before anything is enqueued: k + m > 256 on the seals, k + m > 255
 *     on the open, groups < 0, a null buffer (d_hdr, d_hdr_len, d_pt_len, d_ad_len and d_status
 *     may be NULL as in the uniform calls), a base pointer that is not 16-byte aligned, and on
 *     the seals a d_pkt or pkt_stride that is not 4-byte aligned.
 *   - workspace, streams, graphs: the seals use no workspace; the open -> decode runs in the
 *     decode-workspace bracket like every decode, so everything said above about streams,
 *     contexts and captured graphs holds unchanged, and qfec_reserve(ctx, k, m, largest bb,
 *     groups) covers a capture as it does for qfec_decode_batch_ragged_recovered.
 * Launches: qfec_seal_groups_batch_ragged one; qfec_encode_seal_groups_batch_ragged the
 * ragged encode's and one; qfec_open_decode_batch_ragged two, the ragged decode's, and one.
 * ------------------------------------------------------------------------------- */
/* qfec_seal_groups_batch per group: packet p's plaintext is block i of d_data + d_data_off[g]
 * ([k][bb[g]]) for i < k, block i-k of d_parity + d_par_off[g] ([m][bb[g]]) otherwise. */
QFEC_API int qfec_seal_groups_batch_ragged(qfec_ctx *ctx, int k, int m, long long groups,
                                           const int *d_bb, const unsigned char *d_data,
                                           const long long *d_data_off,
                                           const unsigned char *d_parity,
                                           const long long *d_par_off,
                                           const unsigned char *d_hdr, long long hdr_stride,
                                           const int *d_hdr_len, int hdr_len_all,
                                           const int *d_pt_len, unsigned char *d_pkt,
                                           long long pkt_stride, int *d_pkt_len, void *stream);
/* qfec_encode_batch_ragged into d_parity (d_status [G], may be NULL), then the seal above. */
QFEC_API int qfec_encode_seal_groups_batch_ragged(qfec_ctx *ctx, int k, int m, long long groups,
                                                  const int *d_bb, const unsigned char *d_data,
                                                  const long long *d_data_off,
                                                  unsigned char *d_parity,
                                                  const long long *d_par_off,
                                                  const unsigned char *d_hdr,
                                                  long long hdr_stride, const int *d_hdr_len,
                                                  int hdr_len_all, const int *d_pt_len,
                                                  unsigned char *d_pkt, long long pkt_stride,
                                                  int *d_pkt_len, int *d_status, void *stream);
/* qfec_open_decode_batch per group: d_blocks + d_blocks_off[g] receives [k][bb[g]], d_rec +
 * d_rec_off[g] up to [min(k,m)][bb[g]]; d_rows, d_open_len, d_rec_rows, d_status as there. */
QFEC_API int qfec_open_decode_batch_ragged(qfec_ctx *ctx, int k, int m, long long groups,
                                           const int *d_bb, const unsigned char *d_pkt,
                                           long long pkt_stride, const int *d_pkt_len,
                                           const int *d_ad_len, int ad_len_all,
                                           unsigned char *d_blocks,
                                           const long long *d_blocks_off, unsigned char *d_rows,
                                           int *d_open_len, unsigned char *d_rec,
                                           const long long *d_rec_off, unsigned char *d_rec_rows,
                                           int *d_status, void *stream);
/* Host-pointer variants: synchronous; chunked and pipelined like qfec_*_batch_ragged*_host
 * (chunks cut on group boundaries by bytes, the "host_chunk_mb" option; offsets ascending,
 * non-overlapping multiples of 16 and bb[g] >= 1, -2 otherwise).  Row strides must be > 0.
 *   qfec_encode_seal_groups_batch_ragged_host: the parity is laid out on the device and never
 *     leaves it.  h_pkt rows come back whole, with zeros past h_pkt_len[p] and in rejected
 *     rows (the uniform host seal's contract); h_status [G] (may be NULL) is the encode's.
 *   qfec_open_decode_batch_ragged_host: takes h_bb and h_rec_off only and lays the blocks out
 *     itself.  h_rec bytes the call does not write keep the caller's values (the ragged host
 *     decode's contract); h_status and h_open_len may be NULL. */
QFEC_API int qfec_encode_seal_groups_batch_ragged_host(
    qfec_ctx *ctx, int k, int m, long long groups, const int *h_bb, const unsigned char *h_data,
    const long long *h_data_off, const unsigned char *h_hdr, long long hdr_stride,
    const int *h_hdr_len, int hdr_len_all, const int *h_pt_len, unsigned char *h_pkt,
    long long pkt_stride, int *h_pkt_len, int *h_status);
QFEC_API int qfec_open_decode_batch_ragged_host(
    qfec_ctx *ctx, int k, int m, long long groups, const int *h_bb, const unsigned char *h_pkt,
    long long pkt_stride, const int *h_pkt_len, const int *h_ad_len, int ad_len_all,
    unsigned char *h_rec, const long long *h_rec_off, unsigned char *h_rec_rows, int *h_status,
    int *h_open_len);

/* ---------------------------------------------------------------------------------
 * Framed groups: QuicFecGroup's wire format on the device.
 *
 * The group layer protects the block prefix || payload || zeros, prefix = the 16-bit
 * little-endian (len | pn_len << 14) & 0xffff (quic_fec_group.cc:109-121), padded to
 * bb = roundup8(max(len + 2)) (:344-352).  On the wire a data packet carries the payload alone;
 * only FEC packets carry whole blocks.  The receiver prefixes each opened data packet again
 * (:178-183) and cuts each revived packet out of its block by that prefix (:287-292).  The ragged
 * protected calls above treat a data packet's plaintext as its block, so they are
 * wire-compatible with the reference only for callers who frame the blocks themselves.  The
 * calls here do the framing: payload rows in, wire packets out; wire packets in, revived
 * payloads out.  Ragged only (a framed group has its own bb by construction).
 *
 * Rule: per group, a framed call is the ragged protected call on the framed blocks.  Blocks are
 * packed as in the ragged batches; payload rows (d_pay + (g*k+i)*pay_stride, d_pay_len[g*k+i]
 * bytes), revived rows (d_rev + (g*rmax+j)*rev_stride, rmax = min(k,m)), headers, packets and
 * every per-packet array stay dense.  pn_len is the QuicPacketNumberLength value (1, 2, 4, 6):
 * u8 per packet (d_pn_len [G*k] on the sender, [G*(k+m)] on the receiver), or, where the array
 * is NULL, pn_len_all; the prefix keeps its low two bits (4 -> 0, 6 -> 2, as in the reference).
 * What the rule fixes:
 *   - sender: block (g, i) = prefix || payload || zeros to bb[g] bytes is written to
 *     d_data + d_data_off[g] + i*bb[g] (d_data is an output), the groups are encoded, data packet
 *     p = g*(k+m)+i is header || tag12 || payload (no prefix), FEC packet p is
 *     header || tag12 || parity block i-k.
 *   - a group is rejected when any of its k lengths is < 0, > 0x3fff, > pay_stride (pay_stride
 *     != 0) or > bb[g] - 2, or when bb[g] < 8 (one predicate asked by the frame, the seal and the
 *     status): d_status[g] = -3, all k + m d_pkt_len entries -1, and none of its blocks, parity
 *     or packets is written.
 *   - a group that frames but whose encode status is -1 (m > 1, k > 1, bb[g] % 8 != 0): its
 *     blocks are framed, and the rest is as in qfec_encode_seal_groups_batch_ragged (XOR parity
 *     in its first parity block, no packet sealed, d_status -1).
 *   - receiver: a data packet's plaintext goes to slot + 2, zero-padded to bb[g] - 2, behind the
 *     prefix made of its opened length and pn_len[p]; it is rejected (d_open_len -1) when longer
 *     than bb[g] - 2.  An FEC packet's plaintext goes to slot + 0 and may be bb[g] long.
 *     Everything else (rows, holes, the decode, every status) is qfec_open_decode_batch_ragged's.
 *     bb[g] is the caller's: qfec_framed_rx_block_bytes gives the reference's value, which is
 *     not a multiple of 8 for a group that received no FEC packet (such a group decodes with
 *     status 0 only if it lost nothing).
 *   - revived packets: for recovered block j of group g with d_rec_rows != 255 and d_status[g]
 *     == 0, v = its prefix, len = min(v & 0x3fff, bb[g] - 2) (the reference reads past the block
 *     there; the clamp is include/quic_fec_group.h's), d_rev row g*rmax+j = block[2 .. 2+len),
 *     d_rev_len = len, d_rev_pn_len = v >> 14.  Bytes of the row past len are not written.
 *     Every other entry, and a len above rev_stride: d_rev_len -1 and nothing else written.
 *   - call-level limits, -2 before anything is enqueued: those of the ragged protected calls,
 *     and a NULL d_pay / d_pay_len / d_rev / d_rev_len or a negative pay_stride / rev_stride.
 *     d_pn_len, d_rev_pn_len, d_status may be NULL.  d_rev and rev_stride need no alignment.
 *   - workspace, streams, graphs: both paths run in the decode-workspace bracket (the sender
 *     keeps one int per group there); qfec_reserve(ctx, k, m, largest bb, groups) covers a
 *     capture.
 * Launches: sender one, the ragged encode's, one; receiver two, the ragged decode's, two.
 * ------------------------------------------------------------------------------- */
/* Host helper, no GPU: bb[g] = roundup8(max_i(pay_len[g*k+i] + 2)) (output), then the offsets
 * and totals of qfec_ragged_layout for those sizes.  -2 on a length outside [0, 0x3fff]. */
QFEC_API int qfec_framed_layout(int k, int m, long long groups, const int *pay_len, int *bb,
                                long long *data_off, long long *par_off, long long *rec_off,
                                long long totals[3]);
/* Host helper, no GPU: bb[g] = the largest stored size among group g's received packets
 * (pkt_len[p] >= 0 with at least 12 bytes behind the associated data): plaintext + 2 for a data
 * packet, plaintext for an FEC packet (quic_fec_group.cc:264-265).  Not rounded; 0 when nothing
 * was received.  ad_len may be NULL (ad_len_all). */
QFEC_API int qfec_framed_rx_block_bytes(int k, int m, long long groups, const int *pkt_len,
                                        const int *ad_len, int ad_len_all, int *bb);
/* The sender's framing alone (for a caller who runs the bare codec): blocks from payload rows.
 * d_status [G] (may be NULL): 0, or -3 for a rejected group. */
QFEC_API int qfec_frame_blocks_batch_ragged(qfec_ctx *ctx, int k, long long groups,
                                            const int *d_bb, const unsigned char *d_pay,
                                            long long pay_stride, const int *d_pay_len,
                                            const unsigned char *d_pn_len, int pn_len_all,
                                            unsigned char *d_data, const long long *d_data_off,
                                            int *d_status, void *stream);
/* The receiver's extraction alone, after a recovered-layout ragged decode. */
QFEC_API int qfec_extract_revived_batch_ragged(qfec_ctx *ctx, int k, int m, long long groups,
                                               const int *d_bb, const unsigned char *d_rec,
                                               const long long *d_rec_off,
                                               const unsigned char *d_rec_rows,
                                               const int *d_status, unsigned char *d_rev,
                                               long long rev_stride, int *d_rev_len,
                                               unsigned char *d_rev_pn_len, void *stream);
/* Sender: frame -> qfec_encode_batch_ragged -> seal of every packet. */
QFEC_API int qfec_frame_encode_seal_groups_batch_ragged(
    qfec_ctx *ctx, int k, int m, long long groups, const int *d_bb, unsigned char *d_data,
    const long long *d_data_off, unsigned char *d_parity, const long long *d_par_off,
    const unsigned char *d_hdr, long long hdr_stride, const int *d_hdr_len, int hdr_len_all,
    const unsigned char *d_pay, long long pay_stride, const int *d_pay_len,
    const unsigned char *d_pn_len, int pn_len_all, unsigned char *d_pkt, long long pkt_stride,
    int *d_pkt_len, int *d_status, void *stream);
/* Receiver: framed open -> qfec_decode_batch_ragged_recovered -> extraction. */
QFEC_API int qfec_open_decode_extract_batch_ragged(
    qfec_ctx *ctx, int k, int m, long long groups, const int *d_bb, const unsigned char *d_pkt,
    long long pkt_stride, const int *d_pkt_len, const int *d_ad_len, int ad_len_all,
    const unsigned char *d_pn_len, int pn_len_all, unsigned char *d_blocks,
    const long long *d_blocks_off, unsigned char *d_rows, int *d_open_len, unsigned char *d_rec,
    const long long *d_rec_off, unsigned char *d_rec_rows, int *d_status, unsigned char *d_rev,
    long long rev_stride, int *d_rev_len, unsigned char *d_rev_pn_len, void *stream);

/* ---------------------------------------------------------------------------------
 * Arrival-order receiver: the framed receiver over packets as the socket left them.
 *
 * qfec_open_decode_extract_batch_ragged wants packet p = g*(k+m)+i at row p of d_pkt.  A
 * receiver's ring holds its datagrams in arrival order instead: connections and groups
 * interleaved, with duplicates, packets of groups that already hold k, and packets of no FEC
 * group.  Which of them a group takes depends on which of them decrypt (quic_framer.cc:657, then
 * quic_fec_group.cc:167-169 and :210-213), so the caller cannot sort them beforehand.  The call
 * here reads the ring as it is: n packets, a (group, index) tag per packet, a block size per
 * group.
 *
 * Inputs: arrival a (0 <= a < n) is the wire packet at d_pkt + a*pkt_stride, d_pkt_len[a] bytes,
 * its first d_ad_len[a] (or ad_len_all) bytes the associated data, its packet-number length
 * d_pn_len[a] (or pn_len_all): these three arrays are per arrival here, not per slot.
 * d_arr_group[a] (int32) is the group's index in this batch (which (connection, fec_group) pair a
 * batch index stands for is the caller's bookkeeping); d_arr_index[a] (u8) is packet_number -
 * fec_group, the byte the private header carries (qfec_wire_read_private): below k data packet i,
 * from k to k+m-1 FEC packet i-k.
 *
 * Acceptance, defined sequentially over a = 0 .. n-1 (the device result equals it):
 *   1. group tag outside [0, groups) or index >= k+m: QFEC_ARR_IGNORED.
 *   2. the packet fails the framed open's length checks (d_pkt_len[a] in [0, pkt_stride], the AD
 *      length >= 0, at least 12 bytes behind the AD, a plaintext of at most bb[g]-2 bytes for a
 *      data packet and bb[g] for an FEC packet; none passes where bb[g] < 1) or its tag does not
 *      match: QFEC_ARR_REJECTED.  Such a packet never reaches its group.
 *   3. an earlier arrival with the same (g, i) opened: QFEC_ARR_DUPLICATE.  A rejected first
 *      copy does not stand in the way of a later good one.
 *   4. k distinct indices of group g opened earlier: QFEC_ARR_LATE.
 *   5. otherwise the arrival is accepted: d_arr_state[a] = its plaintext length (>= 0).
 * d_arr_state [n] (int32) may be NULL.
 *
 * Rule for everything else: per group, the call is qfec_open_decode_extract_batch_ragged on the
 * accepted packets placed at p = g*(k+m)+i: d_open_len[p] (the accepted packet's plaintext
 * length, else -1), the placed d_blocks slots with their prefixes, d_rows (the holes take the
 * accepted FEC packets, ascending), d_rec, d_rec_rows, d_status (-3 for a group with fewer than k
 * accepted, -1 for bb[g] % 8 != 0 with a recovery block), d_rev, d_rev_len, d_rev_pn_len.  A data
 * packet that arrives after the group's k-th is late and comes back revived, with the bytes it
 * was sent with.  The bytes that call leaves unspecified stay unspecified.
 * d_arr_at [groups*(k+m)] (int32, output): the arrival accepted for slot p, -1 without one; it
 * maps a slot back to its ring entry.  It and d_open_len are the call's only tables (no
 * workspace beyond the decode's).
 * bb[g] is the caller's; qfec_arrivals_rx_block_bytes gives the reference's value.
 *
 * Call-level limits, -2 before anything is enqueued: those of
 * qfec_open_decode_extract_batch_ragged; n < 0; n or groups*(k+m) above INT32_MAX (arrival
 * indices live in int32 tables); a NULL d_arr_group, d_arr_index or d_arr_at.  n == 0 is valid:
 * every group gets status -3, and the per-arrival arrays (d_pkt, d_pkt_len, d_arr_group,
 * d_arr_index), of which nothing is read then, may be NULL.
 * Streams, graphs: the call only enqueues work, reads no device array back and sets its table up
 * again inside every call, so a captured call can be replayed over new ring contents.  It runs in
 * the decode-workspace bracket like every decode; qfec_reserve(ctx, k, m, largest bb, groups)
 * covers a capture.
 * Launches: five (four without d_arr_state), the ragged decode's, two.
 * ------------------------------------------------------------------------------- */
#define QFEC_ARR_REJECTED (-1)
#define QFEC_ARR_IGNORED (-2)
#define QFEC_ARR_DUPLICATE (-3)
#define QFEC_ARR_LATE (-4)
/* Host helper, no GPU: bb[g] = the largest stored size (plaintext + 2 for a data packet, the
 * plaintext for an FEC packet, quic_fec_group.cc:264-265) among group g's first k distinct
 * arrivals; 0 where nothing arrived.  By lengths alone, like qfec_framed_rx_block_bytes: an
 * arrival counts with at least 12 bytes behind its associated data, only the first copy of an
 * index counts, and tags outside the batch are skipped.  ad_len may be NULL (ad_len_all).
 * -2: k + m > 255, n < 0, groups < 0, a NULL array. */
QFEC_API int qfec_arrivals_rx_block_bytes(int k, int m, long long groups, long long n,
                                          const int *arr_group, const unsigned char *arr_index,
                                          const int *pkt_len, const int *ad_len, int ad_len_all,
                                          int *bb);
/* Receiver over arrivals: open -> bind -> qfec_decode_batch_ragged_recovered -> extraction. */
QFEC_API int qfec_open_decode_extract_arrivals_ragged(
    qfec_ctx *ctx, int k, int m, long long groups, const int *d_bb, long long n,
    const unsigned char *d_pkt, long long pkt_stride, const int *d_pkt_len, const int *d_ad_len,
    int ad_len_all, const unsigned char *d_pn_len, int pn_len_all, const int *d_arr_group,
    const unsigned char *d_arr_index, int *d_arr_state, int *d_arr_at, unsigned char *d_blocks,
    const long long *d_blocks_off, unsigned char *d_rows, int *d_open_len, unsigned char *d_rec,
    const long long *d_rec_off, unsigned char *d_rec_rows, int *d_status, unsigned char *d_rev,
    long long rev_stride, int *d_rev_len, unsigned char *d_rev_pn_len, void *stream);

/* ---------------------------------------------------------------------------------
 * Mixed-code wire path: the framed sender and the arrival-order receiver with a (k, m) per group.
 *
 * One adaptive connection produces groups of several codes back to back, and the configuration
 * travels in every packet's private flags, so a receive ring holds arrivals of groups of
 * different codes.  The two calls here take the codes through a set (qfec_codeset, d_code [G]) as
 * the mixed codec does; no block crosses to the host on either side.
 *
 * Packet geometry: packet p no longer belongs to group p / (k + m).  Two prefix tables, device
 * arrays the kernels read when they run (never read back, like d_code, d_bb and the offsets):
 *   d_pkt_first [G+1] (int32): group g's wire packets and slots are d_pkt_first[g] ..
 *     d_pkt_first[g] + k_g + m_g - 1; packet d_pkt_first[g] + i is data packet i for i < k_g,
 *     else FEC packet i - k_g.
 *   d_pay_first [G+1] (int32, sender only): group g's payload rows, d_pay_len and d_pn_len
 *     entries are d_pay_first[g] .. d_pay_first[g] + k_g - 1.
 * npkt and npay are the capacities of the per-packet and per-payload arrays: upper bounds the
 * host sizes the grids by, so a captured call can be replayed after the tables were rewritten.
 * qfec_mixed_packet_layout builds both tables.
 *
 * Rule, sender: per group the call is qfec_frame_encode_seal_groups_batch_ragged with that
 * group's (k, m) and bb[g]: the same blocks, parity, packets and d_pkt_len, and the same status
 * values (the -3 of a rejected frame and the -1 of bb % 8 != 0 included).  Headers, packets and
 * d_pkt_len are dense by packet index [npkt]; payload rows, d_pay_len and d_pn_len dense by
 * payload index [npay]; blocks and parity lie in qfec_mixed_layout's packed layout.
 * Rule, receiver: the acceptance rule of the arrival-order receiver above, steps 1 - 5, with k
 * and k + m read per group (an index >= k_g + m_g is ignored; late is "after k_g distinct opened
 * indices"); everything else is, per group, qfec_open_decode_extract_arrivals_ragged with that
 * group's (k, m, bb) on that group's arrivals in their order.  The slot of arrival a is
 * d_pkt_first[g] + d_arr_index[a]; d_arr_at and d_open_len are [npkt]; d_rows is [G][kmax] (only
 * the first k_g entries of a row are written); d_rec_rows is [G][rmax] over the set's rmax (255
 * from the group's own min(k_g, m_g) on); d_rev, d_rev_len and d_rev_pn_len rows are g*rmax + j
 * (d_rev_len -1 past the group's own count).
 *
 * A group is rejected with status -2 when d_code[g] >= ncodes, when its d_pkt_first span is not
 * exactly k_g + m_g wide, starts below 0 or reaches past npkt, or (sender) when its d_pay_first
 * span is not exactly k_g wide, starts below 0 or reaches past npay.  None of its blocks, parity,
 * packets, rows, revived rows or payloads is read or written; its d_rec_rows are 255; arrivals
 * tagged to it are QFEC_ARR_IGNORED.  Every packet index below npkt that lies in no valid
 * group's span (the span of a rejected group clipped to npkt, a gap of the table, the capacity
 * past the table's total; all of [0, npkt) when groups == 0) is set to d_pkt_len -1 on the
 * sender, to d_arr_at -1 and d_open_len -1 on the receiver, with either value of
 * arr_optimistic, and nothing else of it is written.  The tables need not be well formed for memory
 * safety: entries are read at indices 0 .. G only and every (group, index) is checked before it
 * is used; a table that is not ascending may give a packet any of the outcomes above.
 *
 * Call-level limits, -2 before anything is enqueued: those of the ragged call of the same
 * direction (with npkt in place of groups*(k+m)) and of the mixed codec calls; a set that holds a
 * code with k + m > 255; npkt or npay negative or above INT32_MAX.  n == 0 stays valid.
 * Streams, graphs: enqueue only; qfec_codeset_reserve(cs, groups) covers a capture of either.
 * Bucket or mix: the sender as the mixed codec (bucket by code when a
 * bucket fills the device, mix a flush of about a thousand groups: a third of the per-code
 * calls' time there, 12 % more at 65,536 groups); the receiver was no slower mixed at either
 * scale, so a ring need not be split by code.
 * ------------------------------------------------------------------------------- */
/* Host helper, no GPU: the two prefix tables ([groups + 1] each, either may be NULL) of groups
 * laid out one after the other.  A group with code[g] >= ncodes gets an empty span in both.
 * -2 on the argument errors of qfec_mixed_layout and on a total above INT32_MAX. */
QFEC_API int qfec_mixed_packet_layout(int ncodes, const int *k, const int *m, long long groups,
                                      const unsigned char *code, int *pkt_first, int *pay_first);
/* Host helper, no GPU: bb[g] = roundup8(max(pay_len + 2)) over the group's own k_g lengths at
 * pay_first[g] (NULL: the dense table of qfec_mixed_packet_layout) in pay_len [npay], then
 * qfec_mixed_layout's offsets and totals.  -2 on a length outside [0, 0x3fff], on a span outside
 * [0, npay] and on qfec_mixed_layout's errors (code[g] >= ncodes among them). */
QFEC_API int qfec_framed_layout_mixed(int ncodes, const int *k, const int *m, long long groups,
                                      const unsigned char *code, const int *pay_first,
                                      long long npay, const int *pay_len, int *bb,
                                      long long *data_off, long long *par_off,
                                      long long *rec_off, long long totals[3]);
/* Host helper, no GPU: qfec_arrivals_rx_block_bytes with the k and k + m of the arrival's own
 * group.  Arrivals tagged to a group without a code are skipped (its bb is 0).  -2 also for a
 * set that holds a code with k + m > 255. */
QFEC_API int qfec_arrivals_rx_block_bytes_mixed(int ncodes, const int *k, const int *m,
                                                long long groups, const unsigned char *code,
                                                long long n, const int *arr_group,
                                                const unsigned char *arr_index,
                                                const int *pkt_len, const int *ad_len,
                                                int ad_len_all, int *bb);
/* Sender: frame -> qfec_encode_batch_mixed -> seal of every packet. */
QFEC_API int qfec_frame_encode_seal_groups_batch_mixed(
    qfec_ctx *ctx, const qfec_codeset *cs, long long groups, const unsigned char *d_code,
    const int *d_bb, const int *d_pkt_first, const int *d_pay_first, long long npkt,
    long long npay, unsigned char *d_data, const long long *d_data_off, unsigned char *d_parity,
    const long long *d_par_off, const unsigned char *d_hdr, long long hdr_stride,
    const int *d_hdr_len, int hdr_len_all, const unsigned char *d_pay, long long pay_stride,
    const int *d_pay_len, const unsigned char *d_pn_len, int pn_len_all, unsigned char *d_pkt,
    long long pkt_stride, int *d_pkt_len, int *d_status, void *stream);
/* Receiver over arrivals: open -> bind -> qfec_decode_batch_mixed_recovered -> extraction. */
QFEC_API int qfec_open_decode_extract_arrivals_mixed(
    qfec_ctx *ctx, const qfec_codeset *cs, long long groups, const unsigned char *d_code,
    const int *d_bb, const int *d_pkt_first, long long npkt, long long n,
    const unsigned char *d_pkt, long long pkt_stride, const int *d_pkt_len, const int *d_ad_len,
    int ad_len_all, const unsigned char *d_pn_len, int pn_len_all, const int *d_arr_group,
    const unsigned char *d_arr_index, int *d_arr_state, int *d_arr_at, unsigned char *d_blocks,
    const long long *d_blocks_off, unsigned char *d_rows, int *d_open_len, unsigned char *d_rec,
    const long long *d_rec_off, unsigned char *d_rec_rows, int *d_status, unsigned char *d_rev,
    long long rev_stride, int *d_rev_len, unsigned char *d_rev_pn_len, void *stream);

/* ---------------------------------------------------------------------------------
 * Receiver window: the arrival-order receiver with its state kept between calls.
 *
 * qfec_open_decode_extract_arrivals_ragged sets its binding table up again inside every call, so a
 * group whose packets fall into two ring reads holds "fewer than k" in both.  A socket's ring
 * does not end at a group boundary: QuicFecGroup keeps a group until its k-th packet comes
 * (quic_fec_group.cc:167-169, 210-213).  A window is that state on the device: `groups` group
 * places of one (k, m), fed by any number of pushes, each a ring in arrival order with the tags of
 * the arrival-order receiver (d_arr_group[a] is the group's place in the window).  A group
 * delivers its revived payloads in the push that brings its k-th packet; a place is used again
 * after qfec_rxwin_release.  
 *
 * What the window owns, all of it allocated by qfec_rxwin_create (a push allocates nothing): one
 * hold row of hold_stride bytes per slot (groups*(k+m) rows: every accepted packet keeps a row of
 * its own, so nothing is packed, placed or copied when a group completes); a state per slot
 * (empty, held with its plaintext length, seen but late); per group the count of held packets and
 * a delivered mark; the tables of one push (binding, pre-pass, rows, block and rec pointers, the
 * effective bb per group); and the context's decode workspace sized for `groups` groups, eager
 * and graph, so a captured push needs no qfec_reserve.  qfec_rxwin_bytes gives the size of the
 * window's own allocation (host, no GPU): with S = groups*(k+m), rmax = min(k, m) and r256(x) = x
 * rounded up to 256,
 *   r256(S*hold_stride) + 3*r256(4*S) + 4*r256(4*groups) + r256(groups*k) + r256(8*groups*k)
 *   + r256(8*groups*rmax).
 * Create limits, -2 with text in qfec_last_error(): those of the ragged calls (k, m >= 1,
 * k <= 255, groups >= 0); k + m > 255; groups*(k+m) > INT32_MAX; hold_stride below 16 or not a
 * multiple of 16; a NULL context or out.  An allocation failure returns a code <= -2 with the HIP
 * text, and nothing is left allocated.  A window belongs to its context and is destroyed before
 * it; qfec_rxwin_destroy waits for the device.
 *
 * Acceptance, defined sequentially over the arrivals of all pushes since the group's last release
 * (the device result equals it; it is the arrival-order receiver's rule over the concatenation
 * of the rings):
 *   1. tag outside [0, groups) or index >= k+m: QFEC_ARR_IGNORED.
 *   2. the packet fails the framed open's length checks against the d_bb[g] of this push (a data
 *      plaintext of at most bb-2 bytes, an FEC plaintext of at most bb; none passes where
 *      bb[g] < 1 or bb[g] > hold_stride) or its tag does not match: QFEC_ARR_REJECTED.  The state
 *      is untouched.
 *   3. the slot is not empty, from an earlier push or earlier in this one: QFEC_ARR_DUPLICATE.
 *   4. the group already holds k: QFEC_ARR_LATE, and the slot becomes seen.
 *   5. otherwise the arrival is accepted: the slot becomes held, d_arr_state[a] = the plaintext
 *      length.
 * Hold rows: a data packet's row is prefix || payload || zeros to hold_stride (prefix = len |
 * pn_len << 14, little-endian, as the framed calls write it), an FEC packet's row is plaintext ||
 * zeros to hold_stride.  The first bb bytes of a row are therefore the one-shot call's block for
 * any bb up to hold_stride: a bb[g] that grows between pushes needs no rewrite.
 *
 * Completion: group g completes in the push that accepts its k-th packet, with bb = d_bb[g] of
 * that push.  Its rows are formed as in the one-shot call (the holes, ascending, take the held
 * FEC packets, ascending); its blocks are the hold rows, read where they lie by the pointer-table
 * decode (qfec_decode_batch_ptrs_recovered's kernels); recovered block j goes to d_rec +
 * d_rec_off[g] + j*bb.  For a completing group d_status[g] (0, or -1 for bb % 8 != 0 with a
 * recovery block), d_rec_rows, the recovered blocks, d_rev, d_rev_len and d_rev_pn_len are byte for
 * byte what qfec_open_decode_extract_arrivals_ragged gives over the concatenated rings with the
 * same bb.  If a held packet's stored size (plaintext + 2 for a data packet) exceeds that push's
 * bb, which happens only when the caller shrank bb[g], the group completes with status -3 and
 * nothing is revived.  For every other group of the push: d_status is QFEC_WIN_OPEN (fewer than k
 * so far) or QFEC_WIN_DELIVERED (completed in an earlier push, not released since), d_rec_rows is
 * 255, d_rev_len is -1, and no rec or rev byte is written; none of those groups' pointer-table
 * entries is dereferenced (their effective bb is 0).  The decode's kernels and the fixed-cost
 * passes run over all `groups` places in every push.
 * d_rec_off is the ragged calls' array (multiples of 16, as qfec_ragged_layout gives); d_rec_rows
 * is [groups][rmax], d_rev rows, d_rev_len and d_rev_pn_len are g*rmax + j.  d_arr_state, d_status
 * and d_rev_pn_len may be NULL.
 *
 * qfec_rxwin_release enqueues one kernel: the listed groups (d_groups, int32 [count], a device
 * array) return to empty: slot states, count and delivered mark.  Entries outside [0, groups) are
 * skipped and repeats are harmless; d_groups == NULL releases every group; count < 0 is -2.
 *
 * Push, call-level -2 before anything is enqueued: a NULL window; n < 0 or n > INT32_MAX; a NULL
 * d_bb, d_rec, d_rec_off, d_rec_rows, d_rev or d_rev_len; d_rec not 16-byte aligned; pkt_stride < 1
 * or rev_stride < 0; ad_len_all < 0 without d_ad_len.  n == 0 is valid and the per-arrival arrays
 * (d_pkt, d_pkt_len, d_arr_group, d_arr_index) may then be NULL.
 * Streams, graphs: push and release only enqueue; they read no device array back and allocate
 * nothing.  A captured push replayed over new ring contents carries the state from replay to
 * replay.  Two calls on one window must be ordered by the caller (one stream, or events); they
 * run under the context's mutex and in the decode-workspace bracket, like every decode.
 * Launches of a push: rxwin_init_kernel, rxwin_pre_kernel (not with arr_optimistic = 0),
 * rxwin_open_kernel, rxwin_assemble_kernel, arrivals_state_kernel (with d_arr_state), the
 * pointer-table decode's, rxwin_finish_kernel, extract_revived_kernel.
 * ------------------------------------------------------------------------------- */
typedef struct qfec_rxwin qfec_rxwin;
#define QFEC_WIN_OPEN (-3)      /* fewer than k accepted so far (the one-shot's value) */
#define QFEC_WIN_DELIVERED (-5) /* completed in an earlier push, not released since */
/* Host helper, no GPU: the bytes of a window's own device allocation (the formula above).  -2 on
 * the create limits and a NULL bytes. */
QFEC_API int qfec_rxwin_bytes(int k, int m, long long groups, int hold_stride, long long *bytes);
QFEC_API int qfec_rxwin_create(qfec_ctx *ctx, int k, int m, long long groups, int hold_stride,
                               qfec_rxwin **out);
QFEC_API void qfec_rxwin_destroy(qfec_rxwin *win);
QFEC_API int qfec_rxwin_release(qfec_rxwin *win, long long count, const int *d_groups,
                                void *stream);
/* One ring read: open -> bind against the carried state -> pointer-table decode of the groups
 * that complete -> extraction. */
QFEC_API int qfec_rxwin_push(qfec_rxwin *win, const int *d_bb, long long n,
                             const unsigned char *d_pkt, long long pkt_stride,
                             const int *d_pkt_len, const int *d_ad_len, int ad_len_all,
                             const unsigned char *d_pn_len, int pn_len_all,
                             const int *d_arr_group, const unsigned char *d_arr_index,
                             int *d_arr_state, unsigned char *d_rec, const long long *d_rec_off,
                             unsigned char *d_rec_rows, int *d_status, unsigned char *d_rev,
                             long long rev_stride, int *d_rev_len, unsigned char *d_rev_pn_len,
                             void *stream);
/* Host helper, no GPU: the running form of qfec_arrivals_rx_block_bytes, its state in the
 * caller's hands.  seen [groups][32] (in/out) is a bitset of the indices counted so far (index i
 * of group g: bit i % 8 of byte g*32 + i / 8); bb [groups] (in/out) the running maximum over the
 * group's first k distinct indices.  From zeroed state, running it over the pieces of a stream
 * gives what qfec_arrivals_rx_block_bytes gives over their concatenation; the caller zeroes a
 * group's 32 bytes and its bb when it releases the group.  -2 as that helper, and a NULL seen. */
QFEC_API int qfec_arrivals_rx_block_bytes_carry(int k, int m, long long groups, long long n,
                                                const int *arr_group,
                                                const unsigned char *arr_index,
                                                const int *pkt_len, const int *ad_len,
                                                int ad_len_all, unsigned char *seen, int *bb);

/* ---------------------------------------------------------------------------------
 * Support: the coefficient tables, a seeded synthetic workload, diagnostics.
 * ------------------------------------------------------------------------------- */
/* Rows 1..m-1 of the Cauchy matrix the reference selects (cauchy_256.cpp:422-480),
 * (m-1) x k bytes, row-major.  Host only.  Returns -1 if m < 2 or k + m > 256. */
QFEC_API int qfec_cauchy_matrix(int k, int m, unsigned char *out);

/* Fill d_dst with bytes [byte_offset, byte_offset + bytes) of the splitmix64 stream
 * (byte_offset % 8 == 0); see quic_amd/synth.py for the definition. */
QFEC_API int qfec_synth_fill(void *d_dst, unsigned long long bytes, unsigned long long seed,
                    unsigned long long byte_offset, void *stream);
/* blocks[g][i] = (src[g][i] < k ? data[g][src] : parity[g][src - k]); src is int16 [G][k]. */
QFEC_API int qfec_synth_gather(const unsigned char *d_data, const unsigned char *d_parity,
                      const short *d_src, unsigned char *d_blocks, int k, int m,
                      int block_bytes, long long groups, void *stream);

QFEC_API const char *qfec_last_error(void);
/* Names of the kernels this thread's last engine call launched, " + "-separated, e.g.
 * "decode_prep_lane_kernel + gf_stream_kernel<decode>" (bench.py reports it).  The ragged
 * calls name "gf_ragged_kernel<encode>", "gf_ragged_kernel<decode>", "xor_ragged_kernel" and
 * "copy_ragged_kernel"; the pointer-table calls name "gf_ptrs_kernel<encode>",
 * "gf_ptrs_kernel<decode>", "xor_ptrs_kernel" and "copy_ptrs_kernel" (and, without d_bb and with
 * bb_all % 8 != 0, "ptrs_decode_status_kernel"); the mixed-code calls name
 * "xor_copy_mixed_kernel<encode>" / "<decode>", "gf_mixed_kernel<encode>" / "<decode>" and
 * "decode_prep_mixed_kernel" ("decode_prep_mixed_kernel<cached>" when the set's encode matrices
 * do not fit in LDS); the ragged protected calls add "null_seal_kernel<ragged>" and
 * "open_group_kernel<ragged> + open_assemble_kernel<ragged>" (the uniform grouped calls name
 * "null_seal_kernel<groups>" and "open_group_kernel + open_assemble_kernel"); the framed calls
 * name "frame_blocks_kernel", "null_seal_kernel<framed>", "open_group_kernel<framed> +
 * open_assemble_kernel<framed>" and "extract_revived_kernel"; the arrivals call names
 * "arrivals_init_kernel", "arrivals_pre_kernel", "open_arrivals_kernel",
 * "arrivals_assemble_kernel" and (with d_arr_state) "arrivals_state_kernel" ahead of the decode's
 * and "extract_revived_kernel"; a window push names "rxwin_init_kernel", "rxwin_pre_kernel",
 * "rxwin_open_kernel", "rxwin_assemble_kernel" and (with d_arr_state) "arrivals_state_kernel" ahead
 * of the pointer-table decode's, then "rxwin_finish_kernel" and "extract_revived_kernel"; a
 * release names "rxwin_release_kernel"; the mixed-code wire calls name "mixed_wire_plan_kernel" first and
 * carry a "<mixed>" suffix on the kernels that read the mixed geometry:
 * "frame_blocks_kernel<mixed>", "null_seal_kernel<mixed>", "arrivals_pre_kernel<mixed>",
 * "open_arrivals_kernel<mixed>", "arrivals_assemble_kernel<mixed>", "arrivals_unowned_kernel",
 * "arrivals_state_kernel<mixed>",
 * "open_status_kernel<mixed>" and "extract_revived_kernel<mixed>" (around the mixed codec's). */
QFEC_API const char *qfec_last_kernels(void);
/* Grids of the persistent kernels the last call on this thread launched, as space-separated
 * "kernel=workgroups" entries (e.g. "gf_psyn_kernel=1024"); diagnostics and tests.  The general
 * decode prep reports "decode_prep_kernel": its workgroups hold 4, 2 or 1 groups each as the
 * min(k, m)^2 solve scratch fills the LDS.  The m = 1 LDS-ring kernel reports "xor_dma_kernel"
 * for its encode and every decode variant: at most one workgroup per CU, or with the xor_wg
 * option about xor_wg groups per wave. */
QFEC_API const char *qfec_last_grids(void);
/* Measurement hook (bench.py's roofline timing).  While set, every engine call on this
 * thread records start_event (a hipEvent_t) at the start of its first kernel and
 * stop_event at the end of its last, through hipExtLaunchKernel, so the pair brackets the
 * call's kernels only.  Pass NULL, NULL to stop.  Returns -2 if only one is NULL. */
QFEC_API int qfec_set_timing_events(void *start_event, void *stop_event);
QFEC_API int qfec_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QUIC_AMD_QUIC_FEC_H */
