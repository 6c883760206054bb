/* pbftv.h -- C ABI of the MI355X batch verifier for simple_pbft's crypto hot path.
 *
 * Drop-in boundary.  The reference (1556174776/simple_pbft,
 * Go) has no FFI; the functions below are what a thin cgo shim binds so the
 * Go call sites keep their signatures (INTEGRATION.md shows the binding):
 *
 *   pbftv_hash_hex            <- utils.Hash(content []byte) string          utils/utils.go:13-17
 *   pbftv_sha256_batch        <- batched utils.Hash over a pool snapshot   utils/utils.go:13-17
 *   pbftv_gojson_*            <- json.Marshal preimages hashed by digest() pbft/consensus/pbft_impl.go:235-243,
 *                                                                          pbft/consensus/pbft_msg_types.go:3-38
 *   pbftv_digest_request_batch<- digest(*RequestMsg) for many requests     pbft/consensus/pbft_impl.go:73,235-243
 *   pbftv_digest_check_batch  <- digest recompute + compare per message    pbft/consensus/pbft_impl.go:190-199
 *   pbftv_verify_msg_batch    <- State.verifyMsg over a vote snapshot      pbft/consensus/pbft_impl.go:176-202
 *   pbftv_register_keys       <- per-node public-key table (planned by the author next to
 *                                NodeTable, 需要改进的地方.md:17 / pbft/network/node.go:60-65)
 *   pbftv_ecdsa_p256_verify_batch <- Go crypto/ecdsa.Verify per signed pool message
 *                                (absent in the reference)
 *   pbftv_qc_verify           <- quorum count of prepared()/committed()    pbft/consensus/pbft_impl.go:207-232
 *
 * Conventions
 *   - The caller owns every buffer; the library never keeps a pointer after a
 *     call returns (cgo rule: no Go pointers retained by C).
 *   - Host-buffer calls are synchronous.  *_dev calls take device pointers on
 *     one of the context's devices and enqueue on `stream` (a hipStream_t, or
 *     NULL for the context's stream of that device) without synchronising.
 *   - Return 0 on success, negative PBFTV_E* on API / device errors.  A failed
 *     signature or digest is never an error: it is a 0 bit.
 *   - Bitmaps are LSB-first: bit i of the batch is (bitmap[i/8] >> (i%8)) & 1.
 *   - Big-endian 32-byte integers (hash, r, s, X, Y) exactly as Go's
 *     big.Int.FillBytes / elliptic.Marshal would lay them out.
 *   - A context is safe to share across threads (one lock per device).
 *   - There is no CPU fallback: with no usable gfx950 device pbftv_open fails
 *     with PBFTV_ENODEV.
 */
#ifndef PBFTV_H
#define PBFTV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBFTV_OK 0
#define PBFTV_EINVAL (-1)   /* bad argument (null pointer, bad device index, ...) */
#define PBFTV_ENODEV (-2)   /* no usable GPU in device_mask */
#define PBFTV_EDEVICE (-3)  /* HIP runtime / kernel error; see pbftv_last_error() */
#define PBFTV_ENOMEM (-4)   /* device or pinned host allocation failed */
#define PBFTV_ENOKEYS (-5)  /* verify called before pbftv_register_keys */
#define PBFTV_ENOSIGNKEYS (-6) /* sign called before pbftv_register_signing_keys */
#define PBFTV_ENOSPACE (-7) /* pbftv_seal_*: out_wire is too small; *out_wire_bytes holds the size needed */

typedef struct pbftv_ctx pbftv_ctx;

/* Open a context on the GPUs in device_mask (bit d = HIP device d; 0 = all
 * visible).  Batches passed to the host-buffer calls are split into
 * contiguous shards, one per device (no collective: the shards are
 * independent and the bitmaps are concatenated). */
int pbftv_open(pbftv_ctx** out, uint32_t device_mask);
void pbftv_close(pbftv_ctx* ctx);
int pbftv_device_count(const pbftv_ctx* ctx);
/* HIP device id of the context's i-th device, or -1. */
int pbftv_device_id(const pbftv_ctx* ctx, int i);
const char* pbftv_strerror(int code);
/* Last error message of the calling thread ("" if none). */
const char* pbftv_last_error(void);
/* Pre-size per-device scratch for batches of up to n items (optional). */
int pbftv_reserve(pbftv_ctx* ctx, uint64_t n);

/* ---- device memory / stream plumbing ---------------------------------- */
/* For callers that keep pool snapshots resident in HBM (and for bench.py):
 * allocations on the context's device index dev, copies on that device's
 * stream (synchronous), and a stream synchronise.  pbftv_dev_alloc memory
 * comes from a stream-ordered pool of the context; pbftv_dev_free returns it
 * once the work queued so far on the context's streams (its own and those
 * from pbftv_stream_create) has passed, without a device-wide
 * synchronisation, and waits on the host for the context's work on other
 * caller streams -- so a free does not stop the armed latency kernels. */
int pbftv_dev_alloc(pbftv_ctx* ctx, int dev, uint64_t bytes, void** out_ptr);
int pbftv_dev_free(pbftv_ctx* ctx, int dev, void* ptr);
/* Pinned host memory (hipHostMalloc, portable): batches placed in it skip the
 * staging copy of the host-buffer verify path (e.g. a cgo shim's pool-flush
 * buffers).  A freed block is kept for the next pbftv_host_alloc of a similar
 * size (at least the size asked for and at most twice it; up to 1 GiB of
 * freed blocks per context, the largest leave first; released at
 * pbftv_close), so a free does not synchronise the GPU either.  Before
 * pbftv_host_free the caller must have synchronised its own asynchronous use
 * of the block (a *_dev call or a copy of its own that still reads or writes
 * it): the block may be handed out again, or unmapped, at once.  The library's
 * own calls that read a host buffer have finished with it when they return. */
int pbftv_host_alloc(pbftv_ctx* ctx, uint64_t bytes, void** out_ptr);
int pbftv_host_free(pbftv_ctx* ctx, void* ptr);
int pbftv_memcpy_h2d(pbftv_ctx* ctx, int dev, void* dst, const void* src, uint64_t bytes);
int pbftv_memcpy_d2h(pbftv_ctx* ctx, int dev, void* dst, const void* src, uint64_t bytes);
int pbftv_memset_dev(pbftv_ctx* ctx, int dev, void* dst, int value, uint64_t bytes);
/* The context's stream of device dev as a hipStream_t (for *_dev calls). */
void* pbftv_stream(pbftv_ctx* ctx, int dev);
int pbftv_stream_sync(pbftv_ctx* ctx, int dev);
/* Caller streams on device dev for *_dev calls.  A stream made here owns its
 * ECDSA verify scratch (stage-1 records, key order, result bytes; freed by
 * pbftv_stream_destroy) AND a hardware queue, so verifies enqueued on two
 * such streams run concurrently on the GPU: a caller that alternates batches
 * between two streams overlaps batch j + 1's scalar stage with batch j's comb.
 * That is how consecutive batches overlap; batches on one stream, or on
 * streams that share a hardware queue, run strictly one after the other.
 * The queue is the stream's alone whatever other streams the process has
 * (the HIP runtime spreads plain streams over GPU_MAX_HW_QUEUES = 4 queues
 * and shares them beyond that; these streams are created with a CU mask of
 * every CU, which the runtime never pools).  At most 8 streams per device
 * and context hold such a queue at a time; the ones created beyond that are
 * plain non-blocking streams and may share.  A stream with a queue of its own
 * is a blocking HIP stream: it orders with work on the null stream, which the
 * library never uses -- keep a caller's null-stream work off the hot path.
 * PBFTV_STREAM_QUEUE=shared (read once per process) makes every stream plain,
 * as before.
 * Other device scratch shared by calls on different streams (d.stream and any
 * foreign hipStream_t) is ordered by the library (an event per device), so
 * concurrent *_dev calls on several streams are safe. */
int pbftv_stream_create(pbftv_ctx* ctx, int dev, void** out_stream);
int pbftv_stream_destroy(pbftv_ctx* ctx, int dev, void* stream);
int pbftv_stream_wait(pbftv_ctx* ctx, int dev, void* stream);

/* Batches of up to n signatures take the latency path (one wave per
 * signature); larger ones the lane path (scalar + comb kernels).  Default
 * 2048, or PBFTV_WAVE_MAX at pbftv_open; 0 disables the latency path.  Read
 * once per call from the context, never from the environment on the call
 * path.
 *
 * Up to 128 signatures of a latency-path call are served by a resident
 * "armed" kernel polling a doorbell in pinned host memory (a workgroup per
 * signature slot: as many as the largest recent certificate, at least 4;
 * up to 128 once calls of 9..128 signatures have been seen), so no launch is
 * on the call's path.  A keeper thread per device replaces it
 * before its budget runs out for as long as calls keep coming.  Environment,
 * read at every arming:
 *   PBFTV_QC_ARM=0            never arm (every call launches);
 *   PBFTV_QC_ARM_MS=100       one armed kernel's budget (ms);
 *   PBFTV_QC_KEEP_MS=10000    keep one armed this long after the last call
 *                             (0: no keeper; the kernel runs out);
 *   PBFTV_QC_WIDE=0           never arm the 128-wave form;
 *   PBFTV_QC_YIELD            whether a lane-path batch halts the armed
 *                             kernel (certificates meanwhile are launched,
 *                             ~0.1 ms beside the batch instead of ~0.04 ms;
 *                             the keeper re-arms after it): "1" always, "0"
 *                             never; unset (default) when no certificate
 *                             came for PBFTV_QC_YIELD_IDLE_MS (50 ms).  A
 *                             resident server costs a busy stream ~3 %
 *                             (narrow) to 6-9 % (wide, 67 votes);
 *   PBFTV_QC_CU_YIELD         while an armed workgroup serves, the lane-path
 *                             comb waves on its CU park at their next step
 *                             (a per-CU flag word; at most 50 µs): "1" the
 *                             default, "0" never, "2" also on the CU that
 *                             shares its instruction cache.  3 signatures
 *                             beside a 1M stream 40.0 -> 33.5 µs p50 at the
 *                             same stream rate;
 *   PBFTV_QC_EXCLUSIVE_CU     armed workgroups take whole CUs, so a
 *                             concurrent batch does not share their SIMDs
 *                             (with PBFTV_QC_YIELD=0): "narrow" the narrow
 *                             kernel (one CU per armed slot), "1" the wide
 *                             one too (128 CUs); off by default;
 *   PBFTV_QC_ROWS=0           the quad schedule (one wave per signature)
 *                             instead of the row schedule (a workgroup per
 *                             signature), for A/B;
 *   PBFTV_QC_ROWS_MAX         launched batches up to this many signatures
 *                             take the row schedule (default 128);
 *   PBFTV_QC_SLOTS=k          arm k narrow slots (1..8) instead of the
 *                             largest recent certificate (at least 4);
 *   PBFTV_QC_STAMPS=1         the kernel records GPU timestamps
 *                             (pbftv_qc_stamps*);
 *   PBFTV_TRACE_QC=1          why a call was launched, on stderr.
 * The library's own device frees (scratch growth, re-registration) stop every
 * armed kernel on the GPU first (hipFree waits for every kernel); the
 * caller's pbftv_dev_free / pbftv_host_free do not. */
int pbftv_set_latency_path_max(pbftv_ctx* ctx, uint64_t n);

/* Per-kernel timing with HIP events recorded on the launch stream around every
 * kernel launch while enabled.  kernel: 0 = ecdsa scalars, 1 = ecdsa comb,
 * 2 = sha256, 3 = ecdsa wave-per-signature (small batches), 4 = Go-JSON message
 * encoder (digest / flush batches), 5 = ecdsa under unregistered keys (the
 * ladder kernel of pbftv_ecdsa_p256_verify_pubkey_batch).  pbftv_kernel_time_ms synchronises the device's stream and
 * returns the summed milliseconds and the launch count since the last reset.
 * Timing id 6, PBFTV_K_ECDSA_DER, is the launch of k_der_to_rs (DER signatures
 * normalised to r||s: pbftv_ecdsa_der_to_rs_batch_dev and every *_der verify
 * and flush), timed and reset with the others.  pbftv_kernel_time_ms accepts
 * the ids 0..5 it always did (any other is PBFTV_EINVAL, as callers may rely
 * on); id 6 is read through pbftv_der_kernel_time_ms, same outputs.
 * Timing id 7, PBFTV_K_ECDSA_SIGN, is the signer's kernels (the sign batches
 * and pbftv_sign_replies below), timed and reset with the others and read
 * through pbftv_sign_kernel_time_ms: stage 0 = all of them summed, 1 = nonce
 * (RFC 6979 DRBG, k^-1), 2 = comb (k*G, r), 3 = tail (s, the rows and ok
 * bits), 4 = the DER writer; out_launches counts the launches of the stage
 * asked for (a sign batch is one launch of each of 1..3). */
#define PBFTV_K_ECDSA_SCALARS 0
#define PBFTV_K_ECDSA_COMB 1
#define PBFTV_K_SHA256 2
#define PBFTV_K_ECDSA_WAVE 3
#define PBFTV_K_GOJSON 4
#define PBFTV_K_ECDSA_VARBASE 5
#define PBFTV_K_ECDSA_DER 6
#define PBFTV_K_ECDSA_SIGN 7
int pbftv_set_kernel_timing(pbftv_ctx* ctx, int enable);
int pbftv_kernel_time_ms(pbftv_ctx* ctx, int dev, int kernel, double* out_ms, uint64_t* out_launches);
int pbftv_der_kernel_time_ms(pbftv_ctx* ctx, int dev, double* out_ms, uint64_t* out_launches);
int pbftv_sign_kernel_time_ms(pbftv_ctx* ctx, int dev, int stage, double* out_ms, uint64_t* out_launches);
int pbftv_reset_kernel_times(pbftv_ctx* ctx);
/* Diagnostics of the last latency-path call (n <= 2048) on device dev:
 * out[0] = host ns from entry to the request being handed over (bell rung or
 * kernel launched), out[1] = host ns from entry to return, out[2] bit 0 = 1
 * if an armed kernel served it, 0 if a launch did, bits 1..31 = host ns from
 * entry to the verdicts of the first 8 signatures all in, bits 32..63 = host
 * ns from entry to holding the device lock, out[3..6] = the armed kernel's
 * slot-0 wave: GPU wall clock and shader clock when it saw the request, and
 * when it wrote its verdict (0 after a launch; written only while
 * PBFTV_QC_STAMPS=1 was set when the kernel was armed), out[7] = the
 * wall-clock rate in kHz. */
int pbftv_qc_stamps(pbftv_ctx* ctx, int dev, uint64_t out[8]);
/* The same GPU stamps for every armed wave of the last call (up to `waves`
 * entries of {seen wall, seen shader clock, done wall, done shader clock};
 * helper waves past the 8 slots included): returns the number written, 0 if a
 * launch served the call.  Stamps of waves that had no signature are stale. */
int pbftv_qc_stamps_all(pbftv_ctx* ctx, int dev, uint64_t* out, uint32_t waves);
/* Counters of the latency path on device dev since pbftv_open (diagnostics;
 * tests assert which path served what): out[0] calls, out[1] calls served by
 * an armed kernel, out[2] armed calls handed to a launched rerun (the armed
 * row kernel met an exceptional signature: a doubling or cancellation in its
 * tree, a live window with two zero digits, r + n < p), out[3] signatures that
 * took a launched row kernel's exact path, out[4] launched latency kernels,
 * out[5] armings, out[6] keeper rotations, out[7] the armed kernel now: its
 * workgroups (0: none armed) | 1 << 32 if it is the wide one. */
int pbftv_qc_counters(pbftv_ctx* ctx, int dev, uint64_t out[8]);
/* Counters of the library's own bookkeeping on device dev since pbftv_open
 * (diagnostics; tests assert on them): out[0] pbftv_dev_free blocks still
 * waiting for their marks, out[1] events held by them, out[2] spare events,
 * out[3] events created for such marks (at every call out[1] + out[2] ==
 * out[3]), out[4] lane-path ECDSA batches that took the key order; out[5..7]
 * are zero. */
int pbftv_lib_counters(pbftv_ctx* ctx, int dev, uint64_t out[8]);

/* ---- SHA-256 digests (utils.Hash) ------------------------------------ */

/* utils.Hash(content): lowercase hex SHA-256, 64 chars + NUL into out_hex. */
int pbftv_hash_hex(pbftv_ctx* ctx, const uint8_t* content, uint64_t len, char out_hex[65]);

/* n messages at data+offsets[i], lengths[i] bytes -> out_digests (n*32 raw bytes). */
int pbftv_sha256_batch(pbftv_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths,
                       uint64_t n, uint8_t* out_digests);

/* As above, plus compare against expected (n*32): bit i = digest matches. */
int pbftv_digest_check_batch(pbftv_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths,
                             const uint8_t* expected, uint64_t n, uint8_t* out_bitmap);

/* Device-resident form on device index dev (0..pbftv_device_count-1).  The
 * data buffer must be readable
 *   - over every 128-byte-aligned line that holds a byte of a message, or the
 *     position of an empty message that is not on a line boundary: the default
 *     kernel (k_sha256_ring) fetches whole lines, so it reads up to 127 bytes
 *     before a message's first byte and up to 127 after its last;
 *   - over every 4-byte-aligned dword that does, so less than 4 bytes past the
 *     end of a message: the PBFTV_SHA_RING=0 kernel (k_sha256) reads those.
 * Memory mapped in pages (pbftv_dev_alloc / hipMalloc allocations, and ranges
 * inside them) meets both, as a line never crosses a page; those bytes are
 * read and masked off, never hashed.  order (may be NULL) is a lane ->
 * message permutation; pbftv_sha256_order_dev builds one that groups messages
 * by block count.  d_expected/d_bitmap may be NULL (digests only); d_bitmap
 * must be ceil(n/32)*4 bytes when used. */
int pbftv_sha256_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_data, const uint64_t* d_offsets,
                           const uint32_t* d_lengths, const uint32_t* d_order, uint64_t n, uint8_t* d_digests,
                           const uint8_t* d_expected, uint8_t* d_bitmap, void* stream);
int pbftv_sha256_order_dev(pbftv_ctx* ctx, int dev, const uint32_t* d_lengths, uint64_t n, uint32_t* d_order,
                           void* stream);

/* ---- Go-JSON digest preimages (json.Marshal of pbft_msg_types.go) ----- */
/* Each writes at most cap bytes to out and returns the full encoded length
 * (call with cap = 0 to size).  Strings are byte strings (ptr, len) and may
 * hold arbitrary bytes; encoding follows Go 1.19 encoding/json exactly. */
uint64_t pbftv_gojson_request(int64_t timestamp, const char* client_id, uint64_t client_id_len, const char* operation,
                              uint64_t operation_len, int64_t sequence_id, uint8_t* out, uint64_t cap);
uint64_t pbftv_gojson_vote(int64_t view_id, int64_t sequence_id, const char* digest, uint64_t digest_len,
                           const char* node_id, uint64_t node_id_len, int64_t msg_type, uint8_t* out, uint64_t cap);
/* Signed VoteMsg on the wire (build-added; no reference
 * counterpart): the VoteMsg fields of pbft_msg_types.go:25-31 followed by
 * Signature []byte `json:"signature"` -- base64.StdEncoding, or null when
 * sig_nil != 0 (Go's nil slice).  The signing preimage is pbftv_gojson_vote. */
uint64_t pbftv_gojson_vote_signed(int64_t view_id, int64_t sequence_id, const char* digest, uint64_t digest_len,
                                  const char* node_id, uint64_t node_id_len, int64_t msg_type, const uint8_t* sig,
                                  uint64_t sig_len, int sig_nil, uint8_t* out, uint64_t cap);
/* Signed RequestMsg / ReplyMsg / PrePrepareMsg on the wire:
 * the struct of pbft_msg_types.go:3-23 followed by "signature" as above.  Each
 * signing preimage is the unsigned encoding (pbftv_gojson_request / _reply /
 * _preprepare).  A client signs its request with the sequenceID it sent (the
 * reference's clients leave it 0; StartConsensus assigns it, pbft_impl.go:67);
 * a pre-prepare's embedded request carries the client's signature on the wire
 * (req_sig*), while the primary's preimage embeds the unsigned request. */
uint64_t pbftv_gojson_request_signed(int64_t timestamp, const char* client_id, uint64_t client_id_len,
                                     const char* operation, uint64_t operation_len, int64_t sequence_id,
                                     const uint8_t* sig, uint64_t sig_len, int sig_nil, uint8_t* out, uint64_t cap);
uint64_t pbftv_gojson_reply_signed(int64_t view_id, int64_t timestamp, const char* client_id, uint64_t client_id_len,
                                   const char* node_id, uint64_t node_id_len, const char* result, uint64_t result_len,
                                   const uint8_t* sig, uint64_t sig_len, int sig_nil, uint8_t* out, uint64_t cap);
uint64_t pbftv_gojson_preprepare_signed(int64_t view_id, int64_t sequence_id, const char* digest, uint64_t digest_len,
                                        int has_request, int64_t req_timestamp, const char* req_client_id,
                                        uint64_t req_client_id_len, const char* req_operation,
                                        uint64_t req_operation_len, int64_t req_sequence_id, const uint8_t* req_sig,
                                        uint64_t req_sig_len, int req_sig_nil, const uint8_t* sig, uint64_t sig_len,
                                        int sig_nil, uint8_t* out, uint64_t cap);
uint64_t pbftv_gojson_reply(int64_t view_id, int64_t timestamp, const char* client_id, uint64_t client_id_len,
                            const char* node_id, uint64_t node_id_len, const char* result, uint64_t result_len,
                            uint8_t* out, uint64_t cap);
uint64_t pbftv_gojson_preprepare(int64_t view_id, int64_t sequence_id, const char* digest, uint64_t digest_len,
                                 int has_request, int64_t req_timestamp, const char* req_client_id,
                                 uint64_t req_client_id_len, const char* req_operation, uint64_t req_operation_len,
                                 int64_t req_sequence_id, uint8_t* out, uint64_t cap);

/* ---- DER signatures (go1.19 crypto/ecdsa.VerifyASN1's cryptobyte parse) ---
 * SEQUENCE { INTEGER r, INTEGER s } with Go's DER strictness -> r||s (64 B
 * big-endian, the sig_rs layout of pbftv_ecdsa_p256_verify_batch).  Returns 1
 * when parsed with 0 <= r, s < 2^256, 0 when Go would reject it at the parse
 * or range check (out_rs zeroed, so the verify yields a 0 bit), PBFTV_EINVAL
 * on null pointers.  The batch form returns the number parsed (or < 0).
 * These two run on the host, one signature after another (25-40 ns each);
 * a caller that verifies what it parses hands the encodings to the *_der
 * calls below (after the *_wirekey ones) instead, which run the same parser
 * on the device in the round trip of the verify. */
int pbftv_ecdsa_der_to_rs(const uint8_t* der, uint64_t der_len, uint8_t* out_rs);
int64_t pbftv_ecdsa_der_to_rs_batch(const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths,
                                    uint64_t n, uint8_t* out_rs);

/* digest(*RequestMsg) for n requests (pbft_impl.go:235-243, called from
 * StartConsensus :73 and verifyMsg :190): the struct fields are shipped
 * column-wise, the Go-JSON preimages are built on the GPU (one lane per
 * message, same encoder as pbftv_gojson_*) and hashed there.  client_ids /
 * operations are concatenated byte strings with per-item offsets/lengths.
 * String columns, here and in every message-batch call below (digest_*_batch,
 * flush_*): the strings may lie in any order in their blob, share bytes, and
 * have other bytes before and between them (those are copied with the span
 * the strings cover, and never encoded).  The offset of a string of length 0
 * is not read: it may hold any value, inside the blob or not.
 * out_digests: n*32 raw bytes. */
int pbftv_digest_request_batch(pbftv_ctx* ctx, uint64_t n, const int64_t* timestamps, const uint8_t* client_ids,
                               const uint64_t* client_id_off, const uint32_t* client_id_len, const uint8_t* operations,
                               const uint64_t* operation_off, const uint32_t* operation_len,
                               const int64_t* sequence_ids, uint8_t* out_digests);

/* digest(*VoteMsg) / digest(*ReplyMsg) / digest(*PrePrepareMsg) for n
 * messages (the signed preimages of votes, replies and pre-prepares): Go-JSON
 * built on the GPU, hashed there.  For pre-prepares, has_request[i] = 0 encodes
 * requestMsg as null (the req_* columns must still hold n entries). */
int pbftv_digest_vote_batch(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                            const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                            const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                            const int64_t* msg_types, uint8_t* out_digests);
int pbftv_digest_reply_batch(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                             const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                             const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                             const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                             uint8_t* out_digests);
int pbftv_digest_preprepare_batch(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                                  const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                                  const uint8_t* has_request, const int64_t* req_timestamps,
                                  const uint8_t* req_client_ids, const uint64_t* req_client_id_off,
                                  const uint32_t* req_client_id_len, const uint8_t* req_operations,
                                  const uint64_t* req_operation_off, const uint32_t* req_operation_len,
                                  const int64_t* req_sequence_ids, uint8_t* out_digests);

/* Pool flush of a snapshot of prepare/commit votes (GetAllPrepareMsg /
 * GetAllCommitMsg, pool/preparePool.go:56-67, pool/commitPool.go:57-68, as
 * drained by resolvePrepareMsg / resolveCommitMsg, pbft/network/node.go:559-598)
 * across any number of consensus states, in one GPU round trip per device:
 *   h_i        = SHA-256(Go-JSON(VoteMsg i))                 -> out_digests (n*32, optional)
 *   sig bit i  = crypto/ecdsa.Verify(key[key_idx[i]], h_i, r_i, s_i)
 *                                                            -> out_sig_bitmap (optional;
 *                                                               needs sig_rs n*64 BE, key_idx)
 *   msg bit i  = State.verifyMsg(view_ids[i], sequence_ids[i], digest_i) against the
 *                state state_idx[i] < n_states = (state_view_ids, state_last_seqs,
 *                32-B request digest)                        -> out_msg_bitmap (optional)
 * (pbft_impl.go:176-202; a state_idx out of range gives 0).  Bitmaps are
 * ceil(n/8) bytes, LSB-first.  A vote counts toward its state's quorum iff both
 * bits are set. */
int pbftv_flush_votes(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                      const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                      const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                      const int64_t* msg_types, const uint8_t* sig_rs, const uint32_t* key_idx, uint32_t n_states,
                      const int64_t* state_view_ids, const int64_t* state_last_seqs,
                      const uint8_t* state_req_digests, const uint32_t* state_idx, uint8_t* out_digests,
                      uint8_t* out_sig_bitmap, uint8_t* out_msg_bitmap);

/* Flushes of the other three signed messages, one GPU round
 * trip per device like pbftv_flush_votes; every output is optional (NULL = not
 * wanted; a signature bitmap needs sig_rs n*64 BE and key_idx).
 *
 * Requests (GetReq / resolveRequestMsg, pbft/network/node.go:150-177, 521-538):
 *   h_i = SHA-256(Go-JSON(RequestMsg i with sequence_ids[i]))  -> out_digests
 *   sig bit i = ecdsa.Verify(key[key_idx[i]], h_i, r_i, s_i)  -> out_sig_bitmap
 *   c_i = digest(RequestMsg i with SequenceID = assigned_seqs[i]), the
 *         StartConsensus digest (pbft_impl.go:67-73)          -> out_consensus_digests
 *                                                                (needs assigned_seqs) */
int pbftv_flush_requests(pbftv_ctx* ctx, uint64_t n, const int64_t* timestamps, const uint8_t* client_ids,
                         const uint64_t* client_id_off, const uint32_t* client_id_len, const uint8_t* operations,
                         const uint64_t* operation_off, const uint32_t* operation_len, const int64_t* sequence_ids,
                         const uint8_t* sig_rs, const uint32_t* key_idx, const int64_t* assigned_seqs,
                         uint8_t* out_digests, uint8_t* out_sig_bitmap, uint8_t* out_consensus_digests);
/* Replies (the client's reply collection, node.go:182-197 / client):
 *   h_i = SHA-256(Go-JSON(ReplyMsg i)) -> out_digests; sig bit i as above. */
int pbftv_flush_replies(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                        const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                        const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                        const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                        const uint8_t* sig_rs, const uint32_t* key_idx, uint8_t* out_digests,
                        uint8_t* out_sig_bitmap);
/* Pre-prepares (replicas, State.PrePrepare pbft_impl.go:91-109):
 *   h_i = SHA-256(Go-JSON(PrePrepareMsg i))                     -> out_digests; sig bit i
 *   q_i = digest(embedded RequestMsg i) (Hash("null") if nil)   -> out_req_digests
 *   msg bit i = verifyMsg(view_ids[i], sequence_ids[i], digest_i) with the state's
 *               ReqMsg = the embedded request: view == state_view_ids[state_idx[i]]
 *               && (last == -1 || last < sequence_ids[i]) && digest_i == hex(q_i)
 *                                                               -> out_msg_bitmap
 * (state_idx out of range -> 0). */
int pbftv_flush_preprepares(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                            const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                            const uint8_t* has_request, const int64_t* req_timestamps, const uint8_t* req_client_ids,
                            const uint64_t* req_client_id_off, const uint32_t* req_client_id_len,
                            const uint8_t* req_operations, const uint64_t* req_operation_off,
                            const uint32_t* req_operation_len, const int64_t* req_sequence_ids, const uint8_t* sig_rs,
                            const uint32_t* key_idx, uint32_t n_states, const int64_t* state_view_ids,
                            const int64_t* state_last_seqs, const uint32_t* state_idx, uint8_t* out_digests,
                            uint8_t* out_req_digests, uint8_t* out_sig_bitmap, uint8_t* out_msg_bitmap);

/* State.verifyMsg (pbft_impl.go:176-202) over n votes against one state:
 * bit i = view_ids[i] == state_view_id
 *         && (state_last_seq == -1 || state_last_seq < sequence_ids[i])
 *         && digest_got[i] (digest_got_len[i] bytes at digest_got + digest_got_off[i])
 *            is exactly the lowercase hex of req_digest (Go string compare). */
int pbftv_verify_msg_batch(int64_t state_view_id, int64_t state_last_seq, const uint8_t req_digest[32], uint64_t n,
                           const int64_t* view_ids, const int64_t* sequence_ids, const char* digest_got,
                           const uint64_t* digest_got_off, const uint32_t* digest_got_len, uint8_t* out_bitmap);

/* ---- ECDSA-P256 signatures (Go crypto/ecdsa.Verify semantics) --------- */

/* Register the replica public keys (k * 64 B, X||Y big-endian); replaces any
 * previous set.  out_valid[j] = 1 if key j is a valid P-256 point (0 <= X,Y < p
 * and on the curve); signatures naming an invalid key always fail.  Builds the
 * fixed-base comb tables on every device (one host thread per GPU).  The G
 * table is built once per GPU and width and shared by every context of the
 * process on that GPU; the key tables of one call share one allocation, and a
 * re-registration at the same width reuses it (no VRAM re-allocation).
 * Geometry: see pbftv_table_config. */
int pbftv_register_keys(pbftv_ctx* ctx, const uint8_t* pub_xy, uint32_t k, uint8_t* out_valid);

/* Incremental key changes (membership changes without a rebuild of every
 * table): pbftv_add_keys appends k keys as indices nkeys .. nkeys + k - 1 at the
 * registered geometry (PBFTV_ENOMEM if their tables do not fit);
 * pbftv_set_key replaces key `index` (< nkeys) in place.  Both need a prior
 * pbftv_register_keys.  They, and pbftv_register_keys, first wait for every
 * verify of THIS context still in flight -- on the library's streams, on
 * streams from pbftv_stream_create and on any other caller stream a *_dev
 * call was given -- so no verify reads a table, validity flag or table
 * pointer while it is rewritten.  Other contexts on the GPU are not waited
 * for (they read their own key tables).  If any device
 * fails, every device of the context drops its key set (PBFTV_ENOKEYS until
 * the next successful pbftv_register_keys), so shards never disagree on the
 * keys. */
int pbftv_add_keys(pbftv_ctx* ctx, const uint8_t* pub_xy, uint32_t k, uint8_t* out_valid);
int pbftv_set_key(pbftv_ctx* ctx, uint32_t index, const uint8_t* pub_xy, uint8_t* out_valid);

/* Comb-table geometry chosen at registration and the HBM its tables take per
 * device.  Window codes: plain W-bit windows (8, 12, 16, 20, 22, 24, 26: 256/W + 1
 * windows, 2^(W-1) entries of 64 B each) or the mixed codes 21 (5 x 22-bit +
 * 7 x 21-bit windows: 1.14 GB per key) and 29 (5 x 29 + 4 x 28: 120 GB).  The
 * pair (G, keys) is the one with the fewest windows in total (= table
 * additions per verify) whose tables fit the device's free HBM minus a 16 GiB
 * reserve for batch scratch: on a 288 GB MI355X, 100 keys -> G 29 + keys 21
 * (9 + 12 windows, 234 GB), 4 keys -> G 29 + keys 24 (5.9 GB each), 1000 keys
 * -> keys 16 (34 MiB each).  PBFTV_TABLE_BUDGET_MB caps the key tables,
 * PBFTV_GBITS / PBFTV_QBITS force a width. */
int pbftv_table_config(const pbftv_ctx* ctx, int* out_gbits, int* out_qbits, uint64_t* out_table_bytes);

/* Verify n signatures: hashes (n*32), sig_rs (n*64: r||s big-endian),
 * key_idx (n, index into the registered table).  out_bitmap: ceil(n/8) B.
 * Batches up to 2048 signatures take the one-launch latency path (inputs read
 * by the kernel straight from pinned memory).  Larger batches are split into
 * one shard per device and each shard is pipelined in chunks: DMA of the
 * caller's buffers as they are (pinned memory, e.g. from pbftv_host_alloc,
 * directly; pageable memory through the runtime's staging) on one copy
 * stream -- every key index first, then each chunk's hashes and signatures
 * back to back into up to PBFTV_HOST_SLOTS = 16 device slots -- and each chunk
 * verified as it lands, even and odd chunks on two streams so the last two
 * overlap (PBFTV_HOST_CHUNK, default 262144 signatures; the last chunk
 * PBFTV_HOST_LAST, default 131072, takes the ragged remainder). */
int pbftv_ecdsa_p256_verify_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* sig_rs,
                                  const uint32_t* key_idx, uint64_t n, uint8_t* out_bitmap);

/* Device-resident form (device index dev); hashes/sigs 16-B aligned;
 * d_bitmap: ceil(n/8) B.  Enqueued on stream, not synchronised. */
int pbftv_ecdsa_p256_verify_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes, const uint8_t* d_sig_rs,
                                      const uint32_t* d_key_idx, uint64_t n, uint8_t* d_bitmap, void* stream);

/* Verify under keys that were NEVER registered: signature i carries its own
 * public key pub_xy[64 i ..] (X||Y big-endian).  For signers outside the
 * registered set -- the clients of request and reply messages, an open set --
 * where a comb table per key (34 MiB and up) cannot pay for itself; a key
 * that signs many messages is better registered.  Semantics
 * are exactly those of pbftv_ecdsa_p256_verify_batch (0 < r, s < n, e not
 * reduced, R = u1 G + u2 Q, reject R = infinity, accept iff R.x mod n == r,
 * high-S accepted); a signature whose key is not a point of the curve with
 * 0 <= x, y < p is a 0 bit, never an error.  out_bitmap: LSB-first,
 * ceil(n/8) bytes, padding bits zero.  n = 0 returns PBFTV_OK and writes
 * nothing; n >= 2^32 is PBFTV_EINVAL.  Neither call needs, reads or disturbs
 * the registered key set (there is no PBFTV_ENOKEYS here).  The G table is
 * the width-16 one (34 MiB) of the per-GPU cache registration uses, built on
 * first use and kept while the context lives; each lane's table of its own
 * key lives in a scratch sized by the GPU's resident lanes, not by n
 * (PBFTV_VARBASE_LANES overrides the lane count).  About 18x the device time
 * of a registered verify.
 * The host form shards contiguously over the context's devices, copies in,
 * verifies and copies the bitmaps back (no chunk overlap).  The _dev form
 * (hashes/sigs/keys 16-B aligned) is enqueued on `stream` (null: the context
 * stream) and not synchronised; its in-flight work is counted by the
 * context's wait before key changes and by pbftv_dev_free like any other
 * *_dev verify. */
int pbftv_ecdsa_p256_verify_pubkey_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* sig_rs,
                                         const uint8_t* pub_xy, uint64_t n, uint8_t* out_bitmap);
int pbftv_ecdsa_p256_verify_pubkey_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes,
                                             const uint8_t* d_sig_rs, const uint8_t* d_pub_xy, uint64_t n,
                                             uint8_t* d_bitmap, void* stream);

/* The same with the keys as they travel: one format per call, key i at
 * keys + pbftv_key_bytes(key_format) * i (packed, no padding between keys).
 * The SEC1 forms are what Go's elliptic.Marshal (uncompressed) and
 * elliptic.MarshalCompressed write, decoded by the rules of SEC1 2.3.3/2.3.4
 * as go1.19 elliptic.Unmarshal / UnmarshalCompressed apply them:
 *   uncompressed  byte 0 must be 04 (the hybrid forms 06/07, 00 and every
 *                 other value are rejected), 0 <= X, Y < p, point on the curve;
 *   compressed    byte 0 must be 02 or 03, X < p, y = sqrt(X^3 - 3X + b) must
 *                 exist (about half of all X have no point), and of the two
 *                 roots the one with y mod 2 == byte 0 mod 2 is the key.
 * The square root is taken on the device (one per key; +5.6 % on the verify
 * step).  A key that fails decoding is a 0 bit, never an
 * error.  PBFTV_KEY_XY is pbftv_ecdsa_p256_verify_pubkey_batch's pub_xy.
 * Everything else -- semantics, bitmap, n = 0, n >= 2^32, no registered keys
 * needed or touched, the _dev form's 16-B aligned base pointers and stream --
 * is as stated above; an unknown key_format is PBFTV_EINVAL. */
#define PBFTV_KEY_XY                0  /* X||Y, 64 B                          */
#define PBFTV_KEY_SEC1_COMPRESSED   1  /* 02|03 || X, 33 B                    */
#define PBFTV_KEY_SEC1_UNCOMPRESSED 2  /* 04 || X || Y, 65 B                  */
uint32_t pbftv_key_bytes(int key_format);   /* 64 / 33 / 65; 0 = unknown     */
int pbftv_ecdsa_p256_verify_wirekey_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* sig_rs,
                                          const uint8_t* keys, int key_format, uint64_t n, uint8_t* out_bitmap);
int pbftv_ecdsa_p256_verify_wirekey_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes,
                                              const uint8_t* d_sig_rs, const uint8_t* d_keys, int key_format,
                                              uint64_t n, uint8_t* d_bitmap, void* stream);

/* Flushes of client-signed messages: pbftv_flush_requests / pbftv_flush_replies
 * with the signer's key carried per message (keys, key_format: as above) in
 * place of key_idx, still one GPU round trip per device -- the digests never
 * leave the device between the hash and the signature stage:
 *   sig bit i = ecdsa.Verify(decode(key i), h_i, r_i, s_i)      -> out_sig_bitmap
 * (a signature bitmap needs sig_rs and keys; n >= 2^32 with a bitmap wanted is
 * PBFTV_EINVAL).  They need no registered keys (no PBFTV_ENOKEYS) and read and
 * disturb nothing of the registered set.  Every other column and output is
 * that of the registered form. */
int pbftv_flush_requests_wirekey(pbftv_ctx* ctx, uint64_t n, const int64_t* timestamps, const uint8_t* client_ids,
                                 const uint64_t* client_id_off, const uint32_t* client_id_len,
                                 const uint8_t* operations, const uint64_t* operation_off,
                                 const uint32_t* operation_len, const int64_t* sequence_ids, const uint8_t* sig_rs,
                                 const uint8_t* keys, int key_format, const int64_t* assigned_seqs,
                                 uint8_t* out_digests, uint8_t* out_sig_bitmap, uint8_t* out_consensus_digests);
int pbftv_flush_replies_wirekey(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                                const uint8_t* client_ids, const uint64_t* client_id_off,
                                const uint32_t* client_id_len, const uint8_t* node_ids, const uint64_t* node_id_off,
                                const uint32_t* node_id_len, const uint8_t* results, const uint64_t* result_off,
                                const uint32_t* result_len, const uint8_t* sig_rs, const uint8_t* keys,
                                int key_format, uint8_t* out_digests, uint8_t* out_sig_bitmap);

/* ---- signatures as ASN.1 DER, parsed on the device ----------------------
 * Go holds a signature as the []byte that ecdsa.SignASN1 wrote and
 * ecdsa.VerifyASN1 reads.  Every call below takes that form as a signature
 * column (der, der_off, der_len) -- signature i is the der_len[i] bytes at
 * der + der_off[i] -- where the call of the same name without _der takes
 * sig_rs, and runs the parser of pbftv_ecdsa_der_to_rs on the device (one lane
 * per signature, k_der_to_rs) in the same round trip as the hash and the
 * verify.  The column follows the string-column rules above: any order,
 * shared bytes, other bytes before and between the encodings, and the offset
 * of an encoding of length 0 is not read.  A signature that does not parse
 * (or whose r or s is outside [0, 2^256)) is a 0 bit, never an error.  n = 0
 * returns PBFTV_OK and writes nothing; n >= 2^32 is PBFTV_EINVAL.  Every
 * other semantic, argument check and the PBFTV_ENOKEYS behaviour is that of
 * the r||s call of the same name.  (pbftv_qc_verify has no DER form: a
 * certificate has 3 to 67 signatures, and the host parse is noise there.)
 *
 * No encoding longer than 72 bytes parses, so only the first min(der_len[i],
 * 72) bytes of an encoding are ever read, whatever der_len[i] claims.
 *
 * pbftv_ecdsa_der_to_rs_batch_dev is the building block: d_out_rs (64 n B,
 * 16-B aligned) receives r||s or zeros, d_parsed_bitmap (may be NULL) the
 * LSB-first bitmap of the signatures that parsed (ceil(n/8) B, padding bits
 * zero).  Enqueued on `stream` (NULL: the context's stream), not synchronised;
 * it composes with any *_dev verify on the same stream, and its in-flight work
 * is counted by the context's wait before key changes and by pbftv_dev_free
 * like any other *_dev call.
 * Readability (every *_dev form here): the data buffer must be readable over
 * every 4-byte-aligned dword that holds one of the first min(der_len[i], 72)
 * bytes of an encoding, so less than 4 bytes before its first byte and past
 * that prefix -- the dword rule of pbftv_sha256_batch_dev.  Memory mapped in
 * pages (pbftv_dev_alloc / hipMalloc allocations, and ranges inside them)
 * meets it.  The host forms pad their own device copy.
 *
 * pbftv_ecdsa_p256_verify_der_batch: registered keys.  Batches up to the
 * latency-path maximum are parsed on the host (the same parser) and handed to
 * pbftv_ecdsa_p256_verify_batch, so an armed latency kernel keeps serving
 * certificates exactly as for an r||s caller.  Larger ones are split into one
 * shard per device; each shard copies its hashes, the span its encodings
 * cover, their offsets and lengths and its key indices in, normalises and
 * verifies on the device and copies its bitmap back -- simple copies, no
 * chunk pipelining (unlike pbftv_ecdsa_p256_verify_batch).  The _dev form
 * (hashes 16-B aligned) keeps the r||s column in one scratch per device that
 * the library orders across streams: *_der batches enqueued on two streams of
 * one device run one after the other, also on streams from
 * pbftv_stream_create (the r||s forms overlap there; to overlap DER batches,
 * normalise into buffers of your own with pbftv_ecdsa_der_to_rs_batch_dev and
 * call the r||s verify).
 * pbftv_ecdsa_p256_verify_wirekey_der_batch: carried keys (keys, key_format:
 * as pbftv_ecdsa_p256_verify_wirekey_batch); no registered keys needed, read
 * or disturbed. */
int pbftv_ecdsa_der_to_rs_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_data, const uint64_t* d_offsets,
                                    const uint32_t* d_lengths, uint64_t n, uint8_t* d_out_rs,
                                    uint8_t* d_parsed_bitmap /* may be NULL */, void* stream);
int pbftv_ecdsa_p256_verify_der_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* der,
                                      const uint64_t* der_off, const uint32_t* der_len, const uint32_t* key_idx,
                                      uint64_t n, uint8_t* out_bitmap);
int pbftv_ecdsa_p256_verify_der_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes, const uint8_t* d_der,
                                          const uint64_t* d_der_off, const uint32_t* d_der_len,
                                          const uint32_t* d_key_idx, uint64_t n, uint8_t* d_bitmap, void* stream);
int pbftv_ecdsa_p256_verify_wirekey_der_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* der,
                                              const uint64_t* der_off, const uint32_t* der_len, const uint8_t* keys,
                                              int key_format, uint64_t n, uint8_t* out_bitmap);
int pbftv_ecdsa_p256_verify_wirekey_der_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes,
                                                  const uint8_t* d_der, const uint64_t* d_der_off,
                                                  const uint32_t* d_der_len, const uint8_t* d_keys, int key_format,
                                                  uint64_t n, uint8_t* d_bitmap, void* stream);

/* The six flushes with the signature column as DER: the encodings travel in
 * the flush's one host->device copy, are normalised on the device after the
 * hash, and the unchanged signature stage runs on the result -- still one GPU
 * round trip per device.  A signature bitmap needs the DER column (der_off and
 * der_len; der may be NULL only if every length is 0) and key_idx / keys. */
int pbftv_flush_votes_der(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                          const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                          const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                          const int64_t* msg_types, const uint8_t* der, const uint64_t* der_off,
                          const uint32_t* der_len, const uint32_t* key_idx, uint32_t n_states,
                          const int64_t* state_view_ids, const int64_t* state_last_seqs,
                          const uint8_t* state_req_digests, const uint32_t* state_idx, uint8_t* out_digests,
                          uint8_t* out_sig_bitmap, uint8_t* out_msg_bitmap);
int pbftv_flush_preprepares_der(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                                const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                                const uint8_t* has_request, const int64_t* req_timestamps,
                                const uint8_t* req_client_ids, const uint64_t* req_client_id_off,
                                const uint32_t* req_client_id_len, const uint8_t* req_operations,
                                const uint64_t* req_operation_off, const uint32_t* req_operation_len,
                                const int64_t* req_sequence_ids, const uint8_t* der, const uint64_t* der_off,
                                const uint32_t* der_len, const uint32_t* key_idx, uint32_t n_states,
                                const int64_t* state_view_ids, const int64_t* state_last_seqs,
                                const uint32_t* state_idx, uint8_t* out_digests, uint8_t* out_req_digests,
                                uint8_t* out_sig_bitmap, uint8_t* out_msg_bitmap);
int pbftv_flush_requests_der(pbftv_ctx* ctx, uint64_t n, const int64_t* timestamps, const uint8_t* client_ids,
                             const uint64_t* client_id_off, const uint32_t* client_id_len, const uint8_t* operations,
                             const uint64_t* operation_off, const uint32_t* operation_len,
                             const int64_t* sequence_ids, const uint8_t* der, const uint64_t* der_off,
                             const uint32_t* der_len, const uint32_t* key_idx, const int64_t* assigned_seqs,
                             uint8_t* out_digests, uint8_t* out_sig_bitmap, uint8_t* out_consensus_digests);
int pbftv_flush_replies_der(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                            const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                            const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                            const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                            const uint8_t* der, const uint64_t* der_off, const uint32_t* der_len,
                            const uint32_t* key_idx, uint8_t* out_digests, uint8_t* out_sig_bitmap);
int pbftv_flush_requests_wirekey_der(pbftv_ctx* ctx, uint64_t n, const int64_t* timestamps, const uint8_t* client_ids,
                                     const uint64_t* client_id_off, const uint32_t* client_id_len,
                                     const uint8_t* operations, const uint64_t* operation_off,
                                     const uint32_t* operation_len, const int64_t* sequence_ids, const uint8_t* der,
                                     const uint64_t* der_off, const uint32_t* der_len, const uint8_t* keys,
                                     int key_format, const int64_t* assigned_seqs, uint8_t* out_digests,
                                     uint8_t* out_sig_bitmap, uint8_t* out_consensus_digests);
int pbftv_flush_replies_wirekey_der(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                                    const uint8_t* client_ids, const uint64_t* client_id_off,
                                    const uint32_t* client_id_len, const uint8_t* node_ids,
                                    const uint64_t* node_id_off, const uint32_t* node_id_len, const uint8_t* results,
                                    const uint64_t* result_off, const uint32_t* result_len, const uint8_t* der,
                                    const uint64_t* der_off, const uint32_t* der_len, const uint8_t* keys,
                                    int key_format, uint8_t* out_digests, uint8_t* out_sig_bitmap);

/* ---- Signing: deterministic ECDSA-P256 in batches ----
 * What a replica sends it signs here: Go's crypto/ecdsa.Sign over a 32-byte
 * digest with the nonce of RFC 6979 section 3.2 (HMAC-SHA256, no additional
 * data), so a (digest, key) pair always gives the same signature.  No low-S
 * normalisation, as in Go; every verify of this library accepts the result.
 *
 * pbftv_register_signing_keys takes k private keys, 32 big-endian bytes each,
 * and replaces any previous set; out_valid[j] (may be NULL) is 0 for d = 0 or
 * d >= n, and such a key signs nothing.  It waits for the context's in-flight
 * work as pbftv_register_keys does.  The keys live in device memory only: the
 * device copy is overwritten with zeros before it is freed or replaced and at
 * pbftv_close, the host staging copy before the call returns, and no call
 * copies a private key back.  The set is independent of the verify keys: no
 * call in this section needs, reads or disturbs pbftv_register_keys' set.
 * Nonces never steer a branch on the device, but the G comb entry a lane
 * loads is addressed by its nonce's digits: the GPU and whoever shares it are
 * trusted.
 *
 * The batch calls sign hashes[i] (32 B) under key skey_idx[i] into
 * out_sig_rs[i] (64 B, r||s big-endian, what the verifies take) and bit i of
 * out_ok_bitmap (LSB-first, ceil(n/8) bytes, padding bits zero; may be NULL).
 * An skey_idx out of range or naming an invalid key is never an error: that
 * row is 64 zero bytes with a 0 bit.  n = 0 returns PBFTV_OK and writes
 * nothing; n >= 2^32 is PBFTV_EINVAL; before any registration the calls
 * return PBFTV_ENOSIGNKEYS.  The host form shards contiguously over the
 * devices with plain copies.  The _dev form takes device pointers (hashes and
 * signatures 16-B aligned), enqueues on `stream` (NULL: the context's) without
 * synchronising, and is counted by the context's in-flight bookkeeping like
 * any *_dev verify, so a verify enqueued behind it on the same stream reads
 * the finished signatures with no host synchronisation in between.
 *
 * The _der forms write ASN.1 DER instead, what crypto/ecdsa.SignASN1 emits:
 * signature i in the 72-byte slot out_der + 72 i (every byte of the slot is
 * written; the _dev form wants the slots 16-B aligned), its length in
 * out_der_len[i]; a length of 0 means not signed.
 *
 * pbftv_sign_replies takes the reply columns of pbftv_digest_reply_batch and
 * does Go-JSON, SHA-256 and the signature in one round trip per device, the
 * digests staying in device memory in between; out_digests may be NULL.
 * pbftv_seal_* below return the signed messages themselves. */
int pbftv_register_signing_keys(pbftv_ctx* ctx, const uint8_t* priv, uint32_t k, uint8_t* out_valid);
int pbftv_ecdsa_p256_sign_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint32_t* skey_idx, uint64_t n,
                                uint8_t* out_sig_rs, uint8_t* out_ok_bitmap);
int pbftv_ecdsa_p256_sign_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes, const uint32_t* d_skey_idx,
                                    uint64_t n, uint8_t* d_out_sig_rs, uint8_t* d_out_ok_bitmap, void* stream);
int pbftv_ecdsa_p256_sign_der_batch(pbftv_ctx* ctx, const uint8_t* hashes, const uint32_t* skey_idx, uint64_t n,
                                    uint8_t* out_der, uint32_t* out_der_len);
int pbftv_ecdsa_p256_sign_der_batch_dev(pbftv_ctx* ctx, int dev, const uint8_t* d_hashes, const uint32_t* d_skey_idx,
                                        uint64_t n, uint8_t* d_out_der, uint32_t* d_out_der_len, void* stream);
int pbftv_sign_replies(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                       const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                       const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                       const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                       const uint32_t* skey_idx, uint8_t* out_digests, uint8_t* out_sig_rs, uint8_t* out_ok_bitmap);
int pbftv_sign_replies_der(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                           const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                           const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                           const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                           const uint32_t* skey_idx, uint8_t* out_digests, uint8_t* out_der, uint32_t* out_der_len);

/* ---- Sealing: what a replica posts, in one round trip per device ----
 * pbftv_seal_votes / _replies / _preprepares take the columns of the matching
 * pbftv_digest_*_batch (same string-column conventions: any order, shared
 * bytes, the offset of an empty string is not read).  Message i is encoded to
 * its unsigned Go-JSON preimage, hashed, signed under signing key skey_idx[i]
 * (pbftv_register_signing_keys' set) and written in its signed wire form:
 * exactly pbftv_gojson_vote_signed / _reply_signed / _preprepare_signed of the
 * same fields with that signature, non-nil.  sig_format selects the signature
 * field's bytes: PBFTV_SIG_RS, the 64 bytes r||s, or PBFTV_SIG_DER, the DER
 * bytes crypto/ecdsa.SignASN1 writes; any other value is PBFTV_EINVAL.
 *
 * Pre-prepares: the embedded request carries the client's signature
 * req_sigs[req_sig_off[i] .. + req_sig_len[i]) on the wire -- free bytes of
 * any length, a string column like the others.  req_sig_nil[i] != 0, or a NULL
 * req_sigs or req_sig_nil column (then for every message), means Go's nil
 * slice, written null; a non-nil signature of length 0 is written "".  The
 * primary's preimage embeds the unsigned request, as pbftv_gojson_preprepare
 * does.  With has_request[i] = 0 the request is null and the signature
 * columns' entry i is not read.
 *
 * out_wire receives the wire forms back to back in message order, with no
 * padding, terminator or separator; out_wire_len[i] is message i's length,
 * out_wire_off[i] the exclusive prefix sum of the lengths over the whole batch
 * (across devices too) and *out_wire_bytes their total.  A row whose skey_idx
 * is out of range or names an invalid key (or that the signer's 2^-32-rare
 * candidate exhaustion hits) is unsigned, never an error: its
 * length is 0, its ok bit 0, it writes no byte and its offset is the running
 * sum.  out_digests (n*32, the signed digests) and out_ok_bitmap (LSB-first,
 * ceil(n/8) bytes, padding bits zero) may be NULL.  A wire form is below 2^32
 * bytes.
 *
 * n = 0 returns PBFTV_OK and writes only *out_wire_bytes = 0; n >= 2^32, a
 * NULL column, skey_idx, out_wire_off, out_wire_len or out_wire_bytes (or a
 * NULL out_wire with wire_cap > 0) is PBFTV_EINVAL; without signing keys the
 * calls return PBFTV_ENOSIGNKEYS.  If the total exceeds wire_cap the call
 * returns PBFTV_ENOSPACE: *out_wire_bytes holds the size needed, out_wire_off,
 * out_wire_len, out_digests and out_ok_bitmap are filled, and nothing is
 * written to out_wire; the same call with a buffer of that size gives the
 * full result.  No trial call is needed: with T = 103 (PBFTV_SIG_RS) or 111
 * (PBFTV_SIG_DER), the signature tail  ,"signature":"<base64>"  of 64 or 72
 * bytes, message i takes at most
 *   vote         120 + 6 (digest_len + node_id_len) + T
 *   reply        102 + 6 (client_id_len + node_id_len + result_len) + T
 *   pre-prepare  189 + 6 (digest_len + req_client_id_len + req_operation_len)
 *                + T + 15 + 4 ceil(req_sig_len / 3)
 * bytes (the Go-JSON bound of its strings, 6 bytes per input byte, plus the
 * tails), and the sum over the batch is enough for wire_cap.
 *
 * Host forms only.  With several devices the shards' bytes pass through host
 * memory once more to land behind each other; with one device the blob is
 * copied straight from the device into out_wire. */
#define PBFTV_SIG_RS  0  /* r||s, 64 B                          */
#define PBFTV_SIG_DER 1  /* ASN.1 DER, 8..72 B                  */
int pbftv_seal_votes(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                     const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                     const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                     const int64_t* msg_types, const uint32_t* skey_idx, int sig_format, uint8_t* out_wire,
                     uint64_t wire_cap, uint64_t* out_wire_off, uint32_t* out_wire_len, uint64_t* out_wire_bytes,
                     uint8_t* out_digests, uint8_t* out_ok_bitmap);
int pbftv_seal_replies(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* timestamps,
                       const uint8_t* client_ids, const uint64_t* client_id_off, const uint32_t* client_id_len,
                       const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                       const uint8_t* results, const uint64_t* result_off, const uint32_t* result_len,
                       const uint32_t* skey_idx, int sig_format, uint8_t* out_wire, uint64_t wire_cap,
                       uint64_t* out_wire_off, uint32_t* out_wire_len, uint64_t* out_wire_bytes, uint8_t* out_digests,
                       uint8_t* out_ok_bitmap);
int pbftv_seal_preprepares(pbftv_ctx* ctx, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                           const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                           const uint8_t* has_request, const int64_t* req_timestamps, const uint8_t* req_client_ids,
                           const uint64_t* req_client_id_off, const uint32_t* req_client_id_len,
                           const uint8_t* req_operations, const uint64_t* req_operation_off,
                           const uint32_t* req_operation_len, const int64_t* req_sequence_ids,
                           const uint8_t* req_sigs, const uint64_t* req_sig_off, const uint32_t* req_sig_len,
                           const uint8_t* req_sig_nil, const uint32_t* skey_idx, int sig_format, uint8_t* out_wire,
                           uint64_t wire_cap, uint64_t* out_wire_off, uint32_t* out_wire_len,
                           uint64_t* out_wire_bytes, uint8_t* out_digests, uint8_t* out_ok_bitmap);

/* Quorum certificate: verify n signatures and count acceptances.
 * *out_accepted = popcount; *out_quorum = (*out_accepted >= quorum).  With
 * quorum = 2f this is the reference's prepared()/committed() count
 * (pbft_impl.go:212,227); with 2f+1 it is a PBFT certificate. */
int pbftv_qc_verify(pbftv_ctx* ctx, const uint8_t* hashes, const uint8_t* sig_rs, const uint32_t* key_idx, uint64_t n,
                    uint32_t quorum, uint8_t* out_bitmap, uint64_t* out_accepted, int* out_quorum);

#ifdef __cplusplus
}
#endif
#endif /* PBFTV_H */
