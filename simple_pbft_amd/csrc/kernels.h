// kernels.h -- host-side launch wrappers for the gfx950 kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "qc_mail.h"

namespace pbftv {

// ---- ECDSA-P256 (p256_kernels.hip) ----
// Comb tables: geometry code w (p256_algo.h CombGeom: W-bit windows, or the
// mixed 21 / 29); table_bytes(w) per base (8: 264 KiB, 16: 34 MiB, 21:
// 1.14 GB, 22: 1.61 GB, 24: 5.9 GB, 26: 21.5 GB, 29: 120 GB).
size_t table_bytes(int w);
int table_windows(int w);  // windows = table entries added per scalar
// (G, key) geometry pairs with instantiated verify kernels
// (split by G width into the instantiation units p256_verify_g*.hip)
#define PBFTV_COMBOS_G29(X) X(29, 24) X(29, 22) X(29, 21) X(29, 20) X(29, 16)
#define PBFTV_COMBOS_G26(X) X(26, 24) X(26, 22) X(26, 21) X(26, 20) X(26, 16)
#define PBFTV_COMBOS_G24(X) X(24, 24) X(24, 22) X(24, 20) X(24, 16)
#define PBFTV_COMBOS_SMALL(X) X(20, 20) X(16, 16) X(16, 12) X(16, 8) X(8, 8)
#define PBFTV_COMBOS(X) PBFTV_COMBOS_G29(X) PBFTV_COMBOS_G26(X) PBFTV_COMBOS_G24(X) PBFTV_COMBOS_SMALL(X)
#define PBFTV_TABLE_WIDTHS(X) X(8) X(12) X(16) X(20) X(21) X(22) X(24) X(26) X(29)
struct TableScratch {
  void* bases;
  void* lbuf;
  void* hbuf;
  void* small_scratch;
  void* entry_scratch;
  uint64_t entry_lanes;
};
struct TableScratchSizes {
  size_t bases, lbuf, hbuf, small_scratch, entry_scratch;
  uint64_t entry_lanes;
};
TableScratchSizes table_scratch_sizes(int w, uint32_t nbases);
// Build nb tables (G first when with_g) of width w; table b is written at
// tabs[b] (a device array of nb pointers to table_bytes(w) each); keys_le:
// {x[8], y[8]} LE words per key, key0 = first key of this launch; valid[key]
// written for every key built.
hipError_t launch_build_tables(int w, const uint32_t* keys_le, uint32_t key0, uint32_t nb, int with_g,
                               uint32_t* valid, uint32_t* const* tabs, TableScratch& sc, hipStream_t st);
// stage 1 -> stage 2 records (verify_kernels.h SigRec: 128 B per signature) and
// the prefix-product scratch of stage 1's batched inversion
size_t ecdsa_record_bytes(uint64_t n);
int scalar_batch(uint64_t n);
size_t scalar_prefix_bytes(uint64_t n);
// key order of a batch (stage 0 -> stage 1): per-key totals and claim
// counters in the key-sort header; total == nullptr: arrival order
struct KeyOrder {
  const uint32_t* total;
  uint32_t* claim;
  uint32_t nkeys;
};
// stage 1: inputs in arrival order; record of signature i written at its
// place in key order (placed by stage 1 itself from ko) or at i
hipError_t launch_ecdsa_scalars(const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx, uint64_t n,
                                const uint32_t* key_valid, uint32_t nkeys, void* rec, void* prefix,
                                const KeyOrder& ko, hipStream_t st);
// stage 2: (wg, wq) one of PBFTV_COMBOS; qtabs = device array of the nkeys
// key tables' addresses (width wq each, one allocation per key).
// okb == nullptr: records in arrival order, LSB-first bitmap (ceil(n/8) B)
// written directly; else one byte per signature at its batch index (okb, n B)
// and launch_pack_bits builds the bitmap.
// cuflag: the device's certificate flags (kCuFlagWords, zeroed; null: the
// comb never yields to an armed certificate on its CU, verify_kernels.h)
hipError_t launch_ecdsa_comb(int wg, int wq, const void* rec, uint64_t n, const uint32_t* gtab,
                             const uint32_t* const* qtabs,
                             uint8_t* bitmap, uint8_t* okb, const uint32_t* cuflag, hipStream_t st);
constexpr uint32_t kCuFlagWords = 4096;  // one word per (XCC, SE, SH, CU)
// stage 0 (optional): per-key totals for the key order (scratch:
// key_sort_scratch_bytes = a header of key_sort_header_bytes, which must be
// ZERO when the scratch is first used and is left zero by every batch).
// parity: the caller's batch counter for this scratch (alternates the header's
// two counter sets; any sequence of values that alternates is fine).  *out is
// what stage 1 needs.
bool key_sort_wanted(uint64_t n, uint32_t nkeys);
size_t key_sort_header_bytes();
size_t key_sort_scratch_bytes(uint64_t n, uint32_t nkeys);
hipError_t launch_key_count(const uint32_t* key_idx, uint64_t n, uint32_t nkeys, void* scratch, uint32_t parity,
                            KeyOrder* out, hipStream_t st);
hipError_t launch_pack_bits(const uint8_t* okb, uint64_t n, uint8_t* bitmap, hipStream_t st);
// latency path for small batches: one wave per signature (scalars, per-window
// points, butterfly sum, check) in one launch.  Output: okbytes[i] (one byte per
// signature) when okbytes != nullptr, else bit i of bitmap set/cleared by word
// atomics (bitmap need not be zeroed; its word-aligned 4-byte span is touched).
// argument packs of the per-geometry launchers (verify_kernels.h)
struct CombArgs {
  const void* rec;
  uint64_t n;
  const uint32_t* gtab;
  const uint32_t* const* qtabs;
  uint8_t* bitmap;
  uint8_t* okb;
  const uint32_t* cuflag;
};
struct WaveArgs {
  const uint8_t* hashes;
  const uint8_t* sigs;
  const uint32_t* key_idx;
  uint64_t n;
  const uint32_t* key_valid;
  uint32_t nkeys;
  const uint32_t* gtab;
  const uint32_t* const* qtabs;
  uint8_t* bitmap;
  uint8_t* okbytes;
  bool one_wave;  // the quad schedule (one 64-thread workgroup per signature) even where rows would serve
};
// one_wave: a workgroup of one wave per signature -- beside a batch that
// holds every wave slot, such a workgroup starts in the first slot a finished
// batch block frees, where a row-schedule workgroup (5-8 waves) waits for
// several on one CU (pbftv_api.cpp launch_range)
hipError_t launch_ecdsa_wave(int wg, int wq, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx,
                             uint64_t n, const uint32_t* key_valid, uint32_t nkeys, const uint32_t* gtab,
                             const uint32_t* const* qtabs, uint8_t* bitmap, uint8_t* okbytes, hipStream_t st,
                             bool one_wave = false);
// batches up to this size take the latency path (env PBFTV_WAVE_MAX overrides; 0 disables)
uint64_t wave_path_max();
// The latency path's result bytes (okbytes): bit 0 = the verdict; the
// launched row kernel (k_ecdsa_rows) sets kRowsExact when the signature took
// its exact rerun (a doubling or cancellation in the row tree, a live window
// with two zero digits, r + n < p); the armed row kernel writes 2 instead
// (the host reruns the certificate with a launch).  Counted by pbftv_qc_counters.
constexpr int kRowsExact = 4;

// The latency path's mailbox (QcMail) and its protocol: qc_mail.h
struct ArmArgs {
  QcMail* mail;
  uint32_t want;       // the request sequence number this launch serves
  uint64_t budget;     // wall-clock ticks before it gives up
  const uint32_t* key_valid;
  uint32_t nkeys;
  const uint32_t* gtab;
  const uint32_t* const* qtabs;
  uint32_t spin;       // between polls: 0 = s_sleep, 1 = none, k >= 2 = k dependent VALU ops
  uint32_t halt;       // the mailbox's halt word at arming: any other value cancels
  uint64_t* relay;     // wide kernel (kQcCap waves): device word {number, n}, zeroed before launch; null: narrow
  uint32_t stamps;     // 1: each serving wave writes its GPU timestamps (pbftv_qc_stamps*; PBFTV_QC_STAMPS=1)
  int slot;            // its armed stream slot: the expired word and live words it writes (QcMail)
  uint32_t slots;      // narrow row-schedule kernel: signature slots armed (<= kQcSlots; one workgroup each)
  uint32_t* cuflag;    // the device's certificate flags (null: none); a serving workgroup raises its CU's word
  uint32_t cuyield;    // 2: also the word of the CU sharing its instruction cache
};
hipError_t launch_ecdsa_wave_armed(int wg, int wq, const ArmArgs& a, hipStream_t st);

// ---- ECDSA-P256 under unregistered keys (p256_varbase.hip, varbase.h) ----
// Every signature carries its key: a column of varbase_key_bytes(key_format)
// bytes each (0: unknown format), 16-B aligned, in one of include/pbftv.h's
// PBFTV_KEY_* formats -- X||Y big-endian (64 B), or SEC1 compressed (33 B) /
// uncompressed (65 B), decoded by sec1.h.  launch_varbase_keys checks the
// keys into aux (varbase_aux_bytes:
// validity words, identity indices -- what launch_ecdsa_scalars takes as
// key_valid / key_idx with nkeys = n, arrival order -- and the keys in
// Montgomery form); launch_varbase then verifies the stage-1 records against
// the width-16 G table, `lanes` signatures at a time (varbase_lanes: the
// resident lanes for a device of `cus` compute units, or PBFTV_VARBASE_LANES;
// tab: varbase_table_bytes(lanes) of scratch), and writes the LSB-first bitmap.
constexpr int kVarbaseGBits = 16;
size_t varbase_aux_bytes(uint64_t n);
const uint32_t* varbase_valid(const void* aux, uint64_t n);
const uint32_t* varbase_index(const void* aux, uint64_t n);
uint64_t varbase_lanes(int cus);
size_t varbase_table_bytes(uint64_t lanes);
constexpr int kVarbaseKeyXY = 0, kVarbaseKeySec1Compressed = 1, kVarbaseKeySec1Uncompressed = 2;  // = PBFTV_KEY_*
uint32_t varbase_key_bytes(int key_format);
hipError_t launch_varbase_keys(const uint8_t* keys, int key_format, uint64_t n, void* aux, hipStream_t st);
hipError_t launch_varbase(const void* rec, const void* aux, uint64_t n, const uint32_t* gtab, void* tab,
                          uint64_t lanes, uint8_t* bitmap, hipStream_t st);

// ---- DER signatures -> r||s (der_kernels.hip, der.h) ----
// Signature i is the lengths[i] bytes at data + offsets[i] (a string column:
// any order, overlaps and other bytes between the encodings allowed; the
// offset of an encoding of length 0 is not read).  out_rs: 64 B per signature,
// 16-B aligned, r||s big-endian or zeros where Go's VerifyASN1 parse or the
// range 0 <= r, s < 2^256 rejects the encoding; parsed (may be null): the
// LSB-first bitmap of those that parsed, ceil(n/8) B, padding bits zero.
// Reads only 4-byte-aligned dwords that hold one of the first
// min(lengths[i], 72) bytes of an encoding.  n < 2^32.
hipError_t launch_der_to_rs(const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                            uint8_t* out_rs, uint8_t* parsed, hipStream_t st);

// ---- ECDSA-P256 signing (p256_sign.hip, sign.h) ----
// One batch is the three stages in order on one stream: nonce (RFC 6979 DRBG,
// k^-1), comb (k*G over the width-16 G table, r), tail (s, the r||s rows, the
// ok bitmap).  keys: 8 LE words per private key, key_valid: one word per key
// (sign_key_words / sign_key_valid make them on the host); rec:
// sign_record_bytes(n) of scratch that holds the nonces between the stages and
// is cleared of them by the tail.  out_rs: 64 B per signature, 16-B aligned,
// zeros where skey_idx is out of range or names an invalid key; okbits (may be
// null): LSB-first, ceil(n/8) B, padding bits zero.  n < 2^32.
struct SignArgs {
  const uint8_t* hashes;
  const uint32_t* skey_idx;
  const uint32_t* keys;
  const uint32_t* key_valid;
  uint32_t nkeys;
  uint64_t n;
  const uint32_t* gtab;
  void* rec;
  uint8_t* out_rs;
  uint8_t* okbits;
};
constexpr int kSignStageNonce = 0, kSignStageComb = 1, kSignStageTail = 2, kSignStages = 3;
size_t sign_record_bytes(uint64_t n);
bool sign_key_valid(const uint8_t be[32]);  // 0 < d < n
void sign_key_words(const uint8_t be[32], uint32_t out[8]);
hipError_t launch_sign_stage(int stage, const SignArgs& a, hipStream_t st);
// r||s rows -> minimal DER (der.h's writer) in 72-byte slots (out_der 8-B
// aligned, every byte of a slot written) and their lengths; 0 and a zero slot
// where okbits (not null here) has a 0
hipError_t launch_sign_der(const uint8_t* rs, const uint8_t* okbits, uint64_t n, uint8_t* out_der, uint32_t* out_len,
                           hipStream_t st);

// ---- SHA-256 (sha256_kernels.hip) ----
// data must stay readable 4 bytes past every message end (device allocations are padded).
// order: optional permutation (lane -> message), used for block-count bucketing.
// If expected != nullptr, also writes the LSB-first match bitmap (ceil(n/8) B).
hipError_t launch_sha256(const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths, const uint32_t* order,
                         uint64_t n, uint8_t* digests, const uint8_t* expected, uint8_t* bitmap, hipStream_t st);
// Sort messages by block count on the device (counting sort): order[n] out.
size_t sha256_order_scratch_bytes(uint64_t n);
hipError_t launch_sha256_order(const uint32_t* lengths, uint64_t n, uint32_t* order, void* scratch, hipStream_t st);

// ---- Go-JSON preimages on the device (gojson_kernels.hip) ----
// Column-wise message fields (device pointers, n entries each); a string
// column is a byte blob with per-message offset and length.
struct StrCol {
  const uint8_t* data;
  const uint64_t* off;
  const uint32_t* len;
};
struct RequestCols {
  const int64_t* ts;
  StrCol cid, op;
  const int64_t* seq;
};
struct VoteCols {
  const int64_t* view;
  const int64_t* seq;
  StrCol digest, node;
  const int64_t* type;
};
struct ReplyCols {
  const int64_t* view;
  const int64_t* ts;
  StrCol cid, node, result;
};
struct PrePrepareCols {
  const int64_t* view;
  const int64_t* seq;
  StrCol digest;
  const uint8_t* has_req;  // 0: requestMsg is nil (request columns still hold n entries)
  RequestCols req;
};
// consensus states a vote batch is checked against (State.verifyMsg)
struct StateCols {
  const int64_t* view;
  const int64_t* last_seq;
  const uint8_t* req_digest;  // 32 B per state
  const uint32_t* idx;        // per vote: its state
  uint32_t n;
};
// Message i's preimage is written at out + slot[i] (slot sized by the
// gojson_enc.h bound), its length to out_len[i].  launch_gojson_vote also
// writes msg_ok[i] = verifyMsg result when msg_ok != nullptr.
hipError_t launch_gojson_request(const RequestCols& c, uint64_t n, const uint64_t* slot, uint8_t* out,
                                 uint32_t* out_len, hipStream_t st);
hipError_t launch_gojson_vote(const VoteCols& c, uint64_t n, const uint64_t* slot, uint8_t* out, uint32_t* out_len,
                              const StateCols& s, uint8_t* msg_ok, hipStream_t st);
hipError_t launch_gojson_reply(const ReplyCols& c, uint64_t n, const uint64_t* slot, uint8_t* out, uint32_t* out_len,
                               hipStream_t st);
hipError_t launch_gojson_preprepare(const PrePrepareCols& c, uint64_t n, const uint64_t* slot, uint8_t* out,
                                    uint32_t* out_len, hipStream_t st);
// pre-prepare flush: preimage i at slot[i], its embedded request's ("null" if
// nil) at slot[n + i]; lengths likewise (out_len has 2n entries)
hipError_t launch_gojson_preprepare_pair(const PrePrepareCols& c, uint64_t n, const uint64_t* slot, uint8_t* out,
                                         uint32_t* out_len, hipStream_t st);
// verifyMsg of pre-prepares against their states, the digest field compared
// with the digest of the message's own request (req_digests, 32 B per message)
hipError_t launch_preprepare_verify(const int64_t* view, const int64_t* seq, const StrCol& digest,
                                   const uint8_t* req_digests, const StateCols& s, uint64_t n, uint8_t* msg_ok,
                                   hipStream_t st);

// ---- Sealed wire forms (seal_kernels.hip, wire.h) ----
// The signatures of a batch as the signer left them: signature i is the len[i]
// bytes (len == nullptr: 64) at sig + stride * i -- r||s rows (stride 64) or
// the DER writer's slots (stride 72) and lengths -- and counts only where
// okbits (LSB-first, not null) has a 1.
struct SealSigs {
  const uint8_t* sig;
  uint32_t stride;
  const uint32_t* len;
  const uint8_t* okbits;
};
// the clients' signatures inside pre-prepares: a string column and one nil
// byte per message (read only where has_req)
struct SealReqSigs {
  StrCol col;
  const uint8_t* nil;
};
// out_len[i] = the signed wire length of message i from the encoder's preimage
// length pre_len[i] (wire.h), 0 where its ok bit is 0.  has_req == nullptr:
// votes and replies (rq is not read); else pre-prepares.
hipError_t launch_seal_lengths(const uint32_t* pre_len, const SealSigs& s, const uint8_t* has_req,
                               const SealReqSigs& rq, uint64_t n, uint32_t* out_len, hipStream_t st);
// off[i] = len[0] + .. + len[i-1] in 64 bits, *total = their sum: three
// launches in stream order (no workgroup waits on another); scratch:
// seal_scan_scratch_bytes(n).  n < 2^32.
size_t seal_scan_scratch_bytes(uint64_t n);
hipError_t launch_seal_offsets(const uint32_t* len, uint64_t n, void* scratch, uint64_t* off, uint64_t* total,
                               hipStream_t st);
// message i's *_signed encoding (gojson_enc.h) to blob + off[i], exactly
// len[i] bytes (none where len[i] == 0); dump: kSealDumpBytes that take what a
// wrong length would have put past a message's end (never read)
constexpr uint32_t kSealDumpBytes = 32;
hipError_t launch_seal_votes(const VoteCols& c, const SealSigs& s, uint64_t n, const uint64_t* off,
                             const uint32_t* len, uint8_t* blob, uint8_t* dump, hipStream_t st);
hipError_t launch_seal_replies(const ReplyCols& c, const SealSigs& s, uint64_t n, const uint64_t* off,
                               const uint32_t* len, uint8_t* blob, uint8_t* dump, hipStream_t st);
hipError_t launch_seal_preprepares(const PrePrepareCols& c, const SealSigs& s, const SealReqSigs& rq, uint64_t n,
                                   const uint64_t* off, const uint32_t* len, uint8_t* blob, uint8_t* dump,
                                   hipStream_t st);

}  // namespace pbftv
