/* seal_baseline.c -- what a caller did before pbftv_seal_votes, as a compiled
 * caller does it (tools/seal_bench.py): after pbftv_digest_vote_batch and
 * pbftv_ecdsa_p256_sign_der_batch, one core walks the batch and builds each
 * signed wire form with pbftv_gojson_vote_signed, back to back into one
 * buffer.  The encoder is passed in, so this file links nothing.  Returns the
 * total; off / len as pbftv_seal_votes fills them (a row with der_len 0 is
 * unsigned: length 0). */
#include <stdint.h>

typedef uint64_t (*vote_signed_fn)(int64_t, int64_t, const char*, uint64_t, const char*, uint64_t, int64_t,
                                   const uint8_t*, uint64_t, int, uint8_t*, uint64_t);

uint64_t seal_baseline_votes(vote_signed_fn encode, uint64_t n, const int64_t* view_ids, const int64_t* sequence_ids,
                             const uint8_t* digests, const uint64_t* digest_off, const uint32_t* digest_len,
                             const uint8_t* node_ids, const uint64_t* node_id_off, const uint32_t* node_id_len,
                             const int64_t* msg_types, const uint8_t* der, const uint32_t* der_len, uint8_t* out,
                             uint64_t cap, uint64_t* off, uint32_t* len) {
  uint64_t pos = 0;
  for (uint64_t i = 0; i < n; ++i) {
    off[i] = pos;
    len[i] = 0;
    if (der_len[i] == 0) continue;
    const uint64_t k = encode(view_ids[i], sequence_ids[i], (const char*)digests + digest_off[i], digest_len[i],
                              (const char*)node_ids + node_id_off[i], node_id_len[i], msg_types[i], der + 72 * i,
                              der_len[i], 0, pos < cap ? out + pos : out, pos < cap ? cap - pos : 0);
    len[i] = (uint32_t)k;
    pos += k;
  }
  return pos;
}
