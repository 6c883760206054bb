// wire.h -- the signed wire forms' lengths, bounds and offsets, stated once for
// the seal kernels (seal_kernels.hip), the host side of pbftv_seal_* and the
// CPU test harness (tests/cpp/wire_harness.cpp, g++).
//
// A sealed message is gojson_enc.h's *_signed encoding of its fields.  Its
// unsigned preimage (vote(), reply(), preprepare()) ends in '}'; the signed
// form replaces that brace with  ,"signature":<bytes field>}  so
//   signed length = preimage length + kSigKeyLen + bytes_field_len(signature)
// and a pre-prepare with a request grows by the same tail once more, inside
// the embedded request (request_signed: the client's signature).
// A []byte field (put_bytes) is  null  for Go's nil slice, else a quoted
// padded base64 string: 2 + 4 * ceil(n / 3) bytes.
#pragma once
#include <stdint.h>

#include "gojson_enc.h"

namespace pbftv {
namespace wire {

constexpr uint32_t kSigKeyLen = 13;  // strlen(",\"signature\":")
constexpr uint32_t kSigRsLen = 64;   // r||s
constexpr uint32_t kSigDerMax = 72;  // der.h: the longest ecdsa.SignASN1 output for P-256

PBFTV_GJ uint64_t bytes_field_len(uint64_t n, bool is_nil) { return is_nil ? 4 : 2 + 4 * ((n + 2) / 3); }

// vote_signed / reply_signed from the encoder's preimage length (sig non-nil)
PBFTV_GJ uint64_t signed_len(uint64_t pre_len, uint64_t sig_len) {
  return pre_len + kSigKeyLen + bytes_field_len(sig_len, false);
}

// preprepare_signed likewise; req_sig_* are read only where has_req
PBFTV_GJ uint64_t preprepare_signed_len(uint64_t pre_len, bool has_req, uint64_t req_sig_len, bool req_sig_nil,
                                        uint64_t sig_len) {
  return signed_len(pre_len, sig_len) + (has_req ? kSigKeyLen + bytes_field_len(req_sig_len, req_sig_nil) : 0);
}

// Upper bounds from the column lengths alone (sig_max: kSigRsLen or kSigDerMax)
PBFTV_GJ uint64_t vote_signed_bound(uint64_t dgn, uint64_t nidn, uint64_t sig_max) {
  return signed_len(gojson::vote_bound(dgn, nidn), sig_max);
}
PBFTV_GJ uint64_t reply_signed_bound(uint64_t cidn, uint64_t nidn, uint64_t resn, uint64_t sig_max) {
  return signed_len(gojson::reply_bound(cidn, nidn, resn), sig_max);
}
PBFTV_GJ uint64_t preprepare_signed_bound(uint64_t dgn, uint64_t rcidn, uint64_t ropn, uint64_t req_sig_len,
                                          uint64_t sig_max) {
  return preprepare_signed_len(gojson::preprepare_bound(dgn, rcidn, ropn), true, req_sig_len, false, sig_max);
}

// The offsets of a batch: the exclusive prefix sum of its lengths in 64 bits;
// returns the total.  The host reference of the device scan; a later shard's
// offsets are its own plus the totals of the shards before it.
inline uint64_t scan_offsets(const uint32_t* len, uint64_t n, uint64_t* off) {
  uint64_t t = 0;
  for (uint64_t i = 0; i < n; ++i) {
    off[i] = t;
    t += len[i];
  }
  return t;
}

// The device scan's geometry (seal_kernels.hip): kScanBlock lengths per
// workgroup in the first and third launch; the second launch is one workgroup
// that walks the block sums kScanChunk at a time with a running carry.
constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanChunk = 256;

}  // namespace wire
}  // namespace pbftv
