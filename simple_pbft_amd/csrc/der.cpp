// der.cpp -- ASN.1 DER ECDSA signatures -> the (r, s) layout of
// pbftv_ecdsa_p256_verify_batch on the host: the parser of der.h (go1.19
// crypto/ecdsa.VerifyASN1's parse with Go's strictness, shared with the
// device normaliser k_der_to_rs) read through a pointer.
#include <cstdint>
#include <cstring>

#include "der.h"

extern "C" {

int pbftv_ecdsa_der_to_rs(const uint8_t* der, uint64_t der_len, uint8_t* out_rs) {
  if (out_rs == nullptr || (der == nullptr && der_len != 0)) return -1;  // PBFTV_EINVAL
  uint32_t rs[16];
  const bool ok = pbftv::der_to_rs_words(pbftv::DerPtrReader{der}, der_len, rs);
  pbftv::der_store_rs(rs, out_rs);
  return ok ? 1 : 0;
}

int64_t pbftv_ecdsa_der_to_rs_batch(const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths,
                                    uint64_t n, uint8_t* out_rs) {
  if (n == 0) return 0;
  if (offsets == nullptr || lengths == nullptr || out_rs == nullptr) return -1;
  if (data == nullptr)
    for (uint64_t i = 0; i < n; ++i)
      if (lengths[i] != 0) return -1;  // PBFTV_EINVAL: encodings promised but no bytes
  int64_t parsed = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const int r = pbftv_ecdsa_der_to_rs(data ? data + offsets[i] : nullptr, data ? lengths[i] : 0, out_rs + 64 * i);
    if (r < 0) return r;
    parsed += r;
  }
  return parsed;
}

}  // extern "C"
