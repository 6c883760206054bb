// der.h -- ASN.1 DER ECDSA signatures -> the (r, s) layout of
// pbftv_ecdsa_p256_verify_batch, one parser for the host (der.cpp, the CPU
// harness tests/cpp/der_harness.cpp) and the device (k_der_to_rs,
// der_kernels.hip).
//
// Restates go1.19 crypto/ecdsa.VerifyASN1's parse over
// golang.org/x/crypto/cryptobyte (vendored in the Go tree):
//   input.ReadASN1(&inner, SEQUENCE) && input.Empty() &&
//   inner.ReadASN1Integer(r) && inner.ReadASN1Integer(s) && inner.Empty()
// followed by the product's range rule 0 <= r, s < 2^256 (a negative integer
// or one >= 2^256 can never pass Verify's 1 <= r, s < n test, so it is rejected
// here: rs zeroed -> 0 bit).  A zero integer parses (as in Go:
// ReadASN1Integer accepts 0) and is rejected by the verify kernels' range
// check, like any r or s >= n.
//
// readASN1 accepts a long-form length (81..84, value >= 128, no leading zero
// byte).  No encoding that uses one can pass ALL of the above, so the parser
// below rejects a long-form length where it meets it:
//   - checkASN1Integer wants a minimal two's complement, so an integer in
//     [0, 2^256) has 1..33 content bytes (33 only with a leading 00): an
//     integer with a long-form length (>= 128 content bytes) is either not
//     minimal or outside the range;
//   - hence each INTEGER is at most 2 + 33 bytes, and since nothing may follow
//     the two integers inside the SEQUENCE, its contents are at most 70 bytes:
//     its own length is short form too (a long form must encode >= 128);
//   - and since nothing may follow the SEQUENCE, the whole encoding is 8
//     (30 06 02 01 r 02 01 s) to 72 bytes.
// So the parser reads only bytes at indices below min(len, 72), whatever len
// claims.  tests/test_der_cpu.py checks this against oracle/der.py, which
// keeps the long forms: never "parsed" past 72 bytes or with a long form, and
// no reader call at index 72 or beyond.
//
// The reader R hands out the encoding's bytes; the parser never forms an
// address itself:
//   uint32_t byte(uint32_t i) const          byte i, i < min(len, 72)
//   uint32_t tail_word(int32_t i, uint32_t lo) const
//       the four bytes i .. i+3 as they lie in memory (byte i in bits 0..7),
//       with every byte at an index below lo as zero; lo <= i + 3, and
//       i + 3 < min(len, 72).  i may be negative (then lo > i).
// The host reads through a pointer (DerPtrReader); the kernel reads aligned
// dwords (DerDwordReader).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBFTV_DER_HD __host__ __device__ __forceinline__
#else
#define PBFTV_DER_HD inline
#endif

namespace pbftv {

constexpr uint32_t kDerMinBytes = 8;   // 30 06 02 01 r 02 01 s
constexpr uint32_t kDerMaxBytes = 72;  // 30 46 02 21 00 r[32] 02 21 00 s[32]

// the value bytes of one INTEGER: [begin, end) as indices into the encoding,
// the sign-padding 00 stripped, so 1 <= end - begin <= 32
struct DerInt {
  uint32_t begin, end;
};

// cryptobyte ReadASN1Integer at index *pos of the sequence that ends at index
// `end` (<= 72), with checkASN1Integer's minimality and the range rule;
// *pos moves past the integer.
template <class R>
PBFTV_DER_HD bool der_read_uint256(const R& rd, uint32_t* pos, uint32_t end, DerInt* v) {
  const uint32_t p = *pos;
  if (end - p < 2) return false;           // (p <= end always)
  const uint32_t tag = rd.byte(p), lb = rd.byte(p + 1);
  if (tag != 0x02) return false;           // (0x02: not the high-tag-number form)
  if (lb & 0x80) return false;             // long form: see the header comment
  if (lb == 0 || end - (p + 2) < lb) return false;
  uint32_t b = p + 2;
  const uint32_t e = b + lb;
  const uint32_t first = rd.byte(b);
  if (lb > 1) {
    const uint32_t second = rd.byte(b + 1);
    if ((first == 0x00 && (second & 0x80) == 0) || (first == 0xff && (second & 0x80) != 0)) return false;
    if (first == 0x00) ++b;                // the sign padding of a value with its top bit set
  }
  if (first & 0x80) return false;          // negative
  if (e - b > 32) return false;            // >= 2^256
  v->begin = b;
  v->end = e;
  *pos = e;
  return true;
}

// The parse: true iff Go's VerifyASN1 parses the len bytes behind rd and
// 0 <= r, s < 2^256; then *r and *s locate the value bytes.
template <class R>
PBFTV_DER_HD bool der_parse(const R& rd, uint64_t len, DerInt* r, DerInt* s) {
  if (len < kDerMinBytes || len > kDerMaxBytes) return false;
  const uint32_t n = (uint32_t)len;
  const uint32_t tag = rd.byte(0), lb = rd.byte(1);
  if (tag != 0x30) return false;
  if (lb & 0x80) return false;             // long form: see the header comment
  if (lb != n - 2) return false;           // the sequence ends short of the input, or input.Empty() fails
  uint32_t pos = 2;
  if (!der_read_uint256(rd, &pos, n, r)) return false;
  if (!der_read_uint256(rd, &pos, n, s)) return false;
  return pos == n;                         // inner.Empty()
}

// The value v as 32 big-endian bytes, in memory order: w[k] holds bytes
// 4k .. 4k+3 of the output (byte 4k in bits 0..7).
template <class R>
PBFTV_DER_HD void der_value_be256(const R& rd, const DerInt& v, uint32_t w[8]) {
  const int32_t at = (int32_t)v.end - 32;  // index of output byte 0 (below v.begin: a zero)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 8; ++k) {
    const int32_t i = at + 4 * k;
    w[k] = i + 3 >= (int32_t)v.begin ? rd.tail_word(i, v.begin) : 0u;
  }
}

// DER signature -> r||s: rs[0..7] = r, rs[8..15] = s as der_value_be256 lays
// them out; all zero when not parsed.  Returns "parsed".
template <class R>
PBFTV_DER_HD bool der_to_rs_words(const R& rd, uint64_t len, uint32_t rs[16]) {
  DerInt r{0, 0}, s{0, 0};
  const bool ok = der_parse(rd, len, &r, &s);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) rs[k] = 0;
  if (ok) {
    der_value_be256(rd, r, rs);
    der_value_be256(rd, s, rs + 8);
  }
  return ok;
}

// the host's reader: bytes through a pointer, nothing outside [p, p + len)
struct DerPtrReader {
  const uint8_t* p;
  uint32_t byte(uint32_t i) const { return p[i]; }
  uint32_t tail_word(int32_t i, uint32_t lo) const {
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j)
      if (i + j >= (int32_t)lo) w |= (uint32_t)p[i + j] << (8 * j);
    return w;
  }
};

// The kernel's reader (also run by the CPU harness over a recording fetch):
// the encoding begins mis (0..3) bytes into dword 0 of a sequence of 4-byte-
// aligned dwords, fetch(k) loads dword k.  Every dword it fetches holds a
// byte of the encoding that the parser asked for.
template <class F>
struct DerDwordReader {
  F fetch;
  uint32_t mis;
  PBFTV_DER_HD uint32_t byte(uint32_t i) const {
    const uint32_t a = mis + i;
    return (fetch(a >> 2) >> (8 * (a & 3u))) & 0xffu;
  }
  // The dword that holds byte i is fetched only if it also holds a byte at or
  // past lo; the next one only if one of i+1 .. i+3 lies in it.
  PBFTV_DER_HD uint32_t tail_word(int32_t i, uint32_t lo) const {
    const int32_t a = (int32_t)mis + i;            // (>= -28)
    const int32_t k = a >> 2;                      // floor
    const uint32_t sh = (uint32_t)a & 3u;
    const bool want_lo = 4 * k + 3 >= (int32_t)(mis + lo);
    const uint32_t w0 = want_lo ? fetch((uint32_t)k) : 0u;
    const uint32_t w1 = sh ? fetch((uint32_t)(k + 1)) : 0u;  // (k + 1 >= 0: it holds byte i + 3 >= lo)
    const uint32_t w = sh ? (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh)) : w0;
    const int32_t z = (int32_t)lo - i;             // leading bytes below lo: <= 3
    return z > 0 ? w & (0xffffffffu << (8 * z)) : w;
  }
};

// ---- the writer: r||s -> DER, what go's crypto/ecdsa.SignASN1 emits ----
// SEQUENCE { INTEGER r, INTEGER s }, each INTEGER minimal: leading zero bytes
// dropped (one byte stays for the value 0), a 00 pad in front when the top bit
// of the first byte is set.  Every length is short form (an INTEGER has at
// most 33 content bytes, the SEQUENCE at most 70), so the encoding is 8 to 72
// bytes.  get(i): byte i of the 64 big-endian bytes r||s; put(i, b): byte i of
// the 72-byte slot, every index 0..71 written once in rising order (zeros past
// the encoding), so a slot never keeps bytes of an earlier use.  Returns the
// encoding's length.
template <class Get, class Put>
PBFTV_DER_HD uint32_t der_write_rs(Get get, Put put) {
  uint32_t skip[2], pad[2], len[2];
  for (int v = 0; v < 2; ++v) {
    uint32_t z = 0;
    bool lead = true;
    for (uint32_t i = 0; i < 31; ++i) {  // (byte 31 always stays)
      lead = lead && get(32 * v + i) == 0;
      z += lead ? 1u : 0u;
    }
    skip[v] = z;
    pad[v] = (get(32 * v + z) & 0x80u) ? 1u : 0u;
    len[v] = pad[v] + 32 - z;
  }
  const uint32_t body = 4 + len[0] + len[1], total = 2 + body;
  uint32_t o = 0;
  put(o++, 0x30u);
  put(o++, body);
  for (int v = 0; v < 2; ++v) {
    put(o++, 0x02u);
    put(o++, len[v]);
    if (pad[v]) put(o++, 0x00u);
    for (uint32_t i = skip[v]; i < 32; ++i) put(o++, get(32 * v + i));
  }
  for (; o < kDerMaxBytes; ++o) put(o, 0x00u);
  return total;
}

// through pointers (the host, the CPU harness; the device's slots are global
// memory it addresses the same way)
PBFTV_DER_HD uint32_t der_from_rs(const uint8_t rs[64], uint8_t out[72]) {
  return der_write_rs([&](uint32_t i) -> uint32_t { return rs[i]; },
                      [&](uint32_t i, uint32_t b) { out[i] = (uint8_t)b; });
}

// r||s words -> 64 bytes on any host
inline void der_store_rs(const uint32_t rs[16], uint8_t* out_rs) {
  for (int k = 0; k < 16; ++k)
    for (int j = 0; j < 4; ++j) out_rs[4 * k + j] = (uint8_t)(rs[k] >> (8 * j));
}

}  // namespace pbftv
