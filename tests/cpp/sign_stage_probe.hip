// sign_stage_probe.hip -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_sign_stages.py).
//
// The signer's stage kernels one at a time, on records the test writes.  This
// file includes p256_sign.hip as a translation unit and launches through its
// own launch_sign_stage / launch_sign_der, so the kernels that run here are
// the library's k_sign_nonce, k_sign_comb, k_sign_tail (with sign_slow behind
// its real call) and k_sign_der: the same source, the same blocks, launch
// bounds and register budgets, compiled with the product library's flags --
// not a probe kernel of sign.h's functions as in sign_probe.hip.  Built to
// tests/cpp/libsign_stage_probe.so; it does not link libpbftv.so and the
// product never loads it.
//
// The 128-byte record between the stages (SignRec) as 32 LE words per row:
// words 0..7 k, 8..15 k^-1, 16 state (0 none, 1 nonce ready, 2 r ready, 3 the
// walk met), 17 candidate index, 18..19 zero, 20..27 r, 28..31 unused.
//
// Every entry point takes host arrays, allocates, copies, launches on the null
// stream, synchronises, copies back and frees, and returns the hipError_t
// (-1: an argument out of range).  Arrays, n rows each unless said otherwise:
//   hashes     32 B per row, big-endian
//   skey_idx   one word per row
//   keys       8 LE words per key (nkeys keys), then one validity word per key
//              -- the layout pbftv_register_signing_keys uploads
//   rec        in and out: n + 1 records; the last one is a guard the kernels
//              must not touch
//   out_rs     out: n + 1 rows of 64 B, set to 0xA5 on the device first
//   okbits     out: ceil(n / 8) + 8 bytes, set to 0xEE on the device first;
//              null: the tail is launched without a bitmap
// sstp_tail refuses (-1) a record in state "walk met" whose key index is out
// of range or names an invalid key: the comb cannot produce that pairing and
// the tail would load a key from outside the array.
// sstp_set_g_table uploads the width-16 comb table of G once (the CPU harness
// builds it); sstp_release frees it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../simple_pbft_amd/csrc/p256_sign.hip"

using namespace pbftv;

namespace {

uint32_t* g_gtab = nullptr;

constexpr uint32_t kRecWords = 32, kStateWord = 16;
static_assert(sizeof(SignRec) == 4 * kRecWords, "the record the test writes is the kernels' SignRec");

struct Bufs {
  void* p[8] = {};
  int n = 0;
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
  ~Bufs() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
};

// stages [first, last] in order on the null stream
int run_stages(int first, int last, const uint8_t* hashes, const uint32_t* skey_idx, const uint32_t* keys,
               uint32_t nkeys, uint64_t n, uint32_t* rec, uint8_t* out_rs, uint8_t* okbits) {
  if (n == 0 || n > 1024 || nkeys == 0 || !rec || !g_gtab) return -1;
  const bool keyed = first == kSignStageNonce || last == kSignStageTail;
  const bool tail = last == kSignStageTail;
  if (keyed && (!hashes || !skey_idx || !keys)) return -1;
  if (tail && !out_rs) return -1;
  if (first == kSignStageTail) {
    const uint32_t* valid = keys + 8 * (size_t)nkeys;
    for (uint64_t i = 0; i < n; ++i)
      if (rec[kRecWords * i + kStateWord] == kSignMet && (skey_idx[i] >= nkeys || valid[skey_idx[i]] == 0)) return -1;
  }
  Bufs b;
  uint8_t *dh = nullptr, *drs = nullptr, *dok = nullptr;
  uint32_t *dki = nullptr, *dkeys = nullptr, *drec = nullptr;
  const size_t rec_bytes = 4 * kRecWords * (size_t)(n + 1), rs_bytes = 64 * (size_t)(n + 1),
               ok_bytes = (size_t)(n + 7) / 8 + 8, key_bytes = 36 * (size_t)nkeys;
  hipError_t e = b.alloc((void**)&drec, rec_bytes);
  if (e == hipSuccess) e = hipMemcpy(drec, rec, rec_bytes, hipMemcpyHostToDevice);
  if (keyed) {
    if (e == hipSuccess) e = b.alloc((void**)&dh, 32 * (size_t)n);
    if (e == hipSuccess) e = b.alloc((void**)&dki, 4 * (size_t)n);
    if (e == hipSuccess) e = b.alloc((void**)&dkeys, key_bytes);
    if (e == hipSuccess) e = hipMemcpy(dh, hashes, 32 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dki, skey_idx, 4 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dkeys, keys, key_bytes, hipMemcpyHostToDevice);
  }
  if (tail) {
    if (e == hipSuccess) e = b.alloc((void**)&drs, rs_bytes);
    if (e == hipSuccess) e = hipMemset(drs, 0xA5, rs_bytes);
    if (okbits) {
      if (e == hipSuccess) e = b.alloc((void**)&dok, ok_bytes);
      if (e == hipSuccess) e = hipMemset(dok, 0xEE, ok_bytes);
    }
  }
  const SignArgs a{dh, dki, dkeys, dkeys ? dkeys + 8 * (size_t)nkeys : nullptr, nkeys, n, g_gtab, drec, drs, dok};
  for (int stage = first; stage <= last && e == hipSuccess; ++stage) e = launch_sign_stage(stage, a, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(rec, drec, rec_bytes, hipMemcpyDeviceToHost);
  if (tail) {
    if (e == hipSuccess) e = hipMemcpy(out_rs, drs, rs_bytes, hipMemcpyDeviceToHost);
    if (okbits && e == hipSuccess) e = hipMemcpy(okbits, dok, ok_bytes, hipMemcpyDeviceToHost);
  }
  return (int)e;
}

}  // namespace

extern "C" {

uint64_t sstp_g_table_bytes() { return CombGeom<kVbGBits>::kBytes; }
uint32_t sstp_record_bytes() { return (uint32_t)sign_record_bytes(1); }

int sstp_set_g_table(const uint32_t* table) {
  if (!table) return -1;
  hipError_t e = hipSuccess;
  if (!g_gtab) e = hipMalloc(&g_gtab, CombGeom<kVbGBits>::kBytes);
  if (e == hipSuccess) e = hipMemcpy(g_gtab, table, CombGeom<kVbGBits>::kBytes, hipMemcpyHostToDevice);
  return (int)e;
}

void sstp_release() {
  if (g_gtab) (void)hipFree(g_gtab);
  g_gtab = nullptr;
}

// k_sign_nonce: hashes and keys -> k, k^-1, state and candidate index of every record
int sstp_nonce(const uint8_t* hashes, const uint32_t* skey_idx, const uint32_t* keys, uint32_t nkeys, uint64_t n,
               uint32_t* rec) {
  return run_stages(kSignStageNonce, kSignStageNonce, hashes, skey_idx, keys, nkeys, n, rec, nullptr, nullptr);
}

// k_sign_comb: the records alone (it reads no hash and no key; nkeys is not used)
int sstp_comb(uint64_t n, uint32_t* rec) {
  return run_stages(kSignStageComb, kSignStageComb, nullptr, nullptr, nullptr, 1, n, rec, nullptr, nullptr);
}

// k_sign_tail: records -> r||s rows, the ok bitmap, k and k^-1 wiped
int sstp_tail(const uint8_t* hashes, const uint32_t* skey_idx, const uint32_t* keys, uint32_t nkeys, uint64_t n,
              uint32_t* rec, uint8_t* out_rs, uint8_t* okbits) {
  return run_stages(kSignStageTail, kSignStageTail, hashes, skey_idx, keys, nkeys, n, rec, out_rs, okbits);
}

// the three stages in order, as sign_on_device launches them
int sstp_chain(const uint8_t* hashes, const uint32_t* skey_idx, const uint32_t* keys, uint32_t nkeys, uint64_t n,
               uint32_t* rec, uint8_t* out_rs, uint8_t* okbits) {
  return run_stages(kSignStageNonce, kSignStageTail, hashes, skey_idx, keys, nkeys, n, rec, out_rs, okbits);
}

// k_sign_der: rs (n rows), okbits (ceil(n / 8) B) -> out_der: n + 1 slots of 72 B, out_len: n + 4 words, both set
// to 0xA5 on the device first
int sstp_der(const uint8_t* rs, const uint8_t* okbits, uint64_t n, uint8_t* out_der, uint32_t* out_len) {
  if (n == 0 || n > 1024 || !rs || !okbits || !out_der || !out_len) return -1;
  Bufs b;
  uint8_t *drs = nullptr, *dok = nullptr, *dder = nullptr;
  uint32_t* dlen = nullptr;
  const size_t der_bytes = 72 * (size_t)(n + 1), len_bytes = 4 * (size_t)(n + 4), ok_bytes = (size_t)(n + 7) / 8;
  hipError_t e = b.alloc((void**)&drs, 64 * (size_t)n);
  if (e == hipSuccess) e = b.alloc((void**)&dok, ok_bytes);
  if (e == hipSuccess) e = b.alloc((void**)&dder, der_bytes);
  if (e == hipSuccess) e = b.alloc((void**)&dlen, len_bytes);
  if (e == hipSuccess) e = hipMemcpy(drs, rs, 64 * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dok, okbits, ok_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dder, 0xA5, der_bytes);
  if (e == hipSuccess) e = hipMemset(dlen, 0xA5, len_bytes);
  if (e == hipSuccess) e = launch_sign_der(drs, dok, n, dder, dlen, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_der, dder, der_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_len, dlen, len_bytes, hipMemcpyDeviceToHost);
  return (int)e;
}

}  // extern "C"
