// qc_mail.h -- the latency path's mailbox: its layout, the host's writer and
// the armed kernels' reader, stated once.  The host (pbftv_api.cpp) posts a
// certificate with qc_post; the armed servers (verify_kernels.h
// k_ecdsa_wave_armed, k_ecdsa_rows_armed) poll, test and decode it with the
// reader below over a wave's snapshot; tests/cpp/qc_mail_harness.cpp runs both
// sides on the host.  Compiled by hipcc and by g++; includes no HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef PBFTV_HD  // (fe29.h's convention)
#if defined(__HIPCC__)
#define PBFTV_HD __host__ __device__ __forceinline__
#define PBFTV_HDM __host__ __device__  // member functions
#define PBFTV_UNROLL _Pragma("unroll")
#else
#define PBFTV_HD static inline
#define PBFTV_HDM
#define PBFTV_UNROLL
#endif
#endif

namespace pbftv {

// The latency path's mailbox in pinned coherent host memory: a 64-B header,
// then the inputs of up to cap signatures (hashes cap*32, r||s cap*64, key
// indices cap*4) and one result byte per signature.  The host writes the
// inputs, n and then bell = the request's sequence number; an armed kernel
// (k_ecdsa_wave_armed) waiting for that number serves it; stop = seq cancels
// the armed kernel, which then reports expired = seq (verify_kernels.h); so
// does any change of halt (a disarm, or the process-wide quiesce of a GPU,
// pbftv_api.cpp).  Two armed kernels can be resident at once (a rotation's
// successor beside its predecessor, one per armed stream), so each armed
// stream slot has its OWN expired word and its own live words (each wave's
// first request number once it is resident): two kernels leaving at once
// (a halt bump) cannot overwrite each other's report.
// The first kQcSlots signatures are also written to their own 3-line slot
// (slot_off): line 0 = {tag, n, key, 0, hash[32], 0, 0, 0, tag}, line 1 =
// {tag, 0, 0, 0, r[32], 0, 0, 0, tag}, line 2 likewise with s; the tags (the
// request number) are written after their line's data, the last dword first.
struct QcMail {
  uint32_t bell, n, stop, expired_s0, cap, halt, expired_s1, pad[9];  // (stop and halt: read by the kernel, kQcHdr*)
  static constexpr uint32_t kQcSlots = 8;
  static constexpr uint32_t kQcCap = 128;  // signatures per call up to which the mailbox is laid out at cap = 128
  static constexpr int kArmSlots = 2;      // armed stream slots (pbftv_api.cpp Device::qstream)
  // the expired word of armed stream slot s
  PBFTV_HDM uint32_t* expired(int s) { return s ? &expired_s1 : &expired_s0; }
  static constexpr size_t slot_off(uint32_t i) { return 64 + 192 * (size_t)i; }
  // each armed wave's first request number once it is resident (4 B per
  // wave), per armed stream slot
  static constexpr size_t live_off(int s = 0) { return 64 + 192 * (size_t)kQcSlots + 4 * (size_t)kQcCap * s; }
  // one verdict byte per signature, right after the live words: with the
  // header and the slot lines in the mailbox's FIRST 4-KiB page, so a
  // certificate of <= kQcSlots touches one page of it (one TLB entry on the
  // host, one translation on the GPU, both warm from the polling)
  static constexpr size_t res_off(uint32_t = kQcCap) { return live_off(kArmSlots); }
  // the input arrays of signatures kQcSlots.. (and of every signature on the
  // launched path), after cap verdict bytes
  static constexpr size_t arrays_off(uint32_t cap = kQcCap) {
    return (res_off() + (cap > kQcCap ? cap : kQcCap) + 63) & ~(size_t)63;
  }
  static constexpr size_t hashes_off(uint32_t cap = kQcCap) { return arrays_off(cap); }
  static constexpr size_t sigs_off(uint32_t cap) { return arrays_off(cap) + 32 * (size_t)cap; }
  static constexpr size_t keys_off(uint32_t cap) { return arrays_off(cap) + 96 * (size_t)cap; }
  // diagnostics: per armed wave (slots and helpers), its {wall clock, shader
  // clock} when it saw its request and when it wrote its verdict (pbftv_qc_stamps)
  static constexpr size_t stamps_off(uint32_t cap) { return (keys_off(cap) + 4 * (size_t)cap + 63) & ~(size_t)63; }
  static constexpr size_t bytes(uint32_t cap) { return stamps_off(cap) + 32 * (size_t)kQcCap + 64; }
};

// ---- the format's numbers ----
constexpr int kQcLineDwords = 16;                                 // a 64-B line
constexpr int kQcSlotLines = 3;                                   // hash, r, s
constexpr int kQcTagFirst = 0, kQcTagLast = kQcLineDwords - 1;    // the request number, in every line
constexpr int kQcLine0N = 1, kQcLine0Key = 2;                     // line 0 alone: n and the key index
constexpr int kQcLineData = 4;                                    // a line's 8 data dwords start here
// A slot wave polls in ONE wave-wide load: lanes below this one read the
// dwords of its slot, the others the header's from dword 0.
constexpr int kQcPollHeaderLane = kQcSlotLines * kQcLineDwords;
constexpr int kQcHdrStop = (int)(offsetof(QcMail, stop) / 4), kQcHdrHalt = (int)(offsetof(QcMail, halt) / 4);
static_assert(sizeof(QcMail) == 64 && QcMail::slot_off(1) - QcMail::slot_off(0) == 4 * kQcPollHeaderLane, "layout");
static_assert(kQcHdrStop == 2 && kQcHdrHalt == 5 && kQcPollHeaderLane + kQcHdrHalt < 64, "the header words a wave polls");
// A helper (slots kQcSlots..) reads its inputs from the arrays in one
// wave-wide load: these lanes the hash, r || s and (every lane from it) the key.
constexpr int kQcHelpHash = 0, kQcHelpSig = 8, kQcHelpKey = 24;
// The relay word wave 0 announces a wide certificate to the helpers with:
// {number, n}, zero before the first one (request numbers are never 0), and
// n = kQcRelayLeft when wave 0 has left.
constexpr uint32_t kQcRelayLeft = 0xFFFFFFFFu;
PBFTV_HD uint64_t qc_relay_pack(uint32_t number, uint32_t n) { return ((uint64_t)n << 32) | number; }
PBFTV_HD uint32_t qc_relay_number(uint64_t r) { return (uint32_t)r; }
PBFTV_HD uint32_t qc_relay_n(uint64_t r) { return (uint32_t)(r >> 32); }

// ---- the reader ----
// Snap: v[l] is the dword lane l loaded (on the device a wave's register read
// with readlane, every l a constant after unrolling; on the host an array).

// byte offset in the mailbox of the dword lane `lane` of slot b's wave polls
PBFTV_HD size_t qc_poll_off(uint32_t b, uint32_t lane) {
  return lane < (uint32_t)kQcPollHeaderLane ? QcMail::slot_off(b) + 4 * lane : 4 * (lane - kQcPollHeaderLane);
}
// A line is read as one snapshot of the host's cache line and x86 stores
// become visible in order, so a line whose two tags match holds its data;
// requiring both also covers a read that tore a line in two.
template <class Snap>
PBFTV_HD bool qc_line_is(const Snap& v, int line, uint32_t want) {
  return v[line * kQcLineDwords + kQcTagFirst] == want && v[line * kQcLineDwords + kQcTagLast] == want;
}
template <class Snap>
PBFTV_HD uint32_t qc_slot_n(const Snap& v) { return v[kQcLine0N]; }  // (of a ready slot)
// Slot b holds request `want`: line 0 carries n; a slot past n needs only
// that line (the host writes no inputs there), a slot below n all three.
template <class Snap>
PBFTV_HD bool qc_slot_ready(const Snap& v, uint32_t b, uint32_t want) {
  return qc_line_is(v, 0, want) && (b >= qc_slot_n(v) || (qc_line_is(v, 1, want) && qc_line_is(v, 2, want)));
}
// the server waiting for `want`, armed at header halt word `halt`, is cancelled
template <class Snap>
PBFTV_HD bool qc_cancelled(const Snap& v, uint32_t want, uint32_t halt) {
  return v[kQcPollHeaderLane + kQcHdrStop] == want || v[kQcPollHeaderLane + kQcHdrHalt] != halt;
}
// 8 big-endian dwords from lane `at` on -> little-endian words
template <class Snap>
PBFTV_HD void qc_be256(const Snap& v, int at, uint32_t w[8]) {
  PBFTV_UNROLL for (int t = 0; t < 8; ++t) w[7 - t] = __builtin_bswap32(v[at + t]);
}
template <class Snap>
PBFTV_HD void qc_slot_decode(const Snap& v, uint32_t e[8], uint32_t r[8], uint32_t s[8], uint32_t& key) {
  qc_be256(v, kQcLineData, e);
  qc_be256(v, kQcLineDwords + kQcLineData, r);
  qc_be256(v, 2 * kQcLineDwords + kQcLineData, s);
  key = v[kQcLine0Key];
}
// A helper's source: byte offset of the dword its lane loads for signature b
// (the armed path's layout is always cap = kQcCap: the host lays the mailbox
// out otherwise only after a disarm), and the decode of that snapshot.
PBFTV_HD size_t qc_helper_off(uint32_t b, uint32_t lane) {
  return lane < (uint32_t)kQcHelpSig   ? QcMail::hashes_off(QcMail::kQcCap) + 32 * (size_t)b + 4 * (lane - kQcHelpHash)
         : lane < (uint32_t)kQcHelpKey ? QcMail::sigs_off(QcMail::kQcCap) + 64 * (size_t)b + 4 * (lane - kQcHelpSig)
                                       : QcMail::keys_off(QcMail::kQcCap) + 4 * (size_t)b;
}
template <class Snap>
PBFTV_HD void qc_helper_decode(const Snap& v, uint32_t e[8], uint32_t r[8], uint32_t s[8], uint32_t& key) {
  qc_be256(v, kQcHelpHash, e);
  qc_be256(v, kQcHelpSig, r);
  qc_be256(v, kQcHelpSig + 8, s);
  key = v[kQcHelpKey];
}

// ---- the writer (host) ----
// (always inlined: a certificate after an idle second pays for every cold line
// of code on its path, and an out-of-line copy is one more)
// the inputs of signatures [lo, hi) into the mailbox arrays (laid out for cap)
__attribute__((always_inline)) inline void qc_write_arrays(uint8_t* mail, uint32_t cap, const uint8_t* hashes, const uint8_t* sig_rs,
                            const uint32_t* key_idx, uint64_t lo, uint64_t hi) {
  memcpy(mail + QcMail::hashes_off(cap) + 32 * lo, hashes + 32 * lo, 32 * (hi - lo));
  memcpy(mail + QcMail::sigs_off(cap) + 64 * lo, sig_rs + 64 * lo, 64 * (hi - lo));
  memcpy(mail + QcMail::keys_off(cap) + 4 * lo, key_idx + lo, 4 * (hi - lo));
}
// Post request `cur` of na signatures (the first na of the caller's arrays)
// to the slots of an armed server: each line's data, then its last tag, then
// its first (release stores), lines 1 and 2 before line 0, n in every slot's
// line 0 (a slot past na: line 0 only; its wave reads na and waits for the
// next), and the bell last.  The caller has written the helpers' inputs
// (qc_write_arrays of signatures kQcSlots..na-1) BEFORE this.
__attribute__((always_inline)) inline void qc_post(uint8_t* mail, uint32_t cur, uint32_t na, const uint8_t* hashes, const uint8_t* sig_rs,
                    const uint32_t* key_idx) {
  auto tag = [cur](uint32_t* line) {
    __atomic_store_n(line + kQcTagLast, cur, __ATOMIC_RELEASE);
    __atomic_store_n(line + kQcTagFirst, cur, __ATOMIC_RELEASE);
  };
  for (uint32_t i = 0; i < QcMail::kQcSlots; ++i) {
    uint32_t* const l0 = reinterpret_cast<uint32_t*>(mail + QcMail::slot_off(i));
    if (i < na) {
      memcpy(l0 + kQcLineData, hashes + 32 * i, 32);
      memcpy(l0 + kQcLineDwords + kQcLineData, sig_rs + 64 * i, 32);
      memcpy(l0 + 2 * kQcLineDwords + kQcLineData, sig_rs + 64 * i + 32, 32);
      l0[kQcLine0Key] = key_idx[i];
      tag(l0 + kQcLineDwords);
      tag(l0 + 2 * kQcLineDwords);
    }
    l0[kQcLine0N] = na;
    tag(l0);
  }
  __atomic_store_n(&reinterpret_cast<QcMail*>(mail)->bell, cur, __ATOMIC_RELEASE);  // inputs and n are in: ring
}

}  // namespace pbftv
