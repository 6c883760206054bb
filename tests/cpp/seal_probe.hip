// seal_probe.hip -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_seal.py).
//
// The offsets stage of the seal calls alone (seal_kernels.hip's three scan
// launches, compiled here with the product library's flags) on lengths the
// test chooses: sums past 2^32 cannot be reached through messages in a test's
// time, so this is where the 64-bit carries of the scan reach the device code.
// Writes no wire bytes.  Built to tests/cpp/libseal_probe.so; it does not link
// libpbftv.so and the product never loads it.
//
// sealp_offsets takes host arrays, allocates, copies, launches on a stream of
// its own, synchronises and frees, and returns the hipError_t (-1: n out of
// range).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../simple_pbft_amd/csrc/seal_kernels.hip"

extern "C" {

int sealp_offsets(const uint32_t* len, uint64_t n, uint64_t* out_off, uint64_t* out_total) {
  if (n == 0 || n >> 32) return -1;
  uint32_t* d_len = nullptr;
  uint64_t *d_off = nullptr, *d_total = nullptr;
  void* d_scan = nullptr;
  hipStream_t st = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&d_len, 4 * n);
  if (e == hipSuccess) e = hipMalloc(&d_off, 8 * n);
  if (e == hipSuccess) e = hipMalloc(&d_total, 8);
  if (e == hipSuccess) e = hipMalloc(&d_scan, pbftv::seal_scan_scratch_bytes(n));
  if (e == hipSuccess) e = hipMemcpyAsync(d_len, len, 4 * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = pbftv::launch_seal_offsets(d_len, n, d_scan, d_off, d_total, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_off, d_off, 8 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_total, d_total, 8, hipMemcpyDeviceToHost, st);
  if (st) {
    const hipError_t s = hipStreamSynchronize(st);
    if (e == hipSuccess) e = s;
  }
  (void)hipFree(d_len);
  (void)hipFree(d_off);
  (void)hipFree(d_total);
  (void)hipFree(d_scan);
  if (st) (void)hipStreamDestroy(st);
  return (int)e;
}

uint32_t sealp_scan_block(void) { return pbftv::wire::kScanBlock; }
uint32_t sealp_scan_chunk(void) { return pbftv::wire::kScanChunk; }

}  // extern "C"
