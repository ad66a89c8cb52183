// Capture bytes -> LSB-first bits, shared by the kernels that read a serial capture
// (cvd_capture.hip, cvd_sweep.hip; formats: include/cvd.h CVD_CAPTURE_*).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// per-byte bit reversal: MSB-first bytes -> LSB-first
__device__ __forceinline__ uint32_t lsb_first(uint32_t x) { return __builtin_bswap32(__builtin_bitreverse32(x)); }

// bit 0 of each of a dword's four bytes -> bits 0..3
__device__ __forceinline__ uint32_t byte_bits4(uint32_t x) {
  x &= 0x01010101u;
  x |= x >> 7;
  x |= x >> 14;
  return x & 0xFu;
}

}  // namespace
