// Captured bitstream -> received-word buffer (cvd_pack_windows, include/cvd.h) for gfx950:
// cuts a device-resident serial capture into windows, at every candidate symbol phase, and
// writes them in the interleaved 16-byte-chunk layout cvd_generate writes, so that
// cvd_detect / cvd_trace / cvd_parity_detect run on streams they did not generate.
//
// The work is a funnel shift plus a transposition: a window's words are contiguous in the
// capture, while the output keeps the 16-byte chunks of neighbouring sequences contiguous.
// A tile is kSeqs = 64 sequences x kChunks = 32 chunks (32 KiB of output), staged through
// LDS so that both sides of a wave's traffic are wide and contiguous:
//   stage  per sequence one row of kRowU4 = 33 aligned 16-byte pieces of the capture (the
//          tile's 4,096 bits for n <= 2, 3,840 for n = 3, plus the alignment slack and the
//          funnel's second word), consecutive lanes on consecutive pieces (528 contiguous
//          bytes per row; BYTES format: 16 capture bytes per lane, 4,224 contiguous bytes
//          per row, packed to 16 bits each), bounds-checked against the buffer's 16-byte
//          pieces, normalised to LSB-first dwords (MSB: a per-byte bit reversal) and
//          written to a row of odd dword stride;
//   emit   lane (s, c) builds chunk c of sequence s from its row: per word two dword LDS
//          reads and one v_alignbit (shift counts 0..31, so a shift of 0 or 32 never
//          arises), masked to the steps below N; a wave's 64 lanes are 64 neighbouring
//          sequences of one chunk row: one contiguous 1-KiB store.
// For n = 3 a layout word holds 30 capture bits: word w starts at bit o + 30 w.  One tile
// per block, the tiles of a window in neighbouring blocks (a block that loops over four
// consecutive tiles, to re-read the lines two tiles share from its own CU's caches, measured
// 4-6% slower).  No scratch; 33.8 KiB of LDS, four blocks per CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSeqs = 64;                  // sequences per tile (one wave's store: 64 chunks = 1 KiB)
constexpr int kChunks = 32;                // 16-byte chunks per sequence and tile
constexpr int kRowU4 = kChunks + 1;        // 16-byte (128-bit) pieces staged per row
constexpr int kRowDw = 4 * kRowU4;         // dwords per row
constexpr int kRowStride = kRowDw + 1;     // odd: lanes on neighbouring rows hit different banks
constexpr int kBatch = 4;                  // global loads a lane keeps in flight while staging
constexpr int64_t kMaxBlocksPerLaunch = 1 << 22;   // 2^30 threads per launch

struct PackArgs {
  const uint4* cap;
  int64_t nu4;          // readable 16-byte pieces of the capture
  int64_t start, stride;
  int32_t n_phase;
  int64_t N;            // steps per window
  int64_t nchunks;      // ceil(W / 4)
  int64_t nseq;         // nwin * n_phase
  uint4* out;
  int64_t pitch, q0;
  int64_t ctiles;       // tiles along a window: ceil(nchunks / kChunks)
  int64_t block0;       // first block of this launch
};

template <int n, int format>
__global__ __launch_bounds__(kBlock) void pack_windows_kernel(PackArgs a) {
  constexpr int SPW = 32 / n, BPW = SPW * n;   // steps and capture bits per layout word
  __shared__ uint32_t rows[kSeqs * kRowStride];
  __shared__ int64_t win_bit[kSeqs];           // first capture bit of each sequence's window
  const int tid = threadIdx.x;
  const int64_t blk = a.block0 + blockIdx.x;
  const int64_t s0 = (blk / a.ctiles) * kSeqs;
  const int64_t ct = blk % a.ctiles;
  const int nrows = (int)(a.nseq - s0 < kSeqs ? a.nseq - s0 : kSeqs);
  if (tid < nrows) {
    const int64_t s = s0 + tid;
    // window s / n_phase, phase s % n_phase (n_phase is 1..3: constant divisors)
    const int64_t w = a.n_phase == 1 ? s : a.n_phase == 2 ? s / 2 : s / 3;
    win_bit[tid] = a.start + w * a.stride + (s - w * a.n_phase);
  }
  __syncthreads();
  const int64_t c0 = ct * kChunks;                            // first chunk of the tile
  const int64_t tile_bits = (int64_t)(4 * BPW) * c0;          // capture bits before the tile
  // ---- stage: row r = 128-bit pieces (win_bit[r] + tile_bits) >> 7 ... + kRowU4 ----------
  if constexpr (format != CVD_CAPTURE_BYTES) {
    const int total = nrows * kRowU4;
    for (int i0 = tid; i0 < total; i0 += kBlock * kBatch) {
      uint4 v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kBlock;
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (i < total) {
          const int r = i / kRowU4, col = i - r * kRowU4;
          const int64_t g = ((win_bit[r] + tile_bits) >> 7) + col;
          if (g < a.nu4) v[u] = a.cap[g];
        }
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kBlock;
        if (i < total) {
          const int r = i / kRowU4, col = i - r * kRowU4;
          uint32_t* d = rows + r * kRowStride + 4 * col;
          if constexpr (format == CVD_CAPTURE_MSB) {
            d[0] = lsb_first(v[u].x); d[1] = lsb_first(v[u].y); d[2] = lsb_first(v[u].z); d[3] = lsb_first(v[u].w);
          } else {
            d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
          }
        }
      }
    }
  } else {
    // one bit per byte: a 128-bit piece of the stream is 128 bytes; a lane packs 16 of
    // them into one halfword of the row
    constexpr int kRowHw = 2 * kRowDw;
    const int total = nrows * kRowHw;
    typedef uint16_t __attribute__((may_alias)) row_hw;
    row_hw* rows16 = reinterpret_cast<row_hw*>(rows);
    for (int i0 = tid; i0 < total; i0 += kBlock * kBatch) {
      uint4 v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kBlock;
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (i < total) {
          const int r = i / kRowHw, h = i - r * kRowHw;
          const int64_t g = ((win_bit[r] + tile_bits) >> 7) * 8 + h;
          if (g < a.nu4) v[u] = a.cap[g];
        }
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int i = i0 + u * kBlock;
        if (i < total) {
          const int r = i / kRowHw, h = i - r * kRowHw;
          rows16[r * (2 * kRowStride) + h] = (uint16_t)(byte_bits4(v[u].x) | (byte_bits4(v[u].y) << 4) |
                                                        (byte_bits4(v[u].z) << 8) | (byte_bits4(v[u].w) << 12));
        }
      }
    }
  }
  __syncthreads();
  // ---- emit: lane (s, c) -> chunk c0 + c of sequence s0 + s ---------------------------
  for (int j = tid; j < kSeqs * kChunks; j += kBlock) {
    const int s = j & (kSeqs - 1), c = j / kSeqs;
    const int64_t chunk = c0 + c;
    if (s < nrows && chunk < a.nchunks) {
      const uint32_t off = (uint32_t)((win_bit[s] + tile_bits) & 127);   // tile's first bit in the row
      const uint32_t* row = rows + s * kRowStride;
      uint32_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t b = off + (uint32_t)(BPW * (4 * c + e));   // < 128 + 32 * 128: dwords b >> 5 (+1) < kRowDw
        uint32_t x = __builtin_amdgcn_alignbit(row[(b >> 5) + 1], row[b >> 5], b & 31u);
        const int64_t left = a.N - (4 * chunk + e) * SPW;           // steps of this word and after
        if (left < SPW) x = left > 0 ? x & ((1u << (uint32_t)(n * left)) - 1u) : 0u;
        else if constexpr (BPW < 32) x &= (1u << BPW) - 1u;
        o[e] = x;
      }
      a.out[chunk * a.pitch + a.q0 + s0 + s] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

#define HIP_CHECK(x)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      cvd::set_error(std::string("HIP error '") + hipGetErrorString(e_) + "' at " #x);     \
      return CVD_E_HIP;                                                                   \
    }                                                                                     \
  } while (0)

int invalid(const char* what) {
  cvd::set_error(std::string("pack_windows: ") + what);
  return CVD_E_INVALID;
}

}  // namespace

extern "C" int cvd_pack_windows(const void* d_capture, int64_t nbits, int32_t format, int32_t n, int64_t N,
                                int64_t start, int64_t stride, int64_t nwin, int32_t n_phase, uint32_t* d_r,
                                int64_t pitch, int64_t q0, void* stream) {
  if (n < 1 || n > 3) return invalid("n must be 1..3");
  if (n_phase < 1 || n_phase > n) return invalid("n_phase must be 1..n");
  if (N < 0 || start < 0 || stride <= 0 || nwin < 0 || nbits < 0) return invalid("needs N, start, nwin, nbits >= 0 and stride > 0");
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES)
    return invalid("unknown capture format");
  int64_t nseq, qend;
  if (__builtin_mul_overflow(nwin, (int64_t)n_phase, &nseq) || __builtin_add_overflow(q0, nseq, &qend))
    return invalid("q0 + nwin * n_phase overflows int64");
  if (q0 < 0 || pitch < qend) return invalid("needs 0 <= q0 and q0 + nwin * n_phase <= pitch");
  const int spw = 32 / n;
  const int64_t W = N / spw + (N % spw != 0), nchunks = W / 4 + (W % 4 != 0);
  int64_t tmp;
  if (__builtin_mul_overflow(nchunks, pitch, &tmp) || __builtin_mul_overflow(tmp, (int64_t)16, &tmp))
    return invalid("buffer size overflows int64");
  if (nwin > 0) {
    // the last window's last phase ends at start + (nwin - 1) * stride + (n_phase - 1) + N * n
    int64_t end, len;
    if (__builtin_mul_overflow(nwin - 1, stride, &end) || __builtin_add_overflow(end, start, &end) ||
        __builtin_add_overflow(end, (int64_t)(n_phase - 1), &end) || __builtin_mul_overflow(N, (int64_t)n, &len) ||
        __builtin_add_overflow(end, len, &end))
      return invalid("window positions overflow int64");
    if (end > nbits) return invalid("a window does not lie inside [0, nbits)");
  }
  if (nwin == 0 || N == 0) return CVD_OK;
  if (!d_capture || !d_r || ((uintptr_t)d_capture & 15) || ((uintptr_t)d_r & 15))
    return invalid("d_capture and d_r must be non-null and 16-byte aligned");
  PackArgs a{};
  a.cap = static_cast<const uint4*>(d_capture);
  const int64_t nbytes = format == CVD_CAPTURE_BYTES ? nbits : nbits / 8 + (nbits % 8 != 0);
  a.nu4 = nbytes / 16 + (nbytes % 16 != 0);
  a.start = start; a.stride = stride; a.n_phase = n_phase; a.N = N; a.nchunks = nchunks; a.nseq = nseq;
  a.out = reinterpret_cast<uint4*>(d_r); a.pitch = pitch; a.q0 = q0;
  a.ctiles = (nchunks + kChunks - 1) / kChunks;
  const int64_t stiles = (nseq + kSeqs - 1) / kSeqs;
  int64_t nblocks;
  if (__builtin_mul_overflow(stiles, a.ctiles, &nblocks)) return invalid("tile count overflows int64");
  using K = void (*)(PackArgs);
  static const K kern[3][3] = {
      {pack_windows_kernel<1, CVD_CAPTURE_LSB>, pack_windows_kernel<1, CVD_CAPTURE_MSB>, pack_windows_kernel<1, CVD_CAPTURE_BYTES>},
      {pack_windows_kernel<2, CVD_CAPTURE_LSB>, pack_windows_kernel<2, CVD_CAPTURE_MSB>, pack_windows_kernel<2, CVD_CAPTURE_BYTES>},
      {pack_windows_kernel<3, CVD_CAPTURE_LSB>, pack_windows_kernel<3, CVD_CAPTURE_MSB>, pack_windows_kernel<3, CVD_CAPTURE_BYTES>}};
  for (int64_t b0 = 0; b0 < nblocks; b0 += kMaxBlocksPerLaunch) {
    a.block0 = b0;
    const unsigned grid = (unsigned)std::min<int64_t>(kMaxBlocksPerLaunch, nblocks - b0);
    hipLaunchKernelGGL(kern[n - 1][format], dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    HIP_CHECK(hipGetLastError());
  }
  return CVD_OK;
}
