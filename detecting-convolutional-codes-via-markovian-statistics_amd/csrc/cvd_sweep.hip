// Blind parity-check sweep of a captured bitstream (cvd_parity_sweep, include/cvd.h) for
// gfx950: the satisfaction count of every one of the 2^B parity templates over a window of
// B = n (span + 1) capture bits, from one histogram and one Walsh-Hadamard transform:
//   hist[f][x] = #{anchors a of phase f whose B-bit word is x}
//   sat[f][mask] = (T + WHT(hist[f])[mask]) / 2,  WHT(h)[mask] = sum_x h[x] (-1)^popcount(mask & x)
// All of it is integer: the result does not depend on launch shape or atomic order.
//
// Histogram (sweep_hist_kernel<n, format, mode>), one phase per blockIdx.y, blocks of 1,024
// threads looping over tiles of kTileU4 = 512 aligned 16-byte pieces of the capture (65,536
// capture bits):
//   stage    consecutive lanes load consecutive pieces (BYTES format: 16 capture bytes per
//            lane, packed to a halfword), bounds-checked against the buffer's 16-byte
//            pieces, normalised to LSB-first dwords as in cvd_capture.hip, into LDS, with
//            one piece of overlap for the words that begin in the tile's last dword;
//   extract  a lane takes dwords tid, tid + 1024 of the tile: two neighbouring LDS dwords
//            and one v_alignbit per word that begins in its dword (for n = 3 the first
//            such bit differs from dword to dword), one atomic add per word.
// Regimes (where they meet: B = 15 | 16 and B = 21 | 22, measured):
//   B <= 15  the block's 2^B x u32 histogram is in LDS beside the 8-KiB tile (B = 15:
//            136 KiB of the CU's 160 KiB, one block per CU; B <= 14: two or more), LDS
//            atomics, and at the end one global atomic per non-zero bin into d_work;
//   16..21   the bins no longer fit one CU: blockIdx.z = one of 2^(B-15) parts of 2^15 bins;
//            a block extracts every word of its tiles and counts in LDS those whose top
//            B - 15 bits are its part.  The extraction is repeated 2^(B-15) times, the
//            atomics are not: 2^30 words take 0.84 / 3.0 / 11.8 ms at B = 16 / 18 / 20,
//            against 39.5 ms of global atomics at every B;
//   B = 22   128 parts would take 47 ms: global u32 atomics straight into d_work.
// A constant capture sends every anchor to one bin; atomics keep that correct.
//
// WHT + finalise (sweep_wht_kernel), i32 exact since every partial sum is a signed count of
// at most T <= 2^31 - 1 anchors:
//   B <= 15  one block per phase holds the whole 2^B x i32 vector in LDS;
//   B >= 16  two passes of 32-KiB LDS tiles: stages 0..12 on contiguous tiles of 2^13,
//            stages 13..B-1 on strided tiles of 2^(B-13) rows x 16 neighbouring columns.
// The last pass adds (T + w) >> 1 into d_sat, one thread per entry, no atomics.  No scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_internal.h"

namespace {

constexpr int kBlock = 1024;
constexpr int kTileU4 = 512;                 // 16-byte pieces per tile
constexpr int kTileDw = 4 * kTileU4;         // dwords whose words a tile emits
constexpr int kStageDw = kTileDw + 4;        // staged: one piece of overlap
constexpr int kLdsMaxB = 15;                 // largest B with the histogram / whole WHT in LDS
constexpr int kMaxB = 22;
constexpr int kGlobalMinB = 22;              // smallest B on global atomics
constexpr int kWhtTileLog = 13;              // passes of the global WHT: 2^13 x i32 = 32 KiB
constexpr int kWhtColsLog = 4;               // strided pass: 16 neighbouring columns (64 B)
constexpr int kMaxGridX = 1024;

struct HistArgs {
  const uint4* cap;
  int64_t nu4;          // readable 16-byte pieces of the capture
  int64_t first;        // capture bit of anchor 0, phase 0
  int64_t T;
  int32_t B;
  int64_t g0;           // first piece of tile 0
  int64_t ntiles;
  uint32_t* hist;       // [n_phase][2^B]
};

// mode: kGlobal = global atomics; kLdsWhole = the whole histogram in LDS; kLdsPart = bins
// [blockIdx.z 2^15, +2^15) in LDS, the words of the other parts skipped
enum { kGlobal = 0, kLdsWhole = 1, kLdsPart = 2 };

template <int n, int format, int mode>
__global__ __launch_bounds__(kBlock) void sweep_hist_kernel(HistArgs a) {
  constexpr bool kLds = mode != kGlobal;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* tile = smem;                     // kStageDw
  uint32_t* lh = smem + kStageDw;            // min(2^B, 2^15) (kLds)
  const int tid = threadIdx.x;
  const int64_t first = a.first + blockIdx.y;              // this phase's first and last word
  const int64_t last = first + (int64_t)n * (a.T - 1);
  const uint32_t mask = (1u << a.B) - 1u;
  const uint32_t bins = mode == kLdsPart ? 1u << kLdsMaxB : 1u << a.B;   // bins of this block
  const uint32_t part = mode == kLdsPart ? blockIdx.z : 0u;
  uint32_t* gh = a.hist + ((size_t)blockIdx.y << a.B) + ((size_t)part << kLdsMaxB);
  if constexpr (kLds)
    for (uint32_t i = tid; i < bins; i += kBlock) lh[i] = 0u;
  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t gbase = a.g0 + t * kTileU4;
    // ---- stage: pieces gbase ... gbase + kTileU4 (inclusive: the overlap) ---------------
    if constexpr (format != CVD_CAPTURE_BYTES) {
      for (int i = tid; i < kTileU4 + 1; i += kBlock) {
        const int64_t g = gbase + i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (g < a.nu4) v = a.cap[g];
        if constexpr (format == CVD_CAPTURE_MSB) v = make_uint4(lsb_first(v.x), lsb_first(v.y), lsb_first(v.z), lsb_first(v.w));
        *reinterpret_cast<uint4*>(tile + 4 * i) = v;
      }
    } else {
      // one bit per byte: a lane packs 16 capture bytes into one halfword
      typedef uint16_t __attribute__((may_alias)) tile_hw;
      tile_hw* tile16 = reinterpret_cast<tile_hw*>(tile);
      for (int i = tid; i < 2 * kStageDw; i += kBlock) {
        const int64_t g = gbase * 8 + i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (g < a.nu4) v = a.cap[g];
        tile16[i] = (uint16_t)(byte_bits4(v.x) | (byte_bits4(v.y) << 4) | (byte_bits4(v.z) << 8) | (byte_bits4(v.w) << 12));
      }
    }
    __syncthreads();
    // ---- extract: the words that begin in dword d ------------------------------------------
    for (int d = tid; d < kTileDw; d += kBlock) {
      const int64_t base = (gbase << 7) + 32 * d;          // capture bit of the dword's bit 0
      const int64_t lo64 = first - base, hi64 = last - base;
      if (hi64 < 0 || lo64 > 31) continue;
      const int i_lo = lo64 > 0 ? (int)lo64 : 0, i_hi = hi64 < 31 ? (int)hi64 : 31;
      // smallest i >= 0 with base + i = first (mod n)
      int i0 = 0;
      if constexpr (n == 2) i0 = (int)((first ^ base) & 1);
      if constexpr (n == 3) {
        const int r = (int)((base - first) % 3);            // -2..2
        i0 = r > 0 ? 3 - r : -r;
      }
      const uint32_t w0 = tile[d], w1 = tile[d + 1];
#pragma unroll
      for (int k = 0; k < (32 + n - 1) / n; ++k) {
        const int i = i0 + n * k;
        if (i >= i_lo && i <= i_hi) {                        // i <= 31: a shift of 32 never arises
          const uint32_t x = __builtin_amdgcn_alignbit(w1, w0, (uint32_t)i) & mask;
          if constexpr (mode == kLdsPart) {
            if ((x >> kLdsMaxB) == part) atomicAdd(&lh[x & (bins - 1u)], 1u);
          } else if constexpr (mode == kLdsWhole) {
            atomicAdd(&lh[x], 1u);
          } else {
            atomicAdd(&gh[x], 1u);
          }
        }
      }
    }
    __syncthreads();
  }
  if constexpr (kLds) {
    __syncthreads();
    for (uint32_t i = tid; i < bins; i += kBlock) {
      const uint32_t c = lh[i];
      if (c) atomicAdd(&gh[i], c);
    }
  }
}

struct WhtArgs {
  int32_t* w;           // [n_phase][2^B]: counts in, transform in place
  int64_t* sat;         // [n_phase][2^B], written by the final pass
  int64_t T;
  int32_t B;
  int32_t s;            // stages done before this pass (the tile's row stride is 2^s)
  int32_t Lj;           // stages of this pass: rows of the tile = 2^Lj
  int32_t Ll;           // log2 of the tile's neighbouring columns (<= s)
  int32_t final;
};

// Tile element i = (row j = i >> Ll, column c = i & (2^Ll - 1)) is entry
// hi 2^(s+Lj) + j 2^s + q 2^Ll + c of the phase's vector, (hi, q) from blockIdx.x; the pass
// runs the butterflies of index bits s .. s+Lj-1, i.e. bits Ll .. Ll+Lj-1 of i.
__global__ __launch_bounds__(kBlock) void sweep_wht_kernel(WhtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  int32_t* v = reinterpret_cast<int32_t*>(smem);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int E = 1 << (a.Lj + a.Ll);
  const uint32_t t = blockIdx.x;
  const uint32_t q = t & ((1u << (a.s - a.Ll)) - 1u), hi = t >> (a.s - a.Ll);
  const size_t gbase = ((size_t)blockIdx.y << a.B) + ((size_t)hi << (a.s + a.Lj)) + ((size_t)q << a.Ll);
  const int cmask = (1 << a.Ll) - 1;
  for (int i = tid; i < E; i += nthr) v[i] = a.w[gbase + ((size_t)(i >> a.Ll) << a.s) + (i & cmask)];
  __syncthreads();
  for (int b = a.Ll; b < a.Ll + a.Lj; ++b) {
    const int low = (1 << b) - 1;
    for (int p = tid; p < E / 2; p += nthr) {
      const int i0 = ((p & ~low) << 1) | (p & low), i1 = i0 | (1 << b);
      const int32_t x = v[i0], y = v[i1];
      v[i0] = x + y;
      v[i1] = x - y;
    }
    __syncthreads();
  }
  for (int i = tid; i < E; i += nthr) {
    const size_t g = gbase + ((size_t)(i >> a.Ll) << a.s) + (i & cmask);
    if (a.final) a.sat[g] += (a.T + (int64_t)v[i]) >> 1;     // T + w is even and >= 0
    else a.w[g] = v[i];
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
  cvd::set_error(std::string("parity_sweep: ") + what);
  return CVD_E_INVALID;
}

// B = n (span + 1) if the shape is valid, else 0 with the error set
int sweep_bits(int32_t n, int32_t span, int32_t n_phase) {
  if (n < 1 || n > 3) return invalid("n must be 1..3"), 0;
  if (span < 0) return invalid("span must be >= 0"), 0;
  if (span > kMaxB || n * (span + 1) > kMaxB) return invalid("B = n * (span + 1) must be <= 22"), 0;
  if (n_phase < 1 || n_phase > n) return invalid("n_phase must be 1..n"), 0;
  return n * (span + 1);
}

int launch_wht(WhtArgs w, int32_t n_phase, hipStream_t stream) {
  const int E = 1 << (w.Lj + w.Ll);
  const size_t lds = (size_t)E * 4;
  if (lds > 64 * 1024)
    HIP_CHECK(hipFuncSetAttribute((const void*)sweep_wht_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned block = (unsigned)std::min(kBlock, std::max(64, E / 2));
  const unsigned tiles = 1u << (w.B - w.Lj - w.Ll);
  hipLaunchKernelGGL(sweep_wht_kernel, dim3(tiles, (unsigned)n_phase), dim3(block), lds, stream, w);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

}  // namespace

extern "C" int64_t cvd_parity_sweep_workspace_bytes(int32_t n, int32_t span, int32_t n_phase) {
  const int B = sweep_bits(n, span, n_phase);
  if (!B) return CVD_E_INVALID;
  return ((int64_t)n_phase << B) * 4;
}

extern "C" int cvd_parity_sweep(const void* d_capture, int64_t nbits, int32_t format, int32_t n, int32_t span,
                                int64_t start, int64_t T, int32_t n_phase, int64_t* d_sat, void* d_work,
                                void* stream) {
  const int B = sweep_bits(n, span, n_phase);
  if (!B) return CVD_E_INVALID;
  if (T < 0 || T > INT32_MAX) return invalid("T must be 0..2^31 - 1");
  if (start < 0 || nbits < 0) return invalid("needs start, nbits >= 0");
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES)
    return invalid("unknown capture format");
  if (T > 0) {
    // the last word of the last phase ends at start + (n_phase - 1) + n (T - 1) + B
    int64_t end;
    if (__builtin_mul_overflow(T - 1, (int64_t)n, &end) || __builtin_add_overflow(end, start, &end) ||
        __builtin_add_overflow(end, (int64_t)(n_phase - 1 + B), &end))
      return invalid("word positions overflow int64");
    if (end > nbits) return invalid("the last word does not lie inside [0, nbits)");
  }
  if (T == 0) return CVD_OK;
  if (!d_capture || !d_sat || !d_work || ((uintptr_t)d_capture & 15) || ((uintptr_t)d_sat & 7) ||
      ((uintptr_t)d_work & 15))
    return invalid("d_capture, d_work (16-byte aligned) and d_sat (8-byte aligned) must be non-null");
  hipStream_t st = (hipStream_t)stream;
  const size_t bins = (size_t)1 << B;
  HIP_CHECK(hipMemsetAsync(d_work, 0, bins * 4 * (size_t)n_phase, st));

  HistArgs h{};
  h.cap = static_cast<const uint4*>(d_capture);
  const int64_t nbytes = format == CVD_CAPTURE_BYTES ? nbits : nbits / 8 + (nbits % 8 != 0);
  h.nu4 = nbytes / 16 + (nbytes % 16 != 0);
  h.first = start; h.T = T; h.B = B;
  h.hist = static_cast<uint32_t*>(d_work);
  h.g0 = start >> 7;
  const int64_t glast = (start + (n_phase - 1) + (int64_t)n * (T - 1)) >> 7;   // piece of the last word's first bit
  h.ntiles = (glast - h.g0) / kTileU4 + 1;
  using K = void (*)(HistArgs);
#define CVD_SWEEP_ROW(N, M) \
  {sweep_hist_kernel<N, CVD_CAPTURE_LSB, M>, sweep_hist_kernel<N, CVD_CAPTURE_MSB, M>, sweep_hist_kernel<N, CVD_CAPTURE_BYTES, M>}
  static const K kern[3][3][3] = {{CVD_SWEEP_ROW(1, kGlobal), CVD_SWEEP_ROW(2, kGlobal), CVD_SWEEP_ROW(3, kGlobal)},
                                  {CVD_SWEEP_ROW(1, kLdsWhole), CVD_SWEEP_ROW(2, kLdsWhole), CVD_SWEEP_ROW(3, kLdsWhole)},
                                  {CVD_SWEEP_ROW(1, kLdsPart), CVD_SWEEP_ROW(2, kLdsPart), CVD_SWEEP_ROW(3, kLdsPart)}};
#undef CVD_SWEEP_ROW
  const bool in_lds = B <= kLdsMaxB;
  int global_b = kGlobalMinB;                  // CVD_SWEEP_GLOBAL_B: the smallest B on global atomics (A/B runs)
  if (const char* e = getenv("CVD_SWEEP_GLOBAL_B")) global_b = std::max(kLdsMaxB + 1, atoi(e));
  const int mode = in_lds ? kLdsWhole : B >= global_b ? kGlobal : kLdsPart;
  const unsigned parts = mode == kLdsPart ? 1u << (B - kLdsMaxB) : 1u;
  const K hk = kern[mode][n - 1][format];
  const size_t lds = ((size_t)kStageDw + (mode == kGlobal ? 0 : std::min(bins, (size_t)1 << kLdsMaxB))) * 4;
  if (lds > 64 * 1024)
    HIP_CHECK(hipFuncSetAttribute((const void*)hk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // about kMaxGridX blocks in all: each LDS block ends with a flush of its bins
  const unsigned gx = (unsigned)std::min<int64_t>(h.ntiles, std::max<int64_t>(1, kMaxGridX / (n_phase * parts)));
  hipLaunchKernelGGL(hk, dim3(gx, (unsigned)n_phase, parts), dim3(kBlock), lds, st, h);
  HIP_CHECK(hipGetLastError());

  WhtArgs w{};
  w.w = static_cast<int32_t*>(d_work); w.sat = d_sat; w.T = T; w.B = B;
  if (in_lds) {
    w.s = 0; w.Lj = B; w.Ll = 0; w.final = 1;
    return launch_wht(w, n_phase, st);
  }
  w.s = 0; w.Lj = kWhtTileLog; w.Ll = 0; w.final = 0;
  if (int rc = launch_wht(w, n_phase, st)) return rc;
  w.s = kWhtTileLog; w.Lj = B - kWhtTileLog; w.Ll = kWhtColsLog; w.final = 1;
  return launch_wht(w, n_phase, st);
}
