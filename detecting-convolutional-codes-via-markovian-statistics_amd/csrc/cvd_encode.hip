// Information bits -> coded capture (cvd_encode_frames, include/cvd.h) for gfx950: the inverse
// of the frames decoders.  F rows of packed information bits become one capture in any of the
// decoders' formats, open, terminated or tail-biting, punctured or not, at a stride or at
// offsets.
//
// The encoder has no recurrence: output j of step t is the parity of the m + 1 information bits
// u_{t-m} .. u_t under output j's tap mask.  So the work is driven by the OUTPUT:
//   piece   a lane owns one aligned 16-byte piece of the capture: 128 positions in the packed
//           formats (four dwords of 32), 16 positions in BYTES / SOFT.  Consecutive lanes own
//           consecutive pieces: a wave's store is one contiguous 1 KiB of dwordx4, and every
//           byte of the capture (gaps and padding included, as zeros) is written exactly once.
//   frames  in stride mode frame f covers positions [start + f*stride, + span); the frames that
//           meet a dword of 32 (a run of 16) positions are found with one division per piece
//           (none for a single frame; in 32 bits where the operands fit) and walked: usually
//           one or two, sixteen per dword at span = stride = 2.
//   window  for the frame-relative position q the lane reads the row's words around step
//           t = q / n and funnels them (v_alignbit) into a window u_{t-m} .. of 64 bits (three
//           dwords) in the packed formats and 32 bits (two dwords) in the byte formats, whose
//           16 positions need at most 9 steps; bits before step 0 come from start_state or,
//           tail-biting, from the row's end; bits at or past T (terminated: T - m) are zero.
//   plain   stream j = XOR over the set taps d of (window >> (m - d)); the n streams are
//           interleaved by bit spreading (multiplication-free; 64-bit for 32 positions, 32-bit
//           for 16) and shifted to the position's phase.
//   punct   the column of q is found from the packed pattern (one division by K), then the
//           lane walks steps, emitting the kept outputs' parities until the run is full.
//   format  LSB: as built; MSB: a per-byte bit reversal; BYTES / SOFT: 16 bits and their
//           coverage mask spread to one byte each (+A / -A / 0).
// Offsets mode (BYTES / SOFT only) cannot be output-driven without sorting: the capture is
// zero-filled on the stream and a second kernel scatters, one lane per 16 positions of a
// frame, byte stores (frames start at any byte).  The tap masks and the pattern are kernel
// arguments.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kDefaultBlocks = 8192;   // grid-stride above this (CVD_ENCODE_BLOCKS: another cap)
const char* const kWho = "encode_frames";

struct EncArgs {
  const uint32_t* info;
  int64_t pitch;          // words per row
  int64_t F;
  int32_t T, w;           // steps per frame, ceil(T / 32)
  int32_t Tlim;           // information bits at or past it read as 0 (T, terminated: T - m)
  int32_t m, mode, format, amplitude;
  uint32_t start_rev;     // bit-reversed start_state: bit 31 - i = bit i of it
  uint32_t rmask[3];      // output j's taps over the window: bit m - d = taps[j][0][d]
  uint64_t pmask;         // punctured: keep[c] in bits 4c .. 4c+3
  int32_t period, K;
  int64_t span;
  int64_t start, stride;  // stride mode
  const int64_t* offsets; // offsets mode
  uint4* out;
  int64_t npieces;        // 16-byte pieces of the capture, padding included
  int64_t nout;
  unsigned long long* stats;
  int64_t chunks;         // offsets mode: ceil(span / 16)
};

// a / b for 0 <= a, 0 < b: a 32-bit division where both fit
__device__ __forceinline__ int64_t div_pos(int64_t a, int64_t b) {
  return ((uint64_t)(a | b) >> 32) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// u_{t} for the 64 (wide) or 32 steps from t_lo of one row (t_lo >= -m), bit i = u_{t_lo + i};
// bits at or past that count are not meaningful
template <bool wide>
__device__ __forceinline__ uint64_t info_window(const EncArgs& a, const uint32_t* row, int32_t t_lo) {
  const int32_t neg = t_lo < 0 ? -t_lo : 0, ts = t_lo < 0 ? 0 : t_lo;
  const int32_t wi = ts >> 5, last = a.w - 1;
  const uint32_t sh = (uint32_t)ts & 31u;
  // words past the row's last are never read: every bit they would give is at or past T
  const uint32_t w0 = row[min(wi, last)], w1 = row[min(wi + 1, last)];
  uint64_t v = (uint64_t)__builtin_amdgcn_alignbit(w1, w0, sh);
  if constexpr (wide) v |= (uint64_t)__builtin_amdgcn_alignbit(row[min(wi + 2, last)], w1, sh) << 32;
  const int32_t valid = a.Tlim - ts;
  if (valid < 64) v = valid > 0 ? v & ((1ull << valid) - 1ull) : 0ull;
  if (neg) {
    uint32_t head;
    if (a.mode != CVD_ENCODE_TAILBITING) {
      head = a.start_rev >> (32 - neg);                   // u_{-d} = bit d - 1 of start_state
    } else if (a.T >= neg) {
      const int32_t tb = a.T - neg, bi = tb >> 5;         // u_{T-neg} .. u_{T-1}
      head = __builtin_amdgcn_alignbit(row[min(bi + 1, last)], row[bi], (uint32_t)tb & 31u) & ((1u << neg) - 1u);
    } else {
      head = 0;                                           // T < m <= 16: the row is one word, wrapped
      int32_t t = (a.T - neg % a.T) % a.T;                // (-neg) mod T
      for (int i = 0; i < neg; ++i) {
        head |= ((row[0] >> t) & 1u) << i;
        t = t + 1 == a.T ? 0 : t + 1;
      }
    }
    v = (v << neg) | head;
  }
  return v;
}

__device__ __forceinline__ uint64_t spread2(uint32_t x) {   // bit i -> bit 2i
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

__device__ __forceinline__ uint64_t spread3(uint32_t x) {   // bit i -> bit 3i, i < 21
  uint64_t v = x & 0x1FFFFFu;
  v = (v | (v << 32)) & 0x001F00000000FFFFull;
  v = (v | (v << 16)) & 0x001F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__device__ __forceinline__ uint32_t spread2_16(uint32_t x) {   // bit i -> bit 2i, i < 16
  x &= 0xFFFFu;
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

__device__ __forceinline__ uint32_t spread3_10(uint32_t x) {   // bit i -> bit 3i, i < 10
  x &= 0x3FFu;
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

// The frame's coded bits at the LEN (32 or 16) frame-relative positions q0 .. q0 + LEN - 1
// (q0 > -LEN, q0 < span), bit i = position q0 + i, zero outside [0, span) and at or above LEN;
// *cov: the positions inside the frame.
template <int n, bool punct, int LEN>
__device__ __forceinline__ uint32_t coded(const EncArgs& a, const uint32_t* row, int64_t q0, uint32_t* cov) {
  constexpr bool wide = LEN == 32;
  constexpr uint32_t full = wide ? 0xFFFFFFFFu : 0xFFFFu;
  const int64_t qs = q0 < 0 ? 0 : q0;
  const int m = a.m;
  uint32_t bits;
  if constexpr (!punct) {
    const int32_t t0 = (int32_t)div_pos(qs, n);
    const uint32_t ph = (uint32_t)(qs - (int64_t)t0 * n);
    const uint64_t W = info_window<wide>(a, row, t0 - m);
    uint32_t s[n];
#pragma unroll
    for (int j = 0; j < n; ++j) {
      uint32_t x = 0;
      // 16 positions: at most 9 steps, window bits <= 8 + m <= 24
      for (uint32_t r = a.rmask[j]; r; r &= r - 1)
        x ^= wide ? (uint32_t)(W >> (__builtin_ctz(r))) : (uint32_t)W >> (__builtin_ctz(r));
      s[j] = x;
    }
    if constexpr (wide) {
      uint64_t c;
      if constexpr (n == 2) c = spread2(s[0]) | (spread2(s[1]) << 1);
      else c = spread3(s[0]) | (spread3(s[1]) << 1) | (spread3(s[2]) << 2);   // 21 steps: 63 bits >= 2 + 32
      bits = (uint32_t)(c >> ph);
    } else {
      uint32_t c;
      if constexpr (n == 2) c = spread2_16(s[0]) | (spread2_16(s[1]) << 1);
      else c = spread3_10(s[0]) | (spread3_10(s[1]) << 1) | (spread3_10(s[2]) << 2);   // 10 steps: 30 bits >= 2 + 16
      bits = c >> ph;
    }
  } else {
    const int64_t blk = div_pos(qs, a.K);
    int32_t skip = (int32_t)(qs - blk * a.K);            // kept bits of the period before qs
    int32_t c = 0;
    for (;;) {
      const int32_t k = __builtin_popcount((uint32_t)(a.pmask >> (4 * c)) & 7u);
      if (skip < k) break;
      skip -= k;
      ++c;
    }
    const int64_t t0 = blk * a.period + c;               // < T: qs < span
    const uint64_t W = info_window<true>(a, row, (int32_t)t0 - m);
    const uint32_t wm = (2u << m) - 1u;
    uint64_t o = 0;
    int32_t nb = 0;
    // every step emits at least one bit: at most LEN steps, window bits i .. i + m <= 47
    for (int32_t i = 0; nb < LEN && t0 + i < a.T; ++i) {
      const uint32_t x = (uint32_t)(W >> i) & wm;
      const uint32_t kp = (uint32_t)(a.pmask >> (4 * c)) & 7u;
#pragma unroll
      for (int j = 0; j < n; ++j) {
        if ((kp >> j) & 1u) {
          if (skip > 0) --skip;
          else { o |= (uint64_t)(__builtin_popcount(x & a.rmask[j]) & 1u) << nb; ++nb; }
        }
      }
      c = c + 1 == a.period ? 0 : c + 1;
    }
    bits = (uint32_t)o;
  }
  const int64_t left = a.span - qs;                      // > 0
  const uint32_t mask = left < LEN ? (1u << (uint32_t)left) - 1u : full;
  const uint32_t lead = (uint32_t)(qs - q0);             // 0 .. LEN - 1
  bits = ((bits & mask) << lead) & full;
  *cov = (mask << lead) & full;
  return bits;
}

// four bits -> bit 0 of four bytes
__device__ __forceinline__ uint32_t nibble_bytes(uint32_t x) {
  return (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21);
}

__device__ __forceinline__ uint32_t value_bytes(const EncArgs& a, uint32_t bits4, uint32_t cov4) {
  const uint32_t b = nibble_bytes(bits4);
  if (a.format == CVD_CAPTURE_BYTES) return b;
  // one term per byte is nonzero and below 256: no carry between bytes
  return b * (uint32_t)a.amplitude + (nibble_bytes(cov4) ^ b) * (uint32_t)(256 - a.amplitude);
}

// stride mode: the whole capture, one 16-byte piece per lane and pass
template <int n, bool punct, bool packed>
__global__ __launch_bounds__(kBlock) void encode_stride_kernel(EncArgs a) {
  constexpr int len = packed ? 32 : 16, ne = packed ? 4 : 1;
  const int64_t step = (int64_t)gridDim.x * kBlock;
  for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < a.npieces; g += step) {
    const int64_t P0 = g * (packed ? 128 : 16);
    uint32_t acc[4] = {0u, 0u, 0u, 0u}, cov = 0u;
    const int64_t rel = P0 - a.start;
    int64_t f = rel > 0 && a.F > 1 ? div_pos(rel, a.stride) : 0;
    int64_t o = a.start + f * a.stride;
#pragma unroll
    for (int e = 0; e < ne; ++e) {
      const int64_t Pe = P0 + 32 * e;
      while (f < a.F && o + a.stride <= Pe) { ++f; o += a.stride; }
      int64_t ff = f, oo = o;
      while (ff < a.F && oo < Pe + len) {
        if (Pe - oo < a.span) {
          uint32_t cv;
          acc[e] |= coded<n, punct, len>(a, a.info + ff * a.pitch, Pe - oo, &cv);
          cov |= cv;
        }
        ++ff;
        oo += a.stride;
      }
    }
    uint4 v;
    if constexpr (packed) {
      if (a.format == CVD_CAPTURE_MSB) {
        acc[0] = lsb_first(acc[0]); acc[1] = lsb_first(acc[1]); acc[2] = lsb_first(acc[2]); acc[3] = lsb_first(acc[3]);
      }
      v = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      const uint32_t b = acc[0];
      v = make_uint4(value_bytes(a, b & 15u, cov & 15u), value_bytes(a, (b >> 4) & 15u, (cov >> 4) & 15u),
                     value_bytes(a, (b >> 8) & 15u, (cov >> 8) & 15u), value_bytes(a, (b >> 12) & 15u, (cov >> 12) & 15u));
    }
    a.out[g] = v;
    if (g == 0 && a.stats) { a.stats[0] = (unsigned long long)a.F; a.stats[1] = 0ull; }
  }
}

// offsets mode (BYTES / SOFT) over a zero-filled capture: lane (f, c) writes positions
// [16c, 16c + 16) of frame f, if the frame lies inside the capture
template <int n, bool punct>
__global__ __launch_bounds__(kBlock) void encode_scatter_kernel(EncArgs a) {
  const int64_t step = (int64_t)gridDim.x * kBlock, total = a.F * a.chunks;
  uint8_t* out = reinterpret_cast<uint8_t*>(a.out);
  for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += step) {
    const int64_t f = div_pos(g, a.chunks), c = g - f * a.chunks;
    const int64_t o = a.offsets[f];
    const bool skipped = o < 0 || o > a.nout - a.span;
    if (c == 0 && a.stats) atomicAdd(&a.stats[skipped ? 1 : 0], 1ull);
    if (skipped) continue;
    uint32_t cov;
    const uint32_t b = coded<n, punct, 16>(a, a.info + f * a.pitch, 16 * c, &cov);
    uint8_t* d = out + o + 16 * c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = value_bytes(a, (b >> (4 * e)) & 15u, (cov >> (4 * e)) & 15u);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((cov >> (4 * e + i)) & 1u) d[4 * e + i] = (uint8_t)(v >> (8 * i));
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
  cvd::set_error(std::string(kWho) + ": " + what);
  return CVD_E_INVALID;
}

}  // namespace

extern "C" int cvd_encode_frames(const cvd_code* code, const uint8_t* keep, int32_t period, const uint32_t* d_info,
                                 int64_t pitch, int64_t F, int64_t T, int32_t mode, int32_t start_state,
                                 int32_t format, int32_t amplitude, void* d_out, int64_t nout, int64_t start,
                                 int64_t stride, const int64_t* d_offsets, int64_t* d_stats, void* stream) {
  if (!code || !code->taps) return invalid("null code");
  if (code->k != 1 || code->n < 2 || code->n > 3 || code->m < 1 || code->m > 16) {
    cvd::set_error(std::string(kWho) + ": needs k = 1, n in 2..3 and m in 1..16");
    return CVD_E_UNSUPPORTED;
  }
  const int n = code->n, m = code->m;
  if (mode != CVD_ENCODE_OPEN && mode != CVD_ENCODE_TERMINATED && mode != CVD_ENCODE_TAILBITING)
    return invalid("unknown mode");
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES && format != CVD_CAPTURE_SOFT)
    return invalid("unknown output format");
  if (format == CVD_CAPTURE_SOFT ? (amplitude < 1 || amplitude > 127) : amplitude != 0)
    return invalid("amplitude must be 1..127 for CVD_CAPTURE_SOFT and 0 otherwise");
  if (mode != CVD_ENCODE_TAILBITING && (start_state < 0 || start_state >= (1 << m)))
    return invalid("start_state outside [0, 2^m)");
  if (F < 0 || nout < 0) return invalid("needs F >= 0 and nout >= 0");
  const bool packed = format == CVD_CAPTURE_LSB || format == CVD_CAPTURE_MSB;
  if (d_offsets && packed) return invalid("d_offsets needs CVD_CAPTURE_BYTES or CVD_CAPTURE_SOFT");
  cvd::VPattern pat;
  bool punct = false;
  if (keep) {
    if (const int rc = cvd::viterbi_pack_pattern(kWho, format == CVD_CAPTURE_SOFT ? "value" : "bit", keep, period, n, &pat))
      return rc;
    for (int c = 0; c < period; ++c) punct |= keep[c] != (1 << n) - 1;   // all kept: the plain kernel
  }
  if (!d_offsets && (start < 0 || stride < 1)) return invalid("stride mode needs start >= 0 and stride >= 1");
  if (F == 0) return CVD_OK;
  if (T < 1 || T > INT32_MAX) return invalid("T must be 1..2^31 - 1");
  if (mode == CVD_ENCODE_TERMINATED && T < m) return invalid("a terminated frame needs T >= m");
  const int64_t w = (T + 31) / 32;
  if (pitch < w) return invalid("pitch is below ceil(T / 32)");
  int64_t span, tmp;
  if (keep ? !pat.span(T, &span) : __builtin_mul_overflow(T, (int64_t)n, &span)) return invalid("the span overflows int64");
  if (__builtin_mul_overflow(F, pitch, &tmp) || __builtin_mul_overflow(tmp, (int64_t)4, &tmp))
    return invalid("F * pitch overflows int64");
  if (nout > INT64_MAX - 127) return invalid("nout overflows int64");
  if (!d_offsets) {
    if (stride < span) return invalid("stride is below the span: frames would overlap");
    int64_t end;
    if (__builtin_mul_overflow(F - 1, stride, &end) || __builtin_add_overflow(end, start, &end) ||
        __builtin_add_overflow(end, span, &end))
      return invalid("frame positions overflow int64");
    if (end > nout) return invalid("the frames do not lie inside [0, nout)");
    if (F == 1) stride = span;   // unused by a single frame; keeps the kernel's o + stride small
  }
  int64_t total = 0;             // offsets mode: the scatter kernel's lanes
  if (d_offsets && __builtin_mul_overflow(F, (span + 15) / 16, &total)) return invalid("F * span overflows int64");
  if (!d_info || ((uintptr_t)d_info & 3)) return invalid("d_info must be non-null and 4-byte aligned");
  if (!d_out || ((uintptr_t)d_out & 15)) return invalid("d_out must be non-null and 16-byte aligned");
  if ((uintptr_t)d_offsets & 7) return invalid("d_offsets must be 8-byte aligned");
  if ((uintptr_t)d_stats & 7) return invalid("d_stats must be 8-byte aligned");
  int64_t cap = kDefaultBlocks;
  if (const char* e = getenv("CVD_ENCODE_BLOCKS")) {
    const long long v = atoll(e);
    if (v >= 1) cap = std::min<int64_t>(v, 1 << 22);
  }
  EncArgs a{};
  a.info = d_info; a.pitch = pitch; a.F = F; a.T = (int32_t)T; a.w = (int32_t)w;
  a.Tlim = (int32_t)(mode == CVD_ENCODE_TERMINATED ? T - m : T);
  a.m = m; a.mode = mode; a.format = format; a.amplitude = amplitude;
  a.start_rev = mode == CVD_ENCODE_TAILBITING ? 0u : __builtin_bitreverse32((uint32_t)start_state);
  for (int j = 0; j < n; ++j)
    for (int d = 0; d <= m; ++d)
      if (code->taps[j * (m + 1) + d] & 1) a.rmask[j] |= 1u << (m - d);
  if (punct) { a.pmask = pat.pmask; a.period = pat.period; a.K = pat.K; }
  a.span = span; a.start = start; a.stride = stride; a.offsets = d_offsets;
  a.out = static_cast<uint4*>(d_out);
  const int64_t nbytes = packed ? nout / 8 + (nout % 8 != 0) : nout;
  a.npieces = nbytes / 16 + (nbytes % 16 != 0);
  a.nout = nout;
  a.stats = reinterpret_cast<unsigned long long*>(d_stats);
  a.chunks = (span + 15) / 16;
  hipStream_t s = (hipStream_t)stream;
  using K = void (*)(EncArgs);
  const int ki = (n - 2) * 2 + (punct ? 1 : 0);
  if (!d_offsets) {
    static const K kern[2][4] = {
        {encode_stride_kernel<2, false, false>, encode_stride_kernel<2, true, false>,
         encode_stride_kernel<3, false, false>, encode_stride_kernel<3, true, false>},
        {encode_stride_kernel<2, false, true>, encode_stride_kernel<2, true, true>,
         encode_stride_kernel<3, false, true>, encode_stride_kernel<3, true, true>}};
    // nout == 0 with F > 0 is impossible (span >= 1): there is at least one piece
    const unsigned grid = (unsigned)std::min<int64_t>(cap, (a.npieces + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(kern[packed][ki], dim3(grid), dim3(kBlock), 0, s, a);
    HIP_CHECK(hipGetLastError());
    return CVD_OK;
  }
  static const K kern[4] = {encode_scatter_kernel<2, false>, encode_scatter_kernel<2, true>,
                            encode_scatter_kernel<3, false>, encode_scatter_kernel<3, true>};
  if (a.npieces > 0) HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)a.npieces * 16, s));
  if (d_stats) HIP_CHECK(hipMemsetAsync(d_stats, 0, 16, s));
  const unsigned grid = (unsigned)std::min<int64_t>(cap, (total + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(kern[ki], dim3(grid), dim3(kBlock), 0, s, a);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}
