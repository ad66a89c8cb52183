// What the terminated-frame decoders share (cvd_decode_frames.hip describes the design; its
// forward kernels and cvd_decode_psoft.hip's are built from this): the kernel arguments, the
// forward kernels' body around a lane type, the trace kernel, and the host path behind the entry
// points.  Everything is in an unnamed namespace, so that a kernel taking FArgs keeps its name
// whichever file defines it; a file that includes this gets its own trace kernels.  Include
// after <hip/hip_runtime.h>.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_decode_common.h"
#include "cvd_decode_lanes.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr int kFrameWaves = 8192;        // forward and count: waves of a launch (256 CUs x 4 SIMDs x 8)
constexpr int kTraceBlocks = 1024;       // trace: blocks of a launch
constexpr int kTraceThreads = 256;
constexpr int64_t kBatchBytes = (int64_t)1 << 30;   // decision words of a batch, unless 64 frames need more

struct FArgs {
  VArgs v;                   // cap, nu4, format, T, the code, the pattern, span, dec, bits; start: of frame 0 (stride mode)
  const int64_t* offsets;    // o_f, or null: o_f = v.start + f stride
  int64_t stride, nbits;
  int64_t f0, fcount;        // the launch's frames: f0 <= f < f0 + fcount; their decisions at dec[(f - f0) fstride]
  int64_t fstride;           // decision words of a frame: T rounded up to 64 steps
  int32_t s0, e;             // start_state, end_state (CVD_FRAME_ANY: -1)
  int32_t w;                 // words of a row of bits
  int32_t soft;              // errors and counted are the count kernel's
  int32_t* frames;           // [F][6]
  unsigned long long* tot;   // d_stats
};

__device__ __forceinline__ int64_t frame_offset(const FArgs& fa, int64_t f) {
  if (!fa.offsets) return fa.v.start + f * fa.stride;
  const int64_t o = fa.offsets[f];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)o >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The forward kernels' body around a lane type (as forward_body and join_body of
// cvd_decode_common.h are the stream decoders'): the wave's frames one after the other.  The
// frame's arguments are a copy of fa.v with start = o_f, in registers unless lds_args.  PLane
// indexes the pattern's fields by the column, which would put a copy that is a local variable
// into scratch: its copy lives in LDS (sa, which lane 0 filled before the call).
template <bool lds_args, class LaneT, class St>
__device__ __forceinline__ void frame_body(const FArgs& fa, LaneT& ln, St* st, int* met, VArgs* sa = nullptr) {
  constexpr int S = LaneT::S, SPL = LaneT::SPL;
  for (int64_t i = blockIdx.x; i < fa.fcount; i += gridDim.x) {
    const int64_t f = fa.f0 + i;
    const int64_t o = frame_offset(fa, f);
    int32_t* rec = fa.frames + f * 6;
    if (o < 0 || o > fa.nbits - fa.v.span) {             // offset mode only: the host has checked the stride
      if (ln.lane < 6) rec[ln.lane] = ln.lane == 3 ? 1 : (ln.lane == 1 || ln.lane == 2) ? -1 : 0;
      continue;
    }
    int D[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) D[k] = fa.s0 < 0 || ln.state(k) == fa.s0 ? 0 : kInf;
    uint64_t* dec = fa.v.dec + i * fa.fstride;
    int sum;
    if constexpr (lds_args) {
      __syncthreads();                                   // the frame before has been read
      if (ln.lane == 0) sa->start = o;
      __syncthreads();
      sum = ln.template run<true>(*sa, 0, fa.v.T, D, dec, st, met);
    } else {
      VArgs a = fa.v;
      a.start = o;
      sum = ln.template run<true>(a, 0, fa.v.T, D, dec, st, met);
    }
    int sT, val;
    if (fa.e >= 0) {
      sT = fa.e;
      val = 0;
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        const int x = __shfl(D[k], sT & (kWave - 1));
        if ((sT >> 6) == k) val = x;
      }
    } else {
      val = D[0];
#pragma unroll
      for (int k = 1; k < SPL; ++k) val = min(val, D[k]);
#pragma unroll
      for (int k = 1; k < kWave; k <<= 1) val = min(val, __shfl_xor(val, k));
      sT = 0;
#pragma unroll
      for (int k = SPL - 1; k >= 0; --k) {
        const uint64_t bal = __ballot(ln.lane < S && D[k] == val);
        if (bal) sT = kWave * k + __builtin_ctzll(bal);
      }
    }
    if (ln.lane == 0) {
      rec[0] = ln.norm_of(val, sum);
      rec[2] = sT;
      rec[3] = 0;
    }
  }
}

// Lane = frame.  A frame's decision words are contiguous (fstride of them, those of the steps at
// or past T allocated and never written); the chain is viterbi_trace_kernel's.
// A chain is a string of dependent loads and shifts, so the waves of a SIMD hide one another's
// latency: left alone the compiler spends 256 VGPRs on it (one wave per SIMD); held to four
// waves it needs 92 and nothing spills.
template <int m>
__global__ __launch_bounds__(kTraceThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void viterbi_frames_trace_kernel(FArgs fa) {
  constexpr int SPL = Shape<m>::SPL, K = 16 / SPL, NT = 5;
  __shared__ unsigned long long part[NT][kTraceThreads / kWave];
  const int len = (int)fa.v.T;
  const int nsub = (int)(fa.fstride / 16);
  unsigned long long tot[NT] = {0ull, 0ull, 0ull, 0ull, 0ull};   // distance, decoded, skipped, errors, counted
  for (int64_t i = (int64_t)blockIdx.x * kTraceThreads + threadIdx.x; i < fa.fcount;
       i += (int64_t)gridDim.x * kTraceThreads) {
    const int64_t f = fa.f0 + i;
    int32_t* rec = fa.frames + f * 6;
    uint32_t* bits = fa.v.bits + f * fa.w;
    if (rec[3] != 0) {
      for (int k = 0; k < fa.w; ++k) bits[k] = 0u;
      ++tot[2];
      continue;
    }
    const uint64_t* d = fa.v.dec + i * fa.fstride;
    int s = rec[2];
    uint64_t w[16], wn[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) wn[k] = d[(int64_t)(nsub - 1) * 16 + k];
    uint32_t out = 0u;
    for (int c = nsub - 1; c >= 0; --c) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        w[k] = wn[k];
        if (c > 0) wn[k] = d[(int64_t)(c - 1) * 16 + k];
      }
#pragma unroll
      for (int k = K - 1; k >= 0; --k) {
        const int t = c * K + k;
        uint64_t x = w[k * SPL];
#pragma unroll
        for (int j = 1; j < SPL; ++j)
          if ((s >> 6) == j) x = w[k * SPL + j];
        const int dd = (int)((x >> (s & 63)) & 1ull);
        if (t < len) {
          out |= (uint32_t)(s & 1) << (t & 31);
          s = (s >> 1) | (dd << (m - 1));
        }
      }
      if (((c * K) & 31) == 0) {                           // steps [cK, cK + 32) are done: one output word
        if (c * K < len) bits[(c * K) >> 5] = out;
        out = 0u;
      }
    }
    rec[1] = s;
    const unsigned long long dist = (unsigned long long)rec[0];
    tot[0] += dist;
    ++tot[1];
    if (!fa.soft) {
      rec[4] = (int32_t)dist;
      rec[5] = (int32_t)fa.v.span;
      tot[3] += dist;
      tot[4] += (unsigned long long)fa.v.span;
    }
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) tot[q] += __shfl_xor(tot[q], k);
    if ((threadIdx.x & (kWave - 1)) == 0) part[q][threadIdx.x / kWave] = tot[q];
  }
  __syncthreads();
  if (threadIdx.x < NT) {
    unsigned long long sum = 0ull;
#pragma unroll
    for (int k = 0; k < kTraceThreads / kWave; ++k) sum += part[threadIdx.x][k];
    if (sum) atomicAdd(&fa.tot[threadIdx.x], sum);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && fa.f0 == 0) fa.tot[5] = (unsigned long long)fa.w;
}

// Soft frames' records [4] and [5] and their totals, after the trace: a wave per frame re-encodes
// the row of bits from s_0 and counts the sign disagreements and the values that are not 0
// (count_signs), as viterbi_soft_count_kernel does for a stream; one pair of atomics per wave.
// punct: the values that the pattern keeps; a: fa.v, or its copy in LDS.
template <bool punct>
__device__ __forceinline__ void count_body(const FArgs& fa, const VArgs& a, int m, int n) {
  const int lane = threadIdx.x;
  unsigned long long terr = 0ull, tseen = 0ull;
  for (int64_t i = blockIdx.x; i < fa.fcount; i += gridDim.x) {
    const int64_t f = fa.f0 + i;
    int32_t* rec = fa.frames + f * 6;
    if (rec[3] != 0) continue;
    const int8_t* v = reinterpret_cast<const int8_t*>(fa.v.cap) + frame_offset(fa, f);
    uint32_t err, seen;
    count_signs<punct>(a, v, fa.v.bits + f * fa.w, (uint32_t)rec[1], (int)fa.v.T, m, n, lane, err, seen);
    if (lane == 0) {
      rec[4] = (int32_t)err;
      rec[5] = (int32_t)seen;
    }
    terr += err;
    tseen += seen;
  }
  if (lane == 0) {
    if (terr) atomicAdd(&fa.tot[3], terr);
    if (tseen) atomicAdd(&fa.tot[4], tseen);
  }
}

using FKern = void (*)(FArgs);
using CKern = void (*)(FArgs, int, int);   // (fa, m, n)
#define CVD_F_ROW(KERN, n) {KERN<1, n>, KERN<2, n>, KERN<3, n>, KERN<4, n>, KERN<5, n>, KERN<6, n>, KERN<7, n>, KERN<8, n>}
#define CVD_F_TABLE(KERN) {CVD_F_ROW(KERN, 2), CVD_F_ROW(KERN, 3)}

// kBatchBytes, or CVD_FRAMES_BATCH_BYTES (a test's way to more than one batch on small frames)
int64_t batch_bytes() {
  const char* e = getenv("CVD_FRAMES_BATCH_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (int64_t)v : kBatchBytes;
}

// the workspace of F frames: all their decision words, or a batch's (monotone in F and in T)
int64_t frames_work_bytes(int m, int64_t T, int64_t F) {
  const int64_t pf = frame_bytes(m, T), cap = std::max(round16(batch_bytes()), 64 * pf);
  return F > cap / pf ? cap : F * pf;
}

// The entry points behind the code shape and the pattern.  who: the entry point's name in the
// errors; fwd: its forward kernel for the code's shape; count: the kernel that writes records
// [4], [5] and their totals after the trace, or null where they are the distance and the span.
int decode_frames(const char* who, FKern fwd, CKern count, const cvd_code* code, const cvd::VPattern* pat,
                  const void* d_capture, int64_t nbits, int32_t format, int64_t start, int64_t stride,
                  const int64_t* d_offsets, int64_t F, int32_t T, int32_t start_state, int32_t end_state,
                  uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream) {
  const int n = code->n, m = code->m;
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES)
    return invalid(who, "unknown capture format");
  if (nbits < 0) return invalid(who, "needs nbits >= 0");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (start_state < CVD_FRAME_ANY || start_state >= (1 << m) || end_state < CVD_FRAME_ANY || end_state >= (1 << m))
    return invalid(who, "start_state and end_state must be CVD_FRAME_ANY or a state in [0, 2^m)");
  if (!d_offsets && (start < 0 || stride < 1)) return invalid(who, "needs start >= 0 and stride >= 1");
  if (F == 0) return CVD_OK;
  if (T < 1 || T > CVD_VITERBI_FRAME_MAX_T) return invalid(who, "T must be 1..65536");
  if (start_state >= 0 && end_state >= 0 && T < m)
    return invalid(who, "with both states fixed T must be at least m: end_state is not reachable before");
  const int64_t w = (T + 31) / 32;
  if (F >= ((int64_t)1 << 31) / w + (((int64_t)1 << 31) % w != 0)) return invalid(who, "F * ceil(T / 32) must be below 2^31 words");
  int64_t span = (int64_t)n * T;
  if (pat && !pat->span(T, &span)) return invalid(who, "the span of a frame overflows int64");
  if (!d_offsets) {
    int64_t end;
    if (__builtin_mul_overflow(F - 1, stride, &end) || __builtin_add_overflow(end, start, &end) ||
        __builtin_add_overflow(end, span, &end))
      return invalid(who, "the position of the last frame's end overflows int64");
    if (end > nbits) return invalid(who, "the frames do not lie inside [0, nbits)");
  }
  if (!d_capture || !d_bits || !d_frames || !d_stats || !d_work || ((uintptr_t)d_capture & 15) ||
      ((uintptr_t)d_work & 15) || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_frames & 3) || ((uintptr_t)d_stats & 7) ||
      ((uintptr_t)d_offsets & 7))
    return invalid(who, "d_capture, d_work (16-byte aligned), d_stats (8-byte), d_bits and d_frames (4-byte) must be "
                        "non-null, d_offsets 8-byte aligned");

  FArgs fa{};
  VArgs& a = fa.v;
  a.cap = static_cast<const uint4*>(d_capture);
  const int64_t nbytes = format == CVD_CAPTURE_BYTES ? nbits : nbits / 8 + (nbits % 8 != 0);
  a.nu4 = nbytes / 16 + (nbytes % 16 != 0);
  a.format = format;
  a.start = d_offsets ? 0 : start;
  a.T = T;
  a.span = span;
  for (int j = 0; j < n; ++j) {
    const uint8_t* t = code->taps + (size_t)j * (m + 1);
    if (t[0] & 1) a.g0 |= 1u << j;
    for (int d = 1; d <= m; ++d)
      if (t[d] & 1) a.gs[j] |= 1u << (d - 1);
  }
  if (pat) {
    a.period = pat->period;
    a.K = pat->K;
    a.pmask = pat->pmask;
    a.ppre[0] = pat->ppre[0];
    a.ppre[1] = pat->ppre[1];
  }
  a.dec = static_cast<uint64_t*>(d_work);
  a.bits = d_bits;
  fa.offsets = d_offsets;
  fa.stride = stride;
  fa.nbits = nbits;
  fa.fstride = frame_bytes(m, T) / 8;
  fa.s0 = start_state;
  fa.e = end_state;
  fa.w = (int32_t)w;
  fa.soft = count != nullptr;
  fa.frames = d_frames;
  fa.tot = reinterpret_cast<unsigned long long*>(d_stats);

  static const FKern trace[8] = {viterbi_frames_trace_kernel<1>, viterbi_frames_trace_kernel<2>,
                                 viterbi_frames_trace_kernel<3>, viterbi_frames_trace_kernel<4>,
                                 viterbi_frames_trace_kernel<5>, viterbi_frames_trace_kernel<6>,
                                 viterbi_frames_trace_kernel<7>, viterbi_frames_trace_kernel<8>};
  const int64_t batch = frames_work_bytes(m, T, F) / frame_bytes(m, T);
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats, 0, 6 * sizeof(int64_t), st));
  for (int64_t f0 = 0; f0 < F; f0 += batch) {
    fa.f0 = f0;
    fa.fcount = std::min(batch, F - f0);
    const unsigned waves = (unsigned)std::min<int64_t>(fa.fcount, kFrameWaves);
    hipLaunchKernelGGL(fwd, dim3(waves), dim3(kWave), 0, st, fa);
    HIP_CHECK(hipGetLastError());
    const int64_t tb = (fa.fcount + kTraceThreads - 1) / kTraceThreads;
    hipLaunchKernelGGL(trace[m - 1], dim3((unsigned)std::min<int64_t>(tb, kTraceBlocks)), dim3(kTraceThreads), 0, st, fa);
    HIP_CHECK(hipGetLastError());
    if (count) {
      hipLaunchKernelGGL(count, dim3(waves), dim3(kWave), 0, st, fa, m, n);
      HIP_CHECK(hipGetLastError());
    }
  }
  return CVD_OK;
}

}  // namespace
