// What the soft-output frame decoders share (cvd_decode_llr.hip describes the design; its kernels
// and cvd_decode_psoft.hip's are built from this): the kernel arguments, the kernel's body around
// a loader of a step's values, and the host path behind the entry points.  Everything is in an
// unnamed namespace, so that a kernel taking LArgs keeps its name whichever file defines it.
// Include after <hip/hip_runtime.h>.
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

constexpr int kInfTest = 1 << 27;        // alpha + beta at or above this: no finite path
constexpr int kSat = 32767;
constexpr int kLlrSeg = 32;              // steps of a segment: a word of bits, half a wave of values
constexpr int kLlrWaves = 8192;          // waves of the launch
constexpr int64_t kLlrWorkBytes = (int64_t)1 << 30;

struct LArgs {
  VArgs v;                   // cap, nu4, T, the code
  const int64_t* offsets;    // o_f, or null: o_f = v.start + f stride
  int64_t stride, nvals, F;
  int64_t slice;             // ints of a wave's checkpoints: (w - 2) S, rounded up to 16 bytes
  int32_t s0, e;             // start_state, end_state (CVD_FRAME_ANY: -1)
  int32_t w;                 // segments of a frame = words of a row of bits
  int* ckpt;                 // d_work
  int16_t* llr;              // [F][32 w]
  int32_t* frames;           // [F][6]
  unsigned long long* tot;   // d_stats
};

__device__ __forceinline__ int64_t frame_offset(const LArgs& la, int64_t f) {
  if (!la.offsets) return la.v.start + f * la.stride;
  const int64_t o = la.offsets[f];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)o >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// A loader: the n values of step t of the frame whose first value is v[0], -128 read as -127,
// packed a byte each; asum += their magnitudes.  Here: every value is in the capture.
template <int n>
struct LoadAll {
  __device__ __forceinline__ int operator()(const int8_t* v, int t, int& asum) const {
    const int8_t* p = v + (int64_t)n * t;
    int vp = 0;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const int x = max((int)p[j], -127);
      asum += abs(x);
      vp |= (x & 255) << (8 * j);
    }
    return vp;
  }
};

// Here: the values that a pattern keeps (a: in LDS), 0 in the place of the others.
struct LoadKept {
  const VArgs* a;
  __device__ __forceinline__ int operator()(const int8_t* v, int t, int& asum) const {
    int vp = 0;
    kept_values(*a, v, t, [&](int j, int x) {
      x = max(x, -127);
      asum += abs(x);
      vp |= (x & 255) << (8 * j);
    });
    return vp;
  }
};

// The kernel's body around a loader.  LDS: rows kLlrSeg max(S, 64) ints, met 2 S ints (S > 64).
template <int m, int n, class Loader>
__device__ __forceinline__ void llr_body(const LArgs& la, int* rows, int* met, Loader load) {
  using Sh = Shape<m>;
  constexpr int S = Sh::S, SPL = Sh::SPL, RS = S > kWave ? S : kWave;
  SLane<m, n> ln;
  ln.init(la.v);
  const int lane = ln.lane;
  int po0[SPL], po1[SPL], ns0[SPL];   // the lane's own states: patterns of out(s, 0), out(s, 1), the successor by u = 0
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const int s = ln.state(i);
    po0[i] = SLane<m, n>::pattern(ln.template branch_out<n>(la.v, s, 0));
    po1[i] = SLane<m, n>::pattern(ln.template branch_out<n>(la.v, s, 1));
    ns0[i] = (s << 1) & (S - 1);
  }
  const int8_t* cap = reinterpret_cast<const int8_t*>(la.v.cap);
  int* ck = la.ckpt + (int64_t)blockIdx.x * la.slice;
  const int T = (int)la.v.T, nseg = la.w;
  int cur = 0;
  unsigned long long tdist = 0ull, tdec = 0ull, tskip = 0ull, tzero = 0ull, tsat = 0ull;

  // lane j < cnt: the values of step t0 + j
  auto load_vals = [&](int64_t o, int t0, int cnt, int& asum) {
    int vp = 0;
    if (lane < cnt) vp = load(cap + o, t0 + lane, asum);
    return vp;
  };

  for (int64_t f = blockIdx.x; f < la.F; f += gridDim.x) {
    const int64_t o = frame_offset(la, f);
    int32_t* rec = la.frames + f * 6;
    int16_t* lrow = la.llr + f * nseg * kLlrSeg;
    uint32_t* brow = la.v.bits + f * nseg;
    if (o < 0 || o > la.nvals - la.v.span) {             // offset mode only: the host has checked the stride
      for (int k = lane; k < nseg * kLlrSeg; k += kWave) lrow[k] = 0;
      for (int k = lane; k < nseg; k += kWave) brow[k] = 0u;
      if (lane < 6) rec[lane] = lane == 3 ? 1 : lane == 2 ? -1 : 0;
      ++tskip;
      continue;
    }

    // forward, up to the start of the last segment: the checkpoints, sum A
    int X[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) X[k] = la.s0 < 0 || ln.state(k) == la.s0 ? 0 : kInf;
    int asum = 0;
    for (int c = 0; c < nseg - 1; ++c) {
      if (c > 0 && lane < S) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) ck[(int64_t)(c - 1) * S + ln.state(k)] = X[k];
      }
      const int vp = load_vals(o, c * kLlrSeg, kLlrSeg, asum);
      acs_chunk<false>(ln, kLlrSeg, X, cur, met, nullptr, [&](int jj) { return __builtin_amdgcn_readlane(vp, jj); });
    }

    // segments, last to first; the last one continues the forward pass and leaves alpha_T
    int sT = 0, dist = 0;
    int Y[SPL];                                          // beta in the same representation
#pragma unroll
    for (int k = 0; k < SPL; ++k) Y[k] = la.e < 0 || ln.state(k) == la.e ? 0 : kInf;
    int weak = kSat;
    uint32_t zeros = 0u, sat = 0u;
    for (int c = nseg - 1; c >= 0; --c) {
      const int t0 = c * kLlrSeg, cnt = min(kLlrSeg, T - t0);
      const bool last = c == nseg - 1;
      if (!last) {
#pragma unroll
        for (int k = 0; k < SPL; ++k)
          X[k] = c > 0 ? ck[(int64_t)(c - 1) * S + ln.state(k)] : la.s0 < 0 || ln.state(k) == la.s0 ? 0 : kInf;
      }
      int amag = 0;
      const int vp = load_vals(o, t0, cnt, amag);
      if (last) asum += amag;
      __syncthreads();                                   // the rows of the segment before have been read
      for (int jj = 0; jj < cnt; ++jj) {                 // rows[jj] = alpha_{t0 + jj + 1}
        const int vs = __builtin_amdgcn_readlane(vp, jj);
        const int* src = rows + max(jj - 1, 0) * RS;
        if constexpr (SPL > 1) {
          if (jj == 0) {
#pragma unroll
            for (int i = 0; i < SPL; ++i) met[cur * S + ln.state(i)] = X[i];
            __syncthreads();
            src = met + cur * S;
            cur ^= 1;
          }
        }
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
          int a0, a1;
          if constexpr (SPL > 1) {
            a0 = src[ln.ps0[i]];
            a1 = src[ln.ps1[i]];
          } else {
            a0 = __shfl(X[0], ln.ps0[0]);
            a1 = __shfl(X[0], ln.ps1[0]);
          }
          X[i] = min(ln.cand0(i, vs, a0), ln.cand1(i, vs, a1));
        }
#pragma unroll
        for (int i = 0; i < SPL; ++i) rows[jj * RS + ln.state(i)] = X[i];
        if constexpr (SPL > 1) __syncthreads();
      }
      if (last) {                                        // s_T and the distance, as the frames call reads them
#pragma unroll
        for (int k = 1; k < kWave; k <<= 1) asum += __shfl_xor(asum, k);
        int val;
        if (la.e >= 0) {
          sT = la.e;
          val = 0;
#pragma unroll
          for (int k = 0; k < SPL; ++k) {
            const int x = __shfl(X[k], sT & (kWave - 1));
            if ((sT >> 6) == k) val = x;
          }
        } else {
          val = X[0];
#pragma unroll
          for (int k = 1; k < SPL; ++k) val = min(val, X[k]);
#pragma unroll
          for (int k = 1; k < kWave; k <<= 1) val = min(val, __shfl_xor(val, k));
#pragma unroll
          for (int k = SPL - 1; k >= 0; --k) {
            const uint64_t bal = __ballot(lane < S && X[k] == val);
            if (bal) sT = kWave * k + __builtin_ctzll(bal);
          }
        }
        dist = ln.norm_of(val, asum);
      }
      __syncthreads();
      for (int jj = cnt - 1; jj >= 0; --jj) {            // Y = beta_{t0 + jj + 1} on entry
        const int vs = __builtin_amdgcn_readlane(vp, jj);
        int mv = rows[jj * RS + ln.state(0)] + Y[0];
#pragma unroll
        for (int i = 1; i < SPL; ++i) mv = min(mv, rows[jj * RS + ln.state(i)] + Y[i]);
        if constexpr (SPL > 1) {
#pragma unroll
          for (int i = 0; i < SPL; ++i) met[cur * S + ln.state(i)] = Y[i];
        }
        // S > 64: the exchange.  Below, a lane's alpha is read before any lane's mv is written by the
        // order of the wave's own LDS instructions: the block is one wave
        if constexpr (SPL > 1) __syncthreads();
        rows[jj * RS + lane] = mv;                       // entry's parity = the parity of the lane's states
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
          int b0, b1;
          if constexpr (SPL > 1) {
            b0 = met[cur * S + ns0[i]];
            b1 = met[cur * S + ns0[i] + 1];
          } else {
            b0 = __shfl(Y[0], ns0[0]);
            b1 = __shfl(Y[0], ns0[0] + 1);
          }
          Y[i] = min(__builtin_amdgcn_sdot4(po0[i], vs, b0, false), __builtin_amdgcn_sdot4(po1[i], vs, b1, false));
        }
        cur ^= 1;
      }
      __syncthreads();
      // lane (jj, u): M_u(t0 + jj) in the x representation
      const int jj = lane & (kLlrSeg - 1), u = lane >> 5;
      int mu = rows[jj * RS + u + 2 * jj];
#pragma unroll
      for (int k = 1; k < kLlrSeg; ++k) mu = min(mu, rows[jj * RS + u + 2 * ((k + jj) & (kLlrSeg - 1))]);
      const int m1 = __shfl_xor(mu, kLlrSeg);
      const bool live = lane < cnt;
      int L = 0;
      if (live) L = mu >= kInfTest ? kSat : m1 >= kInfTest ? -kSat : (mu - m1) / 2;
      if (lane < kLlrSeg) lrow[t0 + lane] = (int16_t)L;
      const uint64_t ones = __ballot(L > 0);
      if (lane == 0) brow[c] = (uint32_t)ones;
      const bool issat = live && abs(L) == kSat;
      zeros += (uint32_t)__builtin_popcountll(__ballot(live && L == 0));
      sat += (uint32_t)__builtin_popcountll(__ballot(issat));
      if (live && !issat) weak = min(weak, abs(L));
    }
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) weak = min(weak, __shfl_xor(weak, k));
    if (lane == 0) {
      rec[0] = dist;
      rec[1] = (int32_t)zeros;
      rec[2] = sT;
      rec[3] = 0;
      rec[4] = weak;
      rec[5] = (int32_t)sat;
    }
    tdist += (unsigned long long)dist;
    ++tdec;
    tzero += zeros;
    tsat += sat;
  }
  if (lane == 0) {
    if (tdist) atomicAdd(&la.tot[0], tdist);
    if (tdec) atomicAdd(&la.tot[1], tdec);
    if (tskip) atomicAdd(&la.tot[2], tskip);
    if (tzero) atomicAdd(&la.tot[3], tzero);
    if (tsat) atomicAdd(&la.tot[4], tsat);
    if (blockIdx.x == 0) la.tot[5] = (unsigned long long)la.w;
  }
}

using LKern = void (*)(LArgs);

// kLlrWaves, or CVD_LLR_WAVES (a test's way to another launch shape)
int64_t llr_wave_cap() {
  const char* e = getenv("CVD_LLR_WAVES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? std::min<int64_t>(v, kLlrWaves) : kLlrWaves;
}

// bytes of a wave's checkpoints: one vector of 2^m ints per segment but the first and the last
int64_t slice_bytes(int m, int64_t T) {
  const int64_t nseg = (T + kLlrSeg - 1) / kLlrSeg;
  return round16(std::max<int64_t>(nseg - 2, 0) * ((int64_t)4 << m));
}

// waves of the launch: at most the frames, the cap, and what kLlrWorkBytes holds (monotone in F)
int64_t waves_of(int m, int64_t T, int64_t F) {
  const int64_t sb = slice_bytes(m, T);
  int64_t waves = std::min(F, llr_wave_cap());
  if (sb) waves = std::min(waves, std::max<int64_t>(1, kLlrWorkBytes / sb));
  return waves;
}

// The entry points behind the code shape and the pattern.  who: the entry point's name in the
// errors; kern: its kernel for the code's shape.
int decode_llr(const char* who, LKern kern, const cvd_code* code, const cvd::VPattern* pat, const int8_t* d_soft,
               int64_t nvals, int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
               int32_t start_state, int32_t end_state, int16_t* d_llr, uint32_t* d_bits, int32_t* d_frames,
               int64_t* d_stats, void* d_work, void* stream) {
  const int n = code->n, m = code->m;
  if (nvals < 0) return invalid(who, "needs nvals >= 0");
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
    if (end > nvals) return invalid(who, "the frames do not lie inside [0, nvals)");
  }
  const int64_t sb = slice_bytes(m, T);
  if (!d_soft || !d_llr || !d_bits || !d_frames || !d_stats || (sb && !d_work) || ((uintptr_t)d_soft & 15) ||
      ((uintptr_t)d_llr & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_frames & 3) ||
      ((uintptr_t)d_stats & 7) || ((uintptr_t)d_offsets & 7))
    return invalid(who, "d_soft, d_llr, d_work (16-byte aligned; d_work null only where the workspace is 0 bytes), "
                        "d_stats (8-byte), d_bits and d_frames (4-byte) must be non-null, d_offsets 8-byte aligned");

  LArgs la{};
  VArgs& a = la.v;
  a.cap = reinterpret_cast<const uint4*>(d_soft);
  a.nu4 = nvals / 16 + (nvals % 16 != 0);
  a.format = CVD_CAPTURE_BYTES;
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
  a.bits = d_bits;
  la.offsets = d_offsets;
  la.stride = stride;
  la.nvals = nvals;
  la.F = F;
  la.slice = sb / 4;
  la.s0 = start_state;
  la.e = end_state;
  la.w = (int32_t)w;
  la.ckpt = static_cast<int*>(d_work);
  la.llr = d_llr;
  la.frames = d_frames;
  la.tot = reinterpret_cast<unsigned long long*>(d_stats);

  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats, 0, 6 * sizeof(int64_t), st));
  hipLaunchKernelGGL(kern, dim3((unsigned)waves_of(m, T, F)), dim3(kWave), 0, st, la);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

}  // namespace
