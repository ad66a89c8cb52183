// What the tail-biting frame decoders share (cvd_decode_tailbite.hip describes the design; its
// kernels and cvd_decode_psoft.hip's are built from this): the kernel arguments, the fused
// kernels' body around a lane type, and the host path behind the entry points.  Everything is in
// an unnamed namespace, so that a kernel taking TArgs keeps its name whichever file defines it.
// Include after <hip/hip_runtime.h>.
#pragma once
#include <limits.h>
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

constexpr int kTailWaves = 8192;                    // waves of a launch (256 CUs x 4 SIMDs x 8)
constexpr int64_t kLdsBytes = 8192;                 // a frame's decision words up to this stay in LDS
constexpr int64_t kLdsBytesMax = 32768;             // what CVD_TAILBITE_LDS_BYTES may raise it to
constexpr int64_t kTailWorkBytes = (int64_t)1 << 30;    // the waves' slices together

struct TArgs {
  VArgs v;                   // cap, nu4, format, T, the code, the pattern, span, bits; dec: d_work; start: of frame 0
  const int64_t* offsets;    // o_f, or null: o_f = v.start + f stride
  int64_t stride, nbits;
  int64_t F;
  int64_t fstride;           // decision words of a frame: T rounded up to 64 steps
  int32_t laps;              // I
  int32_t w;                 // words of a row of bits
  int32_t lds;               // the decision words live in dynamic LDS
  int32_t* frames;           // [F][8]
  unsigned long long* tot;   // d_stats
};

__device__ __forceinline__ int64_t frame_offset(const TArgs& ta, int64_t f) {
  if (!ta.offsets) return ta.v.start + f * ta.stride;
  const int64_t o = ta.offsets[f];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)o >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// step t of a chain at state s (= s_{t+1}): the decision bit of s in the step's words w[0..SPL)
// (scalars, not an array of words: that one the compiler keeps in scratch at SPL = 4)
template <int SPL>
__device__ __forceinline__ int decision(const uint64_t* w, int s) {
  uint64_t x = w[0];
#pragma unroll
  for (int j = 1; j < SPL; ++j) {
    const uint64_t y = w[j];
    if ((s >> 6) == j) x = y;
  }
  return (int)((x >> (s & 63)) & 1ull);
}

// The three kernels' body around a lane type: the wave's frames one after the other.  PLane's
// copy of the arguments lives in LDS (sa), for the reason frame_body of cvd_decode_frames.hip
// gives, and so does PSLane's: soft with lds_args is the punctured soft decoder, whose sign count
// reads the kept values.  sel: S ints of LDS, the lap's start vector by state.
template <int m, int n, bool soft, bool lds_args, class LaneT, class St>
__device__ __forceinline__ void tailbite_body(const TArgs& ta, LaneT& ln, St* st, int* met, int* sel, uint64_t* dec,
                                              VArgs* sa = nullptr) {
  constexpr int S = LaneT::S, SPL = LaneT::SPL;
  const int T = (int)ta.v.T;
  // distance, decoded, skipped, errors, counted, status 2, status 3, laps
  unsigned long long tot[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  for (int64_t f = blockIdx.x; f < ta.F; f += gridDim.x) {
    const int64_t o = frame_offset(ta, f);
    int32_t* rec = ta.frames + f * 8;
    uint32_t* row = ta.v.bits + f * ta.w;
    if (o < 0 || o > ta.nbits - ta.v.span) {             // offset mode only: the host has checked the stride
      if (ln.lane < 8) rec[ln.lane] = ln.lane == 3 ? 1 : (ln.lane == 1 || ln.lane == 2) ? -1 : 0;
      for (int k = ln.lane; k < ta.w; k += kWave) row[k] = 0u;
      ++tot[2];
      continue;
    }
    if constexpr (lds_args) {
      __syncthreads();                                   // the frame before has been read
      if (ln.lane == 0) sa->start = o;
      __syncthreads();
    }
    int E[SPL], DT[SPL], a0[SPL], c[SPL];                // E^{l-1} = D^l_0; D^l_T, a^l and c^l of the lane's end states
#pragma unroll
    for (int k = 0; k < SPL; ++k) E[k] = 0;
    int lap = 0, status, e;
    for (;;) {
      ++lap;
      int D[SPL];
#pragma unroll
      for (int k = 0; k < SPL; ++k) D[k] = soft ? 2 * E[k] : E[k];
      int sum;
      if constexpr (lds_args) {
        sum = ln.template run<true>(*sa, 0, T, D, dec, st, met);
      } else {
        VArgs a = ta.v;
        a.start = o;
        sum = ln.template run<true>(a, 0, T, D, dec, st, met);
      }
      if (ln.lane < S) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) sel[ln.state(k)] = E[k];
      }
      __syncthreads();                                   // the decision words and sel are written
      int mn;
      {
#pragma unroll
        for (int k = 0; k < SPL; ++k) DT[k] = ln.norm_of(D[k], sum);
        mn = DT[0];
#pragma unroll
        for (int k = 1; k < SPL; ++k) mn = min(mn, DT[k]);
#pragma unroll
        for (int k = 1; k < kWave; k <<= 1) mn = min(mn, __shfl_xor(mn, k));
      }
      int es = 0;                                        // e*: the lowest-index state of minimal D_T
#pragma unroll
      for (int k = SPL - 1; k >= 0; --k) {
        const uint64_t bal = __ballot(ln.lane < S && DT[k] == mn);
        if (bal) es = kWave * k + __builtin_ctzll(bal);
      }
      int s[SPL];
#pragma unroll
      for (int k = 0; k < SPL; ++k) s[k] = ln.state(k);
#pragma unroll 4
      for (int t = T - 1; t >= 0; --t) {
        const uint64_t* w = dec + t * SPL;
#pragma unroll
        for (int k = 0; k < SPL; ++k) s[k] = (s[k] >> 1) | (decision<SPL>(w, s[k]) << (m - 1));
      }
      bool closes = false, own = false;                  // e* in B; the lane has a state of B
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        a0[k] = s[k];
        c[k] = DT[k] - sel[s[k]];
        const bool in = s[k] == ln.state(k);
        own |= in;
        closes |= in && ln.state(k) == es;
      }
      if (__any(closes)) {
        status = 0;
        e = es;
        break;
      }
      bool same = lap >= 2;
#pragma unroll
      for (int k = 0; k < SPL; ++k) same &= DT[k] - mn == E[k];
      if (lap == ta.laps || __all(same)) {
        status = 3;
        e = es;
        if (__any(own)) {
          int best = INT_MAX;
#pragma unroll
          for (int k = 0; k < SPL; ++k)
            if (a0[k] == ln.state(k)) best = min(best, c[k]);
#pragma unroll
          for (int k = 1; k < kWave; k <<= 1) best = min(best, __shfl_xor(best, k));
#pragma unroll
          for (int k = SPL - 1; k >= 0; --k) {
            const uint64_t bal = __ballot(ln.lane < S && a0[k] == ln.state(k) && c[k] == best);
            if (bal) e = kWave * k + __builtin_ctzll(bal);
          }
          status = 2;
        }
        break;
      }
#pragma unroll
      for (int k = 0; k < SPL; ++k) E[k] = DT[k] - mn;
    }
    int val = 0, s0 = 0;                                 // c(e), a(e)
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int x = __shfl(c[k], e & (kWave - 1)), y = __shfl(a0[k], e & (kWave - 1));
      if ((e >> 6) == k) {
        val = x;
        s0 = y;
      }
    }
    {
      int sc = e;                                        // the chosen chain: wave-uniform
      uint32_t out = 0u;
#pragma unroll 4
      for (int t = T - 1; t >= 0; --t) {
        out |= (uint32_t)(sc & 1) << (t & 31);
        sc = (sc >> 1) | (decision<SPL>(dec + t * SPL, sc) << (m - 1));
        if ((t & 31) == 0) {
          if (ln.lane == 0) row[t >> 5] = out;
          out = 0u;
        }
      }
    }
    int errs = val, seen = (int)ta.v.span;
    if constexpr (soft) {
      __syncthreads();                                   // the row is written
      const int8_t* v = reinterpret_cast<const int8_t*>(ta.v.cap) + o;
      uint32_t err, cnt;
      if constexpr (lds_args)                            // values behind a pattern: those it keeps
        count_signs<true>(*sa, v, row, (uint32_t)s0, T, m, n, ln.lane, err, cnt);
      else
        count_signs<false>(ta.v, v, row, (uint32_t)s0, T, m, n, ln.lane, err, cnt);
      errs = (int)err;
      seen = (int)cnt;
    }
    if (ln.lane < 8) {
      const int l = ln.lane;
      rec[l] = l == 0 ? val : l == 1 ? s0 : l == 2 ? e : l == 3 ? status : l == 4 ? errs : l == 5 ? seen : l == 6 ? lap : 0;
    }
    tot[0] += (unsigned long long)val;
    ++tot[1];
    tot[3] += (unsigned long long)errs;
    tot[4] += (unsigned long long)seen;
    tot[5] += status == 2;
    tot[6] += status == 3;
    tot[7] += (unsigned long long)lap;
  }
  if (ln.lane == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (tot[q]) atomicAdd(&ta.tot[q < 5 ? q : q + 1], tot[q]);
    if (blockIdx.x == 0) ta.tot[5] = (unsigned long long)ta.w;
  }
}

extern __shared__ uint64_t lds_dec[];

// The body once per placement, not one body behind a pointer chosen at run time: the compiler
// then knows the address space of every access to the decision words (ds_* and global_*; the
// chosen pointer made them all flat_*, which count against both the LDS and the memory counter).
#define CVD_TAILBITE_BODY(SOFT, LDS_ARGS, ...)                                                        \
  do {                                                                                                \
    if (ta.lds)                                                                                       \
      tailbite_body<m, n, SOFT, LDS_ARGS>(ta, ln, st, met, sel, lds_dec, ##__VA_ARGS__);              \
    else                                                                                              \
      tailbite_body<m, n, SOFT, LDS_ARGS>(ta, ln, st, met, sel, ta.v.dec + (int64_t)blockIdx.x * ta.fstride, \
                                          ##__VA_ARGS__);                                             \
  } while (0)

using TKern = void (*)(TArgs);
#define CVD_T_ROW(KERN, n) {KERN<1, n>, KERN<2, n>, KERN<3, n>, KERN<4, n>, KERN<5, n>, KERN<6, n>, KERN<7, n>, KERN<8, n>}
#define CVD_T_TABLE(KERN) {CVD_T_ROW(KERN, 2), CVD_T_ROW(KERN, 3)}

// kLdsBytes, or CVD_TAILBITE_LDS_BYTES (the measurement's and a test's way to the other placement)
int64_t lds_bytes() {
  const char* e = getenv("CVD_TAILBITE_LDS_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? std::min<int64_t>(v, kLdsBytesMax) : kLdsBytes;
}

// kTailWaves, or CVD_TAILBITE_WAVES (a test's way to another launch shape)
int64_t tail_wave_cap() {
  const char* e = getenv("CVD_TAILBITE_WAVES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? std::min<int64_t>(v, kTailWaves) : kTailWaves;
}

bool in_lds(int m, int64_t T) { return frame_bytes(m, T) <= lds_bytes(); }

// the workspace of F frames: a slice per wave, together at most kTailWorkBytes (monotone in F and in T)
int64_t tail_work_bytes(int m, int64_t T, int64_t F) {
  if (in_lds(m, T)) return 0;
  return std::min(std::min(F, tail_wave_cap()) * frame_bytes(m, T), kTailWorkBytes);
}

// The entry points behind the code shape and the pattern.  who: the entry point's name in the
// errors; kern: its kernel for the code's shape.
int decode_tailbiting(const char* who, TKern kern, const cvd_code* code, const cvd::VPattern* pat, const void* d_capture,
                      int64_t nbits, int32_t format, int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                      int32_t T, int32_t max_laps, uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                      void* stream) {
  const int n = code->n, m = code->m;
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES)
    return invalid(who, "unknown capture format");
  if (nbits < 0) return invalid(who, "needs nbits >= 0");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (max_laps < 0 || max_laps > CVD_VITERBI_TAILBITING_MAX_LAPS)
    return invalid(who, "max_laps must be 1..8, or 0 for the default");
  if (!d_offsets && (start < 0 || stride < 1)) return invalid(who, "needs start >= 0 and stride >= 1");
  if (F == 0) return CVD_OK;
  if (T < 1 || T > CVD_VITERBI_FRAME_MAX_T) return invalid(who, "T must be 1..65536");
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
  const int64_t wbytes = tail_work_bytes(m, T, F);
  if (!d_capture || !d_bits || !d_frames || !d_stats || (wbytes && !d_work) || ((uintptr_t)d_capture & 15) ||
      ((uintptr_t)d_work & 15) || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_frames & 3) || ((uintptr_t)d_stats & 7) ||
      ((uintptr_t)d_offsets & 7))
    return invalid(who, "d_capture, d_work (16-byte aligned; null only where the workspace is 0 bytes), d_stats (8-byte), "
                        "d_bits and d_frames (4-byte) must be non-null, d_offsets 8-byte aligned");

  TArgs ta{};
  VArgs& a = ta.v;
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
  ta.offsets = d_offsets;
  ta.stride = stride;
  ta.nbits = nbits;
  ta.F = F;
  ta.fstride = frame_bytes(m, T) / 8;
  ta.laps = max_laps ? max_laps : CVD_VITERBI_TAILBITING_LAPS;
  ta.w = (int32_t)w;
  ta.lds = wbytes == 0;
  ta.frames = d_frames;
  ta.tot = reinterpret_cast<unsigned long long*>(d_stats);

  const int64_t waves = std::min(F, ta.lds ? tail_wave_cap() : wbytes / frame_bytes(m, T));
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats, 0, 9 * sizeof(int64_t), st));
  hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(kWave), ta.lds ? (size_t)frame_bytes(m, T) : 0, st, ta);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

}  // namespace
