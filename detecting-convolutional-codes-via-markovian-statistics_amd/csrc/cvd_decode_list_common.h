// What the list decoders share (cvd_decode_list.hip describes the design; cvd_decode_tblist.hip
// runs it lap after lap): the sort keys and their absent value, the merge of two lists, the word
// that holds a state's decisions, the loader of a chunk's values, one step of the list recursion,
// the tile of decisions in LDS with its copies to and from a wave's slice of d_work, and on the
// host the tiling and the launch shape with their two environment variables.  Everything is in
// an unnamed namespace.  Include after <hip/hip_runtime.h>.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "../../include/cvd.h"
#include "cvd_decode_common.h"
#include "cvd_decode_lanes.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr uint32_t kAbsent = 0x80000000u;          // above every key of a path
constexpr int kListWaves = 8192;                   // waves of the launch
constexpr int64_t kListWorkBytes = (int64_t)1 << 30;
// The tile of decisions in LDS.  16 KiB leaves ten waves per CU (160 KiB) at S <= 64 and six beside
// the exchange buffer of S = 256, L = 8 (8 KiB); frames of 128 steps of 64 states fit it up to L = 4.
constexpr int64_t kListLdsBytes = 16384;
constexpr int64_t kListLdsMin = 1024, kListLdsMax = 49152;   // CVD_LIST_LDS_BYTES is clamped to these

template <int LL> struct DecWord;
template <> struct DecWord<2> { using type = uint8_t; };
template <> struct DecWord<4> { using type = uint16_t; };
template <> struct DecWord<8> { using type = uint32_t; };

// the LL smallest of two ascending lists, ascending
template <int LL>
__device__ __forceinline__ void merge_lists(const uint32_t (&a)[LL], const uint32_t (&b)[LL], uint32_t (&o)[LL]) {
#pragma unroll
  for (int i = 0; i < LL; ++i) o[i] = min(a[i], b[LL - 1 - i]);
#pragma unroll
  for (int h = LL / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int i = 0; i < LL; ++i) {
      if ((i & h) == 0) {
        const uint32_t lo = min(o[i], o[i + h]), hi = max(o[i], o[i + h]);
        o[i] = lo;
        o[i + h] = hi;
      }
    }
  }
}

// lane j < cnt: the n values of step t0 + j of the frame at `frame`, packed a byte each (-128 read
// as -127), and the sum of their magnitudes; the other lanes 0.  Nothing outside the frame is read.
template <int n>
__device__ __forceinline__ void load_values(const int8_t* frame, int t0, int cnt, int lane, int& vp, int& ap) {
  vp = 0;
  ap = 0;
  if (lane < cnt) {
    const int8_t* p = frame + (int64_t)n * (t0 + lane);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const int x = max((int)p[j], -127);
      ap += abs(x);
      vp |= (x & 255) << (8 * j);
    }
  }
}

// One step of the list recursion on the lane's lists K (keys, ascending, kAbsent behind the present
// ones): vs the step's values, at the sum of their magnitudes.  xk: the exchange buffer of S > 64.
// Ranks at or above `cut` are made absent (cut = LL: none).  d[i]: the decisions of state(i), a
// nibble per rank.
template <int m, int n, int LL>
__device__ __forceinline__ void list_step(const SLane<m, n>& ln, uint32_t (&K)[Shape<m>::SPL][LL], uint32_t* xk, int vs,
                                          int at, int cut, uint32_t (&d)[Shape<m>::SPL]) {
  constexpr int S = Shape<m>::S, SPL = Shape<m>::SPL;
  if constexpr (SPL > 1) {
    __syncthreads();                                     // the step before has read xk
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
#pragma unroll
      for (int r = 0; r < LL; ++r) xk[r * S + ln.state(i)] = K[i][r];
    }
    __syncthreads();
  }
  uint32_t N[SPL][LL];
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    const uint32_t add0 = (uint32_t)ln.cand0(i, vs, at) << 4;
    const uint32_t add1 = ((uint32_t)ln.cand1(i, vs, at) << 4) | 8u;
    uint32_t c0[LL], c1[LL];
#pragma unroll
    for (int r = 0; r < LL; ++r) {
      uint32_t a0, a1;
      if constexpr (SPL > 1) {
        a0 = xk[r * S + ln.ps0[i]];
        a1 = xk[r * S + ln.ps1[i]];
      } else {
        a0 = (uint32_t)__shfl((int)K[0][r], ln.ps0[0]);
        a1 = (uint32_t)__shfl((int)K[0][r], ln.ps1[0]);
      }
      c0[r] = (a0 & ~15u) + add0 + (uint32_t)r;
      c1[r] = (a1 & ~15u) + add1 + (uint32_t)r;
    }
    merge_lists<LL>(c0, c1, N[i]);
  }
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    d[i] = 0u;
#pragma unroll
    for (int r = 0; r < LL; ++r) {
      K[i][r] = r < cut ? min(N[i][r], kAbsent) : kAbsent;
      d[i] |= (N[i][r] & 15u) << (4 * r);
    }
  }
}

extern __shared__ uint4 list_tile[];     // the tile of decisions: tile16 pieces

// The tile to the slice's piece g, from it, and exchanged with it.  A lane moves the same pieces
// in all three, so what it reads back from g is what it wrote; the barriers (the block is one
// wave) are waits on the wave's own LDS instructions.
__device__ __forceinline__ void tile_out(uint4* g, int tile16, int lane) {
  __syncthreads();
  for (int k = lane; k < tile16; k += kWave) g[k] = list_tile[k];
  __syncthreads();
}

__device__ __forceinline__ void tile_in(const uint4* g, int tile16, int lane) {
  __syncthreads();                                       // the tile behind has been read
  for (int k = lane; k < tile16; k += kWave) list_tile[k] = g[k];
  __syncthreads();
}

__device__ __forceinline__ void tile_swap(uint4* g, int tile16, int lane) {
  __syncthreads();
  for (int k = lane; k < tile16; k += kWave) {
    const uint4 x = g[k];
    g[k] = list_tile[k];
    list_tile[k] = x;
  }
  __syncthreads();
}

long long env_number(const char* name) {
  const char* e = getenv(name);
  return e ? atoll(e) : 0;
}

// kListWaves, or CVD_LIST_WAVES (a test's way to another launch shape)
int64_t list_wave_cap() {
  const long long v = env_number("CVD_LIST_WAVES");
  return v > 0 ? std::min<int64_t>(v, kListWaves) : kListWaves;
}

// kListLdsBytes, or CVD_LIST_LDS_BYTES (a measurement's way to another tile)
int64_t list_lds_bytes() {
  const long long v = env_number("CVD_LIST_LDS_BYTES");
  return v > 0 ? std::min(std::max<int64_t>(v, kListLdsMin), kListLdsMax) : kListLdsBytes;
}

int list_width(int L) { return L <= 2 ? 2 : L <= 4 ? 4 : 8; }

// how a frame's decisions are tiled: tsteps steps of 2^m LL / 2 bytes each in LDS
struct Tiling {
  int64_t tsteps, ntiles, tile_bytes, slice_bytes;
};

Tiling tiling_of(int m, int64_t T, int L) {
  const int64_t step = ((int64_t)1 << m) * list_width(L) / 2;      // <= 1024 <= kListLdsMin
  Tiling t;
  t.tsteps = std::min<int64_t>(T, list_lds_bytes() / step);
  t.ntiles = (T + t.tsteps - 1) / t.tsteps;
  t.tile_bytes = round16(t.tsteps * step);
  t.slice_bytes = (t.ntiles - 1) * t.tile_bytes;
  return t;
}

// waves of the launch: at most the frames, the cap, and what kListWorkBytes holds (monotone in F)
int64_t list_waves(const Tiling& t, int64_t F) {
  int64_t waves = std::min(F, list_wave_cap());
  if (t.slice_bytes) waves = std::min(waves, std::max<int64_t>(1, kListWorkBytes / t.slice_bytes));
  return waves;
}

// the generator taps of `code` as the lanes read them (VArgs::g0, gs)
inline void list_code_taps(const cvd_code* code, VArgs& a) {
  const int n = code->n, m = code->m;
  for (int j = 0; j < n; ++j) {
    const uint8_t* t = code->taps + (size_t)j * (m + 1);
    if (t[0] & 1) a.g0 |= 1u << j;
    for (int d = 1; d <= m; ++d)
      if (t[d] & 1) a.gs[j] |= 1u << (d - 1);
  }
}

}  // namespace
