// The lane types of the capture decoder's forward passes, by how y_t is read: Lane (every
// output bit of a step is in the capture; cvd_decode.hip describes it), PLane (a puncturing
// pattern says which are; cvd_decode_punct.hip), SLane (an int8 confidence value per bit;
// cvd_decode_soft.hip) and PSLane (values behind a pattern; frames only).  Each brings init, run<record>(a, t0, t1, D, dec, st, met) and cand0 /
// cand1 around cvd_decode_common.h's LaneBase and acs_chunk.  The stream decoders' forward and
// join kernels and the frame decoder's forward kernels (cvd_decode_frames.hip) are built around
// them.  Include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

#include "cvd_decode_common.h"

namespace cvd {
namespace vit {

template <int m, int n>
struct Lane : LaneBase<m> {
  using LaneBase<m>::S;
  using LaneBase<m>::SPL;
  using LaneBase<m>::lane;
  using LaneBase<m>::ps0;
  using LaneBase<m>::ps1;
  using LaneBase<m>::state;
  uint32_t bm0[SPL], bm1[SPL];     // the predecessors' branch metrics: bits 2y..2y+1 = d_H(out(ps_b, u), y)

  __device__ __forceinline__ void init(const VArgs& a) {
    this->init_base();
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int u = state(i) & 1;
      const uint32_t o0 = this->template branch_out<n>(a, ps0[i], u), o1 = this->template branch_out<n>(a, ps1[i], u);
      bm0[i] = bm1[i] = 0u;
#pragma unroll
      for (uint32_t y = 0; y < (1u << n); ++y) {
        bm0[i] |= (uint32_t)__builtin_popcount(o0 ^ y) << (2 * y);
        bm1[i] |= (uint32_t)__builtin_popcount(o1 ^ y) << (2 * y);
      }
    }
  }

  __device__ __forceinline__ int cand0(int i, uint32_t y2, int a) const { return a + (int)((bm0[i] >> y2) & 3u); }
  __device__ __forceinline__ int cand1(int i, uint32_t y2, int a) const { return a + (int)((bm1[i] >> y2) & 3u); }

  // steps [t0, t1) of Eq. 4-5 on D (not normalised); record: the decision words to
  // dec[(t - t0) SPL + i] (acs_chunk).  Returns 0: D is the metric itself.  LDS: st kStageDw
  // dwords, met 2 S ints (S > 64).
  template <bool record>
  __device__ __forceinline__ int run(const VArgs& a, int64_t t0, int64_t t1, int (&D)[SPL], uint64_t* dec,
                                     uint32_t* st, int* met) const {
    constexpr uint32_t ymask = (1u << n) - 1u;
    int cur = 0;
    for (int64_t seg = t0; seg < t1; seg += kSeg) {
      const int cnt = (int)min((int64_t)kSeg, t1 - seg);
      __syncthreads();                                   // the previous segment has been read
      stage_bits(a, a.start + (int64_t)n * seg, n * cnt, st, lane);
      __syncthreads();
      uint32_t q = (uint32_t)((a.start + (int64_t)n * seg) & 31);
      int dw = -1;                                       // the staged dwords dw, dw + 1 in SGPRs: y_t is scalar work
      uint32_t wlo = 0u, whi = 0u;
      for (int j0 = 0; j0 < cnt; j0 += kWave) {
        acs_chunk<record>(*this, min(kWave, cnt - j0), D, cur, met, dec + ((seg - t0) + j0) * SPL, [&](int) {
          if ((int)(q >> 5) != dw) {
            dw = (int)(q >> 5);
            wlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)st[dw]);
            whi = (uint32_t)__builtin_amdgcn_readfirstlane((int)st[dw + 1]);
          }
          const uint32_t y2 = 2u * ((uint32_t)((((uint64_t)whi << 32) | wlo) >> (q & 31u)) & ymask);
          q += n;
          return y2;
        });
      }
    }
    return 0;
  }
};

// pos(t) - start of include/cvd.h, t in 0..2^31 - 1
__device__ __forceinline__ int64_t pos_rel(const VArgs& a, int64_t t, uint32_t* col) {
  const uint32_t tt = (uint32_t)t, per = (uint32_t)a.period;
  const uint32_t r = tt / per, c = tt - r * per;
  *col = c;
  const uint32_t pre = (uint32_t)(a.ppre[c >> 3] >> (8u * (c & 7u))) & 255u;
  return (int64_t)r * a.K + pre;
}

// pos(t)
__device__ __forceinline__ int64_t pos_of(const VArgs& a, int64_t t, uint32_t* col) {
  return a.start + pos_rel(a, t, col);
}

// Step t of a punctured soft frame whose first value is v[0]: f(j, x) for every output j that the
// step's column keeps, ascending, x the value in its place.  `a` indexed by the column: in LDS.
template <class F>
__device__ __forceinline__ void kept_values(const VArgs& a, const int8_t* v, int64_t t, F f) {
  uint32_t c;
  const int8_t* p = v + pos_rel(a, t, &c);
  const uint32_t keep = (uint32_t)(a.pmask >> (4u * c)) & 7u;    // no bit at or above n
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if ((keep >> j) & 1u) f(j, (int)*p++);
}

// A soft frame's errors and counted: a lane per step (64 apart) re-encodes the step from the
// decoded bits -- s_t is the m bits before bit t of row, those before bit 0 are s0 -- and compares
// the signs of the step's values that are not 0; v: the frame's first value.  punct: the values
// are those that the pattern of `a` (in LDS) keeps.  Every lane returns the wave's sums.
template <bool punct>
__device__ __forceinline__ void count_signs(const VArgs& a, const int8_t* v, const uint32_t* row, uint32_t s0, int T,
                                            int m, int n, int lane, uint32_t& err, uint32_t& seen) {
  const uint32_t before = __builtin_bitreverse32(s0);                       // u_{-d} in bit 32 - d
  err = seen = 0u;
  for (int t = lane; t < T; t += kWave) {
    const int w = t >> 5;
    const uint32_t hi = row[w], lo = w ? row[w - 1] : before;
    const uint64_t q = ((uint64_t)hi << 32) | lo;
    const uint32_t sh = (uint32_t)(t & 31);
    const uint32_t r = (uint32_t)(q >> (sh + 32u - (uint32_t)m)) & ((1u << m) - 1u);   // bit i: u_{t-m+i}
    const uint32_t ps = __builtin_bitreverse32(r) >> (32 - m);                       // bit d-1: u_{t-d}
    const uint32_t u = (hi >> sh) & 1u;
    auto one = [&](int j, int x) {
      const uint32_t o = (((a.g0 >> j) & u) ^ (uint32_t)__builtin_popcount(a.gs[j] & ps)) & 1u;
      seen += x != 0;
      err += x != 0 && (uint32_t)(x > 0) != o;
    };
    if constexpr (punct) {
      kept_values(a, v, t, one);
    } else {
      for (int j = 0; j < n; ++j) one(j, v[(int64_t)n * t + j]);
    }
  }
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    err += __shfl_xor(err, k);
    seen += __shfl_xor(seen, k);
  }
}

template <int m, int n>
struct PLane : LaneBase<m> {
  using LaneBase<m>::S;
  using LaneBase<m>::SPL;
  using LaneBase<m>::lane;
  using LaneBase<m>::ps0;
  using LaneBase<m>::ps1;
  using LaneBase<m>::state;
  uint32_t o0[SPL], o1[SPL];       // the outputs of the lane's two branches

  __device__ __forceinline__ void init(const VArgs& a) {
    this->init_base();
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int u = state(i) & 1;
      o0[i] = this->template branch_out<n>(a, ps0[i], u);
      o1[i] = this->template branch_out<n>(a, ps1[i], u);
    }
  }

  // y: a step's byte, y_t | keep << 4
  __device__ __forceinline__ int cand0(int i, uint32_t y, int a) const {
    return __builtin_popcount((o0[i] ^ y) & (y >> 4) & 7u) + a;
  }
  __device__ __forceinline__ int cand1(int i, uint32_t y, int a) const {
    return __builtin_popcount((o1[i] ^ y) & (y >> 4) & 7u) + a;
  }

  // steps [t0, t1) of Eq. 4-5 with the pattern's metric on D (not normalised); record, met and
  // the result as in Lane::run.  LDS: st kPunctStageDw dwords: the segment's capture dwords,
  // then a byte per step, y_t | keep << 4.
  template <bool record>
  __device__ __forceinline__ int run(const VArgs& a, int64_t t0, int64_t t1, int (&D)[SPL], uint64_t* dec,
                                     uint32_t* st, int* met) const {
    int cur = 0;
    uint32_t* sy = st + kStageDw;
    const uint32_t per = (uint32_t)a.period, q64 = (uint32_t)kWave / per, r64 = (uint32_t)kWave - q64 * per;
    for (int64_t seg = t0; seg < t1; seg += kSeg) {
      const int cnt = (int)min((int64_t)kSeg, t1 - seg);
      uint32_t c0, c1;
      const int64_t p0 = pos_of(a, seg, &c0), p1 = pos_of(a, seg + cnt, &c1);
      __syncthreads();                                   // the previous segment has been read
      stage_bits(a, p0, (int)(p1 - p0), st, lane);
      __syncthreads();
      // lane l: steps seg + l, seg + l + 64, ...: the step's period and column (one division,
      // then 64 steps further each time), its bits out of the staged dwords, spread
      {
        const uint32_t tt = (uint32_t)seg + (uint32_t)lane;
        uint32_t rr = tt / per, c = tt - rr * per;
        const int64_t base = a.start - ((p0 >> 5) << 5);     // pos(t) - base: the bit's place in st
        for (int i = lane; i < cnt; i += kWave) {
          const uint32_t pre = (uint32_t)(a.ppre[c >> 3] >> (8u * (c & 7u))) & 255u;
          const uint32_t off = (uint32_t)(base + (int64_t)rr * a.K) + pre;   // < 32 + 3 kSeg
          const uint32_t keep = (uint32_t)(a.pmask >> (4u * c)) & 7u;
          uint32_t r = (uint32_t)((((uint64_t)st[(off >> 5) + 1] << 32) | st[off >> 5]) >> (off & 31u));
          uint32_t y = 0u;                               // the kept bits, j ascending, into their positions j
#pragma unroll
          for (int j = 0; j < n; ++j) {
            const uint32_t k = (keep >> j) & 1u;
            y |= (r & k) << j;
            r >>= k;
          }
          reinterpret_cast<uint8_t*>(sy)[i] = (uint8_t)(y | (keep << 4));
          rr += q64;
          c += r64;
          if (c >= per) {
            c -= per;
            ++rr;
          }
        }
      }
      __syncthreads();
      int dw = -1;                                       // eight steps' bytes in an SGPR pair: y_t, keep are scalar work
      uint32_t wlo = 0u, whi = 0u;
      for (int j0 = 0; j0 < cnt; j0 += kWave) {
        acs_chunk<record>(*this, min(kWave, cnt - j0), D, cur, met, dec + ((seg - t0) + j0) * SPL, [&](int jj) {
          const int j = j0 + jj;
          if ((j >> 3) != dw) {
            dw = j >> 3;
            wlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)sy[2 * dw]);
            whi = (uint32_t)__builtin_amdgcn_readfirstlane((int)sy[2 * dw + 1]);
          }
          return (uint32_t)((((uint64_t)whi << 32) | wlo) >> (8u * ((uint32_t)j & 7u)));
        });
      }
    }
    return 0;
  }
};

constexpr int kPunctStageDw = kStageDw + kSeg / 4;

constexpr int kSoftStageU4 = 3 * kSeg / 16 + 2;   // n <= 3: the segment's 16-byte pieces and alignment slack

template <int m, int n>
struct SLane : LaneBase<m> {
  using LaneBase<m>::S;
  using LaneBase<m>::SPL;
  using LaneBase<m>::lane;
  using LaneBase<m>::ps0;
  using LaneBase<m>::ps1;
  using LaneBase<m>::state;
  int pat0[SPL], pat1[SPL];        // byte j < n: -1 if bit j of the branch's output is 1, else +1; 0 above

  __device__ __forceinline__ static int pattern(uint32_t out) {
    uint32_t p = 0u;
#pragma unroll
    for (int j = 0; j < n; ++j) p |= (((out >> j) & 1u) ? 0xffu : 0x01u) << (8 * j);
    return (int)p;
  }

  __device__ __forceinline__ void init(const VArgs& a) {
    this->init_base();
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int u = state(i) & 1;
      pat0[i] = pattern(this->template branch_out<n>(a, ps0[i], u));
      pat1[i] = pattern(this->template branch_out<n>(a, ps1[i], u));
    }
  }

  // The loop's x = 2 D - sum A_t; the vectors in memory are D, 16-bit, and the end vector also
  // the byte min(D, 255) that look and fix test for zero.
  __device__ __forceinline__ void store16(uint16_t* vec, uint8_t* bytes, const int (&X)[SPL]) const {
    if (lane < S) {
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
        const int d = X[i] >> 1;
        vec[state(i)] = (uint16_t)d;
        if (bytes) bytes[state(i)] = (uint8_t)min(d, 255);
      }
    }
  }
  __device__ __forceinline__ void store_warm(const VArgs& a, int64_t b, const int (&X)[SPL]) const {
    store16(a.warm16 + b * S, nullptr, X);
  }
  __device__ __forceinline__ void store_end(const VArgs& a, int64_t b, const int (&X)[SPL]) const {
    store16(a.end16 + b * S, a.endv + b * S, X);
  }
  __device__ __forceinline__ void load_end(const VArgs& a, int64_t b, int (&X)[SPL]) const {
#pragma unroll
    for (int i = 0; i < SPL; ++i) X[i] = 2 * (int)a.end16[b * S + state(i)];
  }
  __device__ __forceinline__ bool differs_from_warm(const VArgs& a, int64_t b, const int (&X)[SPL]) const {
    bool diff = false;
#pragma unroll
    for (int i = 0; i < SPL; ++i) diff |= X[i] != 2 * (int)a.warm16[b * S + state(i)];
    return diff;
  }
  __device__ __forceinline__ static int norm_of(int mn, int asum) { return (mn + asum) >> 1; }

  // vs: a step's n values, packed
  __device__ __forceinline__ int cand0(int i, int vs, int x) const { return __builtin_amdgcn_sdot4(pat0[i], vs, x, false); }
  __device__ __forceinline__ int cand1(int i, int vs, int x) const { return __builtin_amdgcn_sdot4(pat1[i], vs, x, false); }

  // steps [t0, t1) on x (not normalised); record as in Lane::run.  Returns the sum of A_t over
  // the steps.  LDS: st kSoftStageU4 pieces, met 2 S ints (S > 64).
  template <bool record>
  __device__ __forceinline__ int run(const VArgs& a, int64_t t0, int64_t t1, int (&X)[SPL], uint64_t* dec, uint4* st,
                                     int* met) const {
    int cur = 0;
    int asum = 0;                                        // this lane's share of sum A_t
    const int8_t* sb = reinterpret_cast<const int8_t*>(st);
    for (int64_t seg = t0; seg < t1; seg += kSeg) {
      const int cnt = (int)min((int64_t)kSeg, t1 - seg);
      const int64_t p0 = a.start + (int64_t)n * seg;     // the segment's first value
      const int64_t g0 = p0 >> 4;
      const int off = (int)(p0 & 15);
      const int npc = (off + n * cnt + 15) >> 4;         // <= kSoftStageU4 - 1
      __syncthreads();                                   // the previous segment has been read
      for (int i = lane; i < npc; i += kWave) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (g0 + i < a.nu4) v = a.cap[g0 + i];
        st[i] = v;
      }
      __syncthreads();
      for (int j0 = 0; j0 < cnt; j0 += kWave) {
        const int c64 = min(kWave, cnt - j0);
        int vp = 0;                                      // lane j: the n values of the chunk's step j, packed
        if (lane < c64) {
          const int8_t* p = sb + off + n * (j0 + lane);
#pragma unroll
          for (int j = 0; j < n; ++j) {
            const int v = max((int)p[j], -127);
            asum += abs(v);
            vp |= (v & 255) << (8 * j);
          }
        }
        acs_chunk<record>(*this, c64, X, cur, met, dec + ((seg - t0) + j0) * SPL,
                          [&](int jj) { return __builtin_amdgcn_readlane(vp, jj); });
      }
    }
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) asum += __shfl_xor(asum, k);
    return asum;
  }
};

// SLane behind a puncturing pattern (the frame decoders' punctured soft calls,
// cvd_decode_psoft.hip): the candidates, the vectors and the step loop are SLane's; the loader
// places a step's kept values as PLane places its kept bits, and a byte that the column erases
// is 0, which is what the contract's v' holds there.
template <int m, int n>
struct PSLane : SLane<m, n> {
  using SLane<m, n>::SPL;
  using SLane<m, n>::lane;

  // as SLane::run; a: in LDS (indexed by the column).  LDS: st kSoftStageU4 pieces: the kept
  // values of a segment are at most its n cnt values.
  template <bool record>
  __device__ __forceinline__ int run(const VArgs& a, int64_t t0, int64_t t1, int (&X)[SPL], uint64_t* dec, uint4* st,
                                     int* met) const {
    int cur = 0;
    int asum = 0;
    const int8_t* sb = reinterpret_cast<const int8_t*>(st);
    const uint32_t per = (uint32_t)a.period, q64 = (uint32_t)kWave / per, r64 = (uint32_t)kWave - q64 * per;
    for (int64_t seg = t0; seg < t1; seg += kSeg) {
      const int cnt = (int)min((int64_t)kSeg, t1 - seg);
      uint32_t c0, c1;
      const int64_t p0 = pos_of(a, seg, &c0), p1 = pos_of(a, seg + cnt, &c1);   // the segment's values: [p0, p1)
      const int64_t g0 = p0 >> 4;
      const int npc = (int)(((p1 + 15) >> 4) - g0);      // <= kSoftStageU4 - 1
      __syncthreads();                                   // the previous segment has been read
      for (int i = lane; i < npc; i += kWave) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (g0 + i < a.nu4) v = a.cap[g0 + i];
        st[i] = v;
      }
      __syncthreads();
      // lane l: steps seg + l, seg + l + 64, ...: the step's period and column as in PLane::run
      const uint32_t tt = (uint32_t)seg + (uint32_t)lane;
      uint32_t rr = tt / per, c = tt - rr * per;
      const int64_t base = a.start - (g0 << 4);          // pos(t) - base: the value's place in st
      for (int j0 = 0; j0 < cnt; j0 += kWave) {
        const int c64 = min(kWave, cnt - j0);
        int vp = 0;                                      // lane j: the chunk's step j, kept values at their bytes j
        if (lane < c64) {
          const uint32_t pre = (uint32_t)(a.ppre[c >> 3] >> (8u * (c & 7u))) & 255u;
          const uint32_t keep = (uint32_t)(a.pmask >> (4u * c)) & 7u;
          const int8_t* p = sb + ((uint32_t)(base + (int64_t)rr * a.K) + pre);   // < 16 + 3 kSeg
#pragma unroll
          for (int j = 0; j < n; ++j) {
            if ((keep >> j) & 1u) {
              const int v = max((int)*p++, -127);
              asum += abs(v);
              vp |= (v & 255) << (8 * j);
            }
          }
        }
        rr += q64;
        c += r64;
        if (c >= per) {
          c -= per;
          ++rr;
        }
        acs_chunk<record>(*this, c64, X, cur, met, dec + ((seg - t0) + j0) * SPL,
                          [&](int jj) { return __builtin_amdgcn_readlane(vp, jj); });
      }
    }
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) asum += __shfl_xor(asum, k);
    return asum;
  }
};

}  // namespace vit
}  // namespace cvd
