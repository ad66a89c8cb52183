// What the three forward passes of the capture decoder share (cvd_decode.hip: every output bit
// of a step is in the capture; cvd_decode_punct.hip: a puncturing pattern says which are;
// cvd_decode_soft.hip: an int8 confidence value per bit): the kernel arguments, the staging of
// capture bits into LDS, the part of a lane's state that does not depend on how y_t is read,
// the step loop of Eq. 4-5 (acs_chunk: metric exchange, add-compare-select with the tie rule,
// decision words) around the lane type's candidate metric, and the forward and join kernels'
// bodies around its run().  A lane type brings init, run (staging, the symbol of a step, what
// persists between chunks), cand0 / cand1, and, where its vectors are not 8-bit, the four vector
// members and norm_of.  Behind the device code: what the three files' host code shares beside
// the functions that cvd_internal.h declares (HIP_CHECK, invalid / unsupported, round16, the
// kernel table).  Include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_internal.h"

namespace cvd {
namespace vit {

constexpr int kWave = 64;
constexpr int kSeg = 1024;                   // steps staged at once (a multiple of 64)
constexpr int kStageDw = 3 * kSeg / 32 + 4;  // n <= 3: the segment's dwords, alignment slack, funnel word
// The frame decoders' +inf at a boundary state that is known: even, above every finite metric
// with room for T steps on top (kInf + 127 * 3 * 65536 < 2^31; two of them and
// 2 * 127 * 3 * 65536 stay below 2^31 in the soft-output decoder's alpha + beta)
constexpr int kInf = 1 << 28;

template <int m>
struct Shape {
  static constexpr int S = 1 << m;
  static constexpr int SPL = S > kWave ? S / kWave : 1;   // states per lane = 64-bit words per decision
};

struct VArgs {
  const uint4* cap;
  int64_t nu4;            // readable 16-byte pieces of the capture
  int32_t format;
  int64_t start, T;
  int32_t L, W, D;
  int64_t nb;
  uint32_t gs[3];         // output j: taps of delays 1..m as a mask over the state
  uint32_t g0;            // bit j: tap of delay 0 of output j
  uint64_t* dec;          // [nb L][SPL] decision words
  uint8_t* warm;          // [nb][S]
  uint8_t* endv;          // [nb][S]
  int32_t* norm;          // [nb] min of the block's unnormalised end vector
  int32_t* sst;           // [nb] traced state at step bL
  int32_t* xs;            // [nb] state at step (b+1)L that block b traces from (certified blocks)
  int32_t* mis;           // [nb] warm vector of b != forward pass's end vector of b - 1
  int32_t* unc;           // [nb] block not certified by its lookahead
  unsigned long long* cnt;  // errors, forward reruns, traceback fix-ups
  uint32_t* bits;
  int64_t* stats;
  // the puncturing pattern (cvd_decode_punct.hip; period = 0: none, stats[9] is not written)
  int64_t span;           // stats[9]: pos(T) - start, the capture bits consumed
  int32_t period, K;      // columns, and the capture bits of one period
  uint64_t pmask;         // bits 4c..4c+3: keep[c]
  uint64_t ppre[2];       // byte c: pre[c], the capture bits of a period before column c
  // the soft decoder's 16-bit metric vectors (cvd_decode_soft.hip: D <= 127 n m; null elsewhere).
  // Its capture is cap read as int8, one value per byte; endv holds min(D, 255), which is all
  // that look and fix ask of it (is D zero?).
  uint16_t* warm16;       // [nb][S]
  uint16_t* end16;        // [nb][S]
};

// capture bits [p0, p0 + span) as LSB-first dwords from the dword that holds the first, and one
// more (the funnel word); span <= 3 kSeg
__device__ __forceinline__ void stage_bits(const VArgs& a, int64_t p0, int span, uint32_t* st, int lane) {
  const int64_t g0 = p0 >> 5;
  const int ndw = ((int)(p0 & 31) + span + 31) / 32 + 1;       // <= kStageDw
  for (int i = lane; i < ndw; i += kWave) {
    const int64_t g = g0 + i;
    uint32_t v = 0u;
    if (a.format != CVD_CAPTURE_BYTES) {
      if ((g >> 2) < a.nu4) {
        v = reinterpret_cast<const uint32_t*>(a.cap)[g];
        if (a.format == CVD_CAPTURE_MSB) v = lsb_first(v);
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t piece = 2 * g + h;
        if (piece < a.nu4) {
          const uint4 u = a.cap[piece];
          v |= (byte_bits4(u.x) | (byte_bits4(u.y) << 4) | (byte_bits4(u.z) << 8) | (byte_bits4(u.w) << 12)) << (16 * h);
        }
      }
    }
    st[i] = v;
  }
}

// lane = next state: its predecessors, and the metric vector's normalisation, loads and stores
template <int m>
struct LaneBase {
  static constexpr int S = Shape<m>::S, SPL = Shape<m>::SPL;
  int lane;
  int ps0[SPL], ps1[SPL];          // predecessors of the lane's next states

  __device__ __forceinline__ int state(int i) const { return (lane & (S - 1)) + kWave * i; }

  __device__ __forceinline__ void init_base() {
    lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      ps0[i] = state(i) >> 1;
      ps1[i] = ps0[i] | (1 << (m - 1));
    }
  }

  // the n output bits of the branch from state ps with input u
  template <int n>
  __device__ __forceinline__ uint32_t branch_out(const VArgs& a, int ps, int u) const {
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const uint32_t in = (a.g0 >> j) & (uint32_t)u;
      o |= ((in ^ (uint32_t)__builtin_popcount(a.gs[j] & (uint32_t)ps)) & 1u) << j;
    }
    return o;
  }

  // D -= min D over the states; returns the min
  __device__ __forceinline__ int normalise(int (&D)[SPL]) const {
    int mn = D[0];
#pragma unroll
    for (int i = 1; i < SPL; ++i) mn = min(mn, D[i]);
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) mn = min(mn, __shfl_xor(mn, k));
#pragma unroll
    for (int i = 0; i < SPL; ++i) D[i] -= mn;
    return mn;
  }

  __device__ __forceinline__ void store(uint8_t* vec, const int (&D)[SPL]) const {
    if (lane < S) {
#pragma unroll
      for (int i = 0; i < SPL; ++i) vec[state(i)] = (uint8_t)D[i];
    }
  }

  __device__ __forceinline__ void load(const uint8_t* vec, int (&D)[SPL]) const {
#pragma unroll
    for (int i = 0; i < SPL; ++i) D[i] = vec[state(i)];
  }

  // the bodies' view of block b's vectors (8-bit here), and of its normalisation: mn = min D
  // before normalising, sum = what run returned
  __device__ __forceinline__ void store_warm(const VArgs& a, int64_t b, const int (&D)[SPL]) const { store(a.warm + b * S, D); }
  __device__ __forceinline__ void store_end(const VArgs& a, int64_t b, const int (&D)[SPL]) const { store(a.endv + b * S, D); }
  __device__ __forceinline__ void load_end(const VArgs& a, int64_t b, int (&D)[SPL]) const { load(a.endv + b * S, D); }
  __device__ __forceinline__ bool differs_from_warm(const VArgs& a, int64_t b, const int (&D)[SPL]) const {
    bool diff = false;
#pragma unroll
    for (int i = 0; i < SPL; ++i) diff |= D[i] != (int)a.warm[b * S + state(i)];
    return diff;
  }
  __device__ __forceinline__ static int norm_of(int mn, int sum) { return mn; }
};

// At most 64 steps of Eq. 4-5 on D (not normalised): symbol(jj) is the wave-uniform received
// symbol of the chunk's step jj, ln.cand0 / cand1(i, y, a) the metric of next state state(i)
// through its predecessor ps0[i] / ps1[i], whose metric is a.  The predecessors' metrics come
// over ds_bpermute, for S > 64 through the double-buffered LDS vector met (2 S ints; cur says
// which half is next).  record: lane j keeps the decision word of step j (the ballot of
// "predecessor 1 strictly smaller", the lanes that repeat states masked out) and after the
// chunk the wave stores its c64 words to dec[j SPL + i] as one contiguous piece (a slot per
// step in LDS instead, one ds_write_b64 per step, made the loop LDS-bound: the two ds_bpermute
// already take two thirds of the LDS pipe's time).
template <bool record, class LaneT, class Symbol>
__device__ __forceinline__ void acs_chunk(const LaneT& ln, int c64, int (&D)[LaneT::SPL], int& cur, int* met,
                                          uint64_t* dec, Symbol symbol) {
  constexpr int S = LaneT::S, SPL = LaneT::SPL;
  uint32_t mlo[SPL], mhi[SPL];
#pragma unroll
  for (int i = 0; i < SPL; ++i) mlo[i] = mhi[i] = 0u;
  for (int jj = 0; jj < c64; ++jj) {
    const auto y = symbol(jj);
    if constexpr (SPL > 1) {
#pragma unroll
      for (int i = 0; i < SPL; ++i) met[cur * S + ln.state(i)] = D[i];
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      int a0, a1;
      if constexpr (SPL > 1) {
        a0 = met[cur * S + ln.ps0[i]];
        a1 = met[cur * S + ln.ps1[i]];
      } else {
        a0 = __shfl(D[0], ln.ps0[0]);
        a1 = __shfl(D[0], ln.ps1[0]);
      }
      const int c0 = ln.cand0(i, y, a0), c1 = ln.cand1(i, y, a1);
      bool d = c1 < c0;                                  // ties keep b = 0
      D[i] = min(c0, c1);
      if constexpr (record) {
        if constexpr (S < kWave) d = d && ln.lane < S;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(d);
        if (ln.lane == jj) {
          mlo[i] = (uint32_t)bal;
          mhi[i] = (uint32_t)(bal >> 32);
        }
      }
    }
    cur ^= 1;
  }
  if constexpr (record) {
    if (ln.lane < c64) {
#pragma unroll
      for (int i = 0; i < SPL; ++i) dec[ln.lane * SPL + i] = ((uint64_t)mhi[i] << 32) | mlo[i];
    }
  }
}

// The forward kernel's and the join kernel's bodies around a lane type whose
// run<record>(a, t0, t1, D, dec, st, met) does steps [t0, t1) of Eq. 4-5 and returns what
// enters the normalisation beside min D (0 where D is the metric itself).

// block b's steps from the vector at its start: decisions, end vector and normalisation
template <class LaneT, class St>
__device__ __forceinline__ void block_body(const VArgs& a, LaneT& ln, int64_t b, int (&D)[LaneT::SPL], St* st, int* met) {
  const int64_t lo = b * a.L, hi = min(a.T, lo + a.L);
  const int sum = ln.template run<true>(a, lo, hi, D, a.dec + lo * LaneT::SPL, st, met);
  const int mn = ln.normalise(D);
  ln.store_end(a, b, D);
  if (ln.lane == 0) a.norm[b] = ln.norm_of(mn, sum);
}

template <class LaneT, class St>
__device__ __forceinline__ void forward_body(const VArgs& a, LaneT& ln, St* st, int* met) {
  constexpr int SPL = LaneT::SPL;
  const int64_t b = blockIdx.x;
  const int64_t lo = b * a.L, t0 = max((int64_t)0, lo - a.W);
  int D[SPL];
#pragma unroll
  for (int i = 0; i < SPL; ++i) D[i] = 0;
  if (t0 < lo) {
    ln.template run<false>(a, t0, lo, D, nullptr, st, met);
    ln.normalise(D);
  }
  ln.store_warm(a, b, D);
  block_body(a, ln, b, D, st, met);
}

template <class LaneT, class St>
__device__ __forceinline__ void join_body(const VArgs& a, LaneT& ln, St* st, int* met) {
  int D[LaneT::SPL];
  unsigned long long reruns = 0;
  int64_t b = 1;
  while (b < a.nb) {
    const int64_t idx = b + ln.lane;
    const uint64_t bal = __ballot(idx < a.nb && a.mis[idx] != 0);
    if (!bal) { b += kWave; continue; }
    b += __builtin_ctzll(bal);
    ln.load_end(a, b - 1, D);                            // block b - 1 stands: its end vector is the true one
    while (b < a.nb) {
      if (!__any(ln.differs_from_warm(a, b, D))) break;
      ++reruns;
      block_body(a, ln, b, D, st, met);
      ++b;
    }
    ++b;                                                 // block b joined: scan on behind it
  }
  if (ln.lane == 0) a.cnt[1] = reruns;
}

// ── host side ──

#define HIP_CHECK(x)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      cvd::set_error(std::string("HIP error '") + hipGetErrorString(e_) + "' at " #x);     \
      return CVD_E_HIP;                                                                   \
    }                                                                                     \
  } while (0)

inline int invalid(const char* who, const char* what) {
  cvd::set_error(std::string(who) + ": " + what);
  return CVD_E_INVALID;
}

inline int unsupported(const char* who, const char* what) {
  cvd::set_error(std::string(who) + ": " + what);
  return CVD_E_UNSUPPORTED;
}

inline int64_t round16(int64_t x) { return (x + 15) / 16 * 16; }

// bytes of a frame's decision words (the frame decoders): T rounded up to 64 steps of max(8, 2^m / 8) bytes
inline int64_t frame_bytes(int m, int64_t T) {
  const int64_t spl = ((int64_t)1 << m) > kWave ? ((int64_t)1 << m) / kWave : 1;
  return (T + 63) / 64 * 64 * spl * 8;
}

// pick(m, n, &fwd, &join): a file's forward and join kernels of a code shape (m in 1..8, n in 2..3)
using Kern = void (*)(VArgs);
#define CVD_V_ROW(KERN, n) {KERN<1, n>, KERN<2, n>, KERN<3, n>, KERN<4, n>, KERN<5, n>, KERN<6, n>, KERN<7, n>, KERN<8, n>}
#define CVD_VITERBI_PICK(FWD, JOIN)                                          \
  void pick(int m, int n, Kern* fwd, Kern* join) {                           \
    static const Kern f[2][8] = {CVD_V_ROW(FWD, 2), CVD_V_ROW(FWD, 3)};      \
    static const Kern j[2][8] = {CVD_V_ROW(JOIN, 2), CVD_V_ROW(JOIN, 3)};    \
    *fwd = f[n - 2][m - 1];                                                  \
    *join = j[n - 2][m - 1];                                                 \
  }

}  // namespace vit
}  // namespace cvd
