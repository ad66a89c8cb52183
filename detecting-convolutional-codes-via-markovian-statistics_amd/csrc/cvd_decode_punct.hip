// cvd_viterbi_decode_punctured (include/cvd.h) for gfx950: the capture decoder of
// cvd_decode.hip over a punctured capture.  Only the forward pass knows about the pattern:
// step t, in column c = t mod period, finds its popcount(keep[c]) transmitted bits at
// pos(t) = start + (t div period) K + pre[c] and leaves the erased outputs out of the Hamming
// distance.  Compare, look, trace and fix read decision words and are cvd_decode.hip's
// (cvd::viterbi_launch); the join kernel reruns blocks with this file's forward recursion.
// The step loop and the two kernels' bodies are cvd_decode_common.h's (acs_chunk, forward_body,
// join_body), the pattern's checks and packing cvd_decode.hip's (cvd::viterbi_pack_pattern).
//
// What PLane brings where cvd_decode.hip's Lane has its funnel and 2-bit metric fields:
//   staging   a segment of kSeg steps covers the bits [pos(seg), pos(seg + cnt)), never more
//             than n cnt; once its dwords are in LDS the lanes resolve the pattern, 16 steps
//             each: the step's column (a segment, a warm-up, a block or a rerun may begin in
//             any), keep[c], the step's popcount(keep[c]) bits at pos(t) spread into their
//             positions j.  A byte per step, y_t | keep << 4, goes to LDS.
//   per step  scalar: the byte out of an SGPR pair that holds eight steps'; vector, per branch,
//             popcount((out ^ y) & keep) + D(ps): one three-input bit operation and the count
//             instruction's add form, where the unpunctured loop has a field extract and an
//             add.  (Resolving the pattern on the scalar unit inside the step loop, 21 scalar
//             instructions a step, made the CU's one scalar unit the bound: DESIGN.md §7.12.)
// wave64, one wave per block, lane = next state, ds_bpermute for 2^m <= 64 and the
// double-buffered LDS vector above, as there.  No scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_decode_common.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr const char* kWho = "viterbi_decode_punctured";

// pos(t) of include/cvd.h, t in 0..2^31 - 1
__device__ __forceinline__ int64_t pos_of(const VArgs& a, int64_t t, uint32_t* col) {
  const uint32_t tt = (uint32_t)t, per = (uint32_t)a.period;
  const uint32_t r = tt / per, c = tt - r * per;
  *col = c;
  const uint32_t pre = (uint32_t)(a.ppre[c >> 3] >> (8u * (c & 7u))) & 255u;
  return a.start + (int64_t)r * a.K + pre;
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
  // the result as in cvd_decode.hip's Lane::run.  LDS: st kPunctStageDw dwords: the segment's
  // capture dwords, then a byte per step, y_t | keep << 4.
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

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_punct_forward_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kPunctStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  PLane<m, n> ln;
  ln.init(a);
  forward_body(a, ln, st, met);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_punct_join_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kPunctStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  PLane<m, n> ln;
  ln.init(a);
  join_body(a, ln, st, met);
}

CVD_VITERBI_PICK(viterbi_punct_forward_kernel, viterbi_punct_join_kernel)

}  // namespace

extern "C" int cvd_viterbi_decode_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                            const void* d_capture, int64_t nbits, int32_t format, int64_t start,
                                            int64_t T, int32_t block, int32_t warm, int32_t depth, uint32_t* d_bits,
                                            int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(kWho, code)) return rc;
  const int n = code->n, m = code->m;
  cvd::VPattern pat;
  if (const int rc = cvd::viterbi_pack_pattern(kWho, "bit", keep, period, n, &pat)) return rc;
  // span = pos(T) - start; -1: an int64 overflow (T > 2^31 - 1 is reported as a bad T first)
  int64_t span = 0;
  if (T > 0 && !pat.span(T, &span)) span = -1;
  VArgs a;
  bool launch;
  const int rc = cvd::viterbi_setup(kWho, code, d_capture, nbits, format, start, T, span, block, warm, depth,
                                    CVD_VITERBI_PUNCT_WARM(m, n, period, pat.K),
                                    CVD_VITERBI_PUNCT_DEPTH(m, n, period, pat.K), d_bits, d_stats, d_work, &a, &launch);
  if (rc != CVD_OK || !launch) return rc;
  a.period = period;
  a.K = pat.K;
  a.pmask = pat.pmask;
  a.ppre[0] = pat.ppre[0];
  a.ppre[1] = pat.ppre[1];
  Kern fwd, join;
  pick(m, n, &fwd, &join);
  return cvd::viterbi_launch(m, a, fwd, join, stream);
}
