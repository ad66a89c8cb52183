// cvd_viterbi_decode_punctured (include/cvd.h) for gfx950: the capture decoder of
// cvd_decode.hip over a punctured capture.  Only the forward pass knows about the pattern:
// step t, in column c = t mod period, finds its popcount(keep[c]) transmitted bits at
// pos(t) = start + (t div period) K + pre[c] and leaves the erased outputs out of the Hamming
// distance.  Compare, look, trace and fix read decision words and are cvd_decode.hip's
// (cvd::viterbi_launch); the join kernel reruns blocks with this file's forward recursion.
// The step loop and the two kernels' bodies are cvd_decode_common.h's (acs_chunk, forward_body,
// join_body), the pattern's checks and packing cvd_decode.hip's (cvd::viterbi_pack_pattern).
//
// What PLane (cvd_decode_lanes.h) brings where Lane has its funnel and 2-bit metric fields:
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
#include "cvd_decode_lanes.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr const char* kWho = "viterbi_decode_punctured";

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
