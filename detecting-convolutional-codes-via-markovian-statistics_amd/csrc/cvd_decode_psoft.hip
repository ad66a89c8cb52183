// cvd_viterbi_decode_frames_soft_punctured, _tailbiting_soft_punctured and _llr_punctured
// (include/cvd.h) for gfx950: the three frame decoders on frames of int8 values behind a
// puncturing pattern.  The contract is one rule -- the result is the unpunctured soft call's on
// the frames v'_f that hold a kept value at its output's place and 0 elsewhere -- and the
// kernels follow it literally: everything but the reading of a step's values is the unpunctured
// soft decoders' (frame_body, tailbite_body and llr_body of the three *_body.h headers, the
// host paths behind them, the trace kernel), and a step's values reach the step loop as SLane's
// packed word with a zero byte where the column erases, which is what v'_f holds there.
//
//   forward   frame_body around PSLane (cvd_decode_lanes.h): per segment of 1024 steps the
//             16-byte pieces that cover [pos(seg), pos(seg + cnt)) go to LDS; per chunk of 64
//             steps lane l finds its step's period and column (one division per segment, then
//             increments), reads its kept values from LDS and packs them.  The step loop is
//             SLane's, instruction for instruction.
//   count     records [4], [5]: count_body<true>, the re-encoding of the soft count kernel with
//             the values read at the kept positions.
//   tailbite  tailbite_body around PSLane; its in-kernel sign count reads the kept positions.
//   llr       llr_body with LoadKept: a lane finds pos(t) of its own step with one division per
//             32-step segment.
// The pattern's fields are indexed by the column, so every kernel keeps a copy of the arguments
// in LDS (as the punctured hard kernels do; a local copy would live in scratch).  A frame reads
// nothing outside [o_f, o_f + span): a kept value of step t < T lies below pos(T), and the
// staging reads whole pieces only below nu4.  wave64, no scratch.
#include <hip/hip_runtime.h>

#include "cvd_decode_frames_body.h"
#include "cvd_decode_llr_body.h"
#include "cvd_decode_tailbite_body.h"

namespace {

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_psoft_frames_forward_kernel(FArgs fa) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ VArgs sa;
  PSLane<m, n> ln;
  ln.init(fa.v);
  if (ln.lane == 0) sa = fa.v;
  frame_body<true>(fa, ln, st, met, &sa);
}

__global__ __launch_bounds__(kWave) void viterbi_psoft_frames_count_kernel(FArgs fa, int m, int n) {
  __shared__ VArgs sa;
  if (threadIdx.x == 0) sa = fa.v;
  __syncthreads();
  count_body<true>(fa, sa, m, n);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_psoft_tailbite_kernel(TArgs ta) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ int sel[Sh::S];
  __shared__ VArgs sa;
  PSLane<m, n> ln;
  ln.init(ta.v);
  if (ln.lane == 0) sa = ta.v;
  CVD_TAILBITE_BODY(true, true, &sa);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_psoft_llr_kernel(LArgs la) {
  using Sh = Shape<m>;
  __shared__ int rows[kLlrSeg * (Sh::S > kWave ? Sh::S : kWave)];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ VArgs sa;
  if (threadIdx.x == 0) sa = la.v;
  __syncthreads();
  llr_body<m, n>(la, rows, met, LoadKept{&sa});
}

constexpr const char* kWhoFrames = "viterbi_decode_frames_soft_punctured";
constexpr const char* kWhoTail = "viterbi_decode_frames_tailbiting_soft_punctured";
constexpr const char* kWhoLlr = "viterbi_decode_frames_llr_punctured";

// the code shape and the pattern, as cvd_viterbi_decode_punctured checks them
int shape_and_pattern(const char* who, const cvd_code* code, const uint8_t* keep, int32_t period, cvd::VPattern* pat) {
  if (const int rc = cvd::viterbi_code_shape(who, code)) return rc;
  return cvd::viterbi_pack_pattern(who, "value", keep, period, code->n, pat);
}

}  // namespace

extern "C" int cvd_viterbi_decode_frames_soft_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                        const int8_t* d_soft, int64_t nvals, int64_t start,
                                                        int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                                        int32_t start_state, int32_t end_state, uint32_t* d_bits,
                                                        int32_t* d_frames, int64_t* d_stats, void* d_work,
                                                        void* stream) {
  cvd::VPattern pat;
  if (const int rc = shape_and_pattern(kWhoFrames, code, keep, period, &pat)) return rc;
  static const FKern fwd[2][8] = CVD_F_TABLE(viterbi_psoft_frames_forward_kernel);
  return decode_frames(kWhoFrames, fwd[code->n - 2][code->m - 1], viterbi_psoft_frames_count_kernel, code, &pat, d_soft,
                       nvals, CVD_CAPTURE_BYTES, start, stride, d_offsets, F, T, start_state, end_state, d_bits,
                       d_frames, d_stats, d_work, stream);
}

extern "C" int cvd_viterbi_decode_frames_tailbiting_soft_punctured(const cvd_code* code, const uint8_t* keep,
                                                                   int32_t period, const int8_t* d_soft, int64_t nvals,
                                                                   int64_t start, int64_t stride,
                                                                   const int64_t* d_offsets, int64_t F, int32_t T,
                                                                   int32_t max_laps, uint32_t* d_bits, int32_t* d_frames,
                                                                   int64_t* d_stats, void* d_work, void* stream) {
  cvd::VPattern pat;
  if (const int rc = shape_and_pattern(kWhoTail, code, keep, period, &pat)) return rc;
  static const TKern kern[2][8] = CVD_T_TABLE(viterbi_psoft_tailbite_kernel);
  return decode_tailbiting(kWhoTail, kern[code->n - 2][code->m - 1], code, &pat, d_soft, nvals, CVD_CAPTURE_BYTES, start,
                           stride, d_offsets, F, T, max_laps, d_bits, d_frames, d_stats, d_work, stream);
}

extern "C" int cvd_viterbi_decode_frames_llr_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                       const int8_t* d_soft, int64_t nvals, int64_t start,
                                                       int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                                       int32_t start_state, int32_t end_state, int16_t* d_llr,
                                                       uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats,
                                                       void* d_work, void* stream) {
  cvd::VPattern pat;
  if (const int rc = shape_and_pattern(kWhoLlr, code, keep, period, &pat)) return rc;
  static const LKern kern[2][8] = CVD_F_TABLE(viterbi_psoft_llr_kernel);
  return decode_llr(kWhoLlr, kern[code->n - 2][code->m - 1], code, &pat, d_soft, nvals, start, stride, d_offsets, F, T,
                    start_state, end_state, d_llr, d_bits, d_frames, d_stats, d_work, stream);
}
