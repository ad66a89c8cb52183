// cvd_viterbi_decode_frames_tailbiting, _punctured and _soft (include/cvd.h) for gfx950: a batch
// of F tail-biting frames of T steps each in one call, by the wrap-around Viterbi algorithm.  A
// tail-biting frame starts in the state its own last m bits leave the encoder in, so neither
// boundary state is known; the decoder runs the frame lap after lap, each lap starting from the
// normalised end vector of the lap before, until the best end state's survivor closes on itself.
// Whether a lap was the last is known only after its traceback, so the forward / trace split of
// cvd_decode_frames.hip does not apply: one fused kernel per flavour and (m, n), one wavefront
// per frame, grid-striding over the frames.
//
//   lap       the lane type's run<true> (Lane, PLane, SLane of cvd_decode_lanes.h, as the frame
//             decoder's forward kernels use them) over steps [0, T) from the lap's vector, the
//             decision words going to the wave's own piece of memory: dynamic LDS while a
//             frame's words fit kLdsBytes, else the wave's slice of d_work (per wave, not per
//             frame: a wave reuses it).  run takes a plain pointer, so one body serves both; it
//             is instantiated once per placement inside each kernel (CVD_TAILBITE_BODY).
//   trace     all 2^m end states in lockstep: lane = end state (SPL chains per lane for m = 7,
//             8); step t's decision words are read at a wave-uniform address (an LDS broadcast
//             or one line) and every lane shifts its own chains.  The reads do not depend on the
//             chains, so this costs one chain's time and gives a(e) for every e.
//   select    min and ballots over D_T, D_0(a(e)) through an LDS copy of the start vector.
//   row       the chosen chain once more, lane 0 writing the row of bits.
//   count     soft only: the wave re-encodes the row from s_0, a lane per step, and counts the
//             sign disagreements and the non-erased values (viterbi_frames_soft_count_kernel's
//             loop; that kernel skips every frame of nonzero status, and 2 and 3 are decoded).
//   totals    wave-uniform sums over the wave's frames, one atomic per total per wave.
// Metrics: int32 without a +inf, no state is ever excluded.  Hard: D <= spread + n T with the
// spread of a normalised vector <= n m (T >= m) or <= laps n T; soft: the lane carries
// x = 2 D - sum A from x_0 = 2 D_0 (even), |x| < 2^26.  wave64, no scratch.  The body and the
// host path are in cvd_decode_tailbite_body.h, which cvd_decode_psoft.hip shares.
#include <hip/hip_runtime.h>

#include "cvd_decode_tailbite_body.h"

namespace {

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_tailbite_kernel(TArgs ta) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ int sel[Sh::S];
  Lane<m, n> ln;
  ln.init(ta.v);
  CVD_TAILBITE_BODY(false, false);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_tailbite_punct_kernel(TArgs ta) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kPunctStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ int sel[Sh::S];
  __shared__ VArgs sa;
  PLane<m, n> ln;
  ln.init(ta.v);
  if (ln.lane == 0) sa = ta.v;
  CVD_TAILBITE_BODY(false, true, &sa);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_tailbite_soft_kernel(TArgs ta) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ int sel[Sh::S];
  SLane<m, n> ln;
  ln.init(ta.v);
  CVD_TAILBITE_BODY(true, false);
}

enum Flavour { kHard = 0, kPunct = 1, kSoft = 2 };

TKern kernel_of(Flavour fl, int m, int n) {
  static const TKern f[3][2][8] = {CVD_T_TABLE(viterbi_tailbite_kernel), CVD_T_TABLE(viterbi_tailbite_punct_kernel),
                                   CVD_T_TABLE(viterbi_tailbite_soft_kernel)};
  return f[fl][n - 2][m - 1];
}

const char* who_of(Flavour fl) {
  return fl == kHard    ? "viterbi_decode_frames_tailbiting"
         : fl == kPunct ? "viterbi_decode_frames_tailbiting_punctured"
                        : "viterbi_decode_frames_tailbiting_soft";
}

}  // namespace

extern "C" int64_t cvd_viterbi_tailbiting_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t soft) {
  constexpr const char* who = "viterbi_decode_frames_tailbiting";
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(who, "needs n in 2..3 and m in 1..8");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (soft != 0 && soft != 1) return invalid(who, "soft must be 0 or 1");
  if (F == 0) return 0;
  if (T < 1 || T > CVD_VITERBI_FRAME_MAX_T) return invalid(who, "T must be 1..65536");
  return tail_work_bytes(m, T, F);
}

extern "C" int cvd_viterbi_decode_frames_tailbiting(const cvd_code* code, const void* d_capture, int64_t nbits,
                                                    int32_t format, int64_t start, int64_t stride,
                                                    const int64_t* d_offsets, int64_t F, int32_t T, int32_t max_laps,
                                                    uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                                    void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kHard), code)) return rc;
  return decode_tailbiting(who_of(kHard), kernel_of(kHard, code->m, code->n), code, nullptr, d_capture, nbits, format,
                           start, stride, d_offsets, F, T, max_laps, d_bits, d_frames, d_stats, d_work, stream);
}

extern "C" int cvd_viterbi_decode_frames_tailbiting_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                              const void* d_capture, int64_t nbits, int32_t format,
                                                              int64_t start, int64_t stride, const int64_t* d_offsets,
                                                              int64_t F, int32_t T, int32_t max_laps, uint32_t* d_bits,
                                                              int32_t* d_frames, int64_t* d_stats, void* d_work,
                                                              void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kPunct), code)) return rc;
  cvd::VPattern pat;
  if (const int rc = cvd::viterbi_pack_pattern(who_of(kPunct), "bit", keep, period, code->n, &pat)) return rc;
  return decode_tailbiting(who_of(kPunct), kernel_of(kPunct, code->m, code->n), code, &pat, d_capture, nbits, format,
                           start, stride, d_offsets, F, T, max_laps, d_bits, d_frames, d_stats, d_work, stream);
}

extern "C" int cvd_viterbi_decode_frames_tailbiting_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                                         int64_t start, int64_t stride, const int64_t* d_offsets,
                                                         int64_t F, int32_t T, int32_t max_laps, uint32_t* d_bits,
                                                         int32_t* d_frames, int64_t* d_stats, void* d_work,
                                                         void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kSoft), code)) return rc;
  // one value per byte: the capture checks are those of a CVD_CAPTURE_BYTES capture of nvals bytes
  return decode_tailbiting(who_of(kSoft), kernel_of(kSoft, code->m, code->n), code, nullptr, d_soft, nvals,
                           CVD_CAPTURE_BYTES, start, stride, d_offsets, F, T, max_laps, d_bits, d_frames, d_stats, d_work,
                           stream);
}
