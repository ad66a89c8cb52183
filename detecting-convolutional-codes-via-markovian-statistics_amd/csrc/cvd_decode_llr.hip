// cvd_viterbi_decode_frames_llr (include/cvd.h) for gfx950: soft-in / soft-out decoding of a
// batch of F frames of T steps each, the max-log-MAP value L_t = M_0(t) - M_1(t) of every step.
// One wavefront per frame, lane = state (S > 64: SPL states per lane), grid-striding over the
// frames so that the lane's branch tables are built once per wave.  The forward metric alpha and
// the backward metric beta of a state meet in the same lane, so alpha + beta is a lane-local add.
//
// Keeping alpha for every step would be S * 4 bytes per step and frame; the kernel keeps a
// checkpoint every kLlrSeg = 32 steps instead and recomputes (a segment is one word of bits):
//   forward    the soft lane's step (SLane: sdot4 candidates; acs_chunk without decisions) up to
//              the start of the last segment, the vector at the start of every segment but the
//              first and the last stored into the wave's own slice of the workspace (per wave,
//              not per frame; T <= 64: none).
//   segments   from the last to the first: alpha is recomputed from the checkpoint (D_0 for the
//              first; the last segment continues the forward pass instead and leaves alpha_T,
//              from which s_T and the distance are read as the frames call reads them), every
//              step's vector kept in LDS (rows[jj] = alpha_{t0+jj+1}; for S > 64
//              the row of the step before is also the exchange buffer of the step, so the
//              recomputation costs what the forward pass costs).  Then beta runs backwards
//              through the segment with a second pair of patterns, those of out(s, 0) and
//              out(s, 1) of the lane's own states.  At every step the lane forms alpha + beta,
//              minimises over its SPL states (all of the lane's parity) and writes the value
//              over the dead row.  After the segment, lane (jj, u) = (lane & 31, lane >> 5)
//              minimises row jj over the 32 entries of parity u -- one ds_read per step and
//              lane, rotated by jj so that the 64 lanes hit 64 banks -- in the place of five
//              cross-lane exchanges per step; lanes 0..31 then hold M_0, fetch M_1 from lane
//              + 32, form L_t and store 32 int16 and one word of bits contiguously.
//   totals     wave-uniform sums, one atomic per total per wave (= block) at the end.
// Why LDS and not a register array for the segment's alpha: the array would be indexed by the
// step, so it stays in registers only if both step loops are unrolled 32-fold for every one of
// the sixteen (m, n) instances with ragged last segments peeled, and at S = 256 it is 128 VGPRs
// on top of the loop's; rows in LDS are 8 KiB (S <= 64), 16 KiB (S = 128), 32 KiB (S = 256) per
// wave, compile without scratch and leave 20 / 9 / 4 waves per CU.
// Metrics are the soft lane's x = 2 D - sum A: in M_0 - M_1 the sums cancel and the difference
// is even; only the distance needs sum A.  kInf = 2^28 stands for +inf on either side; finite
// |x| < 2^25, so a sum at or above 2^27 has an infinite term.  wave64, no scratch.  The kernel's
// body (around a loader of a step's values) and the host path are in cvd_decode_llr_body.h, which
// cvd_decode_psoft.hip shares.
#include <hip/hip_runtime.h>

#include "cvd_decode_llr_body.h"

namespace {

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_frames_llr_kernel(LArgs la) {
  using Sh = Shape<m>;
  __shared__ int rows[kLlrSeg * (Sh::S > kWave ? Sh::S : kWave)];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  llr_body<m, n>(la, rows, met, LoadAll<n>());
}

#define CVD_L_ROW(n)                                                                                              \
  {viterbi_frames_llr_kernel<1, n>, viterbi_frames_llr_kernel<2, n>, viterbi_frames_llr_kernel<3, n>,             \
   viterbi_frames_llr_kernel<4, n>, viterbi_frames_llr_kernel<5, n>, viterbi_frames_llr_kernel<6, n>,             \
   viterbi_frames_llr_kernel<7, n>, viterbi_frames_llr_kernel<8, n>}

constexpr const char* kWho = "viterbi_decode_frames_llr";

}  // namespace

extern "C" int64_t cvd_viterbi_llr_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F) {
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(kWho, "needs n in 2..3 and m in 1..8");
  if (F < 0) return invalid(kWho, "needs F >= 0");
  if (F == 0) return 0;
  if (T < 1 || T > CVD_VITERBI_FRAME_MAX_T) return invalid(kWho, "T must be 1..65536");
  return waves_of(m, T, F) * slice_bytes(m, T);
}

extern "C" int cvd_viterbi_decode_frames_llr(const cvd_code* code, const int8_t* d_soft, int64_t nvals, int64_t start,
                                             int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                             int32_t start_state, int32_t end_state, int16_t* d_llr, uint32_t* d_bits,
                                             int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(kWho, code)) return rc;
  static const LKern kern[2][8] = {CVD_L_ROW(2), CVD_L_ROW(3)};
  return decode_llr(kWho, kern[code->n - 2][code->m - 1], code, nullptr, d_soft, nvals, start, stride, d_offsets, F, T,
                    start_state, end_state, d_llr, d_bits, d_frames, d_stats, d_work, stream);
}
