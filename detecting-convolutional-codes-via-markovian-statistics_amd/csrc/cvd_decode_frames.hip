// cvd_viterbi_decode_frames, _punctured and _soft (include/cvd.h) for gfx950: a batch of F
// terminated frames of T steps each in one call.  A frame is tens to a few thousand steps from a
// known state to a known state, so none of the stream decoder's speculation (warm-up, compare,
// join, look, fix: cvd_decode.hip) applies: a frame is one wave's forward pass from a known
// vector and one traceback from a known state.  What this file adds is the batch.
//
//   forward   one wavefront per frame, lane = next state, grid-striding over the frames so that
//             the lane type's init (the branch tables of the code) is paid once per wave.  The
//             wave copies the arguments with start = o_f, sets D_0 (0 at start_state and kInf
//             elsewhere, or 0 everywhere), runs the lane type's run<true> over steps [0, T)
//             with the decision words going to the frame's piece of the workspace, and picks
//             s_T: end_state, or the lowest-index state of minimal D_T.  The three kernels are
//             frame_body around Lane, PLane and SLane (cvd_decode_lanes.h), whose step loops
//             are the stream decoders'.  Metrics are not normalised: D <= 3 * 65536 for hard
//             bits; the soft lane carries x = 2 D - sum A, |x| <= 127 * 3 * 65536 < 2^25, and
//             kInf = 2^28 is even, above every finite metric with room for T steps on top.
//   trace     lane = frame: 64 independent chains per wave, each lane reading its own decision
//             words a 128-byte line at a time with the next line in flight, as
//             viterbi_trace_kernel does for blocks (one chain per wave cost
//             2.9 ms of 8.0 where this cost 0.45).  It writes the frame's row of bits and s_0,
//             zeroes the row of a skipped frame, and adds up the totals: every lane keeps its
//             own sums, a block of four waves reduces them and issues one atomic per total (at
//             most kTraceBlocks blocks: DESIGN.md §7.13 on what atomics per wave cost).
//   count     soft only: a wave per frame re-encodes the row of bits from s_0 and counts the
//             sign disagreements and the non-erased values, as viterbi_soft_count_kernel does
//             for a stream; one pair of atomics per wave.
// The workspace holds the decision words of at most a batch of frames (about 1 GiB, or
// CVD_FRAMES_BATCH_BYTES); the host runs the kernels batch after batch on the stream.  All
// totals are integer sums, so the result does not depend on the grid or the batch.  wave64, no
// scratch.  frame_body, the trace kernel, the count kernel's body and the host path are in
// cvd_decode_frames_body.h, which cvd_decode_psoft.hip (punctured soft frames) shares.
#include <hip/hip_runtime.h>

#include "cvd_decode_frames_body.h"

namespace {

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_frames_forward_kernel(FArgs fa) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  Lane<m, n> ln;
  ln.init(fa.v);
  frame_body<false>(fa, ln, st, met);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_frames_punct_forward_kernel(FArgs fa) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kPunctStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  __shared__ VArgs sa;
  PLane<m, n> ln;
  ln.init(fa.v);
  if (ln.lane == 0) sa = fa.v;
  frame_body<true>(fa, ln, st, met, &sa);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_frames_soft_forward_kernel(FArgs fa) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  SLane<m, n> ln;
  ln.init(fa.v);
  frame_body<false>(fa, ln, st, met);
}

// Soft frames' records [4] and [5] and their totals (count_body).
__global__ __launch_bounds__(kWave) void viterbi_frames_soft_count_kernel(FArgs fa, int m, int n) {
  count_body<false>(fa, fa.v, m, n);
}

enum Flavour { kHard = 0, kPunct = 1, kSoft = 2 };

FKern forward_of(Flavour fl, int m, int n) {
  static const FKern f[3][2][8] = {CVD_F_TABLE(viterbi_frames_forward_kernel),
                                   CVD_F_TABLE(viterbi_frames_punct_forward_kernel),
                                   CVD_F_TABLE(viterbi_frames_soft_forward_kernel)};
  return f[fl][n - 2][m - 1];
}

const char* who_of(Flavour fl) {
  return fl == kHard ? "viterbi_decode_frames" : fl == kPunct ? "viterbi_decode_frames_punctured" : "viterbi_decode_frames_soft";
}

}  // namespace

extern "C" int64_t cvd_viterbi_frames_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t soft) {
  constexpr const char* who = "viterbi_decode_frames";
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(who, "needs n in 2..3 and m in 1..8");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (soft != 0 && soft != 1) return invalid(who, "soft must be 0 or 1");
  if (F == 0) return 0;
  if (T < 1 || T > CVD_VITERBI_FRAME_MAX_T) return invalid(who, "T must be 1..65536");
  return frames_work_bytes(m, T, F);
}

extern "C" int cvd_viterbi_decode_frames(const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                                         int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                         int32_t start_state, int32_t end_state, uint32_t* d_bits, int32_t* d_frames,
                                         int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kHard), code)) return rc;
  return decode_frames(who_of(kHard), forward_of(kHard, code->m, code->n), nullptr, code, nullptr, d_capture, nbits,
                       format, start, stride, d_offsets, F, T, start_state, end_state, d_bits, d_frames, d_stats, d_work,
                       stream);
}

extern "C" int cvd_viterbi_decode_frames_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                   const void* d_capture, int64_t nbits, int32_t format, int64_t start,
                                                   int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                                   int32_t start_state, int32_t end_state, uint32_t* d_bits,
                                                   int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kPunct), code)) return rc;
  cvd::VPattern pat;
  if (const int rc = cvd::viterbi_pack_pattern(who_of(kPunct), "bit", keep, period, code->n, &pat)) return rc;
  return decode_frames(who_of(kPunct), forward_of(kPunct, code->m, code->n), nullptr, code, &pat, d_capture, nbits,
                       format, start, stride, d_offsets, F, T, start_state, end_state, d_bits, d_frames, d_stats, d_work,
                       stream);
}

extern "C" int cvd_viterbi_decode_frames_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals, int64_t start,
                                              int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                              int32_t start_state, int32_t end_state, uint32_t* d_bits,
                                              int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(who_of(kSoft), code)) return rc;
  // one value per byte: the capture checks are those of a CVD_CAPTURE_BYTES capture of nvals bytes
  return decode_frames(who_of(kSoft), forward_of(kSoft, code->m, code->n), viterbi_frames_soft_count_kernel, code,
                       nullptr, d_soft, nvals, CVD_CAPTURE_BYTES, start, stride, d_offsets, F, T, start_state, end_state,
                       d_bits, d_frames, d_stats, d_work, stream);
}
