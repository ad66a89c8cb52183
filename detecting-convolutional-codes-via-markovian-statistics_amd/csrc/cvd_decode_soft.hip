// cvd_viterbi_decode_soft and cvd_soft_depuncture (include/cvd.h) for gfx950: the capture
// decoder of cvd_decode.hip over one int8 confidence value per channel bit.  Only the forward
// pass and the join know what a step's metric is made of; compare, look, trace and fix read
// decision words and are cvd_decode.hip's (cvd::viterbi_launch with wide = true: the metric
// vectors are 16-bit here, D <= 127 n m).  An erased bit is the value 0, so a punctured soft
// capture is depunctured by a streaming kernel and decoded like any other.  The step loop and the
// two kernels' bodies are cvd_decode_common.h's (acs_chunk, forward_body, join_body): SLane
// overrides the four vector members and norm_of, and its run returns sum_t A_t.
//
// What SLane (cvd_decode_lanes.h) brings where Lane has its funnel and 2-bit metric fields:
//   metric    cost(out, t) = sum_j a(v_j) [v_j != 0 and (v_j > 0) != bit j of out], a(v) =
//             min(|v|, 127).  With corr = sum_j (+-1 by bit j of out) v_j and A_t = sum_j a(v_j),
//             2 cost = A_t - corr, and A_t is the same for every state: the loop carries
//             x = 2 D - sum_t A_t, the decisions come from x alone (differences of x are twice
//             those of D), and one v_dot4c_i32_i8 per branch adds -corr onto the predecessor's
//             x in place.  At the block edges x - min x is even and halves exactly; the
//             block's normalisation is (min x + sum_t A_t) / 2.  |x| <= 127 n (L + W) < 2^30.
//   staging   a segment of kSeg steps copies the 16-byte pieces that hold its n kSeg bytes to
//             LDS; per 64-step chunk lane j packs step j's n values (-128 clamped to -127)
//             into a dword and adds their magnitudes to its own partial sum of A (one wave
//             reduction per run, none per step).
//   per step  scalar: v_readlane of the chunk's packed dword; vector, per branch, the dot
//             product with a byte pattern of -+1 (zero above n) accumulating onto x(ps).
// After fix, one streaming kernel re-encodes d_bits from s_0 and counts the sign disagreements
// (stats[9]) and the non-erased values (stats[10]).
// wave64, one wave per block, lane = next state, ds_bpermute for 2^m <= 64 and the
// double-buffered LDS vector above, as in cvd_decode.hip.  No scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cvd.h"
#include "cvd_decode_common.h"
#include "cvd_decode_lanes.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr const char* kWho = "viterbi_decode_soft";
constexpr const char* kWhoDep = "soft_depuncture";
constexpr int64_t kMaxSpan = 1 << 20;             // block + warm: 2 * 127 * 3 * 2^20 < 2^30

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_soft_forward_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  SLane<m, n> ln;
  ln.init(a);
  forward_body(a, ln, st, met);
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_soft_join_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint4 st[kSoftStageU4];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  SLane<m, n> ln;
  ln.init(a);
  join_body(a, ln, st, met);
}

// stats[9], stats[10] (zeroed before the launch): a thread per step re-encodes the step from
// the decoded bits -- s_t is the m bits before bit t, those before bit 0 are s_0 = stats[4] --
// and compares the signs.  At most kCountBlocks blocks, one pair of atomics each (with a pair
// per wave of a grid of 65,536 blocks, half a million adds onto two addresses, the call over
// 2^27 steps took 11.4 ms instead of 5.3: DESIGN.md §7.13).
constexpr int kCountBlocks = 2048;

__global__ __launch_bounds__(256) void viterbi_soft_count_kernel(VArgs a, int m, int n) {
  __shared__ uint32_t part[2][256 / kWave];
  const int8_t* v = reinterpret_cast<const int8_t*>(a.cap) + a.start;
  const uint32_t before = __builtin_bitreverse32((uint32_t)a.stats[4]);   // u_{-d} in bit 32 - d
  uint32_t err = 0u, seen = 0u;                          // a block sees at most 3 * 2^31 / kCountBlocks values
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (int64_t)gridDim.x * 256) {
    const int64_t w = t >> 5;
    const uint32_t hi = a.bits[w], lo = w ? a.bits[w - 1] : before;
    const uint64_t q = ((uint64_t)hi << 32) | lo;
    const uint32_t sh = (uint32_t)(t & 31);
    const uint32_t r = (uint32_t)(q >> (sh + 32u - (uint32_t)m)) & ((1u << m) - 1u);   // bit i: u_{t-m+i}
    const uint32_t ps = __builtin_bitreverse32(r) >> (32 - m);                       // bit d-1: u_{t-d}
    const uint32_t u = (hi >> sh) & 1u;
    for (int j = 0; j < n; ++j) {
      const uint32_t o = (((a.g0 >> j) & u) ^ (uint32_t)__builtin_popcount(a.gs[j] & ps)) & 1u;
      const int x = v[(int64_t)n * t + j];
      seen += x != 0;
      err += x != 0 && (uint32_t)(x > 0) != o;
    }
  }
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    err += __shfl_xor(err, k);
    seen += __shfl_xor(seen, k);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[0][threadIdx.x / kWave] = err;
    part[1][threadIdx.x / kWave] = seen;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* s = reinterpret_cast<unsigned long long*>(a.stats);
    err = seen = 0u;
#pragma unroll
    for (int i = 0; i < 256 / kWave; ++i) {
      err += part[0][i];
      seen += part[1][i];
    }
    if (err) atomicAdd(&s[9], (unsigned long long)err);
    if (seen) atomicAdd(&s[10], (unsigned long long)seen);
  }
}

struct DArgs {
  const int8_t* in;
  uint32_t* out;
  int64_t start, total, ndw;   // n T values, in ndw dwords with the padding
  int32_t period, K, n;
  uint64_t pmask, ppre[2];     // as in VArgs
};

// a thread per output dword: four values, each its kept input value or zero
__global__ __launch_bounds__(256) void soft_depuncture_kernel(DArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.ndw) return;
  uint32_t word = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t idx = 4 * i + k;
    if (idx >= a.total) break;
    const uint32_t t = a.n == 2 ? (uint32_t)(idx >> 1) : (uint32_t)(idx / 3);
    const uint32_t j = (uint32_t)(idx - (int64_t)a.n * t);
    const uint32_t r = t / (uint32_t)a.period, c = t - r * (uint32_t)a.period;
    const uint32_t keep = (uint32_t)(a.pmask >> (4u * c)) & 7u;
    if ((keep >> j) & 1u) {
      const uint32_t pre = (uint32_t)(a.ppre[c >> 3] >> (8u * (c & 7u))) & 255u;
      const int64_t p = a.start + (int64_t)r * a.K + pre + __builtin_popcount(keep & ((1u << j) - 1u));
      word |= (uint32_t)(uint8_t)a.in[p] << (8 * k);
    }
  }
  a.out[i] = word;
}

CVD_VITERBI_PICK(viterbi_soft_forward_kernel, viterbi_soft_join_kernel)

}  // namespace

extern "C" int64_t cvd_viterbi_soft_workspace_bytes(int32_t n, int32_t m, int64_t T, int32_t block) {
  return cvd::viterbi_workspace_bytes(kWho, n, m, T, block, true);
}

extern "C" int cvd_viterbi_decode_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals, int64_t start,
                                       int64_t T, int32_t block, int32_t warm, int32_t depth, uint32_t* d_bits,
                                       int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(kWho, code)) return rc;
  const int n = code->n, m = code->m;
  int64_t span;
  if (T >= 0 && __builtin_mul_overflow(T, (int64_t)n, &span)) span = -1;
  if (T < 0) span = 0;                                   // reported as a bad T
  // the doubled metric of a block runs over block + warm steps without normalisation (a bad
  // block or warm is viterbi_setup's to report)
  if (block >= 0 && warm >= -1 &&
      (int64_t)(block ? block : CVD_VITERBI_BLOCK) + (warm < 0 ? CVD_VITERBI_WARM(m) : warm) > kMaxSpan)
    return invalid(kWho, "block + warm must be at most 2^20");
  VArgs a;
  bool launch;
  // one value per byte: the capture checks are those of a CVD_CAPTURE_BYTES capture of nvals bytes
  const int rc = cvd::viterbi_setup(kWho, code, d_soft, nvals, CVD_CAPTURE_BYTES, start, T, span, block, warm, depth,
                                    CVD_VITERBI_WARM(m), CVD_VITERBI_DEPTH(m), d_bits, d_stats, d_work, &a, &launch, true);
  if (rc != CVD_OK || !launch) return rc;
  Kern fwd, join;
  pick(m, n, &fwd, &join);
  const int lrc = cvd::viterbi_launch(m, a, fwd, join, stream, true);
  if (lrc != CVD_OK) return lrc;
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats + 9, 0, 16, st));
  const int64_t blocks = (T + 255) / 256;
  hipLaunchKernelGGL(viterbi_soft_count_kernel, dim3((unsigned)(blocks < kCountBlocks ? blocks : kCountBlocks)), dim3(256), 0, st, a,
                     m, n);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

extern "C" int cvd_soft_depuncture(const int8_t* d_in, int64_t nvals, int64_t start, const uint8_t* keep,
                                   int32_t period, int32_t n, int64_t T, int8_t* d_out, void* stream) {
  if (n < 2 || n > 3) return invalid(kWhoDep, "needs n in 2..3");
  cvd::VPattern pat;
  if (const int rc = cvd::viterbi_pack_pattern(kWhoDep, "value", keep, period, n, &pat)) return rc;
  if (T < 0 || T > INT32_MAX) return invalid(kWhoDep, "T must be 0..2^31 - 1");
  if (start < 0 || nvals < 0) return invalid(kWhoDep, "needs start, nvals >= 0");
  int64_t span = 0, end;
  if (!pat.span(T, &span) || __builtin_add_overflow(span, start, &end))
    return invalid(kWhoDep, "the position of the last value's end overflows int64");
  if (end > nvals) return invalid(kWhoDep, "the values do not lie inside [0, nvals)");
  if (T == 0) return CVD_OK;
  if (!d_in || !d_out || ((uintptr_t)d_out & 15)) return invalid(kWhoDep, "d_in and d_out (16-byte aligned) must be non-null");
  DArgs a{};
  a.K = pat.K;
  a.pmask = pat.pmask;
  a.ppre[0] = pat.ppre[0];
  a.ppre[1] = pat.ppre[1];
  a.total = (int64_t)n * T;
  const int64_t nout = round16(a.total);
  const uintptr_t i0 = (uintptr_t)d_in, o0 = (uintptr_t)d_out;
  if (i0 < o0 + (uintptr_t)nout && o0 < i0 + (uintptr_t)nvals) return invalid(kWhoDep, "d_out overlaps d_in");
  a.in = d_in;
  a.out = reinterpret_cast<uint32_t*>(d_out);
  a.start = start;
  a.ndw = nout / 4;
  a.period = period;
  a.n = n;
  hipLaunchKernelGGL(soft_depuncture_kernel, dim3((unsigned)((a.ndw + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}
