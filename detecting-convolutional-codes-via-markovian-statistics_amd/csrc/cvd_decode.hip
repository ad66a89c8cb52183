// Hard-decision Viterbi decoder of a captured bitstream (cvd_viterbi_decode, include/cvd.h)
// for gfx950: the Eq. 4-5 recursion of the detector with its survivor decisions kept, cut
// into blocks of L steps that run in parallel, and exact: the result is the sequential
// decoder's whatever the split.  Speculative work counts only where it is certified.
//
//   forward   one wavefront per block b.  It starts W steps early from D = 0, stores the
//             relative metric vector it reaches at step bL (the warm vector), then runs the
//             block's L steps recording per step the 2^m-bit decision word (__ballot of
//             "predecessor b = 1 strictly smaller") and stores the relative vector at the
//             block's end and the amount it was normalised by.  Lane = next state (2^m < 64:
//             the upper lanes repeat states and are masked out of the ballot; 2^m = 128, 256:
//             two / four states per lane).  The predecessor metrics come over ds_bpermute for
//             2^m <= 64 and through a double-buffered LDS vector above; metrics are plain
//             ints normalised at the two block edges only (the decisions do not depend on
//             the common offset; n (L + W) is far from overflow).  The received symbols are
//             staged 1,024 steps at a time into LDS as LSB-first dwords (cvd_capture_bits.h)
//             and shifted out of an SGPR pair; the branch metrics of a lane's two branches
//             for every y sit in 2-bit fields of two registers.  Lane j keeps the decision
//             word of a 64-step chunk's step j and every 64 steps the wave stores 64 of them
//             in one contiguous piece.
//   compare   a thread per block: does the warm vector of b equal the end vector of b - 1?
//   join      one wave walks the mismatch flags in ascending order; where the true vector
//             at bL (in registers after a rerun, else the stored end vector of b - 1) differs
//             from the warm vector of b it reruns block b from the true vector, rewriting its
//             decisions, end vector and normalisation, and goes on to b + 1 (a cascade ends
//             at the first block whose warm vector was right).
//   look      one wave per block.  D lookahead steps with lane = state, each lane following
//             its own survivor back from step e = min(T, (b+1)L + D); if all of them sit in
//             one state at (b+1)L the block is certified to trace from that state (e = T:
//             from the true end state, followed back to (b+1)L).  64 steps at a time: lane j
//             loads the decision word of step base + j (one contiguous piece), the chain
//             reads them with v_readlane.
//   trace     the certified blocks' L-step chains, lane = block: 64 independent chains per
//             wave, each lane reading its own decision words a 128-byte line at a time with
//             the next line in flight (one wave per block, every lane on the same chain,
//             measured 2.9 ms of the 8.0 ms of 2^27 steps; this way 0.5 ms).
//             A block owns whole output words (32 | L).
//   fix       one wave resolves the uncertified blocks in descending order from the start
//             state the block after them traced (the chain in SGPRs, on the scalar unit),
//             and writes d_stats.
// The channel-error count is the path metric of the traced path: the sum of the blocks'
// normalisations (D_0 = 0 and D_T(s_T) = 0, and along the decisions D'(s') = D(ps) + d_H
// holds exactly), integer adds in any order.  No scratch.
// The kernel arguments, the staging helper, the pattern-independent part of a lane, the step
// loop (acs_chunk) and the forward / join bodies are in cvd_decode_common.h: Lane (cvd_decode_lanes.h)
// brings the branch-metric fields, the staging and the SGPR funnel that y_t is shifted out of.
// cvd_decode_punct.hip brings a lane, a forward and a join kernel for punctured captures and
// runs everything else here; cvd_decode_soft.hip does the same for int8 confidence values, whose
// lane keeps 16-bit metric vectors (`wide`: their place in the workspace and the compare step's
// width).  The host code the three share is here too, declared in cvd_internal.h: the
// code-shape check, the packing of a puncturing pattern, the workspace layout, viterbi_setup
// and viterbi_launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/cvd.h"
#include "cvd_capture_bits.h"
#include "cvd_decode_common.h"
#include "cvd_decode_lanes.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;   // kWave, kSeg, kStageDw, Shape, VArgs, stage_bits, LaneBase (cvd_decode_common.h), Lane (cvd_decode_lanes.h)

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_forward_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  Lane<m, n> ln;
  ln.init(a);
  forward_body(a, ln, st, met);
}

__global__ void viterbi_compare_kernel(VArgs a, int S) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.nb) return;
  int diff = 0;
  if (b > 0) {
    const uint8_t* w = a.warm + b * S;
    const uint8_t* e = a.endv + (b - 1) * S;
    for (int s = 0; s < S; ++s) diff |= w[s] != e[s];
  }
  a.mis[b] = diff;
}

template <int m, int n>
__global__ __launch_bounds__(kWave) void viterbi_join_kernel(VArgs a) {
  using Sh = Shape<m>;
  __shared__ uint32_t st[kStageDw];
  __shared__ int met[Sh::SPL > 1 ? 2 * Sh::S : 1];
  Lane<m, n> ln;
  ln.init(a);
  join_body(a, ln, st, met);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

// survivor of state s at step hi followed back to step lo (s may differ from lane to lane);
// write (s wave-uniform, lo a multiple of 32): the input bits of steps [lo, hi) to d_bits
template <int m, bool write>
__device__ __forceinline__ int trace_range(const VArgs& a, int64_t lo, int64_t hi, int s, int lane) {
  constexpr int SPL = Shape<m>::SPL;
  // the block's own chain is wave-uniform: in SGPRs it runs on the scalar unit, whose
  // dependent shift / and / or chain per step is several times shorter than the vector one
  if constexpr (write) s = __builtin_amdgcn_readfirstlane(s);
  const int nch = (int)((hi - lo + 63) >> 6);
  uint64_t w[SPL], wn[SPL];                  // this chunk's words, and the next one's on their way
#pragma unroll
  for (int i = 0; i < SPL; ++i) {
    wn[i] = 0ull;
    if (nch > 0 && lo + 64 * (int64_t)(nch - 1) + lane < hi) wn[i] = a.dec[(lo + 64 * (int64_t)(nch - 1) + lane) * SPL + i];
  }
  for (int c = nch - 1; c >= 0; --c) {
    const int64_t base = lo + 64 * (int64_t)c;
    const int cnt = (int)min((int64_t)64, hi - base);
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      w[i] = wn[i];
      if (c > 0) wn[i] = a.dec[(base - 64 + lane) * SPL + i];   // a whole chunk: below the last one
    }
    uint64_t out = 0ull;
    for (int j = cnt - 1; j >= 0; --j) {
      uint64_t x = readlane64(w[0], j);
#pragma unroll
      for (int i = 1; i < SPL; ++i) {
        const uint64_t xi = readlane64(w[i], j);
        if ((s >> 6) == i) x = xi;
      }
      const int d = (int)((x >> (s & 63)) & 1ull);
      if constexpr (write) out |= (uint64_t)(s & 1) << j;
      s = (s >> 1) | (d << (m - 1));
    }
    if constexpr (write) {
      if (lane == 0) {
        a.bits[base >> 5] = (uint32_t)out;
        if (base + 32 < hi) a.bits[(base >> 5) + 1] = (uint32_t)(out >> 32);
      }
    }
  }
  return s;
}

// lowest-index state with D_T = 0
template <int m>
__device__ __forceinline__ int end_state(const VArgs& a, int lane) {
  constexpr int S = Shape<m>::S, SPL = Shape<m>::SPL;
  int sT = 0;
#pragma unroll
  for (int i = SPL - 1; i >= 0; --i) {
    const uint64_t bal = __ballot(lane < S && a.endv[(a.nb - 1) * S + (lane & (S - 1)) + kWave * i] == 0);
    if (bal) sT = kWave * i + __builtin_ctzll(bal);
  }
  return sT;
}

template <int m>
__global__ __launch_bounds__(kWave) void viterbi_look_kernel(VArgs a) {
  constexpr int S = Shape<m>::S, SPL = Shape<m>::SPL;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t lo = b * a.L, hi = min(a.T, lo + a.L), e = min(a.T, lo + a.L + a.D);
  int x;
  bool cert = true;
  if (e == a.T) {
    x = trace_range<m, false>(a, hi, a.T, end_state<m>(a, lane), lane);
  } else {
    x = 0;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int r = trace_range<m, false>(a, hi, e, (lane & (S - 1)) + kWave * i, lane);
      if (i == 0) x = __builtin_amdgcn_readfirstlane(r);
      cert = cert && __all(r == x);
    }
  }
  if (lane == 0) {
    a.xs[b] = x;
    a.unc[b] = cert ? 0 : 1;
    if (!cert) atomicAdd(&a.cnt[2], 1ull);
    atomicAdd(&a.cnt[0], (unsigned long long)a.norm[b]);
  }
}

// The certified blocks' own chains, lane = block: 64 independent chains per wave instead of
// one chain computed 64 times over.  A lane's decision words are contiguous; it reads them a
// 128-byte line (16 / SPL steps) at a time, the line below already on its way.  The steps of
// the last block at or past T are skipped (their words are allocated, never written).
template <int m>
__global__ __launch_bounds__(kWave) void viterbi_trace_kernel(VArgs a) {
  constexpr int SPL = Shape<m>::SPL, K = 16 / SPL;
  const int64_t b = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (b >= a.nb || a.unc[b] != 0) return;
  const int64_t lo = b * a.L;
  const int len = (int)(min(a.T, lo + a.L) - lo);
  const uint64_t* d = a.dec + lo * SPL;
  uint32_t* bits = a.bits + (lo >> 5);
  int s = a.xs[b];
  uint64_t w[16], wn[16];
  const int nsub = a.L / K;
#pragma unroll
  for (int i = 0; i < 16; ++i) wn[i] = d[(int64_t)(nsub - 1) * 16 + i];
  uint32_t out = 0u;
  for (int c = nsub - 1; c >= 0; --c) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      w[i] = wn[i];
      if (c > 0) wn[i] = d[(int64_t)(c - 1) * 16 + i];
    }
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
      const int t = c * K + k;
      uint64_t x = w[k * SPL];
#pragma unroll
      for (int i = 1; i < SPL; ++i)
        if ((s >> 6) == i) x = w[k * SPL + i];
      const int dd = (int)((x >> (s & 63)) & 1ull);
      if (t < len) {
        out |= (uint32_t)(s & 1) << (t & 31);
        s = (s >> 1) | (dd << (m - 1));
      }
    }
    if (((c * K) & 31) == 0) {                           // steps [cK, cK + 32) are done: one output word
      if (c * K < len) bits[(c * K) >> 5] = out;
      out = 0u;
    }
  }
  a.sst[b] = s;
}

template <int m>
__global__ __launch_bounds__(kWave) void viterbi_fix_kernel(VArgs a) {
  const int lane = threadIdx.x;
  int64_t carry_b = -1;
  int carry_s = 0;
  for (int64_t top = a.nb; top > 0; top -= kWave) {
    const int64_t idx = top - 1 - lane;                  // lane k: block top - 1 - k, so ctz is the highest block
    uint64_t bal = __ballot(idx >= 0 && a.unc[idx] != 0);
    while (bal) {
      const int64_t b = top - 1 - __builtin_ctzll(bal);
      bal &= bal - 1;
      // the last block is always certified, so b + 1 < nb; an uncertified b + 1 was fixed just now
      const int x = carry_b == b + 1 ? carry_s : a.sst[b + 1];
      const int s0 = trace_range<m, true>(a, b * a.L, min(a.T, (b + 1) * a.L), x, lane);
      if (lane == 0) a.sst[b] = s0;
      carry_b = b;
      carry_s = s0;
    }
  }
  const int sT = end_state<m>(a, lane);
  if (lane == 0) {
    a.stats[0] = (int64_t)a.cnt[0];
    a.stats[1] = a.nb;
    a.stats[2] = (int64_t)a.cnt[1];
    a.stats[3] = (int64_t)a.cnt[2];
    a.stats[4] = carry_b == 0 ? carry_s : a.sst[0];
    a.stats[5] = sT;
    a.stats[6] = a.L;
    a.stats[7] = a.W;
    a.stats[8] = a.D;
    if (a.period) a.stats[9] = a.span;                   // cvd_viterbi_decode_punctured's int64[10]
  }
}

constexpr const char* kWho = "viterbi_decode";

struct Layout {
  int64_t nb, dec, warm, endv, norm, sst, xs, mis, unc, cnt, warm16, end16, total;
};

// T in 1..2^31 - 1, L >= 32: nb L < 2^32, every size far below 2^63.  wide: the soft decoder's
// two arrays of 16-bit vectors behind everything else.
Layout layout_of(int m, int64_t T, int64_t L, bool wide) {
  const int64_t S = (int64_t)1 << m, spl = S > kWave ? S / kWave : 1;
  Layout y{};
  y.nb = (T + L - 1) / L;
  int64_t off = 0;
  y.dec = off;  off += round16(y.nb * L * spl * 8);
  y.warm = off; off += round16(y.nb * S);
  y.endv = off; off += round16(y.nb * S);
  y.norm = off; off += round16(y.nb * 4);
  y.sst = off;  off += round16(y.nb * 4);
  y.xs = off;   off += round16(y.nb * 4);
  y.mis = off;  off += round16(y.nb * 4);
  y.unc = off;  off += round16(y.nb * 4);
  y.cnt = off;  off += 64;
  if (wide) {
    y.warm16 = off; off += round16(y.nb * S * 2);
    y.end16 = off;  off += round16(y.nb * S * 2);
  }
  y.total = off;
  return y;
}

// 0 if block is acceptable (resolving 0 to the default), else the error
int resolve_block(const char* who, int32_t block, int32_t* L) {
  if (block == 0) block = CVD_VITERBI_BLOCK;
  if (block < 32 || block % 32) return invalid(who, "block must be 0 (default) or a multiple of 32, at least 32");
  *L = block;
  return CVD_OK;
}

CVD_VITERBI_PICK(viterbi_forward_kernel, viterbi_join_kernel)

}  // namespace

int cvd::viterbi_launch(int m, const VArgs& a, void (*fwd)(VArgs), void (*join)(VArgs), void* stream, bool wide) {
  static const Kern look[8] = {viterbi_look_kernel<1>, viterbi_look_kernel<2>, viterbi_look_kernel<3>,
                               viterbi_look_kernel<4>, viterbi_look_kernel<5>, viterbi_look_kernel<6>,
                               viterbi_look_kernel<7>, viterbi_look_kernel<8>};
  static const Kern trace[8] = {viterbi_trace_kernel<1>, viterbi_trace_kernel<2>, viterbi_trace_kernel<3>,
                                viterbi_trace_kernel<4>, viterbi_trace_kernel<5>, viterbi_trace_kernel<6>,
                                viterbi_trace_kernel<7>, viterbi_trace_kernel<8>};
  static const Kern fix[8] = {viterbi_fix_kernel<1>, viterbi_fix_kernel<2>, viterbi_fix_kernel<3>, viterbi_fix_kernel<4>,
                              viterbi_fix_kernel<5>, viterbi_fix_kernel<6>, viterbi_fix_kernel<7>, viterbi_fix_kernel<8>};
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(a.cnt, 0, 64, st));
  hipLaunchKernelGGL(fwd, dim3((unsigned)a.nb), dim3(kWave), 0, st, a);
  HIP_CHECK(hipGetLastError());
  if (a.nb > 1) {
    VArgs c = a;                                         // the compare step's view of the vectors
    if (wide) {
      c.warm = reinterpret_cast<uint8_t*>(a.warm16);
      c.endv = reinterpret_cast<uint8_t*>(a.end16);
    }
    hipLaunchKernelGGL(viterbi_compare_kernel, dim3((unsigned)((a.nb + 255) / 256)), dim3(256), 0, st, c,
                       (wide ? 2 : 1) << m);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(join, dim3(1), dim3(kWave), 0, st, a);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(look[m - 1], dim3((unsigned)a.nb), dim3(kWave), 0, st, a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(trace[m - 1], dim3((unsigned)((a.nb + kWave - 1) / kWave)), dim3(kWave), 0, st, a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fix[m - 1], dim3(1), dim3(kWave), 0, st, a);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

int cvd::viterbi_code_shape(const char* who, const cvd_code* code) {
  if (!code || !code->taps) return invalid(who, "null code");
  if (code->k != 1 || code->n < 2 || code->n > 3 || code->m < 1 || code->m > 8)
    return unsupported(who, "needs k = 1, n in 2..3 and m in 1..8");
  return CVD_OK;
}

int cvd::viterbi_pack_pattern(const char* who, const char* noun, const uint8_t* keep, int32_t period, int32_t n,
                              VPattern* out) {
  if (!keep) return invalid(who, "null keep");
  if (period < 1 || period > 16) return invalid(who, "period must be 1..16");
  VPattern p;
  p.period = period;
  for (int c = 0; c < period; ++c) {
    if (keep[c] == 0)
      return invalid(who, ("a column of keep is zero: every step transmits at least one " + std::string(noun)).c_str());
    if (keep[c] >> n) return invalid(who, "a column of keep has a bit at or above n");
    p.pre[c] = p.K;
    p.pmask |= (uint64_t)keep[c] << (4 * c);
    p.ppre[c >> 3] |= (uint64_t)p.K << (8 * (c & 7));
    p.K += __builtin_popcount(keep[c]);
  }
  p.pre[period] = p.K;
  *out = p;
  return CVD_OK;
}

int64_t cvd::viterbi_workspace_bytes(const char* who, int32_t n, int32_t m, int64_t T, int32_t block, bool wide) {
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(who, "needs n in 2..3 and m in 1..8");
  if (T < 0 || T > INT32_MAX) return invalid(who, "T must be 0..2^31 - 1");
  int32_t L;
  if (resolve_block(who, block, &L)) return CVD_E_INVALID;
  return layout_of(m, std::max<int64_t>(T, 1), L, wide).total;
}

int cvd::viterbi_setup(const char* who, const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                       int64_t start, int64_t T, int64_t span, int32_t block, int32_t warm, int32_t depth,
                       int32_t warm_default, int32_t depth_default, uint32_t* d_bits, int64_t* d_stats, void* d_work,
                       VArgs* out, bool* launch, bool wide) {
  *launch = false;
  const int n = code->n, m = code->m;
  if (format != CVD_CAPTURE_LSB && format != CVD_CAPTURE_MSB && format != CVD_CAPTURE_BYTES)
    return invalid(who, "unknown capture format");
  if (T < 0 || T > INT32_MAX) return invalid(who, "T must be 0..2^31 - 1");
  if (start < 0 || nbits < 0) return invalid(who, "needs start, nbits >= 0");
  int64_t end;
  if (span < 0 || __builtin_add_overflow(span, start, &end))
    return invalid(who, "the position of the last symbol's end overflows int64");
  if (end > nbits) return invalid(who, "the symbols do not lie inside [0, nbits)");
  int32_t L;
  if (resolve_block(who, block, &L)) return CVD_E_INVALID;
  if (warm < -1) return invalid(who, "warm must be >= 0, or -1 (default)");
  if (depth < -1) return invalid(who, "depth must be >= 0, or -1 (default)");
  const int32_t W = warm < 0 ? warm_default : warm, D = depth < 0 ? depth_default : depth;
  if (T == 0) return CVD_OK;
  if (!d_capture || !d_bits || !d_stats || !d_work || ((uintptr_t)d_capture & 15) || ((uintptr_t)d_work & 15) ||
      ((uintptr_t)d_bits & 3) || ((uintptr_t)d_stats & 7))
    return invalid(who, "d_capture, d_work (16-byte aligned), d_bits (4-byte) and d_stats (8-byte) must be non-null");

  const Layout y = layout_of(m, T, L, wide);
  VArgs a{};
  a.cap = static_cast<const uint4*>(d_capture);
  const int64_t nbytes = format == CVD_CAPTURE_BYTES ? nbits : nbits / 8 + (nbits % 8 != 0);
  a.nu4 = nbytes / 16 + (nbytes % 16 != 0);
  a.format = format; a.start = start; a.T = T; a.L = L; a.W = W; a.D = D; a.nb = y.nb;
  a.span = span;
  for (int j = 0; j < n; ++j) {
    const uint8_t* t = code->taps + (size_t)j * (m + 1);
    if (t[0] & 1) a.g0 |= 1u << j;
    for (int d = 1; d <= m; ++d)
      if (t[d] & 1) a.gs[j] |= 1u << (d - 1);
  }
  char* w = static_cast<char*>(d_work);
  a.dec = reinterpret_cast<uint64_t*>(w + y.dec);
  a.warm = reinterpret_cast<uint8_t*>(w + y.warm);
  a.endv = reinterpret_cast<uint8_t*>(w + y.endv);
  a.norm = reinterpret_cast<int32_t*>(w + y.norm);
  a.sst = reinterpret_cast<int32_t*>(w + y.sst);
  a.xs = reinterpret_cast<int32_t*>(w + y.xs);
  a.mis = reinterpret_cast<int32_t*>(w + y.mis);
  a.unc = reinterpret_cast<int32_t*>(w + y.unc);
  a.cnt = reinterpret_cast<unsigned long long*>(w + y.cnt);
  if (wide) {
    a.warm16 = reinterpret_cast<uint16_t*>(w + y.warm16);
    a.end16 = reinterpret_cast<uint16_t*>(w + y.end16);
  }
  a.bits = d_bits;
  a.stats = d_stats;
  *out = a;
  *launch = true;
  return CVD_OK;
}

extern "C" int64_t cvd_viterbi_workspace_bytes(int32_t n, int32_t m, int64_t T, int32_t block) {
  return cvd::viterbi_workspace_bytes(kWho, n, m, T, block, false);
}

extern "C" int cvd_viterbi_decode(const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                                  int64_t start, int64_t T, int32_t block, int32_t warm, int32_t depth,
                                  uint32_t* d_bits, int64_t* d_stats, void* d_work, void* stream) {
  if (const int rc = cvd::viterbi_code_shape(kWho, code)) return rc;
  const int n = code->n, m = code->m;
  int64_t span;
  if (T >= 0 && __builtin_mul_overflow(T, (int64_t)n, &span)) span = -1;
  if (T < 0) span = 0;                                   // reported as a bad T
  VArgs a;
  bool launch;
  const int rc = cvd::viterbi_setup(kWho, code, d_capture, nbits, format, start, T, span, block, warm, depth,
                                    CVD_VITERBI_WARM(m), CVD_VITERBI_DEPTH(m), d_bits, d_stats, d_work, &a, &launch);
  if (rc != CVD_OK || !launch) return rc;
  Kern fwd, join;
  pick(m, n, &fwd, &join);
  return cvd::viterbi_launch(m, a, fwd, join, stream);
}
