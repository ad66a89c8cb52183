// cvd_viterbi_decode_frames_list and cvd_frames_crc (include/cvd.h) for gfx950: the L best paths of
// every frame of a batch of soft frames (the parallel list Viterbi algorithm), and a CRC over rows
// of decoded bits, so that the first candidate that passes a frame's own check is found without
// the bits leaving the device.
//
// The list kernel has the frames family's launch shape: one wavefront per frame, lane = next state
// (S > 64: SPL states per lane), grid-striding over the frames so that the lane's branch patterns
// (SLane::init, cvd_decode_lanes.h) are built once per wave.  One launch does everything.
//   keys      the LL = 2, 4 or 8 metrics of a state are registers holding sort keys
//             (2 D << 4) | (b << 3) | r: unsigned order on whole keys is the contract's order on
//             (c, b, r), and the low nibble of a surviving key is its decision.  The loop carries
//             2 D, not the soft lane's x = 2 D - sum A: the step adds sdot4(pattern, values, A_t),
//             which is 2 cost >= 0, so keys are unsigned without an offset and the distance needs
//             no sum at the end.  2 D <= 2 * 127 * 3 * 8192 < 2^23, a key is below 2^27; kAbsent =
//             2^31 is above every key of a path, an absent entry plus a cost stays above it, and
//             the merge's result is clamped to it, so absent entries do not drift.  L = 1, 3, 5..7
//             run the next power of two and the outputs are truncated, which the contract states
//             to be exact.
//   step      the two predecessors' lists come over LL ds_bpermute each (S <= 64) or through the
//             LDS exchange xk (S > 64, [rank][state], one buffer: the block is one wave, so the
//             two barriers are waits on the wave's own LDS instructions).  A candidate is
//             (key & ~15) + (2 cost << 4 | b << 3) + r.  The merge is the half-cleaner
//             min(a_i, b_{LL-1-i}) and log2 LL stages of min / max on whole keys.
//   decisions a nibble per (state, rank) per step, packed into one uint8 / uint16 / uint32 per
//             state, written to a tile of `tsteps` steps in LDS.  A frame whose decisions fit the
//             tile never leaves LDS.  Otherwise a full tile is copied, 16 bytes per lane, to the
//             wave's own slice of d_work (reused frame after frame, so it stays in cache) and the
//             traceback brings the tiles back last to first; the last tile is still resident.  A
//             chain of dependent loads from global memory would cost an L2 round trip per step;
//             through a tile it costs an LDS read.
//   end       end_state fixed: lane l takes entry l of that state's list.  CVD_FRAME_ANY: LL rounds
//             of a wave-wide minimum over (2 D << 8 | state) of the lists' heads (the lists are
//             sorted, so the head is a state's least remaining rank); the winner drops its head.
//   trace     lanes l < L trace their paths at once, one serial chain per lane through the tile,
//             each building and storing its own words of its own row.
//   totals    wave-uniform sums, one atomic per total per wave at the end.
// The values are loaded as the soft-output kernel loads them (cvd_decode_llr_body.h): lane j reads
// the n bytes of step t0 + j of a chunk of 64 steps, nothing outside the frame, and the step loop
// takes them by v_readlane.  SLane's staged loader is part of SLane::run, whose acs_chunk carries
// one metric per state; the patterns and sdot4 candidates are SLane's.
//
// cvd_frames_crc: a row per lane, for every w.  The register is kept left-aligned in 32 bits, so
// that one 256-entry table in LDS (built by the block from the call's poly) serves every width
// 1..32; 32 bits of a row at any bit offset come from two words through a funnel shift and are
// bit-reversed, which puts the first bit of each byte in its most significant place; the ragged
// tail (count mod 32 bits) goes bit by bit, and the field is one more funnel read.  A row per wave
// would have to combine 64 partial registers over GF(2) (a 32 x 32 matrix per distance) to save
// strided reads that only matter for rows of hundreds of words; the rows this serves are a few
// words long and there are F L >= 64 of them.  wave64, no scratch.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "../../include/cvd.h"
#include "cvd_decode_common.h"
#include "cvd_decode_lanes.h"
#include "cvd_decode_list_common.h"
#include "cvd_internal.h"

namespace {

using namespace cvd::vit;

constexpr uint32_t kNoHead = 0xffffffffu;          // end selection: a state without a remaining entry
constexpr int kCrcThreads = 256;
constexpr int kCrcBlocks = 4096;

struct LsArgs {
  VArgs v;                   // cap, nu4, T, span, the code
  const int64_t* offsets;    // o_f, or null: o_f = v.start + f stride
  int64_t stride, nvals, F;
  int64_t slice;             // 16-byte pieces of a wave's slice of d_work: (ntiles - 1) tile16
  int32_t s0, e;             // start_state, end_state (CVD_FRAME_ANY: -1)
  int32_t w;                 // words of a row of bits
  int32_t L;                 // paths asked for, <= LL
  int32_t tsteps, ntiles;    // steps of a tile, tiles of a frame
  int32_t tile16;            // 16-byte pieces of a tile
  uint4* work;               // d_work
  int32_t* paths;            // [F][L][3]
  int32_t* frames;           // [F][2]
  unsigned long long* tot;   // d_stats
};

__device__ __forceinline__ int64_t frame_offset(const LsArgs& la, int64_t f) {
  if (!la.offsets) return la.v.start + f * la.stride;
  const int64_t o = la.offsets[f];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)o >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int m, int n, int LL>
__global__ __launch_bounds__(kWave) void viterbi_frames_list_kernel(LsArgs la) {
  using Sh = Shape<m>;
  using E = typename DecWord<LL>::type;
  constexpr int S = Sh::S, SPL = Sh::SPL;
  __shared__ uint32_t xk[SPL > 1 ? LL * S : 1];
  E* dec = reinterpret_cast<E*>(list_tile);
  SLane<m, n> ln;
  ln.init(la.v);
  const int lane = ln.lane;
  const int8_t* cap = reinterpret_cast<const int8_t*>(la.v.cap);
  uint4* slice = la.work + (int64_t)blockIdx.x * la.slice;
  const int T = (int)la.v.T, w = la.w, L = la.L, tsteps = la.tsteps, ntiles = la.ntiles;
  unsigned long long tdist = 0ull, tdec = 0ull, tskip = 0ull, tpaths = 0ull;

  for (int64_t f = blockIdx.x; f < la.F; f += gridDim.x) {
    const int64_t o = frame_offset(la, f);
    uint32_t* row = la.v.bits + (f * L + lane) * w;      // lanes < L
    int32_t* prec = la.paths + (f * L + lane) * 3;       // lanes < L
    int32_t* frec = la.frames + f * 2;
    if (o < 0 || o > la.nvals - la.v.span) {             // offset mode only: the host has checked the stride
      if (lane < L) {
        for (int k = 0; k < w; ++k) row[k] = 0u;
        prec[0] = prec[1] = prec[2] = -1;
      }
      if (lane < 2) frec[lane] = lane;
      ++tskip;
      continue;
    }

    uint32_t K[SPL][LL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      K[i][0] = la.s0 < 0 || ln.state(i) == la.s0 ? 0u : kAbsent;
#pragma unroll
      for (int r = 1; r < LL; ++r) K[i][r] = kAbsent;
    }

    // forward: steps [0, T), the decisions into the tile, full tiles but the last into the slice
    int tile = 0, tin = 0;
    for (int t0 = 0; t0 < T; t0 += kWave) {
      const int cnt = min(kWave, T - t0);
      int vp, ap;                                        // lane j < cnt: the values of step t0 + j, and their magnitudes' sum
      load_values<n>(cap + o, t0, cnt, lane, vp, ap);
      for (int jj = 0; jj < cnt; ++jj) {
        const int vs = __builtin_amdgcn_readlane(vp, jj);
        const int at = __builtin_amdgcn_readlane(ap, jj);
        uint32_t d[SPL];
        list_step<m, n, LL>(ln, K, xk, vs, at, LL, d);
        if (lane < S) {
#pragma unroll
          for (int i = 0; i < SPL; ++i) dec[tin * S + ln.state(i)] = (E)d[i];
        }
        if (++tin == tsteps && t0 + jj + 1 < T) {        // the tile is full and the frame goes on
          tile_out(slice + (int64_t)tile * la.tile16, la.tile16, lane);
          tin = 0;
          ++tile;
        }
      }
    }

    // the end list: lane l < LL takes entry l
    uint32_t metric = 0u;
    int s = 0, r = 0;
    bool present = false;
    if (la.e >= 0) {
      uint32_t mine = kAbsent;
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
#pragma unroll
        for (int q = 0; q < LL; ++q) {
          const uint32_t x = (uint32_t)__shfl((int)K[i][q], la.e & (kWave - 1));
          if ((la.e >> 6) == i && lane == q) mine = x;
        }
      }
      present = mine < kAbsent;
      metric = mine >> 4;
      s = la.e;
      r = lane & (LL - 1);
    } else {
      int used[SPL];
#pragma unroll
      for (int i = 0; i < SPL; ++i) used[i] = 0;
      for (int round = 0; round < LL; ++round) {
        uint32_t v = kNoHead;
#pragma unroll
        for (int i = 0; i < SPL; ++i)
          if (lane < S && K[i][0] < kAbsent) v = min(v, ((K[i][0] >> 4) << 8) | (uint32_t)ln.state(i));
#pragma unroll
        for (int k = 1; k < kWave; k <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, k));
        const int sw = (int)(v & 255u);                  // the winner, if v is a head
        int my = 0;
#pragma unroll
        for (int i = 0; i < SPL; ++i)
          if ((sw >> 6) == i) my = used[i];
        const int rk = __shfl(my, sw & (kWave - 1));
        if (lane == round) {
          present = v != kNoHead;
          metric = v >> 8;
          s = sw;
          r = rk;
        }
        const bool win = v != kNoHead && lane == (sw & (kWave - 1));
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
          if (win && (sw >> 6) == i) {
#pragma unroll
            for (int q = 0; q + 1 < LL; ++q) K[i][q] = K[i][q + 1];
            K[i][LL - 1] = kAbsent;
            ++used[i];
          }
        }
      }
    }
    present = present && lane < L;
    if (!present) s = r = 0;                             // any entry of the tile: what such a lane reads is not used
    const int sT = s;

    // traceback: every lane walks a chain, lanes < L store
    uint32_t out = 0u;
    __syncthreads();                                     // the last tile is written
    for (int tl = ntiles - 1; tl >= 0; --tl) {
      const int tb = tl * tsteps, te = min(T, tb + tsteps);
      if (tl != ntiles - 1) tile_in(slice + (int64_t)tl * la.tile16, la.tile16, lane);
      for (int t = te - 1; t >= tb; --t) {
        out |= (uint32_t)(s & 1) << (t & 31);
        const uint32_t d = dec[(t - tb) * S + s];
        const uint32_t nib = (d >> (4 * r)) & 15u;
        s = (s >> 1) | ((int)(nib >> 3) << (m - 1));
        r = (int)(nib & (uint32_t)(LL - 1));
        if ((t & 31) == 0) {
          if (lane < L) row[t >> 5] = present ? out : 0u;
          out = 0u;
        }
      }
    }
    if (lane < L) {
      prec[0] = present ? (int32_t)(metric >> 1) : -1;
      prec[1] = present ? s : -1;
      prec[2] = present ? sT : -1;
    }
    const int P = __builtin_popcountll(__ballot(present));
    if (lane < 2) frec[lane] = lane == 0 ? P : 0;
    tdist += (unsigned long long)(__builtin_amdgcn_readfirstlane((int)metric) >> 1);
    ++tdec;
    tpaths += (unsigned long long)P;
    __syncthreads();                                     // the tile has been read before the next frame writes it
  }
  if (lane == 0) {
    if (tdist) atomicAdd(&la.tot[0], tdist);
    if (tdec) atomicAdd(&la.tot[1], tdec);
    if (tskip) atomicAdd(&la.tot[2], tskip);
    if (tpaths) atomicAdd(&la.tot[3], tpaths);
    if (blockIdx.x == 0) la.tot[4] = (unsigned long long)la.w;
  }
}

// rows of w words; thread = row.  polyl, initl: left-aligned in 32 bits.
__global__ __launch_bounds__(kCrcThreads) void frames_crc_kernel(const uint32_t* bits, int64_t rows, int32_t w,
                                                                  int32_t first, int32_t count, int32_t width,
                                                                  uint32_t polyl, uint32_t initl, uint32_t* value) {
  __shared__ uint32_t tab[256];
  {
    uint32_t x = (uint32_t)threadIdx.x << 24;            // eight zero bits from a register whose top byte is the index
#pragma unroll
    for (int k = 0; k < 8; ++k) x = (x & 0x80000000u) ? (x << 1) ^ polyl : x << 1;
    tab[threadIdx.x] = x;
  }
  __syncthreads();
  // bits [pos, pos + 32) of the row, bit pos first = most significant; those at or past 32 w read as 0
  auto get32 = [w](const uint32_t* W, int pos) {
    const int idx = pos >> 5, sh = pos & 31;
    const uint32_t lo = W[idx], hi = idx + 1 < w ? W[idx + 1] : 0u;
    return __builtin_bitreverse32((uint32_t)((((uint64_t)hi << 32) | lo) >> sh));
  };
  const int full = count >> 5, rem = count & 31;
  for (int64_t row = (int64_t)blockIdx.x * kCrcThreads + threadIdx.x; row < rows;
       row += (int64_t)gridDim.x * kCrcThreads) {
    const uint32_t* W = bits + row * w;
    uint32_t reg = initl;
    for (int c = 0; c < full; ++c) {
      const uint32_t x = get32(W, first + 32 * c);
#pragma unroll
      for (int k = 0; k < 4; ++k) reg = (reg << 8) ^ tab[((reg ^ (x << (8 * k))) >> 24) & 255u];
    }
    int pos = first + 32 * full;                         // < 32 w: the field follows
    if (rem) {
      uint32_t x = get32(W, pos);
      for (int k = 0; k < rem; ++k) {
        const uint32_t fb = (reg ^ x) & 0x80000000u;
        reg <<= 1;
        x <<= 1;
        if (fb) reg ^= polyl;
      }
      pos += rem;
    }
    const uint32_t field = get32(W, pos);
    value[row] = (reg ^ field) >> (32 - width);
  }
}

using LsKern = void (*)(LsArgs);
#define CVD_LS_ROW(n, LL)                                                                                  \
  {viterbi_frames_list_kernel<1, n, LL>, viterbi_frames_list_kernel<2, n, LL>,                             \
   viterbi_frames_list_kernel<3, n, LL>, viterbi_frames_list_kernel<4, n, LL>,                             \
   viterbi_frames_list_kernel<5, n, LL>, viterbi_frames_list_kernel<6, n, LL>,                             \
   viterbi_frames_list_kernel<7, n, LL>, viterbi_frames_list_kernel<8, n, LL>}

constexpr const char* kWho = "viterbi_decode_frames_list";
constexpr const char* kWhoCrc = "frames_crc";

}  // namespace

extern "C" int64_t cvd_viterbi_list_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t L) {
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(kWho, "needs n in 2..3 and m in 1..8");
  if (F < 0) return invalid(kWho, "needs F >= 0");
  if (L < 1 || L > CVD_VITERBI_LIST_MAX_L) return invalid(kWho, "L must be 1..8");
  if (F == 0) return 0;
  if (T < 1 || T > CVD_VITERBI_LIST_MAX_T) return invalid(kWho, "T must be 1..8192");
  const Tiling t = tiling_of(m, T, L);
  return list_waves(t, F) * t.slice_bytes;
}

extern "C" int cvd_viterbi_decode_frames_list(const cvd_code* code, const int8_t* d_soft, int64_t nvals, int64_t start,
                                              int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                              int32_t start_state, int32_t end_state, int32_t L, uint32_t* d_bits,
                                              int32_t* d_paths, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                              void* stream) {
  constexpr const char* who = kWho;
  if (const int rc = cvd::viterbi_code_shape(who, code)) return rc;
  const int n = code->n, m = code->m;
  if (nvals < 0) return invalid(who, "needs nvals >= 0");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (start_state < CVD_FRAME_ANY || start_state >= (1 << m) || end_state < CVD_FRAME_ANY || end_state >= (1 << m))
    return invalid(who, "start_state and end_state must be CVD_FRAME_ANY or a state in [0, 2^m)");
  if (!d_offsets && (start < 0 || stride < 1)) return invalid(who, "needs start >= 0 and stride >= 1");
  if (L < 1 || L > CVD_VITERBI_LIST_MAX_L) return invalid(who, "L must be 1..8");
  if (F == 0) return CVD_OK;
  if (T < 1 || T > CVD_VITERBI_LIST_MAX_T) return invalid(who, "T must be 1..8192");
  if (start_state >= 0 && end_state >= 0 && T < m)
    return invalid(who, "with both states fixed T must be at least m: end_state is not reachable before");
  const int64_t w = (T + 31) / 32, lw = (int64_t)L * w;
  if (F >= ((int64_t)1 << 31) / lw + (((int64_t)1 << 31) % lw != 0))
    return invalid(who, "F * L * ceil(T / 32) must be below 2^31 words");
  const int64_t span = (int64_t)n * T;
  if (!d_offsets) {
    int64_t end;
    if (__builtin_mul_overflow(F - 1, stride, &end) || __builtin_add_overflow(end, start, &end) ||
        __builtin_add_overflow(end, span, &end))
      return invalid(who, "the position of the last frame's end overflows int64");
    if (end > nvals) return invalid(who, "the frames do not lie inside [0, nvals)");
  }
  const Tiling tl = tiling_of(m, T, L);
  if (!d_soft || !d_bits || !d_paths || !d_frames || !d_stats || (tl.slice_bytes && !d_work) ||
      ((uintptr_t)d_soft & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_paths & 3) ||
      ((uintptr_t)d_frames & 3) || ((uintptr_t)d_stats & 7) || ((uintptr_t)d_offsets & 7))
    return invalid(who, "d_soft, d_work (16-byte aligned; d_work null only where the workspace is 0 bytes), d_stats "
                        "(8-byte), d_bits, d_paths and d_frames (4-byte) must be non-null, d_offsets 8-byte aligned");

  LsArgs la{};
  VArgs& a = la.v;
  a.cap = reinterpret_cast<const uint4*>(d_soft);
  a.nu4 = nvals / 16 + (nvals % 16 != 0);
  a.format = CVD_CAPTURE_BYTES;
  a.start = d_offsets ? 0 : start;
  a.T = T;
  a.span = span;
  list_code_taps(code, a);
  a.bits = d_bits;
  la.offsets = d_offsets;
  la.stride = stride;
  la.nvals = nvals;
  la.F = F;
  la.slice = tl.slice_bytes / 16;
  la.s0 = start_state;
  la.e = end_state;
  la.w = (int32_t)w;
  la.L = L;
  la.tsteps = (int32_t)tl.tsteps;
  la.ntiles = (int32_t)tl.ntiles;
  la.tile16 = (int32_t)(tl.tile_bytes / 16);
  la.work = static_cast<uint4*>(d_work);
  la.paths = d_paths;
  la.frames = d_frames;
  la.tot = reinterpret_cast<unsigned long long*>(d_stats);

  static const LsKern kern[3][2][8] = {{CVD_LS_ROW(2, 2), CVD_LS_ROW(3, 2)},
                                       {CVD_LS_ROW(2, 4), CVD_LS_ROW(3, 4)},
                                       {CVD_LS_ROW(2, 8), CVD_LS_ROW(3, 8)}};
  const int LL = list_width(L);
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats, 0, 5 * sizeof(int64_t), st));
  hipLaunchKernelGGL(kern[LL == 2 ? 0 : LL == 4 ? 1 : 2][n - 2][m - 1], dim3((unsigned)list_waves(tl, F)), dim3(kWave),
                     (size_t)tl.tile_bytes, st, la);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}

extern "C" int cvd_frames_crc(const uint32_t* d_bits, int64_t rows, int32_t w, int32_t first, int32_t count,
                              int32_t width, uint32_t poly, uint32_t init, uint32_t* d_value, void* stream) {
  constexpr const char* who = kWhoCrc;
  if (width < 1 || width > 32) return invalid(who, "width must be 1..32");
  if (width < 32 && ((poly >> width) || (init >> width))) return invalid(who, "poly and init must be below 2^width");
  if (first < 0 || count < 0) return invalid(who, "needs first >= 0 and count >= 0");
  if (w < 1 || rows < 0) return invalid(who, "needs w >= 1 and rows >= 0");
  if ((int64_t)first + count + width > (int64_t)32 * w)
    return invalid(who, "first + count + width must not exceed the 32 w bits of a row");
  if (rows == 0) return CVD_OK;
  if (!d_bits || !d_value || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_value & 3))
    return invalid(who, "d_bits and d_value must be non-null and 4-byte aligned");
  const int64_t blocks = (rows + kCrcThreads - 1) / kCrcThreads;
  hipLaunchKernelGGL(frames_crc_kernel, dim3((unsigned)std::min<int64_t>(blocks, kCrcBlocks)), dim3(kCrcThreads), 0,
                     (hipStream_t)stream, d_bits, rows, w, first, count, width, poly << (32 - width),
                     init << (32 - width), d_value);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}
