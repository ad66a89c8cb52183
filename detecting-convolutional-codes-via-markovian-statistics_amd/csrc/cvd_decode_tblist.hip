// cvd_viterbi_decode_frames_tailbiting_list (include/cvd.h) for gfx950: the L best tail-biting
// paths of every frame of a batch of soft frames, by the wrap-around Viterbi algorithm run on
// lists.  The launch shape, the keys, the step, the decisions and their tile are the list
// kernel's (cvd_decode_list.hip, cvd_decode_list_common.h); the laps and the stopping rule are the
// tail-biting kernel's (cvd_decode_tailbite_body.h).  One wavefront per frame, lane = next state
// (S > 64: SPL states per lane), grid-striding over the frames.  One launch does everything.
//   keys      (2 D << 4) | (b << 3) | r as in the list kernel, a lap seeded with 2 E^{l-1} in rank 0
//             of every state.  E <= 127 n m <= 3048 (a state is m steps from the best one), so
//             2 D <= 2 (127 * 3 * 8192 + 3048) < 2^23 and a key stays below 2^27 < kAbsent: the list
//             kernel's bound holds with room to spare.
//   ranks     the contract's lists hold L entries, the registers LL = 2, 4 or 8.  The result for L
//             is not a prefix of the result for LL (an entry of rank >= L can be tail-biting where
//             the lower ranks of its state are not), so the step makes ranks >= L absent.
//   lap       the step loop; the wave minimum of rank 0 and e*; then every lane walks the L chains
//             of each of its states back through the tile(s) for their start states a(e, r): L T
//             dependent LDS reads per state.  The ballot for B and the test E^l = E^{l-1} follow.
//   tiles     a frame whose decisions fit the tile never leaves LDS.  Otherwise the forward pass
//             leaves tile j < ntiles - 1 in piece j of the wave's slice and the last tile in LDS,
//             as in the list kernel, and both traces bring the tiles back last to first.  The slice
//             has no piece for the last tile, and the second trace needs it again, so the first
//             trace exchanges the tile in LDS with the piece it loads: it ends with tile 0 in LDS
//             and tile j + 1 in piece j, and the second trace reads them from there (its first
//             move is an exchange too, which parks tile 0 in the last piece).
//   choice    on the last lap an entry (e, r) is in C when a(e, r) = e, and then its cost is
//             A_T(e)[r] - E^{l-1}(e): the lane's own value.  Path 0 is the sibling's (e*, or the
//             best of B); only a path 0 of status 3 starts elsewhere, and the E of its start state
//             comes over one shuffle.  Paths 1.. are L - 1 rounds of a wave-wide minimum over
//             (c, e, r) in 64 bits (2 c < 2^24, e < 2^8, r < 2^3 do not fit 32), the winner's bit
//             cleared in its lane's mask of C.
//   trace     lanes l < L trace their chosen entries at once and store their rows, as in the list
//             kernel.
//   totals    wave-uniform sums, one atomic per total per wave at the end.
// wave64, no scratch.  Static LDS: the exchange buffer above 64 states; the tile is dynamic.
#include <hip/hip_runtime.h>
#include <limits.h>
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

constexpr uint64_t kNoEntry = ~0ull;               // choice: no entry of C is left

struct TlArgs {
  VArgs v;                   // cap, nu4, T, span, the code
  const int64_t* offsets;    // o_f, or null: o_f = v.start + f stride
  int64_t stride, nvals, F;
  int64_t slice;             // 16-byte pieces of a wave's slice of d_work: (ntiles - 1) tile16
  int32_t laps;              // I
  int32_t w;                 // words of a row of bits
  int32_t L;                 // paths asked for, <= LL
  int32_t tsteps, ntiles;    // steps of a tile, tiles of a frame
  int32_t tile16;            // 16-byte pieces of a tile
  uint4* work;               // d_work
  int32_t* paths;            // [F][L][3]
  int32_t* frames;           // [F][4]
  unsigned long long* tot;   // d_stats
};

__device__ __forceinline__ int64_t frame_offset(const TlArgs& la, int64_t f) {
  if (!la.offsets) return la.v.start + f * la.stride;
  const int64_t o = la.offsets[f];
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)o >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// x[s >> 6] of lane s & 63, for a wave-uniform state s
template <int SPL>
__device__ __forceinline__ int of_state(const int (&x)[SPL], int s) {
  int mine = x[0];
#pragma unroll
  for (int i = 1; i < SPL; ++i)
    if ((s >> 6) == i) mine = x[i];
  return __shfl(mine, s & (kWave - 1));
}

template <int m, int n, int LL>
__global__ __launch_bounds__(kWave) void viterbi_frames_tblist_kernel(TlArgs la) {
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
  // distance, decoded, skipped, paths, status 2, status 3, laps
  unsigned long long tdist = 0ull, tdec = 0ull, tskip = 0ull, tpaths = 0ull, tfall = 0ull, topen = 0ull, tlaps = 0ull;

  for (int64_t f = blockIdx.x; f < la.F; f += gridDim.x) {
    const int64_t o = frame_offset(la, f);
    uint32_t* row = la.v.bits + (f * L + lane) * w;      // lanes < L
    int32_t* prec = la.paths + (f * L + lane) * 3;       // lanes < L
    int32_t* frec = la.frames + f * 4;
    if (o < 0 || o > la.nvals - la.v.span) {             // offset mode only: the host has checked the stride
      if (lane < L) {
        for (int k = 0; k < w; ++k) row[k] = 0u;
        prec[0] = prec[1] = prec[2] = -1;
      }
      if (lane < 4) frec[lane] = lane == 1;
      ++tskip;
      continue;
    }

    uint32_t K[SPL][LL];
    int E2[SPL], DT[SPL];                                // 2 E^{l-1}; 2 D^l_T of the lane's states
    int as[SPL][LL];                                     // a^l(e, r) of the lane's entries
#pragma unroll
    for (int i = 0; i < SPL; ++i) E2[i] = 0;
    int lap = 0, es;
    bool closes;
    for (;;) {
      ++lap;
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
        K[i][0] = (uint32_t)E2[i] << 4;
#pragma unroll
        for (int r = 1; r < LL; ++r) K[i][r] = kAbsent;
      }

      // forward: steps [0, T), the decisions into the tile, full tiles but the last into the slice
      int tile = 0, tin = 0;
      for (int t0 = 0; t0 < T; t0 += kWave) {
        const int cnt = min(kWave, T - t0);
        int vp, ap;                                      // lane j < cnt: the values of step t0 + j, and their magnitudes' sum
        load_values<n>(cap + o, t0, cnt, lane, vp, ap);
        for (int jj = 0; jj < cnt; ++jj) {
          const int vs = __builtin_amdgcn_readlane(vp, jj);
          const int at = __builtin_amdgcn_readlane(ap, jj);
          uint32_t d[SPL];
          list_step<m, n, LL>(ln, K, xk, vs, at, L, d);
          if (lane < S) {
#pragma unroll
            for (int i = 0; i < SPL; ++i) dec[tin * S + ln.state(i)] = (E)d[i];
          }
          if (++tin == tsteps && t0 + jj + 1 < T) {      // the tile is full and the frame goes on
            tile_out(slice + (int64_t)tile * la.tile16, la.tile16, lane);
            tin = 0;
            ++tile;
          }
        }
      }

      // D^l_T = rank 0 (present in every state), its minimum and e*, the lowest-index state that has it
#pragma unroll
      for (int i = 0; i < SPL; ++i) DT[i] = (int)(K[i][0] >> 4);
      int mn = DT[0];
#pragma unroll
      for (int i = 1; i < SPL; ++i) mn = min(mn, DT[i]);
#pragma unroll
      for (int k = 1; k < kWave; k <<= 1) mn = min(mn, __shfl_xor(mn, k));
      es = 0;
#pragma unroll
      for (int i = SPL - 1; i >= 0; --i) {
        const uint64_t bal = __ballot(lane < S && DT[i] == mn);
        if (bal) es = kWave * i + __builtin_ctzll(bal);
      }

      // the trace of every entry: the chains of an absent entry read decisions of the tile too,
      // and what they reach is not used
      int ar[SPL][LL];
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
#pragma unroll
        for (int r = 0; r < LL; ++r) {
          as[i][r] = ln.state(i);
          ar[i][r] = r;
        }
      }
      __syncthreads();                                   // the last tile is written
      for (int tl = ntiles - 1; tl >= 0; --tl) {
        const int tb = tl * tsteps, te = min(T, tb + tsteps);
        if (tl != ntiles - 1) tile_swap(slice + (int64_t)tl * la.tile16, la.tile16, lane);
        for (int t = te - 1; t >= tb; --t) {
          const E* step = dec + (t - tb) * S;
#pragma unroll
          for (int i = 0; i < SPL; ++i) {
#pragma unroll
            for (int r = 0; r < LL; ++r) {
              if (r < L) {
                const uint32_t nib = ((uint32_t)step[as[i][r]] >> (4 * ar[i][r])) & 15u;
                as[i][r] = (as[i][r] >> 1) | ((int)(nib >> 3) << (m - 1));
                ar[i][r] = (int)(nib & (uint32_t)(LL - 1));
              }
            }
          }
        }
      }

      // the sibling's stopping rule on rank 0
      bool cl = false, same = lap >= 2;
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
        cl |= as[i][0] == ln.state(i) && ln.state(i) == es;
        same &= DT[i] - mn == E2[i];
      }
      closes = __any(cl);
      if (closes || lap == la.laps || __all(same)) break;
      __syncthreads();                                   // the tile has been read before the next lap writes it
#pragma unroll
      for (int i = 0; i < SPL; ++i) E2[i] = DT[i] - mn;
    }

    // C: bit i LL + r of inC says that the lane's entry (state(i), r) is present and tail-biting
    uint32_t inC = 0u;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
#pragma unroll
      for (int r = 0; r < LL; ++r)
        if (lane < S && r < L && K[i][r] < kAbsent && as[i][r] == ln.state(i)) inC |= 1u << (i * LL + r);
    }
    int nC = __builtin_popcount(inC);
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) nC += __shfl_xor(nC, k);
    uint32_t rank0 = 0u;                                 // the bits of rank 0
#pragma unroll
    for (int i = 0; i < SPL; ++i) rank0 |= 1u << (i * LL);
    const int status = closes ? 0 : __any((inC & rank0) != 0u) ? 2 : 3;

    // path 0: the sibling's
    int e0 = es;
    if (status == 2) {
      int best = INT_MAX;
#pragma unroll
      for (int i = 0; i < SPL; ++i)
        if ((inC >> (i * LL)) & 1u) best = min(best, DT[i] - E2[i]);
#pragma unroll
      for (int k = 1; k < kWave; k <<= 1) best = min(best, __shfl_xor(best, k));
#pragma unroll
      for (int i = SPL - 1; i >= 0; --i) {
        const uint64_t bal = __ballot(((inC >> (i * LL)) & 1u) && DT[i] - E2[i] == best);
        if (bal) e0 = kWave * i + __builtin_ctzll(bal);
      }
    }
    int a0[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) a0[i] = as[i][0];
    const int sa = of_state<SPL>(a0, e0);                // a(e0, 0)
    const int c0 = of_state<SPL>(DT, e0) - of_state<SPL>(E2, sa);      // 2 c of path 0
    uint32_t left = inC;                                 // C without (e0, 0) and the entries chosen
#pragma unroll
    for (int i = 0; i < SPL; ++i)
      if (ln.state(i) == e0) left &= ~(1u << (i * LL));

    // the chosen entries: lane l holds path l
    bool present = lane == 0;
    uint32_t metric = (uint32_t)c0;                      // 2 c
    int s = e0, r = 0;
    for (int round = 1; round < L; ++round) {
      uint64_t v = kNoEntry;
#pragma unroll
      for (int i = 0; i < SPL; ++i) {
#pragma unroll
        for (int q = 0; q < LL; ++q) {
          if ((left >> (i * LL + q)) & 1u)
            v = min(v, ((uint64_t)((K[i][q] >> 4) - (uint32_t)E2[i]) << 11) | (uint64_t)(ln.state(i) << 3) | (uint64_t)q);
        }
      }
#pragma unroll
      for (int k = 1; k < kWave; k <<= 1) v = min(v, (uint64_t)__shfl_xor((unsigned long long)v, k));
      if (v == kNoEntry) break;                          // wave-uniform
      const int ew = (int)((v >> 3) & 255u), rw = (int)(v & 7u);
      if (lane == round) {
        present = true;
        metric = (uint32_t)(v >> 11);
        s = ew;
        r = rw;
      }
#pragma unroll
      for (int i = 0; i < SPL; ++i)
        if (ln.state(i) == ew) left &= ~(1u << (i * LL + rw));
    }
    if (!present) s = r = 0;                             // any entry of the tile: what such a lane reads is not used
    const int sT = s;

    // traceback: every lane walks a chain, lanes < L store.  Tile 0 is in LDS and tile j + 1 in
    // piece j; the first move parks tile 0 in the last piece.
    uint32_t out = 0u;
    for (int tl = ntiles - 1; tl >= 0; --tl) {
      const int tb = tl * tsteps, te = min(T, tb + tsteps);
      if (ntiles > 1) {
        if (tl == ntiles - 1)
          tile_swap(slice + (int64_t)(ntiles - 2) * la.tile16, la.tile16, lane);
        else
          tile_in(slice + (int64_t)(tl ? tl - 1 : ntiles - 2) * la.tile16, la.tile16, lane);
      }
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
    if (lane < 4) frec[lane] = lane == 0 ? P : lane == 1 ? status : lane == 2 ? lap : nC;
    tdist += (unsigned long long)(c0 >> 1);
    ++tdec;
    tpaths += (unsigned long long)P;
    tfall += status == 2;
    topen += status == 3;
    tlaps += (unsigned long long)lap;
    __syncthreads();                                     // the tile has been read before the next frame writes it
  }
  if (lane == 0) {
    if (tdist) atomicAdd(&la.tot[0], tdist);
    if (tdec) atomicAdd(&la.tot[1], tdec);
    if (tskip) atomicAdd(&la.tot[2], tskip);
    if (tpaths) atomicAdd(&la.tot[3], tpaths);
    if (blockIdx.x == 0) la.tot[4] = (unsigned long long)la.w;
    if (tfall) atomicAdd(&la.tot[5], tfall);
    if (topen) atomicAdd(&la.tot[6], topen);
    if (tlaps) atomicAdd(&la.tot[7], tlaps);
  }
}

using TlKern = void (*)(TlArgs);
#define CVD_TL_ROW(n, LL)                                                                                  \
  {viterbi_frames_tblist_kernel<1, n, LL>, viterbi_frames_tblist_kernel<2, n, LL>,                         \
   viterbi_frames_tblist_kernel<3, n, LL>, viterbi_frames_tblist_kernel<4, n, LL>,                         \
   viterbi_frames_tblist_kernel<5, n, LL>, viterbi_frames_tblist_kernel<6, n, LL>,                         \
   viterbi_frames_tblist_kernel<7, n, LL>, viterbi_frames_tblist_kernel<8, n, LL>}

constexpr const char* kWho = "viterbi_decode_frames_tailbiting_list";

}  // namespace

extern "C" int64_t cvd_viterbi_tailbiting_list_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t L) {
  if (n < 2 || n > 3 || m < 1 || m > 8) return invalid(kWho, "needs n in 2..3 and m in 1..8");
  if (F < 0) return invalid(kWho, "needs F >= 0");
  if (L < 1 || L > CVD_VITERBI_LIST_MAX_L) return invalid(kWho, "L must be 1..8");
  if (F == 0) return 0;
  if (T < 1 || T > CVD_VITERBI_LIST_MAX_T) return invalid(kWho, "T must be 1..8192");
  const Tiling t = tiling_of(m, T, L);
  return list_waves(t, F) * t.slice_bytes;
}

extern "C" int cvd_viterbi_decode_frames_tailbiting_list(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                                         int64_t start, int64_t stride, const int64_t* d_offsets,
                                                         int64_t F, int32_t T, int32_t max_laps, int32_t L,
                                                         uint32_t* d_bits, int32_t* d_paths, int32_t* d_frames,
                                                         int64_t* d_stats, void* d_work, void* stream) {
  constexpr const char* who = kWho;
  if (const int rc = cvd::viterbi_code_shape(who, code)) return rc;
  const int n = code->n, m = code->m;
  if (nvals < 0) return invalid(who, "needs nvals >= 0");
  if (F < 0) return invalid(who, "needs F >= 0");
  if (max_laps < 0 || max_laps > CVD_VITERBI_TAILBITING_MAX_LAPS)
    return invalid(who, "max_laps must be 1..8, or 0 for the default");
  if (!d_offsets && (start < 0 || stride < 1)) return invalid(who, "needs start >= 0 and stride >= 1");
  if (L < 1 || L > CVD_VITERBI_LIST_MAX_L) return invalid(who, "L must be 1..8");
  if (F == 0) return CVD_OK;
  if (T < 1 || T > CVD_VITERBI_LIST_MAX_T) return invalid(who, "T must be 1..8192");
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

  TlArgs la{};
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
  la.laps = max_laps ? max_laps : CVD_VITERBI_TAILBITING_LAPS;
  la.w = (int32_t)w;
  la.L = L;
  la.tsteps = (int32_t)tl.tsteps;
  la.ntiles = (int32_t)tl.ntiles;
  la.tile16 = (int32_t)(tl.tile_bytes / 16);
  la.work = static_cast<uint4*>(d_work);
  la.paths = d_paths;
  la.frames = d_frames;
  la.tot = reinterpret_cast<unsigned long long*>(d_stats);

  static const TlKern kern[3][2][8] = {{CVD_TL_ROW(2, 2), CVD_TL_ROW(3, 2)},
                                       {CVD_TL_ROW(2, 4), CVD_TL_ROW(3, 4)},
                                       {CVD_TL_ROW(2, 8), CVD_TL_ROW(3, 8)}};
  const int LL = list_width(L);
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(d_stats, 0, 8 * sizeof(int64_t), st));
  hipLaunchKernelGGL(kern[LL == 2 ? 0 : LL == 4 ? 1 : 2][n - 2][m - 1], dim3((unsigned)list_waves(tl, F)), dim3(kWave),
                     (size_t)tl.tile_bytes, st, la);
  HIP_CHECK(hipGetLastError());
  return CVD_OK;
}
