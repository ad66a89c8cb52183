// How often the T_ref count's one-plane necessary test passes (csrc/cvd_bitslice.h, CVD_BS_TREF_FAST):
// the header's host step over recorded streams, compiled and driven by profiles/tref_suspects.py.
//
//   tref_suspects <words file> <nseq> <nsteps>
//
// The file holds nseq * nsteps received words (one byte each, sequence-major, trial-id order).
// Every sequence runs the Eq. 4-5 recursion from D_0 = 0 through bs_step_core (its exact count
// c); beside it, for each plane i, the masked partner difference
//     x_i = ((R[0][i] ^ P[0][i]) & ~e0[0]) | ((R[1][i] ^ P[1][i]) & ~e0[1])
// whose vanishing makes the lane a "suspect" of plane i.  Printed as one JSON object: per
// candidate (single planes and ORs of two), the share of lane-steps that are suspects and the
// share of 64-lane wave-steps (sequences grouped 64 at a time) with at least one, over all steps
// and over steps >= 64; the share of lane-steps with c > 1; and whether a c > 1 step was ever
// not a suspect (must be 0).  CPU only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../detecting-convolutional-codes-via-markovian-statistics_amd/csrc/cvd_bitslice.h"

using namespace cvd;

static int parity(unsigned x) { return __builtin_popcount(x) & 1; }
static unsigned enc_out(const unsigned (&g)[2], unsigned s, unsigned u) {
  unsigned o = 0;
  for (int j = 0; j < 2; ++j) o |= (unsigned)parity(g[j] & (u | (s << 1))) << j;
  return o;
}

constexpr int kCand = 7;   // planes 0..3, then 1|2, 1|3, 2|3
static const char* kCandName[kCand] = {"plane0", "plane1", "plane2", "plane3", "plane1|2", "plane1|3", "plane2|3"};

template <int PH, bool kUni>
static void one(const bs_u32 (&R)[2][4], const BsE& E, bs_u32 (&N)[2][4], bs_u32& c, bs_u32 (&x)[4]) {
  bs_u32 P[2][4], mu;
  bs_partner<PH>(R, P);
  for (int i = 0; i < 4; ++i) x[i] = ((R[0][i] ^ P[0][i]) & ~E.e0[0]) | ((R[1][i] ^ P[1][i]) & ~E.e0[1]);
  bs_step_core<PH, kUni>(R, E.e0, E.e1, E.ez, N, mu, c);
}
template <bool kUni>
static void any(int ph, const bs_u32 (&R)[2][4], const BsE& E, bs_u32 (&N)[2][4], bs_u32& c, bs_u32 (&x)[4]) {
  switch (ph) {
    case 0: one<0, kUni>(R, E, N, c, x); break;
    case 1: one<1, kUni>(R, E, N, c, x); break;
    case 2: one<2, kUni>(R, E, N, c, x); break;
    case 3: one<3, kUni>(R, E, N, c, x); break;
    case 4: one<4, kUni>(R, E, N, c, x); break;
    default: one<5, kUni>(R, E, N, c, x); break;
  }
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const long nseq = std::atol(argv[2]), nsteps = std::atol(argv[3]);
  std::vector<uint8_t> w((size_t)nseq * nsteps);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(w.data(), 1, w.size(), f) != w.size()) return 3;
  std::fclose(f);
  // the decoder: (133,171), taps as tests/bs_host_check.cpp
  const unsigned g[2] = {0x6D, 0x4F};   // "1011011", "1111001", bit d = tap d
  bs_u64 xm = 0;
  bool uni = true;
  for (unsigned j = 0; j < 32; ++j) {
    const unsigned o = enc_out(g, j, 0);
    if (enc_out(g, j, 1) != (o ^ 3u) || enc_out(g, j + 32, 0) != (o ^ 3u)) return 4;
    xm |= (bs_u64)o << (2 * j);
    if (parity(o)) uni = false;
  }
  BsE E[6][4];
  for (int ph = 0; ph < 6; ++ph)
    for (unsigned y = 0; y < 4; ++y) E[ph][y] = bs_eplanes(xm, ph, y);
  // susp[k][t * nseq + s]: candidate k's suspect flag
  std::vector<uint8_t> susp((size_t)kCand * nseq * nsteps);
  long cgt1[2] = {0, 0}, missed = 0;
  for (long s = 0; s < nseq; ++s) {
    bs_u32 R[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    for (long t = 0; t < nsteps; ++t) {
      const unsigned y = w[(size_t)s * nsteps + t] & 3u;
      bs_u32 N[2][4], c, x[4];
      if (uni) any<true>((int)(t % 6), R, E[t % 6][y], N, c, x);
      else any<false>((int)(t % 6), R, E[t % 6][y], N, c, x);
      const bool z[kCand] = {x[0] == 0u, x[1] == 0u, x[2] == 0u, x[3] == 0u,
                             (x[1] | x[2]) == 0u, (x[1] | x[3]) == 0u, (x[2] | x[3]) == 0u};
      for (int k = 0; k < kCand; ++k) {
        susp[((size_t)k * nsteps + t) * nseq + s] = z[k];
        if (c > 1u && !z[k]) ++missed;
      }
      if (c > 1u) {
        ++cgt1[0];
        if (t >= 64) ++cgt1[1];
      }
      for (int r = 0; r < 2; ++r)
        for (int i = 0; i < 4; ++i) R[r][i] = N[r][i];
    }
  }
  const long nw = (nseq + 63) / 64;
  std::printf("{\"nseq\": %ld, \"nsteps\": %ld, \"uni\": %d, \"missed\": %ld, \"c_gt1_lane\": %.3e, \"c_gt1_lane_ge64\": %.3e",
              nseq, nsteps, (int)uni, missed, (double)cgt1[0] / ((double)nseq * nsteps),
              nsteps > 64 ? (double)cgt1[1] / ((double)nseq * (nsteps - 64)) : 0.0);
  for (int k = 0; k < kCand; ++k) {
    long lane[2] = {0, 0}, wave[2] = {0, 0};
    for (long t = 0; t < nsteps; ++t)
      for (long g0 = 0; g0 < nw; ++g0) {
        long n = 0;
        for (long s = 64 * g0; s < nseq && s < 64 * g0 + 64; ++s) n += susp[((size_t)k * nsteps + t) * nseq + s];
        lane[0] += n;
        wave[0] += n != 0;
        if (t >= 64) {
          lane[1] += n;
          wave[1] += n != 0;
        }
      }
    std::printf(", \"%s\": {\"lane\": %.3e, \"wave\": %.3e, \"lane_ge64\": %.3e, \"wave_ge64\": %.3e}", kCandName[k],
                (double)lane[0] / ((double)nseq * nsteps), (double)wave[0] / ((double)nw * nsteps),
                nsteps > 64 ? (double)lane[1] / ((double)nseq * (nsteps - 64)) : 0.0,
                nsteps > 64 ? (double)wave[1] / ((double)nw * (nsteps - 64)) : 0.0);
  }
  std::printf("}\n");
  return 0;
}
