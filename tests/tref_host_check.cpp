// Host check of the T_ref count behind the one-plane test (csrc/cvd_bitslice.h,
// CVD_BS_TREF_FAST), compiled with g++ by tests/test_tref_fast_host.py -- once as the header
// stands and once with -DCVD_BS_TREF_FAST=0, the exact count in every lane; both builds must
// pass and print the same digest of every step's planes, mu and c.
// At every layout phase, every received word y, and kUni false and true, the step's c
// (bs_step_core and bs_step_core_tab) is compared with the exact formulation (bs_halves_diff,
// bs_tref_of over all four planes) and its planes with the other form's, over
//   - random normalised vectors with metrics <= 12,
//   - the all-zero vector,
//   - vectors with equal partners on the even-e butterflies only (c = 2),
//   - vectors with equal halves (c = 4 with kUni, 2 without),
//   - vectors whose partners differ in ONE plane other than the tested one, on one even-e
//     butterfly: they pass the test and have c = 1;
// and every vector with c > 1 must be a suspect (bs_tref_test == 0), every non-suspect must
// report all1.  Stand-alone (its own main): also run under -fsanitize=address,undefined.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../detecting-convolutional-codes-via-markovian-statistics_amd/csrc/cvd_bitslice.h"

using namespace cvd;

static int parity(unsigned x) { return __builtin_popcount(x) & 1; }
static unsigned enc_out(const unsigned (&g)[2], unsigned s, unsigned u) {
  unsigned o = 0;
  for (int j = 0; j < 2; ++j) o |= (unsigned)parity(g[j] & (u | (s << 1))) << j;
  return o;
}
static unsigned g_rng = 2463534242u;
static unsigned rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

static uint64_t g_digest = 1469598103934665603ull;
static void mix(uint32_t v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

static long g_n[5] = {0, 0, 0, 0, 0}, g_susp = 0, g_susp_c1 = 0, g_checked = 0;

static void fail(const char* what, int ph, unsigned y, bool uni, int kind) {
  std::printf("FAIL %s at phase %d y %u uni %d input kind %d\n", what, ph, y, (int)uni, kind);
  std::exit(1);
}

// e0 of the state's location (own or partner: a pair shares its butterfly)
static bool e_even(const BsE& E, int s, int ph) {
  const int A = bs_addr(s, ph), B = bs_addr(s ^ 32, ph);
  return ((E.e0[A >> 5] >> (A & 31)) & 1u) == 0u || ((E.e0[B >> 5] >> (B & 31)) & 1u) == 0u;
}

// kind: 0 random, 1 zero, 2 equal partners on the even-e butterflies only, 3 equal halves,
// 4 one even-e pair differs in one plane other than the tested one
static void make_input(int kind, const BsE& E, int ph, uint8_t (&D)[64]) {
  for (int s = 0; s < 64; ++s) D[s] = kind == 1 ? 0 : (uint8_t)(rnd() % 13u);
  if (kind == 0) D[rnd() & 63u] = 0;
  if (kind >= 2) {
    for (int s = 0; s < 32; ++s) {
      const bool even = e_even(E, s, ph);
      if (kind == 2 && !even) {
        if (D[s + 32] == D[s]) D[s + 32] = (uint8_t)((D[s] + 1u) % 13u);
      } else {
        D[s + 32] = D[s];
      }
    }
    const int z = (int)(rnd() & 31u);
    if (kind != 2 || e_even(E, z, ph)) D[z] = D[z + 32] = 0;
    else { D[z] = 0; if (D[z + 32] == 0) D[z + 32] = 1; }
    if (kind == 4) {
      int s = (int)(rnd() & 31u);
      for (int k = 0; k < 32 && !e_even(E, s, ph); ++k) s = (s + 1) & 31;
      if (!e_even(E, s, ph)) { make_input(3, E, ph, D); return; }   // (no even-e butterfly under this y)
      static const int planes[3] = {0, 2, 3};
      const int pl = planes[rnd() % 3u];
      static_assert(kBsTrefPlane == 1, "the planes this input may differ in");
      D[s] &= 3u;
      D[s + 32] = (uint8_t)(D[s] ^ (1u << pl));
    }
  }
}

template <int PH, bool kUni>
static void check(const BsE& E, unsigned y, int kind, const uint8_t (&D)[64]) {
  bs_u32 img[8], R[2][4];
  bs_image(D, PH, img);
  for (int r = 0; r < 2; ++r)
    for (int i = 0; i < 4; ++i) R[r][i] = img[4 * r + i];
  bs_u32 N[2][4], N2[2][4], mu = 9u, mu2 = 9u, c = 99u, c2 = 99u;
  bool one = false, one2 = false;
  bs_step_core<PH, kUni>(R, E.e0, E.e1, E.ez, N, mu, c, BsNoMid(), &one);
  bs_step_core_tab<PH, kUni>(R, E.e0, [&](bool zero_hit) { return bs_mu_planes(E, !zero_hit); }, N2, mu2, c2,
                             BsNoMid(), &one2);
  // the exact formulation: all four planes of every state against its partner
  bs_u32 P[2][4], dh[2];
  bs_partner<PH>(R, P);
  dh[0] = bs_halves_diff(R[0], P[0]);
  dh[1] = bs_halves_diff(R[1], P[1]);
  const bs_u32 cex = bs_tref_of(dh, E.e0, kUni);
  const bool suspect = bs_tref_test<PH>(R, P, E.e0) == 0u;
  if (c != cex || c2 != cex) fail("count", PH, y, kUni, kind);
  if (mu != mu2 || one != one2) fail("table form", PH, y, kUni, kind);
  for (int r = 0; r < 2; ++r)
    for (int i = 0; i < 4; ++i)
      if (N[r][i] != N2[r][i]) fail("planes", PH, y, kUni, kind);
  if (cex > 1u && !suspect) fail("a c > 1 vector is not a suspect", PH, y, kUni, kind);
  if (CVD_BS_TREF_FAST != 0 && one != !suspect) fail("all1 flag", PH, y, kUni, kind);
  if (CVD_BS_TREF_FAST == 0 && one) fail("all1 flag without the test", PH, y, kUni, kind);
  // what the constructed inputs must give
  if (kind == 1 && cex != (kUni ? 4u : 2u)) fail("zero vector's count", PH, y, kUni, kind);
  if (kind == 2 && cex != 2u && !(kUni && cex == 4u)) fail("c = 2 input", PH, y, kUni, kind);
  if (kind == 3 && cex != (kUni ? 4u : 2u)) fail("equal halves' count", PH, y, kUni, kind);
  if (kind == 4 && !(suspect && (cex == 1u || (dh[0] | dh[1]) == 0u))) fail("one-plane input", PH, y, kUni, kind);
  for (int r = 0; r < 2; ++r)
    for (int i = 0; i < 4; ++i) mix(N[r][i]);
  mix(mu);
  mix(c);
  ++g_n[cex];
  g_susp += suspect;
  g_susp_c1 += suspect && cex == 1u;
  ++g_checked;
}

template <bool kUni>
static void check_any(int ph, const BsE& E, unsigned y, int kind, const uint8_t (&D)[64]) {
  switch (ph) {
    case 0: check<0, kUni>(E, y, kind, D); break;
    case 1: check<1, kUni>(E, y, kind, D); break;
    case 2: check<2, kUni>(E, y, kind, D); break;
    case 3: check<3, kUni>(E, y, kind, D); break;
    case 4: check<4, kUni>(E, y, kind, D); break;
    default: check<5, kUni>(E, y, kind, D); break;
  }
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 200;
  const unsigned g[2] = {0x6D, 0x4F};   // (133,171): "1011011", "1111001", bit d = tap d
  bs_u64 xm = 0;
  for (unsigned j = 0; j < 32; ++j) xm |= (bs_u64)enc_out(g, j, 0) << (2 * j);
  for (int ph = 0; ph < 6; ++ph)
    for (unsigned y = 0; y < 4; ++y) {
      const BsE E = bs_eplanes(xm, ph, y);
      for (int kind = 0; kind < 5; ++kind)
        for (int k = 0; k < (kind == 1 ? 1 : reps); ++k) {
          uint8_t D[64];
          make_input(kind, E, ph, D);
          check_any<false>(ph, E, y, kind, D);
          check_any<true>(ph, E, y, kind, D);
        }
    }
  std::printf("ok checked=%ld fast=%d c1=%ld c2=%ld c4=%ld suspects=%ld suspects_c1=%ld digest=%016llx\n", g_checked,
              (int)(CVD_BS_TREF_FAST != 0), g_n[1], g_n[2], g_n[4], g_susp, g_susp_c1, (unsigned long long)g_digest);
  return 0;
}
