// The m = 6 bit-sliced detector k1s (the JIT's CVD_K1B_BITSLICE=1 variant of the
// code-specialised kernel, cvd_rtc.cpp).  Included at the end of cvd_device.h (whose
// ExpArgs, filter patterns, walk-mode constants and helpers it uses); the run-time compile
// embeds it after that file.
//
// The detector of k1b_body / k1b_walk, sums identical bit for bit, with the 64 metrics as
// four bit-planes of two words in the rotating layout of cvd_bitslice.h.
// Per step: the branch-metric planes of (phase, y) from an LDS table, mu first, the ACS of
// both words (own and partner adds, a borrow-chain min), the T_ref count off the partner
// planes and, for a lane whose new vector must be hashed, the canonical digest hash.  The
// row tables are the bit-sliced ones (cvd_host.cpp build_hash with bs): the Bloom filter
// over the digest hash, 256-byte directory slots {six phase images, the row's record}, six
// images per learned row by row id (walk mode) and the usual dense records; in front of the
// L2 filter, a 2^20-bit pre-filter in LDS (CVD_K1S_PF).  The layout phase is compile-time in
// the lockstep loop (six steps per iteration) and wave-uniform in walk mode.  A launch over
// more sequences than stay resident is persistent: one block per slot, each wave taking 64
// sequences at a time from a work queue (k1s_body).
#pragma once

// Variants that were measured, refuted and removed (DESIGN.md §10 keeps their figures), and forms
// that are now the code: a build that still names one would silently measure the default kernel
#if defined(CVD_K1S_SLOT3) || defined(CVD_K1S_DEEP) || defined(CVD_K1S_T2) || defined(CVD_K1S_TRIM) || \
    defined(CVD_K1S_MIDPOS) || defined(CVD_K1S_VMASK) || defined(CVD_K1S_PADV) || defined(CVD_K1S_ABL) || \
    defined(CVD_WALK_BUF) || defined(CVD_K1S_AMASK) || defined(CVD_K1S_R16) || defined(CVD_K1S_NT_STREAM) || \
    defined(CVD_BS_ETAB2)
#error "removed k1s knob: CVD_K1S_SLOT3, CVD_K1S_DEEP, CVD_K1S_T2, CVD_K1S_TRIM, CVD_K1S_MIDPOS, CVD_K1S_VMASK, CVD_K1S_PADV, CVD_K1S_ABL, CVD_WALK_BUF, CVD_K1S_AMASK, CVD_K1S_R16, CVD_K1S_NT_STREAM and CVD_BS_ETAB2 no longer exist (DESIGN.md §10)"
#endif

#ifndef CVD_K1B_BITSLICE
#define CVD_K1B_BITSLICE 0
#endif

namespace cvd_dev {

constexpr int kBsSlotShift = 6;      // directory slot: 64 dwords
constexpr int kBsRecWord = 48;       // record r at dwords 48 + 4 r of a slot (images 8 x 6 before it)
template <int PH>
__device__ __forceinline__ constexpr uint32_t bs_img_off() { return 32u * PH; }   // byte offset of phase PH's image
constexpr uint32_t kBsRecOff = 4u * kBsRecWord;                                   // and of the record
constexpr int kBsDkeyWords = 48;     // six images per row in a.dkey
constexpr int kBsEarlyGroups = 21;   // early-decision check every 126 steps
// the LDS pre-filter variant (cvd_kernels.hip upload_model; 1,024-thread blocks, 128 KiB of
// dynamic LDS): a lane tests D_t's pre-filter bit before it requests its L2 filter word
#ifndef CVD_K1S_PF
#define CVD_K1S_PF 0
#endif
// chunked launches (-DCVD_K1S_CK=0 compiles them out, for A/Bs of the unchunked
// loop's code: the host then must not chunk, CVD_CHUNK=0)
#ifndef CVD_K1S_CK
#define CVD_K1S_CK 1
#endif
// Walk mode (k1s_walk) compiled in (default) or out (-DCVD_K1S_WALK=0; the host then must not set
// a.walk: cvd_kernels.hip builds the walking variant on first use).  A kernel's VGPR count is
// the largest over all its code, and walk mode's is the larger one: with the pre-filter 115
// against the lockstep loop's 90, so the kernel that only runs the lockstep loop is allocated
// 104 registers per lane (CVD_K1B_ENTRY_ATTR below) instead of 120 and its four waves leave 96
// of a SIMD's 512 to a co-resident kernel -- a generator wave -- instead of 32 (DESIGN.md §7.1,
// register budget)
#ifndef CVD_K1S_WALK
#define CVD_K1S_WALK 1
#endif
// The entries' occupancy attribute (cvd_rtc.cpp entry_source, spec_resource.py).  By its ~90
// registers alone the kernel without walk mode would hold five waves per SIMD, and the compiler
// then schedules for five; its blocks never hold more than CVD_K1B_WAVES (1,024 threads around
// 128 KiB of LDS, or 256 threads with 35 KiB).  Told so, the compiler gives the six-step loop the
// schedule it has in the walking build (32 s_waitcnt instead of 40, the same 90 registers):
// without the attribute the lockstep launches alone measured 0.2-1.2% longer than the walking
// build's (profiles/coresident/ab.json, overlap_0).  The walking build is compiled as before.
#if CVD_K1B_BITSLICE && !CVD_K1S_WALK
#define CVD_K1B_ENTRY_ATTR __attribute__((amdgpu_waves_per_eu(CVD_K1B_WAVES, CVD_K1B_WAVES)))
#else
#define CVD_K1B_ENTRY_ATTR
#endif
// Word offsets: a step's received words enter the cursor and the branch-metric table as byte
// offsets 16 r, each one v_lshrrev and one v_and of the six-step group's window shifted once --
// both take vector or constant operands at ~2.5 cycles per wave64 instruction -- instead of a
// v_bfe (its shift held in a VGPR) then v_lshlrev / v_lshl_add at ~4.2 each (profiles/r05an)
// a raw word r as a cursor / step word parameter, the byte offset 16 r
__device__ __forceinline__ uint32_t word_param(uint32_t r) { return 16u * r; }

// The lockstep lanes read each 16-B stream chunk once: non-temporal loads, so that the 131 GB per
// launch do not evict the row tables' lines from L2 (p = 0.1 / 0.15 2,074 / 2,040 -> 2,041-2,049 /
// 2,008 ms, profiles/r05y)
typedef unsigned int bs_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 stream_load(const uint4* p) {
  const bs_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const bs_u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

// LDS (cvd_bitslice.h bs_step_core_tab): per (phase, y) e0 of both words for the zero test, and
// the mu-specific addend planes -- {e0m, a1, p1, a23} of word 0, the same of word 1, {p23 of
// word 0, of word 1} -- read at the offset mu selects instead of selecting the planes with the
// mu mask: 8 VALU fewer per step than the select form (bs_step_core).
// Same sums (119 GPU parity tests); the six-p sweep 1,375,820-1,377,109 -> 1,397,206-1,399,600
// trials/s on one box (profiles/r06ab, three rounds)
// (16-B strides per word y, so that the word parameter 16 y is the byte offset itself and the
// phase and mu parts are the reads' immediate offsets and one add: e0 at [phase][y] in 16-B
// slots; the mu planes in three sub-tables of [phase][mu][y] 16-B slots each)
constexpr uint32_t kBsMtSub = 6 * 2 * 4 * 16;   // bytes per mu sub-table
__device__ __forceinline__ uint4* bs_e0_lds() {
  __shared__ uint4 s_e0[6 * 4];
  return s_e0;
}
__device__ __forceinline__ uint4* bs_mt_lds() {
  __shared__ uint4 s_mt[3 * 6 * 2 * 4];
  return s_mt;
}
template <uint64_t XM>
__device__ __forceinline__ void fill_bs_etab() {
  uint4* e = bs_e0_lds();
  uint4* t = bs_mt_lds();
  for (int i = threadIdx.x; i < 24; i += blockDim.x) {
    const int ph = i >> 2, y = i & 3;
    const cvd::BsE E = cvd::bs_eplanes(XM, ph, (uint32_t)y);
    e[i] = make_uint4(E.e0[0], E.e0[1], 0u, 0u);
    for (int m = 0; m < 2; ++m) {
      const cvd::BsMu T = cvd::bs_mu_planes(E, m == 1);
      const int k = (ph * 2 + m) * 4 + y;   // 16-B slot in each sub-table
      t[k] = make_uint4(T.e0m[0], T.a1[0], T.p1[0], T.a23[0]);
      t[k + kBsMtSub / 16] = make_uint4(T.e0m[1], T.a1[1], T.p1[1], T.a23[1]);
      t[k + 2 * (kBsMtSub / 16)] = make_uint4(T.p23[0], T.p23[1], 0u, 0u);
    }
  }
}
// the ACS of one step from the mu-specific planes; mid as bs_step_core's
// (one, wave-uniform: no lane of the wave can have c > 1 -- cvd_bitslice.h CVD_BS_TREF_FAST)
template <int PH, bool kUni, class Mid>
__device__ __forceinline__ void bs_core_tab(const uint32_t (&R)[2][4], uint32_t rr, uint32_t (&N)[2][4], uint32_t& c,
                                            bool& one, Mid mid) {
  // e0 of both words at (phase PH, word parameter rr)
  const uint2 E0 = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(bs_e0_lds()) + PH * 64 + rr);
  const uint32_t e0[2] = {E0.x, E0.y};
  uint32_t mu;
  cvd::bs_step_core_tab<PH, kUni>(
      R, e0,
      [&](bool zero_hit) {
        const char* tb = reinterpret_cast<const char*>(bs_mt_lds()) + PH * 128;
        const uint32_t o = rr + (zero_hit ? 0u : 64u);
        const uint4 w0 = *reinterpret_cast<const uint4*>(tb + o);
        const uint4 w1 = *reinterpret_cast<const uint4*>(tb + o + kBsMtSub);
        const uint2 q = *reinterpret_cast<const uint2*>(tb + o + 2u * kBsMtSub);
        cvd::BsMu T;
        T.e0m[0] = w0.x; T.a1[0] = w0.y; T.p1[0] = w0.z; T.a23[0] = w0.w;
        T.e0m[1] = w1.x; T.a1[1] = w1.y; T.p1[1] = w1.z; T.a23[1] = w1.w;
        T.p23[0] = q.x; T.p23[1] = q.y;
        return T;
      },
      N, mu, c, mid, &one);
}
// lr += ltref[c]: the constant ltref[1] (lt1) where the step found no suspect lane in the wave
// (one: c is then not set), without the LDS read
// (the empty asm keeps the two adds apart: merged, the constant would be moved into the LDS
// value's registers at every step)
__device__ __forceinline__ void bs_lt_add(double& lr, const double* s_lt, double lt1, uint32_t c, bool one) {
  if (__builtin_expect(one, 1)) {
    lr += lt1;
  } else {
    lr += s_lt[c];
    asm volatile("" : "+v"(lr));
  }
}

// P̂1 row cursor over the bit-sliced tables (RowCursor's protocol: slot >= 0 known row id,
// -1 known unvisited row, -2 pending hash probe).  The lookup of D_t is issued AHEAD of the
// resolve of D_{t-1} (hash_ahead, right after the ACS): every lane whose D_{t-1} row is not
// known from a successor record (slot < 0) hashes D_t and reads its filter word before the
// step waits for D_{t-1}'s key and record loads; the lanes whose D_{t-1} turns out to be a
// row (a filter-positive candidate that matches) simply do not use it.  So the filter read
// has the rest of the step and half of the next one to land, and the key and record loads
// the second word's ACS plus the hash.
// One record load per step (kBsOneLoad, BsCursor::mid) in the kernels that read the filter from
// L2 (the pre-filter and plain variants; p >= 0.05 of the sweep, 0.7-2.8% shorter launches).  The
// LDS-filter variants (p = 0.01, 0.02; separate builds, CVD_K1B_LDSF) keep the two sites -- a
// known row's dense record requested after the resolve for the next word, a candidate's at mid():
// their H1 lanes are on a row at 94% of the steps, few steps hold both kinds, and the merged
// form's address selection cost them more VALU than the load it saved (p = 0.01 1,278 -> 1,311
// ms, VALU per wave-step 115.7 -> 119.1, VMEM 1.28 -> 1.12; DESIGN.md §2, profiles/record_load)
#if CVD_K1B_LDSF
constexpr bool kBsOneLoad = false;
#else
constexpr bool kBsOneLoad = true;
#endif
struct BsCursor {
  int32_t slot, pnx;
  uint32_t hs, hsn, fb, fw, fb1, fw1, pc;   // hs: home slot of D_{t-1}'s lookup, hsn: of D_t's
  bool cand;
  double plp;
  uint32_t pkey[8];
  // entry rn (16 B {log P̂1, successor row, T_ref count c}) of learned row s, dense records:
  // walk mode's one-step record, and the lockstep loop's without kBsOneLoad
  // (every k1s offset is a 32-bit byte offset from the table's base: the host keeps the
  // bit-sliced tables under 4 GiB)
  __device__ void prefetch_row(const ExpArgs& a, int32_t s, uint32_t rn) {
    uint32_t o;
    asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(o) : "v"((uint32_t)s), "v"(rn));
    take(ld_off<uint4>(a.drow, o));
  }
  __device__ void take(const uint4& v) {
    pc = v.w;
    pnx = (int32_t)v.z;
    plp = __hiloint2double((int)v.y, (int)v.x);
  }
  // (no record is loaded here: with kBsOneLoad every step's is requested at its mid(), without
  // it the caller requests row slot0's for the first word)
  __device__ void start(const ExpArgs& a) {
    slot = a.slot0; pnx = -1; hs = 0u; hsn = 0u; fb = 0u; fw = 0u; fb1 = 0u; fw1 = 0u; cand = false; pc = 1u; plp = 0.0;
  }
  // ordering fences (RowCursor::fence): the waits for the loads issued a step / half a step
  // earlier land after the ACS work the dependency names.  fence_mid: the filter words (the
  // candidate test); fence_resolve: the lookup state of D_{t-1} (its key, record, slot) --
  // not the filter words hash_ahead has just requested
  __device__ void fence_mid(uint32_t dep) {
    asm volatile("" : "+v"(fw), "+v"(fw1), "+v"(slot) : "v"(dep));
  }
  __device__ void fence_resolve(uint32_t dep) {
    asm volatile("" : "+v"(slot), "+v"(pnx), "+v"(plp), "+v"(pc) : "v"(dep));
#pragma unroll
    for (int w = 0; w < 8; ++w) asm volatile("" : "+v"(pkey[w]) : "v"(dep));
  }
  __device__ static uint32_t slot_off(uint32_t s) { return s << (kBsSlotShift + 2); }
  __device__ static void load_image(const uint32_t* base, uint32_t o, uint32_t (&k)[8]) {
    const uint4 u = ld_off<uint4>(base, o), v = ld_off<uint4>(base, o + 16u);
    k[0] = u.x; k[1] = u.y; k[2] = u.z; k[3] = u.w; k[4] = v.x; k[5] = v.y; k[6] = v.z; k[7] = v.w;
  }
  // The record {log P̂1, successor, c} of this step (word r), one load for the wave (kRow): a
  // filter-positive candidate's from its home slot, a known row's dense one -- which lies behind
  // the directory in the same allocation, at a.rec_off -- and for a lane that needs neither
  // one line that such lanes share (as filter word 0 in hash_ahead).  A candidate has
  // slot == -2, so the two kinds never meet in a lane; loaded apart, a wave that holds one lane
  // of each kind issued two instructions per step, and the step's time follows their count
  // (DESIGN.md §2).  No divergent branch around the load; a wave without a lane of either kind
  // (most steps of an H2 wave) skips it by a wave-uniform test.  A candidate also loads the home
  // slot's image of phase PH.
  // (!kRow, walk mode's ACS steps: candidates only, a lane that has just left its rows keeps
  // the record walk_prefetch loaded; so without kBsOneLoad, where next_row() requests a row's)
  template <int PH, bool kRow>
  __device__ void mid(const ExpArgs& a, uint32_t r) {
    // (two v_bitop3: the compiler's form was six VALU)
    cand = slot == -2 && cvd::bs_bop3<cvd::kTtAndNotOr>(fb1, fw1, cvd::bs_bop3<cvd::kTtAndNotOr>(fb, fw, 0u)) == 0u;
    if constexpr (kRow && kBsOneLoad) {
      bs_u32x4 v;
      if (__ballot(cand || slot >= 0) != 0u) {
        // both records as 64-B units from the base: a slot's at 4 hs + 3 (kBsRecOff = 3 * 64),
        // row s's at rec_off / 64 + s; so four VALU to the address: shift-or, add, select, and
        // one shift-add with the word offset.  (A lane that is neither has slot = -1 or -2 and
        // reads the directory's last 128 bytes, a line such lanes share; nothing uses it.)
        static_assert(kBsRecOff == 192u && kBsSlotShift == 6, "a slot's records are its fourth 64-B unit");
        uint32_t uc, o;
        asm("v_lshl_or_b32 %0, %1, 2, 3" : "=v"(uc) : "v"(hs));
        const uint32_t ud = (uint32_t)slot + (a.rec_off >> 6);
        asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(o) : "v"(cand ? uc : ud), "v"(r));
        v = ld_off<bs_u32x4>(a.hkey, o);
      } else {
        // (no lane reads the record: any contents of the four registers will do, and saying so
        // keeps the last step's record from living on through the skipped load, which made the
        // loaded one a copy that is waited for at once)
        asm volatile("" : "=v"(v));
      }
      take(make_uint4(v.x, v.y, v.z, v.w));
      if (cand) load_image(a.hkey, slot_off(hs) + bs_img_off<PH>(), pkey);
    } else if (cand) {
      const uint32_t so = slot_off(hs);
      load_image(a.hkey, so + bs_img_off<PH>(), pkey);
      take(ld_off<uint4>(a.hkey, so + kBsRecOff + r));
    }
  }
  __device__ static bool same(const uint32_t (&k)[8], const uint32_t (&R)[2][4]) {
    uint32_t d = k[0] ^ R[0][0];
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[1], R[0][1], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[2], R[0][2], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[3], R[0][3], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[4], R[1][0], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[5], R[1][1], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[6], R[1][2], d);
    d = cvd::bs_bop3<cvd::kTtXorOr>(k[7], R[1][3], d);
    asm volatile("" : "+v"(d));
    return d == 0u;
  }
  // log P̂1(row(D_{t-1}), r), D_{t-1} = planes R at phase PH; afterwards `slot` describes row(D_t)
  template <int PH>
  __device__ double resolve(const ExpArgs& a, const uint32_t (&R)[2][4], uint32_t r, double lpu) {
    // the known row's record, or the pending state (-2: D_t's lookup) and the unseen-row term, by a
    // sign mask and three v_bitop3 -- not a compare and three selects on it (static loop cost 3,168
    // -> 3,069 cycles per six steps, profiles/r06ad); a candidate implies slot == -2, so it needs
    // no test of the row being known
    const uint32_t m = (uint32_t)(slot >> 31);   // ~0: D_{t-1}'s row is not known
    int32_t ns = (int32_t)cvd::bs_bop3<cvd::kTtSel>(m, (uint32_t)-2, (uint32_t)pnx);
    double lpv =
        __hiloint2double((int)cvd::bs_bop3<cvd::kTtSel>(m, (uint32_t)__double2hiint(lpu), (uint32_t)__double2hiint(plp)),
                         (int)cvd::bs_bop3<cvd::kTtSel>(m, (uint32_t)__double2loint(lpu), (uint32_t)__double2loint(plp)));
    if (cand) {
      if (same(pkey, R)) {
        lpv = plp; ns = pnx;
      } else if (pc != 0u) {
        // the home slot holds another row (an empty slot has c = 0): linear probing up to
        // an empty slot
        uint32_t sl = hs;
        for (int pr = 1; pr <= a.max_probe; ++pr) {
          sl = (sl + 1u) & a.hmask;
          const uint32_t so = slot_off(sl);
          const uint4 v = ld_off<uint4>(a.hkey, so + kBsRecOff + r);
          if (v.w == 0u) break;
          uint32_t k[8];
          load_image(a.hkey, so + bs_img_off<PH>(), k);
          if (same(k, R)) {
            lpv = __hiloint2double((int)v.y, (int)v.x);
            ns = (int32_t)v.z;
            break;
          }
        }
      }
    }
    slot = ns;
    return lpv;
  }
  // D_t (planes N at phase PH) is known, D_{t-1}'s lookup not yet resolved: a lane whose
  // D_{t-1} row is not known from a successor (slot < 0) may need D_t's lookup, so it hashes
  // D_t and requests the filter word now
  // (no divergent branch: a wave hashes whenever one lane needs it anyway, and a load under
  // a divergent branch made the compiler's wait counts conservative -- it waited for this
  // load at the resolve, vmcnt(0).  A lane that does not need the lookup reads filter word 0
  // instead: every such lane of a wave shares that one L2 line; reading each lane's own
  // block measured 26% slower at p = 0.05, where most H1 lanes walk their rows' successors)
  template <int PH>
  __device__ void hash_ahead(const ExpArgs& a, const uint32_t (&N)[2][4]) {
    uint32_t ph, pl;
    cvd::bs_digest_hash<PH>(N, ph, pl);
    hsn = ph & a.hmask;
    const uint2 pp = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(filter_patterns_lds()) +
                                                     (ph & (uint32_t)((cvd::kFilterPatterns - 1) << 3)));
    fb = pp.x;
    fb1 = pp.y;
#if CVD_K1S_PF
    // the pre-filter bit of D_t (LDS): clear -- D_t is not a row -- and the lane reads filter
    // word 0 like a lane that needs no lookup, with an all-ones pattern that word 0 cannot match,
    // so no candidate follows
    const uint32_t pfw = reinterpret_cast<const uint32_t*>(dyn_lds())[__builtin_amdgcn_ubfe(
        pl, 32 - cvd::kBsPfLog2Bits + 5, cvd::kBsPfLog2Bits - 5)];
    // (bit (pl >> (32 - kBsPfLog2Bits)) mod 32 of the word: the extract takes the offset's
    // low five bits)
    const uint32_t pbit = __builtin_amdgcn_ubfe(pfw, pl >> (32 - cvd::kBsPfLog2Bits), 1u);
    // (masks instead of compares and selects: pm = ~0 where the bit is set, sm = ~0 where
    // D_{t-1}'s row is not known)
    const uint32_t pm = 0u - pbit, sm = (uint32_t)(slot >> 31);
    fb = cvd::bs_bop3<0xF3>(fb, pm, 0u);    // fb | ~pm
    fb1 = cvd::bs_bop3<0xF3>(fb1, pm, 0u);
    const uint32_t fo = cvd::bs_bop3<0x80>(pl, pm, sm) & a.fmask4;
#else
    const uint32_t fo = slot < 0 ? (pl & a.fmask4) : 0u;
#endif
#if CVD_K1B_LDSF
    const uint2 f = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(dyn_lds()) + fo);
#else
    const uint2 f = ld_off<uint2>(a.filt, fo);
#endif
    fw = f.x;
    fw1 = f.y;
  }
  // after the resolve: D_t's home slot becomes the pending lookup's
  __device__ void next() { hs = hsn; }
  // the same with two load sites (the lockstep loop without kBsOneLoad): first a known row's
  // dense record for the next word rn
  __device__ void next_row(const ExpArgs& a, uint32_t rn) {
    if (slot >= 0) prefetch_row(a, slot, rn);
    next();
  }
};

// one bit-sliced step of a lane: D_{t-1} = R (phase PH) -> N (phase PH + 1) under word rr,
// the record and filter-positive loads issued between the two words' ACS
template <int PH, bool kUni, bool kRow = true>
__device__ __forceinline__ void bs_step(const ExpArgs& a, BsCursor& cur, const uint32_t (&R)[2][4], uint32_t rr,
                                        uint32_t (&N)[2][4], uint32_t& c, bool& one) {
  bs_core_tab<PH, kUni>(R, rr, N, c, one, [&](uint32_t dep) {
    cur.fence_mid(dep);            // dep: the first word's ACS result
    cur.template mid<PH, kRow>(a, rr);
  });
  cur.template hash_ahead<(PH + 1) % 6>(a, N);   // D_t's filter read before D_{t-1}'s loads are waited for
  cur.fence_resolve(N[1][3]);                    // N[1][3] depends on the whole ACS
}

// H1 waves in walk mode (k1b_walk's schedule; the planes' layout phase is the wave's)
template <uint64_t XM>
__device__ __forceinline__ void k1s_walk(const ExpArgs& a, int64_t qwave, uint64_t vmask, const double* s_lt) {
  constexpr bool kUni = xm_uni<6, XM>();
  if (CVD_WALK_ABL & 1) return;
  const bool valid = qwave + lane_id() < a.nseq;
  const uint32_t N = (uint32_t)a.N;
  const uint32_t nwords = (N + 15u) / 16u;
  const size_t cstride = (size_t)a.nseq * 4;
  auto load_word = [&](uint32_t wi) -> uint32_t {
    if (wi >= nwords) return 0u;
    // (a plain load: walk mode reads a 16-B chunk's four words one at a time, and non-temporal
    // lines were gone before the next word -- p = 0.01 1,411 -> 1,489 ms, profiles/r05y)
    return a.r[(size_t)(wi >> 2) * cstride + (size_t)(qwave + lane_id()) * 4 + (wi & 3u)];
  };
  uint32_t pos = 0u, curw = 0u, nxtw = 0u;
  bool need = false;   // the lane moved into nxtw: the word after it is requested at the loop's top
  // the words pos / 16 and pos / 16 + 1
  auto cur_word = [&]() -> uint32_t { return curw; };
  auto nxt_word = [&]() -> uint32_t { return nxtw; };
  auto word_at = [&]() -> uint32_t { return cur_word() >> (2u * (pos & 15u)); };
  auto advance = [&]() {
    ++pos;
    if ((pos & 15u) == 0u) {
      curw = nxtw;
      need = true;
    }
  };
  uint32_t R[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  double lp = 0.0, lr = 0.0;
  BsCursor cur;
  cur.slot = -1; cur.pnx = -1; cur.hs = 0u; cur.hsn = 0u; cur.fb = 0u; cur.fw = 0u; cur.fb1 = 0u; cur.fw1 = 0u;
  cur.cand = false; cur.plp = 0.0; cur.pc = 1u;
  double plp2 = 0.0;
  auto two_steps = [&]() -> bool { return a.t2 != nullptr && pos + 2u <= N; };
  auto walk_prefetch = [&]() {
    const uint32_t x = __builtin_amdgcn_alignbit(nxt_word(), cur_word(), 2u * (pos & 15u));   // r of steps pos + 1, pos + 2
    if (two_steps() && a.t2c) {
      // the compact record (8 B, cvd_host.cpp t2c): both steps' log P̂1 as indices into the
      // model's value table, copied into LDS by the block; rows + 1 in 16 bits, c in 3
      uint32_t o;
      asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(o) : "v"(x & 15u), "v"((uint32_t)cur.slot << 7));
      const uint2 e = ld_off<uint2>(a.t2, o);
      const double* vt = reinterpret_cast<const double*>(reinterpret_cast<const char*>(dyn_lds()) + a.vtab_off);
      cur.plp = vt[e.x & 0xFFFu];
      plp2 = vt[(e.x >> 12) & 0xFFFu];
      cur.pnx = (int32_t)(__builtin_amdgcn_alignbit(e.y, e.x, 24u) & 0xFFFFu) | (int32_t)(((e.y >> 8) & 7u) << 28);
      cur.pc = ((e.y >> 11) & 0xFFFFu) | (((e.y >> 27) & 7u) << 28);
    } else if (two_steps()) {
      uint32_t o;
      asm("v_lshl_add_u32 %0, %1, 5, %2" : "=v"(o) : "v"(x & 15u), "v"((uint32_t)cur.slot << 9));
      const uint4 v = ld_off<uint4>(a.t2, o);
      const uint2 w = ld_off<uint2>(a.t2, o + 16u);
      cur.pc = w.y;
      cur.pnx = (int32_t)w.x;
      plp2 = __hiloint2double((int)v.w, (int)v.z);
      cur.plp = __hiloint2double((int)v.y, (int)v.x);
    } else {
      cur.prefetch_row(a, cur.slot, word_param(x & 3u));
    }
  };
  uint32_t mode = kWalkDone;
  int dec = 0;
  auto finished = [&]() -> bool {
    if (pos == N) return true;
    if (a.early && (pos & (uint32_t)(kEarlyEvery - 1)) == 0u) dec = early_decide(lp, lr, (int64_t)(N - pos), a.lt_min, a.lp_min);
    return dec != 0;
  };
  if (valid && N > 0u) {
    curw = load_word(0u);
    nxtw = load_word(1u);
    cur.slot = a.slot0;   // D_0 = 0 is a learned row: every lane starts walking
    walk_prefetch();
    mode = kWalkWalk;
  }
  uint32_t phw = 0u;   // layout phase of the ACS lanes' planes (wave-uniform)
  const double lt1 = a.ltref[1];
  // one ACS step of the wave at phase PH (every lane computes; ACS lanes keep the result)
  auto acs_step = [&](auto phc) {
    constexpr int PH = decltype(phc)::value;
    const uint32_t rr = word_param(word_at() & 3u);
    uint32_t Nn[2][4], c;
    bool one;
    bs_step<PH, kUni, false>(a, cur, R, rr, Nn, c, one);
    if (mode == kWalkAcs) {
      lp += cur.template resolve<PH>(a, R, rr, a.lp_unseen);   // Pd_plotter.py:115, T = P̂1
      bs_lt_add(lr, s_lt, lt1, c, one);   // Pd_plotter.py:115, T = T_ref(1/2)
      advance();
      cur.next();
      if (finished()) {
        mode = kWalkDone;
        cur.slot = -1;
      } else if (cur.slot >= 0) {
        mode = kWalkWalk;
        walk_prefetch();
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) R[r][i] = Nn[r][i];
  };
  const uint32_t wmin = (uint32_t)a.walk_wmin, amin = (uint32_t)a.walk_amin;
  const int burst = a.walk_burst;
  for (int64_t it = 0, it_max = CVD_WALK_GUARD * ((int64_t)N + 1); it < it_max; ++it) {
    if (need) {
      nxtw = load_word((pos >> 4) + 1u);
      need = false;
    }
    const uint64_t mA = __ballot(mode == kWalkAcs), mW = __ballot(mode == kWalkWalk);
    if ((mA | mW) == 0u) break;
    const uint32_t nA = (uint32_t)__popcll(mA), nW = (uint32_t)__popcll(mW);
    if (nW != 0u && (nA == 0u || nW >= wmin || nA < amin)) {
      for (int b = 0; b < burst; ++b) {
        if (mode == kWalkWalk) {
          // D_t is not a row: the lane joins the ACS steps with D_{t-1} = row `slot`, its
          // planes the row's image at the wave's phase; that step takes log P̂1 from
          // cur.plp with successor -1
          auto leave = [&]() {
            // (timing ablation, CVD_WALK_ABL & 8: a lane that leaves its rows skips that step and
            // walks on from row 0 -- the walk's own cost without the leavers' ACS steps; every
            // leave still advances the lane, so the loop ends)
            if (CVD_WALK_ABL & 8) {
              cur.slot = a.slot0;
              advance();
              if (finished()) {
                mode = kWalkDone;
                cur.slot = -1;
              } else {
                walk_prefetch();
              }
              return;
            }
            mode = kWalkAcs;
            cur.pnx = -1;
            const uint32_t ko = (uint32_t)cur.slot * (4u * kBsDkeyWords) + 32u * phw;
            const uint4 u = ld_off<uint4>(a.dkey, ko), v = ld_off<uint4>(a.dkey, ko + 16u);
            R[0][0] = u.x; R[0][1] = u.y; R[0][2] = u.z; R[0][3] = u.w;
            R[1][0] = v.x; R[1][1] = v.y; R[1][2] = v.z; R[1][3] = v.w;
          };
          auto done = [&]() {
            mode = kWalkDone;
            cur.slot = -1;
          };
          if (two_steps()) {
            const int32_t d1 = (int32_t)((uint32_t)cur.pnx & 0x0FFFFFFFu) - 1;
            if (d1 < 0) {
              leave();
            } else {
              lp += cur.plp;                 // Pd_plotter.py:115, from the row's records
              lr += s_lt[(uint32_t)cur.pnx >> 28];
              cur.slot = d1;
              advance();
              if (finished()) {
                done();
              } else {
                const int32_t d2 = (int32_t)(cur.pc & 0x0FFFFFFFu) - 1;
                if (d2 < 0) {
                  cur.plp = plp2;
                  leave();
                } else {
                  lp += plp2;
                  lr += s_lt[cur.pc >> 28];
                  cur.slot = d2;
                  advance();
                  if (finished()) done();
                  else walk_prefetch();
                }
              }
            }
          } else if (cur.pnx < 0) {
            leave();
          } else {
            lp += cur.plp;                   // Pd_plotter.py:115, from the row's record
            lr += s_lt[cur.pc];
            cur.slot = cur.pnx;
            advance();
            if (finished()) done();
            else walk_prefetch();
          }
        }
        if (__ballot(mode == kWalkWalk) == 0u) break;
      }
      continue;
    }
    // two ACS steps of the wave (phases phw, phw + 1; phw is even); a lane the first sends
    // back to a walk waits out the second
    if (phw == 0u) {
      acs_step(IntC<0>{});
      acs_step(IntC<1>{});
    } else if (phw == 2u) {
      acs_step(IntC<2>{});
      acs_step(IntC<3>{});
    } else {
      acs_step(IntC<4>{});
      acs_step(IntC<5>{});
    }
    phw = phw == 4u ? 0u : phw + 2u;
  }
  // the guard is never reached (every iteration moves a lane); if it were, the partial
  // sums must not pass for results (k1b_walk)
  if (__ballot(mode != kWalkDone) != 0u && lane_id() == 0 && a.err) atomicOr(a.err, 1);
  if (valid && a.sums) {
    const int64_t qe = qwave + lane_id();
    a.sums[2 * qe] = lp;
    a.sums[2 * qe + 1] = lr;
  }
  early_final(dec, lp, lr);
  count_decisions_masked(vmask, vmask, lp, lr, a.counts);
}

// one wave's 64 sequences [64 gw, 64 gw + 64) through the lockstep loop, or walk mode
// chunked detection (a.ck_n > 0): a lane's 8 plane words into its chunk record
// (dword `off`: 0 = D at the chunk start, 8 = D at its end; both in layout phase 0)
__device__ __forceinline__ void ck_store(const ExpArgs& a, int64_t qwave, int32_t j, uint32_t off,
                                         const uint32_t (&R)[2][4]) {
  uint32_t l = lane_id();
  asm volatile("" : "+v"(l));   // (keeps the address arithmetic in the rarely taken branch)
  uint4* p = reinterpret_cast<uint4*>(a.ck_out + ((size_t)j * (size_t)a.nseq + (size_t)qwave + l) * kCkRecWords + off);
  p[0] = make_uint4(R[0][0], R[0][1], R[0][2], R[0][3]);
  p[1] = make_uint4(R[1][0], R[1][1], R[1][2], R[1][3]);
}

// (kCk: a chunked launch's unit; a separate instantiation, so that the unchunked loop keeps its
// registers and scalar state exactly)
template <uint64_t XM, bool kCk = false>
__device__ __forceinline__ void k1s_wave(const ExpArgs& a, int64_t gw, const double* s_lt, int32_t ck_j = 0) {
  constexpr bool kUni = xm_uni<6, XM>();
  if (a.walk || (a.mix && !kCk)) {
    // H1 and H2 waves alternate on every SIMD (k1b_body; lockstep too where a.mix: the units of
    // a persistent launch are taken in order, so that without it the first half of the launch
    // runs H1 waves only and the second H2 waves only)
    const int64_t half = ((a.nseq + 63) / 64 + 1) / 2, k = gw >> 1;
    if (gw < 2 * half) gw = ((gw ^ (gw >> 2)) & 1) ? half + k : k;
  }
  const int64_t qwave = gw * 64;
  const int64_t q = qwave + lane_id();
  const bool valid = q < a.nseq;
  const uint64_t vmask = __ballot(valid), hmask = __ballot(q < a.n_h1);
  if constexpr (CVD_K1S_WALK != 0) {
    if (a.walk && vmask != 0u && hmask == vmask) {
      k1s_walk<XM>(a, qwave, vmask, s_lt);
      return;
    }
  }
  // (timing ablation, CVD_WALK_ABL & 4: a walk launch's lockstep (H2) waves do nothing)
  if ((CVD_WALK_ABL & 4) && a.walk) return;
  double lp = 0.0, lr = 0.0;
  if (valid) {
    uint32_t R[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};   // D_0 = 0
    double lpu = a.lp_unseen;
    asm volatile("" : "+v"(lpu));
    const int64_t N = a.N, nwords = (N + 15) / 16;
    const size_t cstride = (size_t)a.nseq * 4;
    // the steps this unit runs: all of them, or (chunked) its chunk [t_sum, t_end) after
    // t_sum - t_begin warm-up steps from D = 0 whose sums it drops (every bound but N a multiple
    // of 192: whole 16-B stream chunks and six-step groups, the planes in layout phase 0)
    constexpr bool ck = kCk;
    int64_t t_begin = 0, t_sum = 0, t_end = N;
    if (ck) {
      t_sum = (int64_t)ck_j * a.ck_len;
      t_end = min(N, t_sum + (int64_t)a.ck_len);
      t_begin = max((int64_t)0, t_sum - (int64_t)a.ck_warm);
    }
    uint32_t c4[4];
    auto load_chunk = [&](int64_t ci) {
      const uint32_t* rb = a.r + (size_t)ci * cstride + (size_t)qwave * 4;
      const uint4 v = 4 * ci < nwords ? stream_load(reinterpret_cast<const uint4*>(rb + lane_id() * 4u))
                                      : make_uint4(0u, 0u, 0u, 0u);
      c4[0] = v.x; c4[1] = v.y; c4[2] = v.z; c4[3] = v.w;
    };
    auto pick = [&](int64_t wi) -> uint32_t {
      const uint32_t e = (uint32_t)wi & 3u;
      const uint32_t v = e == 0u ? c4[0] : e == 1u ? c4[1] : e == 2u ? c4[2] : c4[3];
      return wi < nwords ? v : 0u;
    };
    // the received words as a 64-bit window (words wi, wi + 1) and the bit offset of the
    // next step in it (< 32 at the top of a six-step group): one funnel shift per group,
    // one bit-field extract per step
    int64_t wi = t_begin / 16;
    load_chunk(wi >> 2);
    uint32_t cw = pick(wi), nw = pick(wi + 1);
    uint32_t sh = 0u;
    BsCursor cur;
    cur.start(a);
    if constexpr (!kBsOneLoad) cur.prefetch_row(a, cur.slot, word_param(cw & 3u));
    const double lt1 = a.ltref[1];   // (= s_lt[1]: the term of a wave-step without a suspect lane)
    // (rn: the next step's word, for the second load site.  With kBsOneLoad nothing reads it and
    // its extraction at the call sites emits nothing, but without those dead expressions the
    // compiler gives the pre-filter kernel's loop the same instructions with other registers in
    // another order; they stay, so that the loop is the one that was measured)
    auto step = [&](auto phc, uint32_t rr, uint32_t rn) {
      constexpr int PH = decltype(phc)::value;
      uint32_t Nn[2][4], c;
      bool one;
      bs_step<PH, kUni>(a, cur, R, rr, Nn, c, one);
      lp += cur.template resolve<PH>(a, R, rr, lpu);   // Pd_plotter.py:115, T = P̂1
      bs_lt_add(lr, s_lt, lt1, c, one);               // Pd_plotter.py:115, T = T_ref(1/2) = c / 2^n
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) R[r][i] = Nn[r][i];
      if constexpr (kBsOneLoad) cur.next();
      else cur.next_row(a, rn);
    };
    int64_t t = t_begin;
    int grp = 0, dec = 0;
    // word k / 2 of the group's window as the step's parameter: bits k, k + 1 of win sit at
    // k + 5, k + 6 of w5 = win << 5, so (w5 >> (k + 1)) & 0x30 = 16 r
    auto wk = [&](uint32_t w5, auto kc) -> uint32_t {
      constexpr uint32_t k = decltype(kc)::value;
      return (w5 >> (k + 1)) & 0x30u;
    };
    for (; t + 6 <= t_end; t += 6) {
      if (ck && t == t_sum) {   // (wave-uniform) the chunk's first summed step: D_t is its start
        ck_store(a, qwave, ck_j, 0u, R);
        lp = 0.0;
        lr = 0.0;
      }
      const uint32_t win = __builtin_amdgcn_alignbit(nw, cw, sh);
      const uint32_t w5 = win << 5;
      step(IntC<0>{}, wk(w5, IntC<0>{}), wk(w5, IntC<2>{}));
      step(IntC<1>{}, wk(w5, IntC<2>{}), wk(w5, IntC<4>{}));
      step(IntC<2>{}, wk(w5, IntC<4>{}), wk(w5, IntC<6>{}));
      step(IntC<3>{}, wk(w5, IntC<6>{}), wk(w5, IntC<8>{}));
      step(IntC<4>{}, wk(w5, IntC<8>{}), wk(w5, IntC<10>{}));
      step(IntC<5>{}, wk(w5, IntC<10>{}), wk(w5, IntC<12>{}));
      sh += 12u;
      if (sh >= 32u) {
        sh -= 32u;
        ++wi;
        cw = nw;
        nw = pick(wi + 1);
        if (((wi + 1) & 3) == 3) load_chunk((wi + 2) >> 2);   // the word after nw opens a chunk
      }
      if (a.early && ++grp == kBsEarlyGroups) {
        grp = 0;
        if (!dec) dec = early_decide(lp, lr, N - (t + 6), a.lt_min, a.lp_min);
        if (__ballot(dec == 0) == 0) {   // every lane decided: the wave is done
          t = N;
          break;
        }
      }
    }
    // last 1-5 steps
    if (t < t_end) {
      if (ck && t == t_sum) {   // (a last chunk of fewer than six steps)
        ck_store(a, qwave, ck_j, 0u, R);
        lp = 0.0;
        lr = 0.0;
      }
      const uint32_t win = __builtin_amdgcn_alignbit(nw, cw, sh);
      const uint32_t w5 = win << 5;
      step(IntC<0>{}, wk(w5, IntC<0>{}), wk(w5, IntC<2>{}));
      if (t + 1 < t_end) step(IntC<1>{}, wk(w5, IntC<2>{}), wk(w5, IntC<4>{}));
      if (t + 2 < t_end) step(IntC<2>{}, wk(w5, IntC<4>{}), wk(w5, IntC<6>{}));
      if (t + 3 < t_end) step(IntC<3>{}, wk(w5, IntC<6>{}), wk(w5, IntC<8>{}));
      if (t + 4 < t_end) step(IntC<4>{}, wk(w5, IntC<8>{}), wk(w5, IntC<10>{}));
    }
    if (ck) {   // the chunk's record: D at its end (phase 0 unless it is the last) and its sums
      ck_store(a, qwave, ck_j, 8u, R);
      uint32_t l = lane_id();
      asm volatile("" : "+v"(l));
      double* ps = reinterpret_cast<double*>(
          a.ck_out + ((size_t)ck_j * (size_t)a.nseq + (size_t)qwave + l) * kCkRecWords + 16u);
      ps[0] = lp;
      ps[1] = lr;
      return;   // (the decisions: ck_combine_kernel)
    }
    if (a.sums) {
      const int64_t qe = qwave + lane_id();
      a.sums[2 * qe] = lp;
      a.sums[2 * qe + 1] = lr;
    }
    early_final(dec, lp, lr);
  }
  if constexpr (kCk) return;
  count_decisions_masked(vmask, hmask, lp, lr, a.counts);
}

// The block's LDS tables, then its waves' sequences: by block index, or -- a.wq set, the
// persistent launch of cvd_kernels.hip (one block per resident slot) -- from a work queue,
// each wave taking the next 64 sequences until none are left, so that a CU's waves finish
// together whatever their lookups cost and the LDS tables are filled once per block
template <uint64_t XM>
__device__ __forceinline__ void k1s_body(const ExpArgs& a, uint32_t blk) {
  __shared__ double s_lt[5];
  if (threadIdx.x <= 4) s_lt[threadIdx.x] = a.ltref[threadIdx.x];
  fill_filter_patterns();
  fill_bs_etab<XM>();
#if CVD_K1B_LDSF
  {   // the whole filter, 2 (fmask + 1) words, into dynamic LDS
    uint4* d = reinterpret_cast<uint4*>(dyn_lds());
    const uint4* g = reinterpret_cast<const uint4*>(a.filt);
    for (uint32_t i = threadIdx.x; i < (a.fmask + 1u) / 2u; i += blockDim.x) d[i] = g[i];
  }
  if (a.t2c) {   // the compact walk records' value table, after the filter
    double* d = reinterpret_cast<double*>(reinterpret_cast<char*>(dyn_lds()) + a.vtab_off);
    for (int32_t i = (int32_t)threadIdx.x; i < a.nvtab; i += (int32_t)blockDim.x) d[i] = a.vtab[i];
  }
#elif CVD_K1S_PF
  {   // the pre-filter, 2^kBsPfLog2Bits bits, into dynamic LDS
    uint4* d = reinterpret_cast<uint4*>(dyn_lds());
    const uint4* g = reinterpret_cast<const uint4*>(a.pf);
    for (uint32_t i = threadIdx.x; i < (1u << (cvd::kBsPfLog2Bits - 7)); i += blockDim.x) d[i] = g[i];
  }
#endif
  __syncthreads();
  // every wave leaves once the queue is past the last unit (no block barrier below)
  // units: waves of 64 sequences; walk mode's H1 / H2 interleave (k1s_wave) permutes
  // [0, 2 ceil(units / 2)), whose last unit may hold no sequence
  uint32_t nunits = (uint32_t)((a.nseq + 63) / 64);   // < 2^32 (host: grid and queue limits)
  if (a.walk || (a.mix && a.ck_n <= 0)) nunits = (nunits + 1u) & ~1u;
  // chunked: ck_n units (time chunks) per wave of sequences (no walk mode)
  const uint32_t ckn = a.ck_n > 0 ? (uint32_t)a.ck_n : 1u;
  nunits *= ckn;
  auto take = [&]() -> uint32_t {
    uint32_t u = 0u;
    if (lane_id() == 0) u = atomicAdd(a.wq, 1u);
    return __builtin_amdgcn_readfirstlane(u);
  };
  uint32_t u = a.wq ? take() : blk * (uint32_t)(kK1bBlock / 64) + (__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6);
  while (u < nunits) {
    if (CVD_K1S_CK && a.ck_n > 0) k1s_wave<XM, true>(a, (int64_t)(u / ckn), s_lt, (int32_t)(u % ckn));
    else k1s_wave<XM>(a, (int64_t)u, s_lt);
    if (!a.wq) break;
    u = take();
  }
}

template <uint64_t XM>
__device__ __forceinline__ void k1s_multi(const MultiArgs& ma) {
  const uint32_t b = blockIdx.x;
  int i = 0;
  uint32_t b0 = 0u;
  while (i + 1 < ma.nm && b >= ma.blk_end[i]) b0 = ma.blk_end[i++];   // scalar: blockIdx is uniform
  k1s_body<XM>(ma.a[i], b - b0);
}

// the specialised kernel's entries (cvd_rtc.cpp): the butterfly kernel, or for m = 6 its
// bit-sliced form when the model's tables are the bit-sliced ones
template <int m, uint64_t XM>
__device__ __forceinline__ void k1b_spec_entry(const ExpArgs& a) {
  if constexpr (CVD_K1B_BITSLICE && m == 6) k1s_body<XM>(a, blockIdx.x);
  else k1b_body<m, true, XM, false>(a, blockIdx.x);
}
template <int m, uint64_t XM>
__device__ __forceinline__ void k1b_spec_multi_entry(const MultiArgs& ma) {
  if constexpr (CVD_K1B_BITSLICE && m == 6) k1s_multi<XM>(ma);
  else k1b_multi<m, XM>(ma);
}

}  // namespace cvd_dev
