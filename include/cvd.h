/*
 * cvd.h — C-ABI of the MI355X-native Monte-Carlo relative-Viterbi-metric
 * detector (libcvd.so).  Drop-in boundary for the reference's hot path:
 *
 *   reference (So-bonkers/Detecting-Convolutional-Codes-Via-Markovian-Statistics)   this ABI
 *   ───────────────────────────────────────────────────────────────────────────   ─────────────────────
 *   viterbi_markov.py:82-106  branch_output_and_next_state                         cvd_code_tables
 *   viterbi_markov.py:139-159 viterbi_metric_step (Eq. 4-5)                        cvd_metric_step (host), cvd_trace (GPU)
 *   viterbi_markov.py:166-195 enumerate_markov_states_allzero (BFS)                cvd_enumerate (host),
 *                                                                                  cvd_enumerate_device (GPU)
 *   viterbi_markov.py:202-230 + Pd_plotter.py:89-99  T(p) at p = 1/2              cvd_model_* (|Y(i,j)|/2^n, exact)
 *   Pd_plotter.py:123-169     learn_P1_empirical                                   cvd_model_create (host chain),
 *                                                                                  cvd_model_create_device (GPU chain)
 *   viterbi_markov.simulate_markov_sequence (MISSING; called Pd_plotter.py:149,212,219)
 *                                                                                  cvd_generate (+ cvd_trace)
 *   Pd_plotter.py:106-116     log_prob_sequence                                    cvd_detect (per-sequence sums)
 *   Pd_plotter.py:198-233     trial loop, decision, Pd/Pc counting                 cvd_detect (counts) / cvd_mc_run /
 *                                                                                  cvd_mc_fused (generator + table in one kernel)
 *   (none: the reference is single-process)                                        cvd_allreduce_counts / cvd_comm_* (RCCL)
 *   comp_parity.py:90-128     parity_satisfaction_fraction / parity_detector       cvd_parity_detect
 *                             (parity-template baseline)
 *   (none: the reference detects only streams it simulated)                        cvd_pack_windows
 *                             (a captured serial bitstream cut into windows in cvd_generate's layout)
 *   (none: the reference's templates come from known generators)                   cvd_parity_sweep
 *                             (all 2^B parity templates of a capture at once: histogram + WHT)
 *   (none: the reference keeps no survivor decisions, viterbi_markov.py:139-159)   cvd_viterbi_decode
 *                             (hard-decision Viterbi decoder of a capture: bits, error count, end states)
 *   (none: the reference's channel is a BSC, viterbi_markov.py:139-159)            cvd_viterbi_decode_soft,
 *                             (the same decoder over int8 confidence values, 0 = erased) cvd_soft_depuncture
 *   alpha_exponent.py:83-156  learn_transition_tensor (joint counts)              cvd_count_transitions
 *   alpha_exponent.py:159-188 compute_error_exponent: M(u) for a u grid           cvd_chernoff_build(_dense)
 *   alpha_exponent.py:69-76   spectral_radius (Perron root of M(u) >= 0)           cvd_spectral_radius
 *                             (error-exponent engine)
 *
 * Conventions:
 *   - every function returns 0 on success, a negative CVD_E* code on error;
 *     cvd_last_error() returns a thread-local message; no C++ exception crosses the ABI;
 *   - buffers are caller-owned; pointers named d_* are device pointers (HIP),
 *     `stream` is a hipStream_t (NULL = default stream); launches are async;
 *   - host tables are copied in at cvd_model_create / cvd_model_upload;
 *   - generator taps use the reference layout taps[j][i][d] (output j, input i,
 *     delay d = 0..m; d = 0 multiplies the current input bit), flattened row-major.
 */
#ifndef CVD_H
#define CVD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVD_ABI_VERSION 11

#define CVD_OK 0
#define CVD_E_INVALID -1      /* bad argument */
#define CVD_E_UNSUPPORTED -2  /* code shape not supported by the requested path */
#define CVD_E_CAPACITY -3     /* enumeration cap hit / table too large */
#define CVD_E_HIP -4          /* HIP runtime error */
#define CVD_E_STATE -5        /* state not in the model's index (reference: KeyError) */

typedef struct cvd_code {
  int32_t k, n, m;         /* inputs, outputs, memory */
  const uint8_t* taps;     /* [n][k][m+1] delay-ordered taps */
} cvd_code;

typedef struct cvd_learn_params {
  double p;                /* BSC crossover of the learning chain */
  int64_t learn_len;       /* < 0: None -> max(5000, 200*S) (Pd_plotter.py:143-146);
                              non-enumerable codes: default_learn_len */
  int64_t learn_burn;      /* Pd_plotter.py:72 default 200 */
  double laplace;          /* Pd_plotter.py:73 default 1.0 */
  uint64_t seed;           /* learning-chain seed (Pd_plotter.py:70 default 12345) */
  int64_t enum_cap;        /* BFS cap; above it the model is sparse (learned states only) */
  int64_t default_learn_len; /* learn length for non-enumerable codes when learn_len < 0 */
  int64_t laplace_states;  /* non-enumerable codes: > 0 = the S of the Laplace denominator S*laplace
                              (Pd_plotter.py:166-167), e.g. a count or certified lower bound from
                              cvd_enumerate_device, >= the visited rows; <= 0 = the visited rows
                              (DESIGN.md D4).  Enumerable codes: <= 0 or the BFS count S. */
} cvd_learn_params;

typedef struct cvd_model_info {
  int32_t kind;            /* 0 = dense (BFS-enumerated, reference-exact), 1 = sparse (learned states) */
  int32_t k, n, m;
  int64_t S;               /* states in the Laplace denominator (BFS count, or learned count) */
  int64_t n_rows;          /* rows held in the device table */
  int64_t learn_len_eff;   /* learning chain length actually used */
  int64_t hash_capacity;   /* explicit-path hash slots (0 if none) */
  int32_t max_probe;       /* longest probe sequence in the hash */
  int32_t device;          /* device holding the tables, -1 if not uploaded */
  double logp1_unseen;     /* log P̂1 of a row never visited (sparse models) */
  int32_t explicit_kernel; /* kernel CVD_PATH_EXPLICIT launches: CVD_KERNEL_* */
  int32_t mc_fused;        /* 1: cvd_mc_run (CVD_PATH_AUTO) runs the fused generator + table kernel
                              (cvd_mc_fused) for this model: an LDS-resident table small enough for
                              256-thread blocks (measured faster there; the 1024-thread variant of the
                              large tables is slower than the two-kernel pipeline) */
  int32_t walk;            /* 1: the specialised m = 6 kernel runs this model's H1 waves in walk mode
                              (learned-row steps from the row records, no ACS; sums unchanged): the
                              model's rows / learn_len < 1/20 (bit-sliced kernel; 1/10 butterfly
                              kernel), i.e. H1 stays in learned rows (CVD_WALK overrides; traces and,
                              unless CVD_WALK=1, counts-only early decision run lockstep) */
  int32_t lds_filter;      /* 1: the specialised kernel keeps this model's whole Bloom filter in LDS
                              (walking models of <= 32,768 rows: 128 KiB in 1,024-thread blocks for the
                              bit-sliced kernel, 64 KiB in 512-thread blocks for the butterfly kernel;
                              CVD_NO_LDSF=1 keeps it in global memory) */
  int32_t walk_compact;    /* 1: the walk reads 8-B two-step records whose log P̂1 values come from a
                              table in LDS beside the filter (built with CVD_WALK_T2C=1 where rows <
                              2^16, <= 4,096 distinct values and room in LDS; same sums, measured
                              neutral, off by default) */
  int64_t multi_variant;   /* nonzero: the specialised kernel variant this model runs in a
                              cvd_detect_multi launch; consecutive models with equal nonzero values
                              share one launch (at most 8), except a model whose own launch would be
                              persistent (persist_seqs below).  0: the model is detected on its own */
  int64_t persist_seqs;    /* > 0: a launch of this model over more sequences than this (the bit-
                              sliced kernel's resident capacity) is persistent -- one block per
                              resident slot, waves taking 64 sequences at a time from a work queue
                              -- and cvd_detect_multi launches it on its own (ABI 10).  0: never */
} cvd_model_info;

#define CVD_KERNEL_NONE 0       /* explicit path unsupported for this shape */
#define CVD_KERNEL_GENERIC 1    /* detect_explicit_kernel<m,k,n>: ACS for every received word */
#define CVD_KERNEL_ORBIT 2      /* detect_k1_kernel<m,n>: k = 1, ACS for the 2^n/2 orbit representatives */
#define CVD_KERNEL_BUTTERFLY 3  /* detect_k1b_kernel<m>: k = 1, n = 2 standard butterflies, one ACS vector */
#define CVD_KERNEL_BUTTERFLY_RTC 4  /* the same, specialised to the decoder code at model upload (JIT, cvd_rtc.cpp) */
#define CVD_KERNEL_BITSLICE_RTC 5   /* m = 6: its bit-sliced form (k1s, cvd_k1s.h: four bit-planes of two words
                                       per lane, the row tables keyed by a canonical digest; same sums) */

typedef struct cvd_model cvd_model;

/* ---- version / errors ---------------------------------------------------- */
int cvd_version(void);
const char* cvd_last_error(void);

/* Stream tag of the (N, p) grid point (the trial streams' Philox counter word 3). */
#define CVD_LEARN_TAG 0xC0DE1EA7u
uint32_t cvd_grid_tag(int64_t N, double p);

/* ---- host-side code algebra (no GPU needed) --------------------------------
 * out_sym[s*2^k + U] = output word (bit j = output j), next_state[s*2^k + U];
 * U = sum_i u_i << i.                                  (viterbi_markov.py:82-106) */
int cvd_code_tables(const cvd_code* code, int32_t* out_sym, int32_t* next_state);

/* One Eq. 4-5 step on the host, D as 2^m bytes.          (viterbi_markov.py:139-159) */
int cvd_metric_step(const cvd_code* dec, const uint8_t* D_prev, int32_t r, uint8_t* D_out);

/* BFS over relative-metric states from D_0 = 0 (viterbi_markov.py:166-195).
 * Writes S; if states_out != NULL it receives [min(S,cap)][2^m] bytes in discovery
 * order; if next_out != NULL, next_out[i*2^n + r] = index of the successor.
 * Returns CVD_E_CAPACITY if more than `cap` states exist. */
int cvd_enumerate(const cvd_code* dec, int64_t cap, int64_t* S_out,
                  uint8_t* states_out, int32_t* next_out);

/* The same BFS on GPU `device` (for codes past the host
 * BFS, (133,171) > 2e8 states): level-synchronous over a hash set in HBM, states in
 * the reference's discovery order (a level's new states ranked by their first
 * (parent, received word) in itertools.product order).  Same outputs as
 * cvd_enumerate (states_out / next_out nullable), plus level_sizes[l] = states
 * first reached after l steps (nullable, max_levels entries; n_levels_out the
 * number of levels).  mem_bytes: device memory budget (<= 0: 90% of free).
 * CVD_E_CAPACITY when S > cap or the budget cannot hold the search: S_out is then
 * a certified lower bound (distinct reachable states found) and the level sizes
 * describe the levels reached.  Synchronous. */
int cvd_enumerate_device(const cvd_code* dec, int32_t device, int64_t cap, int64_t mem_bytes, int64_t* S_out,
                         uint8_t* states_out, int32_t* next_out, int64_t* level_sizes, int32_t max_levels,
                         int32_t* n_levels_out, void* stream);

/* ---- model: decoder trellis + learned P̂1 + T_ref(1/2) ------------------------ */
int cvd_model_create(const cvd_code* dec, const cvd_learn_params* prm, cvd_model** out);
/* The same model with the learning chain (Pd_plotter.py:143-163) run on GPU `device`
 * (parallel in time: speculative blocks verified at their boundaries, first visits
 * by a radix sort of key hashes; see cvd_learn.hip).  Bit-identical to
 * cvd_model_create.  stats_out (nullable) [7]: seconds, mismatched speculative
 * blocks, re-run passes, blocks re-run sequentially, hash/sort attempts,
 * host fallback (1: the GPU chain refused the code shape, the chain length
 * (>= 2^31) or ran out of device memory for its scratch, and the host chain
 * built the model -- identical results), seconds of the sequential tail.
 * Synchronous; `stream` orders the device work (NULL = default stream). */
int cvd_model_create_device(const cvd_code* dec, const cvd_learn_params* prm, int32_t device, void* stream,
                            cvd_model** out, double* stats_out);
int cvd_model_info_get(const cvd_model* model, cvd_model_info* info);
/* Dense models: the S x S P̂1 matrix exactly as Pd_plotter.py:166-167 builds it. */
int cvd_model_dense_P1(const cvd_model* model, double* P_out, int64_t S);
/* Per-row tables (host copies): logP1[row*2^n + r]; keys[row][2^m] metric bytes. */
int cvd_model_rows(const cvd_model* model, double* logp1_out, uint8_t* keys_out, int64_t n_rows);
/* The decoder code of a model (e.g. one loaded from a file): taps_out receives
 * [n][k][m+1] delay-ordered taps (cvd_code layout); len = its size in bytes. */
int cvd_model_taps(const cvd_model* model, uint8_t* taps_out, int64_t len);
int cvd_model_upload(cvd_model* model, int device);
/* The code-specialised detector kernel (CVD_KERNEL_BUTTERFLY_RTC) of an uploaded
 * model: 1 = built, -1 = unavailable (msg_out receives the compiler's reason, the
 * table-driven kernel runs instead with the same results), 0 = not applicable. */
int cvd_model_jit_status(const cvd_model* model, char* msg_out, int64_t msg_len);
void cvd_model_destroy(cvd_model* model);
/* On-disk model cache (the reference memoises P̂1 per learning key with
 * @lru_cache, Pd_plotter.py:123-127; this makes it persistent): save writes the
 * learned rows atomically (tmp + rename); load rebuilds the model (host tables;
 * upload it before use).  Files carry this build's ABI version. */
int cvd_model_save(const cvd_model* model, const char* path);
int cvd_model_load(const char* path, cvd_model** out);

/* ---- device work ---------------------------------------------------------- */
/* Encoder (enc) -> BSC(p) received words for sequences q0..q0+count-1 of an
 * interleaved buffer; sequence q uses
 * seq_id = seq_base + (q - q0) * seq_stride.  Spec of the missing
 * simulate_markov_sequence.  Layout: W = ceil(N / floor(32/n)) words per
 * sequence, step i of a word in bits [n*i, n*i+n); words grouped in 16-byte
 * chunks: word w of sequence q at d_r[((w/4)*pitch + q)*4 + w%4] (16-B aligned);
 * d_r holds ceil(W/4)*4*pitch words. */
int cvd_generate(const cvd_code* enc, uint64_t seed, uint32_t tag, double p, int64_t N,
                 int32_t random_input, int64_t seq_base, int64_t seq_stride,
                 uint32_t* d_r, int64_t pitch, int64_t q0, int64_t count, void* stream);

/* Captured bitstream -> received-word buffer: the way in for streams cvd_generate did not
 * make (a demodulator's hard decisions; nothing in the reference, whose streams all come
 * from its own simulator).  The capture is the serial channel stream in device memory:
 * relative to a window's first bit, bit n*t + j is output j of step t.  Window i, phase f
 * (0 <= f < n_phase <= n: the candidate symbol phases) begins at capture bit
 * start + i*stride + f, holds N steps (N*n bits) and becomes sequence
 * q = q0 + i*n_phase + f of d_r in exactly cvd_generate's layout: W = ceil(N / floor(32/n))
 * words, step t in bits [n*(t % SPW), +n) of word t / SPW (SPW = floor(32/n)), word w at
 * d_r[((w/4)*pitch + q)*4 + w%4]; the bits of the last word past step N and the padding
 * words up to a multiple of 4 are zero.  Columns of d_r outside [q0, q0 + nwin*n_phase) are
 * not written.  stride: any positive number of bits (stride < N*n: overlapping windows).
 * Bit b of the capture, by format: */
#define CVD_CAPTURE_LSB   0  /* bit b of the capture = bit (b & 7) of byte b >> 3 */
#define CVD_CAPTURE_MSB   1  /* bit b = bit 7 - (b & 7) of byte b >> 3 (numpy.packbits default) */
#define CVD_CAPTURE_BYTES 2  /* one bit per byte: bit b = byte[b] & 1 */
/* d_capture (and d_r) 16-byte aligned; the capture readable up to its byte length
 * (ceil(nbits/8), or nbits for CVD_CAPTURE_BYTES) rounded up to 16: the kernel never reads
 * at or past that, and bits at index >= nbits never reach the output.  Bit positions are
 * 64-bit throughout (a capture may exceed 2^32 bits).  CVD_E_INVALID, without touching the
 * device, for: n outside 1..3, n_phase outside 1..n, N < 0, start < 0, stride <= 0,
 * nwin < 0, an unknown format, q0 < 0, pitch < q0 + nwin*n_phase, a window not entirely
 * inside [0, nbits), or any of these products overflowing int64.  nwin == 0 or N == 0:
 * CVD_OK without a launch.  Asynchronous on `stream`, like cvd_generate. */
int cvd_pack_windows(const void* d_capture, int64_t nbits, int32_t format,
                     int32_t n, int64_t N,
                     int64_t start, int64_t stride, int64_t nwin, int32_t n_phase,
                     uint32_t* d_r, int64_t pitch, int64_t q0, void* stream);

#define CVD_PATH_AUTO 0
#define CVD_PATH_TABLE 1    /* enumerated state automaton (dense models) */
#define CVD_PATH_EXPLICIT 2  /* explicit 2^m metric vector + hashed P̂1 rows (fastest k=1 kernel that applies) */
#define CVD_PATH_EXPLICIT_GENERIC 3  /* explicit path, ACS for every received word (no orbit reduction) */
#define CVD_PATH_EXPLICIT_ORBIT 4    /* explicit path, k=1 two-representative orbit kernel */
#define CVD_PATH_EXPLICIT_BUTTERFLY 5  /* explicit path, k=1 n=2 butterfly kernel, table-driven (not code-specialised) */
/* OR'ed into `path` (cvd_detect, cvd_mc_run): early decision.  A trial's decision
 * (Pd_plotter.py:215, :222) compares only its final sums; every log P̂1 and log T_ref
 * increment lies in [min, 0], so once the running sums are far enough apart the
 * outcome is certain (with a rigorous IEEE rounding margin) and a wavefront whose
 * lanes have all decided stops.  Counts are identical to the full run; per-trial
 * sums are then not produced (d_sums must be NULL). */
#define CVD_DETECT_EARLY_DECISION 0x100

/* Detector over sequences 0..nseq-1 (pitch = nseq): per sequence the sequential
 * fp64 sums log P̂1(D_0^N) and log T_ref(D_0^N) (Pd_plotter.py:106-116); sequences
 * q < n_h1 are H1 streams (success iff logp1 > logref), the rest H2 streams
 * (success iff logp1 <= logref) (Pd_plotter.py:215-223).  d_counts[0] += H1
 * successes, d_counts[1] += H2 successes (int64, accumulated, not cleared).
 * d_sums (nullable): [nseq][2] doubles.
 * A launch of the bit-sliced kernel past cvd_model_info.persist_seqs is persistent: its
 * waves take their sequences from a work-queue counter the call allocates, zeroes and frees
 * on `stream` (stream-ordered, so launches on any number of streams never share one).
 * Chunked launches (counts only: d_sums NULL, no early decision; the bit-sliced kernel): a
 * batch too small to fill the device twice -- the reference's own call shape, e.g. 10,000
 * trials per p -- has every sequence's N steps cut into C time chunks of L steps, each
 * started on a lane of its own W steps early from D = 0 and kept only where the chunks
 * join (D at a chunk's start equals the previous chunk's D at its end) and the decision is
 * certain under the rounding bounds of both summation orders; every other sequence is rerun
 * on the sequential kernel, so the counts equal the unchunked launch's exactly.  Such a
 * call synchronises `stream` once (the rerun list).  CVD_CHUNK=0 disables it, =1 forces it
 * wherever C >= 2; CVD_CHUNK_WARM (1152 steps) and CVD_CHUNK_UNITS set W and the target lane
 * count. */
int cvd_detect(const cvd_model* model, const uint32_t* d_r, int64_t N, int64_t nseq,
               int64_t n_h1, double* d_sums, int64_t* d_counts, int32_t path, void* stream);

/* nm cvd_detect calls in as few launches as possible (a p sweep: one model per p, one
 * stream buffer each; Pd_plotter.py:199-233).  Model i reads d_r[i] (nseq[i] sequences,
 * the first n_h1[i] of them H1) and accumulates d_counts[i][2] (and d_sums[i] when d_sums
 * and d_sums[i] are non-NULL), all with the same N.  Consecutive models that share the
 * code-specialised kernel variant (CVD_KERNEL_BUTTERFLY_RTC: same decoder, block size
 * and filter placement) run in ONE launch, up to 8 per launch, block ranges in model
 * order, so the step pays one last-round tail instead of one per model; others run as
 * cvd_detect.  Results equal the separate calls exactly.  path: CVD_PATH_AUTO or
 * CVD_PATH_EXPLICIT (merged), any other path launches one model at a time; OR
 * CVD_DETECT_EARLY_DECISION as in cvd_detect.  CVD_NO_MULTI=1 disables merging. */
int cvd_detect_multi(const cvd_model* const* models, int32_t nm, const uint32_t* const* d_r, int64_t N,
                     const int64_t* nseq, const int64_t* n_h1, double* const* d_sums, int64_t* const* d_counts,
                     int32_t path, void* stream);

/* Metric trace on the explicit path: d_D[(t*nseq + q)*2^m + s] = D_t(s), t = 0..N. */
int cvd_trace(const cvd_model* model, const uint32_t* d_r, int64_t N, int64_t nseq,
              uint8_t* d_D, void* stream);

/* One (N, p) grid point over global trials [trial_begin, trial_end): generates
 * H1 (enc1) and H2 (enc2) streams in batches of `batch` trials into the caller's
 * workspace d_work (cvd_mc_workspace_bytes) and accumulates d_counts[2]. */
int64_t cvd_mc_workspace_bytes(const cvd_code* enc1, int64_t N, int64_t batch);
int cvd_mc_run(const cvd_model* model, const cvd_code* enc1, const cvd_code* enc2,
               double p, int64_t N, uint64_t seed, int64_t trial_begin, int64_t trial_end,
               int64_t batch, void* d_work, int64_t* d_counts, int32_t path, void* stream);

/* cvd_mc_run: d_work may be NULL when the call runs the fused kernel below (CVD_PATH_AUTO
 * and cvd_model_info.mc_fused); otherwise it returns CVD_E_INVALID without it.  The fused
 * path launches at most 2^28 trials per kernel (HIP grid limit), in slices. */

/* The whole (N, p) grid of Pd_plotter.py:196-233 in one call: N outer,
 * p inner, the global trials [trial_begin, trial_end) at every point (the reference's
 * num_iter per point; a shard of them under trial sharding), with models[i] the model
 * learned at p[i] (learn_P1_empirical is per p, Pd_plotter.py:123-169).  Point
 * (N[j], p[i]) accumulates into d_counts[(j*np + i)*2 + {0: H1, 1: H2}] -- the
 * [nN][np][2] count tensor cvd_allreduce_counts reduces -- exactly the counts np * nN
 * cvd_mc_run calls give.  The p row of one N runs batch by batch: every point's streams
 * are generated into its own workspace slot, then one cvd_detect_multi detects the row
 * (the models sharing the specialised kernel variant in one launch, so a row of small
 * batches -- the reference's num_iter = 10,000 per point -- pays one last-round tail,
 * not one per p); points whose model runs the fused kernel (CVD_PATH_AUTO, mc_fused)
 * run it without a slot.  d_work: cvd_mc_grid_workspace_bytes (one slot of the largest
 * N's batch per non-fused point; 0 = NULL allowed when every point runs fused). */
int64_t cvd_mc_grid_workspace_bytes(const cvd_model* const* models, int32_t np, const cvd_code* enc1,
                                    const int64_t* N, int32_t nN, int64_t batch, int32_t path);
int cvd_mc_run_grid(const cvd_model* const* models, const cvd_code* enc1, const cvd_code* enc2,
                    const double* p, int32_t np, const int64_t* N, int32_t nN, uint64_t seed,
                    int64_t trial_begin, int64_t trial_end, int64_t batch, void* d_work,
                    int64_t* d_counts, int32_t path, void* stream);

/* Kernel error flags of a model's launches since the last call (synchronises its
 * device): bit 0 = a walk-mode wave (k1b_walk) left its scheduler loop by the guard
 * bound with lanes unfinished, so that launch's counts and sums are void.  Returns
 * CVD_E_STATE when any flag is set (then cleared), CVD_OK otherwise.  cvd_detect,
 * cvd_detect_multi, cvd_mc_run and cvd_mc_run_grid do not synchronise, so they cannot
 * report it: a caller checks it once after its launches (the Python host does after
 * run_trials with sums, run_grid, detect_multi's callers, run_experiment and the bench). */
int cvd_model_device_error(cvd_model* model, int32_t* flags_out);

/* The chunked launches of this process's last cvd_detect / cvd_detect_multi call (cvd_mc_run
 * and cvd_mc_run_grid make such calls per batch): out[0] chunked launch groups (0: none),
 * out[1] chunks per sequence C, out[2] steps per chunk L, out[3] sequences the decisions
 * left to the sequential rerun.  Diagnostic (tests, bench); not thread-safe. */
int cvd_chunk_last(int64_t* out4);

/* Compile the code-specialised detector's default variants for decoder `dec` and GPU
 * architecture `arch` (e.g. "gfx950") into `dir` without a device: the prebuilt cache that
 * model upload reads before compiling (its default: <directory of libcvd.so>/jit;
 * CVD_JIT_PREBUILT=off skips it).  Only the bit-sliced codes (m = 6, k = 1, n = 2 standard
 * butterflies) have variants to build; *n_built = how many were built or found. */
int cvd_jit_prebuild(const cvd_code* dec, const char* arch, const char* dir, int32_t* n_built);
/* The same for the variants with walk mode compiled in, which a bit-sliced model's launch runs
 * only when walk mode is forced on (CVD_WALK=1; the default variants leave it out, so that the
 * lockstep kernel keeps the lockstep loop's register count). */
int cvd_jit_prebuild_walk(const cvd_code* dec, const char* arch, const char* dir, int32_t* n_built);

/* The same grid point in ONE kernel per launch, without streams in HBM: every lane
 * generates its own sequence's received words (cvd_generate's encoder and noise, bit
 * for bit) and runs the LDS-resident table automaton on them (dense models with
 * S < 4096 whose tables fit a CU's LDS; (k, n) in {(1,2), (1,3), (2,3)}; otherwise
 * CVD_E_UNSUPPORTED).  Trial t of [trial_begin, trial_end) is sequences 2t (H1, enc1)
 * and 2t + 1 (H2, enc2) as in cvd_mc_run, which uses this path for CVD_PATH_AUTO
 * when it applies.  d_sums (nullable): [trial_end - trial_begin][4] doubles (log P̂1,
 * log T_ref of H1, then of H2).  flags: CVD_DETECT_EARLY_DECISION (counts only). */
int cvd_mc_fused(const cvd_model* model, const cvd_code* enc1, const cvd_code* enc2, double p, int64_t N,
                 uint64_t seed, int64_t trial_begin, int64_t trial_end, double* d_sums, int64_t* d_counts,
                 int32_t flags, void* stream);

/* ---- multi-GPU: the one collective (none in the reference,
 * Pd_plotter.py:176-235 is single-process) --------------------------------
 * Sum-reduce the int64 success counts of a trial-sharded run over RCCL (xGMI).
 * Shard the global trial range [0, num_iter) of every (N, p) grid point over the
 * GPUs, run cvd_mc_run per shard into a per-device count buffer, reduce: every
 * buffer then holds the single-process counts (streams are keyed by the global
 * trial id).  Enqueued on the given streams (async; the caller synchronises).
 *
 * One process, ndev devices: d_counts[i] on devices[i], ordered after streams[i]
 * (streams NULL or streams[i] NULL = that device's default stream).  The
 * communicators are created on first use of a device list and cached. */
int cvd_allreduce_counts(int64_t* const* d_counts, int64_t len, int32_t ndev, const int32_t* devices,
                         void* const* streams);
/* One process per GPU: rank 0 calls cvd_comm_unique_id and hands the 128 bytes to
 * every rank (any channel); each rank calls cvd_comm_init with its device. */
#define CVD_COMM_ID_BYTES 128
typedef struct cvd_comm cvd_comm;
int cvd_comm_unique_id(uint8_t* id_out /* [CVD_COMM_ID_BYTES] */);
int cvd_comm_init(const uint8_t* id, int32_t nranks, int32_t rank, int32_t device, cvd_comm** out);
int cvd_comm_allreduce_counts(cvd_comm* comm, int64_t* d_counts, int64_t len, void* stream);
void cvd_comm_destroy(cvd_comm* comm);

/* ---- parity-template baseline (comp_parity.py, parity_eqn_check.py) --------
 * Per sequence q of a received-word buffer (pitch = nseq, layout as above):
 *   sat = #{t in [max_s, N) : XOR_{(j,s) in terms} y_j[t - s] == 0}
 * with y_j[t] = bit j of step t (comp_parity.py:90-117: anchors from the
 * template's largest delay max_s), P̂ = sat / (N - max_s), 0.0 without anchors.
 * Sequences q < n_h1 succeed iff P̂ >= gamma (decide H1), the rest iff P̂ < gamma
 * (comp_parity.py:120-128); d_counts[2] accumulated as in cvd_detect.
 * terms: [n_terms][2] (output j, delay s), 1 <= n <= 3, 1 <= n_terms <= 96, every term
 * with 0 <= j < n and s >= 0.  A term lies o = n*s - j stream bits behind its anchor's
 * bit, and the kernel keeps 64 bits of history:
 *   n <= 2: o <= 64 (n = 1: s <= 64; n = 2: s <= 32).  The terms fall in three groups by
 *           the word pair they are read from: o <= 0 (the anchor's own word: (0, 0), and
 *           (1, 0) for n = 2), 1 <= o <= 32, and 33 <= o <= 64.  A third term with o <= 0
 *           and a 33rd term in either of the other groups are refused (only a template
 *           with repeated terms can have them).
 *   n = 3:  s <= 54, and at most 32 terms per output.
 * Repeated terms that pass these limits cancel in the XOR, as in the reference; max_s is
 * over all terms given.  CVD_E_INVALID, without a launch, for anything outside these
 * limits.  d_sat (nullable): [nseq] int32 satisfied counts. */
int cvd_parity_detect(const uint32_t* d_r, int32_t n, int64_t N, int64_t nseq, int64_t n_h1,
                      const int32_t* terms, int32_t n_terms, double gamma, int32_t* d_sat,
                      int64_t* d_counts, void* stream);

/* ---- blind parity-check sweep of a capture (nothing in the reference) --------
 * Which parity checks does a captured stream satisfy, and at which symbol phase?  Every
 * one of the 2^B templates over a window of span + 1 symbols, B = n*(span+1), is tested at
 * once: one histogram of the B-bit words the window sees and one Walsh-Hadamard transform,
 *   sat[mask] = (T + sum_x hist[x] * (-1)^popcount(mask & x)) / 2.
 * The capture, `format`, the alignment and 16-byte readability rule of d_capture and the
 * 64-bit bit positions are exactly those of cvd_pack_windows.  1 <= B <= 22.  Anchor a
 * (0 <= a < T) at phase f (0 <= f < n_phase <= n) has the word x whose bit i (i < B) is
 * capture bit start + f + n*a + i: bit n*e + j of x is output j of symbol a + e, and the
 * template term (output j, delay s) of cvd_parity_detect is mask bit n*(span - s) + j.
 *   d_sat[f*2^B + mask] += #{a : popcount(mask & x) even}      (int64 [n_phase][2^B])
 * accumulated, not cleared, like d_counts: sat[f][0] grows by T, and two calls over
 * adjacent anchor ranges equal one call over both.  Integer only: the result does not
 * depend on launch shape or on the order atomics arrive in.  d_work: the histogram
 * workspace, cvd_parity_sweep_workspace_bytes(n, span, n_phase) bytes (n_phase * 2^B * 4;
 * < 0 with the error set for an invalid shape), 16-byte aligned; the call zeroes it on
 * `stream`.  d_sat 8-byte aligned.  Asynchronous on `stream`.
 * CVD_E_INVALID, before the device is touched, for: n outside 1..3, span < 0, B > 22,
 * n_phase outside 1..n, T < 0 or T > 2^31 - 1, start < 0, nbits < 0, an unknown format,
 * the last word not inside [0, nbits) (start + (n_phase-1) + n*(T-1) + B > nbits), an
 * int64 overflow in these products, and null or misaligned pointers when T > 0.
 * T == 0: CVD_OK without a launch.  The block-local histogram lives in LDS up to B = 15
 * and the transform of a phase then runs in one block; B = 16..21 counts 2^15-bin parts of
 * the histogram in LDS, B = 22 uses global atomics, both with a two-pass tiled transform
 * (csrc/cvd_sweep.hip; CVD_SWEEP_GLOBAL_B = the smallest B on global
 * atomics, >= 16, for A/B runs: the result is the same). */
int64_t cvd_parity_sweep_workspace_bytes(int32_t n, int32_t span, int32_t n_phase);
int cvd_parity_sweep(const void* d_capture, int64_t nbits, int32_t format, int32_t n, int32_t span,
                     int64_t start, int64_t T, int32_t n_phase, int64_t* d_sat, void* d_work,
                     void* stream);

/* ---- hard-decision Viterbi decoder of a capture (nothing in the reference) ----
 * What was sent?  The Eq. 4-5 recursion (cvd_metric_step) with its survivor decisions kept:
 * the information bits of the maximum-likelihood path, its Hamming distance to the capture
 * (errors / (n*T) estimates the channel's crossover probability, the p that scan needs) and
 * its end states.  Exact: the result is the sequential decoder's stated here, bit for bit,
 * and does not depend on block, warm, depth or the launch shape.
 *
 * Code shapes: k = 1, n in {2, 3}, 1 <= m <= 8; anything else CVD_E_UNSUPPORTED.
 * Capture: read exactly as cvd_pack_windows reads it (CVD_CAPTURE_*, the same 16-byte
 * alignment and readability rule, 64-bit bit positions); capture bit start + n*t + j is
 * output j of step t, 0 <= t < T; y_t is the received n-bit word of step t.
 * States and branches (viterbi_markov.py:60-106): bit 0 of a state is the most recent input;
 * the branch from state s with input u goes to ((s << 1) | u) & (2^m - 1), and its output j is
 * taps[j][0][0]*u ^ sum_{d>=1} taps[j][0][d]*bit_{d-1}(s).
 * Forward (Eq. 4-5 with the decisions recorded): D_0(s) = 0 for every s.  For step t and
 * next state s', u = s' & 1 and ps_b = (s' >> 1) | (b << (m-1)), b in {0, 1}:
 *   D'(s') = min_b [D_t(ps_b) + d_H(out(ps_b, u), y_t)],
 *   dec_t(s') = 1 iff b = 1 is strictly smaller (ties keep b = 0: the reference's
 *   `val < best` in trellis order, viterbi_markov.py:150-156),
 *   D_{t+1} = D' - min D'.                       (relative metrics fit a byte: D <= n*m <= 24)
 * End and traceback: s_T is the lowest-index state with D_T = 0; for t = T-1 ... 0:
 *   u_t = s_{t+1} & 1,  s_t = (s_{t+1} >> 1) | (dec_t(s_{t+1}) << (m-1));
 *   errors = sum_t d_H(out(s_t, u_t), y_t).
 *
 * d_bits: ceil(T/32) words, bit t = u_t LSB first (as bytes on this little-endian target a
 * CVD_CAPTURE_LSB capture of T bits: it can go back into cvd_parity_sweep, e.g. for an outer
 * code); the bits of the last word at or past T are zero.  4-byte aligned.
 * d_stats: int64[9], written (not accumulated), 8-byte aligned:
 *   [0] errors  [1] number of blocks  [2] forward reruns  [3] traceback fix-ups
 *   [4] s_0  [5] s_T  [6] resolved block  [7] resolved warm  [8] resolved depth
 * block = L: a multiple of 32, at least 32 (a block owns whole output words); 0 = default.
 * warm = W >= 0, depth = D >= 0; -1 = default.  Defaults (measured): */
#define CVD_VITERBI_BLOCK 4096
#define CVD_VITERBI_WARM(m) (64 * (m))
#define CVD_VITERBI_DEPTH(m) (24 * ((m) + 2))
/* The counters are part of the contract (a test can prove which path ran):
 *   block b covers steps [b*L, min(T, (b+1)*L)); its warm vector is the relative metric
 *   vector at step b*L of a recursion started from all zeros at step max(0, b*L - W);
 *   stats[2] = #{b >= 1 : warm vector != the true D_{b*L}} (each such block is run again
 *   from the true vector);
 *   with e_b = min(T, (b+1)*L + D): if e_b = T block b traces from the true s_T and is
 *   certified; otherwise it is certified iff the survivors of all 2^m states at step e_b
 *   (true decisions) pass through one single state at step (b+1)*L;
 *   stats[3] = #{uncertified blocks} (each traced again, in descending order, from the start
 *   state of the block after it).
 * d_work: cvd_viterbi_workspace_bytes(n, m, T, block) bytes, 16-byte aligned: per step
 * max(8, 2^m / 8) bytes of decision words (blocks rounded up to L steps), per block two
 * metric vectors and a few words (< 0 with the error set for n, m outside the shapes above,
 * T < 0 or > 2^31 - 1, or a bad block).  Asynchronous on `stream`.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming viterbi_decode, for:
 * an unknown format; start < 0, nbits < 0, T < 0 or T > 2^31 - 1; start + n*T > nbits or an
 * int64 overflow in it; a bad block, warm or depth; null or misaligned pointers when T > 0
 * (d_capture, d_work 16-byte, d_bits 4-byte, d_stats 8-byte aligned).  T == 0: CVD_OK
 * without a launch (nothing is written).  Kernels: csrc/cvd_decode.hip. */
int64_t cvd_viterbi_workspace_bytes(int32_t n, int32_t m, int64_t T, int32_t block);
int cvd_viterbi_decode(const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                       int64_t start, int64_t T, int32_t block, int32_t warm, int32_t depth,
                       uint32_t* d_bits, int64_t* d_stats, void* d_work, void* stream);

/* The same decoder over a punctured capture (nothing in the reference): DVB-S and 802.11a send
 * (133,171) at rate 2/3 ... 7/8 by leaving output bits out in a periodic pattern.  A hard-bit
 * capture has no value for an erased bit, so the pattern goes into the decoder: a step reads
 * its transmitted bits where the pattern puts them and the erased outputs do not count.
 * Everything that is not restated here is cvd_viterbi_decode's: the code shapes and
 * CVD_E_UNSUPPORTED, the capture formats with their alignment and 16-byte readability rule,
 * states and branches, the tie rule, the end-state rule, the traceback, d_bits, block / warm /
 * depth (0 / -1 / -1 = default), the definitions of stats[0..8] block for block, and the
 * workspace, cvd_viterbi_workspace_bytes(n, m, T, block) (its layout does not depend on the
 * pattern).
 * Pattern: keep[c], 0 <= c < period, 1 <= period <= 16: bit j of keep[c] says that output j
 * of a step in column c was transmitted; step t is in column t mod period.  Every keep[c] is
 * nonzero and has no bit at or above n.  keep is a host pointer, copied in at the call.
 * Bit positions (all 64-bit): pre[c] = sum_{c' < c} popcount(keep[c']), K = pre[period],
 *   pos(t) = start + (t div period)*K + pre[t mod period];
 * the kept outputs of step t, j ascending, are capture bits pos(t), pos(t)+1, ...; y_t has
 * those bits in their positions j and zeros elsewhere.
 * Metric: in the forward recursion d_H(out, y_t) becomes
 *   popcount((out ^ y_t) & keep[t mod period]),
 * and errors counts over the transmitted bits only.  Relative metrics still fit a byte: any
 * state is reached from any other in m steps of at most n kept bits each, so D <= n*m holds
 * as before.
 * d_stats: int64[10]; [0..8] as above, [9] = pos(T) - start, the capture bits consumed (the
 * channel's crossover probability is estimated by errors / stats[9]).
 * Defaults of warm and depth: erased bits make survivors merge later.  With e = n*period - K
 * erased bits per period the unpunctured defaults grow by the factor 1 + GAIN * e / K, rounded
 * up (GAIN = 1 is the scaling by the inverse of the kept fraction, n*period/K; the gains are
 * measured at rates 3/4 and 7/8; without erasures the defaults are
 * cvd_viterbi_decode's): */
#define CVD_VITERBI_PUNCT_WARM_GAIN 2
#define CVD_VITERBI_PUNCT_DEPTH_GAIN 5
#define CVD_VITERBI_PUNCT_WARM(m, n, period, K) \
  ((CVD_VITERBI_WARM(m) * ((K) + CVD_VITERBI_PUNCT_WARM_GAIN * ((n) * (period) - (K))) + (K) - 1) / (K))
#define CVD_VITERBI_PUNCT_DEPTH(m, n, period, K) \
  ((CVD_VITERBI_DEPTH(m) * ((K) + CVD_VITERBI_PUNCT_DEPTH_GAIN * ((n) * (period) - (K))) + (K) - 1) / (K))
/* Consistency: with every keep[c] == 2^n - 1, at any period, the call returns
 * cvd_viterbi_decode's bits and stats[0..8] exactly (at the same block, warm and depth, or at
 * the defaults, which are then cvd_viterbi_decode's), and stats[9] == n*T.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming
 * viterbi_decode_punctured, for: every case cvd_viterbi_decode lists (with pos(T) in the
 * place of start + n*T); null keep; period outside 1..16; a zero column; a bit at or above n;
 * pos(T) > nbits, or an int64 overflow on the way to pos(T).  T == 0: CVD_OK, nothing written.
 * Kernels: csrc/cvd_decode_punct.hip (forward, join), csrc/cvd_decode.hip (the rest). */
int cvd_viterbi_decode_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                 const void* d_capture, int64_t nbits, int32_t format,
                                 int64_t start, int64_t T, int32_t block, int32_t warm, int32_t depth,
                                 uint32_t* d_bits, int64_t* d_stats, void* d_work, void* stream);

/* The same decoder over soft decisions (nothing in the reference): a demodulator's confidence
 * value per channel bit instead of the sliced bit, which costs about 2 dB.  An erased bit is a
 * value of 0, so a depunctured soft capture (cvd_soft_depuncture below) goes through this one
 * decoder; it knows nothing about patterns.
 * Capture: one int8 per channel bit in device memory; value start + n*t + j belongs to output
 * j of step t, 0 <= t < T.  v > 0: the bit is more likely 1; v < 0: more likely 0; v = 0: an
 * erasure; -128 is read as -127, so that with a(v) = min(|v|, 127) the contract is symmetric.
 * d_soft is 16-byte aligned and readable up to nvals rounded up to 16 bytes; nothing at or
 * past that is read.  Positions are 64-bit.
 * Metric: in the forward recursion of cvd_viterbi_decode, d_H(out, y_t) becomes
 *   cost(out, t) = sum_j a(v_{t,j}) * [v_{t,j} != 0 and (v_{t,j} > 0) != bit j of out].
 * Everything that is not restated here is cvd_viterbi_decode's: the code shapes and
 * CVD_E_UNSUPPORTED, states and branches, D_0 = 0, the tie rule, the normalisation, the
 * end-state rule, the traceback, d_bits, block / warm / depth (0 / -1 / -1 = default:
 * CVD_VITERBI_BLOCK, CVD_VITERBI_WARM(m), CVD_VITERBI_DEPTH(m)) and the definitions of
 * stats[1..8] block for block.  Relative metrics obey D <= 127*n*m <= 3048 (any state is
 * reached from any other in m steps of at most 127*n each), so the warm and end vectors are
 * 16-bit and the workspace has a size function of its own.
 * d_stats: int64[11], written (not accumulated), 8-byte aligned:
 *   [0]     the soft distance of the traced path, sum_t cost(out(s_t, u_t), t)
 *   [1..8]  as in cvd_viterbi_decode
 *   [9]     hard errors: #{(t, j) : v != 0 and (v > 0) != bit j of out(s_t, u_t)}
 *   [10]    the non-erased values among the n*T
 * stats[9] / stats[10] estimates the channel's crossover probability (the p that scan needs);
 * the soft distance is not that quantity.
 * Consistency: with every value +-A the call returns cvd_viterbi_decode's bits and
 * stats[1..8] on the signs, stats[0] = A * errors, stats[9] = errors, stats[10] = n*T; with
 * zeros at the erased positions, cvd_viterbi_decode_punctured's.
 * block + warm <= 2^20 (the unnormalised metrics of a block run over block + warm steps;
 * CVD_E_INVALID above that); the result is exact for everything accepted.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming viterbi_decode_soft,
 * for: every case cvd_viterbi_decode lists (nvals in the place of nbits, no format); the
 * block + warm bound; null or misaligned pointers when T > 0 (d_soft, d_work 16-byte, d_bits
 * 4-byte, d_stats 8-byte aligned).  T == 0: CVD_OK without a launch (nothing is written).
 * d_work: cvd_viterbi_soft_workspace_bytes(n, m, T, block) bytes, 16-byte aligned
 * (cvd_viterbi_workspace_bytes and two 16-bit vectors per block; < 0 as that one).
 * Kernels: csrc/cvd_decode_soft.hip (forward, join, the hard-error count),
 * csrc/cvd_decode.hip (the rest). */
int64_t cvd_viterbi_soft_workspace_bytes(int32_t n, int32_t m, int64_t T, int32_t block);
int cvd_viterbi_decode_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                            int64_t start, int64_t T, int32_t block, int32_t warm, int32_t depth,
                            uint32_t* d_bits, int64_t* d_stats, void* d_work, void* stream);
/* A punctured soft capture spread out to n values per step, zeros (erasures) where the pattern
 * transmits nothing.  keep, period and pos(t) exactly as cvd_viterbi_decode_punctured defines
 * them (n in {2, 3}), with values in the place of bits: for 0 <= t < T,
 *   d_out[n*t + j] = d_in[pos(t) + rank of j among the kept outputs of keep[t mod period]]
 * where keep[t mod period] has bit j, and 0 otherwise.  d_out holds n*T values rounded up to
 * 16 bytes, the padding written as zeros; it is 16-byte aligned and does not overlap d_in
 * (any alignment; only values inside [0, nvals) are read).
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming soft_depuncture, for:
 * n outside 2..3; null keep; period outside 1..16; a zero column; a bit at or above n;
 * start < 0, nvals < 0, T < 0 or T > 2^31 - 1; pos(T) > nvals, or an int64 overflow on the way
 * to it; when T > 0 a null d_in or d_out, a misaligned d_out, or overlapping buffers.
 * T == 0: CVD_OK, nothing written.  Kernel: csrc/cvd_decode_soft.hip. */
int cvd_soft_depuncture(const int8_t* d_in, int64_t nvals, int64_t start,
                        const uint8_t* keep, int32_t period, int32_t n, int64_t T,
                        int8_t* d_out, void* stream);

/* ---- framed captures: a batch of terminated frames in one call (nothing in the reference) ----
 * 802.11a/g PPDUs, GSM bursts and CCSDS / AX.25-style packets are terminated frames: a
 * frame starts in a known state (0) and is driven back to a known state by m tail bits, and a
 * capture holds thousands to millions of them, at a regular stride or at offsets that a
 * sync-word search found.  These calls decode F frames of T steps each in one launch, with the
 * boundary states told to the decoder.
 * Inherited: the code shapes (k = 1, n in {2, 3}, 1 <= m <= 8, else CVD_E_UNSUPPORTED), the
 * capture formats with their 16-byte alignment and readability rule, states and branches, the
 * tie rule (`val < best`, ties keep b = 0) and the metric of each flavour are
 * cvd_viterbi_decode's, cvd_viterbi_decode_punctured's (keep, period, pos) and
 * cvd_viterbi_decode_soft's (-128 is read as -127, 0 is an erasure).  Nothing in those three
 * calls changes.
 * Frames: frame f, 0 <= f < F, begins at capture bit (soft: value) o_f = start + f*stride when
 * d_offsets is null, else at o_f = d_offsets[f] (a device array of F int64, 8-byte aligned;
 * start and stride are then ignored).  Every frame has T steps, 1 <= T <= 65536.  Step t of
 * frame f reads capture bits o_f + n*t + j; in the punctured call it reads at pos(t) of that
 * contract with o_f in the place of start, so the pattern restarts at column 0 in every frame.
 * span = n*T, in the punctured call pos(T) - start.  Frames may overlap or repeat; the capture
 * is only read. */
#define CVD_VITERBI_FRAME_MAX_T 65536
#define CVD_FRAME_ANY (-1)
/* Boundary conditions (metrics unnormalised, over the integers extended by +inf):
 *   start_state = CVD_FRAME_ANY: D_0(s) = 0 for every s;
 *   start_state = s0 in [0, 2^m): D_0(s0) = 0 and D_0(s) = +inf elsewhere;
 *   end_state = CVD_FRAME_ANY: s_T is the lowest-index state with minimal D_T;
 *   end_state = e in [0, 2^m): s_T = e.
 * The recursion (without the normalisation), the traceback and u_t are cvd_viterbi_decode's.
 * Any implementation constant larger than every finite path metric gives the same result as
 * +inf: a state of finite metric has a predecessor of finite metric, which wins its comparison,
 * so the traced path never passes through a state of infinite metric and the decisions at such
 * states are never read.  With both states fixed T >= m is required, so that e is reachable.
 * d_bits: F rows of w = ceil(T/32) words, bit t of row f = u_t LSB first, padding bits zero.
 * d_frames: int32[F][6], 4-byte aligned:
 *   [0] the distance D_T(s_T): the Hamming distance, the Hamming distance over the kept bits,
 *       or the soft distance    [1] s_0 as traced    [2] s_T    [3] status: 0 decoded, 1 skipped
 *   [4] hard errors: equal to [0] for hard and punctured frames; soft: the sign disagreements
 *       of the traced path    [5] counted positions: n*T, the kept bits, or the non-erased values
 * d_stats: int64[6], written (not accumulated), 8-byte aligned:
 *   [0] sum of distances  [1] frames decoded  [2] frames skipped  [3] sum of hard errors
 *   [4] sum of counted  [5] w
 * stats[3] / stats[4] estimates the channel's crossover probability.  All sums are integer, so
 * the result does not depend on the launch shape.
 * Skipped frames (offset mode only): a frame with o_f < 0 or o_f + span > nbits is not decoded;
 * its row of bits is zero, its record {0, -1, -1, 1, 0, 0}, and nothing is read for it.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming viterbi_decode_frames
 * (_punctured, _soft), for: an unknown format; nbits < 0; F < 0; start_state or end_state
 * outside {-1} u [0, 2^m); in stride mode start < 0 or stride < 1; and when F > 0: T outside
 * 1..65536; both states fixed and T < m; F*w >= 2^31 words; in stride mode
 * start + (F-1)*stride + span > nbits or an int64 overflow on the way; null or misaligned
 * pointers (d_capture, d_work 16-byte, d_stats, d_offsets 8-byte, d_bits, d_frames 4-byte
 * aligned).  The punctured call reports a bad pattern as cvd_viterbi_decode_punctured does.
 * F == 0: CVD_OK without a launch (nothing is written).
 * d_work: cvd_viterbi_frames_workspace_bytes(n, m, T, F, soft) bytes, 16-byte aligned: the
 * decision words of the frames (T rounded up to 64 steps of max(8, 2^m / 8) bytes), of at most
 * a batch of about 1 GiB (the environment variable CVD_FRAMES_BATCH_BYTES, read at both calls,
 * sets another size; never less than 64 frames), which the call goes through batch after batch
 * on `stream`; the result does not depend on the batch.  0 at
 * F == 0; < 0 with the error set for n, m outside the shapes, T outside 1..65536, F < 0 or
 * soft outside {0, 1}.  A size of 0 allows a null d_work.  Asynchronous on `stream`.
 * Kernels: csrc/cvd_decode_frames.hip. */
int64_t cvd_viterbi_frames_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t soft);
int cvd_viterbi_decode_frames(const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                              int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                              int32_t start_state, int32_t end_state,
                              uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream);
int cvd_viterbi_decode_frames_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                        const void* d_capture, int64_t nbits, int32_t format,
                                        int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                        int32_t start_state, int32_t end_state,
                                        uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                        void* stream);
int cvd_viterbi_decode_frames_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                   int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                   int32_t start_state, int32_t end_state,
                                   uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work, void* stream);

/* ---- tail-biting frames: wrap-around Viterbi, batched in one call (nothing in the reference) ----
 * LTE control blocks (PBCH, PDCCH / DCI: (133,171,165), 24 to about 100 steps), 802.16 FCH and
 * bursts ((171,133), punctured) and the IS-54 / EDGE control channels are tail-biting frames: the
 * encoder starts in the state that the frame's own last m information bits leave it in, so it
 * ends in the state it started in and no tail bits are sent.  Neither boundary state is known
 * to the decoder; what is known is that they are equal.
 * Inherited unchanged from the cvd_viterbi_decode_frames* contract above: the code shapes, the
 * capture formats with their alignment and readability rule, the placement of the frames
 * (stride mode, or d_offsets with skipped frames), 1 <= T <= CVD_VITERBI_FRAME_MAX_T, the metric
 * of each flavour (in the punctured call step t is in column t mod period in every lap), states,
 * branches and the tie rule, the layout of d_bits, F*w < 2^31, and F == 0.  There are no
 * start_state / end_state arguments.
 * max_laps = I, 1 <= I <= CVD_VITERBI_TAILBITING_MAX_LAPS; 0: CVD_VITERBI_TAILBITING_LAPS. */
#define CVD_VITERBI_TAILBITING_LAPS 4
#define CVD_VITERBI_TAILBITING_MAX_LAPS 8
/* The decoder of one frame (the wrap-around Viterbi algorithm; a sequential decoder written from
 * this text reproduces the result bit for bit).  E^0(s) = 0 for all s.  Laps l = 1, 2, ...:
 *   forward    T steps of the inherited recursion from D^l_0 = E^{l-1}, unnormalised within the
 *              lap, decisions dec^l_t(s') recorded; every lap reads the same T received words.
 *   normalise  E^l(s) = D^l_T(s) - min_s D^l_T(s).
 *   trace      for every end state e, a^l(e) = the state at step 0 that the inherited traceback
 *              reaches from s_T = e through dec^l.
 *   B^l = {e : a^l(e) = e}, the tail-biting survivors; c^l(e) = D^l_T(e) - D^l_0(a^l(e)), the
 *   cost of e's survivor over the frame's own T steps; e* = the lowest-index state of minimal
 *   D^l_T.
 *   e* in B^l: stop, return the survivor of e* with status 0.
 *   Otherwise lap l is the last if l = I, or if l >= 2 and E^l = E^{l-1} as vectors (every
 *   further lap would repeat this one exactly).  On the last lap: B^l not empty: return the
 *   survivor of the e in B^l of minimal c^l(e), lowest index on ties, with status 2; B^l empty:
 *   return the survivor of e*, which is not tail-biting (s_0 != s_T), with status 3.
 *   Not the last lap: go on to lap l + 1.
 * The returned path gives u_t, s_0 = a^l(e) and s_T = e as the inherited traceback does.  T < m
 * is allowed (the state then wraps more than once; the rules stay well defined).  Metrics are
 * int32 without a +inf: no state is ever excluded.
 * d_frames: int32[F][8], 4-byte aligned:
 *   [0] c^l(e) of the returned path: the Hamming distance, the Hamming distance over the kept
 *       bits, or the soft distance    [1] s_0    [2] s_T
 *   [3] status: 0, 2 or 3 as above; 1 skipped
 *   [4] hard errors: equal to [0] for hard and punctured frames; soft: the sign disagreements
 *       of the returned path    [5] counted positions: n*T, the kept bits, or the non-erased values
 *   [6] laps run    [7] 0
 * A skipped frame has a zero row of bits and the record {0, -1, -1, 1, 0, 0, 0, 0}.
 * d_stats: int64[9], written (not accumulated), 8-byte aligned:
 *   [0] sum of distances  [1] frames decoded (status 0, 2 or 3)  [2] frames skipped
 *   [3] sum of hard errors  [4] sum of counted  [5] w  [6] frames of status 2
 *   [7] frames of status 3  [8] sum of laps
 * All are integer sums, so the result does not depend on the launch shape.
 * Consistency:
 *   with I = 1 every frame of status 0 or 3 has the row, [0], [1] and [2] of
 *   cvd_viterbi_decode_frames(..., CVD_FRAME_ANY, CVD_FRAME_ANY);
 *   the soft call on values +-A returns the hard call's rows, states, status and laps, with
 *   [0] = A * errors;
 *   the punctured call with every keep[c] = 2^n - 1 returns the hard call's result.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming
 * viterbi_decode_frames_tailbiting (_punctured, _soft), for every case that the frames calls
 * list except those about the boundary states, and for max_laps outside 0..8.
 * d_work: cvd_viterbi_tailbiting_workspace_bytes(n, m, T, F, soft) bytes, 16-byte aligned.  0
 * where the kernel keeps a frame's decision words (T rounded up to 64 steps of max(8, 2^m / 8)
 * bytes) in LDS: up to 8 KiB of them, T <= 1024 at m <= 6.  Otherwise one frame's decision
 * words per wave of the launch (at most 8,192 waves, and as many as about 1 GiB holds): per
 * wave, not per frame, a wave reuses its slice.  The environment variables
 * CVD_TAILBITE_LDS_BYTES (the LDS limit, at most 32 KiB) and CVD_TAILBITE_WAVES (the wave cap),
 * read at both calls, are for measurements and tests.  0 at F == 0; < 0 with the error set as
 * cvd_viterbi_frames_workspace_bytes.  A size of 0 allows a null d_work.  Asynchronous on
 * `stream`: one launch.  Kernels: csrc/cvd_decode_tailbite.hip. */
int64_t cvd_viterbi_tailbiting_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t soft);
int cvd_viterbi_decode_frames_tailbiting(const cvd_code* code, const void* d_capture, int64_t nbits, int32_t format,
                                         int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                         int32_t max_laps,
                                         uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                         void* stream);
int cvd_viterbi_decode_frames_tailbiting_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                   const void* d_capture, int64_t nbits, int32_t format,
                                                   int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                                                   int32_t T, int32_t max_laps,
                                                   uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                                   void* stream);
int cvd_viterbi_decode_frames_tailbiting_soft(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                              int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                                              int32_t T, int32_t max_laps,
                                              uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                              void* stream);

/* ---- soft output: max-log-MAP values per bit of framed soft captures (nothing in the reference) ----
 * Every decoder above ends in hard information bits and one distance per frame.  An outer code
 * (Reed-Solomon with erasures, a CRC-aided list or Chase stage), the ranking of the candidates of
 * a blind search, or the choice of which frames to trust needs to know how sure each bit is.  This
 * call is cvd_viterbi_decode_frames_soft with a value L_t per step beside the bit: the difference
 * between the best path with u_t = 0 and the best path with u_t = 1, in the units of the input.
 * Inherited unchanged from cvd_viterbi_decode_frames_soft: the code shapes (k = 1, n in {2, 3},
 * 1 <= m <= 8, else CVD_E_UNSUPPORTED), the int8 capture (-128 read as -127, 0 an erasure, 16-byte
 * alignment and readability, nothing at or past nvals rounded up to 16 bytes is read), cost(out, t),
 * the placement of the frames (stride mode, or d_offsets with skipped frames), 1 <= T <=
 * CVD_VITERBI_FRAME_MAX_T, CVD_FRAME_ANY, T >= m when both states are fixed, F*w < 2^31 with
 * w = ceil(T/32), and F == 0 (CVD_OK, nothing written).
 * The recursion of one frame, over the integers extended by +inf (a sequential decoder written
 * from this text reproduces the result bit for bit); ps_b and out as in cvd_viterbi_decode, S = 2^m:
 *   alpha_0 = D_0 of the frames contract (0 everywhere, or 0 at start_state and +inf elsewhere);
 *   alpha_{t+1}(s') = min_b [alpha_t(ps_b) + cost(out(ps_b, s' & 1), t)];
 *   beta_T(s) = 0 for every s if end_state is CVD_FRAME_ANY, else beta_T(e) = 0, +inf elsewhere;
 *   beta_t(s) = min_u [cost(out(s, u), t) + beta_{t+1}(((s << 1) | u) & (S - 1))];
 *   M_u(t) = min over the states s' with s' & 1 = u of [alpha_{t+1}(s') + beta_{t+1}(s')], u in
 *   {0, 1}: alpha_{t+1} is already the minimum over the predecessors, so this is the cost of the
 *   best whole path whose input at step t is u.
 * The value of step t:
 *   L_t = M_0(t) - M_1(t): positive when a 1 is more likely, the sign convention and the units of
 *   the input values; L_t = +32767 if M_0(t) = +inf, L_t = -32767 if M_1(t) = +inf.
 * Both minima are never infinite together (some path satisfies the boundary conditions).  A finite
 * L_t obeys |L_t| <= 127*n*(m+1) <= 3429 (flip u_t on the best path and rejoin it m steps later),
 * so int16 holds every value and +-32767 is unambiguous.  With end_state fixed exactly the steps
 * t >= T - m are saturated, with the sign that bit T-1-t of e gives (the tail is known); with
 * end_state CVD_FRAME_ANY nothing is saturated.  Any implementation constant above every finite
 * metric serves as +inf; the frames calls' 2^28 does if two of them may be added.
 * d_llr: F rows of 32*w int16, 16-byte aligned; value t of row f is L_t, values at or past T are 0.
 * d_bits: as the frames calls; bit t of row f = [L_t > 0].
 * d_frames: int32[F][6], 4-byte aligned:
 *   [0] the distance min(M_0(t), M_1(t)): the same for every t, and cvd_viterbi_decode_frames_soft's [0]
 *   [1] #{t : L_t = 0}, the steps the decoder cannot decide
 *   [2] s_T by the frames rule: e, or the lowest-index state of minimal alpha_T
 *   [3] status: 0 decoded, 1 skipped
 *   [4] min |L_t| over the unsaturated t, the frame's weakest bit; 32767 if there is none
 *   [5] #{t : |L_t| = 32767}
 * A skipped frame has zero rows of values and bits and the record {0, 0, -1, 1, 0, 0}.
 * d_stats: int64[6], written (not accumulated), 8-byte aligned:
 *   [0] sum of distances  [1] frames decoded  [2] frames skipped  [3] sum of [1]  [4] sum of [5]  [5] w
 * All sums are integer sums, so the result does not depend on the launch shape.
 * Consistency: wherever L_t != 0, bit t equals the bit of cvd_viterbi_decode_frames_soft on the
 * same arguments (L_t > 0 means that every best path has u_t = 1); [0] and [2] equal that call's.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming viterbi_decode_frames_llr,
 * for every case that cvd_viterbi_decode_frames_soft lists, and for a null or misaligned d_llr.
 * d_work: cvd_viterbi_llr_workspace_bytes(n, m, T, F) bytes, 16-byte aligned.  The kernel does not
 * keep alpha for every step: it keeps the vector at every 32nd step, 2^m int32 each, and
 * recomputes a segment of 32 steps before beta runs back through it; the first segment starts
 * from D_0 and the last one is not computed twice.  0 where T <= 64.  Otherwise ceil(T/32) - 2
 * vectors per wave of the launch (at most 8,192 waves, and as many as about 1 GiB holds): per
 * wave, not per frame, a wave reuses its slice.  The environment variable
 * CVD_LLR_WAVES (the wave cap), read at both calls, is for measurements and tests.  (The segment
 * length is a compile-time constant: there is no CVD_LLR_SEG.)  0 at F == 0; < 0 with the error
 * set for n, m outside the shapes, T outside 1..65536 or F < 0.  A size of 0 allows a null d_work.
 * Asynchronous on `stream`: one launch.  Kernel: csrc/cvd_decode_llr.hip. */
int64_t cvd_viterbi_llr_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F);
int cvd_viterbi_decode_frames_llr(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                  int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                  int32_t start_state, int32_t end_state,
                                  int16_t* d_llr, uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats,
                                  void* d_work, void* stream);

/* ---- punctured soft frames: the three frame decoders on values behind a pattern (nothing in the reference) ----
 * What a receiver hands over at the punctured rates: an 802.11a/g PPDU at rate 2/3 or 3/4 is a
 * terminated, punctured frame of demapper confidences; 802.16 FCH and bursts are tail-biting,
 * punctured and soft.  d_soft / nvals are cvd_viterbi_decode_frames_soft's capture, keep / period
 * cvd_viterbi_decode_punctured's pattern (n in {2, 3}), and the frames are placed as in the frames
 * contract with span = pos(T) - start.  The three calls are specified bit for bit by one rule:
 *   For frame f at o_f let, for 0 <= t < T and 0 <= j < n,
 *     v'_f[n*t + j] = d_soft[pos(t) + rank of j among the kept outputs of keep[t mod period]]
 *   where keep[t mod period] has bit j, and 0 otherwise, with pos taken with o_f in the place of
 *   start: exactly cvd_soft_depuncture's definition with start = o_f, so the pattern restarts at
 *   column 0 in every frame.
 *   The result of the punctured soft call is the result of the corresponding unpunctured soft
 *   call (cvd_viterbi_decode_frames_soft, _tailbiting_soft, _llr) on the frames v'_f: every bit,
 *   every L_t, every field of every record and every total.
 * Only the placement and the skip test use span = pos(T) - start (stride mode:
 * start + (F-1)*stride + span <= nvals; offset mode: a frame with o_f < 0 or o_f + span > nvals
 * is skipped), and the call reads nothing outside [o_f, o_f + span) of a decoded frame, beyond
 * the readability rule's whole 16-byte pieces below nvals rounded up to 16.  It follows that
 * counted ([5] of the frames and tail-biting records) is the number of kept values that are not
 * 0, a kept value of 0 is still an erasure, -128 is still read as -127, the tie rule is
 * unchanged, and every lap of the tail-biting decoder has step t in column t mod period.
 * Workspaces: those of the unpunctured soft calls (cvd_viterbi_frames_workspace_bytes with
 * soft = 1, cvd_viterbi_tailbiting_workspace_bytes with soft = 1, cvd_viterbi_llr_workspace_bytes):
 * a decision word or a checkpoint does not depend on the pattern.  The environment variables of
 * those calls apply.
 * CVD_E_INVALID (CVD_E_UNSUPPORTED for the code shape), before the device is touched,
 * cvd_last_error() naming viterbi_decode_frames_soft_punctured,
 * viterbi_decode_frames_tailbiting_soft_punctured or viterbi_decode_frames_llr_punctured: every
 * case of the unpunctured soft sibling, and a bad pattern (null keep, period outside 1..16, a
 * zero column, a bit at or above n) as cvd_viterbi_decode_punctured reports it; an int64
 * overflow on the way to span.  F == 0: CVD_OK without a launch.  Asynchronous on `stream`.
 * Kernels: csrc/cvd_decode_psoft.hip (the lane type PSLane of csrc/cvd_decode_lanes.h around
 * the bodies that the unpunctured decoders' kernels are built from). */
int cvd_viterbi_decode_frames_soft_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                             const int8_t* d_soft, int64_t nvals,
                                             int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                                             int32_t T, int32_t start_state, int32_t end_state,
                                             uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats, void* d_work,
                                             void* stream);
int cvd_viterbi_decode_frames_tailbiting_soft_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                                        const int8_t* d_soft, int64_t nvals,
                                                        int64_t start, int64_t stride, const int64_t* d_offsets,
                                                        int64_t F, int32_t T, int32_t max_laps,
                                                        uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats,
                                                        void* d_work, void* stream);
int cvd_viterbi_decode_frames_llr_punctured(const cvd_code* code, const uint8_t* keep, int32_t period,
                                            const int8_t* d_soft, int64_t nvals,
                                            int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                                            int32_t T, int32_t start_state, int32_t end_state,
                                            int16_t* d_llr, uint32_t* d_bits, int32_t* d_frames, int64_t* d_stats,
                                            void* d_work, void* stream);

/* ---- list decoding of soft frames, and a CRC over rows of decoded bits (nothing in the reference) ----
 * Every frame decoder above ends in one row of bits per frame and cannot say whether it is right.
 * The frames they were built for carry the answer: an 802.11 PPDU ends in an FCS, GSM / EDGE and
 * LTE control blocks carry a CRC, AX.25 and CCSDS packets a CRC-16.  cvd_viterbi_decode_frames_list
 * returns the L best paths of every frame (the parallel list Viterbi algorithm) and cvd_frames_crc
 * checks rows of bits on the device, so that the first candidate that passes is picked without
 * the bits leaving the GPU: the usual 1 to 2 dB of frame error rate on short frames.
 * Inherited unchanged from cvd_viterbi_decode_frames_soft: the code shapes (k = 1, n in {2, 3},
 * 1 <= m <= 8, else CVD_E_UNSUPPORTED), the int8 capture (-128 read as -127, 0 an erasure, 16-byte
 * alignment and readability) and cost(out, t), states and branches, the placement of the frames
 * (stride mode, or d_offsets with skipped frames; span = n*T), CVD_FRAME_ANY and the rule T >= m
 * when both states are fixed, and F == 0 (CVD_OK, no launch, nothing written).  Here
 * 1 <= T <= CVD_VITERBI_LIST_MAX_T and 1 <= L <= CVD_VITERBI_LIST_MAX_L: a frame's decisions cost
 * 2^m * L / 2 bytes per step, 8 MiB per wave at the caps with m = 8; list decoding pays on short
 * frames.
 * The recursion of one frame, over the integers, unnormalised; a list holds at most L values in
 * ascending order and "absent" stands in the place of +inf (a sequential decoder written from this
 * text reproduces every output bit for bit).  ps_b = (s' >> 1) | (b << (m-1)) and out as in
 * cvd_viterbi_decode:
 *   A_0(s) = [0] for every s if start_state is CVD_FRAME_ANY, else for s = start_state only; every
 *   other list is empty.
 *   For step t and next state s', u = s' & 1: the candidates are
 *     c(b, r) = A_t(ps_b)[r] + cost(out(ps_b, u), t)   for b in {0, 1} and every present rank r;
 *   A_{t+1}(s') is the first min(L, number of candidates) of them in ascending order of the triple
 *   (c, b, r), and dec_t(s')[rank] = (b, r) of the candidate that took that rank.
 *   End: with end_state = e the end list is (A_T(e)[r], e, r) in the order of r; with
 *   CVD_FRAME_ANY it is the first L of all present (A_T(s)[r], s, r) in ascending order of that
 *   triple.  P, the number of paths found, is its length.
 *   Path l, 0 <= l < P, starts from the l-th end entry (distance, s_T, r_T).  For t = T-1 .. 0:
 *     u_t = s_{t+1} & 1;  (b, r) = dec_t(s_{t+1})[r_{t+1}];  s_t = (s_{t+1} >> 1) | (b << (m-1));  r_t = r.
 * Consequences (checked on a sequential decoder of this text): path 0 is
 * cvd_viterbi_decode_frames_soft's, in bits, distance, s_0 and s_T (the order (c, b, r) reduces
 * to `val < best`, ties keep b = 0, and the end rule to the lowest-index state of minimal D_T);
 * the result for L is the first L paths of the result for any L' > L; distances are non-decreasing
 * in l; with a fixed start state the rows of a frame are pairwise distinct, with CVD_FRAME_ANY the
 * pairs (s_0, row) are; with both states fixed P = min(L, 2^(T-m)); for a fixed start state the
 * distances are the L smallest costs over all inputs that satisfy the end condition.
 * d_bits: F*L rows of w = ceil(T/32) words; row f*L + l holds path l of frame f, bit t = u_t LSB
 * first, padding bits zero; the row of an absent path (l >= P) is zero.
 * d_paths: int32[F][L][3], 4-byte aligned: {distance, s_0 as traced, s_T}; an absent path is
 * {-1, -1, -1}.
 * d_frames: int32[F][2], 4-byte aligned: {P in 0..L, status: 0 decoded, 1 skipped}.  A skipped
 * frame (offset mode: o_f < 0 or o_f + span > nvals) has zero rows, absent paths and {0, 1}, and
 * nothing is read for it.
 * d_stats: int64[5], written (not accumulated), 8-byte aligned:
 *   [0] sum of the path-0 distances  [1] frames decoded  [2] frames skipped  [3] sum of P  [4] w
 * All sums are integer sums, so the result does not depend on the launch shape.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming viterbi_decode_frames_list,
 * for: every case that cvd_viterbi_decode_frames_soft lists; L outside 1..8; and when F > 0: T
 * outside 1..8192; F*L*w >= 2^31 words; a null or misaligned d_paths or d_frames (4-byte).
 * d_work: cvd_viterbi_list_workspace_bytes(n, m, T, F, L) bytes, 16-byte aligned.  The kernel keeps
 * a tile of decisions in LDS: tsteps = min(T, 16384 / (2^m * LL / 2)) steps, LL = 2, 4 or 8 the
 * least of them that is >= L.  A frame of at most tsteps steps needs no workspace: 0, and a null
 * d_work is allowed.  Otherwise ceil(T / tsteps) - 1 tiles (tsteps * 2^m * LL / 2 bytes each,
 * rounded up to 16) per wave of the launch (at most 8,192 waves, as many as the frames, and as
 * many as about 1 GiB holds): per wave, not per frame, a wave reuses its slice.  The environment
 * variables CVD_LIST_WAVES (the wave cap) and CVD_LIST_LDS_BYTES (the tile's bytes in the place of
 * 16384, clamped to 1024..49152), read at both calls, are for tests and measurements.  0 at
 * F == 0; < 0 with the error set for n, m outside the shapes, L outside 1..8, T outside 1..8192 or
 * F < 0.  Asynchronous on `stream`: one launch.  Kernels: csrc/cvd_decode_list.hip. */
#define CVD_VITERBI_LIST_MAX_L 8
#define CVD_VITERBI_LIST_MAX_T 8192
int64_t cvd_viterbi_list_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t L);
int cvd_viterbi_decode_frames_list(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                   int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F, int32_t T,
                                   int32_t start_state, int32_t end_state, int32_t L,
                                   uint32_t* d_bits, int32_t* d_paths, int32_t* d_frames, int64_t* d_stats,
                                   void* d_work, void* stream);

/* ---- list decoding of tail-biting soft frames (nothing in the reference) ----
 * The tail-biting frames that the calls above were built for are short frames that end in a CRC:
 * LTE PBCH and PDCCH / DCI (CRC-16, masked with the RNTI on a DCI), 802.16 FCH, EDGE control
 * blocks.  cvd_viterbi_decode_frames_tailbiting_soft returns one path per frame, and
 * cvd_viterbi_decode_frames_list needs boundary states that such a frame does not have.  This call
 * returns up to L tail-biting paths of every frame, for cvd_frames_crc to choose from.
 * Inherited unchanged from cvd_viterbi_decode_frames_tailbiting_soft: the code shapes, the int8
 * capture, cost(out, t), the placement of the frames and skipped frames, states, branches and the
 * tie rule, max_laps = I (0: CVD_VITERBI_TAILBITING_LAPS, at most CVD_VITERBI_TAILBITING_MAX_LAPS),
 * and that T < m is allowed.  From cvd_viterbi_decode_frames_list: 1 <= L <= CVD_VITERBI_LIST_MAX_L,
 * 1 <= T <= CVD_VITERBI_LIST_MAX_T, F*L*w < 2^31 with w = ceil(T/32), and the layout of d_bits
 * (row f*L + l holds path l of frame f; the row of an absent path is zero).
 * The decoder of one frame (a sequential decoder written from this text reproduces every output bit
 * for bit).  E^0(s) = 0 for every s.  Laps l = 1, 2, ...:
 *   forward    T steps of the list recursion of cvd_viterbi_decode_frames_list from
 *              A^l_0(s) = [E^{l-1}(s)], one entry in every state: the candidates in ascending order
 *              of (c, b, r), lists of at most L entries, dec^l_t(s')[rank] = (b, r); every lap reads
 *              the same T received words.
 *   normalise  D^l_T(s) = A^l_T(s)[0]; E^l(s) = D^l_T(s) - min_s D^l_T(s); e* = the lowest-index
 *              state of minimal D^l_T.
 *   trace      for every present entry (e, r) of every end state, a^l(e, r) = the state at step 0
 *              that the list call's traceback reaches from (s_T, r_T) = (e, r) through dec^l.
 *   stop       the rule of cvd_viterbi_decode_frames_tailbiting_soft on rank 0: with
 *              B^l = {e : a^l(e, 0) = e}, lap l is the last if e* is in B^l (status 0), or if l = I, or
 *              if l >= 2 and E^l = E^{l-1} as vectors; in the last two cases the status is 2 if B^l
 *              is not empty and 3 if it is.  Not the last lap: go on to lap l + 1.
 *   On the last lap: C = {(e, r) present : a^l(e, r) = e}, the tail-biting entries, and
 *   c(e, r) = A^l_T(e)[r] - E^{l-1}(a^l(e, r)), the cost of the entry's path over the frame's own T
 *   steps.  Path 0 is the path that cvd_viterbi_decode_frames_tailbiting_soft returns: the entry
 *   (e0, 0) with e0 = e* for status 0 and 3, and the e in B^l of minimal c(e, 0), lowest index on
 *   ties, for status 2.  Paths 1, 2, ... are the members of C other than (e0, 0) in ascending order
 *   of the triple (c, e, r), the first L - 1 of them: P = 1 + min(L - 1, |C \ {(e0, 0)}|) paths.
 *   Every path is traced as in the list call (u_t, s_0 as traced, s_T = e) and reported with its c.
 * Consequences (checked on a sequential decoder of this text):
 *   L = 1 is cvd_viterbi_decode_frames_tailbiting_soft in bits, [0], [1], [2], status and laps, and
 *   for every L path 0, the status and the laps are (on rank 0 the order (c, b, r) is `val < best`);
 *   paths l >= 1 are tail-biting (s_0 = s_T), pairwise distinct as rows, and distinct from a
 *   tail-biting path 0 (a path 0 of status 3 is not tail-biting, and a path l >= 1 may have its row);
 *   c is non-decreasing from l = 1 on;
 *   a path l >= 1 may be cheaper than path 0, of status 0 or 2 too (path 0 is chosen among the
 *   ranks 0 by D^l_T, which holds E^{l-1} of the start state; about 2% of frames at a noise of 1.5
 *   amplitudes);
 *   the result for L is NOT a prefix of the result for a larger L: an entry of rank >= L can be
 *   tail-biting where the lower ranks of its state are not, so lists of more entries find other
 *   members of C.  An implementation whose lists hold more than L entries must make ranks >= L
 *   absent at every step.
 * d_paths: int32[F][L][3], 4-byte aligned: {c, s_0, s_T}; an absent path is {-1, -1, -1}.
 * d_frames: int32[F][4], 4-byte aligned: {P, status (0, 2 or 3 as above; 1 skipped), laps run, |C|}.
 * A skipped frame has zero rows, absent paths and {0, 1, 0, 0}, and nothing is read for it.
 * d_stats: int64[8], written (not accumulated), 8-byte aligned:
 *   [0] sum of the path-0 c  [1] frames decoded  [2] frames skipped  [3] sum of P  [4] w
 *   [5] frames of status 2  [6] frames of status 3  [7] sum of laps
 * All sums are integer sums, so the result does not depend on the launch shape.
 * CVD_E_INVALID (CVD_E_UNSUPPORTED for the code shape), before the device is touched,
 * cvd_last_error() naming viterbi_decode_frames_tailbiting_list, for every case that
 * cvd_viterbi_decode_frames_tailbiting_soft and cvd_viterbi_decode_frames_list list (but those about
 * the boundary states): nvals < 0; F < 0; max_laps outside 0..8; L outside 1..8; in stride mode
 * start < 0 or stride < 1; and when F > 0: T outside 1..8192; F*L*w >= 2^31 words; in stride mode
 * start + (F-1)*stride + n*T > nvals or an int64 overflow on the way; null or misaligned pointers
 * (d_soft, d_work 16-byte, d_stats, d_offsets 8-byte, d_bits, d_paths, d_frames 4-byte aligned).
 * F == 0: CVD_OK without a launch (nothing is written).
 * d_work: cvd_viterbi_tailbiting_list_workspace_bytes(n, m, T, F, L) bytes, 16-byte aligned: the
 * tiling of cvd_viterbi_list_workspace_bytes, to the byte (a tile of decisions in LDS, the other
 * tiles of a frame in a slice per wave of the launch; 0, and a null d_work allowed, when a frame's
 * decisions fit the tile).  CVD_LIST_WAVES and CVD_LIST_LDS_BYTES apply, read at both calls.  0 at
 * F == 0; < 0 with the error set for n, m outside the shapes, L outside 1..8, T outside 1..8192 or
 * F < 0.  Asynchronous on `stream`: one launch.  Kernels: csrc/cvd_decode_tblist.hip.  The rows are
 * in the layout that cvd_frames_crc reads. */
int64_t cvd_viterbi_tailbiting_list_workspace_bytes(int32_t n, int32_t m, int32_t T, int64_t F, int32_t L);
int cvd_viterbi_decode_frames_tailbiting_list(const cvd_code* code, const int8_t* d_soft, int64_t nvals,
                                              int64_t start, int64_t stride, const int64_t* d_offsets, int64_t F,
                                              int32_t T, int32_t max_laps, int32_t L,
                                              uint32_t* d_bits, int32_t* d_paths, int32_t* d_frames, int64_t* d_stats,
                                              void* d_work, void* stream);

/* A CRC over rows of bits in any layout that the decoders write (cvd_viterbi_decode_frames*, the
 * tail-biting calls, the list): `rows` rows of w words, bit t of a row = bit (t & 31) of word
 * t >> 5, called u_t.  One 32-bit value per row.  With mask = 2^width - 1:
 *   reg = init & mask;
 *   for i = 0 .. count-1:  fb = (bit width-1 of reg) ^ u_{first+i};  reg = (reg << 1) & mask;
 *                          if fb, reg ^= poly;
 *   field = sum over i < width of u_{first+count+i} << (width-1-i): the width bits that follow the
 *   data, the first of them most significant;
 *   d_value[row] = reg ^ field.
 * So 0 says "the appended CRC matches"; a CRC masked with an identity (an LTE DCI's RNTI) yields
 * the identity; an 802.11 FCS (the complemented CRC-32, init all ones, the bits in transmission
 * order) yields 0xFFFFFFFF.  Reflected CRCs are served by feeding the bits in transmission order;
 * there is no reflection parameter.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming frames_crc, for: width
 * outside 1..32; poly or init with bits at or above width; first < 0 or count < 0; w < 1 or
 * rows < 0; first + count + width > 32*w; a null or misaligned (4-byte) d_bits or d_value when
 * rows > 0.  rows == 0: CVD_OK, nothing written.  d_value: `rows` uint32.  Asynchronous on
 * `stream`.  Kernel: csrc/cvd_decode_list.hip. */
int cvd_frames_crc(const uint32_t* d_bits, int64_t rows, int32_t w, int32_t first, int32_t count,
                   int32_t width, uint32_t poly, uint32_t init, uint32_t* d_value, void* stream);

/* ---- encoder: information bits -> a capture (comp_parity.py encode_convolutional, batched) ----
 * The inverse of the frames decoders: F rows of information bits become one capture that every
 * cvd_viterbi_decode* call accepts as it stands, so that decode(encode(u)) == u and
 * encode(decode(y)) ^ y (where the channel errors are) are one call each.
 * Code shapes: k = 1, n in {2, 3}, 1 <= m <= 16 (an encoder has no 2^m anywhere; the blind
 * search finds codes past the decoders' m = 8); anything else CVD_E_UNSUPPORTED.  States,
 * branches and tap order are cvd_viterbi_decode's.
 * Input: d_info, F rows of `pitch` words, pitch >= w = ceil(T/32); bit t of row f = bit (t & 31)
 * of word f*pitch + (t >> 5) is u_t: the d_bits layout of every frames decoder (with
 * pitch = L*w and the pointer moved by i*w words it reads path i of a list result).  Bits of a
 * row at or past T are ignored and need not be zero.  4-byte aligned.
 * Coded bits of a frame: output j of step t, 0 <= t < T, is
 *   c_{t,j} = XOR_{d=0..m} taps[j][0][d] * u_{t-d},
 * where, by mode: */
#define CVD_ENCODE_OPEN       0  /* u_{-d} = bit d-1 of start_state, d = 1..m */
#define CVD_ENCODE_TERMINATED 1  /* as OPEN, and u_t is taken as 0 for t >= T - m whatever the row holds */
#define CVD_ENCODE_TAILBITING 2  /* u_{-d} = u_{(T-d) mod T}; start_state is ignored */
#define CVD_CAPTURE_SOFT      3  /* output only: one int8 per channel bit, +A for a 1, -A for a 0 */
/* TERMINATED needs T >= m: a decoder's row, tail included, re-encodes as it is, and a row of
 * T - m data bits needs no zeroing.  TAILBITING allows T < m, as the tail-biting decoders do;
 * the encoder ends in the state it started in.
 * Puncturing: keep == NULL: none; frame position n*t + j holds c_{t,j} and span = n*T.
 * Otherwise keep / period / pos(t) are exactly cvd_viterbi_decode_punctured's, with o_f in the
 * place of start (the pattern restarts at column 0 in every frame): only the outputs j with bit
 * j of keep[t mod period] are emitted, j ascending, at pos(t), pos(t)+1, ...; span = pos(T) - o_f.
 * Output: `nout` positions (bits; bytes for CVD_CAPTURE_BYTES / _SOFT) in format
 * CVD_CAPTURE_LSB / _MSB / _BYTES, read back exactly as the decoders read them, or
 * CVD_CAPTURE_SOFT (amplitude = A, 1 <= A <= 127; amplitude must be 0 in the other formats).
 * d_out is 16-byte aligned and holds the byte length of nout (ceil(nout/8), or nout) rounded up
 * to 16.  The call writes all of it: every position that no frame covers, and the padding, is 0
 * (bit 0; an erasure in SOFT).  Nothing at or past the rounded length is touched.
 * Placement: d_offsets == NULL (stride mode): o_f = start + f*stride, stride >= span.
 * Otherwise o_f = d_offsets[f] (a device array of F int64, 8-byte aligned; BYTES and SOFT only;
 * start and stride are ignored): a frame with o_f < 0 or o_f + span > nout is skipped and
 * nothing is written for it; where frames overlap, a shared position holds the value of one of
 * the frames that cover it, unspecified which.
 * d_stats: NULL, or int64[2], 8-byte aligned, written (not accumulated): [0] frames written,
 * [1] frames skipped.
 * The result is exact and does not depend on the launch shape (the environment variable
 * CVD_ENCODE_BLOCKS, read at the call, caps the blocks of a launch).  Asynchronous on `stream`.
 * CVD_E_INVALID, before the device is touched, cvd_last_error() naming encode_frames, for: a
 * null code; an unknown mode or format; an amplitude outside 1..127 in SOFT or nonzero
 * otherwise; start_state outside [0, 2^m) in OPEN or TERMINATED; F < 0 or nout < 0; d_offsets
 * in a packed format; a bad pattern (as cvd_viterbi_decode_punctured reports it); in stride mode
 * start < 0 or stride < 1; and when F > 0: T outside 1..2^31 - 1; TERMINATED with T < m;
 * pitch < w; in stride mode stride < span (frames would overlap) or
 * start + (F-1)*stride + span > nout; an int64 overflow on the way to the span, F*pitch or the
 * last frame's end; a null or misaligned d_info (4-byte) or d_out (16-byte); a misaligned
 * d_offsets or d_stats (8-byte).  F == 0: CVD_OK without a launch (nothing is written).
 * Kernels: csrc/cvd_encode.hip. */
int cvd_encode_frames(const cvd_code* code, const uint8_t* keep, int32_t period,
                      const uint32_t* d_info, int64_t pitch, int64_t F, int64_t T,
                      int32_t mode, int32_t start_state,
                      int32_t format, int32_t amplitude,
                      void* d_out, int64_t nout, int64_t start, int64_t stride, const int64_t* d_offsets,
                      int64_t* d_stats, void* stream);

/* ---- error-exponent engine (alpha_exponent.py, Eq. 7) ---------------------
 * Joint counts of (metric state i, received word r) along received streams
 * (pitch = nseq) for steps t >= burn_in, on a dense (enumerated) model with
 * S < 4096: d_cnt[i*2^n + r] += count (uint64, accumulated, not cleared).
 * The chain's next state is the model's automaton (alpha_exponent.py:136-149). */
int cvd_count_transitions(const cvd_model* model, const uint32_t* d_r, int64_t N, int64_t nseq,
                          int64_t burn_in, uint64_t* d_cnt, void* stream);
/* M(u) = sum_r P1(i->j,r)^u P2(i->j,r)^(1-u) for u = d_u[0..U) from joint counts
 * cnt1/cnt2 [K*R] (f64) of tensors P = (C + laplace) / rowsum over (j, r)
 * (alpha_exponent.py:152-154), C[i,j,r] = cnt[i,r] iff j = next(i,r): written as
 * d_a[U*K] (rank-one part, M += a 1^T) and d_vals[U*K*R] (entry (i, next(i,r))). */
int cvd_chernoff_build(int32_t K, int32_t R, const double* d_cnt1, const double* d_cnt2, double laplace,
                       const double* d_u, int32_t U, double* d_a, double* d_vals, void* stream);
/* Dense M(u)[i][j] (d_vals[U*K*K]) from arbitrary P1, P2 [K*K*R] (alpha_exponent.py:170-180). */
int cvd_chernoff_build_dense(int32_t K, int32_t R, const double* d_P1, const double* d_P2,
                             const double* d_u, int32_t U, double* d_vals, void* stream);
/* Perron root of each of U nonnegative K x K matrices M = a 1^T + ELL(vals, cols)
 * (E entries per row; d_cols NULL: dense rows, E = K; d_a NULL: no rank-one part)
 * by power iteration with Collatz-Wielandt bounds: d_rho[3u..3u+2] = (estimate,
 * lower, upper bound) once (upper - lower) <= tol * upper (irreducible aperiodic M), else
 * once the power-iteration norm ratio is stable to tol/100 and the bracket has stopped
 * shrinking (the estimate), or after max_iter iterations (d_iters[u]).  The estimate in d_rho[3u] is CERTIFIED only
 * when both bounds are finite and meet that tolerance (then it is their midpoint); in
 * every other case it is the uncertified norm ratio, which for a periodic, reducible or
 * defective M can be far from rho -- the caller checks the bounds.  A bracket is never
 * reported met while some x_i is 0 (the upper bound needs x > 0: it is +inf then).
 * K <= 10232 (2 K doubles + 128 B within 160 KiB): vectors in LDS, one workgroup per u;
 * larger K (structured form only, d_cols non-NULL): vectors in HBM, one launch per phase. */
int cvd_spectral_radius(int32_t K, int32_t E, const double* d_a, const double* d_vals,
                        const int32_t* d_cols, int32_t U, double tol, int32_t max_iter, double* d_rho,
                        int32_t* d_iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CVD_H */
