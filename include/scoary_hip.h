/*
 * scoary_hip.h -- C-ABI of the MI355X-native association engine for Scoary.
 *
 * Drop-in boundary for ONE path of AdmiralenOla/Scoary (v1.6.16): the per-gene
 * 2x2 contingency counting + Fisher exact test of Setup_results /
 * Perform_statistics and the --permute label-shuffling empirical-p loop.
 * The reference is pure Python and has no FFI of its own; each entry point
 * below names the reference code it replaces (paths relative to the reference
 * checkout) -- that call site is where a maintainer binds it (ctypes stub in
 * INTEGRATION.md).
 *
 * Conventions
 *   - every `d_` pointer is DEVICE memory on the handle's GPU, owned by the
 *     caller (e.g. a torch tensor's data_ptr()); nothing is allocated or freed
 *     behind the caller's back except a small per-handle scratch;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream) and never synchronises the device;
 *   - return value: 0 = ok, negative = error (see scoary_last_error); the
 *     library never calls exit();
 *   - one handle per GPU; a handle is used by one host thread at a time.
 *
 * Device layouts (all little-endian)
 *   rows64   : uint64 [R][W64], W64 = ceil(N/64); bit i of word w of a row is
 *              isolate 64*w+i; pad bits are zero.  (How the reference's
 *              genedic / traitsdic 0/1 values are bit-packed)
 *   tiled    : the gene matrix as the kernels read it: uint32 [Qp][Gp][4]
 *              ("word-quad-major"): the 16 bytes at ((q*Gp)+g)*16 hold 32-bit
 *              words 4q..4q+3 of gene g's row.  Qp = scoary_tiled_quads(N),
 *              Gp = scoary_tiled_genes(G); padding genes / words are zero.
 *              One lane owns one gene, so a wavefront's loads are 1 KiB
 *              coalesced and the per-trait operand is wave-uniform.
 *   vecrows  : trait / validity-mask / permuted-label vectors: uint32 [R][Wp],
 *              Wp = scoary_row_words(N) = 4*Qp >= 2*W64 (a rows64 row followed
 *              by zero padding).
 */
#ifndef SCOARY_HIP_H
#define SCOARY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCOARY_ABI_VERSION 11

/* error codes */
#define SCOARY_OK 0
#define SCOARY_ERR_ARG (-1)    /* bad argument (null pointer, negative size) */
#define SCOARY_ERR_HIP (-2)    /* a HIP runtime call failed */
#define SCOARY_ERR_SIZE (-3)   /* problem size outside what the kernels support */
#define SCOARY_ERR_DEVICE (-4) /* no such device / not a gfx950 code object */

typedef struct scoary_ctx *scoary_handle;
typedef void *scoary_stream_t; /* hipStream_t */

int scoary_abi_version(void);

/* Create / destroy the per-GPU context. */
int scoary_create(int device, scoary_handle *out);
void scoary_destroy(scoary_handle h);
/* Message of the last failing call on this handle ("" if none). */
const char *scoary_last_error(scoary_handle h);

/* Layout arithmetic (pure functions, usable without a GPU). */
int64_t scoary_tiled_quads(int64_t N);            /* Qp */
int64_t scoary_tiled_genes(int64_t G);            /* Gp */
int64_t scoary_tiled_bytes(int64_t G, int64_t N); /* 16*Qp*Gp */
int64_t scoary_row_words(int64_t N);              /* Wp */

/* ---- a1: genedic -> packed bits ---------------------------------------
 * Replaces the dict-of-dicts the reference builds in Csv_to_dic_Roary
 * (scoary/methods.py:445-491; presence rule :476-485 applied by the caller).
 * scoary_pack_dense : d_dense is uint8 [G][N], non-zero = present.
 * scoary_tile_rows  : d_rows64 is rows64 [G][W64].
 * Both write the full tiled buffer (scoary_tiled_bytes), padding included. */
int scoary_pack_dense(scoary_handle h, const uint8_t *d_dense, int64_t G,
                      int64_t N, uint32_t *d_tiled, scoary_stream_t stream);
int scoary_tile_rows(scoary_handle h, const uint64_t *d_rows64, int64_t G,
                     int64_t N, uint32_t *d_tiled, scoary_stream_t stream);

/* ---- a3: Perform_statistics (scoary/methods.py:930-982) ----------------
 * For every (trait, gene): tpgp, tpgn, tngp, tngn over the isolates that are
 * valid for that trait.  d_traits / d_masks are vecrows [T][Wp] (label bits,
 * validity bits; traits & ~masks must be 0).
 *   d_counts  : int32 [T][G][4]   (tpgp, tpgn, tngp, tngn)  -- bit-exact
 *   d_margins : int32 [T][2]      (npos, nval) per trait
 * Not for a stream that is capturing a hipGraph (SCOARY_ERR_ARG: it allocates its plan in
 * stream-ordered temporary memory): record scoary_counts_planned instead. */
int scoary_counts(scoary_handle h, const uint32_t *d_tiled,
                  const uint32_t *d_traits, const uint32_t *d_masks, int64_t G,
                  int64_t T, int64_t N, int32_t *d_counts, int32_t *d_margins,
                  scoary_stream_t stream);
/* The same in two parts (ABI 7), for callers that run more than one step per trait set: the
 * trait PLAN -- everything the counts need that depends on the traits alone -- is built once
 * (as the index lists are built once per gene matrix), and the per-step call is one kernel
 * that streams the gene matrix once per pass of up to 32 traits.
 *   scoary_trait_plan : d_margins int32 [T][2] = (npos, nval) per trait (the isolate loop of
 *       scoary/methods.py:940-965 sees exactly the valid isolates: :591-598); d_mask_class
 *       int32 [T] (may be NULL) = the smallest t' <= t IN THE SAME PASS (traits
 *       [k tb, (k + 1) tb), tb = scoary_counts_traits_per_pass(T)) whose validity row equals
 *       trait t's -- traits of one class share popc(gene & valid), counted once per class and
 *       pass (most traits of a real file have no missing values: one class per pass; ABI 8: the
 *       search no longer leaves the pass, at most 31 row compares per trait); d_plan = an opaque
 *       buffer of scoary_trait_plan_bytes(T, N) bytes: the classes as dense slots per pass and
 *       the label / validity rows gathered quad-major, one contiguous operand row per gene
 *       quad and pass (what k_counts reads with wide scalar loads).
 *   scoary_counts_planned : d_counts as scoary_counts; d_plan / d_margins from
 *       scoary_trait_plan of the same traits, masks, T and N.
 * scoary_counts(...) == scoary_trait_plan into stream-ordered temporary memory +
 * scoary_counts_planned. */
int64_t scoary_counts_traits_per_pass(int64_t T);   /* traits one pass over the matrix takes (<= 32) */
int64_t scoary_trait_plan_bytes(int64_t T, int64_t N);
int scoary_trait_plan(scoary_handle h, const uint32_t *d_traits, const uint32_t *d_masks,
                      int64_t T, int64_t N, int32_t *d_margins, int32_t *d_mask_class,
                      void *d_plan, scoary_stream_t stream);
int scoary_counts_planned(scoary_handle h, const uint32_t *d_tiled, const void *d_plan,
                          const int32_t *d_margins, int64_t G, int64_t T, int64_t N,
                          int32_t *d_counts, scoary_stream_t stream);

/* ---- a5: scipy.stats.fisher_exact(obs_table) at scoary/methods.py:854 ---
 * Two-sided Fisher exact p and sample odds ratio for M 2x2 tables
 * [[tpgp, tpgn], [tngp, tngn]] (d_tables int32 [M][4]); SciPy >= 1.7
 * semantics: (nan, 1.0) when a margin is zero, inf odds when tpgn*tngp == 0;
 * a support point counts as "as extreme as observed" iff its weight is
 * <= the observed weight * (1 + 1e-14) -- SciPy's own factor -- and that
 * comparison is decided exactly (double-double) whenever the fp64 weights agree
 * to 1e-9: tables whose two closest support points are 1e-12 apart (they
 * exist: tests/golden/near_ties.json) get SciPy's p, exact ties are ties.
 * Tolerance: |p - scipy| < 1e-12 for N <= 40 000 (measured <= 3e-15).  Above that SciPy
 * 1.15.3 ITSELF leaves the exact value of its rule (6.0e-12 on (5582, 3263, 70693,
 * 40462), N = 120 000); the kernel follows the exact value -- pinned by the oracle
 * against integer arithmetic at N = 50 000 ... 131 070 (tests/test_oracle_golden.py).
 *   d_p, d_or : double [M]
 *   d_crit    : uint32 [M][2] or NULL -- the rejection region of table m as
 *               (base, span): a permuted table with overlap count a' is "as
 *               or more extreme" iff (uint32)(a' - base) >= span.  Consumed by
 *               scoary_permute.  Tables the reference never tests
 *               (gene absent / present in all valid isolates,
 *               scoary/methods.py:804-814) get p = 1, odds = nan, span = 0. */
int scoary_fisher(scoary_handle h, const int32_t *d_tables, int64_t M,
                  double *d_p, double *d_or, uint32_t *d_crit,
                  scoary_stream_t stream);
/* scipy.stats.fisher_exact's OWN double for the tables of 171 ... scoary_fisher_scipy_max_isolates() (104 723)
 * isolates: d_p[m] is overwritten with the value SciPy >= 1.7 returns for table m, to the last bit (Boost.Math's
 * prime-factorised hypergeometric pmf, its tail recurrences and fisher_exact's binary search restated in fp64;
 * scoary_amd/csrc/scoary_scipy.hip).  Replaces, for what a caller PRINTS, the per-gene call the reference makes
 * (scoary/methods.py:854): with it the result files are the reference's bytes at any size, not only up to 170
 * isolates where scoary_fisher already returns SciPy's double.  Tables with an empty margin, with fewer than 171
 * isolates or with more than the maximum are left as they are; *d_skipped (uint64, may be NULL; zero it first)
 * counts the tables above the maximum.  About 50 x the work of scoary_fisher per table (15 pmf evaluations over the
 * primes up to N; 9.5 ms per 500 000 tables at N = 2000): an output-fidelity pass for the command line, not part of the association step bench.py times.
 * The first call on a device uploads the prime table (a synchronous 40 KB copy: not inside a graph capture). */
int64_t scoary_fisher_scipy_max_isolates(void);
int scoary_fisher_scipy(scoary_handle h, const int32_t *d_tables, int64_t M, double *d_p,
                        uint64_t *d_skipped, scoary_stream_t stream);
/* The same test for the list-driven permutation path, one launch fewer per step:
 * tables [T][G][4] are visited in LIST-SLOT order (slot k of trait t = gene
 * d_lorder[k]; slots are sorted by minority count, so the lanes of a wavefront walk
 * supports of similar length), results land at the gene's own index as in
 * scoary_fisher (d_crit may be NULL), and the rejection region is also written in
 * the form scoary_permute_lists consumes: d_lcrit uint32 [T][G][2] = (lo, hi1) of the
 * LIST count in slot order (ones-list: [base, base + span); zeros-list:
 * [npos - base - span + 1, npos - base + 1); span 0 -> (0, 0)).
 *   d_lorder / d_lflipped : from scoary_lists_plan */
int scoary_fisher_lists(scoary_handle h, const int32_t *d_tables, int64_t T, int64_t G,
                        const int32_t *d_lorder, const uint8_t *d_lflipped,
                        double *d_p, double *d_or, uint32_t *d_crit, uint32_t *d_lcrit,
                        scoary_stream_t stream);
/* scoary_fisher_lists with one weight chain per margin class: the hypergeometric weights a table's walk passes
 * through depend on (trait, canonical gene count) alone, so a first kernel (k_fisher_chains) walks every class of
 * the step once -- both sides of the mode, weights and running sums, up to scoary_fisher_chains_capacity() entries
 * per side or until a weight falls below scoary_fisher_chains_floor() of the mode's -- and the table kernel
 * (k_fisher_tables) reads a weight where scoary_fisher_lists divides; past the end of a stored chain it walks on by
 * itself.  Every output is scoary_fisher_lists' own, bit for bit.
 *   N        : the isolates of the matrix the tables were counted on (every a + b + c + d <= N)
 *   d_chains : scoary_fisher_chains_bytes(T, N) bytes of caller-owned scratch, rewritten by every call (nothing
 *              is kept between calls); chains_bytes = its size.  scoary_fisher_chains_bytes returns 0 when the
 *              slabs would exceed 256 MiB (T * floor(N / 2) > 65536): then, with d_chains = NULL, or with
 *              scoary_set_fisher_route(h, SCOARY_FISHER_ROUTE_WALK), the call is scoary_fisher_lists.
 *   scoary_set_fisher_route : for this handle, WALK (scoary_fisher_lists' kernel), CHAINS (the two kernels whenever
 *              d_chains is given) or AUTO (the default): the two kernels for launches of at least four table
 *              wavefronts per SIMD of the device (T * G >= 128 per SIMD) -- below that the one kernel is a single
 *              short round and the chain kernel's serial walks would only be added to it */
#define SCOARY_FISHER_ROUTE_WALK 0
#define SCOARY_FISHER_ROUTE_CHAINS 1
#define SCOARY_FISHER_ROUTE_AUTO 2
int64_t scoary_fisher_chains_bytes(int64_t T, int64_t N);
int64_t scoary_fisher_chains_capacity(void);
double scoary_fisher_chains_floor(void);
int scoary_set_fisher_route(scoary_handle h, int mode);
int scoary_fisher_lists_chained(scoary_handle h, const int32_t *d_tables, int64_t T, int64_t G, int64_t N,
                                const int32_t *d_lorder, const uint8_t *d_lflipped,
                                double *d_p, double *d_or, uint32_t *d_crit, uint32_t *d_lcrit,
                                void *d_chains, int64_t chains_bytes, scoary_stream_t stream);

/* ---- a8: PermuteGTC (scoary/methods.py:1371-1384) ----------------------
 * Label permutations pi = perm_base .. perm_base+P-1 of the T traits whose
 * rows are given (their global trait numbers are trait_base .. trait_base+T-1,
 * the number that enters the Philox counter): the trait's npos positive labels
 * placed on a uniformly random subset of its valid isolates.  The reference's
 * shuffle is unseeded; here the bits are a pure function of (seed, trait,
 * permutation) -- Philox4x32-10 keyed by `seed` -- by a sampler in which no isolate
 * depends on the one before it (spec S4 of DESIGN.md, ABI 8; rounds 1-4 used
 * sequential selection sampling): min(npos, nval - npos) marks; round 0 marks every
 * valid isolate with an 8-bit probability (eight words of counter (isolate, pi >> 5,
 * trait, "SCOB" / "SCOC") shared by 32 permutations, compared bit-sliced); the
 * surplus or deficit is removed / added at uniformly drawn positions (counter
 * (draw >> 2, pi, trait, "SCOD"), Lemire rejection, non-candidates rejected).
 * Exactly uniform under ideal random words; the CPU oracle (oracle/oracle.c)
 * regenerates the same bits.
 *   d_perms : vecrows [T][P][Wp]
 * N <= scoary_perm_max_isolates() (a block keeps its rows in LDS). */
int64_t scoary_perm_max_isolates(void);
int scoary_perm_generate(scoary_handle h, const uint32_t *d_masks,
                         const int32_t *d_margins, int64_t T, int64_t N,
                         int64_t P, int64_t perm_base, int64_t trait_base,
                         uint64_t seed, uint32_t *d_perms, scoary_stream_t stream);

/* ---- a7: Permute (scoary/methods.py:1314-1369), Fisher statistic --------
 * d_r[t][g] += #{ pi < P : popcount(gene_g & perm_{t,pi}) lies in the
 * rejection region d_crit[t][g] }.  The caller zeroes d_r (uint32 [T][G])
 * before the first chunk of permutations; Empirical_p = (r+1)/(P_total+1)
 * (scoary/methods.py:1365). */
int scoary_permute(scoary_handle h, const uint32_t *d_tiled,
                   const uint32_t *d_perms, const uint32_t *d_crit, int64_t G,
                   int64_t T, int64_t N, int64_t P, uint32_t *d_r,
                   scoary_stream_t stream);

/* ---- a7 with the reference's sequential early abort (scoary/methods.py:1348-1365) ----
 * Opt-in (--permute-early-abort): every (gene, trait) consumes the permutations in index
 * order, r counting the ones in the rejection region; from permutation index i >= 30 on, the
 * first i with r >= d_thr[i] stops that gene: d_nstop[t][g] = i + 1 and Empirical_p =
 * (r + 1) / (i + 2) (`emp_p = (r+1.0)/(i+2.0)`, :1362); genes that never stop keep
 * d_nstop = 0 and get (r + 1) / (P_total + 1) (:1365).  d_thr[i] = smallest r with
 * 1 - binom.cdf(r, i, 0.1) < 0.05 (:1361) for 30 <= i < P_total, 0xffffffff below 30
 * (uint32 [P_total], built by the caller).  Call once per batch of permutations
 * [perm_base, perm_base + P) in ascending order; the caller zeroes d_r and d_nstop (uint32
 * [T][G]) before the first batch.  d_perms: vecrows [T][P][Wp] (scoary_perm_generate). */
int scoary_permute_seq(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_perms,
                       const uint32_t *d_crit, const uint32_t *d_thr, int64_t G, int64_t T,
                       int64_t N, int64_t P, int64_t perm_base, uint32_t *d_r,
                       uint32_t *d_nstop, scoary_stream_t stream);

/* ---- Westfall-Young single-step minP (ABI 11; spec S7 of DESIGN.md) -------------------
 * No counterpart in the reference (its only corrections are Bonferroni and Benjamini-Hochberg,
 * scoary/methods.py:903-925): for every permuted labelling the SMALLEST raw Fisher p over all genes,
 *   d_minp[t][pi] = min(d_minp[t][pi], min over g of p_tg(popcount(gene_g & perm_{t,pi}))),
 * p_tg(a) = what scoary_fisher returns, bit for bit, for the table (a, npos - a, gm - a,
 * nval - npos - gm + a) with the margins of d_counts[t][g].  The family-wise adjusted p of gene g is
 * (#{pi : minp[t][pi] <= p[t][g]} + 1) / (P + 1), counted by the caller from scoary_fisher's own p.
 *   scoary_minp_plan : per (trait, gene) the support [lo, hi] = [max(0, npos + gm - nval), min(npos, gm)]
 *       of the overlap count: d_lo int32 [T][G] = lo, d_off int64 [T * G + 1] = the exclusive prefix sum
 *       of the support sizes hi - lo + 1 (CSR offsets; the total last), *entries_out (HOST) = that
 *       total.  Synchronises `stream` (the caller needs the count to allocate d_tab), like
 *       scoary_lists_plan.
 *   scoary_minp_fill : d_tab double [entries]: d_tab[d_off[t G + g] + a - lo] = p_tg(a).  The entries
 *       are produced by scoary_fisher's own kernel over the enumerated tables, a chunk at a time;
 *       d_scratch = scoary_minp_fill_scratch_bytes(entries) bytes (the table list of one chunk).
 *   scoary_permute_minp : d_perms = vecrows [T][P][Wp] as scoary_perm_generate writes them (the
 *       permutations perm_base .. perm_base + P - 1 of these T traits); d_minp = double
 *       [T][minp_stride], the batch lands at columns perm_base .. perm_base + P - 1.  The CALLER
 *       initialises d_minp to 1.0 (the identity of the minimum); the call accumulates by min (a 64-bit
 *       atomic on the bit pattern of the non-negative double), so batches of permutations, gene
 *       shards (each with the plan / tables of its own genes) and trait groups (pointers moved to
 *       the group's first trait) compose.  Any N scoary_permute takes. */
int64_t scoary_minp_fill_scratch_bytes(int64_t entries);
int scoary_minp_plan(scoary_handle h, const int32_t *d_counts, int64_t T, int64_t G, int64_t *d_off,
                     int32_t *d_lo, int64_t *entries_out, scoary_stream_t stream);
int scoary_minp_fill(scoary_handle h, const int32_t *d_counts, const int64_t *d_off,
                     const int32_t *d_lo, int64_t T, int64_t G, int64_t entries, void *d_scratch,
                     double *d_tab, scoary_stream_t stream);
int scoary_permute_minp(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_perms,
                        const int64_t *d_off, const int32_t *d_lo, const double *d_tab, int64_t G,
                        int64_t T, int64_t N, int64_t P, int64_t perm_base, int64_t minp_stride,
                        double *d_minp, scoary_stream_t stream);

/* ---- Westfall-Young step-down minP (spec S8 of DESIGN.md) ------------------------------
 * Added after ABI 11 without a version change: three new entry points, nothing existing changes its
 * meaning, so a caller built against ABI 11 keeps working (backward compatible).
 * Per trait the genes are ranked ascending by (p, gene index): d_order int32 [T][G] = the gene at rank k,
 * d_psorted double [T][G] = its p (scoary_fisher's own double).  With the p tables of scoary_minp_plan /
 * _fill, for every label row b of the batch
 *   q_b[k] = min over j >= k of p_{t,order[j]}(popcount(gene_order[j] & perm_{t,b})),
 *   d_c[t][k] += #{ b : q_b[k] <= d_psorted[t][k] }          (uint32, BY RANK POSITION, doubles compared exactly),
 *   d_minp[t][perm_base + b] = min(itself, q_b[0])           (scoary_permute_minp's value, bit for bit; NULL: not kept).
 * The CALLER zeroes d_c before the first batch of permutations (batches add) and initialises d_minp to 1.0.
 * Ties, the running maximum over the ranks and the scatter back to gene order (S8 steps 4-6) are the caller's.
 * The rank order is walked in chunks and two passes: chunk minima first, then every chunk starts from the
 * minimum of the later chunks and counts -- no block waits for another.  scoary_stepdown_chunks = the number
 * of chunks for this (G, T, P) on this handle's device (host only, the launch shape's own value).
 * A chunk is ceil(G / chunks) positions rounded up to a multiple of 64.
 * scoary_stepdown_scratch_bytes = the size of d_scratch: the rank-ordered position arrays, every trait's gene
 * rows copied into rank order (one tiled matrix per trait, which is why it takes N), the chunk minima and one
 * count byte per trait, group of 64 permutations and position.  Nothing in it has to survive the call.  Asynchronous on `stream`, allocates nothing.  Any N scoary_permute_minp takes, the same size
 * refusals. */
int64_t scoary_stepdown_chunks(scoary_handle h, int64_t G, int64_t T, int64_t P);
int64_t scoary_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P);
int scoary_permute_stepdown(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_perms,
                            const int64_t *d_off, const int32_t *d_lo, const double *d_tab,
                            const int32_t *d_order, const double *d_psorted, int64_t G, int64_t T,
                            int64_t N, int64_t P, int64_t perm_base, int64_t minp_stride,
                            double *d_minp, uint32_t *d_c, void *d_scratch, scoary_stream_t stream);

/* ---- a7/a8, list-driven variant -------------------------------------------
 * Same result as scoary_perm_generate + scoary_permute (d_r is bit-identical),
 * different data flow: genes as lists of the isolates that carry their
 * minority value (built once per dataset, on the device: scoary_lists_plan /
 * scoary_lists_fill below), permuted labels as isolate-major tiles of 512 / 256 /
 * 128 / 64 permutations (N <= 2559 / 5119 / 10239 / beyond) that live in LDS, overlap
 * counts as bit-sliced counters, 128 (64 for the last) permutations per lane.  Cost
 * is proportional to the list length, so sparse (or near-core) genes are
 * cheap.  One 64-permutation tile fits in LDS up to N = 20479; wider matrices, up to N =
 * scoary_list_max_isolates() = 131070, are cut into scoary_list_segments(N) = 2 ... 7
 * SEGMENTS of 20352 isolates: a block loads its tile one segment at a time, a gene's
 * list is one sub-list per segment, the counters live across the reloads (round 3; the
 * dense kernels took over at N = 40960 before).
 *   d_tiles : uint32 [scoary_list_tiles_words(N, P, T)]
 *   d_lidx / d_lstart / d_lngroups / d_lorder / d_lflipped : the index lists of the
 *             gene matrix, built on the device by scoary_lists_plan + scoary_lists_fill
 *             (below); `entries` = the entry count scoary_lists_plan returned
 *   d_scratch : scoary_permute_lists_scratch_bytes(G, T, N, P) bytes: the rejection
 *             regions in list order and one 16-bit exceedance count per (trait,
 *             tile, list slot) -- the kernel writes them with plain stores and a
 *             small second kernel (k_lists_reduce) sums the tiles into d_r; no
 *             atomics (a device-scope atomic is a 32-byte memory-side write)
 *   d_crit  : regions in gene order from scoary_fisher (converted by a small kernel,
 *             needs d_margins), or NULL when
 *   d_lcrit : regions in slot order from scoary_fisher_lists is given (d_margins unused)
 *   d_r     : uint32 [T][G]; accumulate != 0: += like scoary_permute (further batches of
 *             permutations); accumulate == 0: overwritten (no zero fill needed) */
int64_t scoary_list_tiles_words(int64_t N, int64_t P, int64_t T);
int64_t scoary_list_tile_words(int64_t N);   /* dwords per (trait, tile) */
int64_t scoary_list_max_isolates(void);
int64_t scoary_list_segments(int64_t N);     /* 1 for N <= 20479, else ceil(N / 20352); 0: too large */
/* out5 = { tile row width in dwords of 32 permutations (16 for N <= 2559, 8 for N <= 5119,
 * 4 for N <= 10239, 2 beyond), row stride in bytes, genes per wavefront, residue classes,
 * interleave piece } -- the last four are the arguments scoary_lists_build
 * wants.  Error if N is too large. */
int scoary_list_params(int64_t N, int64_t *out5);
/* Label tiles of the permutations perm_base .. perm_base + P - 1 (perm_base a multiple of 32):
 * d_tiles = uint32 [T][ntiles][scoary_list_tile_words(N)], the same labels as
 * scoary_perm_generate.  _range writes only the flat (trait, tile) indices first_tile ..
 * first_tile + n_tiles - 1 of that array, in place: the ranks of a multi-GPU run can each
 * generate one contiguous share and all-gather the rest (scoary_amd/dist.py). */
int scoary_perm_generate_tiles(scoary_handle h, const uint32_t *d_masks,
                               const int32_t *d_margins, int64_t T, int64_t N, int64_t P,
                               int64_t perm_base, int64_t trait_base, uint64_t seed,
                               uint32_t *d_tiles, scoary_stream_t stream);
int scoary_perm_generate_tiles_range(scoary_handle h, const uint32_t *d_masks,
                                     const int32_t *d_margins, int64_t T, int64_t N, int64_t P,
                                     int64_t perm_base, int64_t trait_base, uint64_t seed,
                                     int64_t first_tile, int64_t n_tiles, uint32_t *d_tiles,
                                     scoary_stream_t stream);
/* ---- labels shuffled within strata (spec S9 of DESIGN.md; additive, ABI 11) --------------
 * Restricted exchangeability: d_strata[i] in [0, S) names the stratum (lineage, cluster, ...) of isolate i,
 * the same for all traits.  Independently for every stratum the trait's npos_ts positives among the
 * stratum's members lie on a uniformly random subset of its nval_ts valid members: S4's plan per
 * (trait, stratum), S4's round 0 with the stratum's q, and the fix-up per (permutation, stratum) over the
 * stratum's members (Philox counter ((s << 20) | (draw >> 2), pi, trait, "SCOD")).  With S = 1 the labels
 * are scoary_perm_generate's bit for bit.  npos and nval of the trait are unchanged, so margins, crit and
 * the p tables of the unstratified path stay valid and every consumer of label rows / tiles takes these.
 *   d_strata   : uint16 [N]
 *   d_members  : int32 [N], the isolates ordered by (stratum, index)
 *   d_offsets  : int32 [S + 1], members of stratum s = d_members[d_offsets[s] .. d_offsets[s + 1]);
 *                d_offsets[0] = 0 and d_offsets[S] = N.  A DEVICE array: that it partitions [0, N) is
 *                checked by the caller on its host copy (scoary_amd/engine.py: strata_plan); the kernel
 *                clamps every index it derives, so a bad table gives wrong labels, not a wild access
 *   d_smargins : int32 [T][S][2] = (npos_ts, nval_ts), written by scoary_strata_margins from the label rows
 *                d_labels and validity rows d_masks (vecrows [T][Wp])
 * S <= scoary_perm_max_strata(), N <= scoary_perm_strata_max_isolates() (unsegmented label tiles),
 * T <= 65535, permutation indices < 2^32: SCOARY_ERR_SIZE otherwise.  Rows: vecrows [T][P][Wp]; tiles: the
 * layout and the (first_tile, n_tiles) range of scoary_perm_generate_tiles_range, perm_base a multiple
 * of 32. */
int scoary_perm_max_strata(void);
int64_t scoary_perm_strata_max_isolates(void);
int scoary_strata_margins(scoary_handle h, const uint32_t *d_labels, const uint32_t *d_masks,
                          const uint16_t *d_strata, int64_t T, int64_t N, int64_t S,
                          int32_t *d_smargins, scoary_stream_t stream);
int scoary_perm_generate_strata(scoary_handle h, const uint32_t *d_masks, const uint16_t *d_strata,
                                const int32_t *d_members, const int32_t *d_offsets,
                                const int32_t *d_smargins, int64_t T, int64_t N, int64_t S, int64_t P,
                                int64_t perm_base, int64_t trait_base, uint64_t seed,
                                uint32_t *d_perms, scoary_stream_t stream);
int scoary_perm_generate_tiles_strata_range(scoary_handle h, const uint32_t *d_masks,
                                            const uint16_t *d_strata, const int32_t *d_members,
                                            const int32_t *d_offsets, const int32_t *d_smargins,
                                            int64_t T, int64_t N, int64_t S, int64_t P,
                                            int64_t perm_base, int64_t trait_base, uint64_t seed,
                                            int64_t first_tile, int64_t n_tiles, uint32_t *d_tiles,
                                            scoary_stream_t stream);
/* ---- Cochran-Mantel-Haenszel test over the strata (spec S10 of DESIGN.md; additive, ABI 11) -----------
 * No counterpart in the reference.  Per (trait, gene) the 2x2 tables of the S strata -- a = popc(gene & label &
 * stratum), m = popc(gene & valid & stratum), k = npos_ts, n = nval_ts -- are counted and folded in ascending
 * stratum order into fp64 sums whose operation order S10 fixes: the continuity-corrected CMH chi-square (R's
 * mantelhaen.test(correct = TRUE)), its p = erfc(sqrt(stat / 2)), the Mantel-Haenszel common odds ratio, and the
 * rejection region of the POOLED overlap count a' = popc(gene & label) under within-stratum shuffles (S9), in
 * the (base, span) form scoary_permute / scoary_permute_lists / scoary_permute_hybrid consume: the exact
 * stratified permutation test of the CMH statistic is those kernels run with this d_crit.
 *   d_labels / d_masks : vecrows [T][Wp], as scoary_strata_margins took them
 *   d_strata / d_members / d_offsets / d_smargins : the strata plan of scoary_perm_generate_strata (d_offsets is
 *       part of the plan and is not read: the stratum of a member is d_strata's)
 *   d_stat, d_p, d_odds, d_e2 (twice the expectation of the pooled count), d_var : double [T][G];
 *   d_a : int32 [T][G], the pooled count; d_crit : uint32 [T][G][2]
 *   (trait, gene) pairs without an informative stratum (d_var = 0; the genes the reference never tests among
 *   them) get stat = nan, p = 1 and the region (0, 0): every permutation counts
 *   d_scounts : int32 [T][G][S][2] = (a, m) of every stratum, or NULL (the usual case: the per-stratum tables
 *       live in registers only)
 *   d_scratch : scoary_cmh_scratch_bytes(N) bytes, the strata as a table of (word, stratum, mask) segments,
 *       rebuilt by every call; nothing in it has to survive the call
 * Asynchronous on `stream`, allocates nothing, may be recorded into a graph.  The size limits of the strata
 * plan: S <= scoary_perm_max_strata(), N <= scoary_perm_strata_max_isolates(), T <= 65535 (SCOARY_ERR_SIZE). */
int64_t scoary_cmh_scratch_bytes(int64_t N);
int scoary_cmh(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_labels, const uint32_t *d_masks,
               const uint16_t *d_strata, const int32_t *d_members, const int32_t *d_offsets,
               const int32_t *d_smargins, int64_t G, int64_t T, int64_t N, int64_t S, double *d_stat,
               double *d_p, double *d_odds, double *d_e2, double *d_var, int32_t *d_a, uint32_t *d_crit,
               int32_t *d_scounts, void *d_scratch, scoary_stream_t stream);
/* ---- Westfall-Young tables of the CMH statistic (spec S11 of DESIGN.md; additive, ABI 11) ---------------
 * The family-wise adjusted p of the stratified test: scoary_permute_minp / scoary_permute_stepdown run unchanged
 * over tables of the CMH statistic instead of Fisher's p.  Under within-stratum shuffles (S9) E and V of a
 * (trait, gene) are constants, so its statistic is a function of the pooled count a' = popc(gene & label) alone:
 * the table holds u(x) = 1 / (1 + stat(x)) in (0, 1] -- smaller is more extreme, 1.0 the identity of the minimum --
 * for every x of the support of a', in the CSR layout of scoary_minp_plan / _fill.
 *   scoary_cmh_minp_plan : per (trait, gene), with m_s = popc(gene & valid & stratum_s) and (k_s, n_s) = d_smargins,
 *       strata with n_s = 0 skipped: lo = sum max(0, k_s + m_s - n_s), hi = sum min(k_s, m_s).  d_lo int32 [T][G]
 *       = lo, d_off int64 [T * G + 1] = the exclusive prefix sum of hi - lo + 1 (the total last), *entries_out
 *       (HOST) = that total.  The strata plan and d_masks are scoary_cmh's; d_scratch = scoary_cmh_scratch_bytes(N)
 *       bytes (the segment table, rebuilt here).  Synchronises `stream` like scoary_minp_plan.  [lo, hi] lies
 *       inside the support scoary_minp_plan gives the same (trait, gene).
 *   scoary_cmh_minp_fill : d_tab double [entries]; with E2 = d_e2[t][g], V = d_var[t][g] as scoary_cmh wrote them,
 *       E2' = rint(E2) if |E2 - rint(E2)| <= 1e-6 else E2 (an exact tie a' + A = 2E needs an integer 2E; the fp64
 *       sum is off by up to 1.5e-8), every operation rounded on its own:
 *         D = |(double)x - 0.5 E2'|, y = min(0.5, D), stat = ((D - y)(D - y)) / V,
 *         d_tab[d_off[t G + g] + x - lo] = 1.0 / (1.0 + stat)          (1.0 when V == 0).
 *       entries may exceed 2^31; no scratch.  Asynchronous on `stream`, allocates nothing.
 * The observed value of a gene is ITS OWN table entry at x = d_a[t][g] (gathered, never recomputed), so an observed
 * and a permuted gene at the same count tie exactly.  Limits: S <= scoary_perm_max_strata(), N <=
 * scoary_perm_strata_max_isolates(), T <= 65535 (SCOARY_ERR_SIZE). */
int scoary_cmh_minp_plan(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_masks,
                         const uint16_t *d_strata, const int32_t *d_members, const int32_t *d_offsets,
                         const int32_t *d_smargins, int64_t G, int64_t T, int64_t N, int64_t S,
                         void *d_scratch, int64_t *d_off, int32_t *d_lo, int64_t *entries_out,
                         scoary_stream_t stream);
int scoary_cmh_minp_fill(scoary_handle h, const double *d_e2, const double *d_var, const int64_t *d_off,
                         const int32_t *d_lo, int64_t T, int64_t G, int64_t entries, double *d_tab,
                         scoary_stream_t stream);
/* ---- Exact conditional test over the strata (spec S12 of DESIGN.md; additive, ABI 11) ---------------------
 * Under within-stratum shuffles (S9) every stratum's margins are fixed and its count is hypergeometric, so the
 * pooled count a' = popc(gene & label) of a (trait, gene) is distributed as the CONVOLUTION of the strata's
 * hypergeometrics.  k_cmh_exact builds that pmf f on the support [lo, hi] of scoary_cmh_minp_plan, in fp64 (every
 * stratum's pmf by the ratio recurrence outward from its mode and normalised to sum 1, strata in ascending order,
 * strata with n_s = 0 skipped; the summation order inside a convolution is the kernel's, so the results are held
 * to a tolerance -- 1e-12 absolute and relative -- not to the bit), and from it
 *   p(x) = min(1, sum{f(y) : f(y) <= (1 + 1e-7) f(x)} / sum f)    for every x of [lo, hi]
 * -- the two-sided exact conditional p under the probability-ordering rule with the relErr of R's fisher.test and
 * mantelhaen.test(exact = TRUE); with one stratum Fisher's exact test.
 *   d_a / d_crit : scoary_cmh's, int32 [T][G] and uint32 [T][G][2]
 *   d_off / d_lo / entries : scoary_cmh_minp_plan's (the rows are taken in its CSR order)
 *   d_p        : double [T][G] or NULL, p(d_a[t][g]) -- the gene's own table entry (read back from d_tab when there
 *                is one), so an observed and a permuted gene at the same count tie exactly
 *   d_p_region : double [T][G] or NULL, sum{f(x) : (uint32)(x - base) >= span} / sum f with (base, span) = d_crit,
 *                at most 1 and 1 for the region (0, 0): the exact mass of S10's rejection region, what
 *                (r_cmh + 1) / (P + 1) estimates
 *   d_tab      : double [entries] or NULL, p(x) at d_off[t G + g] + x - lo: the layout scoary_permute_minp /
 *                scoary_permute_stepdown gather from (smaller is more extreme, 1.0 the identity of the minimum)
 *   (not all three NULL.)  A support of one entry gives p = p_region = 1 and the table entry 1.0; below 1e-290 the
 *   tails may underflow and any value in [0, 1e-290] stands for the true one.
 *   d_scratch  : scoary_cmh_scratch_bytes(N) bytes (the segment table, rebuilt here)
 * Asynchronous on `stream`, allocates nothing; entries may exceed 2^31.  Limits: those of the strata plan, T <=
 * 65535, G <= 2^30 and N <= 8190, which scoary_cmh_exact_max_isolates reports (a support of at most 4096 entries:
 * the pmf of a gene is held in LDS) -- SCOARY_ERR_SIZE with a message, never a partial result. */
int64_t scoary_cmh_exact_max_isolates(void);
int scoary_cmh_exact(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_masks, const uint16_t *d_strata,
                     const int32_t *d_members, const int32_t *d_offsets, const int32_t *d_smargins, int64_t G,
                     int64_t T, int64_t N, int64_t S, const int32_t *d_a, const uint32_t *d_crit,
                     const int64_t *d_off, const int32_t *d_lo, int64_t entries, double *d_p, double *d_p_region,
                     double *d_tab, void *d_scratch, scoary_stream_t stream);
/* ---- Exact conditional odds ratio and confidence limits (spec S13 of DESIGN.md; additive, ABI 11) ------------
 * From the same pmf f of the pooled count (S12 steps 1 and 2, the same code) and the tilted family
 * f_psi(x) ~ f(x) psi^x, at the observed count A = d_a[t][g] of the support [lo, hi]:
 *   d_or    : double [T][G], the conditional maximum-likelihood estimate of the common odds ratio: E_psi[X] = A;
 *             0 when A = lo, +inf when A = hi
 *   d_or_lo : double [T][G], the lower confidence limit: P_psi(X >= A) = half; 0 when A = lo
 *   d_or_hi : double [T][G], the upper confidence limit: P_psi(X <= A) = half; +inf when A = hi
 *   half    : 0.5 * (1.0 - level), computed in double by the caller, 0 < half < 0.5
 * -- R's mantelhaen.test(exact = TRUE) (its estimate and conf.int); with one stratum fisher.test's.  A support of
 * one entry (no informative stratum) gives (nan, 0, +inf).  k_cmh_odds_exact solves the three monotone equations
 * in theta = log psi over [-700, 700] by safeguarded Newton steps on terms taken in the log domain; every finite
 * positive result is within 1e-12 relative of the exact root, the special values are exact, a root outside the
 * range is 0 or +inf.  Where f(A) < 1e-290 the values are unspecified, non-negative and not nan.
 *   d_a / d_off / d_lo / entries / d_scratch : as scoary_cmh_exact takes them (d_off is checked, not read)
 * Asynchronous on `stream`, allocates nothing.  Limits and errors: scoary_cmh_exact's. */
int scoary_cmh_exact_odds(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_masks,
                          const uint16_t *d_strata, const int32_t *d_members, const int32_t *d_offsets,
                          const int32_t *d_smargins, int64_t G, int64_t T, int64_t N, int64_t S,
                          const int32_t *d_a, const int64_t *d_off, const int32_t *d_lo, int64_t entries, double half,
                          double *d_or, double *d_or_lo, double *d_or_hi, void *d_scratch,
                          scoary_stream_t stream);
/* ---- Homogeneity of the odds ratios over the strata (spec S14 of DESIGN.md; additive, ABI 11) -----------------
 * The Breslow-Day test with Tarone's correction of the assumption every other CMH statistic makes: one common odds
 * ratio in all strata.  Per (trait, gene), with psi = d_odds[t][g] as scoary_cmh wrote it (read, never recomputed,
 * so the fitted tables belong to the printed odds ratio) and per stratum (k, n) = d_smargins, m = popc(gene & valid &
 * stratum), a = popc(gene & label & stratum): over the informative strata (n > 0, 0 < k < n, 0 < m < n; L of them,
 * ascending) x = the root of x (n - k - m + x) = psi (k - x) (m - x) inside the stratum's support,
 * w = 1/x + 1/(k - x) + 1/(m - x) + 1/(n - k - m + x), d = a - x; fp64, every operation rounded on its own.
 *   d_stat_bd     : double [T][G], sum d^2 w, the Breslow-Day statistic
 *   d_stat_tarone : double [T][G], max(stat_bd - (sum d)^2 / sum (1 / w), 0), Tarone's
 *   d_df          : int32 [T][G], L - 1
 *   d_p           : double [T][G], the chi-square upper tail of stat_tarone at df degrees of freedom: within 1e-10
 *                   relative of the true tail where that is >= 1e-290, any value in [0, 1e-290] below
 *   psi nan, 0 or +inf, or L < 2: (nan, nan, 0, 1), scoary_cmh's convention for a gene without a test.
 *   the strata plan, d_labels, d_masks, d_scratch: as scoary_cmh takes them (the segment table is rebuilt here)
 * Asynchronous on `stream`, allocates nothing.  Limits and errors: scoary_cmh's. */
int scoary_cmh_homogeneity(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_labels,
                           const uint32_t *d_masks, const uint16_t *d_strata, const int32_t *d_members,
                           const int32_t *d_offsets, const int32_t *d_smargins, int64_t G, int64_t T, int64_t N,
                           int64_t S, const double *d_odds, double *d_stat_bd, double *d_stat_tarone, int32_t *d_df,
                           double *d_p, void *d_scratch, scoary_stream_t stream);
/* ---- Quantitative traits: the rank-sum test with value permutations (spec S15 of DESIGN.md; additive, ABI 11) ----
 * A trait is a row of centred doubled midranks of a measured value, d_rc int16 [T][N] (Rc_i = R_i - (n + 1), 0 for
 * an isolate without a value), its validity bits d_valid uint32 [T][Wp] (vecrows, bits >= N ignored) and
 * d_tiesum int64 [T] = sum (tau^3 - tau) over its tie groups; the host ranks (exact double comparisons).  Per
 * (trait, gene): m = popc(gene & valid), D = sum of Rc over the isolates of the gene.
 *   scoary_ranksum_max_isolates()  16320: |Rc| <= 16319 splits into two signed bytes, Rc = 128 hi + lo
 *   scoary_ranksum        d_d, d_m int32 [T][G]; d_auc = 0.5 + D / (2 m (n - m)); d_p = erfc(z / sqrt 2),
 *                         z = max(0, |D| / 2 - 1/2) / sqrt(m (n - m) / 12 * f), f = n + 1 - tiesum / (n (n - 1)),
 *                         fp64, every operation rounded on its own (scipy.stats.mannwhitneyu, asymptotic, with
 *                         continuity).  n < 2, m = 0, m = n or f <= 0: (auc 0.5, p 1), and D is 0 by itself.
 *   scoary_ranksum_perm_generate   d_rows int16 [T][P][N]: the Rc rows of the permutations perm_base .. + P - 1 of
 *                         the traits trait_base .. + T - 1 under `seed`: the values shuffled over the valid isolates
 *                         by the order of 50 Philox bits | isolate (counter (i, pi, t, "SCOQ")), 0 where invalid
 *   scoary_ranksum_bfrag_bytes     bytes of the same rows as the B operand of scoary_permute_ranksum (0: bad size)
 *   scoary_ranksum_perm_generate_bfrag   d_bfrag: those rows in that form, hi and lo digit planes, permutation
 *                         p of the call in column p; K padded with zeros to whole chunks of 256 isolates.  Byte
 *                         order: [t][stage of 64 columns][K-step of 32 isolates][plane hi, lo][column tile of 32]
 *                         [lane of 64] x 16 bytes; lane l of a fragment = column 64 stage + 32 tile + (l & 31),
 *                         isolates 32 K-step + 16 (l >> 5) .. + 15, one signed byte each; every stage has all its
 *                         K-steps, 8 per chunk.  What the columns from P to the end of the last stage hold is not
 *                         specified, and scoary_permute_ranksum does not count them
 *   scoary_permute_ranksum  d_r[t][g] += #{p < P : |D_p| >= |d_dobs[t][g]|}, int32 [T][G], D_p the gene's sum over
 *                         permuted row p of d_bfrag (T traits, P permutations as generated), exact in integers on the
 *                         int8 matrix cores; the caller zeroes d_r before the first batch, batches add up
 * Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1 or negative base;
 * SCOARY_ERR_SIZE, with nothing written: N > scoary_ranksum_max_isolates(), T > 65535, G or P >= 2^31. */
int64_t scoary_ranksum_max_isolates(void);
int scoary_ranksum(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_rc, const uint32_t *d_valid,
                   const int64_t *d_tiesum, int64_t G, int64_t T, int64_t N, int32_t *d_d, int32_t *d_m,
                   double *d_auc, double *d_p, scoary_stream_t stream);
int scoary_ranksum_perm_generate(scoary_handle h, const int16_t *d_rc, const uint32_t *d_valid, int64_t T, int64_t N,
                                 int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed, int16_t *d_rows,
                                 scoary_stream_t stream);
int64_t scoary_ranksum_bfrag_bytes(int64_t N, int64_t P, int64_t T);
int scoary_ranksum_perm_generate_bfrag(scoary_handle h, const int16_t *d_rc, const uint32_t *d_valid, int64_t T,
                                       int64_t N, int64_t P, int64_t perm_base, int64_t trait_base, uint64_t seed,
                                       void *d_bfrag, scoary_stream_t stream);
int scoary_permute_ranksum(scoary_handle h, const uint32_t *d_tiled, const void *d_bfrag, const int32_t *d_dobs,
                           int64_t G, int64_t T, int64_t N, int64_t P, int32_t *d_r, scoary_stream_t stream);
/* ---- Categorical traits: the gene x K-class chi-square test with label permutations (spec S20 of DESIGN.md;
 * additive, ABI 11) ----
 * A trait is a row of class codes d_codes int16 [T][N] (1 .. K, 0 for an isolate without a label; the host numbers
 * the classes) and its class sizes d_nk int32 [T][8] over the isolates with a code (entries from K on are 0).  Per
 * (trait, gene): a_k = |gene & class k|, m = sum a_k, n = sum n_k, K' = #{k : n_k > 0}.
 *   scoary_categorical_max_classes()  8: eight 16-bit count fields in two 64-bit words
 *   scoary_categorical    d_a int32 [T][G][8] (the entries from K on are 0 for a sound row); d_m int32 [T][G];
 *                         d_x2 = (sum over n_k > 0, ascending k, of (double)(c_k c_k) / (double)n_k) /
 *                         ((double)m (double)(n - m)), c_k = n a_k - m n_k in int64 -- the Pearson chi-square of the
 *                         2 x K table without cancellation, fp64, every operation rounded on its own; d_p = the
 *                         chi-square upper tail of it at K' - 1 degrees of freedom (scoary_cmh_homogeneity's tail:
 *                         within 1e-10 relative of the true tail where that is >= 1e-290); d_v = sqrt(x2 / n),
 *                         Cramer's V.  n < 2, m = 0, m = n or K' < 2: (x2 0, p 1, v 0).
 *   scoary_permute_categorical  d_r[t][g] += #{p < P : S_p >= S_obs}, int32 [T][G], S = sum a_k^2 / n_k (X2 is
 *                         increasing in it), a^p the gene's table under row p of d_rows int16 [T][P][N] -- the code
 *                         rows shuffled by scoary_ranksum_perm_generate with d_codes in the place of d_rc -- and
 *                         a^obs = d_a as scoary_categorical wrote it.  Decided in integers: with d_w uint64 [T][8][2]
 *                         = the limbs (low, high) of w_k = lcm{n_k > 0} / n_k (0 where n_k = 0), the permutation
 *                         counts iff sum (a^p_k^2 - a^obs_k^2) w_k >= 0.  The caller zeroes d_r before the first
 *                         batch, batches add up.
 * A code read from a row is clamped into [0, 8] before it indexes anything (scoary_permute_categorical only compares
 * it with the classes): a bad row gives wrong numbers, never an access outside the buffers.  Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer or a size < 1;
 * SCOARY_ERR_SIZE, with nothing written: K outside [1, 8], N > scoary_ranksum_max_isolates() (the rows are the
 * rank-sum generator's), T > 65535, G or P >= 2^31. */
int64_t scoary_categorical_max_classes(void);
int scoary_categorical(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_codes, const int32_t *d_nk, int64_t G,
                       int64_t T, int64_t N, int64_t K, int32_t *d_a, int32_t *d_m, double *d_x2, double *d_p,
                       double *d_v, scoary_stream_t stream);
int scoary_permute_categorical(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_rows, const int32_t *d_a,
                               const int32_t *d_nk, const uint64_t *d_w, int64_t G, int64_t T, int64_t N, int64_t P,
                               int32_t *d_r, scoary_stream_t stream);
/* ---- Categorical traits over strata: the generalized Cochran-Mantel-Haenszel test of the 2 x K x S table with label
 * permutations within the strata (spec S21 of DESIGN.md; additive, ABI 11) ----
 * A trait is scoary_categorical's d_codes int16 [T][N] and d_nk int32 [T][8], and d_nsk int32 [T][S][8], the class
 * sizes inside every stratum (entries from K on are 0); the strata are d_strata uint16 [N] and d_members int32 [N] as
 * the CMH entry points take them.  Per (trait, gene): m_s = the gene's labelled isolates of stratum s, a_k = |gene &
 * class k| pooled, n_s = sum_k n_sk, klast = the last class with n_k > 0; the contrasts are the classes j < klast - 1
 * (0-based), at most 7.  In ascending s, fp64, every operation rounded on its own:
 *     E_k += (double)(m_s n_sk) / (double)n_s                                      (n_s >= 1)
 *     c = ((double)m_s (double)(n_s - m_s)) / (((double)n_s (double)n_s) (double)(n_s - 1))         (n_s >= 2)
 *     V_jk += c (double)B_sjk,  B_sjk = n_s n_sj [j = k] - n_sj n_sk in int64      (k <= j < 7)
 * LDL' without pivoting in class order, rows from klast - 1 on taken as zero: u_jk = V_jk - sum_{l<k} u_jl f_kl (l
 * ascending), f_jk = u_jk invp_k, p_j = V_jj - sum_{k<j} u_jk f_jk (k ascending); pivot j is skipped (invp_j = 0, so
 * every multiplier of its column is 0) iff p_j <= 1e-8 V_jj, else invp_j = 1.0 / p_j; df = the pivots kept.  The FORM
 * of a (trait, gene) is scoary_gcmh_form_doubles() = 35 doubles: E[7] (0 from klast - 1 on), f[21] (f_ij at
 * i (i - 1) / 2 + j), invp[7].  Q(a) = sum_j (y_j y_j) invp_j, y_i = ((double)a_i - E_i) - sum_{j<i} f_ij y_j, both in
 * ascending j.
 *   scoary_gcmh           d_a int32 [T][G][8], d_m int32 [T][G] (m = sum m_s), d_e double [T][G][8] (E of all eight
 *                         classes), d_form double [T][G][35], d_q = Q(a), d_df int32 [T][G], d_p = the chi-square
 *                         upper tail of Q at df degrees of freedom (scoary_cmh_homogeneity's tail; 1 for df = 0),
 *                         d_thr = Q (1 - 1e-6).  df = 0: the form is E and zeros, Q = 0, thr = 0.  d_scratch:
 *                         scoary_cmh_scratch_bytes(N) bytes, the segment table of the strata, built by the call
 *   scoary_permute_gcmh   d_r[t][g] += #{p < P : Q(a^p) >= thr}, int32 [T][G], a^p the gene's counts under row p of
 *                         d_rows int16 [T][P][N] -- the code rows shuffled within the strata by
 *                         scoary_vanelteren_perm_generate with the codes of the labelled isolates by (stratum,
 *                         isolate) as d_l -- d_form and d_thr as scoary_gcmh wrote them.  The same operations as
 *                         d_q's: an identical table gives identical bits.  The caller zeroes d_r before the first
 *                         batch, batches add up.
 * A code read from a row is clamped into [0, 8] before it indexes anything (scoary_permute_gcmh only compares it with
 * the classes), a stratum and a word read from the segment table are clamped into theirs, a class size below 0 counts
 * as 0: a bad plan or row gives wrong numbers, never an access outside the buffers.  Asynchronous on `stream`, nothing
 * is allocated.  SCOARY_ERR_ARG: null pointer or a size < 1; SCOARY_ERR_SIZE, with nothing written: K outside [1, 8],
 * S > scoary_perm_max_strata(), N > scoary_ranksum_max_isolates(), T > 65535, G or P >= 2^31. */
int64_t scoary_gcmh_form_doubles(void);
int scoary_gcmh(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_codes, const int32_t *d_nk,
                const int32_t *d_nsk, const uint16_t *d_strata, const int32_t *d_members, int64_t G, int64_t T,
                int64_t N, int64_t K, int64_t S, int32_t *d_a, int32_t *d_m, double *d_e, double *d_form, double *d_q,
                int32_t *d_df, double *d_p, double *d_thr, void *d_scratch, scoary_stream_t stream);
int scoary_permute_gcmh(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_rows, const double *d_form,
                        const double *d_thr, const int32_t *d_nk, int64_t G, int64_t T, int64_t N, int64_t P,
                        int32_t *d_r, scoary_stream_t stream);
/* ---- Categorical traits: Westfall-Young single-step maxT over the chi-square and the generalized CMH statistic
 * (spec S22 of DESIGN.md; additive, ABI 11) ----
 * The chi-square statistic of a cell (gene, row) with the table a_k, per trait with n = sum n_k and per gene with m =
 * sum a^obs_k:  s = (sum over ascending k of ((double)c_k (double)c_k) inv[k]) ivm,  c_k = n a_k - m n_k in int32,
 * inv[k] = 1.0 / (double)n_k where n_k > 0 and 0 where not, ivm = 1.0 / ((double)m (double)(n - m)) where the gene is
 * testable by scoary_categorical's rule and 0 where not; fp64, every operation rounded on its own; X2 in the reals
 * (not d_x2 bit for bit: that divides by n_k).  The generalized CMH statistic of a cell is Q(a) of scoary_gcmh, as
 * scoary_permute_gcmh computes it.
 *   scoary_cat_wy_prepare   d_inv double [T][8]; d_ivm, d_sobs, d_thr double [T][G]: s_obs = s of d_a
 *                           (scoary_categorical's) and thr = s_obs (1.0 - 1e-9), the comparison point of the
 *                           family-wise count: an exact X2_p >= X2_obs implies s_p >= thr
 *   scoary_permute_cat_wy   scoary_permute_categorical with the family-wise maxima in the same pass: d_r as there, bit
 *                           for bit, and d_maxs[t * maxs_stride + p] = max(what it held, max over g < G of s of the
 *                           cell (g, p)) for p < P -- d_maxs points at the batch's first column inside a double
 *                           [T][maxs_stride] array that the caller fills with zeros before the first batch; columns
 *                           at and past P are not written.  The maximum is exact and does not depend on the order the
 *                           blocks run in (a 64-bit unsigned atomic maximum on the bits of the non-negative double)
 *   scoary_permute_gcmh_wy  scoary_permute_gcmh in the same way: d_r as there, bit for bit, and d_maxs the maximum of
 *                           Q over the genes; the comparison point of the family-wise count is scoary_gcmh's d_thr
 * Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1, maxs_stride < P;
 * SCOARY_ERR_SIZE, with nothing written: K outside [1, 8], N > scoary_ranksum_max_isolates(), T > 65535, G or
 * P >= 2^31. */
int scoary_cat_wy_prepare(scoary_handle h, const int32_t *d_a, const int32_t *d_nk, int64_t G, int64_t T, int64_t K,
                          double *d_inv, double *d_ivm, double *d_sobs, double *d_thr, scoary_stream_t stream);
int scoary_permute_cat_wy(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_rows, const int32_t *d_a,
                          const int32_t *d_nk, const uint64_t *d_w, const double *d_inv, const double *d_ivm,
                          int64_t G, int64_t T, int64_t N, int64_t P, int32_t *d_r, double *d_maxs,
                          int64_t maxs_stride, scoary_stream_t stream);
int scoary_permute_gcmh_wy(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_rows, const double *d_form,
                           const double *d_thr, const int32_t *d_nk, int64_t G, int64_t T, int64_t N, int64_t P,
                           int32_t *d_r, double *d_maxs, int64_t maxs_stride, scoary_stream_t stream);
/* ---- Categorical traits: Westfall-Young step-down maxT over the chi-square and the generalized CMH statistic
 * (spec S23 of DESIGN.md; additive, ABI 11) ----
 * S22's statistic s of a cell with the genes of a trait walked in rank order: order[t][k] = the gene at rank k of trait
 * t, ranks by descending comparison point thr (scoary_cat_wy_prepare's d_thr, or scoary_gcmh's) and ascending gene
 * index among equals: one stable descending sort of thr, made by the caller.  u[k] of a permuted row = the maximum of s
 * over the genes at the ranks k and behind, 0.0 behind the last.
 *   scoary_cat_stepdown_scratch_bytes   the size of d_scratch for batches of up to P permutations of the chi-square
 *       test (gcmh = 0) or the generalized CMH test (gcmh = 1).  With Gs = G rounded up to 1024 and Qs = ceil(ceil(N /
 *       32) / 4), in this order: rows uint32 [T][Qs][Gs][4], a tiled matrix per trait by POSITION -- position 1024 sg +
 *       64 i + 4 w + j holds rank 1024 sg + 64 w + 4 i + j (i, w < 16, j < 4) --; then per position, gcmh = 0: a_obs
 *       int32 [T][Gs][8], ivm double [T][Gs], thr double [T][Gs]; gcmh = 1: form double [T][Gs][35], thr double [T][Gs];
 *       then gmax double [T][Gs / 64][64 ceil(P / 64)].  Everything before gmax does not depend on P.
 *   scoary_cat_stepdown_gather          once per analysis, chi-square: the rows and per-position values from d_tiled,
 *       d_order int32 [T][G], d_a (scoary_categorical's), d_ivm and d_thr (scoary_cat_wy_prepare's).  A position whose
 *       rank is >= G holds a zero row, zeros and thr = +inf; an entry of d_order outside [0, G) makes such a position
 *       too (its rank is counted like any other: s = 0 in every row, u >= +inf never).
 *   scoary_gcmh_stepdown_gather         the same for the generalized CMH test: d_form and d_thr are scoary_gcmh's.
 *   scoary_permute_cat_stepdown         one batch of P permutations -- d_rows int16 [T][P][N], the columns perm_base ..
 *       perm_base + P - 1 -- in three launches on `stream`: d_r_rank[t * G + k] += scoary_permute_categorical's count of
 *       the gene at rank k (d_nk, d_w as there), d_c_rank[t * G + k] += #{columns < P : u[k] >= thr of rank k}, doubles
 *       compared exactly, and d_maxs[t * maxs_stride + perm_base + p] = u[0] of column p < P -- written, not combined,
 *       and equal to scoary_permute_cat_wy's maximum bit for bit (d_inv: scoary_cat_wy_prepare's).  d_maxs is the whole
 *       double [T][maxs_stride] array.  The caller zeroes d_r_rank and d_c_rank (int32 [T][G]) before the first batch.
 *   scoary_permute_gcmh_stepdown        the same with s = Q under the position's form and the rows shuffled within the
 *       strata: d_r_rank adds scoary_permute_gcmh's count, d_maxs is scoary_permute_gcmh_wy's.
 * Ranks at and past G and columns at and past P reach none of d_r_rank, d_c_rank, d_maxs; their cells of gmax hold
 * anything.  No block waits for another and gmax has one writer per cell; the counts are integer atomic additions.
 * Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1, perm_base < 0, maxs_stride
 * < perm_base + P; SCOARY_ERR_SIZE, with nothing written: N > scoary_ranksum_max_isolates(), T > 65535, G >= 2^31 -
 * 1024, P >= 2^31, a grid past 2^31 - 1 blocks.  scoary_cat_stepdown_scratch_bytes returns 0 for a null handle, a
 * size < 1 or such a G. */
int64_t scoary_cat_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P, int64_t gcmh);
int scoary_cat_stepdown_gather(scoary_handle h, const uint32_t *d_tiled, const int32_t *d_order, const int32_t *d_a,
                               const double *d_ivm, const double *d_thr, int64_t G, int64_t T, int64_t N,
                               void *d_scratch, scoary_stream_t stream);
int scoary_gcmh_stepdown_gather(scoary_handle h, const uint32_t *d_tiled, const int32_t *d_order, const double *d_form,
                                const double *d_thr, int64_t G, int64_t T, int64_t N, void *d_scratch,
                                scoary_stream_t stream);
int scoary_permute_cat_stepdown(scoary_handle h, void *d_scratch, const int16_t *d_rows, const int32_t *d_nk,
                                const uint64_t *d_w, const double *d_inv, int64_t G, int64_t T, int64_t N, int64_t P,
                                int64_t perm_base, int32_t *d_r_rank, int32_t *d_c_rank, double *d_maxs,
                                int64_t maxs_stride, scoary_stream_t stream);
int scoary_permute_gcmh_stepdown(scoary_handle h, void *d_scratch, const int16_t *d_rows, const int32_t *d_nk,
                                 int64_t G, int64_t T, int64_t N, int64_t P, int64_t perm_base, int32_t *d_r_rank,
                                 int32_t *d_c_rank, double *d_maxs, int64_t maxs_stride, scoary_stream_t stream);
/* ---- Covariate-adjusted score tests: the logistic and the linear Rao score test of a gene next to up to eight
 * covariates (spec S24 of DESIGN.md; additive, ABI 11) ----
 * The host fits the null model of a trait (intercept and covariates, no gene) over its valid isolates and hands over
 * d_rows double [T][q + 1][N] -- row 0 the residuals r_i, row 1 + j the weighted design column z_ij = w_i x_ij (j < q;
 * x_i0 = 1, so row 1 holds the weights), every row 0.0 at an isolate outside the valid set --, the validity bits
 * d_valid uint32 [T][Wp], d_chol double [T][q (q + 1) / 2] = the lower Cholesky factor L of A = sum w_i x_i x_i',
 * packed by rows, and for the linear kind d_rss double [T] = the null model's residual sum of squares (not read and
 * may be null for linear = 0).  Per (trait, gene), n = popc(valid), fp64, every operation rounded on its own:
 *     m = popc(gene & valid);  U = sum r_i, b_j = sum z_ij over the gene's valid isolates in ascending isolate order,
 *     each a running sum from +0.0;  L u = b by forward substitution (s = b_i; s = s - L_ij u_j for ascending j < i;
 *     u_i = s / L_ii; ascending i);  Vg = b_0 - (sum of u_j u_j from 0.0 in ascending j)
 *     testable: 0 < m < n and Vg > 2^-26 b_0 (and, linear, df = n - q - 1 >= 1); else (stat 0, beta 0, se 0, p 1)
 *     beta = U / Vg
 *     linear = 0:  stat = (U U) / Vg, se = 1 / sqrt(Vg), p = the chi-square upper tail of stat at one degree of
 *                  freedom (scoary_cmh_homogeneity's tail)
 *     linear = 1:  RSS1 = rss - (U U) / Vg;  se = sqrt((RSS1 / df) / Vg), stat = t = beta / se, p = the two-sided tail
 *                  of Student's t at df (within 1e-10 relative of the true tail above 1e-290).  RSS1 <= 0: se 0,
 *                  t = +inf or -inf by the sign of U and p 0, or (t 0, p 1) where U = 0
 *   scoary_score_max_covariates()  8: q = 1 + covariates is in [1, 9]
 *   scoary_score          d_m int32 [T][G]; d_u, d_vg, d_stat, d_beta, d_se, d_p double [T][G]; d_b double [T][G][q]
 * Only isolates below N with their validity bit enter any sum.  Asynchronous on `stream`, nothing is allocated.
 * SCOARY_ERR_ARG: null pointer, a size < 1, linear not 0 or 1; SCOARY_ERR_SIZE, with nothing written: q outside [1, 9],
 * T > 65535, G or N >= 2^31. */
int64_t scoary_score_max_covariates(void);
int scoary_score(scoary_handle h, const uint32_t *d_tiled, const double *d_rows, const uint32_t *d_valid,
                 const double *d_chol, const double *d_rss, int64_t G, int64_t T, int64_t N, int64_t q, int64_t linear,
                 int32_t *d_m, double *d_u, double *d_b, double *d_vg, double *d_stat, double *d_beta, double *d_se,
                 double *d_p, scoary_stream_t stream);
/* ---- The saddlepoint-corrected p of the logistic score test (spec S25 of DESIGN.md; additive, ABI 11) ----
 * Runs behind scoary_score with linear = 0, on its outputs d_u, d_b, d_vg, d_stat, d_p as they are, its d_rows (only
 * row 1 of a trait, the weights w_i = mu_i (1 - mu_i), is read), d_valid and d_chol, and d_spa_rows double
 * [T][q + 1][N]: row 0 the fitted mu_i of the null model, row 1 + j the scaled design column x_ij (row 1 is ones).
 * Per (trait, gene), values and not bits (exp and log1p on the device are not libm's):
 *     stat < cutoff2:  status 0, spa_p = the bits of d_p, z = t = 0, nothing else is computed
 *     else  c = A^-1 b (L u = b, L' c = u), g~_i = g_i - sum_j x_ij c_j over the valid isolates, and the two tails
 *           of S = sum g~_i (y_i - mu_i) at x = +|U| and x = -|U|: 0 beyond the end of S's support, the point mass
 *           at the end itself (within 1e-9 relative), else 1/2 erfc(|z| / sqrt 2) with z = omega + log(v / omega) /
 *           omega, omega = sign(t^) sqrt(2 (t^ x - K(t^))), v = t^ sqrt(K''(t^)), at the root t^ of K'(t) = x (within
 *           1e-10 relative), K the cumulant generating function of S;  status 1, spa_p = min(1, upper + lower tail)
 *           status 2, spa_p = the bits of d_p:  a side's search did not end within 60 evaluations, or t^ x - K, K'' or
 *           v / omega is not positive and finite, or z has not the sign of x (z and t then hold what the sides left)
 *   d_spa_p double [T][G]; d_spa_z, d_spa_t double [T][G][2] (side 0: x = +|U|, side 1: x = -|U|; z = 0 and t = +inf
 *   / -inf on a side that is a point mass or beyond the support); d_spa_status int32 [T][G]
 *   scoary_score_spa_max_isolates()     65 536: a pair is one wavefront's walk over the isolates
 *   scoary_score_spa_scratch_bytes(G, T)  the bytes of d_scratch, which is aligned to 8 bytes (a counter, the work
 *                                         list, four doubles a pair; 0 for sizes refused)
 * Only isolates below N with their validity bit enter any sum, whatever the rows hold elsewhere.  Asynchronous on
 * `stream`, nothing is allocated, no host round trip (the work list's length stays on the device).  SCOARY_ERR_ARG:
 * null pointer, d_scratch not aligned to 8 bytes, a size < 1, cutoff2 below 0.01 or not finite; SCOARY_ERR_SIZE,
 * with nothing launched and nothing written: q outside [1, 9], N above scoary_score_spa_max_isolates(), T > 65535,
 * G T >= 2^31. */
int64_t scoary_score_spa_max_isolates(void);
int64_t scoary_score_spa_scratch_bytes(int64_t G, int64_t T);
int scoary_score_spa(scoary_handle h, const uint32_t *d_tiled, const double *d_spa_rows, const double *d_rows,
                     const uint32_t *d_valid, const double *d_chol, const double *d_u, const double *d_b,
                     const double *d_vg, const double *d_stat, const double *d_p, int64_t G, int64_t T, int64_t N,
                     int64_t q, double cutoff2, double *d_spa_p, double *d_spa_z, double *d_spa_t,
                     int32_t *d_spa_status, void *d_scratch, scoary_stream_t stream);
/* ---- Quantitative traits over strata: the van Elteren test with value permutations within the strata (spec S16 of
 * DESIGN.md; additive, ABI 11) ----
 * The strata are d_strata uint16 [N] (the stratum of every isolate, in [0, S)) and d_members int32 [N] (the isolates
 * by (stratum, isolate)), as the CMH entry points take them.  The host ranks inside every stratum: a trait is its row
 * of scores d_score int16 [T][N], a_i = w_s Rc_i with Rc the centred doubled midrank inside the stratum and w_s =
 * max(1, floor(16319 / (n_s + 1))) (0 for an isolate without a value; |a| <= 16319), its validity bits d_valid
 * uint32 [T][Wp], d_wn int32 [T][S][2] = (w_s, n_s), d_c double [T][S] = w_s^2 f_s / 12 with f_s = n_s + 1 -
 * tiesum_s / (n_s (n_s - 1)) (0 for n_s < 2), and d_l int16 [T][N] = the scores of the valid isolates in (stratum,
 * isolate) order, the rest of the row 0.  Per (trait, gene): m_s = popc(gene & valid) inside stratum s, D = the sum
 * of the scores over the isolates of the gene.
 *   scoary_vanelteren     d_d, d_m int32 [T][G] (m = sum m_s); d_var = sum_s c_s (m_s (n_s - m_s)), fp64 in ascending
 *                         s, every operation rounded on its own; d_p = erfc(z / sqrt 2), z = (|D| / 2) / sqrt(var)
 *                         (no continuity correction); d_auc = 0.5 + D / (2 sum_s w_s m_s (n_s - m_s)).  var <= 0:
 *                         (auc 0.5, p 1), and D is 0 by itself.  d_scratch: scoary_cmh_scratch_bytes(N) bytes, the
 *                         segment table of the strata, built by the call
 *   scoary_vanelteren_perm_generate   d_rows int16 [T][P][N]: the score rows of the permutations perm_base .. + P - 1
 *                         of the traits trait_base .. + T - 1 under `seed`: the valid isolate whose composite
 *                         (stratum << (64 - b)) | (((key64 >> 14) >> b) << 14) | isolate has rank rho takes d_l[rho];
 *                         key64 = Philox words 0 and 1 of counter (i, pi, t, "SCOQ"), b = 0 for S = 1, else the bit
 *                         length of S - 1.  A shuffle within the strata; 0 where invalid
 *   scoary_vanelteren_perm_generate_bfrag   d_bfrag: those rows as the B operand of scoary_permute_ranksum, in
 *                         exactly the bytes scoary_ranksum_perm_generate_bfrag writes for the same rows
 *                         (scoary_ranksum_bfrag_bytes(N, P, T) of them), and the columns from P to the end of the
 *                         last stage as zeros: every byte of d_bfrag is written.  The exceedance counts are
 *                         scoary_permute_ranksum's, on d_d
 * Every index read from d_strata, d_members and the segment table is clamped: a bad plan gives wrong numbers, never
 * a wild access.  Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1 or negative
 * base; SCOARY_ERR_SIZE, with nothing written: S > scoary_perm_max_strata(), N > scoary_ranksum_max_isolates(),
 * T > 65535, G or P >= 2^31, perm_base + P or trait_base + T > 2^32 (the last counter words are those sums - 1). */
int scoary_vanelteren(scoary_handle h, const uint32_t *d_tiled, const int16_t *d_score, const uint32_t *d_valid,
                      const uint16_t *d_strata, const int32_t *d_members, const int32_t *d_wn, const double *d_c,
                      int64_t G, int64_t T, int64_t N, int64_t S, int32_t *d_d, int32_t *d_m, double *d_var,
                      double *d_auc, double *d_p, void *d_scratch, scoary_stream_t stream);
int scoary_vanelteren_perm_generate(scoary_handle h, const int16_t *d_l, const uint32_t *d_valid,
                                    const uint16_t *d_strata, int64_t T, int64_t N, int64_t S, int64_t P,
                                    int64_t perm_base, int64_t trait_base, uint64_t seed, int16_t *d_rows,
                                    scoary_stream_t stream);
int scoary_vanelteren_perm_generate_bfrag(scoary_handle h, const int16_t *d_l, const uint32_t *d_valid,
                                          const uint16_t *d_strata, int64_t T, int64_t N, int64_t S, int64_t P,
                                          int64_t perm_base, int64_t trait_base, uint64_t seed, void *d_bfrag,
                                          scoary_stream_t stream);
/* ---- Quantitative traits: Westfall-Young single-step maxT over the rank statistics (spec S17 of DESIGN.md; additive,
 * ABI 11) ----
 * One statistic for the rank-sum test (S15, cc = 1) and the van Elteren test (S16, cc = 0).  A cell (gene, row) with
 * the integer D has s = ((double)E * (double)E) * iv, E = max(0, |D| - cc), iv = 1 / var of the gene where it is
 * testable and 0 where not; fp64, every operation rounded on its own; 4 z^2 in the reals.
 *   scoary_ranksum_var      d_var double [T][G]: S15's var = (m (n - m) / 12) f of scoary_ranksum, operations in its
 *                           order, from d_m (scoary_ranksum's), the validity bits and the tie sums; 0 where the gene
 *                           is untestable.  (S16's var is scoary_vanelteren's d_var.)
 *   scoary_rank_wy_prepare  d_iv double [T][G] = 1 / var where var > 0, else 0; d_sobs double [T][G] = s of d_dobs
 *   scoary_permute_rank_wy  scoary_permute_ranksum with the family-wise maxima in the same pass: d_r as there, bit
 *                           for bit, and d_maxs[t * maxs_stride + p] = max(what it held, max over g < G of s of the
 *                           cell (g, p)) for p < P -- d_maxs points at the batch's first column inside a double
 *                           [T][maxs_stride] array that the caller fills with zeros before the first batch; columns
 *                           at and past P are not written, whatever d_bfrag holds there.  The maximum is exact and
 *                           does not depend on the order the blocks run in
 * Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1, cc not 0 or 1,
 * maxs_stride < P; SCOARY_ERR_SIZE, with nothing written: N > scoary_ranksum_max_isolates(), T > 65535, G or
 * P >= 2^31. */
int scoary_ranksum_var(scoary_handle h, const int32_t *d_m, const uint32_t *d_valid, const int64_t *d_tiesum,
                       int64_t G, int64_t T, int64_t N, double *d_var, scoary_stream_t stream);
int scoary_rank_wy_prepare(scoary_handle h, const double *d_var, const int32_t *d_dobs, int64_t cc, int64_t G,
                           int64_t T, double *d_iv, double *d_sobs, scoary_stream_t stream);
int scoary_permute_rank_wy(scoary_handle h, const uint32_t *d_tiled, const void *d_bfrag, const int32_t *d_dobs,
                           const double *d_iv, int64_t cc, int64_t G, int64_t T, int64_t N, int64_t P, int32_t *d_r,
                           double *d_maxs, int64_t maxs_stride, scoary_stream_t stream);
/* ---- Quantitative traits: Westfall-Young step-down maxT over the rank statistics (spec S18 of DESIGN.md; additive,
 * ABI 11) ----
 * S17's statistic s with the genes of a trait walked in rank order: order[t][k] = the gene at rank k of trait t, ranks
 * by descending s_obs and ascending gene index among equals (one stable descending sort of scoary_rank_wy_prepare's
 * d_sobs, made by the caller).  u[k] of a permuted row = the maximum of s over the genes at the ranks k and behind.
 *   scoary_rank_stepdown_scratch_bytes  the size of d_scratch for batches of up to P permutations.  With Gp =
 *       scoary_tiled_genes(G), Qp = scoary_tiled_quads(N), in this order: rows uint32 [T][Qp][Gp][4] (a tiled matrix
 *       per trait, position k where the tiled matrix has gene k), ss double [T][Gp], iv double [T][Gp], |D_obs| int32
 *       [T][Gp], gmax double [T][Gp / 64][64 ceil(P / 64)].  Everything before gmax does not depend on P.
 *   scoary_rank_stepdown_gather         once per analysis: rows, ss, iv and |D_obs| from d_tiled, d_order int32 [T][G],
 *       d_sobs and d_iv (scoary_rank_wy_prepare's) and d_dobs.  The positions k >= G hold zero rows, iv 0, ss 0 and a
 *       threshold no |D| reaches; an entry of d_order outside [0, G) makes such a position too.
 *   scoary_permute_rank_stepdown        one batch of P permutations, the columns perm_base .. perm_base + P - 1, in
 *       three launches on `stream`: d_r_rank[t * G + k] += #{columns < P : |D| >= |D_obs|} of the gene at rank k
 *       (scoary_permute_ranksum's count by rank position), d_c_rank[t * G + k] += #{columns < P : u[k] >= ss[k]},
 *       doubles compared exactly, and d_maxs[t * maxs_stride + perm_base + p] = u[0] of column p < P -- written, not
 *       combined, and equal to scoary_permute_rank_wy's maximum bit for bit.  d_maxs is the whole double
 *       [T][maxs_stride] array.  The caller zeroes d_r_rank and d_c_rank (int32 [T][G]) before the first batch.
 *       Columns at and past P reach none of the three, whatever d_bfrag holds there; their cells of gmax hold anything.
 * No block waits for another and gmax has one writer per cell; the counts are integer atomic additions, as d_r's are.
 * Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size < 1, cc not 0 or 1, perm_base
 * < 0, maxs_stride < perm_base + P; SCOARY_ERR_SIZE, with nothing written: N > scoary_ranksum_max_isolates(),
 * T > 65535, G or P >= 2^31, a grid past 2^31 - 1 blocks.  scoary_rank_stepdown_scratch_bytes returns 0 for a
 * null handle or a size < 1. */
int64_t scoary_rank_stepdown_scratch_bytes(scoary_handle h, int64_t G, int64_t T, int64_t N, int64_t P);
int scoary_rank_stepdown_gather(scoary_handle h, const uint32_t *d_tiled, const int32_t *d_order,
                                const double *d_sobs, const double *d_iv, const int32_t *d_dobs, int64_t G, int64_t T,
                                int64_t N, void *d_scratch, scoary_stream_t stream);
int scoary_permute_rank_stepdown(scoary_handle h, void *d_scratch, const void *d_bfrag, int64_t cc, int64_t G,
                                 int64_t T, int64_t N, int64_t P, int64_t perm_base, int32_t *d_r_rank,
                                 int32_t *d_c_rank, double *d_maxs, int64_t maxs_stride, scoary_stream_t stream);
/* ---- Quantitative traits: the Hodges-Lehmann shift of the rank-sum test and its confidence limits (spec S19 of
 * DESIGN.md; additive, ABI 11) ----
 * The K = m (n - m) differences fl(x_i - x_j), carrier i minus non-carrier j over the isolates with a value, are never
 * written: their order statistics are selected exactly, by counting.
 *   scoary_ranksum_shift     d_xs double [T][N]: a trait's valid values ascending in its first n places (no NaN, no
 *                            -0.0, |x| <= 1e150; the places behind hold anything); d_pos int32 [T][N]: the isolate at
 *                            each sorted place (an entry outside [0, N) is clamped into it); d_valid, d_m, d_var:
 *                            scoary_ranksum's validity rows and m, scoary_ranksum_var's var; zq = the normal quantile
 *                            of 0.5 + level / 2.  Writes, [T][G]: d_ca int64 = floor(0.5 K - zq sqrt(var)) (at most
 *                            K / 2), d_shift = (d_(floor((K-1)/2)+1) + d_(floor(K/2)+1)) 0.5, d_lower = d_(ca) and
 *                            d_upper = d_(K+1-ca) where ca >= 1, else -inf and +inf.  An untestable gene (var = 0)
 *                            has (0, -inf, +inf, ca 0); a gene whose bits at d_pos do not count to its d_m -- a plan
 *                            of other values or genes -- has NaN in all three and ca 0.  A zero is +0.0.
 *   scoary_rank_shift_waves  the wavefronts of a block at N isolates (a trait's d_xs and every wavefront's lists
 *                            share the LDS): 16 while they fit, then 8, 4, 2, 1; 0 for an N the stage does not take
 * No block waits for another.  Asynchronous on `stream`, nothing is allocated.  SCOARY_ERR_ARG: null pointer, size
 * < 1, zq not positive and finite; SCOARY_ERR_SIZE, with nothing written: N > scoary_ranksum_max_isolates(),
 * T > 65535, G >= 2^31. */
int64_t scoary_rank_shift_waves(int64_t N);
int scoary_ranksum_shift(scoary_handle h, const uint32_t *d_tiled, const double *d_xs, const int32_t *d_pos,
                         const uint32_t *d_valid, const int32_t *d_m, const double *d_var, double zq, int64_t G,
                         int64_t T, int64_t N, double *d_shift, double *d_lower, double *d_upper, int64_t *d_ca,
                         scoary_stream_t stream);
int64_t scoary_permute_lists_scratch_bytes(int64_t G, int64_t T, int64_t N, int64_t P);
int scoary_permute_lists(scoary_handle h, const uint32_t *d_tiles, const uint32_t *d_lidx,
                         int64_t entries, const int32_t *d_lstart, const int32_t *d_lngroups,
                         const int32_t *d_lorder, const uint8_t *d_lflipped,
                         const uint32_t *d_crit, const uint32_t *d_lcrit,
                         const int32_t *d_margins, void *d_scratch,
                         int64_t G, int64_t T, int64_t N, int64_t P, uint32_t *d_r,
                         int accumulate, scoary_stream_t stream);

/* ---- matrix-core kernel for the long-list slots (N <= scoary_mfma_max_isolates() = 2048) ----
 * The list count is a 0/1 GEMM whose cost does not depend on the list length, so the slots with
 * the longest lists -- slots [0, k_split), the slot order is by descending length -- can take
 * v_mfma_f32_16x16x128_f8f6f4 (E2M1 operands, exact in fp32) instead of the list walk; d_r
 * stays bit-identical.
 *   scoary_mfma_panels_build : once per data set, after scoary_lists_plan: d_panels =
 *       scoary_mfma_panels_bytes(G, N) bytes, the minority rows of all list slots as A fragments
 *   scoary_mfma_bfrag_bytes  : the per-step B-operand buffer d_bfrag (caller-owned, like d_scratch)
 *   scoary_mfma_breakeven_entries : padded list length (d_lngroups * 16) at which the two kernels
 *       cost the same, from the two measured rates in scoary_mfma.hip
 *   scoary_set_mfma_route    : NONE / ALL / AUTO (the default) for this handle
 *   scoary_mfma_route        : host only -- the k_split scoary_permute_hybrid will accept: 0 (NONE,
 *       N > 2048, or fewer than one round of blocks over the CUs), G (ALL), or (AUTO) the whole
 *       number of 256-slot blocks that the two measured rates make cheapest -- the break-even
 *       length, moved to a block count that fills whole rounds over the CUs.  block_start: HOST
 *       int64 [ceil(G/256) + 1] = index entries in front of every 256-slot block
 *       (32 * d_lstart[256 b]) and the entry count last
 *   scoary_mfma_plan         : host only, no handle -- the launch plan of k_permute_mfma for the slots
 *       [0, k_split) of a (T, P) launch on num_cu CUs (the launch asks with the device's count):
 *       out[0] = 256-slot gene blocks, out[1] = R, the ranges the T * ceil(P/64) stages of a gene
 *       block are cut into, out[2] = L, the stages of a range (the last one may be shorter),
 *       out[3] = blocks = out[0] * out[1].  SCOARY_ERR_ARG on a non-positive size or out = NULL
 *   scoary_permute_hybrid   : scoary_permute_lists with the slots [0, k_split) on the matrix cores;
 *       routed_entries = index entries in front of slot k_split (32 * d_lstart[k_split]; sizes the
 *       list kernel's chunks).  k_split = 0 is scoary_permute_lists (d_panels / d_bfrag unused). */
#define SCOARY_MFMA_ROUTE_NONE 0
#define SCOARY_MFMA_ROUTE_ALL 1
#define SCOARY_MFMA_ROUTE_AUTO 2
int64_t scoary_mfma_max_isolates(void);
int64_t scoary_mfma_panels_bytes(int64_t G, int64_t N);
int64_t scoary_mfma_bfrag_bytes(int64_t N, int64_t P, int64_t T);
int64_t scoary_mfma_breakeven_entries(void);
int scoary_mfma_panels_build(scoary_handle h, const uint32_t *d_tiled, int64_t G, int64_t N,
                             const int32_t *d_order, const uint8_t *d_flipped, void *d_panels,
                             scoary_stream_t stream);
int scoary_set_mfma_route(scoary_handle h, int mode);
int64_t scoary_mfma_route(scoary_handle h, const int64_t *block_start, int64_t G, int64_t T,
                          int64_t N, int64_t P);
int scoary_mfma_plan(int num_cu, int64_t k_split, int64_t T, int64_t P, int64_t *out);
int scoary_permute_hybrid(scoary_handle h, const uint32_t *d_tiles, const uint32_t *d_lidx,
                          int64_t entries, const int32_t *d_lstart, const int32_t *d_lngroups,
                          const int32_t *d_lorder, const uint8_t *d_lflipped,
                          const uint32_t *d_crit, const uint32_t *d_lcrit,
                          const int32_t *d_margins, void *d_scratch,
                          int64_t G, int64_t T, int64_t N, int64_t P, uint32_t *d_r,
                          int accumulate, const void *d_panels, void *d_bfrag, int64_t k_split,
                          int64_t routed_entries, scoary_stream_t stream);
/* ---- B fragments written by the label generator (additive, ABI 11) -----------------------------
 * The generator holds a stage's label bits in LDS when it writes its tile rows, so it can write the
 * stage's B fragments as well and the conversion pass (k_mfma_bfrag) goes.
 *   scoary_perm_generate_tiles_bfrag_range / scoary_perm_generate_tiles_strata_bfrag_range : their
 *       namesakes without _bfrag, which ALSO write into d_bfrag (scoary_mfma_bfrag_bytes(N, P, T)
 *       bytes, of any content) the fragments of every stage of 64 permutations whose (trait, tile)
 *       lies in the range -- the bytes scoary_permute_hybrid would make of these tiles; stages of
 *       tiles outside the range are left as they are.  The tiles are those of the namesake, byte
 *       for byte.  SCOARY_ERR_SIZE (nothing written) unless N <= scoary_mfma_max_isolates()
 *   scoary_permute_hybrid_bfrag : scoary_permute_hybrid with bfrag_ready = 1 saying that d_bfrag
 *       already holds the fragments of d_tiles (a generator call above, same N, P, T, every tile):
 *       the conversion is skipped.  bfrag_ready = 0 is scoary_permute_hybrid. */
int scoary_perm_generate_tiles_bfrag_range(scoary_handle h, const uint32_t *d_masks,
                                           const int32_t *d_margins, int64_t T, int64_t N, int64_t P,
                                           int64_t perm_base, int64_t trait_base, uint64_t seed,
                                           int64_t first_tile, int64_t n_tiles, uint32_t *d_tiles,
                                           void *d_bfrag, scoary_stream_t stream);
int scoary_perm_generate_tiles_strata_bfrag_range(scoary_handle h, const uint32_t *d_masks,
                                                  const uint16_t *d_strata, const int32_t *d_members,
                                                  const int32_t *d_offsets, const int32_t *d_smargins,
                                                  int64_t T, int64_t N, int64_t S, int64_t P,
                                                  int64_t perm_base, int64_t trait_base, uint64_t seed,
                                                  int64_t first_tile, int64_t n_tiles,
                                                  uint32_t *d_tiles, void *d_bfrag,
                                                  scoary_stream_t stream);
int scoary_permute_hybrid_bfrag(scoary_handle h, const uint32_t *d_tiles, const uint32_t *d_lidx,
                                int64_t entries, const int32_t *d_lstart, const int32_t *d_lngroups,
                                const int32_t *d_lorder, const uint8_t *d_lflipped,
                                const uint32_t *d_crit, const uint32_t *d_lcrit,
                                const int32_t *d_margins, void *d_scratch,
                                int64_t G, int64_t T, int64_t N, int64_t P, uint32_t *d_r,
                                int accumulate, const void *d_panels, void *d_bfrag, int64_t k_split,
                                int64_t routed_entries, int bfrag_ready, scoary_stream_t stream);

/* ---- index lists of the list-driven kernel, built on the device -----------------
 * From the tiled gene matrix already in HBM (no host pass, no PCIe copy of the
 * lists): for every gene the positions of its MINORITY value (ones if popcount <=
 * N/2, else zeros: d_flipped[g] = 1), genes ordered by descending list length
 * (stable), lists padded to 16 entries (half a kernel step) and to the longest list of their wavefront
 * group, the lists of a group interleaved in pieces of `piece` entries, entries in
 * the bank-rotation order of spec S6 (the same layout
 * scoary_lists_build of include/scoary_io.h -- the checker -- produces on the host).
 *   scoary_lists_plan : popcount -> flip -> radix sort by length -> padded lengths
 *       and group bases (prefix sum).  Writes d_order (int32 [G], per list slot),
 *       d_start / d_ngroups (int32 [scoary_list_segments(N)][G]: per segment and list
 *       slot -- plain [G] for N <= 20479) and d_flipped (uint8 [G], per gene); *entries_out (HOST)
 *       = total number of 32-bit words of index array (= entries for N <= 20479).  Synchronises `stream` (the caller needs the
 *       count to allocate d_idx).
 *   scoary_lists_fill : d_idx = uint32 [entries + scoary_lists_slack_entries()],
 *       entry = position * row stride (the LDS byte offset of that isolate's label
 *       row), padding = N * row stride (the all-zero row).  Segmented lists (N > 20479,
 *       round 4): 16-BIT entries, two per word of d_idx -- entry = position - segment start
 *       (the kernel scales it to the LDS address), padding = the segment's own zero row (=
 *       the segment's row count); *entries_out then counts 32-bit WORDS of d_idx (half the
 *       number of entries), eight entries per lane and 16-byte index vector, the entries of a
 *       sub-list in grid-compaction order (scoary_listbuild.hip).
 *   d_scratch : scoary_lists_scratch_bytes(G, N) bytes, the SAME buffer in both calls
 *       (plan leaves the lengths and group bases in it). */
int64_t scoary_lists_scratch_bytes(int64_t G, int64_t N);
int64_t scoary_lists_slack_entries(void);
int scoary_lists_plan(scoary_handle h, const uint32_t *d_tiled, int64_t G, int64_t N,
                      void *d_scratch, int32_t *d_start, int32_t *d_ngroups, int32_t *d_order,
                      uint8_t *d_flipped, int64_t *entries_out, scoary_stream_t stream);
int scoary_lists_fill(scoary_handle h, const uint32_t *d_tiled, int64_t G, int64_t N,
                      const void *d_scratch, const int32_t *d_order, const uint8_t *d_flipped,
                      int64_t entries, uint32_t *d_idx, scoary_stream_t stream);

/* ======================================================================
 * Population-structure stage
 * ====================================================================== */

/* ---- pdist(zeroonesmatrix, 'hamming') at scoary/methods.py:627-628 -------
 * Pairwise Hamming COUNTS between the R rows of a tiled bit matrix (here the
 * rows are isolates and the N columns are the variable genes; build it with
 * scoary_tile_rows from the transposed presence matrix):
 *   d_out[i][j] = popcount(row_i XOR row_j)        int32 [R][R]
 * d_vecrows is the same matrix as vecrows [R][Wp] (the wave-uniform operand).
 * The caller divides by the number of columns to get the reference's
 * fractions. */
int scoary_hamming(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_vecrows,
                   int64_t R, int64_t N, int32_t *d_out, scoary_stream_t stream);

/* ---- UPGMA merge loop (scoary/methods.py:640-707, scoary/classes.py:68-196) ----
 * From the n x n Hamming counts (scoary_hamming) over ncols variable genes: the
 * reference's merge order -- distances count / ncols with the diagonal forced to
 * 1, repeatedly the cell with the smallest (value, position in the reference's
 * quad tree of 2x2 block minima), size-weighted averaging in the same fp64
 * operations.  Writes the n-1 merged index pairs (i keeps the new cluster, j is
 * retired) to d_merges[2*(n-1)] and 0 to d_status[0]; a non-zero status means
 * the degenerate case (a minimum >= 1 or on the diagonal, in which the
 * reference merges retired clusters): the caller then runs the host loop
 * (scoary_upgma_merges, include/scoary_io.h), which mirrors that.
 *   d_scratch : scoary_upgma_scratch_bytes(n) bytes */
int64_t scoary_upgma_scratch_bytes(int64_t n);
int scoary_upgma(scoary_handle h, const int32_t *d_counts, int64_t n, int64_t ncols, void *d_scratch,
                 int32_t *d_merges, int32_t *d_status, scoary_stream_t stream);

/* ---- bit gather: reorder the columns of bit rows --------------------------
 * d_out[r] bit k = d_rows[r] bit d_index[k]   (k < K; output rows are
 * uint32 [R][Wout], Wout = (K+31)/32, pad bits zero).  Used to bring gene rows
 * and permuted label rows into the tip order of a (pruned) tree. */
int scoary_gather_bits(scoary_handle h, const uint32_t *d_rows, int64_t R, int64_t Wsrc,
                       const int32_t *d_index, int64_t K, uint32_t *d_out,
                       scoary_stream_t stream);

/* ---- PhyloTree maxima: ConvertUPGMAtoPhyloTree, scoary/methods.py:1386-1402
 *      + PhyloTree/Tip, scoary/classes.py:199-592 ---------------------------
 * The binary tree is a stack program over its K tips (children order is
 * irrelevant to the result):  op >= 0: push tip `op`;  op == -1: merge the two
 * top entries;  op <= -2: merge the top entry with tip (-2 - op).
 * `stack_depth` = the deepest the stack gets (host computes it; <= 32).  K <= 32767
 * (pair counts are packed into 14-bit fields; more tips: SCOARY_ERR_SIZE).
 * Tip k of evaluation (g, l) is in state  (gene bit k of row g ? A : a) +
 * (label bit k of row l ? B : b); d_gene_bits uint32 [G][Wt], d_label_bits
 * uint32 [L][Wt], Wt = (K+31)/32.
 *   d_out : int32 [G][L][3] = max contrasting pairs, max supporting pairs,
 *           max opposing pairs (classes.py:246-249). */
int scoary_tree_pairs(scoary_handle h, const int32_t *d_ops, int64_t nops, int64_t stack_depth,
                      const uint32_t *d_gene_bits, const uint32_t *d_label_bits, int64_t G,
                      int64_t L, int64_t K, int32_t *d_out, scoary_stream_t stream);

/* ---- Permute with the reference's tree statistic, methods.py:1314-1369 ----
 * Same evaluation for L permuted label rows, reduced to the exceedance flag
 *   d_exceed[g][l] = Total_l > 0  &&  double(X_l)/double(Total_l) >= est_g,
 * X = supporting pairs if the OBSERVED tree has Pro >= Anti else opposing pairs
 * (methods.py:1333-1355); d_obs int32 [G][3] = observed (Total, Pro, Anti).
 * A permuted tree with Total == 0 (ZeroDivisionError in the reference) is 0.
 * The host applies the sequential estimator / early abort (methods.py:1360-1365)
 * to the flags. */
int scoary_tree_permute(scoary_handle h, const int32_t *d_ops, int64_t nops,
                        int64_t stack_depth, const uint32_t *d_gene_bits,
                        const uint32_t *d_label_bits, int64_t G, int64_t L, int64_t K,
                        const int32_t *d_obs, uint8_t *d_exceed, scoary_stream_t stream);

/* ---- --collapse: presence-pattern identity, scoary/methods.py:816-840, :981
 * 128-bit hash of every gene's presence pattern restricted to each trait's
 * valid isolates (row AND mask):  d_out uint64 [T][G][2].  Equal patterns give
 * equal hashes; the host groups by hash and confirms equality on the bit rows,
 * so a collision can cost time but never correctness. */
int scoary_row_hash(scoary_handle h, const uint32_t *d_tiled, const uint32_t *d_masks,
                    int64_t G, int64_t T, int64_t N, uint64_t *d_out, scoary_stream_t stream);

/* ---- result records for the one exchange step of the path --------------
 * The reference weaves per-gene result dicts back from its worker processes
 * (scoary/methods.py:1115-1122); here every rank packs its shard into fixed records and
 * one RCCL gather / all-gather moves them (scoary_amd/dist.py):
 *   d_rec[i] = { tpgp, tpgn, tngp, tngn, p lo, p hi, odds lo, odds hi, r, nstop }
 * (uint32 [M][10], bit patterns preserved) for the M = T * G_shard (trait, gene) pairs of
 * d_counts [M][4] / d_p / d_odds / d_r / d_nstop; d_r and d_nstop may be NULL (zeros). */
int scoary_pack_records(scoary_handle h, const int32_t *d_counts, const double *d_p,
                        const double *d_odds, const uint32_t *d_r, const uint32_t *d_nstop,
                        int64_t M, uint32_t *d_rec, scoary_stream_t stream);

/* ---- e: the exchange step itself, for hosts that do not go through torch.distributed ----------
 * (replaces the pickled result weave of scoary/methods.py:1115-1122.)  Gather to `root`:
 * every rank sends `bytes` bytes at d_send (its scoary_pack_records block); the root receives nranks
 * blocks into d_recv, rank r's at offset r * bytes (d_recv may be NULL elsewhere).  One RCCL group of
 * ncclSend / ncclRecv on `stream`, over xGMI inside a node; returns once the group is enqueued.
 *   comm    : the caller's ncclComm_t (as void*: this header does not include rccl.h)
 *   rccl_dl : dlopen handle of the RCCL instance `comm` was created with (a process can hold more
 *             than one librccl -- PyTorch ships its own); NULL: the one the loader already has,
 *             else "librccl.so.1".  libscoary_hip.so has no link-time dependency on RCCL.
 * scoary_amd itself issues the same exchange through torch.distributed (scoary_amd/dist.py). */
int scoary_gather(scoary_handle h, void *rccl_dl, void *comm, const void *d_send, void *d_recv,
                  int64_t bytes, int rank, int nranks, int root, scoary_stream_t stream);

/* ---- hipGraph capture ----------------------------------------------------------
 * Small workloads are launch-bound (BASELINE configs[1]: six kernels, 0.14 ms).
 * scoary_graph_begin puts `stream` into capture mode; every scoary_* call made on
 * that stream (and on streams forked from it by event waits) until
 * scoary_graph_end is recorded instead of executed.  The captured sequence must not
 * allocate, synchronise or read results back: use caller-owned buffers that stay
 * alive for as long as the graph is replayed (so: scoary_counts_planned with a plan
 * built beforehand, not the one-call scoary_counts, which takes temporary memory for
 * its plan).  scoary_graph_launch replays it.
 * Not available while per-kernel timing (scoary_set_timing) is on. */
typedef struct scoary_graph *scoary_graph_t;
int scoary_graph_begin(scoary_handle h, scoary_stream_t stream);
int scoary_graph_end(scoary_handle h, scoary_stream_t stream, scoary_graph_t *out);
int scoary_graph_launch(scoary_handle h, scoary_graph_t g, scoary_stream_t stream);
void scoary_graph_destroy(scoary_graph_t g);

/* Name + average device time (ms, hipEvent on `stream`) of the kernels the
 * last scoary_permute call launched; for bench.py's roofline line.  Costs a
 * stream sync; timing is recorded only after scoary_set_timing(h, 1). */
int scoary_set_timing(scoary_handle h, int enabled);
int scoary_last_kernel_ms(scoary_handle h, const char *kernel, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* SCOARY_HIP_H */
