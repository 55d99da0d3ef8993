/*
 * scanfold_hip_long.h — whole-record folds past the window limit (SF_MAX_W), an extension of include/scanfold_hip.h
 * exported by the same library (libscanfold_hip.so).  Conventions as there: 0 or a negative sf_status, caller-owned host
 * buffers, the resident parameter set and base-pair span (sf_params_load, sf_set_max_bp_span).
 *
 * Kept out of scanfold_hip.h on purpose: that header is the contract the CPU twin of the C ABI implements symbol for
 * symbol, and the twin has no long fold.  Bind these symbols only where the loaded library exports them.
 *
 * sf_fold_long gives the MFE and its structure, sf_pf_long the partition function (ensemble free energy, centroid, ensemble
 * diversity) of the same whole record; sf_fold_long_batch is sf_fold_long for many sequences of any lengths side by side
 * (a record and its shuffles: the z-score of a sequence past SF_MAX_W), and sf_pf_long_batch is sf_pf_long for many
 * sequences, constraints and hints side by side (the three ensembles of --global_ensemble; fc.pf() over long fragments),
 * every row bit for bit what sf_pf_long returns for it.  sf_fold_banded is sf_fold_long under a base-pair span in banded
 * tables: memory and work linear in the record's length, records up to SF_MAX_BANDED nucleotides, the same bytes;
 * sf_pf_banded is sf_pf_long under a span in banded tables likewise, to rounding.  sf_fold_banded_batch is sf_fold_banded
 * for many sequences side by side (a genome and its shuffles under a span: the z-score of a record of any length).
 * Soft constraints (SHAPE) are not provided past SF_MAX_W.
 */
#ifndef SCANFOLD_HIP_LONG_H
#define SCANFOLD_HIP_LONG_H

#include "scanfold_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF_MAX_LONG 32767 /* longest sequence sf_fold_long accepts (int16 bracket partners of the constraint model) */

/* fc = RNA.fold_compound(seq, md); fc.hc_add_from_db(cons); fc.mfe() for one sequence of any length 1..SF_MAX_LONG
 * (ScanFold.py:1520-1539, --global_refold).  seq: L bytes as in scanfold_hip.h.  cons: L characters with the meaning of
 * sf_fold_constrained, or NULL.  db_out: L+1 bytes or NULL (energy only, no traceback).
 * Structures are those of the window kernels and of the oracle's traceback, byte for byte, at every length.
 * The DP tables live in device memory, allocated for the call and freed before it returns:
 *   12 * L (L+1) / 2 + ~80 L bytes  (5.4 GB at L = 29 903).
 * Not enough device memory: SF_ERR_HIP with the text in sf_last_hip_error().  Unbalanced brackets: SF_ERR_CONSTRAINT.
 * L < 1, L > SF_MAX_LONG, seq NULL: SF_ERR_BAD_ARG. */
int sf_fold_long(const uint8_t *seq, int L, const char *cons, int32_t *mfe_dcal_out, char *db_out);

/* Device-event times (ms) of the phases of the last successful sf_fold_long: the fill of c / fML (one launch per
 * diagonal), the exterior loop f5, and the traceback (0 when it was not asked for).  Any pointer may be NULL. */
int sf_fold_long_times(double *fill_ms, double *f5_ms, double *trace_ms);

#define SF_MAX_BANDED 4194304 /* longest sequence sf_fold_banded accepts (positions are int32; memory is the real limit) */
/* device memory of one sf_fold_banded call with band B = min(span, L): three int32 band tables and what is linear in L */
#define SF_BANDED_BYTES(L, B) (12 * (size_t)(L) * (size_t)(B) + 75 * (size_t)(L) + 4 * (size_t)(B) + 153)

/* sf_fold_long under the resident base-pair span S (sf_set_max_bp_span, S >= 1) with the tables stored as a band:
 * a cell (i, j) with j - i >= S can neither pair nor be read by a cell that can, so only the B = min(S, L) diagonals
 * 0 .. B-1 are kept and filled.  Energy and structure are those of sf_fold_long under the same span, byte for byte, at
 * every length both accept; this call also takes records past SF_MAX_LONG, up to SF_MAX_BANDED (bracket partners of the
 * constraint are int32 here).  seq, cons, mfe_dcal_out, db_out as for sf_fold_long.  S >= L is legal (B = L: a full fold
 * in banded storage).  B fill launches, then f5 in O(L B) and the traceback, each in one workgroup.
 * The tables live in device memory, allocated for the call and freed before it returns: SF_BANDED_BYTES(L, B) bytes, of
 * which 9 (L + 2) (the constraint's arrays) only with a constraint and 49 L + 97 (the traceback stack and the structure)
 * only with db_out, in at most seven allocations: 12 L B + 75 L + 4 B + 153
 * (218 MB at L = 29 903, S = 600; 3.6 GB at L = 500 000, S = 600).
 * No span set, L < 1, L > SF_MAX_BANDED, seq NULL: SF_ERR_BAD_ARG (without a span, call sf_fold_long).  Unbalanced
 * brackets: SF_ERR_CONSTRAINT, before anything is launched.  Not enough device memory: SF_ERR_HIP with the text in
 * sf_last_hip_error().  On any error no output is written. */
int sf_fold_banded(const uint8_t *seq, int L, const char *cons, int32_t *mfe_dcal_out, char *db_out);

/* Of the last successful sf_fold_banded: device-event times (ms) of the fill, the exterior loop f5 and the traceback (0
 * when it was not asked for), the band B it ran with and the number of fill launches (= B).  Any pointer may be NULL. */
int sf_fold_banded_times(double *fill_ms, double *f5_ms, double *trace_ms, int *band, int *fill_launches);

/* What sf_fold_banded would allocate for a record of L nucleotides under the span `span`: SF_BANDED_BYTES(L, min(span, L)).
 * Needs sf_init only; nothing is allocated.  L < 1, L > SF_MAX_BANDED, span < 1, bytes NULL: SF_ERR_BAD_ARG. */
int sf_fold_banded_bytes(int L, int span, size_t *bytes);

/* sf_fold_long for n sequences at once.  Row s of seqs (n rows of ld bytes) holds len[s] bytes, 1 <= len[s] <= SF_MAX_LONG
 * and <= ld; the rows may differ in length freely.  cons: NULL, or n rows of ld characters with the meaning of
 * sf_fold_constrained, row s holding len[s] of them; a row of '.' only is no constraint.  mfe_dcal_out: n energies.
 * db_out: n rows of ld + 1 bytes (row s: len[s] characters and a NUL), or NULL: energies only, no traceback and no memory
 * for it.  The resident parameter set and base-pair span apply.  Energies and structures are those of sf_fold_long, byte
 * for byte, whatever the order of the rows and however the call is chunked.
 * One fill launch per anti-diagonal covers every sequence of a chunk; a chunk holds as many consecutive rows as fit the
 * byte budget (each row counted as 12 * L (L+1) / 2 + 80 L bytes; always at least one row), and its tables are a few device
 * allocations made for the chunk and freed after it.  The budget is 8 GiB unless sf_set_long_batch_bytes changed it.
 * n == 0: SF_OK.  n < 0, a length < 1, > SF_MAX_LONG or > ld, seqs / len / mfe_dcal_out NULL with n > 0: SF_ERR_BAD_ARG.
 * Unbalanced brackets in any row: SF_ERR_CONSTRAINT.  Not enough device memory: SF_ERR_HIP with the text in
 * sf_last_hip_error().  On any error no output is written. */
int sf_fold_long_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, int32_t *mfe_dcal_out,
                       char *db_out);

/* Device-event times (ms) of the last successful sf_fold_long_batch, summed over its chunks: fill, f5, traceback (0 when it
 * was not asked for), and the number of chunks it ran as.  Any pointer may be NULL. */
int sf_fold_long_batch_times(double *fill_ms, double *f5_ms, double *trace_ms, int *chunks);

/* The byte budget of one chunk of sf_fold_long_batch, sf_fold_banded_batch and sf_pf_long_batch; 0 restores the default
 * (8 GiB). */
int sf_set_long_batch_bytes(size_t bytes);

/* sf_fold_banded for n sequences at once, under the resident base-pair span S (sf_set_max_bp_span, S >= 1).  seqs, n, ld,
 * len, cons, mfe_dcal_out, db_out exactly as for sf_fold_long_batch, with 1 <= len[s] <= SF_MAX_BANDED: ragged rows, a
 * constraint row of '.' only is no constraint, db_out NULL means energies only, no traceback and no memory for it.  Row s
 * lives in its own band of B_s = min(S, len[s]) diagonals.  Energies and structures are those of sf_fold_banded, byte for
 * byte, whatever the order of the rows and however the call is chunked (every value is an integer minimum).
 * One fill launch per diagonal d = 0 .. max B_s - 1 covers every row of a chunk (a row is absent from the launches
 * d >= B_s); then the exterior loop f5 and the traceback run in one workgroup per row, the rows side by side, where
 * sf_fold_banded has a single workgroup at work.  A chunk holds as many consecutive rows as fit the byte budget of
 * sf_set_long_batch_bytes (8 GiB by default), each row counted as SF_BANDED_BYTES(L, B_s), always at least one row, and no
 * more than keep rows * ceil(64 Lmax / 256) workgroups inside an int; its tables are a fixed number of device allocations
 * made for the chunk and freed after it, with one hairpin table of max B_s + 1 entries.  The constraints are parsed on the
 * host (int32 bracket partners).
 * n == 0: SF_OK.  No span set, n < 0, a length < 1, > SF_MAX_BANDED or > ld, seqs / len / mfe_dcal_out NULL with n > 0:
 * SF_ERR_BAD_ARG.  Unbalanced brackets in any row: SF_ERR_CONSTRAINT, before anything is launched.  Not enough device
 * memory: SF_ERR_HIP with the text in sf_last_hip_error().  On any error no output is written. */
int sf_fold_banded_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, int32_t *mfe_dcal_out,
                         char *db_out);

/* Of the last successful sf_fold_banded_batch, summed over its chunks: device-event times (ms) of the fill, the exterior
 * loop f5 and the traceback (0 when it was not asked for), the number of chunks, and the number of fill launches (a
 * chunk's is its max B_s).  Any pointer may be NULL. */
int sf_fold_banded_batch_times(double *fill_ms, double *f5_ms, double *trace_ms, int *chunks, int *fill_launches);

/* fc.pf(); fc.centroid(); fc.mean_bp_distance() — RNAfold -p — for one sequence of any length 1..SF_MAX_LONG
 * (ScanFoldFunctions.py:758-772, rna_refold).  seq, cons as for sf_fold_long; the resident parameter set (rescaled
 * temperature sets included) and base-pair span apply.  mfe_dcal_hint: NULL, or the sequence's MFE in dcal/mol under the same
 * model and constraint (sf_fold_long's), from which the per-nucleotide scale of the first attempt is taken; without it a fixed
 * estimate is used and a long record usually costs a second inside pass.  Outputs: the ensemble free energy (kcal/mol), the
 * mean base-pair distance 2 sum p (1 - p), the centroid (pairs with p > 0.5; L+1 bytes, or NULL) and its mean distance to
 * the ensemble.  Any output pointer may be NULL.  Two calls with the same arguments on the same device return bit-identical
 * results.  Agreement with sf_pf_batch / sf_fold_constrained at L <= SF_MAX_W is to rounding (sums in another order).
 * The tables live in device memory, allocated for the call and freed before it returns:
 *   56 * L (L+1) / 2 + ~60 L bytes  (25.0 GB at L = 29 903, 30.1 GB at SF_MAX_LONG).
 * Not enough device memory: SF_ERR_HIP with the text in sf_last_hip_error().  Unbalanced brackets: SF_ERR_CONSTRAINT.
 * L < 1, L > SF_MAX_LONG, seq NULL: SF_ERR_BAD_ARG.  The scaled tables left FP64's range on every attempt: SF_ERR_RANGE
 * (no output is written). */
int sf_pf_long(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double *ens_dG, double *mean_bp_dist,
               char *centroid_out, double *centroid_dist);

/* Of the last sf_pf_long that ran: device-event times (ms) of the inside passes (all attempts, q5 / q3 included) and of the
 * outside pass with the probabilities, the number of attempts, and the final per-nucleotide scale ln s.  Any pointer may be
 * NULL. */
int sf_pf_long_times(double *inside_ms, double *outside_ms, int *attempts, double *lns);

/* device memory of one sf_pf_banded call with band B = min(span, L): seven FP64 band tables and what is linear in L and B
 * (mantissas and exponents of q5 / q3, sequence, centroid, the constraint's 9 (L + 2); the powers of the scale and the
 * hairpin weights up to B; 64 KiB of partial sums) */
#define SF_PF_BANDED_BYTES(L, B) (56 * (size_t)(L) * (size_t)(B) + 35 * (size_t)(L) + 24 * (size_t)(B) + 65677)

/* sf_pf_long under the resident base-pair span S (sf_set_max_bp_span, S >= 1) with the tables stored as a band of
 * B = min(S, L) diagonals: a cell (i, j) with j - i >= S cannot pair, and no cell inside the band reads one outside it, so
 * the band holds the same sums as sf_pf_long's triangles.  Arguments, outputs and staging as for sf_pf_long (any output
 * pointer may be NULL; nothing reaches the caller unless the call succeeds); limits and argument errors as for
 * sf_fold_banded: 1 <= L <= SF_MAX_BANDED, S >= L is legal (B = L), the constraint's bracket partners are int32.
 * Memory is SF_PF_BANDED_BYTES(L, B) (1.0 GB at L = 29 903, S = 600, where sf_pf_long takes 25 GB; 16.8 GB at L = 500 000) and a pass costs about
 * L B^2 / 2 terms in B launches, where sf_pf_long's costs L^3 / 6.
 * The exterior loop (q5 / q3) carries a binary exponent per position, so it does not depend on one scale holding for L
 * nucleotides: records whose composition changes along their length, and records past SF_MAX_LONG, work.  The band tables
 * keep one per-nucleotide scale ln s: the first from mfe_dcal_hint as in sf_pf_long; an inside pass whose ln Z_s / L = eps
 * has |eps| B > 300 is repeated with ln s + eps (exact: the exterior loop cannot leave the range), one whose tables left
 * FP64 with ln s +- 700 / B; non-finite outputs of the outside pass re-centre once.  After 6 attempts: SF_ERR_RANGE, and no
 * output is written.  Known limit: the band tables need |g - ln s| B <~ 700 for the local growth g of ln Z per nucleotide,
 * everywhere along the record; a strongly heterogeneous record under a span of several thousand can end in SF_ERR_RANGE.
 * Two calls with the same arguments on the same device return bit-identical results; agreement with sf_pf_long under the
 * same span is to rounding (sums in another order), not bit for bit.
 * No span set, L < 1, L > SF_MAX_BANDED, seq NULL: SF_ERR_BAD_ARG.  Unbalanced brackets: SF_ERR_CONSTRAINT, before anything
 * is launched.  Not enough device memory: SF_ERR_HIP with the text in sf_last_hip_error(). */
int sf_pf_banded(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double *ens_dG, double *mean_bp_dist,
                 char *centroid_out, double *centroid_dist);

/* Of the last sf_pf_banded that ran: device-event times (ms) of the inside passes (all attempts, q5 / q3 included) and of
 * the outside passes with the probabilities, the number of attempts, the final per-nucleotide scale ln s, the band B, and
 * the number of diagonal launches over all attempts (B per inside pass, B - 4 per outside pass).  Any pointer may be NULL. */
int sf_pf_banded_times(double *inside_ms, double *outside_ms, int *attempts, double *lns, int *band, int *launches);

/* What sf_pf_banded would allocate for a record of L nucleotides under the span `span`: SF_PF_BANDED_BYTES(L, min(span, L)).
 * Needs sf_init only; nothing is allocated.  L < 1, L > SF_MAX_BANDED, span < 1, bytes NULL: SF_ERR_BAD_ARG. */
int sf_pf_banded_bytes(int L, int span, size_t *bytes);

/* One base pair of the sparse list of sf_pf_banded_probs: positions 1-based, i < j, p = its probability in the ensemble. */
typedef struct { int32_t i, j; double p; } sf_pair_prob;

/* sf_pf_banded with the base-pair probabilities brought out: the dot plot of RNAfold -p / RNAplfold, the probability that
 * a nucleotide is unpaired, and the positional entropy.  Arguments, limits, attempts and errors are sf_pf_banded's, and
 * ens_dG, mean_bp_dist, the centroid and centroid_dist are bit for bit what sf_pf_banded returns for the same arguments:
 * both run one host path, and the extraction reads the tables of the attempt that succeeded after its outside pass.
 * sf_pf_banded_times reports for this call what it reports for sf_pf_banded.  S >= L is legal (B = L): a short record gets
 * its unrestricted probabilities.
 * cutoff: a pair is listed when p >= cutoff; it must lie in (0, 1] (a NaN, 0, a negative value or one above 1:
 * SF_ERR_BAD_ARG before anything is launched).
 * unpaired_out[k-1] = clamp(1 - sum_j p(k, j) - sum_i p(i, k), 0, 1), L doubles.
 * entropy_out[k-1] = - sum p log2 p over the pairs of k - unpaired log2 unpaired, L doubles, in BITS, with 0 log 0 = 0 (the
 * Shannon entropy of "k pairs with ..., or with nothing").  No parity with another package's entropy track is claimed.
 * *n_pairs: the length of the pair list, which is staged in host memory owned by the library and read with
 * sf_pf_probs_pairs: every pair with p >= cutoff, ascending in i and then in j, p being the very double the centroid was
 * decided on (ob qb, a cell with qb = 0 skipped).  Since sum_j p(i, j) <= 1 a position has at most floor(1 / cutoff)
 * listed partners, so the list holds at most L * floor(1 / cutoff) / 2 records.
 * Any output pointer may be NULL; nothing reaches the caller, and the staged list does not change, unless the call
 * succeeds.  Two calls with the same arguments on the same device return the same bits in all three arrays.
 * Device memory on top of SF_PF_BANDED_BYTES(L, B), alive beside the band tables while the extraction runs: the rows' counts
 * (4 L) and 64-bit offsets (8 L), two vectors of L doubles (16 L) and the list (16 n), allocated once n is known:
 * 28 L + 16 n bytes, reported as measured by sf_pf_banded_probs_times.  The counts are scanned on the host. */
int sf_pf_banded_probs(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double cutoff,
                       double *ens_dG, double *mean_bp_dist, char *centroid_out, double *centroid_dist,
                       double *unpaired_out /* L */, double *entropy_out /* L */, size_t *n_pairs);

/* The pair list of the last successful sf_pf_banded_probs: copies its first min(cap, n) records to out and always reports
 * n (out may be NULL with cap 0; cap > 0 with out NULL: SF_ERR_BAD_ARG).  Before any successful call n = 0.  The list lives
 * until the next successful sf_pf_banded_probs or until the library is unloaded; a call that fails, for whatever reason,
 * leaves the previous list in place. */
int sf_pf_probs_pairs(sf_pair_prob *out, size_t cap, size_t *n);

/* Of the last successful sf_pf_banded_probs: the device-event time (ms) of the extraction's launches (per-nucleotide pass,
 * count, writing pass; the host's scan between them is left out), which sf_pf_banded_times's outside_ms does not contain;
 * the length of its list; and the device bytes it allocated on top of SF_PF_BANDED_BYTES.  Any pointer may be NULL. */
int sf_pf_banded_probs_times(double *extract_ms, size_t *n_pairs, size_t *extra_bytes);

/* ---- the maximum-expected-accuracy (MEA) structure of a pair list: RNAfold -p --MEA [gamma] ----
 * Inputs: a record length L; a list of pairs (i, j, p), 1-based, i < j, strictly ascending in (i, j) (sf_pair_prob, the list
 * sf_pf_banded_probs produces); L unpaired probabilities u; gamma > 0.
 * Score.  A structure S is a nested set of listed pairs in which every position has at most one partner;
 *   score(S) = sum over k unpaired in S of u_k + sum over (i, j) in S of w_ij,  w_ij = (2.0 * gamma) * p_ij,
 * w rounded once and stored: every later operation is an addition or a maximum of doubles, so no expression can be
 * contracted into an FMA and the result does not depend on how lanes are grouped.
 * Recurrences.  B = 1 + the largest j - i in the list (1 for an empty list).  For j - i < B
 *   M[i][j] = max( u_i + M[i+1][j] , max over listed (i, k) with k <= j of (w_ik + M[i+1][k-1]) + M[k+1][j] ),
 * M = 0 for j < i; for the record, from i = L down to 1,
 *   E[i] = max( u_i + E[i+1] , max over listed (i, k) of (w_ik + M[i+1][k-1]) + E[k+1] ),  E[L+1] = 0;
 * score = E[1].  The additions are associated exactly as written.
 * Traceback.  At a segment or suffix starting at i, position i is unpaired if the stored value equals the first candidate
 * bit for bit; otherwise i pairs with the smallest k whose candidate equals it.  With that rule the structure and the 64
 * bits of the score are a function of the inputs alone.
 * On the device: one fill launch per diagonal d = 0 .. B-1 over a table of L * B doubles stored by diagonals, the exterior
 * pass and the traceback in one workgroup each. */

/* device memory of the MEA that is linear in L and in the list's length n: the weights (8 n), E (8 (L + 2)), the traceback
 * stack (8 (L / 2 + 2)) and the structure (L + 1) */
#define SF_MEA_BYTES(L, n) (8 * (size_t)(n) + 9 * (size_t)(L) + 8 * ((size_t)(L) / 2) + 33)
/* device memory of one sf_mea_pairs call: the table M, the list (16 n), its rows' offsets and the unpaired vector (16 L),
 * and the linear part */
#define SF_MEA_PAIRS_BYTES(L, B, n) (8 * (size_t)(L) * (size_t)(B) + 16 * (size_t)(n) + 16 * (size_t)(L) + SF_MEA_BYTES(L, n))

/* MEA structure of a caller's list.  pairs: n records, strictly ascending in (i, j), 1 <= i < j <= L, p finite in [0, 1];
 * unpaired: L finite values in [0, 1]; gamma finite > 0.  mea_out: L + 1 bytes or NULL; mea_score or NULL.
 * A position may have any number of listed partners.  Needs sf_init only: neither parameters nor a span.
 * Device memory, allocated for the call and freed before it returns: SF_MEA_PAIRS_BYTES(L, B, n), B as above.
 * L < 1, L > SF_MAX_BANDED, pairs NULL with n > 0, unpaired NULL, gamma NaN, infinite or <= 0, a record out of order, with
 * i >= j, i < 1, j > L, or p outside [0, 1] or not finite, an unpaired value outside [0, 1] or not finite: SF_ERR_BAD_ARG
 * before anything is allocated on the device or launched.  Not enough device memory: SF_ERR_HIP with the text in
 * sf_last_hip_error().  Nothing reaches the caller unless the call succeeds. */
int sf_mea_pairs(int L, const sf_pair_prob *pairs, size_t n, const double *unpaired, double gamma,
                 char *mea_out, double *mea_score);

/* sf_pf_banded_probs, then the MEA structure of the list and unpaired vector it produced, from device memory.
 * The ten outputs it shares with sf_pf_banded_probs are bit for bit what that call returns for the same arguments (one host
 * path), the list is staged for sf_pf_probs_pairs in the same way, and sf_pf_banded_times / sf_pf_banded_probs_times report
 * for this call what they report for a probs call.  sf_mea_pairs on that list and vector returns the same structure and the
 * same score bits: both run one device path.
 * The table M is not a new allocation: it lives in the second of the seven band tables ("qb by columns"), all of which are
 * dead once the extraction has read ob and qb; the band of the list is at most the band of the call.  Device memory on top
 * of sf_pf_banded_probs's is SF_MEA_BYTES(L, n), reported by sf_mea_times.
 * Errors are sf_pf_banded_probs's, and gamma NaN, infinite or <= 0: SF_ERR_BAD_ARG before anything is allocated or launched.
 * Any output pointer may be NULL; nothing reaches the caller, and neither the staged list nor sf_mea_times's figures change,
 * unless the call succeeds. */
int sf_pf_banded_mea(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double cutoff, double gamma,
                     double *ens_dG, double *mean_bp_dist, char *centroid_out, double *centroid_dist,
                     double *unpaired_out, double *entropy_out, size_t *n_pairs, char *mea_out, double *mea_score);

/* of the last successful call of either: device-event ms of fill, exterior pass and traceback, the band B of the list,
 * the fill launches (one per diagonal, = B; the one launch that forms the weights before them is timed with the fill but
 * not counted), and the device bytes allocated for the MEA on top of what the call had anyway (sf_mea_pairs: all of
 * SF_MEA_PAIRS_BYTES; sf_pf_banded_mea: SF_MEA_BYTES).  Any pointer may be NULL. */
int sf_mea_times(double *fill_ms, double *ext_ms, double *trace_ms, int *band, int *fill_launches, size_t *extra_bytes);

/* One row of sf_pf_long_batch: sf_pf_long's three numbers, the final per-nucleotide scale ln s and the number of inside
 * passes the row took (what sf_pf_long_times reports for the row folded alone). */
typedef struct { double ens_dG, mean_bp_dist, centroid_dist, lns; int32_t attempts, reserved; } sf_pf_long_row;
#define SF_PF_LONG_NO_HINT INT32_MIN /* mfe_dcal_hint[s]: no MFE known for row s */

/* sf_pf_long for n sequences at once.  seqs, n, ld, len, cons exactly as for sf_fold_long_batch: ragged rows of
 * 1 <= len[s] <= SF_MAX_LONG and <= ld; cons NULL or n rows of ld characters, a row of '.' only being no constraint.
 * mfe_dcal_hint: NULL, or n values with the meaning of sf_pf_long's, SF_PF_LONG_NO_HINT where a row has none.
 * out: n records, or NULL.  centroid_out: n rows of ld + 1 bytes (row s: len[s] characters and a NUL), or NULL.
 * For every row ens_dG, mean_bp_dist, centroid_dist, the centroid, lns and attempts are bit for bit what sf_pf_long (and
 * sf_pf_long_times) gives for that sequence, constraint and hint on the same device, whatever else is in the call, in
 * whatever row order and however the call is chunked: a row's lane groups, its probability waves and the powers of its
 * scale are those of the single call.
 * One launch per anti-diagonal covers every row of a chunk, in the inside and in the outside pass.  Each row has its own
 * scale: after an inside pass only the rows whose ln Z_s left the range repeat it, the others wait for the outside pass.
 * A chunk holds as many consecutive rows as fit the byte budget of sf_set_long_batch_bytes (8 GiB by default), each row
 * counted as 56 * L (L+1) / 2 + 60 L bytes, always at least one row; its tables are a fixed number of device allocations
 * made for the chunk and freed after it.
 * n == 0: SF_OK.  n < 0, a length < 1, > SF_MAX_LONG or > ld, seqs / len NULL with n > 0: SF_ERR_BAD_ARG.  Unbalanced
 * brackets in any row: SF_ERR_CONSTRAINT, before anything is launched.  Not enough device memory: SF_ERR_HIP with the text
 * in sf_last_hip_error().  A row that used up its attempts: SF_ERR_RANGE.  On any error no output is written. */
int sf_pf_long_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, const int32_t *mfe_dcal_hint,
                     sf_pf_long_row *out, char *centroid_out);

/* Of the last successful sf_pf_long_batch, summed over its chunks: device-event times (ms) of the inside passes (q5 / q3
 * included) and of the outside and probability passes, the number of chunks, and the number of inside passes run (one per
 * chunk when no row needed another scale).  Any pointer may be NULL. */
int sf_pf_long_batch_times(double *inside_ms, double *outside_ms, int *chunks, int *inside_passes);

#ifdef __cplusplus
}
#endif
#endif
