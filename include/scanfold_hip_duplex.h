/*
 * scanfold_hip_duplex.h — duplex folds (RNA.duplexfold) and the long-range-interaction scan of ScanFold.py --lri, an
 * extension of include/scanfold_hip.h exported by the same library (libscanfold_hip.so).  Conventions as there: 0 or a
 * negative status, caller-owned host buffers, the resident parameter set (sf_params_load).
 *
 * Kept out of scanfold_hip.h for the reason scanfold_hip_long.h is: that header is the contract the CPU twin of the C ABI
 * implements symbol for symbol, and the twin has no duplex fold.  Bind these symbols only where the library exports them.
 *
 * The model (DESIGN.md "Duplex folds"): ViennaRNA's duplexfold — inter-strand pairs only, dangles = 2, interior loops up to
 * SF_MAXLOOP, DuplexInit once.  Emin is the FIRST strict minimum in the order i = 1..n1, j = n2..1.
 */
#ifndef SCANFOLD_HIP_DUPLEX_H
#define SCANFOLD_HIP_DUPLEX_H

#include "scanfold_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF_DUPLEX_MAX_LEN 64 /* longest strand of a duplex, and largest kmer of the scan (the traceback keeps each strand's
                                pairs in one 64-bit mask; the int16 table, with 32767 for "cannot pair", holds 64 stacked
                                pairs of -5 kcal/mol each: no table in use comes near that) */
#define SF_DUPLEX_STRUCT_LEN 132 /* bytes of one structure row: n1 + 1 + n2 characters and a NUL, padded */
#define SF_DUPLEX_NONE 2147483647 /* energy of two strands that cannot form a single pair (upstream leaves Emin at INF
                                     there); structure "&", i = j = 0 */
#define SF_DUPLEX_SKIPPED (-2147483647 - 1) /* dense scan: a (j_win, k_win) the reference's distance test leaves out */
#define SF_ERR_DUPLEX_HITS (-20) /* sf_lri_scan: more hits than max_hits; raise the capacity or lower the cutoff */

/* one pair below the cutoff: j_win, k_win are the 0-based starts of the two k-mers in the record */
typedef struct sf_lri_hit {
  int32_t j_win, k_win, energy_dcal, i, j;
} sf_lri_hit;

/* duplex = RNA.duplexfold(s1, s2) for n pairs (ScanFold.py:785; ScanFoldFunctions.py:824).  Row p of s1 / s2 starts at
 * byte p * ld and holds len1[p] / len2[p] nucleotides (ASCII or codes 0..4), 0 <= len <= SF_DUPLEX_MAX_LEN <= ld.
 * energy_out: Emin in dcal/mol or SF_DUPLEX_NONE; i_out / j_out: duplexT's .i / .j (1-based; 0 with SF_DUPLEX_NONE);
 * structure_out: NULL, or n rows of SF_DUPLEX_STRUCT_LEN bytes, NUL-terminated "((.((&)).))". */
int sf_duplex_batch(const uint8_t *s1, const uint8_t *s2, int n, int ld, const int32_t *len1, const int32_t *len2,
                    int32_t *energy_out, int32_t *i_out, int32_t *j_out, char *structure_out);

/* The (j_win, k_win) grid of ScanFold.py:773-783,1019-1024 on a record of L nucleotides: j_win = jx * step for jx < *n_j,
 * k_win = kx * step for kx < *n_k.  Both are 0 when L < kmer (the reference's single 0/0 iteration fails its distance test). */
int sf_lri_grid(int L, int kmer, int step, int32_t *n_j, int32_t *n_k);

/* The all-pairs k-mer duplex scan (ScanFold.py:773-812): every grid point with (k_win+3) < (j_win-kmer) or
 * k_win > (j_win+kmer+3) folds seq[j_win : j_win+kmer] (kmer-1 long at j_win = L-kmer+1) against seq[k_win : k_win+kmer].
 * Compacted mode (dense_e NULL): the pairs with Emin < cutoff_dcal go to hits_out (capacity max_hits), sorted by
 * (j_win, k_win); *n_hits_out is their number.  More than max_hits: SF_ERR_DUPLEX_HITS, *n_hits_out = the number needed,
 * hits_out untouched.  Dense mode (dense_e / dense_i / dense_j: n_j * n_k int32 each, row-major): every grid point's
 * (Emin, i, j), SF_DUPLEX_SKIPPED / 0 / 0 where the distance test fails; hits_out may be NULL then.
 * 2 <= kmer <= SF_DUPLEX_MAX_LEN (tables past the LDS budget, kmer > 35, live in device memory), step >= 1; anything else:
 * SF_ERR_BAD_ARG. */
int sf_lri_scan(const uint8_t *seq, int L, int kmer, int step, int32_t cutoff_dcal, int64_t max_hits, sf_lri_hit *hits_out,
                int64_t *n_hits_out, int32_t *dense_e, int32_t *dense_i, int32_t *dense_j);

/* Device-event time (ms) of the scan kernels of the last successful sf_lri_scan, and the duplexes they folded. */
int sf_lri_scan_time(double *ms, int64_t *duplexes);

/* energy_list = cofold_energies(frag, [dup_frag] + scramble(dup_frag, r, type)) for n_hits pairs (ScanFold.py:813-817;
 * ScanFoldFunctions.py:817-829): r + 1 energies per hit.  Element 0 folds the native seq[k_win : k_win+kmer], elements
 * 1..r its shuffles (kind: SF_SHUFFLE_MONO / SF_SHUFFLE_DI); strand 1 of EVERY element, 0 included, is a fresh mono shuffle
 * of seq[j_win : j_win+kmer] (ScanFoldFunctions.py:820).  Random stream: Philox4x32-10 keyed by (seed, j_win, k_win,
 * element), so a hit's row does not depend on the other hits of the call.  SF_DUPLEX_NONE energies are returned as they
 * are.  rows1_out / rows2_out: NULL, or n_hits * (r+1) rows of kmer codes (0..4; row of a short strand 1 zero-padded). */
int sf_lri_background(const uint8_t *seq, int L, int kmer, const int32_t *j_win, const int32_t *k_win, int n_hits, int r,
                      int kind, uint64_t seed, int32_t *energies_out, uint8_t *rows1_out, uint8_t *rows2_out);

#ifdef __cplusplus
}
#endif
#endif
