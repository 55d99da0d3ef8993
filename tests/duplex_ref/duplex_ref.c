/*
 * duplex_ref.c — TEST-ONLY plain-C restatement of the duplex model of DESIGN.md ("Duplex folds"): ViennaRNA's duplexfold
 * as published (inter-strand pairs only, dangles = 2, interior loops up to MAXLOOP, DuplexInit once), the first-minimum
 * rule, the traceback and the duplexT record.  Written from that statement, not from the kernels: it shares no code with
 * scanfold_amd/csrc, only the parameter blob's layout (include/sf_params_blob.h).  tests/test_duplex_ref.py pins it by
 * exhaustive enumeration against tests/py_model.py.
 */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sf_params_blob.h"

#define MAXLEN 64
#define INF SF_INF
#define NONE INT_MAX

static sf_params_blob P;

/* The exterior-stem terms are used as ViennaRNA's get_scaled_params leaves them: never above 0. */
void dr_set_params(const void *blob) {
  int t, a, b;
  memcpy(&P, blob, sizeof P);
  for (t = 0; t < 8; t++)
    for (a = 0; a < 5; a++) {
      if (P.dangle5[t][a] > 0) P.dangle5[t][a] = 0;
      if (P.dangle3[t][a] > 0) P.dangle3[t][a] = 0;
      for (b = 0; b < 5; b++)
        if (P.mismatchExt[t][a][b] > 0) P.mismatchExt[t][a][b] = 0;
    }
}

static int code_of(uint8_t c) {
  if (c <= 4) return c;
  switch (c) {
    case 'A': case 'a': return 1;
    case 'C': case 'c': return 2;
    case 'G': case 'g': return 3;
    case 'U': case 'u': case 'T': case 't': return 4;
  }
  return 0;
}

static const int PAIR[5][5] = {
    /* N */ {0, 0, 0, 0, 0},
    /* A */ {0, 0, 0, 0, 5},
    /* C */ {0, 0, 0, 1, 0},
    /* G */ {0, 0, 2, 0, 3},
    /* U */ {0, 6, 0, 4, 0}};
static const int RTYPE[8] = {0, 2, 1, 4, 3, 6, 5, 7};

static int imin(int a, int b) { return a < b ? a : b; }

/* exterior stem: 5' neighbour a, 3' neighbour b of the pair; -1 = there is none */
static int ext_stem(int type, int a, int b) {
  int e = 0;
  if (a >= 0 && b >= 0) e = P.mismatchExt[type][a][b];
  else if (a >= 0) e = P.dangle5[type][a];
  else if (b >= 0) e = P.dangle3[type][b];
  if (type > 2) e += P.TerminalAU;
  return e;
}

/* E_IntLoop(n1, n2, type, type_2, si1, sj1, sp1, sq1) */
static int int_loop(int n1, int n2, int type, int type_2, int si1, int sj1, int sp1, int sq1) {
  int nl, ns, u;
  if (n1 > n2) { nl = n1; ns = n2; } else { nl = n2; ns = n1; }
  if (nl == 0) return P.stack[type][type_2];
  if (ns == 0) {
    int e = P.bulge[nl];
    if (nl == 1) e += P.stack[type][type_2];
    else {
      if (type > 2) e += P.TerminalAU;
      if (type_2 > 2) e += P.TerminalAU;
    }
    return e;
  }
  if (ns == 1) {
    if (nl == 1) return P.int11[type][type_2][si1][sj1];
    if (nl == 2) {
      if (n1 == 1) return P.int21[type][type_2][si1][sq1][sj1];
      return P.int21[type_2][type][sq1][si1][sp1];
    }
    return P.internal_loop[nl + 1] + imin(P.max_ninio, (nl - ns) * P.ninio) + P.mismatch1nI[type][si1][sj1] +
           P.mismatch1nI[type_2][sq1][sp1];
  }
  if (ns == 2) {
    if (nl == 2) return P.int22[type][type_2][si1][sp1][sq1][sj1];
    if (nl == 3) return P.internal_loop[5] + P.ninio + P.mismatch23I[type][si1][sj1] + P.mismatch23I[type_2][sq1][sp1];
  }
  u = nl + ns;
  return P.internal_loop[u] + imin(P.max_ninio, (nl - ns) * P.ninio) + P.mismatchI[type][si1][sj1] +
         P.mismatchI[type_2][sq1][sp1];
}

/* s1 / s2: ASCII or codes.  Returns Emin (NONE: no pair); *ri, *rj = duplexT's i, j; structure: >= n1 + n2 + 2 bytes or NULL */
int dr_fold(const uint8_t *a1, int n1, const uint8_t *a2, int n2, int *ri, int *rj, char *structure) {
  static __thread int c[MAXLEN + 1][MAXLEN + 2];
  int S1[MAXLEN + 2], S2[MAXLEN + 2];
  int i, j, k, l, Emin = INF, i_min = 0, j_min = 0;
  for (i = 1; i <= n1; i++) S1[i] = code_of(a1[i - 1]);
  for (j = 1; j <= n2; j++) S2[j] = code_of(a2[j - 1]);
  for (i = 1; i <= n1; i++)
    for (j = n2; j >= 1; j--) {
      int type = PAIR[S1[i]][S2[j]], E;
      c[i][j] = INF;
      if (!type) continue;
      c[i][j] = P.DuplexInit + ext_stem(type, i > 1 ? S1[i - 1] : -1, j < n2 ? S2[j + 1] : -1);
      for (k = i - 1; k > 0; k--) {
        for (l = j + 1; l <= n2; l++) {
          int type2, e;
          if ((i - k - 1) + (l - j - 1) > SF_MAXLOOP) break;
          type2 = PAIR[S1[k]][S2[l]];
          if (!type2) continue;
          e = c[k][l] + int_loop(i - k - 1, l - j - 1, type2, RTYPE[type], S1[k + 1], S2[l - 1], S1[i - 1], S2[j + 1]);
          if (e < c[i][j]) c[i][j] = e;
        }
      }
      E = c[i][j] + ext_stem(RTYPE[type], j > 1 ? S2[j - 1] : -1, i < n1 ? S1[i + 1] : -1);
      if (E < Emin) { Emin = E; i_min = i; j_min = j; }
    }
  if (Emin >= INF) {
    *ri = 0; *rj = 0;
    if (structure) strcpy(structure, "&");
    return NONE;
  }
  *ri = i_min < n1 ? i_min + 1 : n1;
  *rj = j_min > 1 ? j_min - 1 : 1;
  if (structure) {
    char st1[MAXLEN + 2], st2[MAXLEN + 2];
    int o = 0, traced;
    memset(st1, '.', sizeof st1);
    memset(st2, '.', sizeof st2);
    i = i_min; j = j_min;
    for (;;) {
      int type = PAIR[S1[i]][S2[j]];
      st1[i] = '('; st2[j] = ')';
      traced = 0;
      for (k = i - 1; k > 0 && !traced; k--)
        for (l = j + 1; l <= n2; l++) {
          int type2;
          if ((i - k - 1) + (l - j - 1) > SF_MAXLOOP) break;
          type2 = PAIR[S1[k]][S2[l]];
          if (!type2) continue;
          if (c[i][j] == c[k][l] + int_loop(i - k - 1, l - j - 1, type2, RTYPE[type], S1[k + 1], S2[l - 1], S1[i - 1], S2[j + 1])) {
            i = k; j = l; traced = 1;
            break;
          }
        }
      if (!traced) break;
    }
    /* i, j: the outermost pair; one more nucleotide on each strand if there is one */
    if (i > 1) i--;
    if (j < n2) j++;
    for (k = i; k <= *ri; k++) structure[o++] = st1[k];
    structure[o++] = '&';
    for (k = *rj; k <= j; k++) structure[o++] = st2[k];
    structure[o] = 0;
  }
  return Emin;
}

/* n pairs; row p at p * ld; structures: rows of `sld` bytes or NULL */
void dr_batch(const uint8_t *s1, const uint8_t *s2, int n, int ld, const int32_t *len1, const int32_t *len2, int32_t *e,
              int32_t *ri, int32_t *rj, char *structures, int sld, int nthreads) {
  int p;
#pragma omp parallel for schedule(dynamic, 64) num_threads(nthreads)
  for (p = 0; p < n; p++) {
    int a, b;
    e[p] = dr_fold(s1 + (size_t)p * ld, len1[p], s2 + (size_t)p * ld, len2[p], &a, &b, structures ? structures + (size_t)p * sld : NULL);
    ri[p] = a; rj[p] = b;
  }
}

/* k-mer pairs of one record: seq[jw : jw+kmer] (cut at L) against seq[kw : kw+kmer] */
void dr_pairs(const uint8_t *seq, int L, int kmer, const int32_t *jw, const int32_t *kw, long n, int32_t *e, int32_t *ri,
              int32_t *rj, int nthreads) {
  long p;
#pragma omp parallel for schedule(dynamic, 256) num_threads(nthreads)
  for (p = 0; p < n; p++) {
    int a, b, n1 = L - jw[p] < kmer ? L - jw[p] : kmer;
    e[p] = dr_fold(seq + jw[p], n1, seq + kw[p], kmer, &a, &b, NULL);
    ri[p] = a; rj[p] = b;
  }
}
