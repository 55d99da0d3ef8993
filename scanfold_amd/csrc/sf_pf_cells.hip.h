// sf_pf_cells.hip.h — what the whole-record partition functions share: the weights of a cell, the lane-group scheme and the
// inside, probability and finishing passes, as function templates over the state T (SfPfLong of sf_pf_long.hip.h:
// triangular tables, also every row of sf_pf_long_batch.hip.h; SfPfBand of sf_pf_banded.hip.h: banded tables).  Not here:
//   * the exterior loop q5 / q3: one is a plain FP64 recurrence in one workgroup, the other a mantissa / exponent recurrence
//     in two, and the one shared sequential exterior loop this project tried (f5, profiles/long_shared) cost 12 %;
//   * the outside pass (sfpl_outside, sfpb_outside): one body for both layouts returned the same bits but cost
//     sf_pflong_outside_kernel 1.8 % of its time at 1 000 nt where 0.3 % was allowed (profiles/pf_cells_shared), so each
//     family keeps its own, on the helpers below.
//
// Recurrences: those in the header of sf_pf.hip.h (qb / qm1 / qm), FP64 throughout.  A cell is handled by a group of G lanes
// (a power of two <= 64) which take its terms round-robin, two accumulators each, and add their partial sums in a butterfly
// of __shfl_xor; a group walks cells group, group + ngroups, ...  The order of every sum is the same for both layouts and is
// fixed by (L, d, G, the launch's share of lanes) alone.
//
// T has S, hpx, sc, mlbs, L, qb, qbt, qm, qmt, qm1t, ob, part, out and cen with the meaning given at SfPfLong.  The templates
// see the layout of the tables and the place of Z_s only through six overloads declared beside each struct:
//   sfp_type(D, F, a, b)    pair type of (a, b) under the span limit and F's constraint, 0: cannot pair
//   sfp_row(F, i, j)        offset of [i][j] in a row-wise table (qb, qm, ob)
//   sfp_col(F, j, i)        offset of [i][j] in a column-wise table (qbt, qmt, qm1t)
//   sfp_colp(F, table, j)   p with p[i - 1] = table[i][j] for a column-wise table
//   sfp_xhi(F, i)           the largest j - i for which [i][j] is kept: L - i, or min(L - i, B - 1) in a band
//   sfp_z(F)                what ob qb is divided by for the pair probability: Z_s, or 1 where ob is stored over Z_s
// A sum without terms (n <= 0) still forms the pointers to where its first term would be and reads nothing; in a band they
// may lie outside the run of a row or column that is kept.
#pragma once
#include "sf_pf.hip.h"

template <class T>
__device__ __forceinline__ double sfp_hairpin(const SfDevParams *D, const SfDevParamsPF *X, const T &F, int i, int j, int type) {
  const int size = j - i - 1;
  if (size <= SF_MAX_W + 1) return sfx_hairpin(D, X, F.S, i, j, type);
  return F.hpx[size] * X->mismatchH[type][F.S[i + 1]][F.S[j - 1]];  // (no special hairpin is that long)
}
template <class T>
__device__ __forceinline__ double sfp_ext(const SfDevParamsPF *X, const T &F, int type, int i, int j) {
  return sfx_extloop(X, type, i > 1 ? F.S[i - 1] : -1, j < F.L ? F.S[j + 1] : -1);
}
// sum over the G lanes of a cell's group (every lane of the wave takes part)
__device__ __forceinline__ double sfpl_group_sum(double v, int G) {
  for (int m = G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// lanes per cell of a diagonal with `cells` cells whose longest sum has `terms` terms: fill the lane budget, at most one wave,
// and no more lanes than leave each some sixteen terms (four lanes for the interior loops of a short diagonal).  The host
// (sf_pf_long, sf_pf_banded) and the batched kernels (sf_pf_long_batch.hip.h) all size a group with this one function.
__host__ __device__ inline int pfl_group(size_t cells, int terms, size_t lanes) {
  int G = 1;
  while (G < 64 && (size_t)(2 * G) * cells <= lanes && 32 * G <= (terms > 64 ? terms : 64)) G *= 2;
  return G;
}
// waves of the probability pass of a sequence of L nt under a budget of `lanes` lanes: one per row of the table at most
__host__ __device__ inline int pfl_prob_waves(int L, size_t lanes) {
  return (size_t)L < lanes / 64 ? L : (int)(lanes / 64);
}

// The three passes below are functions of (F, the lane's position gt within its sequence's share of the launch, the share's
// size nl): the single kernels give a sequence the whole launch, those of sf_pf_long_batch.hip.h a run of workgroups.

// Diagonal d of the inside pass (d < B in a band).  Lane r = gt % G of group gt / G; a group takes cells group, group + ngroups, ...
template <class T>
__device__ __forceinline__ void sfp_inside(const T &F, int d, int G, size_t gt, size_t nl, const SfDevParams *__restrict__ D,
                                           const SfDevParamsPF *__restrict__ X) {
  const int L = F.L;
  const int r = (int)(gt % (size_t)G);
  const size_t group = gt / (size_t)G, ngroups = nl / (size_t)G;
  const size_t ncell = (size_t)(L - d);
  const size_t rounds = (ncell + ngroups - 1) / ngroups;  // the same for every lane: the butterflies stay convergent
  for (size_t it = 0; it < rounds; it++) {
    const size_t cell = group + it * ngroups;
    const bool valid = cell < ncell;
    const int i = (int)cell + 1, j = i + d;
    if (d < SFD_TURN + 1) {  // no pair and no multiloop this short (the same for every thread of the launch)
      if (valid && r == 0) {
        const size_t ro = sfp_row(F, i, j), co = sfp_col(F, j, i);
        F.qb[ro] = 0.0; F.qbt[co] = 0.0; F.qm[ro] = 0.0; F.qmt[co] = 0.0; F.qm1t[co] = 0.0;
      }
      continue;
    }
    double z = 0.0, ml = 0.0, m = 0.0;
    int type = 0;
    if (valid) {
      type = sfp_type(D, F, i, j);
      if (type) {
        if (r == 0) z = sfp_hairpin(D, X, F, i, j, type) * F.sc[d + 1];
        const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
        const int si1 = F.S[i + 1], sj1 = F.S[j - 1];
        for (int u1 = 0; u1 <= umax; u1++) {
          const int p = i + 1 + u1;
          const double *row = F.qb + sfp_row(F, p, p);  // row[q - p] = qb[p][q]
          for (int u2 = r; u2 <= umax - u1; u2 += G) {
            const int q = j - 1 - u2;
            const double v = row[q - p];
            if (v == 0.0) continue;
            const int t2 = sfp_type(D, F, p, q);
            if (!t2) continue;
            z += sfx_intloop(X, u1, u2, type, sfd_rtype(t2), si1, sj1, F.S[p - 1], F.S[q + 1]) * v * F.sc[u1 + u2 + 2];
          }
        }
        // multiloop closed by (i, j): sum_u qm[i+1][u-1] qm1[u][j-1], u = i+2+TURN .. j-TURN-2
        const double *a = F.qm + sfp_row(F, i + 1, i + 1);  // a[x] = qm[i+1][i+1+x]
        const double *b = sfp_colp(F, F.qm1t, j - 1);       // b[x] = qm1[x+1][j-1]
        const int n = j - SFD_TURN - 2 - (i + 2 + SFD_TURN) + 1;
        const double *aa = a + SFD_TURN, *bb = b + i + 1 + SFD_TURN;  // term x: u = i+2+TURN+x
        double s1 = 0.0;
        int x = r;
        for (; x + G < n; x += 2 * G) {
          ml += aa[x] * bb[x];
          s1 += aa[x + G] * bb[x + G];
        }
        if (x < n) ml += aa[x] * bb[x];
        ml += s1;
      }
      {
        // qm[i][j] = qm1[i][j] + sum_u (MLbase^(u-i) + qm[i][u-1]) qm1[u][j], u = i+1 .. j-TURN-1
        const double *a = F.qm + sfp_row(F, i, i);             // a[x] = qm[i][i+x]; term x (u = i+1+x) reads a[x]
        const double *b = sfp_colp(F, F.qm1t, j) + i;          // b[x] = qm1[i+1+x][j]
        const double *pw = F.mlbs + 1;                         // pw[x] = (MLbase/s)^(x+1)
        const int n = j - SFD_TURN - 1 - (i + 1) + 1;
        double s1 = 0.0;
        int x = r;
        for (; x + G < n; x += 2 * G) {
          m += (pw[x] + a[x]) * b[x];
          s1 += (pw[x + G] + a[x + G]) * b[x + G];
        }
        if (x < n) m += (pw[x] + a[x]) * b[x];
        m += s1;
      }
    }
    // (one butterfly for the pair's weight: the multiloop factor is the cell's, the same in every lane)
    if (type) z += ml * (X->MLclosing * sfx_mlstem(X, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) * F.sc[2]);
    z = sfpl_group_sum(z, G);
    m = sfpl_group_sum(m, G);
    if (valid && r == 0) {
      const size_t ro = sfp_row(F, i, j), co = sfp_col(F, j, i);
      const double qbij = type ? z : 0.0;
      double m1 = F.qm1t[sfp_col(F, j - 1, i)] * X->MLbase * F.sc[1];
      if (type) m1 += qbij * sfx_mlstem(X, type, i > 1 ? F.S[i - 1] : -1, j < L ? F.S[j + 1] : -1);
      const double qmij = m1 + m;
      F.qb[ro] = qbij; F.qbt[co] = qbij;
      F.qm1t[co] = m1;
      F.qm[ro] = qmij; F.qmt[co] = qmij;
    }
  }
}

// p = ob qb / sfp_z over every kept cell: the centroid's pairs (p > 0.5) and each wave's share of sum p(1-p) and of the
// centroid distance, into part[2 * wave]; a wave takes rows wave, wave + nwaves, ... and reads them contiguously.
template <class T>
__device__ __forceinline__ void sfp_prob(const T &F, size_t wave, size_t nwaves) {
  const int L = F.L, lane = threadIdx.x & 63;
  const double Z = sfp_z(F);
  double mbd = 0.0, cd = 0.0;
  for (size_t i = wave + 1; i <= (size_t)L; i += nwaves) {
    const double *po = F.ob + sfp_row(F, (int)i, (int)i), *pq = F.qb + sfp_row(F, (int)i, (int)i);
    const int xhi = sfp_xhi(F, (int)i);
    for (int x = SFD_TURN + 1 + lane; x <= xhi; x += 64) {
      const double q = pq[x];
      if (q == 0.0) continue;
      const double p = po[x] * q / Z;
      mbd += p * (1.0 - p);
      if (p > 0.5) {
        cd += 1.0 - p;
        F.cen[i - 1] = '(';
        F.cen[i - 1 + x] = ')';
      } else cd += p;
    }
  }
  mbd = sfpl_group_sum(mbd, 64);
  cd = sfpl_group_sum(cd, 64);
  if (lane == 0) { F.part[2 * wave] = mbd; F.part[2 * wave + 1] = cd; }
}

// The partial sums in wave order; one wave.
template <class T>
__device__ __forceinline__ void sfp_finish(const T &F, int nwaves) {
  const int tid = threadIdx.x;
  double mbd = 0.0, cd = 0.0;
  for (int w = tid; w < nwaves; w += 64) { mbd += F.part[2 * w]; cd += F.part[2 * w + 1]; }
  mbd = sfpl_group_sum(mbd, 64);
  cd = sfpl_group_sum(cd, 64);
  if (tid == 0) { F.out[1] = 2.0 * mbd; F.out[2] = cd; }
}
