// sf_mfe_trace.hip.h — what the whole-record MFE folds share: the energy helpers of a cell and the traceback, as function
// templates over the fold's state T (SfLong of sf_mfe_long.hip.h: triangular tables, also every row of
// sf_mfe_long_batch.hip.h; SfBand of sf_mfe_banded.hip.h: banded tables).  The exterior loop f5 is not here: one body for
// both layouts cost sf_long_f5_kernel 6 VGPRs and 12 % of its time (profiles/long_shared), so each family keeps its own.
//
// T has S, hp, L, c, fML, fMLt, f5, stk, db and status with the meaning given at SfLong.  The templates see the layout of
// the tables only through six overloads declared beside each struct:
//   sft_type(D, F, a, b)    pair type of (a, b) under the span limit and F's constraint, 0: cannot pair
//   sft_row(F, i, j)        offset of [i][j] in the row-wise table (fML)
//   sft_col(F, j, i)        offset of [i][j] in the column-wise tables (c, fMLt)
//   sft_colp(F, table, j)   p with p[i] = table[i][j] for a column-wise table
//   sft_lo(F, j)            the smallest i for which [i][j] is kept: 1, or max(1, j - B + 1) in a band
//   sft_in(F, i, j)         [i][j] is kept: true, or j - i < B in a band
#pragma once
#include "sf_mfe_full.hip.h"

#define SF_LONG_STACK_INTS(L) (3 * (4 * (size_t)(L) + 8))  // traceback stack of one fold, int32 entries

template <class T>
__device__ __forceinline__ int sft_hairpin(const SfDevParams *D, const T &F, int i, int j, int type) {
  const int size = j - i - 1;
  if (size <= SF_MAX_W + 1) return sfd_hairpin(D, F.S, i, j, type);
  return F.hp[size] + D->P.mismatchH[type][F.S[i + 1]][F.S[j - 1]];  // (no special hairpin is that long)
}
template <class T>
__device__ __forceinline__ int sft_ext(const SfDevParams *D, const T &F, int type, int i, int j) {
  return sfd_extloop(D, type, i > 1 ? F.S[i - 1] : -1, j < F.L ? F.S[j + 1] : -1);
}
template <class T>
__device__ __forceinline__ int sft_mlstem_out(const SfDevParams *D, const T &F, int type, int i, int j) {
  return sfd_mlstem(D, type, i > 1 ? F.S[i - 1] : -1, j < F.L ? F.S[j + 1] : -1);
}
// interior loop (i, j) -> (p, q) with u1 / u2 unpaired bases; SFD_INF if (p, q) cannot pair
template <class T>
__device__ __forceinline__ int sft_intloop(const SfDevParams *D, const T &F, int i, int j, int type, int u1, int u2) {
  const int p = i + 1 + u1, q = j - 1 - u2;
  const int t2 = sft_type(D, F, p, q);
  if (!t2) return SFD_INF;
  return sfd_intloop(D, u1, u2, type, sfd_rtype(t2), F.S[i + 1], F.S[j - 1], F.S[p - 1], F.S[q + 1]) + F.c[sft_col(F, q, p)];
}

// Traceback in one workgroup (oracle/sf_oracle.c's mfe_traceback step by step).  Thread 0 keeps the stack and the nibbling
// loops; each search over candidates is spread over the workgroup and takes the first match in the oracle's order (a block
// minimum over the candidate's position in that order).  In a band every search is clipped to the cells that are kept.
template <class T>
__device__ __forceinline__ void sft_trace(const T &F, const SfDevParams *__restrict__ D) {
  __shared__ int red[16];
  __shared__ int sh_i, sh_j, sh_ml, sh_s, sh_bad, sh_pair;
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L;
  const sf_params_blob &P = D->P;
  const int32_t *f5 = F.f5;
  int32_t *stk = F.stk;
  for (int x = tid; x < L; x += nt) F.db[x] = '.';
  if (tid == 0) {
    F.db[L] = 0;
    stk[0] = 1; stk[1] = L; stk[2] = 0;
    sh_s = 1;
    sh_bad = 0;
  }
  __syncthreads();
  for (;;) {
    if (sh_s == 0 || sh_bad) break;
    __syncthreads();  // (every thread has read sh_s / sh_bad before thread 0 changes them)
    if (tid == 0) {
      const int s = --sh_s;
      int i = stk[3 * s], j = stk[3 * s + 1];
      const int ml = stk[3 * s + 2];
      int pair = 0;
      if (ml == 0) {
        while (j > 0 && f5[j] == f5[j - 1]) j--;  // 3' end unpaired
      } else if (j - i < SFD_TURN + 1 || !sft_in(F, i, j)) {
        sh_bad = 1;
      } else {
        while (j - i > SFD_TURN + 1 && F.fML[sft_row(F, i, j - 1)] < SFD_INF &&
               F.fML[sft_row(F, i, j)] == F.fML[sft_row(F, i, j - 1)] + P.MLbase) j--;
        while (j - i > SFD_TURN + 1 && F.fML[sft_row(F, i + 1, j)] < SFD_INF &&
               F.fML[sft_row(F, i, j)] == F.fML[sft_row(F, i + 1, j)] + P.MLbase) i++;
        const int type = sft_type(D, F, i, j);
        pair = type && F.fML[sft_row(F, i, j)] == F.c[sft_col(F, j, i)] + sft_mlstem_out(D, F, type, i, j);
      }
      sh_i = i; sh_j = j; sh_ml = ml; sh_pair = pair;
    }
    __syncthreads();
    if (sh_bad) break;
    int i = sh_i, j = sh_j;
    const int ml = sh_ml;
    bool have_pair = sh_pair != 0;
    if (ml == 0) {
      if (j < SFD_TURN + 2) continue;
      // exterior stem (k, j): k from j-TURN-1 downwards to the first cell kept, the first match = the largest k
      const int fij = f5[j];
      const int32_t *cj = sft_colp(F, F.c, j);
      const int lo = sft_lo(F, j);
      int best = SFD_INF;
      for (int k = j - SFD_TURN - 1 - tid; k >= lo; k -= nt) {
        const int type = sft_type(D, F, k, j);
        if (type && fij == f5[k - 1] + cj[k] + sft_ext(D, F, type, k, j)) { best = -k; break; }
      }
      best = sf_block_min(best, red);
      if (best == SFD_INF) { if (tid == 0) sh_bad = 1; __syncthreads(); break; }
      const int k = -best;
      if (tid == 0) {
        const int s = sh_s++;
        stk[3 * s] = 1; stk[3 * s + 1] = k - 1; stk[3 * s + 2] = 0;
      }
      i = k;
      have_pair = true;
    } else if (!have_pair) {
      // split of fML[i][j] with ascending k
      const int fij = F.fML[sft_row(F, i, j)];
      const int32_t *a = F.fML + sft_row(F, i, i), *b = sft_colp(F, F.fMLt, j) + 1;  // a[k - i] = fML[i][k], b[k] = fML[k+1][j]
      int best = SFD_INF;
      for (int k = i + SFD_TURN + 1 + tid; k <= j - SFD_TURN - 2; k += nt) {
        const int x = a[k - i], y = b[k];
        if (x < SFD_INF && y < SFD_INF && fij == x + y) { best = k; break; }
      }
      best = sf_block_min(best, red);
      if (best == SFD_INF) { if (tid == 0) sh_bad = 1; __syncthreads(); break; }
      if (tid == 0) {
        const int s = sh_s;
        stk[3 * s] = i; stk[3 * s + 1] = best; stk[3 * s + 2] = 1;
        stk[3 * s + 3] = best + 1; stk[3 * s + 4] = j; stk[3 * s + 5] = 1;
        sh_s = s + 2;
      }
      __syncthreads();
      continue;
    }
    while (have_pair) {
      if (tid == 0) { F.db[i - 1] = '('; F.db[j - 1] = ')'; }
      const int type = sft_type(D, F, i, j);
      const int cij = F.c[sft_col(F, j, i)];
      if (cij == sft_hairpin(D, F, i, j, type)) break;
      // interior loops: p ascending, then q descending = (u1, u2) in lexicographic order
      const int d = j - i;
      const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
      int best = SFD_INF;
      for (int t = tid; t < 32 * 32; t += nt) {
        const int u1 = t >> 5, u2 = t & 31;
        if (u1 + u2 > umax) continue;
        if (cij == sft_intloop(D, F, i, j, type, u1, u2)) { best = t; break; }
      }
      best = sf_block_min(best, red);
      if (best != SFD_INF) {
        i = i + 1 + (best >> 5);
        j = j - 1 - (best & 31);
        continue;
      }
      // multiloop closed by (i, j): split of fML[i+1][j-1] with ascending k
      const int mm = P.MLclosing + sfd_mlstem(D, sfd_rtype(type), F.S[j - 1], F.S[i + 1]);
      const int32_t *a = F.fML + sft_row(F, i + 1, i + 1), *b = sft_colp(F, F.fMLt, j - 1) + 1;
      for (int k = i + 1 + SFD_TURN + 1 + tid; k <= j - 1 - SFD_TURN - 2; k += nt) {
        const int x = a[k - i - 1], y = b[k];
        if (x < SFD_INF && y < SFD_INF && cij == x + y + mm) { best = k; break; }
      }
      best = sf_block_min(best, red);
      if (best == SFD_INF) {
        if (tid == 0) sh_bad = 1;
      } else if (tid == 0) {
        const int s = sh_s;
        stk[3 * s] = i + 1; stk[3 * s + 1] = best; stk[3 * s + 2] = 1;
        stk[3 * s + 3] = best + 1; stk[3 * s + 4] = j - 1; stk[3 * s + 5] = 1;
        sh_s = s + 2;
      }
      break;
    }
    __syncthreads();
  }
  if (tid == 0 && sh_bad) atomicOr(F.status, 1);
}
