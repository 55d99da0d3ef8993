// sf_mea.hip.h — the maximum-expected-accuracy (MEA) structure of a sparse list of base-pair probabilities: the third
// banded dynamic programme of the whole-record family, after the MFE fold (sf_mfe_banded.hip.h) and the partition function
// (sf_pf_banded.hip.h).  Model (include/scanfold_hip_long.h): over the listed pairs (i, k, p) and the
// unpaired probabilities u, with w_ik = (2.0 * gamma) * p_ik rounded once and stored,
//   M[i][j] = max( u_i + M[i+1][j] , max over listed (i, k), k <= j, of (w_ik + M[i+1][k-1]) + M[k+1][j] ),  j - i < B,
//   E[i]    = max( u_i + E[i+1]    , max over listed (i, k)          of (w_ik + M[i+1][k-1]) + E[k+1]    ),  E[L+1] = 0,
// M = 0 for j < i, B = 1 + the largest k - i of the list; the score is E[1].  Every operation after the weights is an
// addition or a maximum of doubles, associated as written, so no expression can be contracted and the value of a cell does
// not depend on which lane formed it.
//
// Layout.  M is L * B doubles, diagonal-major: M[i][j] at (j - i) * L + (i - 1).  The cells of one launch are neighbours in
// memory, the first candidate's M[i+1][j] is the neighbouring run of the diagonal before, and a partner's M[k+1][j] is a
// gather at 1-3 places per cell.
//
// The inner term A_ik = w_ik + M[i+1][k-1] of a listed pair does not depend on j.  It is formed once, by the cell (i, k) on
// the diagonal k - i (M[i+1][k-1] lies two diagonals before), and replaces w_ik in the weights' array `wa`: in the launch
// of diagonal d only the thread of cell (i, i + d) touches the records of row i, so the replacement races with nothing.
// Every later reader (the cells (i, j > k), the exterior pass, the traceback) adds to the stored A: the same expression.
//   * sf_mea_weights_kernel: wa[t] = g2 * p[t] with g2 = 2.0 * gamma from the host; a product alone, then a store.
//   * sf_mea_fill_kernel: one launch per diagonal d = 0 .. B-1, a thread per cell.  The partners of i are the records
//     off[i-1] .. off[i] of the list (64-bit offsets, ascending in k), walked until k > j: any number of them.
//   * sf_mea_exterior_kernel: one wave.  The chain over i is serial, but it needs no M at all (A is stored), and a step's
//     E[k+1] is an old value unless k lies within the 64 positions the wave works on.  Per chunk of 64 positions, lane t
//     first folds every partner beyond the chunk into one maximum (`far`) and loads its first SFM_NEAR partners inside
//     the chunk, all lanes at once and off the chain; then the lanes take their turns, each reading E[i+1] and the E of
//     its near partners from LDS.  Near partners past SFM_NEAR (a caller's dense list) are read on the lane's turn.
//   * sf_mea_trace_kernel: one wave, an explicit stack of (i, j) segments in device memory (j = 0: the suffix from i).
//     At a segment or suffix starting at i, i is unpaired when the stored value equals the first candidate; else it pairs
//     with the smallest k whose candidate equals it.  The wave tests 64 positions ahead at once and jumps to the first
//     that is not unpaired (__ballot, __ffsll), then tests 64 partners at once, in ascending k.  No match: bit 0 of the
//     status word (SF_ERR_INTERNAL).
// Both one-wave kernels hand values from one lane to the others through device memory (E of the chunk before, the stack's
// top): the __syncthreads() between the write and the reads is what makes them visible.  In a workgroup of one wave the
// barrier itself may be elided, but its workgroup-scope fence is kept, and the fence is what is needed.
// No atomics, no cooperative launch, no grid barrier.  Wave-level primitives: __ballot, __shfl, __ffsll, with wave-uniform
// loop bounds around each.
#pragma once
#include "sf_launch.h"
#include "sf_pf_probs.hip.h"

#define SFM_NEAR 4                                           // partners inside the exterior pass's chunk kept in registers
#define SF_MEA_STACK_INTS(L) (2 * ((size_t)(L) / 2 + 2))     // traceback stack, int32: a segment per open pair, and the suffix

struct SfMea {
  int L, B;
  unsigned long long n;           // records of the list
  const SfPairProb *list;         // ascending in (i, j), 1-based
  const unsigned long long *off;  // L offsets: row i is list[off[i-1] .. off[i]), the last row ends at n
  const double *u;                // L unpaired probabilities
  double *wa;                     // n: w_ik, then A_ik once diagonal k - i has run
  double *M;                      // L * B, diagonal-major
  double *E;                      // L + 2: E[1 .. L + 1]
  int32_t *stk;                   // SF_MEA_STACK_INTS(L)
  char *db;                       // L + 1
  int *status;
};

__device__ __forceinline__ unsigned long long sfm_row_end(const SfMea &F, int i) { return i < F.L ? F.off[i] : F.n; }
__device__ __forceinline__ double sfm_m(const SfMea &F, int i, int j) {
  return j < i ? 0.0 : F.M[(size_t)(j - i) * (size_t)F.L + (size_t)(i - 1)];
}

__global__ void __launch_bounds__(256) sf_mea_weights_kernel(SfMea F, double g2) {
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < F.n; t += step) F.wa[t] = g2 * F.list[t].p;
}

__global__ void __launch_bounds__(256) sf_mea_fill_kernel(SfMea F, int d) {
  const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= (size_t)(F.L - d)) return;
  const int i = (int)x + 1, j = i + d;
  double best = F.u[i - 1] + sfm_m(F, i + 1, j);
  const unsigned long long te = sfm_row_end(F, i);
  for (unsigned long long t = F.off[i - 1]; t < te; t++) {
    const int k = F.list[t].j;
    if (k > j) break;
    double a = F.wa[t];
    if (k == j) {  // the pair's own cell: w becomes A for every later reader
      a = a + sfm_m(F, i + 1, k - 1);
      F.wa[t] = a;
    }
    const double c = a + sfm_m(F, k + 1, j);
    best = c > best ? c : best;
  }
  F.M[(size_t)d * (size_t)F.L + x] = best;
}

__global__ void __launch_bounds__(64) sf_mea_exterior_kernel(SfMea F) {
  __shared__ double ech[65];  // ech[0] = E[i0 + 1]; ech[1 + t] = E[i0 - t], lane t's
  const int lane = threadIdx.x, L = F.L;
  if (lane == 0) {
    F.E[L + 1] = 0.0;
    ech[0] = 0.0;
  }
  __syncthreads();
  for (int i0 = L; i0 >= 1; i0 -= 64) {
    const int i = i0 - lane;
    // off the chain: the partners beyond the chunk (E[k+1] is final), and the first near ones into registers
    double ui = 0.0, far = -1.0;  // (every candidate is >= 0: -1 is "none")
    double na[SFM_NEAR];
    int nk[SFM_NEAR];
    unsigned long long t0 = 0, tn = 0;  // the near partners, k < i0: records t0 .. tn (they come first, ascending in k)
#pragma unroll
    for (int q = 0; q < SFM_NEAR; q++) { na[q] = 0.0; nk[q] = 0; }
    if (i >= 1) {
      ui = F.u[i - 1];
      const unsigned long long te = sfm_row_end(F, i);
      unsigned long long t = t0 = F.off[i - 1];
      while (t < te && F.list[t].j < i0) t++;
      tn = t;
      for (; t < te; t++) {
        const double c = F.wa[t] + F.E[F.list[t].j + 1];
        far = c > far ? c : far;
      }
#pragma unroll
      for (int q = 0; q < SFM_NEAR; q++)
        if (t0 + q < tn) {
          na[q] = F.wa[t0 + q];
          nk[q] = F.list[t0 + q].j;
        }
    }
    // the chain: lane s takes position i0 - s
    for (int s = 0; s < 64; s++) {
      if (lane == s && i >= 1) {
        double best = ui + ech[s];
        best = far > best ? far : best;
#pragma unroll
        for (int q = 0; q < SFM_NEAR; q++)
          if (t0 + q < tn) {
            const double c = na[q] + ech[i0 - nk[q]];  // E[k + 1] = ech[1 + (i0 - (k + 1))]
            best = c > best ? c : best;
          }
        for (unsigned long long t = t0 + SFM_NEAR; t < tn; t++) {
          const double c = F.wa[t] + ech[i0 - F.list[t].j];
          best = c > best ? c : best;
        }
        ech[1 + s] = best;
      }
      SF_WAVE_SYNC();
    }
    if (i >= 1) F.E[i] = ech[1 + lane];
    __syncthreads();
    if (lane == 0) ech[0] = ech[64];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) sf_mea_trace_kernel(SfMea F) {
  const int lane = threadIdx.x, L = F.L;
  int32_t *stk = F.stk;
  for (int x = lane; x < L; x += 64) F.db[x] = '.';
  if (lane == 0) {
    F.db[L] = 0;
    stk[0] = 1;  // the suffix from 1: the whole record
    stk[1] = 0;
  }
  int top = 1;
  bool bad = false;
  __syncthreads();
  while (top > 0 && !bad) {
    top--;
    int i = stk[2 * top];
    const int j = stk[2 * top + 1];
    const bool ext = j == 0;
    const int hi = ext ? L : j;
    // the value of the segment or suffix starting at x (0 past its end)
    auto value = [&](int x) { return ext ? F.E[x] : sfm_m(F, x, j); };
    while (i <= hi) {
      const int x = i + lane;
      double val = 0.0;
      bool unp = true;
      if (x <= hi) {
        val = value(x);
        unp = val == F.u[x - 1] + value(x + 1);
      }
      const unsigned long long paired = __ballot(!unp);
      if (!paired) {
        i += 64;
        continue;
      }
      const int f = __ffsll(paired) - 1;
      i += f;
      const double v = __shfl(val, f);
      const unsigned long long t0 = F.off[i - 1], te = sfm_row_end(F, i);
      int kf = 0;
      for (unsigned long long tb = t0; tb < te && !kf; tb += 64) {
        const unsigned long long t = tb + (unsigned long long)lane;
        bool hit = false;
        int k = 0;
        if (t < te) {
          k = F.list[t].j;
          if (k <= hi) hit = F.wa[t] + value(k + 1) == v;
        }
        const unsigned long long m = __ballot(hit);
        if (m) kf = __shfl(k, __ffsll(m) - 1);
      }
      if (!kf) {
        bad = true;
        break;
      }
      const bool open = kf - 1 >= i + 1;
      if (lane == 0) {
        F.db[i - 1] = '(';
        F.db[kf - 1] = ')';
        if (open) {
          stk[2 * top] = i + 1;
          stk[2 * top + 1] = kf - 1;
        }
      }
      if (open) top++;
      i = kf + 1;
    }
    __syncthreads();  // (one wave: orders lane 0's pushes before every lane's pop)
  }
  if (bad && lane == 0) *F.status |= 1;
}
