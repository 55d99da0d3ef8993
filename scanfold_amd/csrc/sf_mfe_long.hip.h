// sf_mfe_long.hip.h — Zuker MFE fill + traceback of ONE sequence of any length 1 <= L <= SF_MAX_LONG (32 767), spread over
// the whole GPU: fc = RNA.fold_compound(seq, md); fc.hc_add_from_db(cons); fc.mfe() on a whole record (ScanFold.py:1509-1547,
// --global_refold).  The window kernels stop at SF_MAX_W = 400 because their tables live in LDS or in per-fold scratch.
//
// Recurrences and traceback order are those of oracle/sf_oracle.c (mfe_fill / mfe_traceback), already restated for W <= 400
// by sf_mfe_full.hip.h: dangles = 2, MAXLOOP 30, DML[i][j] = min_k fML[i][k] + fML[k+1][j] the only O(L^3) term, f5 the
// exterior loop.  The traceback takes the same first decomposition in the same order, so structures are byte-identical.
//
// Launches.  Cell (i, j) on anti-diagonal d = j - i depends only on diagonals below d: one fill launch per diagonal, so every
// ordering between workgroups comes from kernel boundaries (no grid barrier).  A cell is handled by a group of G lanes
// (G a power of two <= 64, chosen per diagonal by the host: 1 lane while the split is short, up to a whole wave on the late,
// short diagonals whose cells have up to L split terms each); the group's minimum is a butterfly of __shfl_xor inside the wave.
// Then f5 (sequential in j) in one workgroup that reduces over i for each j, then the traceback in one workgroup: sft_trace
// of sf_mfe_trace.hip.h, which the banded fold instantiates too; the energy helpers of a cell (sft_*) live there as well.
//
// Layout (int32, 64-bit offsets throughout; a triangle holds L(L+1)/2 entries):
//   fML   row-major upper triangle: row i holds j = i..L        FR(i, j) = (i-1)L - (i-1)(i-2)/2 + (j-i)
//   fMLt  the same values column-major: row j holds i = 1..j    FT(j, i) = j(j-1)/2 + (i-1)
//   c     column-major like fMLt (f5 and the exterior traceback read a column of c contiguously)
//   DML   a ring of three diagonals (c reads DML two diagonals down; the traceback recomputes the split it needs)
// so the split min_k fML[i][k] + fML[k+1][j] reads row i of fML and row j of fMLt, both contiguous in k.
//
// Device memory of one call (bytes):  12 * L(L+1)/2  (c, fML, fMLt)  +  12 (L+2)  (DML ring)  +  ~68 L  (sequence, hairpin
// initiation, constraint arrays, f5, traceback stack, structure).  L = 29 903: 5.37 GB; L = 32 767: 6.44 GB.
#pragma once
#include "sf_mfe_trace.hip.h"

#define SF_LONG_TRI(L) ((size_t)(L) * ((size_t)(L) + 1) / 2)

__device__ __forceinline__ size_t sfl_row(int L, int i, int j) {  // row-major triangle (fML)
  const size_t a = (size_t)(i - 1);
  return a * (size_t)L - a * (a - 1) / 2 + (size_t)(j - i);
}
__device__ __forceinline__ size_t sfl_col(int j, int i) {  // column-major triangle (c, fMLt)
  return (size_t)j * (size_t)(j - 1) / 2 + (size_t)(i - 1);
}

// The device state of one long fold.  S: codes 0..4 at S[1..L], S[0] = S[L+1] = 0.  hp: hairpin initiation by loop size
// 0..L (the resident model's table only reaches SF_MAX_W + 1).  hc.c == nullptr: no constraint.
struct SfLong {
  const uint8_t *S;
  const int32_t *hp;
  SfHc hc;
  int L;
  int32_t *c, *fML, *fMLt, *dml, *f5, *stk;
  char *db;
  int *status;
};

// the layout as sf_mfe_trace.hip.h's templates see it
__device__ __forceinline__ int sft_type(const SfDevParams *D, const SfLong &F, int a, int b) {
  const bool ok = b - a <= D->max_pair_dist;
  return sf_hc_type(F.hc, ok ? D->pair[F.S[a]][F.S[b]] : 0, a, b, ok);
}
__device__ __forceinline__ size_t sft_row(const SfLong &F, int i, int j) { return sfl_row(F.L, i, j); }
__device__ __forceinline__ size_t sft_col(const SfLong &, int j, int i) { return sfl_col(j, i); }
__device__ __forceinline__ const int32_t *sft_colp(const SfLong &, const int32_t *t, int j) { return t + sfl_col(j, 1) - 1; }
__device__ __forceinline__ int sft_lo(const SfLong &, int) { return 1; }
__device__ __forceinline__ bool sft_in(const SfLong &, int, int) { return true; }

// Cell i = cell + 1 of diagonal d, as lane r of the cell's group of G lanes (shared with sf_mfe_long_batch.hip.h).  Every lane
// of a wave comes here, with or without a cell: the group's minimum is a butterfly over the wave.
__device__ __forceinline__ void sfl_fill_cell(const SfLong &F, int d, int G, int r, size_t cell, const SfDevParams *__restrict__ D) {
  const int L = F.L;
  const bool valid = cell < (size_t)(L - d);
  const int i = (int)cell + 1, j = i + d;
  int32_t *dml_d = F.dml + (size_t)(d % 3) * (size_t)(L + 2);
  if (d < SFD_TURN + 1) {  // no pair and no multiloop this short (the same for every thread of the launch)
    if (valid && r == 0) {
      F.c[sfl_col(j, i)] = SFD_INF;
      F.fML[sfl_row(L, i, j)] = SFD_INF;
      F.fMLt[sfl_col(j, i)] = SFD_INF;
      dml_d[i] = SFD_INF;
    }
    return;
  }
  const sf_params_blob &P = D->P;
  int type = 0, e = SFD_INF;
  if (valid) {
    type = sft_type(D, F, i, j);  // max_bp_span, hard constraint
    if (type) {
      if (r == 0) {
        e = sft_hairpin(D, F, i, j, type);
        const int dml = F.dml[(size_t)((d - 2) % 3) * (size_t)(L + 2) + i + 1];
        if (dml < SFD_INF) e = sfd_min(e, dml + sfd_mlstem(D, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) + P.MLclosing);
      }
      const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
      for (int u1 = 0; u1 <= umax; u1++)
        for (int u2 = r; u2 <= umax - u1; u2 += G) e = sfd_min(e, sft_intloop(D, F, i, j, type, u1, u2));
    }
  }
  int dec = SFD_INF;
  if (valid) {
    // DML[i][j] = min_k fML[i][k] + fML[k+1][j], k = i+TURN+1 .. j-TURN-2: row i of fML, row j of fMLt
    const int32_t *a = F.fML + sfl_row(L, i, i);  // a[k - i] = fML[i][k]
    const int32_t *b = F.fMLt + sfl_col(j, 1);    // b[k] = fML[k+1][j]
    int dec2 = SFD_INF;
    int k = i + SFD_TURN + 1 + r;
    const int kend = j - SFD_TURN - 2;
    for (; k + G <= kend; k += 2 * G) {
      const int x0 = a[k - i], y0 = b[k], x1 = a[k + G - i], y1 = b[k + G];
      if (x0 < SFD_INF && y0 < SFD_INF) dec = sfd_min(dec, x0 + y0);
      if (x1 < SFD_INF && y1 < SFD_INF) dec2 = sfd_min(dec2, x1 + y1);
    }
    if (k <= kend) {
      const int x0 = a[k - i], y0 = b[k];
      if (x0 < SFD_INF && y0 < SFD_INF) dec = sfd_min(dec, x0 + y0);
    }
    dec = sfd_min(dec, dec2);
  }
  for (int m = G >> 1; m >= 1; m >>= 1) {  // minimum over the cell's group (every lane of the wave takes part)
    const long long o = __shfl_xor((long long)(((unsigned long long)(uint32_t)e << 32) | (uint32_t)dec), m);
    e = sfd_min(e, (int)(o >> 32));
    dec = sfd_min(dec, (int)(uint32_t)o);
  }
  if (valid && r == 0) {
    const int cij = type ? e : SFD_INF;
    F.c[sfl_col(j, i)] = cij;
    int f = SFD_INF;
    const int fa = F.fML[sfl_row(L, i + 1, j)], fb = F.fML[sfl_row(L, i, j - 1)];
    if (fa < SFD_INF) f = sfd_min(f, fa + P.MLbase);
    if (fb < SFD_INF) f = sfd_min(f, fb + P.MLbase);
    if (type) f = sfd_min(f, cij + sft_mlstem_out(D, F, type, i, j));
    dml_d[i] = dec;
    f = sfd_min(f, dec);
    F.fML[sfl_row(L, i, j)] = f;
    F.fMLt[sfl_col(j, i)] = f;
  }
}

// Diagonal d of the fill.  Thread t of the grid is lane t % G of the group of cell i = t / G + 1.
__global__ void sf_long_fill_kernel(SfLong F, int d, int G, const SfDevParams *__restrict__ D) {
  const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  sfl_fill_cell(F, d, G, (int)(gt % (size_t)G), gt / (size_t)G, D);
}

// f5[j] = min(f5[j-1], min_i f5[i-1] + c[i][j] + ExtLoop(i, j)); one workgroup, column j of c read contiguously.
__device__ __forceinline__ void sfl_f5(const SfLong &F, const SfDevParams *__restrict__ D, int32_t *mfe_out) {
  __shared__ int red[16];
  const int tid = threadIdx.x, L = F.L;
  if (tid == 0) F.f5[0] = 0;
  __syncthreads();
  for (int j = 1; j <= L; j++) {
    int v = SFD_INF;
    const int32_t *cj = F.c + sfl_col(j, 1);  // cj[i - 1] = c[i][j]
    for (int i = tid + 1; i + SFD_TURN + 1 <= j; i += blockDim.x) {
      const int type = sft_type(D, F, i, j);
      if (type) v = sfd_min(v, F.f5[i - 1] + cj[i - 1] + sft_ext(D, F, type, i, j));
    }
    v = sf_block_min(v, red);
    if (tid == 0) F.f5[j] = sfd_min(F.f5[j - 1], v);
    __syncthreads();
  }
  if (tid == 0 && mfe_out) *mfe_out = F.f5[L];
}
__global__ void sf_long_f5_kernel(SfLong F, const SfDevParams *__restrict__ D, int32_t *mfe_out) { sfl_f5(F, D, mfe_out); }
__global__ void sf_long_trace_kernel(SfLong F, const SfDevParams *__restrict__ D) { sft_trace(F, D); }
