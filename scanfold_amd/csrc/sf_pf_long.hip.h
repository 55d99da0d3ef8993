// sf_pf_long.hip.h — McCaskill partition function of ONE sequence of any length 1 <= L <= SF_MAX_LONG, spread over the whole
// GPU: RNAfold -p on a whole record (ScanFoldFunctions.py:758-772, rna_refold) — ensemble free energy, centroid, centroid
// distance and mean base-pair distance (ensemble diversity).  sf_pf.hip.h stops at SF_MAX_W = 400 (one workgroup per fold).
//
// Recurrences: those in the header of sf_pf.hip.h (qb / qm1 / qm, q5 / q3, the outside pass through w, A0, A1 in O(L^3)),
// FP64 throughout, pair admissibility from sf_hc_type with the resident max_bp_span.  The inside, probability and finishing
// passes are the templates of sf_pf_cells.hip.h, which the banded partition function instantiates too; this file has the
// state, the layout as those templates see it, the exterior loop, the outside pass and the kernels.  Only sums are taken in another order
// (a cell's terms are spread over a group of lanes), so results agree with the window kernels to rounding, not bit for bit.
//
// Scaling.  ln Z grows by ~0.5 per nucleotide (1.5 for G/C-only sequences), so a whole record never fits FP64 unscaled and
// this file has only the scaled form (sf_pf_kernel<true>): with s = e^lns every weight carries s^-k for the k nucleotides it
// newly covers, Z_s = Z s^-L, ens_dG = -(ln Z_s + L lns) kT.  A pass costs O(L^3), so lns has to be right the first time:
//   * with the caller's MFE (sf_pf_long's mfe_dcal_hint; rna_refold has it anyway): lns = SF_PFLONG_MFE_FACTOR * (-MFE / kT) / L
//     — the ensemble free energy of natural and random sequences lies a few percent below the MFE;
//   * without: lns = SF_PFLONG_LNS_DEFAULT = 0.5, the per-nucleotide ln Z of a random sequence at 37 C.
// After the inside pass, ln Z_s not finite or |ln Z_s| > SF_PF_LNZ_MAX repeats it with lns += ln Z_s / L (700 / L with the
// sign of the excursion where it is not finite: the oracle's rule); the outside pass runs only after an inside pass in range.
// Outputs that are not finite (the outside tables left the range although Z_s did not) take the same step once ln Z_s is
// centred.  After SF_PFLONG_MAX_ATTEMPTS the call returns SF_ERR_RANGE; it never returns numbers made from non-finite tables.
//
// Launches.  One launch per anti-diagonal d = j - i, ascending for the inside pass and descending for the outside pass: all
// ordering between workgroups comes from kernel boundaries (no grid barrier, no floating-point atomics).  A cell is handled
// by a group of G lanes (a power of two <= 64) which take its terms round-robin and add their partial sums in a butterfly of
// __shfl_xor.  pfl_group of sf_pf_cells.hip.h (host and device: sf_pf_long_batch.hip.h calls it per row) sizes G so that cells * G fills the lane budget of the device (SF_PFLONG_LANES_PER_CU per compute unit: a
// compile-time figure, smaller in the CPU emulation build of the tests, which pays per lane) and lets a group walk several cells where the diagonal has more
// cells than the budget has groups.  G is a function of L, d and the device's number of compute units only, so two calls on the same input on
// the same device add in the same order and return bit-identical doubles.  q5 / q3 are sequential in j / i: one wave each, reducing over the other index.
//
// Layout (FP64, 64-bit offsets; a triangle holds L(L+1)/2 entries; R = row-major, row i holds j = i..L; C = column-major,
// column j holds i = 1..j; sfl_row / sfl_col of sf_mfe_long.hip.h).  Consecutive lanes of a group read consecutive entries:
//   qb   R (interior loops read q descending in row p; p = ob qb; q3 reads row i)  and  C (q5 reads column j)
//   qm   R (the splits of qb, qm and ob read row i+1 / i / j+1)                     and  C (A1 reads column i-1)
//   qm1  C (the splits of qb and qm read column j-1 / j)
//   ob   R (interior loops read l ascending in row k; p)
//   w    C (A1 reads column l)        — in the storage of qm1, which the outside pass no longer needs
//   A0   R (ob's sum over l > j)      — in the storage of qb's column-major copy, dead after q5
//   A1   R (ob's sum over l > j)
// The span limit bounds the loops, not the tables: A1's sum starts at k = l - max_pair_dist, ob's ends at l = i - 1 +
// max_pair_dist, and qb's multiloop split is skipped where (i, j) cannot pair; qm's split stays O(L) per cell.
//
// Device memory of one call (bytes):  7 * 8 * L(L+1)/2  (the triangles above)  +  ~60 L  (sequence, constraint arrays,
// hairpin weights, the powers of s, q5, q3, centroid, partial sums).  L = 29 903: 25.04 GB; L = 32 767: 30.06 GB.
// An allocation that fails returns SF_ERR_HIP with the text in sf_last_hip_error().
#pragma once
#include "sf_mfe_long.hip.h"
#include "sf_pf_cells.hip.h"

#define SF_PFLONG_NTRI 7
#ifdef SF_EMUL
#define SF_PFLONG_LANES_PER_CU 128   // (the emulated device has two compute units and runs every lane as a fiber)
#else
#define SF_PFLONG_LANES_PER_CU 1024  // lane budget of a diagonal launch: four waves per SIMD
#endif
#define SF_PFLONG_MAX_ATTEMPTS 6
#define SF_PFLONG_LNS_DEFAULT 0.5
#define SF_PFLONG_MFE_FACTOR 1.04
#define SF_PFLONG_BYTES(L) (SF_PFLONG_NTRI * sizeof(double) * SF_LONG_TRI(L) + 60 * (size_t)(L))

// The device state of one long partition function.  S as in SfLong.  hpx: hairpin initiation weights by loop size 0..L (the
// resident table only reaches SF_MAX_W + 1).  sc[k] = s^-k, mlbs[k] = (MLbase / s)^k, k = 0..L+1.
struct SfPfLong {
  const uint8_t *S;
  const double *hpx, *sc, *mlbs;
  SfHc hc;
  int L;
  double *qb, *qbt, *qm, *qmt, *qm1t, *ob, *wt, *a0, *a1, *q5, *q3;
  double *part;   // per-wave partial sums of the probability pass: 2 per wave
  double *out;    // ln Z_s, mean_bp_dist, centroid_dist
  char *cen;
};

// the layout and the place of Z_s as sf_pf_cells.hip.h's templates see them
__device__ __forceinline__ int sfp_type(const SfDevParams *D, const SfPfLong &F, int a, int b) {
  const bool ok = b - a <= D->max_pair_dist;
  return sf_hc_type(F.hc, ok ? D->pair[F.S[a]][F.S[b]] : 0, a, b, ok);
}
__device__ __forceinline__ size_t sfp_row(const SfPfLong &F, int i, int j) { return sfl_row(F.L, i, j); }
__device__ __forceinline__ size_t sfp_col(const SfPfLong &, int j, int i) { return sfl_col(j, i); }
__device__ __forceinline__ const double *sfp_colp(const SfPfLong &, const double *t, int j) { return t + sfl_col(j, 1); }
__device__ __forceinline__ int sfp_xhi(const SfPfLong &F, int i) { return F.L - i; }
__device__ __forceinline__ double sfp_z(const SfPfLong &F) { return F.q5[F.L]; }

// The kernels of this file give the sequence the whole launch (those of sf_pf_long_batch.hip.h give a row a run of workgroups).
__global__ void sf_pflong_inside_kernel(SfPfLong F, int d, int G, const SfDevParams *__restrict__ D,
                                     const SfDevParamsPF *__restrict__ X) {
  sfp_inside(F, d, G, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, D, X);
}

// q5[j] = q5[j-1] / s + sum_i q5[i-1] qb[i][j] ext(i, j), then q3 mirrored; one wave, which reads column j (row i) of qb
// contiguously and adds in a butterfly.  out[0] = ln Z_s.
__device__ __forceinline__ void sfpl_exterior(const SfPfLong &F, const SfDevParams *__restrict__ D,
                                              const SfDevParamsPF *__restrict__ X) {
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L;  // nt == 64
  if (tid == 0) { F.q5[0] = 1.0; F.q3[L + 1] = 1.0; }
  __syncthreads();
  for (int j = 1; j <= L; j++) {
    double v = 0.0;
    const double *cj = F.qbt + sfl_col(j, 1);  // cj[i - 1] = qb[i][j]
    for (int i = tid + 1; i + SFD_TURN + 1 <= j; i += nt) {
      const double q = cj[i - 1];
      if (q == 0.0) continue;
      const int type = sfp_type(D, F, i, j);
      if (type) v += F.q5[i - 1] * q * sfp_ext(X, F, type, i, j);
    }
    v = sfpl_group_sum(v, 64);
    if (tid == 0) F.q5[j] = F.q5[j - 1] * F.sc[1] + v;
    __syncthreads();
  }
  for (int i = L; i >= 1; i--) {
    double v = 0.0;
    const double *ri = F.qb + sfl_row(L, i, i);  // ri[j - i] = qb[i][j]
    for (int j = i + SFD_TURN + 1 + tid; j <= L; j += nt) {
      const double q = ri[j - i];
      if (q == 0.0) continue;
      const int type = sfp_type(D, F, i, j);
      if (type) v += q * sfp_ext(X, F, type, i, j) * F.q3[j + 1];
    }
    v = sfpl_group_sum(v, 64);
    if (tid == 0) F.q3[i] = F.q3[i + 1] * F.sc[1] + v;
    __syncthreads();
  }
  if (tid == 0) F.out[0] = log(F.q5[L]);
}
__global__ void sf_pflong_exterior_kernel(SfPfLong F, const SfDevParams *__restrict__ D, const SfDevParamsPF *__restrict__ X) {
  sfpl_exterior(F, D, X);
}

// Diagonal d of the outside pass (d descending from L-1 to TURN+1); groups and rounds as in the inside pass.
__device__ __forceinline__ void sfpl_outside(const SfPfLong &F, int d, int G, size_t gt, size_t nl, const SfDevParams *__restrict__ D,
                                             const SfDevParamsPF *__restrict__ X) {
  const int L = F.L;
  const int r = (int)(gt % (size_t)G);
  const size_t group = gt / (size_t)G, ngroups = nl / (size_t)G;
  const size_t ncell = (size_t)(L - d);
  const size_t rounds = (ncell + ngroups - 1) / ngroups;
  const int mpd = D->max_pair_dist;
  for (size_t it = 0; it < rounds; it++) {
    const size_t cell = group + it * ngroups;
    const bool valid = cell < ncell;
    const int i = (int)cell + 1, j = i + d;
    double a1 = 0.0, o = 0.0, mlsum = 0.0, qbij = 0.0;
    int type = 0;
    if (valid) {
      // A1[i][j] = sum_{k<i} w(k, j) qm[k+1][i-1], k <= i-2-TURN-1; w(k, j) = 0 where j - k passes the span limit
      if (i > 1) {
        const int klo = (mpd < j - 1) ? j - mpd : 1, khi = i - 2 - SFD_TURN - 1;
        const double *a = F.wt + sfl_col(j, 1) + (klo - 1);      // a[x] = w(klo + x, j)
        const double *b = F.qmt + sfl_col(i - 1, 1) + klo;        // b[x] = qm[klo + x + 1][i-1]
        const int n = khi - klo + 1;
        double s1 = 0.0;
        int x = r;
        for (; x + G < n; x += 2 * G) {
          a1 += a[x] * b[x];
          s1 += a[x + G] * b[x + G];
        }
        if (x < n) a1 += a[x] * b[x];
        a1 += s1;
      }
      type = sfp_type(D, F, i, j);
      qbij = F.qb[sfl_row(L, i, j)];
      if (type && qbij != 0.0) {
        if (r == 0) o = F.q5[i - 1] * F.q3[j + 1] * sfp_ext(X, F, type, i, j);
        if (i > 1 && j < L) {
          const int rt = sfd_rtype(type);
          const int sp1 = F.S[i - 1], sq1 = F.S[j + 1];
          const int u1max = sfd_min(SFD_MAXLOOP, i - 2);
          for (int u1 = 0; u1 <= u1max; u1++) {
            const int kk = i - 1 - u1;
            const int u2max = sfd_min(SFD_MAXLOOP - u1, L - j - 1);
            const double *row = F.ob + sfl_row(L, kk, kk);  // row[l - kk] = ob[kk][l]
            for (int u2 = r; u2 <= u2max; u2 += G) {
              const int l = j + 1 + u2;
              const double v = row[l - kk];
              if (v == 0.0) continue;
              const int tk = sfp_type(D, F, kk, l);
              if (!tk) continue;
              o += v * sfx_intloop(X, u1, u2, tk, rt, F.S[kk + 1], F.S[l - 1], sp1, sq1) * F.sc[u1 + u2 + 2];
            }
          }
          // sum_{l>j} A1[i][l] ((MLbase/s)^(l-1-j) + qm[j+1][l-1]) + A0[i][l] qm[j+1][l-1]; A0 = A1 = 0 past the span limit
          const int lhi = (mpd < L - i + 1) ? i - 1 + mpd : L;
          const double *pa1 = F.a1 + sfl_row(L, i, j + 1), *pa0 = F.a0 + sfl_row(L, i, j + 1);  // [x]: l = j+1+x
          const double *pq = F.qm + sfl_row(L, j + 1, j + 1) - 1;  // pq[x] = qm[j+1][j+x] (x >= 1)
          const int n = lhi - j;
          double s1 = 0.0;
          int x = r;
          if (x == 0 && n > 0) { mlsum += pa1[0] * F.mlbs[0]; x += G; }  // l = j+1: qm[j+1][j] is empty
          for (; x + G < n; x += 2 * G) {
            const double q0 = pq[x], q1 = pq[x + G];
            mlsum += pa1[x] * (F.mlbs[x] + q0) + pa0[x] * q0;
            s1 += pa1[x + G] * (F.mlbs[x + G] + q1) + pa0[x + G] * q1;
          }
          if (x < n) { const double q0 = pq[x]; mlsum += pa1[x] * (F.mlbs[x] + q0) + pa0[x] * q0; }
          mlsum += s1;
        }
      }
    }
    const bool paired = type && qbij != 0.0;
    if (paired && i > 1 && j < L) o += mlsum * sfx_mlstem(X, type, F.S[i - 1], F.S[j + 1]);  // (the cell's factor)
    a1 = sfpl_group_sum(a1, G);
    o = sfpl_group_sum(o, G);
    if (valid && r == 0) {
      const size_t ro = sfl_row(L, i, j);
      double a0 = 0.0;
      if (i > 1) a0 = F.a0[sfl_row(L, i - 1, j)] * X->MLbase * F.sc[1] + F.wt[sfl_col(j, i - 1)];
      F.a0[ro] = a0;
      F.a1[ro] = a1;
      double ow = 0.0;
      if (paired) {
        ow = o * X->MLclosing * sfx_mlstem(X, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) * F.sc[2];
      } else o = 0.0;
      F.ob[ro] = o;
      F.wt[sfl_col(j, i)] = ow;
    }
  }
}
__global__ void sf_pflong_outside_kernel(SfPfLong F, int d, int G, const SfDevParams *__restrict__ D,
                                      const SfDevParamsPF *__restrict__ X) {
  sfpl_outside(F, d, G, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, D, X);
}
__global__ void sf_pflong_prob_kernel(SfPfLong F) {
  sfp_prob(F, ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, ((size_t)gridDim.x * blockDim.x) >> 6);
}
__global__ void sf_pflong_finish_kernel(SfPfLong F, int nwaves) { sfp_finish(F, nwaves); }
