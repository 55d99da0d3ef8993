// sf_pf_banded.hip.h — McCaskill partition function of ONE sequence of 1 <= L <= SF_MAX_BANDED under a base-pair span S, in
// BANDED tables (sf_pf_banded): the ensemble free energy, centroid and ensemble diversity of a viral genome, a pre-mRNA or a
// chromosome region folded with md.max_bp_span set.  sf_pf_long.hip.h under a span bounds loops, not tables, and stops at
// SF_MAX_LONG; here memory is linear in L and a pass costs about L B^2 / 2 terms.
//
// Why the band is exact.  With max_pair_dist = S - 1 a cell (i, j) with j - i >= B = min(S, L) has pair type 0, so qb = ob =
// w = 0 there, and every table read made by a cell inside the band lies inside the band: qb's multiloop split reads
// qm[i+1][u-1] and qm1[u][j-1], qm's split qm[i][u-1] and qm1[u][j], qm1 reads qm1[i][j-1]; A1[i][j] reads w(k, j) for
// j - k <= S - 1 and qm[k+1][i-1]; A0[i][j] reads A0[i-1][j] (0 on diagonal B) and w(i-1, j); ob's sum over l ends at
// l = i - 1 + max_pair_dist and reads A1[i][l], A0[i][l], qm[j+1][l-1]; interior loops read qb inside (i, j) and ob[k][l]
// around it, which is 0 outside the band (the (u1, u2) loop is clipped to l - k < B); q5 / q3 read qb only.  So B diagonals
// of each table give the sums of sf_pf_long.hip.h's triangles.  The inside, probability and finishing passes are the
// templates of sf_pf_cells.hip.h which sf_pf_long.hip.h instantiates too: one body, which sees the band through the
// overloads below.  The outside pass is this file's own (sfpb_outside: sf_pf_long.hip.h's recurrences and lane-group scheme,
// every loop clipped to the band; one body for both cost the triangle's kernel time, profiles/pf_cells_shared).  Every sum
// has sf_pf_long.hip.h's order; the exterior loop and the place of Z_s differ (Two scales, below), so the two agree to
// rounding, not bit for bit.
//
// Layout (FP64, 64-bit offsets; a band table holds L * B entries, the cells 0 <= j - i <= B - 1; R = row-banded, row i holds
// j = i .. i+B-1 at (i-1) B + (j-i); C = column-banded, column j holds i = j-B+1 .. j at (j-1) B + (i-j+B-1): SfBand's).
// Every O(B) sum reads two contiguous runs:
//   qb   R (interior loops, p = ob qb, q3)  and  C (q5 reads column j)
//   qm   R (the splits of qb, qm and ob)    and  C (A1 reads column i-1)
//   qm1  C (the splits of qb and qm)
//   ob   R (interior loops, p)
//   w    C (A1 reads column j)   — in the storage of qm1, which the outside pass no longer needs
//   A0   R (ob's sum over l)     — in the storage of qb's column copy, dead after q5
//   A1   R (ob's sum over l)
// Seven band tables, as sf_pf_long.hip.h has seven triangles: A0 is a running sum down a column but is read along a row, and
// A1 is read along the row it is written in on later (shorter) diagonals, so neither fits a ring of diagonals.
// Entries of a row or column that fall outside the record (j > L, i < 1) exist in memory and are never written or read.
//
// Two scales.  The band tables carry one per-nucleotide scale s = e^lns like sf_pf_long.hip.h's (sc[k] = s^-k, mlbs[k] =
// (MLbase / s)^k, needed for k <= B + 1 only; hpx up to B): a cell covers at most B nucleotides, so its weight stays in
// FP64 while |g - lns| B <~ 700 for the growth g of ln Z per nucleotide around it.  The exterior loop covers the whole
// record, where no single scale holds once the composition changes along it (ten G/C-only blocks of 300 nt followed by ten
// A/U-only ones leave every scale at least e^1290 off somewhere), so q5[j] = Z(1..j) s^-j and q3 are a double mantissa in
// [0.5, 1) (m5, m3) and an int32 binary exponent (e5, e3) per position.  They are renormalised by powers of two only (frexp /
// ldexp), which is exact: the result does not depend on when it happens.  ln Z_s = ln m5[L] + e5[L] ln 2 may be thousands.
// ob is stored already divided by Z_s: the exterior seed of a cell is q5[i-1] q3[j+1] / Z_s put together from the three
// mantissas and exponents, every other outside recurrence is linear in ob, and the probability is ob qb.
// Known limit: a record so heterogeneous, under a span so wide, that |g_local - lns| B passes ~700 somewhere for every lns
// leaves FP64 in the band tables and ends in SF_ERR_RANGE (a position-dependent scale is not provided).
//
// Launches: one per diagonal, d = 0 .. B-1 for the inside pass and B-1 .. TURN+1 for the outside pass; all ordering between
// workgroups comes from kernel boundaries (no grid barrier, no cooperative launch, no floating-point atomics).  A cell is a
// group of G = pfl_group(cells, d, lanes) lanes which take its terms round-robin and add them in a __shfl_xor butterfly; a
// group walks several cells where the diagonal has more cells than the launch has groups.  The order of every sum is a
// function of L, B, d and the device's number of compute units only: two calls return bit-identical doubles.  q5 and q3 are
// sequential in j / i with at most B terms a step: one wave each, side by side in one launch of two workgroups.
//
// Device memory of one call: SF_PF_BANDED_BYTES(L, B) = 56 L B + 35 L + 24 B + 65 677 bytes (include/scanfold_hip_long.h).
#pragma once
#include "sf_mfe_banded.hip.h"
#include "sf_pf_cells.hip.h"

#define SF_PFBAND_NTAB 7
#define SF_PFBAND_MAX_WAVES 4096  // waves of the probability pass at most: the partial sums are a fixed 64 KiB

// The device state of one banded partition function.  S as in SfBand.  hpx: hairpin initiation weights by loop size 0..B.
// sc[k] = s^-k, mlbs[k] = (MLbase / s)^k, k = 0 .. B + 1.  q5[j] = m5[j] 2^e5[j], j = 0..L; q3[i] = m3[i] 2^e3[i], i = 1..L+1.
struct SfPfBand {
  const uint8_t *S;
  const double *hpx, *sc, *mlbs;
  SfHc32 hc;
  int L, B;
  double *qb, *qbt, *qm, *qmt, *qm1t, *ob, *wt, *a0, *a1, *m5, *m3;
  int32_t *e5, *e3;
  double *part;   // per-wave partial sums of the probability pass: 2 per wave
  double *out;    // ln Z_s, mean_bp_dist, centroid_dist
  char *cen;
};

// the layout and the place of Z_s as sf_pf_cells.hip.h's templates see them
__device__ __forceinline__ int sfp_type(const SfDevParams *D, const SfPfBand &F, int a, int b) {
  const bool ok = b - a <= D->max_pair_dist;
  return sf_hc_type_of(F.hc, ok ? D->pair[F.S[a]][F.S[b]] : 0, a, b, ok);
}
__device__ __forceinline__ size_t sfp_row(const SfPfBand &F, int i, int j) { return sfb_row(F.B, i, j); }
__device__ __forceinline__ size_t sfp_col(const SfPfBand &F, int j, int i) { return sfb_col(F.B, j, i); }
// (p[i - 1] is in the table for i = max(1, j-B+1) .. j)
__device__ __forceinline__ const double *sfp_colp(const SfPfBand &F, const double *t, int j) {
  return t + ((long long)(j - 1) * F.B + (F.B - j));
}
__device__ __forceinline__ int sfp_xhi(const SfPfBand &F, int i) { return sfd_min(F.L - i, F.B - 1); }
__device__ __forceinline__ double sfp_z(const SfPfBand &) { return 1.0; }  // (ob is divided by Z_s already; x / 1.0 is x)

__global__ void sf_pfband_inside_kernel(SfPfBand F, int d, int G, const SfDevParams *__restrict__ D,
                                        const SfDevParamsPF *__restrict__ X) {
  sfp_inside(F, d, G, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, D, X);
}

// Workgroup 0: q5[j] = q5[j-1] / s + sum_i q5[i-1] qb[i][j] ext(i, j), i >= j-B+1, and out[0] = ln Z_s.  Workgroup 1: q3
// mirrored.  One wave each, which reads column j (row i) of qb contiguously and adds in a butterfly.  The terms of a step
// are brought to the exponent of the step's neighbour (q5[j-1], q3[i+1]) by ldexp; the sum is split again by frexp.
__global__ void sf_pfband_exterior_kernel(SfPfBand F, const SfDevParams *__restrict__ D, const SfDevParamsPF *__restrict__ X) {
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L, B = F.B;  // nt == 64
  if (blockIdx.x == 0) {
    if (tid == 0) { F.m5[0] = 0.5; F.e5[0] = 1; }
    __syncthreads();
    for (int j = 1; j <= L; j++) {
      double v = 0.0;
      const double *cj = sfp_colp(F, F.qbt, j);  // cj[i - 1] = qb[i][j]
      const int lo = j - B + 1 > 1 ? j - B + 1 : 1, eref = F.e5[j - 1];
      for (int i = lo + tid; i + SFD_TURN + 1 <= j; i += nt) {
        const double q = cj[i - 1];
        if (q == 0.0) continue;
        const int type = sfp_type(D, F, i, j);
        if (type) v += ldexp(F.m5[i - 1] * (q * sfp_ext(X, F, type, i, j)), F.e5[i - 1] - eref);
      }
      v = sfpl_group_sum(v, 64);
      if (tid == 0) {
        int ex;
        F.m5[j] = frexp(F.m5[j - 1] * F.sc[1] + v, &ex);
        F.e5[j] = eref + ex;
      }
      __syncthreads();
    }
    if (tid == 0) F.out[0] = log(F.m5[L]) + (double)F.e5[L] * 0.693147180559945309417;
  } else {
    if (tid == 0) { F.m3[L + 1] = 0.5; F.e3[L + 1] = 1; }
    __syncthreads();
    for (int i = L; i >= 1; i--) {
      double v = 0.0;
      const double *ri = F.qb + sfb_row(B, i, i);  // ri[j - i] = qb[i][j]
      const int hi = i + B - 1 < L ? i + B - 1 : L, eref = F.e3[i + 1];
      for (int j = i + SFD_TURN + 1 + tid; j <= hi; j += nt) {
        const double q = ri[j - i];
        if (q == 0.0) continue;
        const int type = sfp_type(D, F, i, j);
        if (type) v += ldexp(F.m3[j + 1] * (q * sfp_ext(X, F, type, i, j)), F.e3[j + 1] - eref);
      }
      v = sfpl_group_sum(v, 64);
      if (tid == 0) {
        int ex;
        F.m3[i] = frexp(F.m3[i + 1] * F.sc[1] + v, &ex);
        F.e3[i] = eref + ex;
      }
      __syncthreads();
    }
  }
}

// p[i] = (column-banded table)[i][j] for i = max(1, j-B+1) .. j: sfp_colp(F, t, j) - 1.  Kept beside sfp_colp because the
// outside kernel written with sfp_colp(...) + (klo - 1) compiled to other address arithmetic and took 2 % longer
// (profiles/pf_cells_shared)
__device__ __forceinline__ const double *sfpb_colp(const double *t, int B, int j) {
  return t + ((long long)(j - 1) * B + (B - 1 - j));
}

// Diagonal d < B of the outside pass (d descending from B-1 to TURN+1); groups and rounds as in the inside pass.
__device__ __forceinline__ void sfpb_outside(const SfPfBand &F, int d, int G, size_t gt, size_t nl, const SfDevParams *__restrict__ D,
                                             const SfDevParamsPF *__restrict__ X) {
  const int L = F.L, B = F.B;
  const int r = (int)(gt % (size_t)G);
  const size_t group = gt / (size_t)G, ngroups = nl / (size_t)G;
  const size_t ncell = (size_t)(L - d);
  const size_t rounds = (ncell + ngroups - 1) / ngroups;
  for (size_t it = 0; it < rounds; it++) {
    const size_t cell = group + it * ngroups;
    const bool valid = cell < ncell;
    const int i = (int)cell + 1, j = i + d;
    double a1 = 0.0, o = 0.0, mlsum = 0.0, qbij = 0.0;
    int type = 0;
    if (valid) {
      // A1[i][j] = sum_{k<i} w(k, j) qm[k+1][i-1], k <= i-2-TURN-1; w(k, j) lies in the band for k >= j-B+1
      if (i > 1) {
        const int klo = j - B + 1 > 1 ? j - B + 1 : 1, khi = i - 2 - SFD_TURN - 1;
        const int n = khi - klo + 1;
        if (n > 0) {
          const double *a = sfpb_colp(F.wt, B, j) + klo;             // a[x] = w(klo + x, j)
          const double *b = sfpb_colp(F.qmt, B, i - 1) + (klo + 1);  // b[x] = qm[klo + x + 1][i-1]
          double s1 = 0.0;
          int x = r;
          for (; x + G < n; x += 2 * G) {
            a1 += a[x] * b[x];
            s1 += a[x + G] * b[x + G];
          }
          if (x < n) a1 += a[x] * b[x];
          a1 += s1;
        }
      }
      type = sfp_type(D, F, i, j);
      qbij = F.qb[sfb_row(B, i, j)];
      if (type && qbij != 0.0) {
        // the exterior seed q5[i-1] q3[j+1] / Z_s, from the three mantissas and exponents
        if (r == 0)
          o = ldexp(F.m5[i - 1] * F.m3[j + 1] / F.m5[L] * sfp_ext(X, F, type, i, j), F.e5[i - 1] + F.e3[j + 1] - F.e5[L]);
        if (i > 1 && j < L) {
          const int rt = sfd_rtype(type);
          const int sp1 = F.S[i - 1], sq1 = F.S[j + 1];
          const int u1max = sfd_min(SFD_MAXLOOP, i - 2);
          for (int u1 = 0; u1 <= u1max; u1++) {
            const int kk = i - 1 - u1;
            // l - kk = d + 2 + u1 + u2 stays inside the band: ob is 0 past it
            const int u2max = sfd_min(sfd_min(SFD_MAXLOOP - u1, L - j - 1), B - 1 - (d + 2 + u1));
            const double *row = F.ob + sfb_row(B, kk, kk);  // row[l - kk] = ob[kk][l]
            for (int u2 = r; u2 <= u2max; u2 += G) {
              const int l = j + 1 + u2;
              const double v = row[l - kk];
              if (v == 0.0) continue;
              const int tk = sfp_type(D, F, kk, l);
              if (!tk) continue;
              o += v * sfx_intloop(X, u1, u2, tk, rt, F.S[kk + 1], F.S[l - 1], sp1, sq1) * F.sc[u1 + u2 + 2];
            }
          }
          // sum_{l>j} A1[i][l] ((MLbase/s)^(l-1-j) + qm[j+1][l-1]) + A0[i][l] qm[j+1][l-1]; A0 = A1 = 0 from l = i+B-1 on
          const int lhi = i + B - 2 < L ? i + B - 2 : L;
          const int n = lhi - j;
          if (n > 0) {
            const double *pa1 = F.a1 + sfb_row(B, i, j + 1), *pa0 = F.a0 + sfb_row(B, i, j + 1);  // [x]: l = j+1+x
            const double *pq = F.qm + sfb_row(B, j + 1, j + 1) - 1;  // pq[x] = qm[j+1][j+x] (x >= 1)
            double s1 = 0.0;
            int x = r;
            if (x == 0) { mlsum += pa1[0] * F.mlbs[0]; x += G; }  // l = j+1: qm[j+1][j] is empty
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
    }
    const bool paired = type && qbij != 0.0;
    if (paired && i > 1 && j < L) o += mlsum * sfx_mlstem(X, type, F.S[i - 1], F.S[j + 1]);  // (the cell's factor)
    a1 = sfpl_group_sum(a1, G);
    o = sfpl_group_sum(o, G);
    if (valid && r == 0) {
      const size_t ro = sfb_row(B, i, j);
      double a0 = 0.0;  // (cell (i-1, j) lies on diagonal d + 1: outside the band its A0 and w are 0)
      if (i > 1 && d + 1 < B) a0 = F.a0[sfb_row(B, i - 1, j)] * X->MLbase * F.sc[1] + F.wt[sfb_col(B, j, i - 1)];
      F.a0[ro] = a0;
      F.a1[ro] = a1;
      double ow = 0.0;
      if (paired) {
        ow = o * X->MLclosing * sfx_mlstem(X, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) * F.sc[2];
      } else o = 0.0;
      F.ob[ro] = o;
      F.wt[sfb_col(B, j, i)] = ow;
    }
  }
}
__global__ void sf_pfband_outside_kernel(SfPfBand F, int d, int G, const SfDevParams *__restrict__ D,
                                         const SfDevParamsPF *__restrict__ X) {
  sfpb_outside(F, d, G, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, D, X);
}
__global__ void sf_pfband_prob_kernel(SfPfBand F) {
  sfp_prob(F, ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, ((size_t)gridDim.x * blockDim.x) >> 6);
}
__global__ void sf_pfband_finish_kernel(SfPfBand F, int nwaves) { sfp_finish(F, nwaves); }
