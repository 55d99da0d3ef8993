// sf_pf_probs.hip.h — the base-pair probabilities of a whole-record partition function, brought out of the device: what
// sfp_prob (sf_pf_cells.hip.h) forms for the centroid and throws away.  Function templates over the state T, as sfp_prob is;
// they see the tables only through sfp_row, sfp_xhi and sfp_z and read ob and qb as the outside pass left them (neither is
// aliased after it).  Instantiated for SfPfBand only (sf_pf_banded_probs); SfPfLong can follow.
//
// The probability of a kept cell is sfp_prob's expression to the letter, p = ob[x] * qb[x] / sfp_z, a cell with qb == 0
// being skipped: a listed p is the number the centroid was decided on.
//
// Per-nucleotide pass.  paired[k] = sum_j p(k, j) + sum_i p(i, k) and h[k] = sum p log2 p over the same terms (a term with
// p <= 0 adds 0); unpaired[k] = clamp(1 - paired[k], 0, 1); entropy[k] = -h[k] - unpaired[k] log2 unpaired[k] with
// 0 log 0 = 0.  The positional entropy is in BITS (log2).  No parity with another package's entropy track is claimed.
//   * Row part (sfp_nuc_rows): sfp_prob's walk.  A wave takes rows wave, wave + nwaves, ...; lane l reads x = TURN+1+l,
//     +64, ... of the row's run and the 64 partial sums are added in a __shfl_xor butterfly.  It leaves paired's and h's
//     row parts in the two output vectors.
//   * Column part (sfp_nuc_cols), in a launch after it.  The tables are stored by rows, so a column is a stride of B - 1
//     doubles; instead a wave owns the 64 consecutive columns [j0, j0 + 64) and walks the rows i = max(1, j0 - B + 1) ..
//     min(L, j0 + 62 - TURN) in ascending order (B - 1 is sfp_xhi(F, 1), the widest row's run).  On row i lane l reads
//     element x = j0 + l - i of the row's run where TURN + 1 <= x <= sfp_xhi(F, i): the 64 lanes read 64 neighbouring
//     doubles of ONE row of ob and of qb, so every access of the wave is one contiguous run of at most 512 bytes.  Each lane keeps its own column's two sums, in ascending i;
//     no lane ever adds another lane's term, so there is no reduction at all.  The lane then adds its sums to the row
//     parts of its own position and finishes unpaired and entropy in place.
// The order of every sum is a function of L and B alone (not even of the number of waves): two calls return the same bits.
//
// Sparse pair list: all (i, j, p) with p >= cutoff as 16-byte records {int32 i, int32 j, double p}, 1-based, i < j, sorted
// by i and then by j.  Three steps, no atomics of any kind:
//   1. sfp_pairs_count: a wave per row; over 64-cell chunks of the row's run, __ballot of "p >= cutoff" and __popcll; one
//      int32 count per row.
//   2. an exclusive scan of the L counts into 64-bit offsets, on the HOST over the copied counts (sf_pf_banded_probs,
//      scanfold_hip.hip: 4 L bytes down, 8 L bytes up; the list's device buffer is allocated between the two, once the
//      total is known).
//   3. sfp_pairs_write: the same walk; the lane of a listed cell puts its record at
//      offset[row] + (records of the row's chunks before) + __popcll(ballot & lanes below).
// The place of a record is a function of the probabilities alone: the order is the definition, not an accident of scheduling.
//
// Wave-level primitives used: __shfl_xor, __ballot, __popcll; every lane of a wave takes part in each of them (the loops
// over chunks have wave-uniform bounds).
#pragma once
#include "sf_pf_cells.hip.h"

struct SfPairProb {  // sf_pair_prob of include/scanfold_hip_long.h
  int32_t i, j;
  double p;
};

// row parts of paired and h into unp[i - 1] and ent[i - 1]
template <class T>
__device__ __forceinline__ void sfp_nuc_rows(const T &F, size_t wave, size_t nwaves, double *__restrict__ unp,
                                             double *__restrict__ ent) {
  const int L = F.L, lane = threadIdx.x & 63;
  const double Z = sfp_z(F);
  for (size_t i = wave + 1; i <= (size_t)L; i += nwaves) {
    const double *po = F.ob + sfp_row(F, (int)i, (int)i), *pq = F.qb + sfp_row(F, (int)i, (int)i);
    const int xhi = sfp_xhi(F, (int)i);
    double s = 0.0, h = 0.0;
    for (int x = SFD_TURN + 1 + lane; x <= xhi; x += 64) {
      const double q = pq[x];
      if (q == 0.0) continue;
      const double p = po[x] * q / Z;
      s += p;
      if (p > 0.0) h += p * log2(p);
    }
    s = sfpl_group_sum(s, 64);
    h = sfpl_group_sum(h, 64);
    if (lane == 0) { unp[i - 1] = s; ent[i - 1] = h; }
  }
}

// column parts, added to the row parts; unpaired and entropy finished in place.  A wave takes the column blocks wave,
// wave + nwaves, ... of 64 columns each.
template <class T>
__device__ __forceinline__ void sfp_nuc_cols(const T &F, size_t wave, size_t nwaves, double *__restrict__ unp,
                                             double *__restrict__ ent) {
  const int L = F.L, lane = threadIdx.x & 63;
  const double Z = sfp_z(F);
  const size_t nblk = ((size_t)L + 63) / 64;
  for (size_t blk = wave; blk < nblk; blk += nwaves) {
    const int j0 = (int)(blk * 64) + 1, j = j0 + lane;
    // rows that keep a cell of one of the block's columns: j - i <= sfp_xhi(F, i) <= sfp_xhi(F, 1), the widest row's
    int ilo = j0 - sfp_xhi(F, 1), ihi = j0 + 62 - SFD_TURN;
    if (ilo < 1) ilo = 1;
    if (ihi > L) ihi = L;
    double s = 0.0, h = 0.0;
    for (int i = ilo; i <= ihi; i++) {
      const int xhi = sfp_xhi(F, i), x = j - i;
      if (j > L || x < SFD_TURN + 1 || x > xhi) continue;
      const size_t o = sfp_row(F, i, i) + (size_t)x;
      const double q = F.qb[o];
      if (q == 0.0) continue;
      const double p = F.ob[o] * q / Z;
      s += p;
      if (p > 0.0) h += p * log2(p);
    }
    if (j <= L) {
      double u = 1.0 - (unp[j - 1] + s);
      u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
      const double hh = ent[j - 1] + h;
      unp[j - 1] = u;
      ent[j - 1] = (0.0 - hh) - (u > 0.0 ? u * log2(u) : 0.0);
    }
  }
}

// One row's chunks for the two list passes: calls put(mask, pred, x, p, before) in every lane once per chunk, `before`
// being the row's listed cells in the chunks before it; -> the row's count.
template <class T, class Put>
__device__ __forceinline__ int sfp_pairs_row(const T &F, int i, double Z, double cutoff, Put put) {
  const int lane = threadIdx.x & 63;
  const double *po = F.ob + sfp_row(F, i, i), *pq = F.qb + sfp_row(F, i, i);
  const int xhi = sfp_xhi(F, i);
  int n = 0;
  for (int x0 = SFD_TURN + 1; x0 <= xhi; x0 += 64) {  // (wave-uniform bounds: every lane reaches the ballot)
    const int x = x0 + lane;
    double p = 0.0;
    bool in = false;
    if (x <= xhi) {
      const double q = pq[x];
      if (q != 0.0) {
        p = po[x] * q / Z;
        in = p >= cutoff;
      }
    }
    const unsigned long long mask = __ballot(in);
    put(mask, in, x, p, n);
    n += __popcll(mask);
  }
  return n;
}

template <class T>
__device__ __forceinline__ void sfp_pairs_count(const T &F, size_t wave, size_t nwaves, double cutoff, int32_t *__restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const double Z = sfp_z(F);
  for (size_t i = wave + 1; i <= (size_t)F.L; i += nwaves) {
    const int n = sfp_pairs_row(F, (int)i, Z, cutoff, [](unsigned long long, bool, int, double, int) {});
    if (lane == 0) cnt[i - 1] = n;
  }
}

// off: the exclusive scan of cnt; total: the length of the list (no record is written at or past it)
template <class T>
__device__ __forceinline__ void sfp_pairs_write(const T &F, size_t wave, size_t nwaves, double cutoff,
                                                const unsigned long long *__restrict__ off, unsigned long long total,
                                                SfPairProb *__restrict__ list) {
  const int lane = threadIdx.x & 63;
  const double Z = sfp_z(F);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (size_t i = wave + 1; i <= (size_t)F.L; i += nwaves) {
    const unsigned long long base = off[i - 1];
    sfp_pairs_row(F, (int)i, Z, cutoff, [&](unsigned long long mask, bool in, int x, double p, int before) {
      if (!in) return;
      const unsigned long long at = base + (unsigned long long)before + (unsigned long long)__popcll(mask & below);
      if (at < total) {
        SfPairProb r;
        r.i = (int32_t)i;
        r.j = (int32_t)i + x;
        r.p = p;
        list[at] = r;
      }
    });
  }
}

// ---- banded tables (sf_pf_banded_probs); the waves of a launch as sf_pfband_prob_kernel counts them ----
#include "sf_pf_banded.hip.h"

__device__ __forceinline__ size_t sfp_wave() { return ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
__device__ __forceinline__ size_t sfp_nwaves() { return ((size_t)gridDim.x * blockDim.x) >> 6; }

__global__ void sf_pfband_nuc_rows_kernel(SfPfBand F, double *__restrict__ unp, double *__restrict__ ent) {
  sfp_nuc_rows(F, sfp_wave(), sfp_nwaves(), unp, ent);
}
__global__ void sf_pfband_nuc_cols_kernel(SfPfBand F, double *__restrict__ unp, double *__restrict__ ent) {
  sfp_nuc_cols(F, sfp_wave(), sfp_nwaves(), unp, ent);
}
__global__ void sf_pfband_pairs_count_kernel(SfPfBand F, double cutoff, int32_t *__restrict__ cnt) {
  sfp_pairs_count(F, sfp_wave(), sfp_nwaves(), cutoff, cnt);
}
__global__ void sf_pfband_pairs_write_kernel(SfPfBand F, double cutoff, const unsigned long long *__restrict__ off,
                                             unsigned long long total, SfPairProb *__restrict__ list) {
  sfp_pairs_write(F, sfp_wave(), sfp_nwaves(), cutoff, off, total, list);
}
