// sf_mfe_banded.hip.h — Zuker MFE fill + traceback of ONE sequence of 1 <= L <= SF_MAX_BANDED under a base-pair span S, in
// BANDED tables (sf_fold_banded): a viral genome, a pre-mRNA or a chromosome region folded with md.max_bp_span set.
//
// With max_pair_dist = S - 1 a cell (i, j) with j - i >= S has pair type 0.  Its c is INF; its fML is finite in full tables, but
// is read only by a c cell that closes a multiloop around it, which lies outside the band too; the exterior loop and the
// traceback follow cells with a pair type only.  So the whole fold lives in the B = min(S, L) diagonals 0 .. B - 1, and
// energies and structures are those of sf_mfe_long.hip.h under the same span, byte for byte: the recurrences, the order of
// the traceback's searches and every helper of the energy model are the same, every search clipped to the band.
//
// Layout (int32, 64-bit offsets throughout; a band table holds L * B entries, the cells 0 <= j - i <= B - 1):
//   fML   row-banded:    row i holds j = i .. i+B-1           sfb_row(B, i, j) = (i-1) B + (j-i)
//   fMLt  the same values column-banded: column j holds i = j-B+1 .. j    sfb_col(B, j, i) = (j-1) B + (i-j+B-1)
//   c     column-banded like fMLt
//   DML   a ring of three diagonals, L + 2 entries each
// The split min_k fML[i][k] + fML[k+1][j] reads row i of fML and column j of fMLt, both contiguous in k, so the lanes of a
// cell read consecutive words; the interior loops of a cell are spread with the 5' gap u1 fastest, so its lanes read
// consecutive words of column q of c.  f5 and the exterior traceback read column j of c contiguously.  Entries of a row or
// column that fall outside the record (j > L, i < 1) exist in memory and are never written or read.
//
// Launches: one fill launch per diagonal d = 0 .. B - 1 and no more; all ordering comes from kernel boundaries (no grid
// barrier, no cooperative launch; the only atomic is the status word).  A diagonal has L - d cells of at most d split terms
// and at most 496 interior-loop candidates each — many cells, short sums, the opposite of sf_long_fill_kernel's late
// diagonals — so the host picks the lanes per cell G (a power of two <= 64) from how many cells the diagonal has against the
// lanes the device holds, and from the cell's work: one lane per cell on a long record, a whole wave on a short one.  Every
// value is an integer minimum: no grouping changes a result.
// Then f5 (sequential in j, at most B terms a step) in one workgroup, and the traceback in one workgroup.
//
// Bracket partners and enclosing pairs are int32 here (SfHc32), built on the host: positions pass 32 767.
// Device memory of one call: 12 L B + 75 L + 4 B + 153 bytes (SF_BANDED_BYTES; the constraint's 9 (L + 2) included).
#pragma once
#include "sf_mfe_full.hip.h"

#define SF_BAND_STACK_INTS(L) (3 * (4 * (size_t)(L) + 8))

__device__ __forceinline__ size_t sfb_row(int B, int i, int j) { return (size_t)(i - 1) * (size_t)B + (size_t)(j - i); }
__device__ __forceinline__ size_t sfb_col(int B, int j, int i) { return (size_t)(j - 1) * (size_t)B + (size_t)(i - j + B - 1); }
// p[i] = (column-banded table)[i][j] for i = max(1, j-B+1) .. j
__device__ __forceinline__ const int32_t *sfb_colptr(const int32_t *t, int B, int j) {
  return t + ((long long)(j - 1) * B + (B - 1 - j));
}

// The device state of one banded fold.  S: codes 0..4 at S[1..L], S[0] = S[L+1] = 0.  hp: hairpin initiation by loop size
// 0..B (the resident model's table only reaches SF_MAX_W + 1).  hc.c == nullptr: no constraint.
struct SfBand {
  const uint8_t *S;
  const int32_t *hp;
  SfHc32 hc;
  int L, B;
  int32_t *c, *fML, *fMLt, *dml, *f5, *stk;
  char *db;
  int *status;
};

__device__ __forceinline__ int sfb_type(const SfDevParams *D, const SfBand &F, int a, int b) {
  const bool ok = b - a <= D->max_pair_dist;
  return sf_hc_type32(F.hc, ok ? D->pair[F.S[a]][F.S[b]] : 0, a, b, ok);
}
__device__ __forceinline__ int sfb_hairpin(const SfDevParams *D, const SfBand &F, int i, int j, int type) {
  const int size = j - i - 1;
  if (size <= SF_MAX_W + 1) return sfd_hairpin(D, F.S, i, j, type);
  return F.hp[size] + D->P.mismatchH[type][F.S[i + 1]][F.S[j - 1]];  // (no special hairpin is that long)
}
__device__ __forceinline__ int sfb_ext(const SfDevParams *D, const SfBand &F, int type, int i, int j) {
  return sfd_extloop(D, type, i > 1 ? F.S[i - 1] : -1, j < F.L ? F.S[j + 1] : -1);
}
__device__ __forceinline__ int sfb_mlstem_out(const SfDevParams *D, const SfBand &F, int type, int i, int j) {
  return sfd_mlstem(D, type, i > 1 ? F.S[i - 1] : -1, j < F.L ? F.S[j + 1] : -1);
}
// interior loop (i, j) -> (p, q) with u1 / u2 unpaired bases; SFD_INF if (p, q) cannot pair
__device__ __forceinline__ int sfb_intloop(const SfDevParams *D, const SfBand &F, int i, int j, int type, int u1, int u2) {
  const int p = i + 1 + u1, q = j - 1 - u2;
  const int t2 = sfb_type(D, F, p, q);
  if (!t2) return SFD_INF;
  return sfd_intloop(D, u1, u2, type, sfd_rtype(t2), F.S[i + 1], F.S[j - 1], F.S[p - 1], F.S[q + 1]) + F.c[sfb_col(F.B, q, p)];
}

// Diagonal d of the fill (d < B).  Thread t of the grid is lane t % G of the group of cell i = t / G + 1; every lane of a wave
// takes part in the butterfly, with or without a cell.
__global__ void sf_band_fill_kernel(SfBand F, int d, int G, const SfDevParams *__restrict__ D) {
  const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = (int)(gt % (size_t)G);
  const size_t cell = gt / (size_t)G;
  const int L = F.L, B = F.B;
  const bool valid = cell < (size_t)(L - d);
  const int i = (int)cell + 1, j = i + d;
  int32_t *dml_d = F.dml + (size_t)(d % 3) * (size_t)(L + 2);
  if (d < SFD_TURN + 1) {  // no pair and no multiloop this short (the same for every thread of the launch)
    if (valid && r == 0) {
      F.c[sfb_col(B, j, i)] = SFD_INF;
      F.fML[sfb_row(B, i, j)] = SFD_INF;
      F.fMLt[sfb_col(B, j, i)] = SFD_INF;
      dml_d[i] = SFD_INF;
    }
    return;
  }
  const sf_params_blob &P = D->P;
  int type = 0, e = SFD_INF, dec = SFD_INF;
  if (valid) {
    type = sfb_type(D, F, i, j);  // max_bp_span, hard constraint
    if (type) {
      if (r == 0) {
        e = sfb_hairpin(D, F, i, j, type);
        const int dml = F.dml[(size_t)((d - 2) % 3) * (size_t)(L + 2) + i + 1];
        if (dml < SFD_INF) e = sfd_min(e, dml + sfd_mlstem(D, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) + P.MLclosing);
      }
      // candidate t: u1 = t & 31 (fastest over the lanes: consecutive words of column q of c), u2 = t >> 5
      const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
      for (int t = r; t < 32 * (umax + 1); t += G) {
        const int u1 = t & 31, u2 = t >> 5;
        if (u1 + u2 <= umax) e = sfd_min(e, sfb_intloop(D, F, i, j, type, u1, u2));
      }
    }
    // DML[i][j] = min_k fML[i][k] + fML[k+1][j], k = i+TURN+1 .. j-TURN-2: row i of fML, column j of fMLt
    const int32_t *a = F.fML + sfb_row(B, i, i);     // a[k - i] = fML[i][k]
    const int32_t *b = sfb_colptr(F.fMLt, B, j) + 1;  // b[k] = fML[k+1][j]
    const int kend = j - SFD_TURN - 2;
    for (int k = i + SFD_TURN + 1 + r; k <= kend; k += G) {
      const int x = a[k - i], y = b[k];
      if (x < SFD_INF && y < SFD_INF) dec = sfd_min(dec, x + y);
    }
  }
  for (int m = G >> 1; m >= 1; m >>= 1) {  // minimum over the cell's group (every lane of the wave takes part)
    const long long o = __shfl_xor((long long)(((unsigned long long)(uint32_t)e << 32) | (uint32_t)dec), m);
    e = sfd_min(e, (int)(o >> 32));
    dec = sfd_min(dec, (int)(uint32_t)o);
  }
  if (valid && r == 0) {
    const int cij = type ? e : SFD_INF;
    F.c[sfb_col(B, j, i)] = cij;
    int f = SFD_INF;
    const int fa = F.fML[sfb_row(B, i + 1, j)], fb = F.fML[sfb_row(B, i, j - 1)];  // diagonal d - 1: inside the band
    if (fa < SFD_INF) f = sfd_min(f, fa + P.MLbase);
    if (fb < SFD_INF) f = sfd_min(f, fb + P.MLbase);
    if (type) f = sfd_min(f, cij + sfb_mlstem_out(D, F, type, i, j));
    dml_d[i] = dec;
    f = sfd_min(f, dec);
    F.fML[sfb_row(B, i, j)] = f;
    F.fMLt[sfb_col(B, j, i)] = f;
  }
}

// f5[j] = min(f5[j-1], min_i f5[i-1] + c[i][j] + ExtLoop(i, j)), i >= max(1, j-B+1); one workgroup (a single wave when the
// band is narrow: its barriers cost nothing then), column j of c read contiguously.
__global__ void sf_band_f5_kernel(SfBand F, const SfDevParams *__restrict__ D, int32_t *mfe_out) {
  __shared__ int red[16];
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L, B = F.B;
  if (tid == 0) F.f5[0] = 0;
  __syncthreads();
  for (int j = 1; j <= L; j++) {
    int v = SFD_INF;
    const int32_t *cj = sfb_colptr(F.c, B, j);  // cj[i] = c[i][j]
    const int lo = j - B + 1 > 1 ? j - B + 1 : 1;
    for (int i = lo + tid; i + SFD_TURN + 1 <= j; i += nt) {
      const int type = sfb_type(D, F, i, j);
      if (type) {
        const int w = cj[i] + sfb_ext(D, F, type, i, j);
        v = sfd_min(v, F.f5[i - 1] + w);
      }
    }
    v = sf_block_min(v, red);
    if (tid == 0) F.f5[j] = sfd_min(F.f5[j - 1], v);
    __syncthreads();
  }
  if (tid == 0 && mfe_out) *mfe_out = F.f5[L];
}

// Traceback in one workgroup: sfl_trace's steps in sfl_trace's order (exterior stem from the largest k down, interior loops in
// (u1, u2) lexicographic order, splits with ascending k), every search clipped to the band.
__global__ void sf_band_trace_kernel(SfBand F, const SfDevParams *__restrict__ D) {
  __shared__ int red[16];
  __shared__ int sh_i, sh_j, sh_ml, sh_s, sh_bad, sh_pair;
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L, B = F.B;
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
      } else if (j - i < SFD_TURN + 1 || j - i >= B) {
        sh_bad = 1;
      } else {
        while (j - i > SFD_TURN + 1 && F.fML[sfb_row(B, i, j - 1)] < SFD_INF &&
               F.fML[sfb_row(B, i, j)] == F.fML[sfb_row(B, i, j - 1)] + P.MLbase) j--;
        while (j - i > SFD_TURN + 1 && F.fML[sfb_row(B, i + 1, j)] < SFD_INF &&
               F.fML[sfb_row(B, i, j)] == F.fML[sfb_row(B, i + 1, j)] + P.MLbase) i++;
        const int type = sfb_type(D, F, i, j);
        pair = type && F.fML[sfb_row(B, i, j)] == F.c[sfb_col(B, j, i)] + sfb_mlstem_out(D, F, type, i, j);
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
      // exterior stem (k, j): k from j-TURN-1 downwards to the band's edge, the first match = the largest k
      const int fij = f5[j];
      const int32_t *cj = sfb_colptr(F.c, B, j);
      const int lo = j - B + 1 > 1 ? j - B + 1 : 1;
      int best = SFD_INF;
      for (int k = j - SFD_TURN - 1 - tid; k >= lo; k -= nt) {
        const int type = sfb_type(D, F, k, j);
        if (type && fij == f5[k - 1] + cj[k] + sfb_ext(D, F, type, k, j)) { best = -k; break; }
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
      const int fij = F.fML[sfb_row(B, i, j)];
      const int32_t *a = F.fML + sfb_row(B, i, i), *b = sfb_colptr(F.fMLt, B, j) + 1;
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
      const int type = sfb_type(D, F, i, j);
      const int cij = F.c[sfb_col(B, j, i)];
      if (cij == sfb_hairpin(D, F, i, j, type)) break;
      // interior loops: p ascending, then q descending = (u1, u2) in lexicographic order
      const int d = j - i;
      const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
      int best = SFD_INF;
      for (int t = tid; t < 32 * 32; t += nt) {
        const int u1 = t >> 5, u2 = t & 31;
        if (u1 + u2 > umax) continue;
        if (cij == sfb_intloop(D, F, i, j, type, u1, u2)) { best = t; break; }
      }
      best = sf_block_min(best, red);
      if (best != SFD_INF) {
        i = i + 1 + (best >> 5);
        j = j - 1 - (best & 31);
        continue;
      }
      // multiloop closed by (i, j): split of fML[i+1][j-1] with ascending k
      const int mm = P.MLclosing + sfd_mlstem(D, sfd_rtype(type), F.S[j - 1], F.S[i + 1]);
      const int32_t *a = F.fML + sfb_row(B, i + 1, i + 1), *b = sfb_colptr(F.fMLt, B, j - 1) + 1;
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
