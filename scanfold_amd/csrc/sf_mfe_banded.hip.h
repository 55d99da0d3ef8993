// sf_mfe_banded.hip.h — Zuker MFE fill + traceback of ONE sequence of 1 <= L <= SF_MAX_BANDED under a base-pair span S, in
// BANDED tables (sf_fold_banded): a viral genome, a pre-mRNA or a chromosome region folded with md.max_bp_span set.
//
// With max_pair_dist = S - 1 a cell (i, j) with j - i >= S has pair type 0.  Its c is INF; its fML is finite in full tables, but
// is read only by a c cell that closes a multiloop around it, which lies outside the band too; the exterior loop and the
// traceback follow cells with a pair type only.  So the whole fold lives in the B = min(S, L) diagonals 0 .. B - 1, and
// energies and structures are those of sf_mfe_long.hip.h under the same span, byte for byte: the recurrences, the order of
// the traceback's searches and every helper of the energy model are the same code (the templates of sf_mfe_trace.hip.h),
// every search clipped to the band.
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
// Then f5 (sequential in j, at most B terms a step) in one workgroup, and the traceback (sft_trace) in one workgroup.
//
// Bracket partners and enclosing pairs are int32 here (SfHc32): positions pass 32 767.  The host builds them, as it does
// the int16 ones of the full tables (hc_parse_host in scanfold_hip.hip).
// Device memory of one call: 12 L B + 75 L + 4 B + 153 bytes (SF_BANDED_BYTES; the constraint's 9 (L + 2) included).
#pragma once
#include "sf_mfe_trace.hip.h"

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

// the layout as sf_mfe_trace.hip.h's templates see it
__device__ __forceinline__ int sft_type(const SfDevParams *D, const SfBand &F, int a, int b) {
  const bool ok = b - a <= D->max_pair_dist;
  return sf_hc_type_of(F.hc, ok ? D->pair[F.S[a]][F.S[b]] : 0, a, b, ok);
}
__device__ __forceinline__ size_t sft_row(const SfBand &F, int i, int j) { return sfb_row(F.B, i, j); }
__device__ __forceinline__ size_t sft_col(const SfBand &F, int j, int i) { return sfb_col(F.B, j, i); }
__device__ __forceinline__ const int32_t *sft_colp(const SfBand &F, const int32_t *t, int j) { return sfb_colptr(t, F.B, j); }
__device__ __forceinline__ int sft_lo(const SfBand &F, int j) { return j - F.B + 1 > 1 ? j - F.B + 1 : 1; }
__device__ __forceinline__ bool sft_in(const SfBand &F, int i, int j) { return j - i < F.B; }

// Cell i = cell + 1 of diagonal d of the fill (d < B), as lane r of its group of G; every lane of a wave takes part in the
// butterfly, with or without a cell.  The body of sf_band_fill_kernel and of sf_bandb_fill_kernel (sf_mfe_banded_batch.hip.h).
__device__ __forceinline__ void sfb_fill_cell(const SfBand &F, int d, int G, int r, size_t cell, const SfDevParams *D) {
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
    type = sft_type(D, F, i, j);  // max_bp_span, hard constraint
    if (type) {
      if (r == 0) {
        e = sft_hairpin(D, F, i, j, type);
        const int dml = F.dml[(size_t)((d - 2) % 3) * (size_t)(L + 2) + i + 1];
        if (dml < SFD_INF) e = sfd_min(e, dml + sfd_mlstem(D, sfd_rtype(type), F.S[j - 1], F.S[i + 1]) + P.MLclosing);
      }
      // candidate t: u1 = t & 31 (fastest over the lanes: consecutive words of column q of c), u2 = t >> 5
      const int umax = sfd_min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
      for (int t = r; t < 32 * (umax + 1); t += G) {
        const int u1 = t & 31, u2 = t >> 5;
        if (u1 + u2 <= umax) e = sfd_min(e, sft_intloop(D, F, i, j, type, u1, u2));
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
    if (type) f = sfd_min(f, cij + sft_mlstem_out(D, F, type, i, j));
    dml_d[i] = dec;
    f = sfd_min(f, dec);
    F.fML[sfb_row(B, i, j)] = f;
    F.fMLt[sfb_col(B, j, i)] = f;
  }
}

// Thread t of the grid is lane t % G of the group of cell i = t / G + 1.
__global__ void sf_band_fill_kernel(SfBand F, int d, int G, const SfDevParams *__restrict__ D) {
  const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  sfb_fill_cell(F, d, G, (int)(gt % (size_t)G), gt / (size_t)G, D);
}

// f5[j] = min(f5[j-1], min_i f5[i-1] + c[i][j] + ExtLoop(i, j)), i >= max(1, j-B+1); one workgroup (a single wave when the
// band is narrow: its barriers cost nothing then), column j of c read contiguously.
__device__ __forceinline__ void sfb_f5(const SfBand &F, const SfDevParams *D, int32_t *mfe_out) {
  __shared__ int red[16];
  const int tid = threadIdx.x, nt = blockDim.x, L = F.L, B = F.B;
  if (tid == 0) F.f5[0] = 0;
  __syncthreads();
  for (int j = 1; j <= L; j++) {
    int v = SFD_INF;
    const int32_t *cj = sfb_colptr(F.c, B, j);  // cj[i] = c[i][j]
    const int lo = j - B + 1 > 1 ? j - B + 1 : 1;
    for (int i = lo + tid; i + SFD_TURN + 1 <= j; i += nt) {
      const int type = sft_type(D, F, i, j);
      if (type) {
        const int w = cj[i] + sft_ext(D, F, type, i, j);
        v = sfd_min(v, F.f5[i - 1] + w);
      }
    }
    v = sf_block_min(v, red);
    if (tid == 0) F.f5[j] = sfd_min(F.f5[j - 1], v);
    __syncthreads();
  }
  if (tid == 0 && mfe_out) *mfe_out = F.f5[L];
}
__global__ void sf_band_f5_kernel(SfBand F, const SfDevParams *__restrict__ D, int32_t *mfe_out) { sfb_f5(F, D, mfe_out); }
__global__ void sf_band_trace_kernel(SfBand F, const SfDevParams *__restrict__ D) { sft_trace(F, D); }
