// sf_duplex.hip.h — duplex folds on the device (include/scanfold_hip_duplex.h).
//
// Replaces RNA.duplexfold(frag, dup_frag) in the k-mer double loop of ScanFold.py:773-812 and the 101 folds per hit of
// cofold_energies (ScanFoldFunctions.py:817-829).  The model is ViennaRNA's duplexfold as DESIGN.md states it: only
// inter-strand pairs, dangles = 2, interior loops up to SF_MAXLOOP, DuplexInit once;
//   c[i][j] = min(DuplexInit + ext(type, s1[i-1], s2[j+1]),
//                 min over k < i, l > j of c[k][l] + intloop(i-k-1, l-j-1, type(k,l), rtype(type(i,j)), ...))
//   E(i,j)  = c[i][j] + ext(rtype(type), s2[j-1], s1[i+1]);   Emin = first strict minimum for i = 1..n1, j = n2..1.
//
// Mapping: ONE LANE PER DUPLEX, one DP body (sf_duplex_fill) for every use.
//  * all-pairs scan (sf_lri_scan_kernel): a 64-lane workgroup takes one j_win and 64 consecutive k_win.  Strand 1, both
//    lengths and therefore the whole loop nest (i, j, k, l) are the same in every lane: loop sizes, the case analysis of
//    sfd_intloop and every strand-1 index are scalar, only strand-2 codes, pair types and table values differ per lane.
//    The c table is int16 [cell][lane] in LDS (two lanes per bank, conflict-free): 128 * n1 * n2 bytes per wave, 51 kB at
//    k = 20.  Past the LDS budget (35 < k <= SF_DUPLEX_MAX_LEN) the same table lives in device memory, [cell][thread], coalesced.
//  * arbitrary pairs (sf_duplex_batch_kernel): each lane has its own strands and lengths, the table is in device memory,
//    and the lane walks the traceback itself.  The backgrounds of the hits are this kernel on rows sf_lri_shuffle_kernel made.
#pragma once
#include "../../include/scanfold_hip_duplex.h"
#include "sf_energy.h"
#include "sf_shuffle.hip.h"

#define SF_DUP_INF16 32767  // c[i][j] of two bases that cannot pair; real entries stay far below (header: SF_DUPLEX_MAX_LEN)
#define SF_DUP_BLOCK 64
#define SF_DUP_LDS_BUDGET (160 * 1024)  // one workgroup may take all of a CU's LDS

// pair type of two nucleotide codes (sf_params_blob.h: 1 CG, 2 GC, 3 GU, 4 UG, 5 AU, 6 UA), from a 3-bit-per-entry constant:
// no memory access, and no table gather where the codes differ per lane
__device__ __forceinline__ int sf_dup_pair(int a, int b) {
  // row a = 5 entries of 3 bits, entry b at bit 3 b:   A: U->5   C: G->1   G: C->2, U->3   U: A->6, G->4
  const uint32_t row = a == 1 ? (5u << 12) : a == 2 ? (1u << 9) : a == 3 ? ((2u << 6) | (3u << 12)) : a == 4 ? ((6u << 3) | (4u << 9)) : 0u;
  return (int)((row >> (3 * b)) & 7u);
}

// strand accessors: 1-based position -> code 0..4
struct SfDupRow {  // contiguous codes
  const uint8_t *p;
  __device__ __forceinline__ int operator()(int x) const { return p[x - 1]; }
};
struct SfDupCol {  // [position][lane] image in LDS
  const uint8_t *p;
  __device__ __forceinline__ int operator()(int x) const { return p[(x - 1) * SF_DUP_BLOCK]; }
};
// the c table of one lane: cell (i, j) at p[((i-1) * n2 + (j-1)) * stride]
struct SfDupTable {
  int16_t *p;
  int n2, stride;
  __device__ __forceinline__ int get(int i, int j) const { return p[(size_t)((i - 1) * n2 + (j - 1)) * stride]; }
  __device__ __forceinline__ void set(int i, int j, int v) const { p[(size_t)((i - 1) * n2 + (j - 1)) * stride] = (int16_t)v; }
};

struct SfDupBest {
  int e, i, j;  // Emin (SFD_INF: no pair), and the cell it was found at
};

template <class S1, class S2>
__device__ __forceinline__ SfDupBest sf_duplex_fill(const SfDevParams *D, const S1 &s1, int n1, const S2 &s2, int n2,
                                                    const SfDupTable &c) {
  SfDupBest best = {SFD_INF, 0, 0};
  const int dinit = D->P.DuplexInit;
  for (int i = 1; i <= n1; i++) {
    const int a = s1(i), am = i > 1 ? s1(i - 1) : -1, ap = i < n1 ? s1(i + 1) : -1;
    for (int j = n2; j >= 1; j--) {
      const int type = sf_dup_pair(a, s2(j));
      if (!type) {
        c.set(i, j, SF_DUP_INF16);
        continue;
      }
      const int bp = j < n2 ? s2(j + 1) : -1, bm = j > 1 ? s2(j - 1) : -1;
      const int rt = sfd_rtype(type);
      int e = dinit + sfd_extloop(D, type, am, bp);
      for (int k = i - 1; k >= 1 && i - k - 1 <= SFD_MAXLOOP; k--) {
        const int ak = s1(k), ak1 = s1(k + 1);
        for (int l = j + 1; l <= n2 && (i - k - 1) + (l - j - 1) <= SFD_MAXLOOP; l++) {
          const int ckl = c.get(k, l);
          if (ckl == SF_DUP_INF16) continue;
          const int t2 = sf_dup_pair(ak, s2(l));
          e = sfd_min(e, ckl + sfd_intloop(D, i - k - 1, l - j - 1, t2, rt, ak1, s2(l - 1), am, bp));
        }
      }
      c.set(i, j, e);
      const int E = e + sfd_extloop(D, rt, bm, ap);
      if (E < best.e) {
        best.e = E;
        best.i = i;
        best.j = j;
      }
    }
  }
  return best;
}

// duplexT's .i / .j of a fill result
__device__ __forceinline__ void sf_dup_record(const SfDupBest &b, int n1, int *e, int *i, int *j) {
  if (b.e >= SFD_INF) {
    *e = SF_DUPLEX_NONE; *i = 0; *j = 0;
  } else {
    *e = b.e; *i = b.i < n1 ? b.i + 1 : n1; *j = b.j > 1 ? b.j - 1 : 1;
  }
}

// Traceback from (b.i, b.j): at each cell the first (k, l), k = i-1 downwards, l = j+1 upwards, whose sum equals c[i][j]; a
// cell none matches must equal its own initial term and ends the helix.  Writes duplexT's structure; returns 0, or 1 if the
// last cell is not its initial term.
template <class S1, class S2>
__device__ inline int sf_duplex_trace(const SfDevParams *D, const S1 &s1, int n1, const S2 &s2, int n2, const SfDupTable &c,
                                      const SfDupBest &b, char *out) {
  if (b.e >= SFD_INF) {
    out[0] = '&'; out[1] = 0;
    return 0;
  }
  uint64_t m1 = 0, m2 = 0;  // paired positions of the two strands
  int i = b.i, j = b.j, bad = 0;
  for (;;) {
    m1 |= 1ull << (i - 1);
    m2 |= 1ull << (j - 1);
    const int E = c.get(i, j);
    const int type = sf_dup_pair(s1(i), s2(j)), rt = sfd_rtype(type);
    const int am = i > 1 ? s1(i - 1) : -1, bp = j < n2 ? s2(j + 1) : -1;
    int traced = 0;
    for (int k = i - 1; k >= 1 && i - k - 1 <= SFD_MAXLOOP && !traced; k--)
      for (int l = j + 1; l <= n2 && (i - k - 1) + (l - j - 1) <= SFD_MAXLOOP; l++) {
        const int ckl = c.get(k, l);
        if (ckl == SF_DUP_INF16) continue;
        const int t2 = sf_dup_pair(s1(k), s2(l));
        if (E == ckl + sfd_intloop(D, i - k - 1, l - j - 1, t2, rt, s1(k + 1), s2(l - 1), am, bp)) {
          i = k; j = l; traced = 1;
          break;
        }
      }
    if (!traced) {
      if (E != D->P.DuplexInit + sfd_extloop(D, type, am, bp)) bad = 1;
      break;
    }
  }
  const int i0 = b.i < n1 ? b.i + 1 : n1, j0 = b.j > 1 ? b.j - 1 : 1;
  const int ia = i > 1 ? i - 1 : i, jb = j < n2 ? j + 1 : j;
  int o = 0;
  for (int x = ia; x <= i0; x++) out[o++] = ((m1 >> (x - 1)) & 1) ? '(' : '.';
  out[o++] = '&';
  for (int x = j0; x <= jb; x++) out[o++] = ((m2 >> (x - 1)) & 1) ? ')' : '.';
  out[o] = 0;
  return bad;
}

// ---------------- (a) the all-pairs scan ----------------
struct SfLriScan {
  const uint8_t *codes;  // the record as codes 0..4, L bytes
  int L, kmer, step, n_j, n_k, n_chunk;  // n_chunk = ceil(n_k / 64) workgroup tasks per j_win
  int cutoff;                            // dcal/mol
  unsigned max_hits;
  sf_lri_hit *hits;                      // compacted mode
  unsigned *n_hits;                      // every hit counts, stored or not
  int32_t *dense_e, *dense_i, *dense_j;  // dense mode (all three, or none)
  int16_t *scratch;                      // c tables in device memory (LDSC = false): cells * gridDim.x * 64 entries
};

// LDS (LDSC): c[n1 * n2][64] int16, then strand 2 as [kmer][64] bytes, then strand 1 (kmer bytes)
template <bool LDSC>
__global__ void __launch_bounds__(SF_DUP_BLOCK) sf_lri_scan_kernel(SfLriScan A, long long task0, long long task1,
                                                                    const SfDevParams *__restrict__ D) {
  SF_DYN_SMEM(smem);
  const int lane = threadIdx.x;
  const int kmer = A.kmer;
  int16_t *ctab;
  uint8_t *s2img, *s1img;
  if (LDSC) {
    ctab = (int16_t *)smem + lane;
    s2img = (uint8_t *)smem + (size_t)kmer * kmer * SF_DUP_BLOCK * sizeof(int16_t);
  } else {
    ctab = A.scratch + (size_t)blockIdx.x * SF_DUP_BLOCK + lane;
    s2img = (uint8_t *)smem;
  }
  s1img = s2img + (size_t)kmer * SF_DUP_BLOCK;
  const int cstride = LDSC ? SF_DUP_BLOCK : (int)(gridDim.x * SF_DUP_BLOCK);

  for (long long t = task0 + blockIdx.x; t < task1; t += gridDim.x) {
    const int jx = (int)(t / A.n_chunk), kx0 = (int)(t % A.n_chunk) * SF_DUP_BLOCK;
    const int j_win = jx * A.step;
    const int kx = kx0 + lane, k_win = kx * A.step;
    const bool scanned = kx < A.n_k && ((k_win + 3) < (j_win - kmer) || k_win > (j_win + kmer + 3));
    // the same test on the first and the last k_win of the chunk: does any lane have work?
    const int kx1 = (kx0 + SF_DUP_BLOCK - 1 < A.n_k ? kx0 + SF_DUP_BLOCK - 1 : A.n_k - 1);
    const bool any = (kx0 * A.step + 3) < (j_win - kmer) || kx1 * A.step > (j_win + kmer + 3);
    int e = SF_DUPLEX_SKIPPED, ri = 0, rj = 0;
    // Lanes of a working chunk that are not scanned (the band around the diagonal, the tail past n_k) fold the record's first
    // k-mer and drop the result: the loop nest is the same in every lane, so masking them off would not shorten the wave.
    if (any) {
      const int n1 = A.L - j_win < kmer ? A.L - j_win : kmer;
      const uint8_t *src2 = A.codes + (scanned ? k_win : 0);
      __syncthreads();  // the previous task's strands are no longer read
      for (int x = 0; x < kmer; x++) s2img[x * SF_DUP_BLOCK + lane] = src2[x];
      for (int x = lane; x < n1; x += SF_DUP_BLOCK) s1img[x] = A.codes[j_win + x];
      __syncthreads();
      const SfDupRow s1 = {s1img};
      const SfDupCol s2 = {s2img + lane};
      const SfDupTable c = {ctab, kmer, cstride};
      const SfDupBest b = sf_duplex_fill(D, s1, n1, s2, kmer, c);
      if (scanned) sf_dup_record(b, n1, &e, &ri, &rj);
    }
    if (A.dense_e) {
      if (kx < A.n_k) {
        const size_t o = (size_t)jx * A.n_k + kx;
        A.dense_e[o] = e; A.dense_i[o] = ri; A.dense_j[o] = rj;
      }
    } else if (scanned && e != SF_DUPLEX_NONE && e < A.cutoff) {
      const unsigned slot = atomicAdd(A.n_hits, 1u);
      if (slot < A.max_hits) {
        sf_lri_hit h = {j_win, k_win, e, ri, rj};
        A.hits[slot] = h;
      }
    }
  }
}

// ---------------- (b) arbitrary pairs ----------------
struct SfDupBatch {
  const uint8_t *s1, *s2;  // codes; row p at p * ld
  const int32_t *len1, *len2;  // per pair, or null: n1 / n2 for every pair
  int n, ld, n1, n2, max2;     // max2: row length of the c table (the longest strand 2)
  int16_t *scratch;            // max1 * max2 * gridDim.x * 64 entries
  int32_t *e, *i, *j;          // i / j may be null
  char *structure;             // null, or rows of SF_DUPLEX_STRUCT_LEN
  int *status;
};

__global__ void __launch_bounds__(SF_DUP_BLOCK) sf_duplex_batch_kernel(SfDupBatch A, const SfDevParams *__restrict__ D) {
  const int stride = (int)(gridDim.x * SF_DUP_BLOCK);
  const int tid = (int)(blockIdx.x * SF_DUP_BLOCK + threadIdx.x);
  const SfDupTable c = {A.scratch + tid, A.max2, stride};
  for (int p = tid; p < A.n; p += stride) {
    const int n1 = A.len1 ? A.len1[p] : A.n1, n2 = A.len2 ? A.len2[p] : A.n2;
    const SfDupRow s1 = {A.s1 + (size_t)p * A.ld}, s2 = {A.s2 + (size_t)p * A.ld};
    const SfDupBest b = sf_duplex_fill(D, s1, n1, s2, n2, c);
    int e, ri, rj;
    sf_dup_record(b, n1, &e, &ri, &rj);
    A.e[p] = e;
    if (A.i) A.i[p] = ri;
    if (A.j) A.j[p] = rj;
    if (A.structure && sf_duplex_trace(D, s1, n1, s2, n2, c, b, A.structure + (size_t)p * SF_DUPLEX_STRUCT_LEN))
      atomicOr(A.status, 1);
  }
}

// ---------------- (c) the shuffled rows behind a hit's z-score ----------------
// One thread per (hit, element): rows1 = a mono shuffle of the hit's strand 1 (element 0 too: ScanFoldFunctions.py:820),
// rows2 = the native strand 2 (element 0) or its shuffle.  Rows are kmer codes; len1 receives strand 1's length.
// LDS per block: out[64][kmer] + lst[64][kmer] + cnt[64][25] uint16, as sf_shuffle_kernel.
__global__ void sf_lri_shuffle_kernel(const uint8_t *__restrict__ codes, int L, int kmer, const int32_t *__restrict__ j_win,
                                      const int32_t *__restrict__ k_win, int n_hits, int r, int kind, uint64_t seed,
                                      uint8_t *__restrict__ rows1, uint8_t *__restrict__ rows2, int32_t *__restrict__ len1) {
  SF_DYN_SMEM(smem);
  uint8_t *outs = (uint8_t *)smem;
  uint8_t *lsts = outs + (size_t)SF_SHUF_BLOCK * kmer;
  uint16_t *cnts = (uint16_t *)(lsts + (((size_t)SF_SHUF_BLOCK * kmer + 3) & ~(size_t)3));
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * SF_SHUF_BLOCK + lane;
  if (row >= (long long)n_hits * (r + 1)) return;
  uint8_t *out = outs + (size_t)lane * kmer, *lst = lsts + (size_t)lane * kmer;
  uint16_t *cnt = cnts + lane * 25;
  const int h = (int)(row / (r + 1)), el = (int)(row % (r + 1));
  const int jw = j_win[h], kw = k_win[h];
  const int n1 = L - jw < kmer ? L - jw : kmer;
  SfPhilox g;
  g.k0 = (uint32_t)seed; g.k1 = (uint32_t)(seed >> 32);
  g.c0 = 0; g.c1 = (uint32_t)el; g.c2 = (uint32_t)jw; g.c3 = (uint32_t)kw;  // strand 1: stream bit 31 of c1 clear
  g.have = 0;
  uint8_t *d1 = rows1 + (size_t)row * kmer, *d2 = rows2 + (size_t)row * kmer;
  sf_shuffle_row(codes + jw, n1, SF_SHUFFLE_MONO, g, out, lst, cnt);
  for (int x = 0; x < kmer; x++) d1[x] = x < n1 ? out[x] : 0;
  len1[row] = n1;
  if (el == 0) {
    for (int x = 0; x < kmer; x++) d2[x] = codes[kw + x];
  } else {
    g.c0 = 0; g.c1 = (uint32_t)el | 0x80000000u | ((uint32_t)kind << 30);  // strand 2: its own stream, per shuffle kind
    g.have = 0;
    sf_shuffle_row(codes + kw, kmer, kind, g, out, lst, cnt);
    for (int x = 0; x < kmer; x++) d2[x] = out[x];
  }
}
