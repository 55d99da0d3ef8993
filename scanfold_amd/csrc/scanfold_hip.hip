// scanfold_hip.hip — host side of libscanfold_hip.so: the C ABI of include/scanfold_hip.h over the HIP kernels.
//
// The reference drives this path from Python with a 12-process pool created per call
// (ScanFold-Scan.py:73-77,256,274); here one process owns one GPU and every call is a few batched launches
// on one HIP stream.  No CPU compute path exists in this file: without a GPU sf_init fails.
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/scanfold_hip_long.h"
#include "sf_launch.h"
#include "sf_energy.h"
#include "sf_mfe_full.hip.h"
#include "sf_mfe_fast.hip.h"
#include "sf_mfe_long.hip.h"
#include "sf_mfe_long_batch.hip.h"
#include "sf_mfe_banded.hip.h"
#include "sf_mfe_banded_batch.hip.h"
#include "sf_pf.hip.h"
#include "sf_pf_long.hip.h"
#include "sf_pf_long_batch.hip.h"
#include "sf_pf_banded.hip.h"
#include "sf_pf_probs.hip.h"
#include "sf_mea.hip.h"
#include "sf_pf_fast.hip.h"
#include "sf_pf_lds.hip.h"
#include "sf_shuffle.hip.h"
#include "sf_tabulate.hip.h"
#include "sf_duplex.hip.h"

namespace {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

struct Ctx {
  bool init = false;
  bool have_params = false;
  int dev = 0;
  int n_cu = 0;
  std::string dev_name;
  hipStream_t stream = nullptr;
  SfDevParams *dP = nullptr;  // the resident model the launches use: one of the two slots below
  SfDevParamsPF *dX = nullptr;
  SfFastParams *dF = nullptr;
  // Two models stay resident (a scan with -t folds the native windows at T and the shuffles at 37 C, chunk after chunk:
  // ScanFold-Scan.py:70-71 with F8 of SURVEY.md): loading a set that is already in a slot switches the pointers above, nothing
  // is rebuilt, copied or waited for.
  struct ModelSlot {
    SfDevParams *dP = nullptr;
    SfDevParamsPF *dX = nullptr;
    SfFastParams *dF = nullptr;
    uint64_t key = 0;                 // FNV-1a of the blobs it was built from: finds the candidate ...
    std::vector<unsigned char> src;   // ... and their bytes decide (1 blob, or 3 for a rescaled set)
    bool valid = false;
    int fast_ok = 0;
    int span = 0;          // the max_bp_span its max_pair_dist field was written for
    double temperature = 37.0;
    double pf_kT = 0.0, pf_MLbase = 1.0, pf_hp30 = 0.0;  // host copies of X.kT, X.MLbase, X.hp_init[30] (sf_pf_long)
    uint64_t used = 0;     // load counter value of its last use
  } slot[2];
  uint64_t loads = 0;
  int cur = 0;
  double temperature = 37.0;
  DevBuf full_scratch, pf_scratch, pf_share, fast_scratch, seqs, energies, db, cen, dbl, status, transcript, ovf, cons, sc, pf_flag;
  // the rolling-row offsets (SfFastRows, 8.7 kB) of every width that has been launched: one device table per width, written
  // once and never again, so launches of different widths on different caller streams (sf_mfe_device) cannot see each other's
  std::map<int, SfFastRows *> fast_rows;
  DevBuf tab_in, tab_partner, tab_counts, tab_out;  // sf_tabulate_pairs
  int64_t tab_groups = -1;
  std::string last_hip_error;
  // profiling of the dominant kernel
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // recorded only while profiling is on (sf_prof_reset)
  bool prof_on = false;
  double prof_ms = 0.0;
  int64_t prof_launches = 0, prof_folds = 0;
  int force_full = 0;
  int fast_ok = 0;
  int max_bp_span = 0;  // RNA.md().max_bp_span; <= 0: no limit
  int pf_kernel = 0;  // 0: LDS-resident kernel where it fits; 1: device-memory tables (SCANFOLD_PF_KERNEL=global)
  int pf_blocks_per_cu = 4;  // 256 VGPRs per thread: 2 waves per SIMD
  int pf_share_inside = 1;   // sf_scan, step 1: consecutive native windows share their inside tables (SCANFOLD_PF_SHARE=0: off)
} g;

#define HIPCHK(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      char b_[512];                                                               \
      snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      g.last_hip_error = b_;                                                      \
      return SF_ERR_HIP;                                                          \
    }                                                                             \
  } while (0)

int ensure(DevBuf &b, size_t need) {
  if (need <= b.cap) return SF_OK;
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  size_t cap = need + need / 8 + 256;
  HIPCHK(hipMalloc(&b.p, cap));
  b.cap = cap;
  return SF_OK;
}

int block_threads(int W) {
  int t = ((W + 63) / 64) * 64;
  return t < 64 ? 64 : t;
}

// Every entry point that touches the device: the library must be initialised, and HIP's current device is PER THREAD —
// hipSetDevice in sf_init binds only the thread that called it, so a caller's helper thread (scan.py runs the engine
// from one) would otherwise allocate and copy on device 0 while g.stream and the kernels belong to g.dev.
#define SF_ENTER()                          \
  do {                                      \
    if (!g.init) return SF_ERR_NOT_INIT;    \
    HIPCHK(hipSetDevice(g.dev));            \
  } while (0)

int check_ready() {
  SF_ENTER();
  if (!g.have_params) return SF_ERR_NO_PARAMS;
  return SF_OK;
}

double smooth_term(double x) {  // ViennaRNA's SMOOTH() with pf_smooth=1
  const double SCALE = 10.0;
  if (x / SCALE < -1.2283697) return 0.0;
  if (x / SCALE > 0.8660254) return x;
  const double s = sin(x / SCALE - 0.34242663) + 1.0;
  return SCALE * 0.38490018 * s * s;
}

uint32_t pack_key(const char *s, int len) {
  uint32_t k = 0;
  for (int i = 0; i < len; i++) k = (k << 3) | sf_encode_nt((uint8_t)s[i]);
  return k;
}

// P37 / PdH (both or neither): the 37 C free energies and the enthalpies `P` was rescaled from.  With them every Boltzmann
// weight comes from the un-truncated double dG(T) = dH - (dH - dG37) (T + K0) / (37 + K0), as ViennaRNA's
// get_boltzmann_factors computes it (md.pf_smooth, its default) [EXT]; the MFE tables stay the truncated integers of P.
void build_dev_params(const sf_params_blob &P, SfDevParams &D, SfDevParamsPF &X, const sf_params_blob *P37 = nullptr,
                      const sf_params_blob *PdH = nullptr) {
  memset(&D, 0, sizeof D);
  D.P = P;
  for (int s = 0; s <= SF_MAX_W + 1; s++)
    D.hp_init[s] = (s <= 30) ? P.hairpin[s] : P.hairpin[30] + (int)(P.lxc * log(s / 30.));
  for (int k = 0; k < SF_NSPECIAL; k++) {
    D.tetra_key[k] = k < P.n_tetra ? pack_key(P.tetra_seq[k], 6) : 0xFFFFFFFFu;
    D.tri_key[k] = k < P.n_tri ? pack_key(P.tri_seq[k], 5) : 0xFFFFFFFFu;
    D.hexa_key[k] = k < P.n_hexa ? pack_key(P.hexa_seq[k], 8) : 0xFFFFFFFFu;
  }
  D.pair[2][3] = 1; D.pair[3][2] = 2; D.pair[3][4] = 3; D.pair[4][3] = 4; D.pair[1][4] = 5; D.pair[4][1] = 6;

  memset(&X, 0, sizeof X);
  const double kT = (P.temperature + 273.15) * 1.98717;
  X.kT = kT;
  const double tempf = (P.temperature + 273.15) / (37.0 + 273.15);
  auto ex = [&](const int32_t &ref) -> double {  // the energy behind field `ref` of P
    if (!P37 || !PdH) return (double)ref;
    const size_t off = (size_t)((const char *)&ref - (const char *)&P);
    const int32_t g37 = *(const int32_t *)((const char *)P37 + off), dh = *(const int32_t *)((const char *)PdH + off);
    if (g37 >= SF_INF || g37 <= -SF_INF) return (double)ref;
    return (double)dh - ((double)dh - (double)g37) * tempf;
  };
  auto bw = [kT](double e) { return exp(-e * 10.0 / kT); };
  auto bws = [kT](double e) { return exp(smooth_term(-e) * 10.0 / kT); };
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 8; b++) X.stack[a][b] = bw(ex(P.stack[a][b]));
  for (int i = 0; i <= 30; i++) {
    X.bulge[i] = bw(ex(P.bulge[i]));
    X.internal_loop[i] = bw(ex(P.internal_loop[i]));
    X.ninio[i] = bw(std::min((double)P.max_ninio, i * ex(P.ninio)));
  }
  for (int s = 0; s <= SF_MAX_W + 1; s++)
    X.hp_init[s] = (s <= 30) ? bw(ex(P.hairpin[s])) : bw(ex(P.hairpin[30])) * exp(-(P.lxc * log(s / 30.)) * 10. / kT);
  for (int t = 0; t < 8; t++)
    for (int a = 0; a < 5; a++) {
      X.dangle5[t][a] = bws(ex(P.dangle5[t][a]));
      X.dangle3[t][a] = bws(ex(P.dangle3[t][a]));
      for (int b = 0; b < 5; b++) {
        X.mismatchI[t][a][b] = bw(ex(P.mismatchI[t][a][b]));
        X.mismatchH[t][a][b] = bw(ex(P.mismatchH[t][a][b]));
        X.mismatch1nI[t][a][b] = bw(ex(P.mismatch1nI[t][a][b]));
        X.mismatch23I[t][a][b] = bw(ex(P.mismatch23I[t][a][b]));
        X.mismatchM[t][a][b] = bws(ex(P.mismatchM[t][a][b]));
        X.mismatchExt[t][a][b] = bws(ex(P.mismatchExt[t][a][b]));
      }
    }
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 8; b++)
      for (int c = 0; c < 5; c++)
        for (int d = 0; d < 5; d++) {
          X.int11[a][b][c][d] = bw(ex(P.int11[a][b][c][d]));
          for (int e = 0; e < 5; e++) {
            X.int21[a][b][c][d][e] = bw(ex(P.int21[a][b][c][d][e]));
            for (int f = 0; f < 5; f++) X.int22[a][b][c][d][e][f] = bw(ex(P.int22[a][b][c][d][e][f]));
          }
        }
  X.MLbase = bw(ex(P.MLbase));
  X.MLclosing = bw(ex(P.MLclosing));
  for (int t = 0; t < 8; t++) X.MLintern[t] = bw(ex(P.MLintern[t]));
  X.TermAU = bw(ex(P.TerminalAU));
  for (int k = 0; k < SF_NSPECIAL; k++) {
    X.tetra[k] = bw(ex(P.tetra_E[k]));
    X.tri[k] = bw(ex(P.tri_E[k]));
    X.hexa[k] = bw(ex(P.hexa_E[k]));
  }
  for (int u = 2; u <= SF_MAXLOOP; u++) X.il1n[u] = X.internal_loop[u] * X.ninio[u - 2];
  X.mlbase_pow[0] = 1.0;
  for (int k = 1; k <= SF_MAX_W + 1; k++) X.mlbase_pow[k] = X.mlbase_pow[k - 1] * X.MLbase;
  // MFE model: dangle / multiloop / exterior mismatch terms are stored as min(0, x), as ViennaRNA's get_scaled_params
  // does ("must be <= 0") [EXT]; the Boltzmann weights above come from the unclamped values through SMOOTH().
  for (int t = 0; t < 8; t++)
    for (int a = 0; a < 5; a++) {
      if (D.P.dangle5[t][a] > 0) D.P.dangle5[t][a] = 0;
      if (D.P.dangle3[t][a] > 0) D.P.dangle3[t][a] = 0;
      for (int b = 0; b < 5; b++) {
        if (D.P.mismatchM[t][a][b] > 0) D.P.mismatchM[t][a][b] = 0;
        if (D.P.mismatchExt[t][a][b] > 0) D.P.mismatchExt[t][a][b] = 0;
      }
    }
}

// sf_pf_fast_kernel is compiled for two waves per SIMD (256 VGPRs): eight waves per CU = four workgroups of 128 threads
// (W <= 128) or two of 256.  A grid larger than that only runs its surplus workgroups as a second round — on a second set of
// 2-MB table slices (W = 200: 2.1 GB instead of 1.07 GB of scratch).
static int pf_fast_blocks_per_cu(int W) { return W > 128 ? g.pf_blocks_per_cu / 2 : g.pf_blocks_per_cu; }
int max_resident_blocks() { return g.n_cu * 4; }

// FULL kernel over n items; see sf_mfe_full_kernel for the indexing arguments
int launch_full(const uint8_t *d_seqs, const int *d_idx, const int *d_count, int n, int row_stride, int mfe_stride,
                int W, int32_t *d_mfe, char *d_db, int db_stride, hipStream_t st, const char *d_cons = nullptr,
                const int32_t *d_sc = nullptr) {
  if (n <= 0) return SF_OK;
  int grid = n < max_resident_blocks() ? n : max_resident_blocks();
  int rc = ensure(g.full_scratch, (size_t)grid * SF_FULL_SCRATCH_INTS(W) * sizeof(int32_t));
  if (rc) return rc;
  SF_LAUNCH(sf_mfe_full_kernel, grid, block_threads(W), 0, st, d_seqs, d_idx, d_count, n, row_stride, mfe_stride, W,
            (const SfDevParams *)g.dP, (int32_t *)g.full_scratch.p, d_mfe, d_db, db_stride, (int *)g.status.p, d_cons, d_sc);
  HIPCHK(hipGetLastError());
  return SF_OK;
}

// Partition functions past FP64's range (sf_pf.hip.h): every PF launch clears a flag per row, the kernel flags the folds
// whose ln Z passes SF_PF_LNZ_MAX, and sf_pf_kernel<true> redoes those — on the device, so that the _dev paths stay
// free of host round trips (as the int16 -> int32 MFE list does).  pf_begin sizes the scratch of both launches up front
// (the redo reuses g.pf_scratch behind the first launch on the same stream).
static int pf_begin(int n, int W, size_t scratch_bytes, hipStream_t st) {
  const size_t redo = (size_t)(n < SF_PF_REDO_GRID ? n : SF_PF_REDO_GRID) * SF_PF_SCRATCH_DOUBLES(W) * sizeof(double);
  int rc = ensure(g.pf_scratch, scratch_bytes > redo ? scratch_bytes : redo);
  if (!rc) rc = ensure(g.pf_flag, (size_t)n * sizeof(int));
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(g.pf_flag.p, 0, (size_t)n * sizeof(int), st));
  return SF_OK;
}
static int pf_redo_flagged(const uint8_t *d_seqs, int n, int row_stride, int W, double *d_dG, double *d_mbd, char *d_cen,
                           double *d_cd, const char *d_cons, hipStream_t st) {
  HIPCHK(hipGetLastError());
  const int grid = n < SF_PF_REDO_GRID ? n : SF_PF_REDO_GRID;
  SF_LAUNCH((sf_pf_kernel<true>), grid, block_threads(W), 0, st, d_seqs, n, row_stride, W, (const SfDevParams *)g.dP,
            (const SfDevParamsPF *)g.dX, (double *)g.pf_scratch.p, d_dG, d_mbd, d_cen, d_cd, d_cons, (int *)nullptr,
            (int *)g.pf_flag.p);
  HIPCHK(hipGetLastError());
  return SF_OK;
}

// Which kernel folds the ensembles of a batch of windows, and the shape of its launch: the one place that decides it (the
// table of DESIGN.md §4).  No HIP call in here.
enum PfKernel { PF_GENERAL, PF_LDS, PF_TABLES };  // sf_pf_kernel<false>, sf_pf_lds_kernel, sf_pf_fast_kernel
struct PfRoute {
  PfKernel kernel;
  int grid_cap, block;
  size_t scratch_doubles;  // of g.pf_scratch, per workgroup
};
static PfRoute pf_route(int W, bool constrained, bool type7, int force_full, int pf_kernel) {
  if (!force_full && !type7) {
    // every table of a fold in the LDS of one CU: one workgroup per CU
    if (pf_kernel == 0 && sf_pfl_supported(W) && (!constrained || sf_pfl_lds_bytes(W, true) <= SF_PFL_LDS_LIMIT))
      return {PF_LDS, g.n_cu, SF_PFL_NT, 0};
    if (W >= 16 && W <= (constrained ? SF_PFF_HC_MAXW : SF_PFF_MAXW))
      return {PF_TABLES, g.n_cu * pf_fast_blocks_per_cu(W), sf_pff_threads(W), SF_PFF_SCRATCH_DOUBLES(W)};
  }
  return {PF_GENERAL, max_resident_blocks(), block_threads(W), SF_PF_SCRATCH_DOUBLES(W)};
}

// The only caller of the windowed partition-function kernels.  d_cons: a constraint row per fold (sf_fold_constrained), type7:
// some row has a bracket pair of non-complementary bases.
// d_tr != null: the n rows are the native windows of transcript d_tr (length L) that start at win0, win0+1, ...
// (sf_scan with step 1): consecutive windows share their inside tables (sf_pf_lds.hip.h).  A flagged window keeps its
// place in the run: the tables it hands on hold the same (unscaled) values as its neighbours' own folds would, and only
// its own outputs are redone.
int launch_pf(const uint8_t *d_seqs, int n, int row_stride, int W, double *d_dG, double *d_mbd, char *d_cen,
              double *d_cd, hipStream_t st, const char *d_cons = nullptr, bool type7 = false, const uint8_t *d_tr = nullptr,
              int L = 0, int win0 = 0, int step = 1) {
  if (n <= 0) return SF_OK;
  const PfRoute r = pf_route(W, d_cons != nullptr, type7, g.force_full, g.pf_kernel);
  int grid = n < r.grid_cap ? n : r.grid_cap;
  int rc = pf_begin(n, W, (size_t)grid * r.scratch_doubles * sizeof(double), st);
  if (rc) return rc;
  const SfDevParams *dP = g.dP;
  const SfDevParamsPF *dX = g.dX;
  double *scratch = (double *)g.pf_scratch.p;
  int *d_status = d_cons ? (int *)g.status.p : nullptr, *d_flag = (int *)g.pf_flag.p;
  bool started = true;
  if (r.kernel == PF_LDS) {
    int run_len = 1;
    double *share = nullptr;
    if (!d_cons && d_tr && g.pf_share_inside && n >= 2 && step >= 1 && step <= W / 4) {
      // run length: the makespan of ceil(runs / CUs) runs per workgroup; a resumed window costs the outside pass
      // (~0.6 of a full fold) plus its share of the inside pass
      const double resumed = 0.6 + 0.4 * step / (double)(W - 4);
      double best = 1e300;
      for (int t = 1; t <= 128; t++) {
        const int runs = (n + t - 1) / t, per = (runs + g.n_cu - 1) / g.n_cu;
        const double cost = per * (1.0 + resumed * (t - 1));
        if (cost < best) { best = cost; run_len = t; }
      }
      if (run_len > 1) {
        grid = (n + run_len - 1) / run_len < g.n_cu ? (n + run_len - 1) / run_len : g.n_cu;
        rc = ensure(g.pf_share, (size_t)((grid + 7) & ~7) * SF_PFL_SHARE_DOUBLES(W) * sizeof(double));  // whole groups of eight slices: see sv in the kernel
        if (rc) return rc;
        share = (double *)g.pf_share.p;
      }
    }
    started = sf_pf_lds_launch(d_cons != nullptr, share != nullptr, grid, r.block, W, st, d_seqs, n, row_stride, W, dP, dX,
                               d_dG, d_mbd, d_cen, d_cd, d_tr, L, win0, step, run_len, share, d_cons, d_status, d_flag);
  } else if (r.kernel == PF_TABLES) {
    started = sf_pf_fast_launch(d_cons != nullptr, grid, r.block, W, st, d_seqs, n, row_stride, W, dP, dX, scratch, d_dG,
                                d_mbd, d_cen, d_cd, d_cons, d_status, d_flag);
  } else {
    SF_LAUNCH((sf_pf_kernel<false>), grid, r.block, 0, st, d_seqs, n, row_stride, W, dP, dX, scratch, d_dG, d_mbd, d_cen,
              d_cd, d_cons, d_status, d_flag);
  }
  if (!started) {
    g.last_hip_error = "launch_pf: no instantiation of the partition-function kernel for this batch";
    return SF_ERR_HIP;
  }
  return pf_redo_flagged(d_seqs, n, row_stride, W, d_dG, d_mbd, d_cen, d_cd, d_cons, st);
}

// energies of n rows: LDS-resident int16 kernel, then the exact int32 kernel on the rows it flagged.
// If d_db, every row that is a multiple of trace_stride also gets its structure, row/trace_stride-th string.
// HIP events around the dominant kernel, only while profiling is on; a failed call never leaks a pair
struct ProfPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool armed = false;
  int begin(hipStream_t st) {
    if (!g.prof_on) return SF_OK;
    if (g.ev.size() >= 1024) {  // bounded: fold what has accumulated into the running sum
      int rc = prof_drain();
      if (rc) return rc;
    }
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, st) != hipSuccess) {
      drop();
      g.last_hip_error = "hipEventCreate/Record failed in launch_mfe";
      return SF_ERR_HIP;
    }
    armed = true;
    return SF_OK;
  }
  int end(hipStream_t st) {
    if (!armed) return SF_OK;
    if (hipEventRecord(e1, st) != hipSuccess) {
      drop();
      g.last_hip_error = "hipEventRecord failed in launch_mfe";
      return SF_ERR_HIP;
    }
    g.ev.push_back({e0, e1});
    armed = false;
    e0 = e1 = nullptr;
    return SF_OK;
  }
  void drop() {
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    e0 = e1 = nullptr;
    armed = false;
  }
  ~ProfPair() { drop(); }
  static int prof_drain() {
    for (auto &e : g.ev) {
      float t = 0.f;
      hipError_t err = hipEventSynchronize(e.second);
      if (err == hipSuccess) err = hipEventElapsedTime(&t, e.first, e.second);
      hipEventDestroy(e.first);
      hipEventDestroy(e.second);
      if (err == hipSuccess) g.prof_ms += t;
    }
    g.ev.clear();
    return SF_OK;
  }
};

// SCANFOLD_MFE_POISON=1..5 (tests only): the LDS kernel's poison build — every byte a fold has not written itself holds an
// adversarial pattern (sf_mfe_fast.hip.h, PZ).  Read at every launch so that a test can switch it inside one process.
static int mfe_poison() {
  const char *e = getenv("SCANFOLD_MFE_POISON");
  const int v = e ? atoi(e) : 0;
  if (v < 1 || v > 5) return 0;
  static bool said = false;
  if (!said) {  // a test hook in the product library: never silent
    fprintf(stderr, "scanfold_hip: SCANFOLD_MFE_POISON=%d — TEST MODE: the MFE kernel refills its LDS slack with an adversarial "
                    "pattern before every fold (slower; results must not change). Unset it for production runs.\n", v);
    said = true;
  }
  return v;
}

// Which kernel folds a batch of windows: the LDS-resident int16 kernel (with the exact int32 kernel behind it, on the folds it
// flags) or the int32 kernel alone.  The one place that decides it; no HIP call in here.
enum MfeKernel { MFE_GENERAL, MFE_LDS };  // sf_mfe_full_kernel, sf_mfe_fast_kernel
static MfeKernel mfe_route(int W, bool constrained, bool type7, int trace_stride, int force_full, int fast_ok) {
  if (force_full || !fast_ok || type7 || !sf_fast_w_supported(W)) return MFE_GENERAL;
  if (constrained && (W > 250 || trace_stride != 1)) return MFE_GENERAL;  // (the HC instantiations: W <= 250, every fold traced)
  return MFE_LDS;
}

// d_cons / d_sc: every fold has its own hard constraint / Deigan pseudo-energies (row k of each; trace_stride 1): the
// constrained native windows of sf_fold_constrained; type7: some row has a bracket pair of non-complementary bases
int launch_mfe(const uint8_t *d_seqs, int n, int W, int32_t *d_out, hipStream_t st, int trace_stride = 1,
               char *d_db = nullptr, const char *d_cons = nullptr, const int32_t *d_sc = nullptr, bool type7 = false) {
  if (n <= 0) return SF_OK;
  ProfPair prof;
  int rc = SF_OK;
  const bool hc = d_cons || d_sc;
  if (mfe_route(W, hc, type7, trace_stride, g.force_full, g.fast_ok) == MFE_GENERAL) {
    if ((rc = prof.begin(st))) return rc;
    rc = launch_full(d_seqs, nullptr, nullptr, n, 1, 1, W, d_out, d_db, d_db ? trace_stride : 0, st, d_cons, d_sc);
    if (rc) return rc;
    if ((rc = prof.end(st))) return rc;
  } else {
    rc = ensure(g.ovf, sizeof(int) * ((size_t)n + 2));
    if (rc) return rc;
    // [overflow count][work counter][overflow list]: the counter (+ grid size) hands out the folds beyond each workgroup's first
    int *d_cnt = (int *)g.ovf.p, *d_work = d_cnt + 1, *d_list = d_cnt + 2;
    int grid = 0, threads = 0;
    size_t lds = 0, scratch_bytes = 0;
    sf_fast_geometry(W, g.n_cu, n, &grid, &threads, &lds, &scratch_bytes, hc);
    HIPCHK(hipMemsetAsync(d_cnt, 0, 2 * sizeof(int), st));
    rc = ensure(g.fast_scratch, scratch_bytes);
    if (rc) return rc;
    // the rolling rows' offsets for this width (SfFastRows): built on first use, immutable afterwards
    const SfFastRows *d_rows = nullptr;
    {
      auto it = g.fast_rows.find(W);
      if (it == g.fast_rows.end()) {
        static SfFastRows host_rows;
        SfFastRows *d = nullptr;
        sf_fast_build_rows(W, host_rows);
        HIPCHK(hipMalloc((void **)&d, sizeof(SfFastRows)));
        if (hipMemcpy(d, &host_rows, sizeof(SfFastRows), hipMemcpyHostToDevice) != hipSuccess) {  // synchronous: host_rows is reused
          hipFree(d);
          g.last_hip_error = "hipMemcpy of the rolling-row offset table failed";
          return SF_ERR_HIP;
        }
        it = g.fast_rows.emplace(W, d).first;
      }
      d_rows = it->second;
    }
    if ((rc = prof.begin(st))) return rc;
    // (constrained folds have no poison build; without a constraint d_cons and d_sc are null)
    if (!sf_fast_launch(hc, hc ? 0 : mfe_poison(), grid, threads, lds, st, d_seqs, n, W, (const SfDevParams *)g.dP,
                        (const SfFastParams *)g.dF, d_rows, (int16_t *)g.fast_scratch.p, d_out, d_cnt, d_list, trace_stride, d_db,
                        (int *)g.status.p, d_work, d_cons, d_sc)) {
      g.last_hip_error = "launch_mfe: no instantiation of sf_mfe_fast_kernel for this width";
      return SF_ERR_HIP;
    }
    HIPCHK(hipGetLastError());
    if ((rc = prof.end(st))) return rc;
    // folds that left the int16 range (or hold a forced pair of non-complementary bases) are redone exactly
    rc = launch_full(d_seqs, d_list, d_cnt, n, 1, 1, W, d_out, d_db, d_db ? trace_stride : 0, st, d_cons, d_sc);
  }
  if (g.prof_on) {
    g.prof_launches++;
    g.prof_folds += n;
  }
  return rc;
}

// The four partition-function results of n windows (d_dG, then mean bp distance and centroid distance behind it in g.dbl;
// centroids in g.cen) to the caller's arrays, those it asked for.
int pf_results_to_host(int n, int W, double *ens_dG, double *mbd, char *centroid, double *cdist) {
  const double *d_dG = (const double *)g.dbl.p, *d_mbd = d_dG + n, *d_cd = d_mbd + n;
  if (ens_dG) HIPCHK(hipMemcpyAsync(ens_dG, d_dG, n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (mbd) HIPCHK(hipMemcpyAsync(mbd, d_mbd, n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (cdist) HIPCHK(hipMemcpyAsync(cdist, d_cd, n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (centroid) HIPCHK(hipMemcpyAsync(centroid, g.cen.p, (size_t)n * (W + 1), hipMemcpyDeviceToHost, g.stream));
  return SF_OK;
}

// Read the sticky traceback status word after everything queued on `st` (nullptr: the whole device) has finished,
// and clear it.  Non-zero means a traceback found no decomposition: SF_ERR_INTERNAL.
int read_status(hipStream_t st, bool whole_device) {
  int v = 0;
  if (whole_device) HIPCHK(hipDeviceSynchronize());
  else HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(&v, g.status.p, sizeof(int), hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemset(g.status.p, 0, sizeof(int)));
  if (v & 2) return SF_ERR_CONSTRAINT;  // unbalanced brackets in a window's constraint string
  if (v & (SF_TAB_ST_UNBALANCED | SF_TAB_ST_TOO_MANY)) return SF_ERR_TABLE;
  return v ? SF_ERR_INTERNAL : SF_OK;
}

}  // namespace

extern "C" {

const char *sf_strerror(int status) {
  switch (status) {
    case SF_OK: return "ok";
    case SF_ERR_NOT_INIT: return "sf_init has not been called";
    case SF_ERR_NO_PARAMS: return "no energy parameters loaded (sf_params_load)";
    case SF_ERR_BAD_ARG: return "bad argument";
    case SF_ERR_BAD_PARAMS: return "parameter blob has the wrong size, magic or version";
    case SF_ERR_TEMPERATURE: return "temperature differs from the one the parameter blob is valid at";
    case SF_ERR_HIP: return "HIP runtime error (see sf_last_hip_error)";
    case SF_ERR_NO_DEVICE: return "no usable GPU device";
    case SF_ERR_INTERNAL: return "internal error: traceback found no decomposition";
    case SF_ERR_TABLE: return "scan table: unbalanced structure string, or window starts not ascending";
    case SF_ERR_CONSTRAINT: return "unbalanced brackets in a window's constraint string";
    case SF_ERR_RANGE: return "partition function left the FP64 range under every scale tried (sf_pf_long)";
    case SF_ERR_DUPLEX_HITS: return "LRI scan: more hits than max_hits (raise the capacity or lower the cutoff)";
    default: return "unknown status";
  }
}
const char *sf_last_hip_error(void) { return g.last_hip_error.c_str(); }

int sf_init(int device_ordinal) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SF_ERR_NO_DEVICE;
  if (device_ordinal < 0 || device_ordinal >= ndev) return SF_ERR_BAD_ARG;
  if (g.init) {
    if (g.dev == device_ordinal) return SF_OK;
    sf_shutdown();
  }
  HIPCHK(hipSetDevice(device_ordinal));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_ordinal));
  g.n_cu = prop.multiProcessorCount;
  char nm[256];
  snprintf(nm, sizeof nm, "%s (%s), %d CUs", prop.name[0] ? prop.name : "AMD GPU", prop.gcnArchName, g.n_cu);
  g.dev_name = nm;
  g.dev = device_ordinal;
  HIPCHK(hipStreamCreate(&g.stream));
  for (auto &m : g.slot) {
    HIPCHK(hipMalloc((void **)&m.dP, sizeof(SfDevParams)));
    HIPCHK(hipMalloc((void **)&m.dX, sizeof(SfDevParamsPF)));
    HIPCHK(hipMalloc((void **)&m.dF, sizeof(SfFastParams)));
    m.valid = false;
  }
  g.cur = 0;
  g.dP = g.slot[0].dP; g.dX = g.slot[0].dX; g.dF = g.slot[0].dF;
  {  // the sticky device status word every traceback ORs into (read and cleared by read_status)
    int rc = ensure(g.status, sizeof(int));
    if (rc) return rc;
    HIPCHK(hipMemset(g.status.p, 0, sizeof(int)));
  }
  HIPCHK(sf_fast_configure());
  HIPCHK(sf_pfl_configure());
  if (const char *pk = getenv("SCANFOLD_PF_KERNEL")) g.pf_kernel = (strcmp(pk, "global") == 0);
  if (const char *ps = getenv("SCANFOLD_PF_SHARE")) g.pf_share_inside = atoi(ps) != 0;
  g.force_full = 0;  // (sf_set_kernel_mode(1) selects the general kernels)
  g.init = true;
  g.have_params = false;
  return SF_OK;
}

int sf_shutdown(void) {
  if (!g.init) return SF_OK;
  hipDeviceSynchronize();
  DevBuf *bufs[] = {&g.pf_flag, &g.full_scratch, &g.pf_scratch, &g.pf_share, &g.fast_scratch, &g.seqs, &g.energies, &g.db, &g.cen,
                    &g.dbl, &g.status, &g.transcript, &g.ovf, &g.cons, &g.sc, &g.tab_in, &g.tab_partner, &g.tab_counts,
                    &g.tab_out};
  for (DevBuf *b : bufs) {
    if (b->p) hipFree(b->p);
    b->p = nullptr;
    b->cap = 0;
  }
  for (auto &e : g.ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  g.ev.clear();
  for (auto &m : g.slot) {
    if (m.dP) hipFree(m.dP);
    if (m.dX) hipFree(m.dX);
    if (m.dF) hipFree(m.dF);
    m.dP = nullptr; m.dX = nullptr; m.dF = nullptr; m.valid = false;
  }
  g.dP = nullptr; g.dX = nullptr; g.dF = nullptr;
  if (g.stream) hipStreamDestroy(g.stream);
  g.stream = nullptr;
  g.init = false;
  for (auto &kv : g.fast_rows) hipFree(kv.second);
  g.fast_rows.clear();
  g.have_params = false;
  return SF_OK;
}

int sf_device_name(char *buf, size_t n) {
  SF_ENTER();
  if (!buf || n == 0) return SF_ERR_BAD_ARG;
  snprintf(buf, n, "%s", g.dev_name.c_str());
  return SF_OK;
}

int sf_params_load(const void *blob, size_t nbytes, double temperature_c) {
  return sf_params_load_rescaled(blob, nbytes, temperature_c, nullptr, nullptr);
}

int sf_params_load_rescaled(const void *blob, size_t nbytes, double temperature_c, const void *blob_37c,
                            const void *blob_enthalpy) {
  SF_ENTER();
  if (!blob || nbytes != sizeof(sf_params_blob)) return SF_ERR_BAD_PARAMS;
  if ((blob_37c == nullptr) != (blob_enthalpy == nullptr)) return SF_ERR_BAD_ARG;
  static sf_params_blob P, P37, PdH;
  memcpy(&P, blob, sizeof P);
  if (P.magic != SF_PARAMS_MAGIC || P.version != SF_PARAMS_VERSION) return SF_ERR_BAD_PARAMS;
  if (blob_37c) {
    memcpy(&P37, blob_37c, sizeof P37);
    memcpy(&PdH, blob_enthalpy, sizeof PdH);
    if (P37.magic != SF_PARAMS_MAGIC || P37.version != SF_PARAMS_VERSION) return SF_ERR_BAD_PARAMS;
    if (PdH.magic != SF_PARAMS_MAGIC || PdH.version != SF_PARAMS_VERSION) return SF_ERR_BAD_PARAMS;
    if (fabs(P37.temperature - 37.0) > 1e-9) return SF_ERR_TEMPERATURE;  // the record the rescale starts from
  }
  if (fabs(P.temperature - temperature_c) > 1e-9) return SF_ERR_TEMPERATURE;
  // the set's identity: FNV-1a over the bytes handed in
  uint64_t key = 1469598103934665603ull;
  auto mix = [&key](const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t k = 0; k < n; k++) { key ^= b[k]; key *= 1099511628211ull; }
  };
  mix(&P, sizeof P);
  if (blob_37c) { mix(&P37, sizeof P37); mix(&PdH, sizeof PdH); }
  const int32_t md = g.max_bp_span > 0 ? g.max_bp_span - 1 : 0x7fffffff;
  g.loads++;
  int hit = -1;
  // (the hash only finds the candidate: a slot is this set iff the bytes it was built from are these bytes)
  const size_t nb = sizeof(sf_params_blob);
  for (int k = 0; k < 2; k++) {
    auto &m = g.slot[k];
    if (!m.valid || m.key != key || m.src.size() != (blob_37c ? 3 : 1) * nb) continue;
    if (memcmp(m.src.data(), &P, nb) != 0) continue;
    if (blob_37c && (memcmp(m.src.data() + nb, &P37, nb) != 0 || memcmp(m.src.data() + 2 * nb, &PdH, nb) != 0)) continue;
    hit = k;
  }
  if (hit < 0) {
    // the slot not in use (or the older one) is rebuilt; queued work may still read it
    const int k = !g.slot[0].valid ? 0 : (!g.slot[1].valid ? 1 : (g.have_params ? 1 - g.cur : (g.slot[0].used <= g.slot[1].used ? 0 : 1)));
    static SfDevParams D;
    static SfDevParamsPF X;
    static SfFastParams F;
    build_dev_params(P, D, X, blob_37c ? &P37 : nullptr, blob_37c ? &PdH : nullptr);
    D.max_pair_dist = md;
    sf_fast_build_params(D, F);
    HIPCHK(hipDeviceSynchronize());  // *_dev work queued on the callers' own streams may still read that slot's old tables
    g.slot[k].valid = false;
    HIPCHK(hipMemcpy(g.slot[k].dP, &D, sizeof D, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g.slot[k].dX, &X, sizeof X, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g.slot[k].dF, &F, sizeof F, hipMemcpyHostToDevice));
    g.slot[k].src.assign((const unsigned char *)&P, (const unsigned char *)&P + nb);
    if (blob_37c) {
      g.slot[k].src.insert(g.slot[k].src.end(), (const unsigned char *)&P37, (const unsigned char *)&P37 + nb);
      g.slot[k].src.insert(g.slot[k].src.end(), (const unsigned char *)&PdH, (const unsigned char *)&PdH + nb);
    }
    g.slot[k].key = key; g.slot[k].valid = true; g.slot[k].fast_ok = F.fast_ok; g.slot[k].span = g.max_bp_span;
    g.slot[k].temperature = temperature_c;
    g.slot[k].pf_kT = X.kT; g.slot[k].pf_MLbase = X.MLbase; g.slot[k].pf_hp30 = X.hp_init[30];
    hit = k;
  } else if (g.slot[hit].span != g.max_bp_span) {  // sf_set_max_bp_span was called while the other model was the resident one
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy((char *)g.slot[hit].dP + offsetof(SfDevParams, max_pair_dist), &md, sizeof md, hipMemcpyHostToDevice));
    g.slot[hit].span = g.max_bp_span;
  }
  g.slot[hit].used = g.loads;
  g.cur = hit;
  g.dP = g.slot[hit].dP; g.dX = g.slot[hit].dX; g.dF = g.slot[hit].dF;
  g.fast_ok = g.slot[hit].fast_ok;
  g.temperature = temperature_c;
  g.have_params = true;
  return SF_OK;
}

int sf_mfe_batch_dev(const uint8_t *d_seqs, int n, int W, int32_t *d_out, void *stream) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || W < 1 || W > SF_MAX_W || (n > 0 && (!d_seqs || !d_out))) return SF_ERR_BAD_ARG;
  return launch_mfe(d_seqs, n, W, d_out, stream ? (hipStream_t)stream : g.stream);
}

int sf_mfe_batch(const uint8_t *seqs, int n, int W, int32_t *out) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || W < 1 || W > SF_MAX_W || (n > 0 && (!seqs || !out))) return SF_ERR_BAD_ARG;
  if (n == 0) return SF_OK;
  if ((rc = ensure(g.seqs, (size_t)n * W))) return rc;
  if ((rc = ensure(g.energies, (size_t)n * sizeof(int32_t)))) return rc;
  HIPCHK(hipMemcpyAsync(g.seqs.p, seqs, (size_t)n * W, hipMemcpyHostToDevice, g.stream));
  if ((rc = launch_mfe((const uint8_t *)g.seqs.p, n, W, (int32_t *)g.energies.p, g.stream))) return rc;
  HIPCHK(hipMemcpyAsync(out, g.energies.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return SF_OK;
}

int sf_mfe_trace_batch(const uint8_t *seqs, int n, int W, int32_t *mfe_out, char *db_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || W < 1 || W > SF_MAX_W || (n > 0 && (!seqs || !db_out))) return SF_ERR_BAD_ARG;
  if (n == 0) return SF_OK;
  if ((rc = ensure(g.seqs, (size_t)n * W))) return rc;
  if ((rc = ensure(g.energies, (size_t)n * sizeof(int32_t)))) return rc;
  if ((rc = ensure(g.db, (size_t)n * (W + 1)))) return rc;
  HIPCHK(hipMemcpyAsync(g.seqs.p, seqs, (size_t)n * W, hipMemcpyHostToDevice, g.stream));
  if ((rc = launch_mfe((const uint8_t *)g.seqs.p, n, W, (int32_t *)g.energies.p, g.stream, 1, (char *)g.db.p)))
    return rc;
  if (mfe_out)
    HIPCHK(hipMemcpyAsync(mfe_out, g.energies.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(db_out, g.db.p, (size_t)n * (W + 1), hipMemcpyDeviceToHost, g.stream));
  return read_status(g.stream, false);
}

int sf_pf_batch(const uint8_t *seqs, int n, int W, double *ens_dG, double *mbd, char *centroid, double *cdist) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || W < 1 || W > SF_MAX_W || (n > 0 && !seqs)) return SF_ERR_BAD_ARG;
  if (n == 0) return SF_OK;
  if ((rc = ensure(g.seqs, (size_t)n * W))) return rc;
  if ((rc = ensure(g.dbl, (size_t)n * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(g.cen, (size_t)n * (W + 1)))) return rc;
  double *d_dG = (double *)g.dbl.p, *d_mbd = d_dG + n, *d_cd = d_mbd + n;
  HIPCHK(hipMemcpyAsync(g.seqs.p, seqs, (size_t)n * W, hipMemcpyHostToDevice, g.stream));
  if ((rc = launch_pf((const uint8_t *)g.seqs.p, n, 1, W, d_dG, d_mbd, (char *)g.cen.p, d_cd, g.stream))) return rc;
  if ((rc = pf_results_to_host(n, W, ens_dG, mbd, centroid, cdist))) return rc;
  HIPCHK(hipStreamSynchronize(g.stream));
  return SF_OK;
}

// Host-side look at the constraint rows before anything is launched.  Returns SF_ERR_CONSTRAINT for unbalanced brackets (ViennaRNA
// aborts there); *noncanonical = some bracket pair joins two bases that cannot pair (a "type 7" pair: only the general
// kernels carry its table rows).
static int scan_constraints(const uint8_t *seqs, const char *cons, int n, int W, bool *noncanonical) {
  static const uint8_t can[5][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 1}, {0, 0, 0, 1, 0}, {0, 0, 1, 0, 1}, {0, 1, 0, 1, 0}};  // N A C G U
  std::vector<int> stack((size_t)W + 1);
  *noncanonical = false;
  for (int k = 0; k < n; k++) {
    const char *c = cons + (size_t)k * W;
    const uint8_t *s = seqs + (size_t)k * W;
    int sp = 0;
    for (int i = 0; i < W; i++) {
      if (c[i] == '(') stack[sp++] = i;
      else if (c[i] == ')') {
        if (sp == 0) return SF_ERR_CONSTRAINT;
        const int o = stack[--sp];
        if (!can[sf_encode_nt(s[o])][sf_encode_nt(s[i])]) *noncanonical = true;
      }
    }
    if (sp) return SF_ERR_CONSTRAINT;
  }
  return SF_OK;
}

// fc.hc_add_from_db(window_constraints) / fc.sc_add_SHAPE_deigan(...) followed by fc.mfe(), fc.pf(), fc.centroid(),
// fc.mean_bp_distance() on n windows (ScanFold-Scan.py:405-418; ScanFold.py:508-544).  Only native windows come here — the
// reference folds its shuffles unconstrained.  The window's constraint is applied where a kernel makes a
// cell's pair type: in the LDS kernels of the hot path (sf_mfe_fast_kernel / sf_pf_lds_kernel, HC instantiations) where
// they apply, else — W beyond their range, a bracket pair of non-complementary bases, sf_set_kernel_mode(1) — in the general
// int32 / FP64 kernels.
int sf_fold_constrained(const uint8_t *seqs, int n, int W, const char *cons, const int32_t *sc_stack_dcal, unsigned flags,
                        int32_t *mfe_out, char *db_out, double *ens_dG, double *mbd, char *centroid, double *cdist) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || W < 1 || W > SF_MAX_W || (n > 0 && !seqs)) return SF_ERR_BAD_ARG;
  if (n == 0) return SF_OK;
  const bool want_mfe = !(flags & SF_FOLD_NO_MFE), want_pf = !(flags & SF_FOLD_NO_PF);
  bool noncanonical = false;
  if (cons && (rc = scan_constraints(seqs, cons, n, W, &noncanonical))) return rc;
  if ((rc = ensure(g.seqs, (size_t)n * W))) return rc;
  HIPCHK(hipMemcpyAsync(g.seqs.p, seqs, (size_t)n * W, hipMemcpyHostToDevice, g.stream));
  const char *d_cons = nullptr;
  const int32_t *d_sc = nullptr;
  if (cons) {
    if ((rc = ensure(g.cons, (size_t)n * W))) return rc;
    HIPCHK(hipMemcpyAsync(g.cons.p, cons, (size_t)n * W, hipMemcpyHostToDevice, g.stream));
    d_cons = (const char *)g.cons.p;
  }
  if (sc_stack_dcal) {
    if ((rc = ensure(g.sc, (size_t)n * W * sizeof(int32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(g.sc.p, sc_stack_dcal, (size_t)n * W * sizeof(int32_t), hipMemcpyHostToDevice, g.stream));
    d_sc = (const int32_t *)g.sc.p;
  }
  if (want_mfe) {
    if ((rc = ensure(g.energies, (size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = ensure(g.db, (size_t)n * (W + 1)))) return rc;
    // (every fold traced: the structure is the point)
    rc = launch_mfe((const uint8_t *)g.seqs.p, n, W, (int32_t *)g.energies.p, g.stream, 1, (char *)g.db.p, d_cons, d_sc, noncanonical);
    if (rc) return rc;
    if (mfe_out)
      HIPCHK(hipMemcpyAsync(mfe_out, g.energies.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
    if (db_out) HIPCHK(hipMemcpyAsync(db_out, g.db.p, (size_t)n * (W + 1), hipMemcpyDeviceToHost, g.stream));
  }
  if (want_pf) {
    if ((rc = ensure(g.dbl, (size_t)n * 3 * sizeof(double)))) return rc;
    if ((rc = ensure(g.cen, (size_t)n * (W + 1)))) return rc;
    double *d_dG = (double *)g.dbl.p, *d_mbd = d_dG + n, *d_cd = d_mbd + n;
    // (SHAPE data alone do not touch the partition function: without constraint rows these are plain folds)
    if ((rc = launch_pf((const uint8_t *)g.seqs.p, n, 1, W, d_dG, d_mbd, (char *)g.cen.p, d_cd, g.stream, d_cons, noncanonical)))
      return rc;
    if ((rc = pf_results_to_host(n, W, ens_dG, mbd, centroid, cdist))) return rc;
  }
  return read_status(g.stream, false);
}

static int check_scan_args(int L, int W, int step, int win_begin, int n_win, int r, int kind) {
  if (L < 1 || W < 1 || W > SF_MAX_W || step < 1 || win_begin < 0 || n_win < 0 || r < 0) return SF_ERR_BAD_ARG;
  if (kind != SF_SHUFFLE_MONO && kind != SF_SHUFFLE_DI) return SF_ERR_BAD_ARG;
  if (n_win > 0 && (long long)(win_begin + n_win - 1) * step + W > L) return SF_ERR_BAD_ARG;
  return SF_OK;
}

static int launch_shuffle(const uint8_t *d_tr, int L, int W, int step, int win_begin, int n_win, int r, int kind,
                          uint64_t seed, uint8_t *d_seqs, hipStream_t st) {
  const long long total = (long long)n_win * (r + 1);
  if (total <= 0) return SF_OK;
  const int grid = (int)((total + SF_SHUF_BLOCK - 1) / SF_SHUF_BLOCK);
  SF_LAUNCH(sf_shuffle_kernel, grid, SF_SHUF_BLOCK, sf_shuffle_lds_bytes(W), st, d_tr, L, W, step, win_begin, n_win, r, kind, seed, d_seqs);
  HIPCHK(hipGetLastError());
  return SF_OK;
}

int sf_shuffle_windows(const uint8_t *transcript, int L, int W, int step, int win_begin, int n_win, int r, int kind,
                       uint64_t seed, uint8_t *seqs_out) {
  SF_ENTER();
  int rc = check_scan_args(L, W, step, win_begin, n_win, r, kind);
  if (rc) return rc;
  if (!transcript || (n_win > 0 && !seqs_out)) return SF_ERR_BAD_ARG;
  if (n_win == 0) return SF_OK;
  const size_t nb = (size_t)n_win * (r + 1) * W;
  if ((rc = ensure(g.transcript, (size_t)L))) return rc;
  if ((rc = ensure(g.seqs, nb))) return rc;
  HIPCHK(hipMemcpyAsync(g.transcript.p, transcript, (size_t)L, hipMemcpyHostToDevice, g.stream));
  if ((rc = launch_shuffle((const uint8_t *)g.transcript.p, L, W, step, win_begin, n_win, r, kind, seed,
                           (uint8_t *)g.seqs.p, g.stream)))
    return rc;
  HIPCHK(hipMemcpyAsync(seqs_out, g.seqs.p, nb, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return SF_OK;
}

int sf_scan_dev(const uint8_t *d_tr, int L, int W, int step, int win_begin, int n_win, int r, int kind, uint64_t seed,
                unsigned flags, int32_t *d_energies, char *d_structure, char *d_centroid, double *d_ens_div,
                double *d_ens_dG, void *stream) {
  int rc = check_ready();
  if (rc) return rc;
  if ((rc = check_scan_args(L, W, step, win_begin, n_win, r, kind))) return rc;
  if (!d_tr || (n_win > 0 && !d_energies)) return SF_ERR_BAD_ARG;
  if (n_win == 0) return SF_OK;
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;
  // windows are processed in chunks so the materialised shuffles stay below ~1 GiB
  const size_t row_bytes = (size_t)(r + 1) * W;
  int chunk = (int)(((size_t)1 << 30) / row_bytes);
  if (chunk < 1) chunk = 1;
  if (chunk > n_win) chunk = n_win;
  if ((rc = ensure(g.seqs, (size_t)chunk * row_bytes))) return rc;
  uint8_t *d_seqs = (uint8_t *)g.seqs.p;
  for (int w0 = 0; w0 < n_win; w0 += chunk) {
    const int nw = (n_win - w0 < chunk) ? n_win - w0 : chunk;
    if ((rc = launch_shuffle(d_tr, L, W, step, win_begin + w0, nw, r, kind, seed, d_seqs, st))) return rc;
    char *dbp = (!(flags & SF_SCAN_NO_TRACE) && d_structure) ? d_structure + (size_t)w0 * (W + 1) : nullptr;
    // r+1 energies per window; the native row (every (r+1)-th) also gets its structure in the same launch
    if ((rc = launch_mfe(d_seqs, nw * (r + 1), W, d_energies + (size_t)w0 * (r + 1), st, r + 1, dbp))) return rc;
    if (!(flags & SF_SCAN_NO_PF)) {
      if ((rc = launch_pf(d_seqs, nw, r + 1, W, d_ens_dG ? d_ens_dG + w0 : nullptr, d_ens_div ? d_ens_div + w0 : nullptr,
                          d_centroid ? d_centroid + (size_t)w0 * (W + 1) : nullptr, nullptr, st, nullptr, false,
                          d_tr, L, win_begin + w0, step)))
        return rc;
    }
  }
  return SF_OK;
}

int sf_scan(const uint8_t *transcript, int L, int W, int step, int win_begin, int n_win, int r, int kind, uint64_t seed,
            unsigned flags, int32_t *energies, char *structure, char *centroid, double *ens_div, double *ens_dG) {
  int rc = check_ready();
  if (rc) return rc;
  if ((rc = check_scan_args(L, W, step, win_begin, n_win, r, kind))) return rc;
  if (!transcript || (n_win > 0 && !energies)) return SF_ERR_BAD_ARG;
  if (n_win == 0) return SF_OK;
  const size_t ne = (size_t)n_win * (r + 1);
  if ((rc = ensure(g.transcript, (size_t)L))) return rc;
  if ((rc = ensure(g.energies, ne * sizeof(int32_t)))) return rc;
  if ((rc = ensure(g.db, (size_t)n_win * (W + 1)))) return rc;
  if ((rc = ensure(g.cen, (size_t)n_win * (W + 1)))) return rc;
  if ((rc = ensure(g.dbl, (size_t)n_win * 2 * sizeof(double)))) return rc;
  double *d_div = (double *)g.dbl.p, *d_dG = d_div + n_win;
  HIPCHK(hipMemcpyAsync(g.transcript.p, transcript, (size_t)L, hipMemcpyHostToDevice, g.stream));
  rc = sf_scan_dev((const uint8_t *)g.transcript.p, L, W, step, win_begin, n_win, r, kind, seed, flags,
                   (int32_t *)g.energies.p, structure ? (char *)g.db.p : nullptr, centroid ? (char *)g.cen.p : nullptr,
                   ens_div ? d_div : nullptr, ens_dG ? d_dG : nullptr, g.stream);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(energies, g.energies.p, ne * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (structure && !(flags & SF_SCAN_NO_TRACE))
    HIPCHK(hipMemcpyAsync(structure, g.db.p, (size_t)n_win * (W + 1), hipMemcpyDeviceToHost, g.stream));
  if (!(flags & SF_SCAN_NO_PF)) {
    if (centroid) HIPCHK(hipMemcpyAsync(centroid, g.cen.p, (size_t)n_win * (W + 1), hipMemcpyDeviceToHost, g.stream));
    if (ens_div) HIPCHK(hipMemcpyAsync(ens_div, d_div, n_win * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    if (ens_dG) HIPCHK(hipMemcpyAsync(ens_dG, d_dG, n_win * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  }
  return read_status(g.stream, false);
}

// output arrays of sf_tabulate_pairs inside g.tab_out: four int32 arrays, then three double arrays, n entries each
struct TabOut {
  int32_t *gk, *gj, *gcount, *gfirst;
  double *sz, *sm, *se;
};
static TabOut tab_out_views(int64_t n) {
  TabOut o;
  char *p = (char *)g.tab_out.p;
  const size_t n8 = ((size_t)n + 1) & ~(size_t)1;  // keeps the doubles 8-byte aligned
  o.gk = (int32_t *)p;
  o.gj = o.gk + n8;
  o.gcount = o.gj + n8;
  o.gfirst = o.gcount + n8;
  o.sz = (double *)(o.gfirst + n8);
  o.sm = o.sz + n8;
  o.se = o.sm + n8;
  return o;
}

int sf_tabulate_pairs(const char *structures, int row_stride, int structures_on_device, int n_win, int W,
                      const int32_t *starts, const double *z, const double *mfe, const double *ed, int64_t *n_groups) {
  SF_ENTER();
  g.tab_groups = -1;
  if (n_win < 1 || W < 1 || W > SF_MAX_W || row_stride < W || !structures || !starts || !z || !mfe || !ed || !n_groups)
    return SF_ERR_BAD_ARG;
  for (int w = 1; w < n_win; w++)
    if (starts[w] <= starts[w - 1]) return SF_ERR_TABLE;
  const int64_t span = (int64_t)starts[n_win - 1] + W - starts[0];  // coordinates starts[0] .. last start + W - 1
  if (span > 0x7fffff00 || (int64_t)n_win * W > 0x7fffff00) return SF_ERR_BAD_ARG;
  const int lo = starts[0], n_coords = (int)span;
  hipStream_t st = g.stream;
  // inputs: [starts int32 n (padded to 8 bytes)] [z] [mfe] [ed] [structures, host case]
  const size_t off_z = (((size_t)n_win * 4) + 7) & ~(size_t)7;
  const size_t off_s = off_z + 3 * (size_t)n_win * 8;
  int rc = ensure(g.tab_in, off_s + (structures_on_device ? 0 : (size_t)n_win * row_stride));
  if (rc) return rc;
  char *in = (char *)g.tab_in.p;
  HIPCHK(hipMemcpyAsync(in, starts, (size_t)n_win * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(in + off_z, z, (size_t)n_win * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(in + off_z + (size_t)n_win * 8, mfe, (size_t)n_win * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(in + off_z + 2 * (size_t)n_win * 8, ed, (size_t)n_win * 8, hipMemcpyHostToDevice, st));
  const char *d_structs = structures;
  if (!structures_on_device) {
    HIPCHK(hipMemcpyAsync(in + off_s, structures, (size_t)n_win * row_stride, hipMemcpyHostToDevice, st));
    d_structs = in + off_s;
  } else {
    HIPCHK(hipDeviceSynchronize());  // the table may have been written on the caller's stream
  }
  const int32_t *d_starts = (const int32_t *)in;
  const double *d_z = (const double *)(in + off_z), *d_m = d_z + n_win, *d_e = d_m + n_win;
  rc = ensure(g.tab_partner, (size_t)n_win * W * sizeof(int16_t));
  if (rc) return rc;
  rc = ensure(g.tab_counts, ((size_t)n_coords + 1) * sizeof(int32_t));
  if (rc) return rc;
  int16_t *d_partner = (int16_t *)g.tab_partner.p;
  int32_t *d_counts = (int32_t *)g.tab_counts.p;
  int *d_status = (int *)g.status.p;
  SF_LAUNCH(sf_tab_partner_kernel, (n_win + 63) / 64, 64, (size_t)64 * (W / 2 + 1) * sizeof(int16_t), st, d_structs,
            row_stride, n_win, W, d_partner, d_status);
  SF_LAUNCH(sf_tab_groups_kernel<false>, n_coords, 64, 0, st, (const int16_t *)d_partner, d_starts, n_win, W, lo, d_counts,
            d_z, d_m, d_e, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
            (double *)nullptr, (double *)nullptr, (double *)nullptr, d_status);
  SF_LAUNCH(sf_tab_scan_kernel, 1, 256, 0, st, d_counts, n_coords);
  HIPCHK(hipGetLastError());
  int32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_counts + n_coords, sizeof total, hipMemcpyDeviceToHost, st));
  rc = read_status(st, false);
  if (rc) return rc;
  const size_t n8 = ((size_t)total + 1) & ~(size_t)1;
  rc = ensure(g.tab_out, n8 * (4 * sizeof(int32_t) + 3 * sizeof(double)) + 16);
  if (rc) return rc;
  TabOut o = tab_out_views(total);
  SF_LAUNCH(sf_tab_groups_kernel<true>, n_coords, 64, 0, st, (const int16_t *)d_partner, d_starts, n_win, W, lo, d_counts,
            d_z, d_m, d_e, o.gk, o.gj, o.gcount, o.gfirst, o.sz, o.sm, o.se, d_status);
  HIPCHK(hipGetLastError());
  rc = read_status(st, false);
  if (rc) return rc;
  g.tab_groups = total;
  *n_groups = total;
  return SF_OK;
}

int sf_tabulate_fetch(int32_t *group_k, int32_t *group_j, int32_t *group_windows, int32_t *group_first_window,
                      double *group_sum_z, double *group_sum_mfe, double *group_sum_ed) {
  SF_ENTER();
  if (g.tab_groups < 0) return SF_ERR_BAD_ARG;  // no finished sf_tabulate_pairs
  const int64_t n = g.tab_groups;
  if (n == 0) return SF_OK;
  TabOut o = tab_out_views(n);
  hipStream_t st = g.stream;
  if (group_k) HIPCHK(hipMemcpyAsync(group_k, o.gk, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (group_j) HIPCHK(hipMemcpyAsync(group_j, o.gj, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (group_windows) HIPCHK(hipMemcpyAsync(group_windows, o.gcount, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (group_first_window) HIPCHK(hipMemcpyAsync(group_first_window, o.gfirst, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (group_sum_z) HIPCHK(hipMemcpyAsync(group_sum_z, o.sz, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (group_sum_mfe) HIPCHK(hipMemcpyAsync(group_sum_mfe, o.sm, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (group_sum_ed) HIPCHK(hipMemcpyAsync(group_sum_ed, o.se, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return SF_OK;
}

int sf_last_status(void) {
  SF_ENTER();
  return read_status(nullptr, true);
}

int sf_set_max_bp_span(int span) {
  SF_ENTER();
  g.max_bp_span = span > 0 ? span : 0;
  if (g.have_params) {  // patch the field of the resident model
    const int32_t md = g.max_bp_span > 0 ? g.max_bp_span - 1 : 0x7fffffff;
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipMemcpy((char *)g.dP + offsetof(SfDevParams, max_pair_dist), &md, sizeof md, hipMemcpyHostToDevice));
    g.slot[g.cur].span = g.max_bp_span;  // (the other resident model is patched when it is switched to)
  }
  return SF_OK;
}

int sf_set_kernel_mode(int mode) {
  SF_ENTER();
  if (mode < 0 || mode > 1) return SF_ERR_BAD_ARG;
  g.force_full = (mode == 1);
  return SF_OK;
}


int sf_prof_reset(void) {
  SF_ENTER();
  HIPCHK(hipDeviceSynchronize());
  for (auto &e : g.ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  g.ev.clear();
  g.prof_ms = 0.0;
  g.prof_launches = 0;
  g.prof_folds = 0;
  g.prof_on = true;  // from now on launch_mfe brackets the dominant kernel with two events
  return SF_OK;
}

int sf_prof_get(double *ms, int64_t *launches, int64_t *folds) {
  SF_ENTER();
  HIPCHK(hipDeviceSynchronize());
  ProfPair::prof_drain();
  if (ms) *ms = g.prof_ms;
  if (launches) *launches = g.prof_launches;
  if (folds) *folds = g.prof_folds;
  return SF_OK;
}

int sf_prof_stop(void) {
  SF_ENTER();
  g.prof_on = false;
  return SF_OK;
}

}  // extern "C"

// ---------------- whole-record folds (include/scanfold_hip_long.h) ----------------
namespace {
double g_long_ms[3] = {0, 0, 0};  // fill, f5, traceback of the last sf_fold_long

// Every device buffer (and timing event) of one call of a whole-record fold, a duplex batch or the LRI scan; all freed when it
// goes out of scope (after the stream has drained).
struct CallBufs {
  std::vector<void *> ptrs;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  const char *who;  // the entry point named in an out-of-memory text
  explicit CallBufs(const char *who_) : who(who_) {}
  ~CallBufs() {
    hipStreamSynchronize(g.stream);
    for (void *p : ptrs) hipFree(p);
    for (hipEvent_t e : ev)
      if (e) hipEventDestroy(e);
  }
  // hipMalloc of `count` T that reports (and clears) an out-of-memory instead of leaving it for the next call's hipGetLastError
  template <class T>
  int alloc(T **p, size_t count, const char *what) {
    const size_t bytes = count * sizeof(T);
    void *v = nullptr;
    const hipError_t e = hipMalloc(&v, bytes ? bytes : 1);
    *p = (T *)v;
    if (e != hipSuccess) {
      hipGetLastError();
      char b[512];
      snprintf(b, sizeof b, "%s: hipMalloc of %zu bytes (%s) failed: %s", who, bytes, what, hipGetErrorString(e));
      g.last_hip_error = b;
      *p = nullptr;
      return SF_ERR_HIP;
    }
    ptrs.push_back(v);
    return SF_OK;
  }
  // alloc, and the copy of h[0 .. count) into it on g.stream
  template <class T>
  int upload(T **d, const T *h, size_t count, const char *what) {
    const int rc = alloc(d, count, what);
    if (rc) return rc;
    if (count) HIPCHK(hipMemcpyAsync(*d, h, count * sizeof(T), hipMemcpyHostToDevice, g.stream));
    return SF_OK;
  }
};

// lanes per cell of diagonal d: enough that no lane walks more than ~64 split terms, at most one wave
int long_group(int d) {
  int G = 1;
  while (G < 64 && G * 64 < d) G *= 2;
  return G;
}

// What sf_fold_long_batch and sf_pf_long_batch share: the rows of a call, their checks, the walk over chunks, and the head
// of a chunk's byte block.
const size_t kLongBatchBytesDefault = (size_t)8 << 30;  // device memory one chunk's tables may take
const int kLongBatchMaxSeqs = 1 << 15;                  // sequences per chunk: keeps every grid far inside an int
size_t g_longb_bytes = kLongBatchBytesDefault;

// The rows of one batched call.
struct LongRows {
  const uint8_t *seqs;
  int n, ld;
  const int32_t *len;
  const char *cons;               // NULL, or n rows of ld characters
  const char *who;                // the entry point the caller used
  std::vector<char> constrained;  // per row: it has a constraint (made by long_rows_check)
};

// The argument checks the batch entry points make (max_len: the longest row the caller takes), and a look at every constraint
// row before anything is launched: a row of dots is no constraint.
int long_rows_check(LongRows &R, int max_len) {
  if (R.n < 0 || (R.n > 0 && (!R.seqs || !R.len))) return SF_ERR_BAD_ARG;
  for (int k = 0; k < R.n; k++)
    if (R.len[k] < 1 || R.len[k] > max_len || R.len[k] > R.ld) return SF_ERR_BAD_ARG;
  R.constrained.assign((size_t)R.n, 0);
  if (R.cons)
    for (int k = 0; k < R.n; k++) {
      const char *c = R.cons + (size_t)k * R.ld;
      bool any = false, noncanonical = false;  // (a type-7 bracket pair needs nothing special here: the tables carry it)
      for (int x = 0; x < R.len[k] && !any; x++) any = c[x] != '.';
      if (!any) continue;
      const int rc = scan_constraints(R.seqs + (size_t)k * R.ld, c, 1, R.len[k], &noncanonical);
      if (rc) return rc;
      R.constrained[k] = 1;
    }
  return SF_OK;
}

// Walks the rows in chunks: as many consecutive rows as fit the byte budget at row_bytes(L) each, always at least one.
// chunk(s0, m, str) works on rows s0 .. s0 + m - 1 and leaves their strings (structures, centroids) back to back at str,
// L + 1 bytes each; str is NULL when str_out is.  The strings are staged here (they outlive the chunks' device buffers) and
// reach str_out, n rows of ld + 1 bytes, only when every chunk has succeeded.
// grid_lanes > 0 (rows past SF_MAX_LONG): a chunk's rows times the workgroups of grid_lanes lanes per nucleotide of its
// longest row stay inside an int, the size of a one-dimensional grid that gives every row that many workgroups.
template <class RowBytes, class Chunk>
int long_for_chunks(const LongRows &R, RowBytes row_bytes, char *str_out, int *chunks, Chunk chunk, int grid_lanes = 0) {
  std::vector<char> str;
  if (str_out) {
    size_t total = 0;
    for (int k = 0; k < R.n; k++) total += (size_t)R.len[k] + 1;
    str.resize(total);
  }
  size_t off = 0;
  *chunks = 0;
  for (int s0 = 0; s0 < R.n;) {
    size_t bytes = 0, str_bytes = 0;
    int m = 0, Lmax = 0;
    while (s0 + m < R.n && m < kLongBatchMaxSeqs) {
      const size_t b = row_bytes(R.len[s0 + m]);
      if (m > 0 && bytes + b > g_longb_bytes) break;
      Lmax = std::max(Lmax, R.len[s0 + m]);
      if (m > 0 && grid_lanes > 0 && (size_t)(m + 1) * (((size_t)Lmax * grid_lanes + 255) / 256) >= ((size_t)1 << 31)) break;
      bytes += b;
      str_bytes += (size_t)R.len[s0 + m] + 1;
      m++;
    }
    const int rc = chunk(s0, m, str_out ? str.data() + off : nullptr);
    if (rc) return rc;
    off += str_bytes;
    s0 += m;
    (*chunks)++;
  }
  off = 0;
  if (str_out)
    for (int k = 0; k < R.n; k++) {
      memcpy(str_out + (size_t)k * ((size_t)R.ld + 1), str.data() + off, (size_t)R.len[k] + 1);
      off += (size_t)R.len[k] + 1;
    }
  return SF_OK;
}

// The head of a chunk's byte block, the same in every family: every row's sequence (codes, zero on both sides: L + 2
// bytes); a family's own bytes follow from o_end.
struct LongPack {
  int Lmax = 0;
  size_t n_L = 0;           // nucleotides of all rows
  size_t o_end;
  std::vector<uint8_t> h8;  // the sequences, copied up in one piece
};

LongPack long_pack(const LongRows &R, int s0, int n) {
  LongPack K;
  for (int k = 0; k < n; k++) {
    K.Lmax = std::max(K.Lmax, (int)R.len[s0 + k]);
    K.n_L += (size_t)R.len[s0 + k];
  }
  K.o_end = K.n_L + 2 * (size_t)n;
  K.h8.assign(K.o_end, 0);
  size_t a_L = 0;
  for (int k = 0; k < n; k++) {
    const int L = R.len[s0 + k];
    const uint8_t *row = R.seqs + (size_t)(s0 + k) * R.ld;
    uint8_t *hS = K.h8.data() + a_L + 2 * (size_t)k;
    for (int x = 0; x < L; x++) hS[x + 1] = sf_encode_nt(row[x]);
    a_L += (size_t)L;
  }
  return K;
}

// The constraint of one whole record as the device reads it (sf_hc_parse of sf_energy.h, on the host): c[1 .. L] its
// characters, partner[i] the bracket partner of i, encl[i] the opening position of the innermost bracket pair around i,
// all 1-based and 0 for none; entries 0 and L + 1 of the three arrays are zero.  Pos: int16 in full tables (SfHc), int32 in
// banded ones (SfHc32), whose positions pass 32 767.  SF_ERR_CONSTRAINT for unbalanced brackets.
static_assert(SF_MAX_LONG <= INT16_MAX, "a position in full tables fits SfHc's int16");
template <class Pos>
int hc_parse_host(const char *cons, int L, char *c, Pos *partner, Pos *encl) {
  std::fill(c, c + L + 2, (char)0);
  std::fill(partner, partner + L + 2, (Pos)0);
  std::fill(encl, encl + L + 2, (Pos)0);
  std::vector<Pos> stack;
  for (int i = 1; i <= L; i++) {
    const char ch = cons[i - 1];
    c[i] = ch;
    if (ch == ')') {
      if (stack.empty()) return SF_ERR_CONSTRAINT;
      const Pos o = stack.back();
      stack.pop_back();
      partner[o] = (Pos)i;
      partner[i] = o;
    }
    encl[i] = stack.empty() ? (Pos)0 : stack.back();
    if (ch == '(') stack.push_back((Pos)i);
  }
  return stack.empty() ? SF_OK : SF_ERR_CONSTRAINT;
}

// The parsed constraints of a chunk's constrained rows as they are copied up: the bracket partners of all of them, then
// their enclosing pairs (pos), and their characters (c), L + 2 of each a row.  A caller declares it BEFORE the call's
// CallBufs: that destructor drains the async copies out of these vectors, so they must still stand when it runs.
template <class State>
struct HcStage {
  typedef typename std::remove_const<typename std::remove_pointer<decltype(std::declval<State>().hc.partner)>::type>::type Pos;
  std::vector<Pos> pos;
  std::vector<char> c;
};

// Binds the rows s0 .. s0 + hF.size() - 1 of R to the chunk's row states (SfLong, SfPfLong, SfBand or SfPfBand): clears each
// state and sets what all four have, L, S and hc.  Copies the packed sequences to d_u8, parses the constrained rows into H
// and copies them into one allocation of their own, (2 sizeof(Pos) + 1) (L + 2) bytes a constrained row.  A row of dots, or
// a row without a constraint, has none (hc.c == nullptr).
template <class State>
int bind_rows(CallBufs &B, const LongPack &K, const LongRows &R, int s0, uint8_t *d_u8, std::vector<State> &hF, HcStage<State> &H) {
  typedef typename HcStage<State>::Pos Pos;
  int rc;
  size_t n_hc = 0, a_L = 0, a = 0;
  for (size_t k = 0; k < hF.size(); k++)
    if (R.constrained[s0 + k]) n_hc += (size_t)R.len[s0 + k] + 2;
  H.pos.resize(2 * n_hc);
  H.c.resize(n_hc);
  char *p = nullptr;
  if (n_hc && (rc = B.alloc(&p, (2 * sizeof(Pos) + 1) * n_hc, "bracket partners, enclosing pairs, constraints"))) return rc;
  const Pos *d_part = (const Pos *)p, *d_encl = d_part + n_hc;
  const char *d_c = (const char *)(d_encl + n_hc);
  HIPCHK(hipMemcpyAsync(d_u8, K.h8.data(), K.h8.size(), hipMemcpyHostToDevice, g.stream));
  for (size_t k = 0; k < hF.size(); k++) {
    const int L = R.len[s0 + k];
    State &F = hF[k];
    memset(&F, 0, sizeof F);
    F.L = L;
    F.S = d_u8 + a_L + 2 * k;
    if (R.constrained[s0 + k]) {
      if ((rc = hc_parse_host(R.cons + (size_t)(s0 + k) * R.ld, L, H.c.data() + a, H.pos.data() + a, H.pos.data() + n_hc + a)))
        return rc;
      F.hc.partner = d_part + a;
      F.hc.encl = d_encl + a;
      F.hc.c = d_c + a;
      a += (size_t)L + 2;
    }
    a_L += (size_t)L;
  }
  if (n_hc) {
    HIPCHK(hipMemcpyAsync(p, H.pos.data(), 2 * sizeof(Pos) * n_hc, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(p + 2 * sizeof(Pos) * n_hc, H.c.data(), n_hc, hipMemcpyHostToDevice, g.stream));
  }
  return SF_OK;
}

// Hairpin initiation by loop size 0..n for the whole-record folds (the resident model's table only reaches SF_MAX_W + 1).
std::vector<int32_t> long_hairpin_table(const sf_params_blob *P, int n) {
  std::vector<int32_t> hp((size_t)n + 1);
  for (int s = 0; s <= n; s++) hp[s] = (s <= 30) ? P->hairpin[s] : P->hairpin[30] + (int)(P->lxc * log(s / 30.));
  return hp;
}

// The minimum free energy folds of rows s0 .. s0 + n - 1 of R: the host side of sf_fold_long and sf_fold_banded (their one
// row) and of one chunk of sf_fold_long_batch and sf_fold_banded_batch, after their argument checks; the counterpart of
// pf_long_rows below.  e_host / db_host: the caller's staging buffers (the energies at e_host[s0 ..], the structures back
// to back, L + 1 bytes each, at db_host, or NULL: no traceback and no memory for it); they hold the results once the stream
// has drained, which read_status waits for.  ms_out grows by the device-event times of fill, f5 and traceback.  A fixed
// number of device allocations whatever n is, all freed on return: c, fML, fMLt (ops.entries(L) a row), the DML rings, one
// int32 block (a hairpin table of ops.hairpin_entries(Lmax) + 1 entries, energies, f5, traceback stacks), one byte block
// (the packed rows, structures), what bind_rows allocates for the constraints, and the row states unless the kernels take
// the state by value (Ops::by_value).  The caller's ops supply what differs between the layouts (Ops::State, entries,
// hairpin_entries, band: a banded row's B) and the launches over the states at F, in host memory when they go by value and
// on the device otherwise: fill (every diagonal), f5 (energies to d_mfe) and trace.
template <class Ops>
int fold_rows(const LongRows &R, int s0, int n, Ops &ops, int32_t *e_host, char *db_host, double ms_out[3]) {
  typedef typename Ops::State State;
  int rc;
  const LongPack K = long_pack(R, s0, n);
  const int Lmax = K.Lmax;
  const size_t n_L = K.n_L;
  size_t cells = 0, n_stk = 0;
  for (int k = 0; k < n; k++) {
    cells += ops.entries(R.len[s0 + k]);
    n_stk += SF_LONG_STACK_INTS(R.len[s0 + k]);
  }
  const bool trace = db_host != nullptr;
  // slices of the int32 allocation, in elements; the structures follow the packed rows in the byte block
  const std::vector<int32_t> hhp = long_hairpin_table((const sf_params_blob *)g.slot[g.cur].src.data(), ops.hairpin_entries(Lmax));
  const size_t o_hp = 0, o_mfe = o_hp + hhp.size(), o_f5 = o_mfe + (size_t)n, o_stk = o_f5 + n_L + (size_t)n;
  const size_t n_i32 = o_stk + (trace ? n_stk : 0);
  const size_t o_db = K.o_end, n_u8 = o_db + (trace ? n_L + (size_t)n : 0);
  std::vector<State> hF((size_t)n);
  HcStage<State> H;  // (before B: see HcStage)

  CallBufs B(R.who);
  int32_t *d_tab[3], *d_dml, *d_i32;
  uint8_t *d_u8;
  State *d_F = nullptr;
  static const char *const names[3] = {"c", "fML", "fML transposed"};
  for (int k = 0; k < 3; k++)
    if ((rc = B.alloc(&d_tab[k], cells, names[k]))) return rc;
  if ((rc = B.alloc(&d_dml, 3 * (n_L + 2 * (size_t)n), "DML rings"))) return rc;
  if ((rc = B.alloc(&d_i32, n_i32, "hairpin table, energies, f5, traceback stacks"))) return rc;
  if ((rc = B.alloc(&d_u8, n_u8, "sequences, structures"))) return rc;
  if (!Ops::by_value && (rc = B.alloc(&d_F, (size_t)n, "fold states"))) return rc;
  const State *F = Ops::by_value ? hF.data() : d_F;
  if ((rc = bind_rows(B, K, R, s0, d_u8, hF, H))) return rc;

  size_t a_cells = 0, a_L = 0, a_stk = 0;
  for (int k = 0; k < n; k++) {
    const int L = R.len[s0 + k];
    State &Fk = hF[k];
    ops.band(Fk);
    Fk.hp = d_i32 + o_hp;
    Fk.c = d_tab[0] + a_cells;
    Fk.fML = d_tab[1] + a_cells;
    Fk.fMLt = d_tab[2] + a_cells;
    Fk.dml = d_dml + 3 * (a_L + 2 * (size_t)k);
    Fk.f5 = d_i32 + o_f5 + a_L + (size_t)k;
    Fk.status = (int *)g.status.p;
    if (trace) {
      Fk.stk = d_i32 + o_stk + a_stk;
      Fk.db = (char *)d_u8 + o_db + a_L + (size_t)k;
    }
    a_cells += ops.entries(L);
    a_L += (size_t)L;
    a_stk += SF_LONG_STACK_INTS(L);
  }
  HIPCHK(hipMemcpyAsync(d_i32 + o_hp, hhp.data(), hhp.size() * sizeof(int32_t), hipMemcpyHostToDevice, g.stream));
  if (!Ops::by_value) HIPCHK(hipMemcpyAsync((void *)F, hF.data(), (size_t)n * sizeof(State), hipMemcpyHostToDevice, g.stream));

  for (auto &e : B.ev) HIPCHK(hipEventCreate(&e));
  const SfDevParams *D = (const SfDevParams *)g.dP;
  const int32_t *len = R.len + s0;
  HIPCHK(hipEventRecord(B.ev[0], g.stream));
  ops.fill(F, len, n, Lmax, D);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(B.ev[1], g.stream));
  ops.f5(F, n, Lmax, D, d_i32 + o_mfe);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(B.ev[2], g.stream));
  if (trace) {
    ops.trace(F, n, D);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(B.ev[3], g.stream));
  HIPCHK(hipMemcpyAsync(e_host + s0, d_i32 + o_mfe, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (trace) HIPCHK(hipMemcpyAsync(db_host, d_u8 + o_db, n_L + (size_t)n, hipMemcpyDeviceToHost, g.stream));
  if ((rc = read_status(g.stream, false))) return rc;
  for (int k = 0; k < 3; k++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, B.ev[k], B.ev[k + 1]));
    ms_out[k] += (k == 2 && !trace) ? 0.0 : ms;
  }
  return SF_OK;
}

// A single call as the driver's one row, one chunk under any byte budget: R holds the row (ld = L, len = &L).  Energy and
// structure are staged and, like the time record rec, written only when the call has succeeded.
template <class Ops>
int fold_single(LongRows &R, int max_len, Ops &ops, int32_t *mfe_out, char *db_out, double rec[3]) {
  int rc;
  if ((rc = long_rows_check(R, max_len))) return rc;
  const size_t nL = (size_t)R.len[0];
  int32_t e = 0;  // (these outlive the driver's buffers, whose destructor drains the copies into them)
  std::vector<char> hdb(db_out ? nL + 1 : 0);
  double ms[3] = {0, 0, 0};
  if ((rc = fold_rows(R, 0, 1, ops, &e, db_out ? hdb.data() : nullptr, ms))) return rc;
  if (mfe_out) *mfe_out = e;
  if (db_out) memcpy(db_out, hdb.data(), nL + 1);
  for (int k = 0; k < 3; k++) rec[k] = ms[k];
  return SF_OK;
}

// What the triangular folds hand the driver: a row's tables hold SF_LONG_TRI(L) entries, the hairpin table reaches the
// longest row, and there is no band.
struct TriRows {
  typedef SfLong State;
  size_t entries(int L) const { return SF_LONG_TRI(L); }
  int hairpin_entries(int Lmax) const { return Lmax; }
  void band(SfLong &) const {}
};

// sf_fold_long's launches: the one row's state goes to its kernels by value, with the row's own lane groups and grids.
struct LongSingle : TriRows {
  static const bool by_value = true;
  void fill(const SfLong *F, const int32_t *, int, int L, const SfDevParams *D) {
    const int threads = 256;
    for (int d = 0; d < L; d++) {
      const int G = long_group(d);
      const size_t total = (size_t)(L - d) * (size_t)G;
      const int grid = (int)((total + threads - 1) / threads);
      SF_LAUNCH(sf_long_fill_kernel, grid, threads, 0, g.stream, *F, d, G, D);
    }
  }
  void f5(const SfLong *F, int, int, const SfDevParams *D, int32_t *d_mfe) {
    SF_LAUNCH(sf_long_f5_kernel, 1, 256, 0, g.stream, *F, D, d_mfe);
  }
  void trace(const SfLong *F, int, const SfDevParams *D) { SF_LAUNCH(sf_long_trace_kernel, 1, 256, 0, g.stream, *F, D); }
};
}  // namespace

extern "C" {

int sf_fold_long(const uint8_t *seq, int L, const char *cons, int32_t *mfe_out, char *db_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (!seq || L < 1 || L > SF_MAX_LONG) return SF_ERR_BAD_ARG;
  LongRows R = {seq, 1, L, &L, cons, "sf_fold_long"};
  LongSingle ops;
  return fold_single(R, SF_MAX_LONG, ops, mfe_out, db_out, g_long_ms);
}

int sf_fold_long_times(double *fill_ms, double *f5_ms, double *trace_ms) {
  SF_ENTER();
  if (fill_ms) *fill_ms = g_long_ms[0];
  if (f5_ms) *f5_ms = g_long_ms[1];
  if (trace_ms) *trace_ms = g_long_ms[2];
  return SF_OK;
}

}  // extern "C"

// ---------------- whole-record folds under a span in banded tables (sf_mfe_banded.hip.h) ----------------
namespace {
double g_band_ms[3] = {0, 0, 0};  // fill, f5, traceback of the last sf_fold_banded
int g_band_B = 0, g_band_launches = 0;

// Lanes per cell of diagonal d of a banded fill: as many as it takes to fill the device with the diagonal's cells (a
// quarter of the lanes it holds at once: the diagonals follow each other closely), but no more than the cell has work for
// (d split terms and up to 496 interior-loop candidates, eight terms a lane at least); a power of two, at most one wave.
int band_group(int d, size_t cells) {
  const int umax = std::min(SFD_MAXLOOP, d - 2 - (SFD_TURN + 1));
  const int work = std::max(0, d - 2 * SFD_TURN - 2) + (umax >= 0 ? (umax + 1) * (umax + 2) / 2 : 0);
  const size_t lanes = (size_t)g.n_cu * 512;
  int G = 1;
  while (G < 64 && (size_t)G * cells < lanes && G * 8 < work) G *= 2;
  return G;
}

// What the banded folds hand fold_rows: a row's tables hold L B entries, B = min(S, L), and the hairpin table reaches the
// widest band.
struct BandRows {
  typedef SfBand State;
  const int S = g.max_bp_span;
  size_t entries(int L) const { return (size_t)L * (size_t)std::min(S, L); }
  int hairpin_entries(int Lmax) const { return std::min(S, Lmax); }
  void band(SfBand &F) const { F.B = std::min(S, F.L); }
};

// sf_fold_banded's launches: the one row's state by value, one fill launch per diagonal of its band.
struct BandSingle : BandRows {
  static const bool by_value = true;
  void fill(const SfBand *F, const int32_t *, int, int L, const SfDevParams *D) {
    const int threads = 256;
    for (int d = 0; d < F->B; d++) {
      const size_t cells = (size_t)(L - d);
      const int G = band_group(d, cells);
      const int grid = (int)((cells * (size_t)G + threads - 1) / threads);
      SF_LAUNCH(sf_band_fill_kernel, grid, threads, 0, g.stream, *F, d, G, D);
    }
  }
  void f5(const SfBand *F, int, int, const SfDevParams *D, int32_t *d_mfe) {
    SF_LAUNCH(sf_band_f5_kernel, 1, F->B <= 256 ? 64 : 256, 0, g.stream, *F, D, d_mfe);
  }
  void trace(const SfBand *F, int, const SfDevParams *D) { SF_LAUNCH(sf_band_trace_kernel, 1, 256, 0, g.stream, *F, D); }
};
}  // namespace

extern "C" {

int sf_fold_banded_bytes(int L, int span, size_t *bytes) {
  SF_ENTER();
  if (L < 1 || L > SF_MAX_BANDED || span < 1 || !bytes) return SF_ERR_BAD_ARG;
  *bytes = SF_BANDED_BYTES(L, std::min(span, L));
  return SF_OK;
}

int sf_fold_banded(const uint8_t *seq, int L, const char *cons, int32_t *mfe_out, char *db_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (!seq || L < 1 || L > SF_MAX_BANDED || g.max_bp_span < 1) return SF_ERR_BAD_ARG;
  LongRows R = {seq, 1, L, &L, cons, "sf_fold_banded"};
  BandSingle ops;
  if ((rc = fold_single(R, SF_MAX_BANDED, ops, mfe_out, db_out, g_band_ms))) return rc;
  g_band_B = g_band_launches = std::min(ops.S, L);  // one fill launch per diagonal
  return SF_OK;
}

int sf_fold_banded_times(double *fill_ms, double *f5_ms, double *trace_ms, int *band, int *fill_launches) {
  SF_ENTER();
  if (fill_ms) *fill_ms = g_band_ms[0];
  if (f5_ms) *f5_ms = g_band_ms[1];
  if (trace_ms) *trace_ms = g_band_ms[2];
  if (band) *band = g_band_B;
  if (fill_launches) *fill_launches = g_band_launches;
  return SF_OK;
}

}  // extern "C"

// ---------------- many whole-record folds at once (sf_mfe_long_batch.hip.h) ----------------
namespace {
double g_longb_ms[3] = {0, 0, 0};  // fill, f5, traceback of the last sf_fold_long_batch, summed over its chunks
int g_longb_chunks = 0;

size_t long_batch_seq_bytes(int L) { return 12 * SF_LONG_TRI(L) + 80 * (size_t)L; }

// A chunk's launches: the row states in a device array, every launch over all rows, the lanes per cell cut down until a
// diagonal's launch fits the lane budget.
struct LongBatch : TriRows {
  static const bool by_value = false;
  const int threads = SF_LONGB_THREADS;
  void fill(const SfLong *d_F, const int32_t *, int n, int Lmax, const SfDevParams *D) {
    const size_t budget = (size_t)(g.n_cu > 0 ? g.n_cu : 1) * SF_LONGB_LANES_PER_CU;
    for (int d = 0; d < Lmax; d++) {
      int G = long_group(d);
      while (G > 1 && (size_t)n * (size_t)(Lmax - d) * (size_t)G > budget) G >>= 1;
      const int bps = (int)(((size_t)(Lmax - d) * (size_t)G + threads - 1) / threads);
      SF_LAUNCH(sf_longb_fill_kernel, n * bps, threads, 0, g.stream, d_F, d, G, bps, D);
    }
  }
  void f5(const SfLong *d_F, int n, int, const SfDevParams *D, int32_t *d_mfe) {
    SF_LAUNCH(sf_longb_f5_kernel, n, threads, 0, g.stream, d_F, D, d_mfe);
  }
  void trace(const SfLong *d_F, int n, const SfDevParams *D) { SF_LAUNCH(sf_longb_trace_kernel, n, threads, 0, g.stream, d_F, D); }
};
}  // namespace

extern "C" {

int sf_fold_long_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, int32_t *mfe_out, char *db_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (n > 0 && !mfe_out) return SF_ERR_BAD_ARG;
  LongRows R = {seqs, n, ld, len, cons, "sf_fold_long_batch"};
  if ((rc = long_rows_check(R, SF_MAX_LONG))) return rc;
  // the energies are staged and handed over, like the structures, only when every chunk has succeeded
  std::vector<int32_t> e_host((size_t)n);
  double ms[3] = {0, 0, 0};
  int chunks;
  LongBatch ops;
  rc = long_for_chunks(R, long_batch_seq_bytes, db_out, &chunks, [&](int s0, int m, char *db_host) {
    return fold_rows(R, s0, m, ops, e_host.data(), db_host, ms);
  });
  if (rc) return rc;  // (n == 0: no chunk)
  if (n) memcpy(mfe_out, e_host.data(), (size_t)n * sizeof(int32_t));
  for (int k = 0; k < 3; k++) g_longb_ms[k] = ms[k];
  g_longb_chunks = chunks;
  return SF_OK;
}

int sf_fold_long_batch_times(double *fill_ms, double *f5_ms, double *trace_ms, int *chunks) {
  SF_ENTER();
  if (fill_ms) *fill_ms = g_longb_ms[0];
  if (f5_ms) *f5_ms = g_longb_ms[1];
  if (trace_ms) *trace_ms = g_longb_ms[2];
  if (chunks) *chunks = g_longb_chunks;
  return SF_OK;
}

int sf_set_long_batch_bytes(size_t bytes) {
  g_longb_bytes = bytes ? bytes : kLongBatchBytesDefault;
  return SF_OK;
}

}  // extern "C"

// ---------------- many whole-record folds under a span at once (sf_mfe_banded_batch.hip.h) ----------------
namespace {
double g_bandb_ms[3] = {0, 0, 0};  // fill, f5, traceback of the last sf_fold_banded_batch, summed over its chunks
int g_bandb_chunks = 0, g_bandb_launches = 0;

// A chunk's launches under the span S, each row in a band of B_s = min(S, L_s) diagonals: the row states in a device array,
// one fill launch per diagonal d < max B_s over all rows, its lanes per cell sized by the cells of the rows still live on it.
// `launches` grows by a chunk's fill launches.
struct BandBatch : BandRows {
  static const bool by_value = false;
  const int threads = SF_BANDB_THREADS;
  int launches = 0;
  void fill(const SfBand *d_F, const int32_t *len, int n, int Lmax, const SfDevParams *D) {
    const int Bmax = std::min(S, Lmax);
    std::vector<int> lens(len, len + n);
    std::sort(lens.begin(), lens.end());  // the rows live on diagonal d (d < B_s, that is d < L_s: d < S here) are a suffix
    size_t live = 0, live_L = 0;          // rows with L_s > d, and their nucleotides
    for (int L : lens) live_L += (size_t)L;
    for (int d = 0; d < Bmax; d++) {
      while (live < (size_t)n && lens[live] <= d) live_L -= (size_t)lens[live++];
      const int G = band_group(d, live_L - ((size_t)n - live) * (size_t)d);  // the cells of all rows on this diagonal
      const int bps = (int)(((size_t)(Lmax - d) * (size_t)G + threads - 1) / threads);
      SF_LAUNCH(sf_bandb_fill_kernel, n * bps, threads, 0, g.stream, d_F, d, G, bps, D);
    }
    launches += Bmax;
  }
  void f5(const SfBand *d_F, int n, int Lmax, const SfDevParams *D, int32_t *d_mfe) {
    SF_LAUNCH(sf_bandb_f5_kernel, n, std::min(S, Lmax) <= 256 ? 64 : 256, 0, g.stream, d_F, D, d_mfe);
  }
  void trace(const SfBand *d_F, int n, const SfDevParams *D) { SF_LAUNCH(sf_bandb_trace_kernel, n, threads, 0, g.stream, d_F, D); }
};
}  // namespace

extern "C" {

int sf_fold_banded_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, int32_t *mfe_out, char *db_out) {
  int rc = check_ready();
  if (rc) return rc;
  const int S = g.max_bp_span;
  if (S < 1 || (n > 0 && !mfe_out)) return SF_ERR_BAD_ARG;
  LongRows R = {seqs, n, ld, len, cons, "sf_fold_banded_batch"};
  if ((rc = long_rows_check(R, SF_MAX_BANDED))) return rc;
  // the energies are staged and handed over, like the structures, only when every chunk has succeeded
  std::vector<int32_t> e_host((size_t)n);
  double ms[3] = {0, 0, 0};
  int chunks;
  BandBatch ops;
  auto row_bytes = [S](int L) { return (size_t)SF_BANDED_BYTES(L, std::min(S, L)); };
  rc = long_for_chunks(R, row_bytes, db_out, &chunks, [&](int s0, int m, char *db_host) {
    return fold_rows(R, s0, m, ops, e_host.data(), db_host, ms);
  }, 64);
  if (rc) return rc;  // (n == 0: no chunk)
  if (n) memcpy(mfe_out, e_host.data(), (size_t)n * sizeof(int32_t));
  for (int k = 0; k < 3; k++) g_bandb_ms[k] = ms[k];
  g_bandb_chunks = chunks;
  g_bandb_launches = ops.launches;
  return SF_OK;
}

int sf_fold_banded_batch_times(double *fill_ms, double *f5_ms, double *trace_ms, int *chunks, int *fill_launches) {
  SF_ENTER();
  if (fill_ms) *fill_ms = g_bandb_ms[0];
  if (f5_ms) *f5_ms = g_bandb_ms[1];
  if (trace_ms) *trace_ms = g_bandb_ms[2];
  if (chunks) *chunks = g_bandb_chunks;
  if (fill_launches) *fill_launches = g_bandb_launches;
  return SF_OK;
}

}  // extern "C"

// ---------------- whole-record partition function (sf_pf_long.hip.h): one host driver, the launches its callers' ----------------
namespace {
double g_pfl_ms[2] = {0, 0};  // inside (all attempts, with q5 / q3), outside (with the probabilities) of the last sf_pf_long
int g_pfl_attempts = 0;
double g_pfl_lns = 0.0;

// sc[k] = s^-k and mlbs[k] = (MLbase / s)^k, k = 0 .. L + 1, for the per-nucleotide scale s = e^lns.  Made on the host: a
// device exp may differ from it in the last bit.
void pfl_scale_powers(double lns, double ln_mlbase, int L, double *sc, double *mlbs) {
  for (int k = 0; k <= L + 1; k++) {
    sc[k] = exp(-lns * k);
    mlbs[k] = exp((ln_mlbase - lns) * k);
  }
}
// the scale of a row's first attempt
double pfl_first_lns(const int32_t *mfe_dcal_hint, double kT, int L) {
  return mfe_dcal_hint ? SF_PFLONG_MFE_FACTOR * (-(double)*mfe_dcal_hint * 10.0 / kT) / L : SF_PFLONG_LNS_DEFAULT;
}
// the scale of the next attempt after an inside pass that left the range (ln Z_s = lz)
double pfl_next_lns(double lns, double lz, int L) {
  // (q5[L] = +inf: log = +inf; an underflow to 0: -inf; NaN counts as an overflow)
  return lns + (isfinite(lz) ? lz / L : ((lz < 0 ? -700.0 : 700.0) / L));
}
// Hairpin initiation weights by loop size 0..n (read only past the resident table, SF_MAX_W + 1: build_dev_params'
// extrapolation), from the slot's host copies of kT and the weight at 30 and the set as it was handed in.
std::vector<double> pfl_hairpin_table(const Ctx::ModelSlot &M, int n) {
  const sf_params_blob *P = (const sf_params_blob *)M.src.data();
  std::vector<double> hp((size_t)n + 1);
  for (int s = 0; s <= n; s++) hp[s] = (s <= 30) ? 0.0 : M.pf_hp30 * exp(-(P->lxc * log(s / 30.)) * 10. / M.pf_kT);
  return hp;
}
// the lane budget of ONE sf_pf_long call: it sizes every row's lane groups and probability waves, whatever a batch holds
size_t pfl_lanes() { return (size_t)(g.n_cu > 0 ? g.n_cu : 1) * SF_PFLONG_LANES_PER_CU; }

// the seven tables of a state (SfPfLong, SfPfBand) out of seven allocations, `off` elements into each; their names in the
// text of a failed allocation
const char *const kPfTableNames[7] = {"qb", "qb by columns / A0", "qm", "qm by columns", "qm1 / w", "ob", "A1"};
template <class T>
void pfl_bind_tables(T &F, double *const tab[7], size_t off) {
  F.qb = tab[0] + off; F.qbt = tab[1] + off; F.qm = tab[2] + off; F.qmt = tab[3] + off;
  F.qm1t = tab[4] + off; F.ob = tab[5] + off; F.a1 = tab[6] + off;
  F.a0 = F.qbt;   // (dead after q5)
  F.wt = F.qm1t;  // (dead after the inside pass)
}
// one diagonal of the inside or outside pass of a single sequence: its own lane groups and grid
template <class T>
void pfl_launch_diagonal(void (*kernel)(T, int, int, const SfDevParams *, const SfDevParamsPF *), const T &F, int d, size_t lanes) {
  const int threads = 256;
  const size_t cells = (size_t)(F.L - d);
  const int G = pfl_group(cells, d, lanes);
  const size_t total = std::min(cells * (size_t)G, lanes);
  SF_LAUNCH(kernel, (int)((total + threads - 1) / threads), threads, 0, g.stream, F, d, G, (const SfDevParams *)g.dP,
            (const SfDevParamsPF *)g.dX);
}

// The partition functions of rows s0 .. s0 + n - 1 of R: the host side of sf_pf_long (its one row) and of one chunk of
// sf_pf_long_batch, after their argument checks.  hint: NULL, or one value per row of the call (SF_PF_LONG_NO_HINT: none).
// rows_host / cen_host: the caller's staging buffers (the records at rows_host[s0 ..], the centroids back to back, L + 1
// bytes each, at cen_host, or NULL); a call that ends in SF_ERR_RANGE still leaves every row's lns and attempts there.
// ms_out: inside, outside; *passes: inside passes run.  A fixed number of device allocations whatever n is; all freed on
// return.  The launches are the caller's: launch.bind(B, hF) takes the row states, launch.mark(act) the rows the next
// launches work on (bytes, one per row), and launch.inside(Ltop, d), exterior(), outside(Ltop, d), prob() and finish() run
// one pass over the marked rows, the longest of which has Ltop nt.
template <class Launch>
int pf_long_rows(const LongRows &R, const int32_t *hint, int s0, int n, Launch &launch, sf_pf_long_row *rows_host,
                 char *cen_host, double ms_out[2], int *passes) {
  int rc;
  const Ctx::ModelSlot &M = g.slot[g.cur];  // its host copies of kT, MLbase and the hairpin initiation weight at 30
  const double kT = M.pf_kT, ln_mlbase = log(M.pf_MLbase);
  const size_t lanes = pfl_lanes();
  const LongPack K = long_pack(R, s0, n);
  const int Lmax = K.Lmax;
  const size_t n_L = K.n_L;
  size_t tri = 0, n_part = 0;
  for (int k = 0; k < n; k++) {
    tri += SF_LONG_TRI(R.len[s0 + k]);
    n_part += 2 * (size_t)pfl_prob_waves(R.len[s0 + k], lanes);
  }
  // slices of the FP64 allocation, in elements: the results first (one copy reads every row's), then the powers of every
  // row's scale (one copy writes them), the shared hairpin table, q5, q3 and the partial sums.  The centroids follow the
  // packed rows in the byte block.
  const size_t o_out = 0, o_pow = o_out + 3 * (size_t)n, n_pow = 2 * (n_L + 2 * (size_t)n), o_hp = o_pow + n_pow;
  const size_t o_q5 = o_hp + (size_t)Lmax + 1, o_q3 = o_q5 + n_L + 2 * (size_t)n, o_part = o_q3 + n_L + 3 * (size_t)n;
  const size_t n_f64 = o_part + n_part;
  const size_t o_cen = K.o_end, n_u8 = o_cen + n_L + (size_t)n;

  const std::vector<double> hhp = pfl_hairpin_table(M, Lmax);
  std::vector<double> hpow(n_pow), hout(3 * (size_t)n);
  std::vector<SfPfLong> hF((size_t)n);
  HcStage<SfPfLong> H;  // (before B: see HcStage)
  std::vector<char> hcen(n_L + (size_t)n);

  CallBufs B(R.who);
  double *d_tri[SF_PFLONG_NTRI], *d_f64;
  uint8_t *d_u8;
  for (int k = 0; k < SF_PFLONG_NTRI; k++)
    if ((rc = B.alloc(&d_tri[k], tri, kPfTableNames[k]))) return rc;
  if ((rc = B.alloc(&d_f64, n_f64, "results, scale powers, hairpin weights, q5, q3, partial sums"))) return rc;
  if ((rc = B.alloc(&d_u8, n_u8, "sequences, centroids"))) return rc;
  if ((rc = bind_rows(B, K, R, s0, d_u8, hF, H))) return rc;

  std::vector<size_t> pow_off((size_t)n), cen_off((size_t)n);
  size_t a_tri = 0, a_L = 0, a_part = 0;
  for (int k = 0; k < n; k++) {
    const int L = R.len[s0 + k];
    SfPfLong &F = hF[k];
    F.hpx = d_f64 + o_hp;
    pow_off[k] = 2 * (a_L + 2 * (size_t)k);
    F.sc = d_f64 + o_pow + pow_off[k];
    F.mlbs = F.sc + (size_t)L + 2;
    pfl_bind_tables(F, d_tri, a_tri);
    F.q5 = d_f64 + o_q5 + a_L + 2 * (size_t)k;
    F.q3 = d_f64 + o_q3 + a_L + 3 * (size_t)k;
    F.part = d_f64 + o_part + a_part;
    F.out = d_f64 + o_out + 3 * (size_t)k;
    cen_off[k] = a_L + (size_t)k;
    F.cen = (char *)d_u8 + o_cen + cen_off[k];
    a_tri += SF_LONG_TRI(L);
    a_L += (size_t)L;
    a_part += 2 * (size_t)pfl_prob_waves(L, lanes);
  }
  HIPCHK(hipMemcpyAsync(d_f64 + o_hp, hhp.data(), hhp.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
  if ((rc = launch.bind(B, hF))) return rc;
  for (auto &e : B.ev) HIPCHK(hipEventCreate(&e));

  // 0: waits for an inside pass; 1: in range, waits for the outside pass; 2: done
  enum { PENDING = 0, READY = 1, DONE = 2 };
  std::vector<int> state((size_t)n, PENDING), attempts((size_t)n, 0);
  std::vector<double> lns((size_t)n), lz((size_t)n, 0.0);
  std::vector<uint8_t> act((size_t)n);
  for (int k = 0; k < n; k++)
    lns[k] = pfl_first_lns(hint && hint[s0 + k] != SF_PF_LONG_NO_HINT ? &hint[s0 + k] : nullptr, kT, R.len[s0 + k]);
  // every way out once something was launched: the status word is read, and the scales and attempts go with the rows
  auto leave = [&](int range_rc) {
    for (int k = 0; k < n; k++) {
      rows_host[s0 + k].lns = lns[k];
      rows_host[s0 + k].attempts = attempts[k];
    }
    const int status_rc = read_status(g.stream, false);
    return status_rc ? status_rc : range_rc;
  };
  int n_done = 0;
  float ms = 0;
  while (n_done < n) {
    // inside passes until every row that is not done is in range; only the rows out of range repeat
    for (;;) {
      int Ltop = 0;
      for (int k = 0; k < n; k++) {
        act[k] = state[k] == PENDING;
        if (!act[k]) continue;
        if (attempts[k] >= SF_PFLONG_MAX_ATTEMPTS) return leave(SF_ERR_RANGE);
        attempts[k]++;
        const int L = R.len[s0 + k];
        Ltop = std::max(Ltop, L);
        pfl_scale_powers(lns[k], ln_mlbase, L, hpow.data() + pow_off[k], hpow.data() + pow_off[k] + (size_t)L + 2);
      }
      if (!Ltop) break;
      // (the rows that keep their scale keep their powers: the copy writes them the values they have)
      HIPCHK(hipMemcpyAsync(d_f64 + o_pow, hpow.data(), n_pow * sizeof(double), hipMemcpyHostToDevice, g.stream));
      if ((rc = launch.mark(act.data()))) return rc;
      HIPCHK(hipEventRecord(B.ev[0], g.stream));
      for (int d = 0; d < Ltop; d++) launch.inside(Ltop, d);
      HIPCHK(hipGetLastError());
      launch.exterior();
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(B.ev[1], g.stream));
      HIPCHK(hipMemcpyAsync(hout.data(), d_f64 + o_out, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
      HIPCHK(hipStreamSynchronize(g.stream));
      HIPCHK(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
      ms_out[0] += ms;
      (*passes)++;
      for (int k = 0; k < n; k++) {
        if (!act[k]) continue;
        lz[k] = hout[3 * (size_t)k];
        if (!isfinite(lz[k]) || fabs(lz[k]) > SF_PF_LNZ_MAX) lns[k] = pfl_next_lns(lns[k], lz[k], R.len[s0 + k]);
        else state[k] = READY;
      }
    }
    // the outside pass, the probabilities and their sums of every row in range
    int Ltop = 0;
    for (int k = 0; k < n; k++) {
      act[k] = state[k] == READY;
      if (act[k]) Ltop = std::max(Ltop, (int)R.len[s0 + k]);
    }
    if ((rc = launch.mark(act.data()))) return rc;
    HIPCHK(hipMemsetAsync(d_u8 + o_cen, '.', n_L + (size_t)n, g.stream));  // (the rows done before are on the host already)
    HIPCHK(hipEventRecord(B.ev[2], g.stream));
    for (int d = Ltop - 1; d >= SFD_TURN + 1; d--) launch.outside(Ltop, d);
    HIPCHK(hipGetLastError());
    launch.prob();
    launch.finish();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(B.ev[3], g.stream));
    HIPCHK(hipMemcpyAsync(hout.data(), d_f64 + o_out, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(hcen.data(), d_u8 + o_cen, n_L + (size_t)n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipEventElapsedTime(&ms, B.ev[2], B.ev[3]));
    ms_out[1] += ms;
    for (int k = 0; k < n; k++) {
      if (!act[k]) continue;
      const int L = R.len[s0 + k];
      const double *res = hout.data() + 3 * (size_t)k;
      if (isfinite(res[1]) && isfinite(res[2])) {
        const double dG = -(res[0] + (double)L * lns[k]) * kT / 1000.0;
        if (!isfinite(dG)) return leave(SF_ERR_RANGE);
        sf_pf_long_row &r = rows_host[s0 + k];
        r.ens_dG = dG;
        r.mean_bp_dist = res[1];
        r.centroid_dist = res[2];
        r.reserved = 0;
        if (cen_host) {
          memcpy(cen_host + cen_off[k], hcen.data() + cen_off[k], (size_t)L);
          cen_host[cen_off[k] + (size_t)L] = 0;
        }
        state[k] = DONE;
        n_done++;
      } else {
        if (fabs(lz[k]) < 1.0) return leave(SF_ERR_RANGE);  // Z_s is centred and the outside tables still leave the range
        lns[k] += lz[k] / L;
        state[k] = PENDING;
      }
    }
  }
  return leave(SF_OK);
}

// sf_pf_long's launches: the one row's state goes to its kernels by value, so nothing of it lives on the device, and the
// row is marked whenever the driver launches at all.  The lane groups and the grids are the row's own.
struct PflSingleLaunch {
  const size_t lanes = pfl_lanes();
  const SfDevParams *D = (const SfDevParams *)g.dP;
  const SfDevParamsPF *X = (const SfDevParamsPF *)g.dX;
  SfPfLong F;
  int prob_waves = 0;
  int bind(CallBufs &, const std::vector<SfPfLong> &hF) {
    F = hF[0];
    prob_waves = pfl_prob_waves(F.L, lanes);
    return SF_OK;
  }
  int mark(const uint8_t *) { return SF_OK; }
  void inside(int, int d) { pfl_launch_diagonal(sf_pflong_inside_kernel, F, d, lanes); }
  void exterior() { SF_LAUNCH(sf_pflong_exterior_kernel, 1, 64, 0, g.stream, F, D, X); }
  void outside(int, int d) { pfl_launch_diagonal(sf_pflong_outside_kernel, F, d, lanes); }
  void prob() { SF_LAUNCH(sf_pflong_prob_kernel, prob_waves, 64, 0, g.stream, F); }
  void finish() { SF_LAUNCH(sf_pflong_finish_kernel, 1, 64, 0, g.stream, F, prob_waves); }
};
}  // namespace

extern "C" {

int sf_pf_long(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double *ens_dG, double *mean_bp_dist,
               char *centroid_out, double *centroid_dist) {
  int rc = check_ready();
  if (rc) return rc;
  if (!seq || L < 1 || L > SF_MAX_LONG) return SF_ERR_BAD_ARG;
  LongRows R = {seq, 1, L, &L, cons, "sf_pf_long"};
  if ((rc = long_rows_check(R, SF_MAX_LONG))) return rc;
  // the record and the centroid are staged: nothing reaches the caller unless the call succeeds
  sf_pf_long_row row = {};
  std::vector<char> cen((size_t)L + 1);
  double ms[2] = {0, 0};
  int passes = 0;
  PflSingleLaunch launch;
  rc = pf_long_rows(R, mfe_dcal_hint, 0, 1, launch, &row, cen.data(), ms, &passes);
  if (rc && rc != SF_ERR_RANGE) return rc;
  g_pfl_ms[0] = ms[0];
  g_pfl_ms[1] = ms[1];
  g_pfl_attempts = row.attempts;
  g_pfl_lns = row.lns;
  if (rc) return rc;
  if (ens_dG) *ens_dG = row.ens_dG;
  if (mean_bp_dist) *mean_bp_dist = row.mean_bp_dist;
  if (centroid_dist) *centroid_dist = row.centroid_dist;
  if (centroid_out) memcpy(centroid_out, cen.data(), (size_t)L + 1);
  return SF_OK;
}

int sf_pf_long_times(double *inside_ms, double *outside_ms, int *attempts, double *lns) {
  SF_ENTER();
  if (inside_ms) *inside_ms = g_pfl_ms[0];
  if (outside_ms) *outside_ms = g_pfl_ms[1];
  if (attempts) *attempts = g_pfl_attempts;
  if (lns) *lns = g_pfl_lns;
  return SF_OK;
}

}  // extern "C"

// ---------------- whole-record partition function under a span in banded tables (sf_pf_banded.hip.h) ----------------
namespace {
double g_pfb_ms[2] = {0, 0};  // inside (all attempts, with q5 / q3), outside (with the probabilities) of the last sf_pf_banded
int g_pfb_attempts = 0, g_pfb_band = 0, g_pfb_launches = 0;
double g_pfb_lns = 0.0;

// |ln Z_s / L| B above which an inside pass is repeated with the scale it measured: a cell of B nucleotides is then within
// e^+-300 of its neighbours' weights, which leaves the outside pass (products of two such cells) inside FP64
const double kPfBandEpsB = 300.0;

// What sf_mea_pairs and sf_pf_banded_mea ask of mea_run, and where it is staged: the structure (L + 1 bytes), the score, the
// device-event times of fill, exterior pass and traceback, the band of the list, the fill launches, the device bytes.
struct MeaRun {
  double gamma;
  std::vector<char> db;
  double score = 0;
  double ms[3] = {0, 0, 0};
  int band = 0, launches = 0;
  size_t bytes = 0;
};
// of the last successful sf_mea_pairs or sf_pf_banded_mea
double g_mea_ms[3] = {0, 0, 0};
int g_mea_band = 0, g_mea_launches = 0;
size_t g_mea_bytes = 0;

void mea_keep(const MeaRun &R) {
  for (int k = 0; k < 3; k++) g_mea_ms[k] = R.ms[k];
  g_mea_band = R.band;
  g_mea_launches = R.launches;
  g_mea_bytes = R.bytes;
}

// B of the model: 1 + the largest j - i of the list
int mea_band(const sf_pair_prob *pairs, size_t n) {
  int B = 1;
  for (size_t t = 0; t < n; t++) B = std::max(B, 1 + (int)(pairs[t].j - pairs[t].i));
  return B;
}

// The one device path of the MEA structure (sf_mea.hip.h): weights, fill, exterior pass and traceback over a list, its
// rows' offsets and an unpaired vector that are in device memory already; Bf's four events are free.  d_M: L * B doubles
// the caller has to spare (sf_pf_banded_mea: a dead band table), or NULL: allocated here.  R.bytes counts what is
// allocated here: SF_MEA_BYTES(L, n), and 8 L B with the table.
int mea_run(CallBufs &Bf, int L, int B, const SfPairProb *d_list, const unsigned long long *d_off, size_t n, const double *d_unp,
            double *d_M, MeaRun &R) {
  int rc;
  const size_t nL = (size_t)L;
  SfMea F;
  F.L = L;
  F.B = B;
  F.n = (unsigned long long)n;
  F.list = d_list;
  F.off = d_off;
  F.u = d_unp;
  F.M = d_M;
  F.status = (int *)g.status.p;
  R.bytes = SF_MEA_BYTES(L, n);
  if (!d_M) {
    if ((rc = Bf.alloc(&F.M, nL * (size_t)B, "MEA table"))) return rc;
    R.bytes += nL * (size_t)B * sizeof(double);
  }
  if ((rc = Bf.alloc(&F.wa, n, "MEA weights"))) return rc;
  if ((rc = Bf.alloc(&F.E, nL + 2, "MEA exterior values"))) return rc;
  if ((rc = Bf.alloc(&F.stk, SF_MEA_STACK_INTS(L), "MEA traceback stack"))) return rc;
  if ((rc = Bf.alloc(&F.db, nL + 1, "MEA structure"))) return rc;
  R.db.resize(nL + 1);
  HIPCHK(hipEventRecord(Bf.ev[0], g.stream));
  if (n) SF_LAUNCH(sf_mea_weights_kernel, (int)std::min((n + 255) / 256, (size_t)4096), 256, 0, g.stream, F, 2.0 * R.gamma);
  for (int d = 0; d < B; d++) SF_LAUNCH(sf_mea_fill_kernel, (int)((nL - (size_t)d + 255) / 256), 256, 0, g.stream, F, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(Bf.ev[1], g.stream));
  SF_LAUNCH(sf_mea_exterior_kernel, 1, 64, 0, g.stream, F);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(Bf.ev[2], g.stream));
  SF_LAUNCH(sf_mea_trace_kernel, 1, 64, 0, g.stream, F);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(Bf.ev[3], g.stream));
  HIPCHK(hipMemcpyAsync(R.db.data(), F.db, nL + 1, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(&R.score, F.E + 1, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if ((rc = read_status(g.stream, false))) return rc;
  for (int k = 0; k < 3; k++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, Bf.ev[k], Bf.ev[k + 1]));
    R.ms[k] = ms;
  }
  R.band = B;
  R.launches = B;  // (the fill's, one per diagonal; the weights' launch before them is not counted)
  return SF_OK;
}

// What sf_pf_banded_probs asks of the shared host path on top of sf_pf_banded's outputs, and where it is staged: unp / ent
// hold L doubles, pairs the list; ms, bytes: the extraction's device-event time and its device allocations.  mea: NULL, or
// sf_pf_banded_mea's request, run on the extraction's device buffers (d_unp, d_off, d_list) while they are alive.
struct PfbProbs {
  double cutoff;
  std::vector<double> unp, ent;
  std::vector<sf_pair_prob> pairs;
  std::vector<int32_t> cnt;             // the rows' counts and their scan (they outlive the call's device buffers, whose
  std::vector<unsigned long long> off;  // destructor drains the copies on an early return)
  double ms = 0;
  size_t bytes = 0;
  MeaRun *mea = nullptr;
  const double *d_unp = nullptr;
  const unsigned long long *d_off = nullptr;
  const SfPairProb *d_list = nullptr;
};
static_assert(sizeof(sf_pair_prob) == 16 && sizeof(SfPairProb) == 16 && offsetof(sf_pair_prob, p) == offsetof(SfPairProb, p),
              "the device's pair record is the header's");
// of the last successful sf_pf_banded_probs: its list (host memory of the library's, freed with it) and its figures
std::vector<sf_pair_prob> g_pfbp_pairs;
double g_pfbp_ms = 0;
size_t g_pfbp_bytes = 0;

// The extraction passes of sf_pf_probs.hip.h over the tables of the attempt that succeeded, before they are freed: the
// per-nucleotide pass, the count, the scan of the counts (here, on the host), the list's allocation and the writing pass.
// Bf's events are free again by now; the two timed stretches leave out the host's scan between them.
int pfb_extract(CallBufs &Bf, const SfPfBand &F, int waves, PfbProbs &P) {
  int rc;
  const size_t nL = (size_t)F.L;
  double *d_unp, *d_ent;
  int32_t *d_cnt;
  unsigned long long *d_off;
  SfPairProb *d_list;
  if ((rc = Bf.alloc(&d_unp, nL, "unpaired probabilities"))) return rc;
  if ((rc = Bf.alloc(&d_ent, nL, "positional entropies"))) return rc;
  if ((rc = Bf.alloc(&d_cnt, nL, "pairs per row"))) return rc;
  if ((rc = Bf.alloc(&d_off, nL, "offsets of the rows in the pair list"))) return rc;
  const int col_waves = (int)std::min((nL + 63) / 64, (size_t)waves);
  float ms0 = 0, ms1 = 0;
  HIPCHK(hipEventRecord(Bf.ev[0], g.stream));
  SF_LAUNCH(sf_pfband_nuc_rows_kernel, waves, 64, 0, g.stream, F, d_unp, d_ent);
  SF_LAUNCH(sf_pfband_nuc_cols_kernel, col_waves, 64, 0, g.stream, F, d_unp, d_ent);
  SF_LAUNCH(sf_pfband_pairs_count_kernel, waves, 64, 0, g.stream, F, P.cutoff, d_cnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(Bf.ev[1], g.stream));
  std::vector<int32_t> &cnt = P.cnt;
  std::vector<unsigned long long> &off = P.off;
  cnt.resize(nL);
  off.resize(nL);
  P.unp.resize(nL);
  P.ent.resize(nL);
  HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, nL * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(P.unp.data(), d_unp, nL * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(P.ent.data(), d_ent, nL * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  unsigned long long total = 0;
  for (size_t k = 0; k < nL; k++) {
    off[k] = total;
    total += (unsigned long long)cnt[k];
  }
  P.pairs.resize((size_t)total);
  P.bytes = nL * (2 * sizeof(double) + sizeof(int32_t) + sizeof(unsigned long long)) + (size_t)total * sizeof(SfPairProb);
  if (total) {
    if ((rc = Bf.alloc(&d_list, (size_t)total, "pair list"))) return rc;
    HIPCHK(hipMemcpyAsync(d_off, off.data(), nL * sizeof(unsigned long long), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipEventRecord(Bf.ev[2], g.stream));
    SF_LAUNCH(sf_pfband_pairs_write_kernel, waves, 64, 0, g.stream, F, P.cutoff, (const unsigned long long *)d_off, total, d_list);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(Bf.ev[3], g.stream));
    HIPCHK(hipMemcpyAsync(P.pairs.data(), d_list, (size_t)total * sizeof(SfPairProb), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipEventElapsedTime(&ms1, Bf.ev[2], Bf.ev[3]));
  }
  HIPCHK(hipEventElapsedTime(&ms0, Bf.ev[0], Bf.ev[1]));
  P.ms = (double)ms0 + (double)ms1;
  if (P.mea) {  // (an empty list never had its offsets copied up)
    if (!total) HIPCHK(hipMemsetAsync(d_off, 0, nL * sizeof(unsigned long long), g.stream));
    P.d_unp = d_unp;
    P.d_off = d_off;
    P.d_list = total ? d_list : nullptr;
  }
  return SF_OK;
}

// The host path of sf_pf_banded and sf_pf_banded_probs, after check_ready.  probs == NULL: sf_pf_banded, whose
// allocations (SF_PF_BANDED_BYTES) and launches are exactly these; else the extraction follows the outside pass of the
// attempt that succeeded and is staged in *probs.  `who` names the entry point in an out-of-memory text.
int pf_banded_run(const char *who, const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double *ens_dG,
                  double *mean_bp_dist, char *centroid_out, double *centroid_dist, PfbProbs *probs) {
  int rc;
  if (!seq || L < 1 || L > SF_MAX_BANDED || g.max_bp_span < 1) return SF_ERR_BAD_ARG;
  const int B = std::min(g.max_bp_span, L);
  LongRows R = {seq, 1, L, &L, cons, who};  // the record as a batch's one row; unbalanced brackets end the call here
  if ((rc = long_rows_check(R, SF_MAX_BANDED))) return rc;

  const Ctx::ModelSlot &M = g.slot[g.cur];
  const double kT = M.pf_kT, ln_mlbase = log(M.pf_MLbase);
  const size_t nL = (size_t)L, nB = (size_t)B, lanes = pfl_lanes();
  const int prob_waves = std::min(pfl_prob_waves(L, lanes), SF_PFBAND_MAX_WAVES);
  const LongPack K = long_pack(R, 0, 1);
  const std::vector<double> hhp = pfl_hairpin_table(M, B);
  // (these outlive Bf: the copies out of and into them are drained by its destructor on an early return)
  std::vector<SfPfBand> hF(1);
  HcStage<SfPfBand> H;
  std::vector<double> hpow(2 * (nB + 2));
  std::vector<char> hcen(nL + 1);
  double hout[3] = {0, 0, 0};

  // slices of the FP64 block, in elements: results, the powers of the scale, hairpin weights, the mantissas of q5 and q3,
  // the partial sums of the probability pass.  SF_PF_BANDED_BYTES counts exactly these allocations.
  const size_t o_out = 0, o_pow = o_out + 4, o_hp = o_pow + 2 * (nB + 2), o_m5 = o_hp + nB + 1, o_m3 = o_m5 + nL + 2;
  const size_t o_part = o_m3 + nL + 2, n_f64 = o_part + 2 * (size_t)SF_PFBAND_MAX_WAVES;
  CallBufs Bf(who);
  double *d_tab[SF_PFBAND_NTAB], *d_f64;
  uint8_t *d_u8;
  for (int k = 0; k < SF_PFBAND_NTAB; k++)
    if ((rc = Bf.alloc(&d_tab[k], nL * nB, kPfTableNames[k]))) return rc;
  if ((rc = Bf.alloc(&d_f64, n_f64, "results, scale powers, hairpin weights, q5, q3, partial sums"))) return rc;
  if ((rc = Bf.alloc(&d_u8, K.o_end + nL + 1, "sequence, centroid"))) return rc;
  if ((rc = bind_rows(Bf, K, R, 0, d_u8, hF, H))) return rc;
  SfPfBand &F = hF[0];
  F.B = B;
  if ((rc = Bf.alloc(&F.e5, 2 * (nL + 2), "exponents of q5 and q3"))) return rc;
  F.e3 = F.e5 + nL + 2;
  F.cen = (char *)d_u8 + K.o_end;
  pfl_bind_tables(F, d_tab, 0);
  F.out = d_f64 + o_out;
  F.sc = d_f64 + o_pow;
  F.mlbs = F.sc + nB + 2;
  F.hpx = d_f64 + o_hp;
  F.m5 = d_f64 + o_m5;
  F.m3 = d_f64 + o_m3;
  F.part = d_f64 + o_part;
  HIPCHK(hipMemcpyAsync(d_f64 + o_hp, hhp.data(), hhp.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
  for (auto &e : Bf.ev) HIPCHK(hipEventCreate(&e));

  const SfDevParams *D = (const SfDevParams *)g.dP;
  const SfDevParamsPF *X = (const SfDevParamsPF *)g.dX;
  // (a band of at most TURN + 1 diagonals holds no pair: Z = 1 whatever the scale, and scale 1 gives it exactly)
  double lns = B <= SFD_TURN + 1 ? 0.0 : pfl_first_lns(mfe_dcal_hint, kT, L), ms_in = 0, ms_out = 0, dG = 0;
  int attempts = 0, launches = 0;
  // every way out once something was launched: the status word is read, and the times, scale and attempts are kept
  auto leave = [&](int range_rc) {
    const int status_rc = read_status(g.stream, false);
    if (status_rc) return status_rc;
    g_pfb_ms[0] = ms_in;
    g_pfb_ms[1] = ms_out;
    g_pfb_attempts = attempts;
    g_pfb_lns = lns;
    g_pfb_band = B;
    g_pfb_launches = launches;
    return range_rc;
  };
  float ms = 0;
  for (;;) {
    if (attempts >= SF_PFLONG_MAX_ATTEMPTS) return leave(SF_ERR_RANGE);
    attempts++;
    pfl_scale_powers(lns, ln_mlbase, B, hpow.data(), hpow.data() + nB + 2);
    HIPCHK(hipMemcpyAsync(d_f64 + o_pow, hpow.data(), hpow.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipEventRecord(Bf.ev[0], g.stream));
    for (int d = 0; d < B; d++) pfl_launch_diagonal(sf_pfband_inside_kernel, F, d, lanes);
    HIPCHK(hipGetLastError());
    SF_LAUNCH(sf_pfband_exterior_kernel, 2, 64, 0, g.stream, F, D, X);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(Bf.ev[1], g.stream));
    HIPCHK(hipMemcpyAsync(hout, d_f64 + o_out, sizeof hout, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipEventElapsedTime(&ms, Bf.ev[0], Bf.ev[1]));
    ms_in += ms;
    launches += B;
    // The exterior loop carries its own exponents, so a finite ln Z_s gives the scale's error per nucleotide exactly
    // whatever its size; where the band tables left the range, step by what a cell of B nucleotides can bear.
    const double lz = hout[0], eps = lz / L;
    if (!isfinite(lz)) {  // (an overflow gives +inf or NaN; NaN counts as an overflow)
      lns += (lz < 0 ? -700.0 : 700.0) / B;
      continue;
    }
    if (fabs(eps) * B > kPfBandEpsB) {
      lns += eps;
      continue;
    }
    HIPCHK(hipMemsetAsync(F.cen, '.', nL + 1, g.stream));
    HIPCHK(hipEventRecord(Bf.ev[2], g.stream));
    for (int d = B - 1; d >= SFD_TURN + 1; d--) pfl_launch_diagonal(sf_pfband_outside_kernel, F, d, lanes);
    HIPCHK(hipGetLastError());
    SF_LAUNCH(sf_pfband_prob_kernel, prob_waves, 64, 0, g.stream, F);
    SF_LAUNCH(sf_pfband_finish_kernel, 1, 64, 0, g.stream, F, prob_waves);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(Bf.ev[3], g.stream));
    HIPCHK(hipMemcpyAsync(hout, d_f64 + o_out, sizeof hout, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(hcen.data(), F.cen, nL, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipEventElapsedTime(&ms, Bf.ev[2], Bf.ev[3]));
    ms_out += ms;
    launches += std::max(0, B - 1 - SFD_TURN);
    if (isfinite(hout[1]) && isfinite(hout[2])) {
      dG = -(lz + (double)L * lns) * kT / 1000.0;
      if (!isfinite(dG)) return leave(SF_ERR_RANGE);
      break;
    }
    if (fabs(eps) * B < 1.0) return leave(SF_ERR_RANGE);  // Z_s is centred and the outside tables still leave the range
    lns += eps;
  }
  if (probs && (rc = pfb_extract(Bf, F, prob_waves, *probs))) return rc;
  // The MEA structure of that list, from the device buffers of the extraction.  All seven band tables are dead once the
  // extraction has read ob and qb; M (L doubles a diagonal of the list's band, which is at most B) lives in the second,
  // "qb by columns / A0".
  if (probs && probs->mea &&
      (rc = mea_run(Bf, L, mea_band(probs->pairs.data(), probs->pairs.size()), probs->d_list, probs->d_off, probs->pairs.size(),
                    probs->d_unp, d_tab[1], *probs->mea)))
    return rc;
  if ((rc = leave(SF_OK))) return rc;
  // staged until here: nothing reaches the caller unless the call succeeds
  hcen[nL] = 0;
  if (ens_dG) *ens_dG = dG;
  if (mean_bp_dist) *mean_bp_dist = hout[1];
  if (centroid_dist) *centroid_dist = hout[2];
  if (centroid_out) memcpy(centroid_out, hcen.data(), nL + 1);
  return SF_OK;
}
}  // namespace

extern "C" {

int sf_pf_banded_bytes(int L, int span, size_t *bytes) {
  SF_ENTER();
  if (L < 1 || L > SF_MAX_BANDED || span < 1 || !bytes) return SF_ERR_BAD_ARG;
  *bytes = SF_PF_BANDED_BYTES(L, std::min(span, L));
  return SF_OK;
}

int sf_pf_banded(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double *ens_dG, double *mean_bp_dist,
                 char *centroid_out, double *centroid_dist) {
  const int rc = check_ready();
  if (rc) return rc;
  return pf_banded_run("sf_pf_banded", seq, L, cons, mfe_dcal_hint, ens_dG, mean_bp_dist, centroid_out, centroid_dist, nullptr);
}

}  // extern "C"

namespace {
// sf_pf_banded_probs (mea == NULL) and sf_pf_banded_mea after check_ready: one body, so the ten outputs they share are the
// same bytes.  *mea comes back staged; its caller hands it on.
int pf_banded_probs_call(const char *who, const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double cutoff,
                         double *ens_dG, double *mean_bp_dist, char *centroid_out, double *centroid_dist, double *unpaired_out,
                         double *entropy_out, size_t *n_pairs, MeaRun *mea) {
  if (!(cutoff > 0.0 && cutoff <= 1.0)) return SF_ERR_BAD_ARG;  // (a NaN fails both comparisons)
  // the vectors and the list are staged like the four classic outputs, which wait in locals until the extraction is in
  PfbProbs P;
  P.cutoff = cutoff;
  P.mea = mea;
  double dG = 0, mbd = 0, cd = 0;
  std::vector<char> cen(centroid_out ? (size_t)std::max(L, 0) + 1 : 0);
  const int rc = pf_banded_run(who, seq, L, cons, mfe_dcal_hint, &dG, &mbd, centroid_out ? cen.data() : nullptr, &cd, &P);
  if (rc) return rc;  // (the list of the last successful call stays as it is)
  g_pfbp_pairs.swap(P.pairs);
  g_pfbp_ms = P.ms;
  g_pfbp_bytes = P.bytes;
  if (ens_dG) *ens_dG = dG;
  if (mean_bp_dist) *mean_bp_dist = mbd;
  if (centroid_dist) *centroid_dist = cd;
  if (centroid_out) memcpy(centroid_out, cen.data(), (size_t)L + 1);
  if (unpaired_out) memcpy(unpaired_out, P.unp.data(), (size_t)L * sizeof(double));
  if (entropy_out) memcpy(entropy_out, P.ent.data(), (size_t)L * sizeof(double));
  if (n_pairs) *n_pairs = g_pfbp_pairs.size();
  return SF_OK;
}

bool mea_gamma_ok(double gamma) { return isfinite(gamma) && gamma > 0.0; }
}  // namespace

extern "C" {

int sf_pf_banded_probs(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double cutoff, double *ens_dG,
                       double *mean_bp_dist, char *centroid_out, double *centroid_dist, double *unpaired_out,
                       double *entropy_out, size_t *n_pairs) {
  const int rc = check_ready();
  if (rc) return rc;
  return pf_banded_probs_call("sf_pf_banded_probs", seq, L, cons, mfe_dcal_hint, cutoff, ens_dG, mean_bp_dist, centroid_out,
                              centroid_dist, unpaired_out, entropy_out, n_pairs, nullptr);
}

int sf_pf_banded_mea(const uint8_t *seq, int L, const char *cons, const int32_t *mfe_dcal_hint, double cutoff, double gamma,
                     double *ens_dG, double *mean_bp_dist, char *centroid_out, double *centroid_dist, double *unpaired_out,
                     double *entropy_out, size_t *n_pairs, char *mea_out, double *mea_score) {
  int rc = check_ready();
  if (rc) return rc;
  if (!mea_gamma_ok(gamma)) return SF_ERR_BAD_ARG;
  MeaRun R;
  R.gamma = gamma;
  rc = pf_banded_probs_call("sf_pf_banded_mea", seq, L, cons, mfe_dcal_hint, cutoff, ens_dG, mean_bp_dist, centroid_out,
                            centroid_dist, unpaired_out, entropy_out, n_pairs, &R);
  if (rc) return rc;
  mea_keep(R);
  if (mea_out) memcpy(mea_out, R.db.data(), (size_t)L + 1);
  if (mea_score) *mea_score = R.score;
  return SF_OK;
}

int sf_mea_pairs(int L, const sf_pair_prob *pairs, size_t n, const double *unpaired, double gamma, char *mea_out,
                 double *mea_score) {
  SF_ENTER();
  if (L < 1 || L > SF_MAX_BANDED || (!pairs && n) || !unpaired || !mea_gamma_ok(gamma)) return SF_ERR_BAD_ARG;
  for (int k = 0; k < L; k++)
    if (!(unpaired[k] >= 0.0 && unpaired[k] <= 1.0)) return SF_ERR_BAD_ARG;  // (a NaN fails both comparisons)
  // the rows' offsets, on the host as sf_pf_banded_probs scans its counts
  std::vector<unsigned long long> off((size_t)L, 0);
  for (size_t t = 0; t < n; t++) {
    const sf_pair_prob &r = pairs[t];
    if (r.i < 1 || r.i >= r.j || r.j > L || !(r.p >= 0.0 && r.p <= 1.0)) return SF_ERR_BAD_ARG;
    if (t && (r.i < pairs[t - 1].i || (r.i == pairs[t - 1].i && r.j <= pairs[t - 1].j))) return SF_ERR_BAD_ARG;
    if (r.i < L) off[(size_t)r.i]++;  // (counted at the next row: the running sum below makes it that row's start)
  }
  for (int k = 1; k < L; k++) off[(size_t)k] += off[(size_t)k - 1];
  int rc;
  MeaRun R;
  R.gamma = gamma;
  {
    CallBufs Bf("sf_mea_pairs");
    SfPairProb *d_list;
    unsigned long long *d_off;
    double *d_unp;
    if ((rc = Bf.upload(&d_list, (const SfPairProb *)pairs, n, "pair list"))) return rc;
    if ((rc = Bf.upload(&d_off, (const unsigned long long *)off.data(), (size_t)L, "offsets of the rows in the pair list"))) return rc;
    if ((rc = Bf.upload(&d_unp, unpaired, (size_t)L, "unpaired probabilities"))) return rc;
    for (auto &e : Bf.ev) HIPCHK(hipEventCreate(&e));
    if ((rc = mea_run(Bf, L, mea_band(pairs, n), d_list, d_off, n, d_unp, nullptr, R))) return rc;
  }
  R.bytes += n * sizeof(SfPairProb) + 2 * (size_t)L * sizeof(double);
  mea_keep(R);
  if (mea_out) memcpy(mea_out, R.db.data(), (size_t)L + 1);
  if (mea_score) *mea_score = R.score;
  return SF_OK;
}

int sf_mea_times(double *fill_ms, double *ext_ms, double *trace_ms, int *band, int *fill_launches, size_t *extra_bytes) {
  SF_ENTER();
  if (fill_ms) *fill_ms = g_mea_ms[0];
  if (ext_ms) *ext_ms = g_mea_ms[1];
  if (trace_ms) *trace_ms = g_mea_ms[2];
  if (band) *band = g_mea_band;
  if (fill_launches) *fill_launches = g_mea_launches;
  if (extra_bytes) *extra_bytes = g_mea_bytes;
  return SF_OK;
}

int sf_pf_probs_pairs(sf_pair_prob *out, size_t cap, size_t *n) {
  SF_ENTER();
  if (cap && !out) return SF_ERR_BAD_ARG;
  const size_t have = g_pfbp_pairs.size(), m = std::min(cap, have);
  if (m) memcpy(out, g_pfbp_pairs.data(), m * sizeof(sf_pair_prob));
  if (n) *n = have;
  return SF_OK;
}

int sf_pf_banded_probs_times(double *extract_ms, size_t *n_pairs, size_t *extra_bytes) {
  SF_ENTER();
  if (extract_ms) *extract_ms = g_pfbp_ms;
  if (n_pairs) *n_pairs = g_pfbp_pairs.size();
  if (extra_bytes) *extra_bytes = g_pfbp_bytes;
  return SF_OK;
}

int sf_pf_banded_times(double *inside_ms, double *outside_ms, int *attempts, double *lns, int *band, int *launches) {
  SF_ENTER();
  if (inside_ms) *inside_ms = g_pfb_ms[0];
  if (outside_ms) *outside_ms = g_pfb_ms[1];
  if (attempts) *attempts = g_pfb_attempts;
  if (lns) *lns = g_pfb_lns;
  if (band) *band = g_pfb_band;
  if (launches) *launches = g_pfb_launches;
  return SF_OK;
}

}  // extern "C"

// ---------------- many whole-record partition functions at once (sf_pf_long_batch.hip.h) ----------------
namespace {
double g_pflb_ms[2] = {0, 0};  // inside passes (q5 / q3 included), outside and probability passes of the last sf_pf_long_batch
int g_pflb_chunks = 0, g_pflb_passes = 0;

size_t pf_long_row_bytes(int L) { return SF_PFLONG_BYTES(L); }

// A chunk's launches: the row states and the marks of the rows at work in one device allocation, every launch over all rows.
struct PflBatchLaunch {
  const size_t lanes = pfl_lanes();
  const size_t budget = (size_t)(g.n_cu > 0 ? g.n_cu : 1) * SF_PFLONGB_LANES_PER_CU;  // the chunk's own, per launch
  const SfDevParams *D = (const SfDevParams *)g.dP;
  const SfDevParamsPF *X = (const SfDevParamsPF *)g.dX;
  const int threads = SF_PFLONGB_THREADS;
  int n = 0, wmax = 0;
  const SfPfLong *d_F = nullptr;
  uint8_t *d_act = nullptr;
  int bind(CallBufs &B, const std::vector<SfPfLong> &hF) {
    n = (int)hF.size();
    for (const SfPfLong &F : hF) wmax = std::max(wmax, pfl_prob_waves(F.L, lanes));
    uint8_t *p;  // the states, then a mark a row
    const int rc = B.alloc(&p, (size_t)n * (sizeof(SfPfLong) + 1), "partition function states, row marks");
    if (rc) return rc;
    d_F = (const SfPfLong *)p;
    d_act = p + (size_t)n * sizeof(SfPfLong);
    HIPCHK(hipMemcpyAsync(p, hF.data(), (size_t)n * sizeof(SfPfLong), hipMemcpyHostToDevice, g.stream));
    return SF_OK;
  }
  int mark(const uint8_t *act) {
    HIPCHK(hipMemcpyAsync(d_act, act, (size_t)n, hipMemcpyHostToDevice, g.stream));
    return SF_OK;
  }
  // workgroups per row on diagonal d when the longest live row has Ltop nt: what sf_pf_long would give that row, cut down
  // until the whole launch fits the batch's budget (at least one).  It orders no sum: a group walks more cells instead.
  int blocks_per_row(int Ltop, int d) const {
    const size_t cells = (size_t)(Ltop - d);
    const size_t want = std::min(cells * (size_t)pfl_group(1, d, lanes), lanes);
    const size_t bps = (want + threads - 1) / threads, fit = budget / ((size_t)n * threads);
    return (int)std::max<size_t>(1, std::min(bps, fit));
  }
  void inside(int Ltop, int d) {
    const int bps = blocks_per_row(Ltop, d);
    SF_LAUNCH(sf_pflongb_inside_kernel, n * bps, threads, 0, g.stream, d_F, (const uint8_t *)d_act, d, bps, (int)lanes, D, X);
  }
  void exterior() { SF_LAUNCH(sf_pflongb_exterior_kernel, n, 64, 0, g.stream, d_F, (const uint8_t *)d_act, D, X); }
  void outside(int Ltop, int d) {
    const int bps = blocks_per_row(Ltop, d);
    SF_LAUNCH(sf_pflongb_outside_kernel, n * bps, threads, 0, g.stream, d_F, (const uint8_t *)d_act, d, bps, (int)lanes, D, X);
  }
  void prob() {
    const int pbps = (wmax + threads / 64 - 1) / (threads / 64);
    SF_LAUNCH(sf_pflongb_prob_kernel, n * pbps, threads, 0, g.stream, d_F, (const uint8_t *)d_act, pbps, (int)lanes);
  }
  void finish() { SF_LAUNCH(sf_pflongb_finish_kernel, n, 64, 0, g.stream, d_F, (const uint8_t *)d_act, (int)lanes); }
};
}  // namespace

extern "C" {

int sf_pf_long_batch(const uint8_t *seqs, int n, int ld, const int32_t *len, const char *cons, const int32_t *mfe_dcal_hint,
                     sf_pf_long_row *out, char *centroid_out) {
  int rc = check_ready();
  if (rc) return rc;
  LongRows R = {seqs, n, ld, len, cons, "sf_pf_long_batch"};
  if ((rc = long_rows_check(R, SF_MAX_LONG))) return rc;
  // the records are staged and handed over, like the centroids, only when every chunk has succeeded
  std::vector<sf_pf_long_row> rows_host((size_t)n);
  double ms[2] = {0, 0};
  int chunks, passes = 0;
  rc = long_for_chunks(R, pf_long_row_bytes, centroid_out, &chunks, [&](int s0, int m, char *cen_host) {
    PflBatchLaunch launch;
    return pf_long_rows(R, mfe_dcal_hint, s0, m, launch, rows_host.data(), cen_host, ms, &passes);
  });
  if (rc) return rc;  // (n == 0: no chunk)
  if (out && n > 0) memcpy(out, rows_host.data(), (size_t)n * sizeof(sf_pf_long_row));
  g_pflb_ms[0] = ms[0];
  g_pflb_ms[1] = ms[1];
  g_pflb_chunks = chunks;
  g_pflb_passes = passes;
  return SF_OK;
}

int sf_pf_long_batch_times(double *inside_ms, double *outside_ms, int *chunks, int *inside_passes) {
  SF_ENTER();
  if (inside_ms) *inside_ms = g_pflb_ms[0];
  if (outside_ms) *outside_ms = g_pflb_ms[1];
  if (chunks) *chunks = g_pflb_chunks;
  if (inside_passes) *inside_passes = g_pflb_passes;
  return SF_OK;
}

}  // extern "C"

// ---------------- duplex folds and the LRI scan (include/scanfold_hip_duplex.h) ----------------
namespace {
double g_lri_ms = 0.0;
int64_t g_lri_duplexes = 0;

int dup_grid(long long tasks) {  // workgroups of a grid-stride launch: enough for every CU's LDS, bounded scratch
  const long long cap = (long long)(g.n_cu > 0 ? g.n_cu : 1) * 8;
  return (int)(tasks < cap ? (tasks < 1 ? 1 : tasks) : cap);
}

// n pairs that are already on the device as codes -> energies (and records) on the device
int launch_duplex_batch(CallBufs &B, SfDupBatch A, int max1, int max2) {
  if (A.n <= 0) return SF_OK;
  const int grid = dup_grid(((long long)A.n + SF_DUP_BLOCK - 1) / SF_DUP_BLOCK);
  int rc = B.alloc(&A.scratch, (size_t)(max1 > 0 ? max1 : 1) * (max2 > 0 ? max2 : 1) * grid * SF_DUP_BLOCK, "duplex tables");
  if (rc) return rc;
  A.max2 = max2 > 0 ? max2 : 1;
  A.status = (int *)g.status.p;
  SF_LAUNCH(sf_duplex_batch_kernel, grid, SF_DUP_BLOCK, 0, g.stream, A, (const SfDevParams *)g.dP);
  HIPCHK(hipGetLastError());
  return SF_OK;
}

void lri_grid(int L, int kmer, int step, int *n_j, int *n_k) {
  // j_win = 0, step, ... while j_win == 0 or j_win <= L - kmer + 1;  k_win likewise up to L - kmer (ScanFold.py:774,780).
  // L < kmer: the single (0, 0) iteration never passes the distance test.
  if (L < kmer) { *n_j = 0; *n_k = 0; return; }
  *n_j = (L - kmer + 1) / step + 1;
  *n_k = (L - kmer) / step + 1;
}
}  // namespace

extern "C" {

int sf_duplex_batch(const uint8_t *s1, const uint8_t *s2, int n, int ld, const int32_t *len1, const int32_t *len2,
                    int32_t *energy_out, int32_t *i_out, int32_t *j_out, char *structure_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (n < 0 || ld < 1 || (n > 0 && (!s1 || !s2 || !len1 || !len2 || !energy_out))) return SF_ERR_BAD_ARG;
  if (n == 0) return SF_OK;
  int max1 = 0, max2 = 0;
  for (int p = 0; p < n; p++) {
    if (len1[p] < 0 || len2[p] < 0 || len1[p] > SF_DUPLEX_MAX_LEN || len2[p] > SF_DUPLEX_MAX_LEN || len1[p] > ld || len2[p] > ld)
      return SF_ERR_BAD_ARG;
    if (len1[p] > max1) max1 = len1[p];
    if (len2[p] > max2) max2 = len2[p];
  }
  std::vector<uint8_t> c1((size_t)n * ld), c2((size_t)n * ld);
  for (size_t x = 0; x < c1.size(); x++) { c1[x] = sf_encode_nt(s1[x]); c2[x] = sf_encode_nt(s2[x]); }
  CallBufs B("sf_duplex_batch");
  SfDupBatch A;
  memset(&A, 0, sizeof A);
  uint8_t *d1, *d2;
  int32_t *dl1, *dl2;
  if ((rc = B.upload(&d1, c1.data(), c1.size(), "first strands")) || (rc = B.upload(&d2, c2.data(), c2.size(), "second strands")) ||
      (rc = B.upload(&dl1, len1, (size_t)n, "first lengths")) || (rc = B.upload(&dl2, len2, (size_t)n, "second lengths")))
    return rc;
  if ((rc = B.alloc(&A.e, (size_t)n, "energies")) || (rc = B.alloc(&A.i, (size_t)n, "i")) || (rc = B.alloc(&A.j, (size_t)n, "j")))
    return rc;
  if (structure_out && (rc = B.alloc(&A.structure, (size_t)n * SF_DUPLEX_STRUCT_LEN, "structures"))) return rc;
  A.s1 = d1; A.s2 = d2; A.len1 = dl1; A.len2 = dl2; A.n = n; A.ld = ld;
  if ((rc = launch_duplex_batch(B, A, max1, max2))) return rc;
  HIPCHK(hipMemcpyAsync(energy_out, A.e, n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (i_out) HIPCHK(hipMemcpyAsync(i_out, A.i, n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (j_out) HIPCHK(hipMemcpyAsync(j_out, A.j, n * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (structure_out)
    HIPCHK(hipMemcpyAsync(structure_out, A.structure, (size_t)n * SF_DUPLEX_STRUCT_LEN, hipMemcpyDeviceToHost, g.stream));
  return read_status(g.stream, false);
}

int sf_lri_grid(int L, int kmer, int step, int32_t *n_j, int32_t *n_k) {
  if (L < 0 || kmer < 2 || step < 1 || !n_j || !n_k) return SF_ERR_BAD_ARG;
  int a, b;
  lri_grid(L, kmer, step, &a, &b);
  *n_j = a; *n_k = b;
  return SF_OK;
}

int sf_lri_scan(const uint8_t *seq, int L, int kmer, int step, int32_t cutoff_dcal, int64_t max_hits, sf_lri_hit *hits_out,
                int64_t *n_hits_out, int32_t *dense_e, int32_t *dense_i, int32_t *dense_j) {
  int rc = check_ready();
  if (rc) return rc;
  const bool dense = dense_e != nullptr;
  if (!seq || L < 1 || kmer < 2 || kmer > SF_DUPLEX_MAX_LEN || step < 1 || max_hits < 0 || max_hits > 0x7fffffffLL)
    return SF_ERR_BAD_ARG;
  if (dense ? (!dense_i || !dense_j) : (!n_hits_out || (max_hits > 0 && !hits_out))) return SF_ERR_BAD_ARG;
  if (n_hits_out) *n_hits_out = 0;
  int n_j, n_k;
  lri_grid(L, kmer, step, &n_j, &n_k);
  g_lri_ms = 0.0;
  g_lri_duplexes = 0;
  if (n_j == 0 || n_k == 0) return SF_OK;
  if (dense && (long long)n_j * n_k > 0x7fffffffLL / 4) return SF_ERR_BAD_ARG;

  std::vector<uint8_t> codes((size_t)L);
  for (int x = 0; x < L; x++) codes[x] = sf_encode_nt(seq[x]);
  CallBufs B("sf_lri_scan");
  SfLriScan A;
  memset(&A, 0, sizeof A);
  uint8_t *dcodes;
  if ((rc = B.upload(&dcodes, codes.data(), codes.size(), "sequence"))) return rc;
  A.codes = dcodes; A.L = L; A.kmer = kmer; A.step = step; A.n_j = n_j; A.n_k = n_k;
  A.n_chunk = (n_k + SF_DUP_BLOCK - 1) / SF_DUP_BLOCK;
  A.cutoff = cutoff_dcal;
  A.max_hits = (unsigned)max_hits;
  const size_t nd = (size_t)n_j * n_k;
  if (dense) {
    if ((rc = B.alloc(&A.dense_e, nd, "dense energies")) || (rc = B.alloc(&A.dense_i, nd, "dense i")) ||
        (rc = B.alloc(&A.dense_j, nd, "dense j")))
      return rc;
  } else {
    if ((rc = B.alloc(&A.hits, (size_t)max_hits, "hits"))) return rc;
  }
  if ((rc = B.alloc(&A.n_hits, 1, "hit count"))) return rc;
  HIPCHK(hipMemsetAsync(A.n_hits, 0, sizeof(unsigned), g.stream));

  const long long tasks = (long long)n_j * A.n_chunk;
  const int grid = dup_grid(tasks);
  const size_t strands = (size_t)kmer * SF_DUP_BLOCK + (size_t)kmer;
  const size_t ctab = (size_t)kmer * kmer * SF_DUP_BLOCK * sizeof(int16_t);
  const bool ldsc = ctab + strands <= SF_DUP_LDS_BUDGET;
  const size_t lds = ldsc ? ctab + strands : strands;
  if (strands > SF_DUP_LDS_BUDGET) return SF_ERR_BAD_ARG;
  if (ldsc) {
    HIPCHK(hipFuncSetAttribute((const void *)sf_lri_scan_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  } else {
    if ((rc = B.alloc(&A.scratch, ctab / sizeof(int16_t) * grid, "duplex tables"))) return rc;
  }
  // Bound the TIME of one launch, not its task count: the work of a duplex grows with kmer^4 (measured: 3.7e6 duplexes/s at
  // k = 20, 4.6e5 at k = 40), so a launch takes 8e6 * (20 / kmer)^4 duplexes — one to two seconds — and never fewer tasks
  // than the grid has workgroups.
  long long per_launch = (long long)(8.0e6 * (20.0 / kmer) * (20.0 / kmer) * (20.0 / kmer) * (20.0 / kmer)) / SF_DUP_BLOCK;
  if (per_launch < grid) per_launch = grid;
  for (int k = 0; k < 2; k++) HIPCHK(hipEventCreate(&B.ev[k]));
  HIPCHK(hipEventRecord(B.ev[0], g.stream));
  for (long long t0 = 0; t0 < tasks; t0 += per_launch) {
    const long long t1 = t0 + per_launch < tasks ? t0 + per_launch : tasks;
    if (ldsc)
      SF_LAUNCH(sf_lri_scan_kernel<true>, grid, SF_DUP_BLOCK, lds, g.stream, A, t0, t1, (const SfDevParams *)g.dP);
    else
      SF_LAUNCH(sf_lri_scan_kernel<false>, grid, SF_DUP_BLOCK, lds, g.stream, A, t0, t1, (const SfDevParams *)g.dP);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(B.ev[1], g.stream));
  unsigned count = 0;
  HIPCHK(hipMemcpyAsync(&count, A.n_hits, sizeof count, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
  g_lri_ms = ms;
  {  // the pairs the distance test lets through
    long long nd2 = 0;
    for (int jx = 0; jx < n_j; jx++) {
      const long long jw = (long long)jx * step;
      // k_win + 3 < j_win - kmer  <=>  k_win <= j_win - kmer - 4;   k_win > j_win + kmer + 3
      const long long lo = jw - kmer - 4;
      long long below = lo < 0 ? 0 : lo / step + 1;
      if (below > n_k) below = n_k;
      long long above = n_k - ((jw + kmer + 3) / step + 1);
      if (above < 0) above = 0;
      nd2 += below + above;
    }
    g_lri_duplexes = nd2;
  }
  if (dense) {
    HIPCHK(hipMemcpy(dense_e, A.dense_e, nd * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dense_i, A.dense_i, nd * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dense_j, A.dense_j, nd * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SF_OK;
  }
  *n_hits_out = (int64_t)count;
  if ((int64_t)count > max_hits) return SF_ERR_DUPLEX_HITS;
  if (count) {
    std::vector<sf_lri_hit> h(count);
    HIPCHK(hipMemcpy(h.data(), A.hits, (size_t)count * sizeof(sf_lri_hit), hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end(), [](const sf_lri_hit &a, const sf_lri_hit &b) {
      return a.j_win != b.j_win ? a.j_win < b.j_win : a.k_win < b.k_win;
    });
    memcpy(hits_out, h.data(), (size_t)count * sizeof(sf_lri_hit));
  }
  return SF_OK;
}

int sf_lri_scan_time(double *ms, int64_t *duplexes) {
  SF_ENTER();
  if (ms) *ms = g_lri_ms;
  if (duplexes) *duplexes = g_lri_duplexes;
  return SF_OK;
}

int sf_lri_background(const uint8_t *seq, int L, int kmer, const int32_t *j_win, const int32_t *k_win, int n_hits, int r,
                      int kind, uint64_t seed, int32_t *energies_out, uint8_t *rows1_out, uint8_t *rows2_out) {
  int rc = check_ready();
  if (rc) return rc;
  if (!seq || L < 1 || kmer < 2 || kmer > SF_DUPLEX_MAX_LEN || n_hits < 0 || r < 0 || r > 0x3fffffff) return SF_ERR_BAD_ARG;
  if (kind != SF_SHUFFLE_MONO && kind != SF_SHUFFLE_DI) return SF_ERR_BAD_ARG;
  if (n_hits == 0) return SF_OK;
  if (!j_win || !k_win || !energies_out) return SF_ERR_BAD_ARG;
  const long long rows = (long long)n_hits * (r + 1);
  if (rows > 0x7fffffffLL / SF_DUPLEX_MAX_LEN) return SF_ERR_BAD_ARG;
  for (int h = 0; h < n_hits; h++)
    if (j_win[h] < 0 || j_win[h] > L - kmer + 1 || k_win[h] < 0 || k_win[h] > L - kmer) return SF_ERR_BAD_ARG;
  std::vector<uint8_t> codes((size_t)L);
  for (int x = 0; x < L; x++) codes[x] = sf_encode_nt(seq[x]);
  CallBufs B("sf_lri_background");
  uint8_t *dcodes, *r1, *r2;
  int32_t *djw, *dkw, *l1;
  if ((rc = B.upload(&dcodes, codes.data(), codes.size(), "sequence")) || (rc = B.upload(&djw, j_win, (size_t)n_hits, "j_win")) ||
      (rc = B.upload(&dkw, k_win, (size_t)n_hits, "k_win")))
    return rc;
  SfDupBatch A;
  memset(&A, 0, sizeof A);
  const size_t nb = (size_t)rows * kmer;
  if ((rc = B.alloc(&r1, nb, "first strands")) || (rc = B.alloc(&r2, nb, "second strands")) ||
      (rc = B.alloc(&l1, (size_t)rows, "lengths")) || (rc = B.alloc(&A.e, (size_t)rows, "energies")))
    return rc;
  const int sgrid = (int)((rows + SF_SHUF_BLOCK - 1) / SF_SHUF_BLOCK);
  SF_LAUNCH(sf_lri_shuffle_kernel, sgrid, SF_SHUF_BLOCK, sf_shuffle_lds_bytes(kmer), g.stream, (const uint8_t *)dcodes, L, kmer,
            (const int32_t *)djw, (const int32_t *)dkw, n_hits, r, kind, seed, r1, r2, l1);
  HIPCHK(hipGetLastError());
  A.s1 = r1; A.s2 = r2; A.len1 = l1; A.len2 = nullptr;
  A.n = (int)rows; A.ld = kmer; A.n2 = kmer;
  if ((rc = launch_duplex_batch(B, A, kmer, kmer))) return rc;
  HIPCHK(hipMemcpyAsync(energies_out, A.e, rows * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
  if (rows1_out) HIPCHK(hipMemcpyAsync(rows1_out, r1, nb, hipMemcpyDeviceToHost, g.stream));
  if (rows2_out) HIPCHK(hipMemcpyAsync(rows2_out, r2, nb, hipMemcpyDeviceToHost, g.stream));
  return read_status(g.stream, false);
}

}  // extern "C"
