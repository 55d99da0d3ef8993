// sf_pf_long_batch.hip.h — the five passes of sf_pf_long.hip.h for MANY sequences of 1 <= L <= SF_MAX_LONG at once
// (sf_pf_long_batch): the three ensembles of --global_ensemble, fc.pf() over long fragments.  One partition function per call
// leaves the device idle: two launches per anti-diagonal and a single wave for q5 / q3, whatever the record's length.
//
// State: a device array of SfPfLong, one per row of the chunk; its tables are slices of a few allocations the host makes per
// chunk.  act[s] != 0 marks the rows a launch works on: the rows still waiting for an inside pass in range, then the rows in
// range for the outside pass.  A workgroup of any other row returns at once.
//
// Every pass is the function sf_pf_long.hip.h runs (sfp_inside, sfp_prob, sfp_finish of sf_pf_cells.hip.h over SfPfLong;
// sfpl_exterior and sfpl_outside), and what orders a row's sums is computed here from the row alone, exactly as sf_pf_long
// computes it:
//   * the group size G of diagonal d = pfl_group(L_s - d, d, lanes), lanes = the SINGLE call's budget (n_cu *
//     SF_PFLONG_LANES_PER_CU), never the batch's, never Lmax's;
//   * the probability pass's wave count = pfl_prob_waves(L_s, lanes), a wave taking rows wave, wave + nwaves, ... of the
//     triangle, and the finish adding the partial sums of that many waves in that order;
//   * sc / mlbs, the row's own powers of its own scale, made on the host by the one loop both entry points run
//     (pfl_scale_powers in pf_long_rows, scanfold_hip.hip).
// So a row's doubles are sf_pf_long's bit for bit, whatever else is in the call, in whatever order, however it is chunked.
// How many workgroups a row gets (bps), hence how many cells a group walks, is free and comes from the batch's own budget.
//
// Mapping: the grid stays one-dimensional; with bps workgroups of 256 lanes per row, workgroup b works on row b / bps at
// lanes (b % bps) * 256 .. of the row's share of bps * 256 lanes.  A wave never mixes rows, and G divides 64, so the butterfly
// of a cell's group stays inside one row.  A row with L_s <= d, and a workgroup whose first group lies past the row's cells,
// return at once; in the row's last live workgroup the lanes past L_s - d walk the butterflies without a cell.
// q5 / q3: one wave per row.  Probabilities: four waves per workgroup, the waves past the row's count return.  No grid
// barrier, no floating-point atomics and, since the host parses the constraints, no atomic at all.
#pragma once
#include "sf_pf_long.hip.h"

#ifndef SF_PFLONGB_LANES_PER_CU
#ifdef SF_EMUL
#define SF_PFLONGB_LANES_PER_CU 256   // (the emulated device has two compute units and runs every lane as a fiber)
#else
#define SF_PFLONGB_LANES_PER_CU 8192  // lane budget of a diagonal launch over all rows: four times what a compute unit holds
#endif
#endif
#define SF_PFLONGB_THREADS 256

__global__ void sf_pflongb_inside_kernel(const SfPfLong *__restrict__ Fs, const uint8_t *__restrict__ act, int d, int bps, int lanes,
                                         const SfDevParams *__restrict__ D, const SfDevParamsPF *__restrict__ X) {
  const int s = (int)blockIdx.x / bps;
  if (!act[s]) return;
  const SfPfLong F = Fs[s];
  if (d >= F.L) return;
  const int G = pfl_group((size_t)(F.L - d), d, (size_t)lanes);
  const size_t first = (size_t)((int)blockIdx.x - s * bps) * blockDim.x;  // this workgroup's first lane within the row's share
  if (first / (size_t)G >= (size_t)(F.L - d)) return;                     // no cell of this row here (the same for the workgroup)
  sfp_inside(F, d, G, first + threadIdx.x, (size_t)bps * blockDim.x, D, X);
}

__global__ void sf_pflongb_exterior_kernel(const SfPfLong *__restrict__ Fs, const uint8_t *__restrict__ act,
                                           const SfDevParams *__restrict__ D, const SfDevParamsPF *__restrict__ X) {
  if (!act[blockIdx.x]) return;
  const SfPfLong F = Fs[blockIdx.x];
  sfpl_exterior(F, D, X);
}

__global__ void sf_pflongb_outside_kernel(const SfPfLong *__restrict__ Fs, const uint8_t *__restrict__ act, int d, int bps, int lanes,
                                          const SfDevParams *__restrict__ D, const SfDevParamsPF *__restrict__ X) {
  const int s = (int)blockIdx.x / bps;
  if (!act[s]) return;
  const SfPfLong F = Fs[s];
  if (d >= F.L) return;
  const int G = pfl_group((size_t)(F.L - d), d, (size_t)lanes);
  const size_t first = (size_t)((int)blockIdx.x - s * bps) * blockDim.x;
  if (first / (size_t)G >= (size_t)(F.L - d)) return;
  sfpl_outside(F, d, G, first + threadIdx.x, (size_t)bps * blockDim.x, D, X);
}

// bps workgroups of four waves per row; the row's waves are 0 .. pfl_prob_waves(L_s, lanes) - 1
__global__ void sf_pflongb_prob_kernel(const SfPfLong *__restrict__ Fs, const uint8_t *__restrict__ act, int bps, int lanes) {
  const int s = (int)blockIdx.x / bps;
  if (!act[s]) return;
  const SfPfLong F = Fs[s];
  const size_t nwaves = (size_t)pfl_prob_waves(F.L, (size_t)lanes);
  const size_t wave = (size_t)((int)blockIdx.x - s * bps) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave >= nwaves) return;  // (the same for the wave; sfp_prob has no workgroup barrier)
  sfp_prob(F, wave, nwaves);
}

__global__ void sf_pflongb_finish_kernel(const SfPfLong *__restrict__ Fs, const uint8_t *__restrict__ act, int lanes) {
  if (!act[blockIdx.x]) return;
  const SfPfLong F = Fs[blockIdx.x];
  sfp_finish(F, pfl_prob_waves(F.L, (size_t)lanes));
}
