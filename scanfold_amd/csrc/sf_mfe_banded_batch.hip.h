// sf_mfe_banded_batch.hip.h — the three kernels of sf_mfe_banded.hip.h for MANY sequences of 1 <= L <= SF_MAX_BANDED at once
// (sf_fold_banded_batch): a record and its shuffles under a base-pair span S, the z-score of a whole genome.  One fold per
// call leaves the device idle twice over: the exterior loop f5 is sequential in j and runs in one workgroup, and a diagonal
// of a record of a few thousand nucleotides has L - d cells of at most 64 lanes each.
//
// State: a device array of SfBand, one per sequence of the chunk; its tables are slices of a few allocations the host makes
// per chunk.  Cell body and f5 are sf_mfe_banded.hip.h's own functions (sfb_fill_cell, sfb_f5), the traceback is
// sf_mfe_trace.hip.h's sft_trace as sf_fold_banded instantiates it, so energies and structures are sf_fold_banded's, byte
// for byte.
//
// Each sequence has its own band B_s = min(S, L_s).  Fill: one launch per diagonal d = 0 .. max_s B_s - 1 covers every
// sequence.  The grid stays one-dimensional: with bps = ceil((Lmax - d) G / 256) workgroups per sequence, workgroup b works on
// sequence b / bps, so every lane of a wave belongs to the same sequence and the butterfly of a cell's group stays inside it.
// A workgroup leaves before any shuffle when its sequence has d >= B_s (the sequence is absent from this launch) or when its
// first cell lies past L_s - d; in the last workgroup of a sequence the lanes past L_s - d take part in the butterfly without
// a cell, as in sf_band_fill_kernel.  G is the same for every sequence of a launch.  All arithmetic is an integer minimum:
// results do not depend on G, on the chunking or on the order of the sequences.
// f5 and traceback: one workgroup per sequence.  No grid barrier; the only atomic is the shared status word.
#pragma once
#include "sf_mfe_banded.hip.h"

#define SF_BANDB_THREADS 256

__global__ void sf_bandb_fill_kernel(const SfBand *__restrict__ Fs, int d, int G, int bps, const SfDevParams *__restrict__ D) {
  const int s = (int)blockIdx.x / bps;
  const SfBand F = Fs[s];
  const size_t first = (size_t)((int)blockIdx.x - s * bps) * blockDim.x;  // this workgroup's first lane within the sequence
  if (d >= F.B || first / (size_t)G >= (size_t)(F.L - d)) return;         // no cell of this sequence here (the same for the workgroup)
  const size_t gt = first + threadIdx.x;
  sfb_fill_cell(F, d, G, (int)(gt % (size_t)G), gt / (size_t)G, D);
}

__global__ void sf_bandb_f5_kernel(const SfBand *__restrict__ Fs, const SfDevParams *__restrict__ D, int32_t *mfe_out) {
  const SfBand F = Fs[blockIdx.x];
  sfb_f5(F, D, mfe_out + blockIdx.x);
}

__global__ void sf_bandb_trace_kernel(const SfBand *__restrict__ Fs, const SfDevParams *__restrict__ D) {
  const SfBand F = Fs[blockIdx.x];
  sft_trace(F, D);
}
