// sf_mfe_long_batch.hip.h — the three kernels of sf_mfe_long.hip.h for MANY sequences of 1 <= L <= SF_MAX_LONG at once
// (sf_fold_long_batch): energies([native] + shuffles) on a record past the window limit, where one fold per call leaves the
// device idle — a diagonal of a 1 000-nt fold has at most 1 000 x G lanes of work.
//
// State: a device array of SfLong, one per sequence of the chunk; its tables are slices of a few allocations the host makes
// per chunk.  Cell body and f5 are sf_mfe_long.hip.h's own functions (sfl_fill_cell, sfl_f5), the traceback is
// sf_mfe_trace.hip.h's sft_trace as sf_fold_long instantiates it, so energies and structures are sf_fold_long's, byte for byte.
//
// Fill: one launch per diagonal d = 0 .. Lmax - 1 covers every sequence.  The grid stays one-dimensional: with
// bps = ceil((Lmax - d) G / 256) workgroups per sequence, workgroup b works on sequence b / bps, so every lane of a wave
// belongs to the same sequence and the butterfly of a cell's group stays inside it.  A workgroup whose cells all lie past
// L_s - d (a shorter sequence, or one shorter than d) leaves at once; in the last workgroup of a sequence the lanes past
// L_s - d take part in the butterfly without a cell, as in sf_long_fill_kernel.  G is the same for every sequence of a launch.
// All arithmetic is an integer minimum: results do not depend on G, on the chunking or on the order of the sequences.
// f5 and traceback: one workgroup per sequence.  No grid barrier; the only atomic is the shared status word.
#pragma once
#include "sf_mfe_long.hip.h"

#ifdef SF_EMUL
#define SF_LONGB_LANES_PER_CU 512   // (the emulated device has two compute units and runs every lane as a fiber)
#else
#define SF_LONGB_LANES_PER_CU 8192  // lane budget of a diagonal launch: four times what a compute unit holds at once
#endif
#define SF_LONGB_THREADS 256

__global__ void sf_longb_fill_kernel(const SfLong *__restrict__ Fs, int d, int G, int bps, const SfDevParams *__restrict__ D) {
  const int s = (int)blockIdx.x / bps;
  const SfLong F = Fs[s];
  const size_t first = (size_t)((int)blockIdx.x - s * bps) * blockDim.x;  // this workgroup's first lane within the sequence
  if (d >= F.L || first / (size_t)G >= (size_t)(F.L - d)) return;         // no cell of this sequence here (the same for the workgroup)
  const size_t gt = first + threadIdx.x;
  sfl_fill_cell(F, d, G, (int)(gt % (size_t)G), gt / (size_t)G, D);
}

__global__ void sf_longb_f5_kernel(const SfLong *__restrict__ Fs, const SfDevParams *__restrict__ D, int32_t *mfe_out) {
  const SfLong F = Fs[blockIdx.x];
  sfl_f5(F, D, mfe_out + blockIdx.x);
}

__global__ void sf_longb_trace_kernel(const SfLong *__restrict__ Fs, const SfDevParams *__restrict__ D) {
  const SfLong F = Fs[blockIdx.x];
  sft_trace(F, D);
}
