// Host side of the MLP backward, shared by mlp_bwd.hip (the entry points and the exact-fp32 dgrad), mlp_bwd_bf.hip (the bf16x3
// dgrad) and wgrad.hip (the weight gradients).  No device code.
#pragma once
#include "common.hpp"

// One network of a backward launch, with its operands as the kernels take them: first_ray is already applied (mlp_bwd.hip,
// operands(): the one place that does it), so every field below speaks of the LAUNCHED rays only.
struct CnBwdNet {
  NetGeom g;
  const void* packed;        // dgrad: the fp32 buffer (cnerf_pack_weights) or the bf16x3 bytes (cnerf_pack_weights_bf, 3 planes)
  const float* d_raw;        // dgrad
  const float* stash;
  float* G;                  // gradient workspace [Mp][g_rows]: dgrad writes it, wgrad reads it
  int64_t M, Mp;             // points, and rounded up to the 32-point tile
  float* partials;           // wgrad: the split partials behind G ...
  int cap;                   // ... and their capacity in slices (cn_wgrad_nsplit)
  const cnerf_ptrs* grads;   // wgrad
  int live_mul, live_sub;    // launches that stop at a device-side count of live rays: points per ray (else 0), rays left out in front
};

int cn_wgrad_nsplit(int64_t Mp);
int64_t cn_param_floats(const NetGeom& g);
// Weight gradients of nets[0, n), n = 1 or 2, in one grid + one reduction.  `live`: device count of live rays or nullptr.
int cn_wgrad_launch(const CnBwdNet* nets, int n, int accumulate, hipStream_t st, int bf3, const int* live);
// The bf16x3 dgrad: its architecture envelope, and nets[0, n) of ONE architecture in one grid.
int cn_dgrad_bf3_supported(const NetGeom& g);
int cn_dgrad_bf3(const CnBwdNet* nets, int n, hipStream_t st);
