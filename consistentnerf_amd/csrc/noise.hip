// The Gaussian draws of the training step as own kernels: the density noise of raw2outputs (R:287-288, `raw_noise_std > 0`: every
// LLFF config) and the `--use_noise` label noise (V:1633-1638), from the standard-normal stream of rng.hpp.  Both levels of one
// render_rays call come from ONE launch (streams offset and offset + 1); the compositing kernels keep reading the noise as a
// tensor, so their forward and backward see the same numbers without regenerating them.
#include "rng.hpp"

namespace {
// one thread per element of [rows0, cols0] followed by [rows0, cols1] (n1 = 0: one level); consecutive threads store consecutive floats
__global__ void normal_rng_k(CnRngK rngk, int64_t n0, int cols0, int64_t n1, int cols1, float scale, float* __restrict__ out0,
                             float* __restrict__ out1) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n0 + n1) return;
  const int level = idx >= n0;
  if (level) idx -= n0;
  const int cols = level ? cols1 : cols0;
  const int64_t b = idx / cols;
  const float n = CnRngDev(rngk).normal(b, cols, (int)(idx - b * cols), (uint64_t)level);
  (level ? out1 : out0)[idx] = n * scale;
}
}  // namespace

extern "C" int cnerf_normal_rng(const cnerf_rng* rng, int64_t rows, int cols, float scale, float* out, void* stream) {
  if (!rng || !out || rows < 0 || cols <= 0) return CNERF_E_ARG;
  if (rows == 0) return CNERF_OK;
  hipLaunchKernelGGL(normal_rng_k, dim3((unsigned)cn_div_up(rows * cols, 256)), dim3(256), 0, cn_stream(stream), cn_rng_arg(rng),
                     rows * cols, cols, (int64_t)0, 1, scale, out, (float*)nullptr);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_density_noise_rng(const cnerf_rng* rng, int64_t B, int Nc, int S1, float std, float* noise0, float* noise1,
                                       void* stream) {
  if (!rng || !noise0 || B < 0 || Nc <= 0 || S1 < 0) return CNERF_E_ARG;
  if (B == 0) return CNERF_OK;
  const int64_t n0 = B * Nc, n1 = (noise1 && S1 > 0) ? B * S1 : 0;
  hipLaunchKernelGGL(normal_rng_k, dim3((unsigned)cn_div_up(n0 + n1, 256)), dim3(256), 0, cn_stream(stream), cn_rng_arg(rng), n0, Nc,
                     n1, n1 ? S1 : 1, std, noise0, noise1);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
