// Does v_mfma_f32_32x32x16_f16 honour SUBNORMAL fp16 operands on gfx950, or flush them?  A = one fp16 bit pattern in every
// element, B = 1024: an output element is 16 A 1024.  A = 0x0010 (2^-20, subnormal) gives 2^-6 = 0.015625 if subnormal inputs count
// and 0 if the matrix pipe flushes them; A = 0x0400 (2^-14, the smallest normal) is the control (1.0).  The fp16x2 forward is
// correct either way (its operands are scaled past the question, csrc/mlp_fwd_bf.hip); this only says how much margin that buys.
//   hipcc --offload-arch=gfx950 -O2 scripts/mfma_f16_subnormal_probe.hip -o scripts/mfma_f16_subnormal_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(64) void probe(float* out, unsigned short abits, unsigned short bbits) {
  f16x8 a, b;
  for (int i = 0; i < 8; ++i) { a[i] = __builtin_bit_cast(_Float16, abits); b[i] = __builtin_bit_cast(_Float16, bbits); }
  f32x16 c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  out[threadIdx.x] = c[0];
}
int main() {
  float* d; float h[64];
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) { printf("no device\n"); return 1; }
  const unsigned short A[3] = {0x0010, 0x0001, 0x0400}; const char* what[3] = {"2^-20 (subnormal)", "2^-24 (smallest subnormal)", "2^-14 (smallest normal)"};
  for (int k = 0; k < 3; ++k) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, A[k], (unsigned short)0x6400);      // B = 1024
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 1; }
    const double want = 16.0 * 1024.0 * (k == 0 ? 0x1p-20 : k == 1 ? 0x1p-24 : 0x1p-14);
    printf("A = %-27s as A operand: got %.9g, exact %.9g -> %s\n", what[k], h[0], want, h[0] == (float)want ? "counted" : h[0] == 0.f ? "FLUSHED" : "other");
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, (unsigned short)0x6400, A[k]);      // the same value as the B operand
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 1; }
    printf("A = %-27s as B operand: got %.9g, exact %.9g -> %s\n", what[k], h[0], want, h[0] == (float)want ? "counted" : h[0] == 0.f ? "FLUSHED" : "other");
  }
  (void)hipFree(d);
  return 0;
}
