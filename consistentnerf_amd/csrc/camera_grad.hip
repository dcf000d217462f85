// NDC and intrinsics gradients: from a pixel to the finished ray row [o, d, near, far (, viewdirs)] of render()'s batch (H:164-173,
// R:103-116, H:186-202) in ONE launch, from poses and, optionally, a camera matrix K that stay in DEVICE memory — and the backward of
// that map w.r.t. the poses and K.  The forward is cn_raw_dir + cn_finish_ray of raygen.hpp (the one definition: the rows equal
// cnerf_gen_rays bit for bit); the backward of the finish is cn_finish_ray_bwd of camera_grad.hpp, which cnerf_ndc_rays_bwd applies
// on its own to rays the caller holds.  Compiled without FMA contraction like every file here.
//
// The backward is a reduction over the rays, shaped as gen_rays_at_bwd_k / gen_rays_at_reduce_k (rays_grad.hip).  No floating-point
// atomics, one summation order:
//   stage 1  one wave per CHUNK of 64 consecutive rays (a fixed size: the grid only decides which wave takes which chunk).  Per ray
//            the pixel direction, the pre-NDC ray and the warp are recomputed in fp64 from the fp32 inputs.  Per view the wave sums
//            its rays of that view with the xor butterfly and writes one record of 12 doubles at rec[chunk][view][12]; the four
//            intrinsics sums (fx, fy, cx, cy) are over all rays of the chunk, one record of 4 doubles at recK[chunk][4].
//   stage 2  one wave per view (+ one for K): lane l adds the records of chunks l, l + 64, ... in order, the 64 lane sums go through
//            the same butterfly, and the results are rounded to fp32 once.
// With K in device memory the two NDC coefficients are functions of K[0][0] (H:193-199 uses the focal length for both axes):
// a = -1 / (W / (2 f)) = -2 f / W, d a / d f = a / f, and their gradients flow into d_K[0][0].  With host intrinsics the
// coefficients are arguments of their own and d_K holds the derivative at fixed coefficients.
#include "camera_grad.hpp"

namespace {

constexpr int CG_CHUNK = 64;      // rays per stage-1 record = one wave
constexpr int CG_WAVES = 4;       // waves per stage-1 workgroup

struct CamPose {                  // what cn_raw_dir reads of a camera
  float fx, fy, cx, cy;
  float r[9];
};

struct CamIntr {                  // host intrinsics and coefficients; K != nullptr overrides them on the device
  float fx, fy, cx, cy, ax, ay;
  const float* K;
};

__device__ __forceinline__ void cg_pixel_of(const int64_t* __restrict__ coords, int64_t first, int W, int64_t b, int& j, int& i) {
  if (coords) {
    j = (int)coords[2 * b]; i = (int)coords[2 * b + 1];
  } else {
    const int64_t idx = first + b;
    j = (int)(idx / W); i = (int)(idx - (int64_t)j * W);
  }
}

__global__ void camera_rows_k(int H, int W, CamIntr in, const float* __restrict__ c2w, const int64_t* __restrict__ coords,
                              const int64_t* __restrict__ view, int64_t first, int64_t B, float near, float far, int vd, int ndc,
                              float* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  CamPose g;
  float ax = in.ax, ay = in.ay;
  if (in.K) {      // the coefficients in fp32 as the reference's tensor arithmetic forms them
    g.fx = in.K[0]; g.fy = in.K[4]; g.cx = in.K[2]; g.cy = in.K[5];
    ax = -1.f / ((float)W / (2.f * g.fx));
    ay = -1.f / ((float)H / (2.f * g.fx));
  } else {
    g.fx = in.fx; g.fy = in.fy; g.cx = in.cx; g.cy = in.cy;
  }
  int j, i;
  cg_pixel_of(coords, first, W, b, j, i);
  const float* p = c2w + (view ? view[b] : 0) * 12;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g.r[3 * r] = p[4 * r]; g.r[3 * r + 1] = p[4 * r + 1]; g.r[3 * r + 2] = p[4 * r + 2];
  }
  float dx, dy, dz, o[3], d[3], v[3];
  cn_raw_dir(g, j, i, dx, dy, dz);
  cn_finish_ray(p[3], p[7], p[11], dx, dy, dz, vd, ndc, ax, ay, o, d, v);
  float* out = rows + b * (vd ? 11 : 8);
  out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = d[0]; out[4] = d[1]; out[5] = d[2]; out[6] = near; out[7] = far;
  if (vd) { out[8] = v[0]; out[9] = v[1]; out[10] = v[2]; }
}

// the first N of a wave's sums, each to lane k: lane k < N returns sum k, the other lanes 0
template <int N>
__device__ __forceinline__ double cg_sums_to_lanes(const double (&t)[N], bool mine, int lane) {
  double keep = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double x = wave_sum(mine ? t[k] : 0.0);
    if (lane == k) keep = x;
  }
  return keep;
}

__global__ __launch_bounds__(CG_CHUNK* CG_WAVES) void camera_rows_bwd_k(int H, int W, CamIntr in, const float* __restrict__ c2w,
                                                                        const int64_t* __restrict__ coords,
                                                                        const int64_t* __restrict__ view, int64_t first, int64_t B,
                                                                        int n_views, int vd, int ndc, const float* __restrict__ g,
                                                                        int64_t n_chunks, double* __restrict__ rec,
                                                                        double* __restrict__ recK) {
  const int lane = threadIdx.x & 63;
  const int gs = vd ? 11 : 8;
  double fx, fy, cx, cy, ax, ay;
  if (in.K) {
    fx = (double)in.K[0]; fy = (double)in.K[4]; cx = (double)in.K[2]; cy = (double)in.K[5];
    ax = -1.0 / ((double)W / (2.0 * fx)); ay = -1.0 / ((double)H / (2.0 * fx));
  } else {
    fx = (double)in.fx; fy = (double)in.fy; cx = (double)in.cx; cy = (double)in.cy; ax = (double)in.ax; ay = (double)in.ay;
  }
  const int64_t nwaves = (int64_t)gridDim.x * CG_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * CG_WAVES + (threadIdx.x >> 6); c < n_chunks; c += nwaves) {   // (wave-uniform)
    const int64_t b = c * CG_CHUNK + lane;
    int64_t v = b < B ? (view ? view[b] : 0) : -1;
    const bool live = v >= 0 && v < n_views;      // (a view value outside [0, n_views) contributes nowhere and reads nothing)
    double t[12], k[4];
#pragma unroll
    for (int q = 0; q < 12; ++q) t[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) k[q] = 0.0;
    if (live) {
      int j, i;
      cg_pixel_of(coords, first, W, b, j, i);
      const float* p = c2w + v * 12;
      const float* gr = g + b * gs;
      const double dir[3] = {((double)i - cx) / fx, -((double)j - cy) / fy, -1.0};      // H:167
      double R[9], o[3], d[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        R[3 * r] = (double)p[4 * r]; R[3 * r + 1] = (double)p[4 * r + 1]; R[3 * r + 2] = (double)p[4 * r + 2];
        o[r] = (double)p[4 * r + 3];                                                     // H:172
        d[r] = dir[0] * R[3 * r] + dir[1] * R[3 * r + 1] + dir[2] * R[3 * r + 2];       // H:170
      }
      const double g_o[3] = {(double)gr[0], (double)gr[1], (double)gr[2]}, g_d[3] = {(double)gr[3], (double)gr[4], (double)gr[5]};
      const double g_v[3] = {vd ? (double)gr[8] : 0.0, vd ? (double)gr[9] : 0.0, vd ? (double)gr[10] : 0.0};
      const CnRayGrad y = cn_finish_ray_bwd(o, d, vd, ndc, ax, ay, g_o, g_d, g_v);
      double g_dir[2] = {0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        t[4 * r] = y.d[r] * dir[0]; t[4 * r + 1] = y.d[r] * dir[1]; t[4 * r + 2] = y.d[r] * dir[2];
        t[4 * r + 3] = y.o[r];
        g_dir[0] += R[3 * r] * y.d[r]; g_dir[1] += R[3 * r + 1] * y.d[r];
      }
      // dir_x = (i - cx) / fx, dir_y = -(j - cy) / fy
      k[0] = -g_dir[0] * dir[0] / fx; k[1] = -g_dir[1] * dir[1] / fy; k[2] = -g_dir[0] / fx; k[3] = g_dir[1] / fy;
      if (in.K && ndc) k[0] += (y.ax * ax + y.ay * ay) / fx;      // d a / d f = a / f for both coefficients
    }
    if (rec) {
      for (int q = 0; q < n_views; ++q) {
        const bool mine = live && v == q;
        double keep = 0.0;
        if (__ballot(mine) != 0) keep = cg_sums_to_lanes(t, mine, lane);      // (wave-uniform)
        if (lane < 12) rec[(c * n_views + q) * 12 + lane] = keep;
      }
    }
    if (recK) {
      const double keep = cg_sums_to_lanes(k, live, lane);
      if (lane < 4) recK[c * 4 + lane] = keep;
    }
  }
}

// block q < n_views: d_c2w[q] (when rec); block n_views: d_K (when recK)
__global__ __launch_bounds__(64) void camera_rows_reduce_k(const double* __restrict__ rec, const double* __restrict__ recK,
                                                           int64_t n_chunks, int n_views, float* __restrict__ d_c2w,
                                                           float* __restrict__ d_K) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q < n_views) {
    if (!rec) return;
    double s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0.0;
    for (int64_t c = lane; c < n_chunks; c += 64) {
      const double* r = rec + (c * n_views + q) * 12;
#pragma unroll
      for (int k = 0; k < 12; ++k) s[k] += r[k];
    }
    const double keep = cg_sums_to_lanes(s, true, lane);
    if (lane < 12) d_c2w[(int64_t)q * 12 + lane] = (float)keep;
    return;
  }
  if (!recK) return;
  double s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = 0.0;
  for (int64_t c = lane; c < n_chunks; c += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += recK[c * 4 + k];
  }
  const double keep = cg_sums_to_lanes(s, true, lane);
  // K[0][0] = fx, K[1][1] = fy, K[0][2] = cx, K[1][2] = cy: the four entries read; the other five get zeros (lane 63 holds one)
  const int src = lane == 0 ? 0 : lane == 4 ? 1 : lane == 2 ? 2 : lane == 5 ? 3 : 63;
  const double val = __shfl(keep, src, 64);
  if (lane < 9) d_K[lane] = (float)val;
}

__global__ void ndc_rays_bwd_k(const float* __restrict__ g_o, const float* __restrict__ g_d, const float* __restrict__ ro,
                               const float* __restrict__ rd, int64_t B, float ax, float ay, float* __restrict__ d_o,
                               float* __restrict__ d_d) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double o[3] = {(double)ro[3 * b], (double)ro[3 * b + 1], (double)ro[3 * b + 2]};
  const double d[3] = {(double)rd[3 * b], (double)rd[3 * b + 1], (double)rd[3 * b + 2]};
  const double go[3] = {(double)g_o[3 * b], (double)g_o[3 * b + 1], (double)g_o[3 * b + 2]};
  const double gd[3] = {(double)g_d[3 * b], (double)g_d[3 * b + 1], (double)g_d[3 * b + 2]};
  const double none[3] = {0.0, 0.0, 0.0};
  const CnRayGrad y = cn_finish_ray_bwd(o, d, 0, 1, (double)ax, (double)ay, go, gd, none);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d_o[3 * b + k] = (float)y.o[k];
    d_d[3 * b + k] = (float)y.d[k];
  }
}

inline bool camera_args_ok(int H, int W, float fx, float fy, const float* K, const float* c2w, int n_views, const int64_t* coords,
                           int64_t first, int64_t B) {
  if (H <= 0 || W <= 0 || n_views <= 0 || B <= 0 || !c2w) return false;
  if (!K && (!(fx != 0.f) || !(fy != 0.f))) return false;                // (a device K is not read here: no synchronisation)
  return coords || (first >= 0 && first <= (int64_t)H * W - B);      // the row-major window lies inside the image
}

}  // namespace

extern "C" int cnerf_camera_rows(int H, int W, float fx, float fy, float cx, float cy, float ndc_ax, float ndc_ay, const float* K,
                                 const float* c2w, int n_views, const int64_t* coords, const int64_t* view, int64_t first, int64_t B,
                                 float near, float far, int use_viewdirs, int ndc, float* rows, void* stream) {
  if (!rows || !camera_args_ok(H, W, fx, fy, K, c2w, n_views, coords, first, B)) return CNERF_E_ARG;
  const CamIntr in = {fx, fy, cx, cy, ndc_ax, ndc_ay, K};
  hipLaunchKernelGGL(camera_rows_k, dim3((unsigned)cn_div_up(B, 256)), dim3(256), 0, cn_stream(stream), H, W, in, c2w, coords, view,
                     first, B, near, far, use_viewdirs ? 1 : 0, ndc ? 1 : 0, rows);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int64_t cnerf_camera_rows_bwd_ws_floats(int64_t B, int n_views) {
  if (B <= 0 || n_views <= 0) return 0;
  return 2 * (12 * (int64_t)n_views + 4) * cn_div_up(B, CG_CHUNK);      // [chunks][n_views][12] + [chunks][4] doubles
}

extern "C" int cnerf_camera_rows_bwd(int H, int W, float fx, float fy, float cx, float cy, float ndc_ax, float ndc_ay, const float* K,
                                     const float* c2w, int n_views, const int64_t* coords, const int64_t* view, int64_t first,
                                     int64_t B, int use_viewdirs, int ndc, const float* g, float* d_c2w, float* d_K, float* workspace,
                                     int grid, void* stream) {
  if (!g || (!d_c2w && !d_K) || !workspace || ((uintptr_t)workspace & 7) || grid < 0 ||
      !camera_args_ok(H, W, fx, fy, K, c2w, n_views, coords, first, B))
    return CNERF_E_ARG;
  const int64_t n_chunks = cn_div_up(B, CG_CHUNK);
  const int64_t blocks = grid > 0 ? grid : (cn_div_up(n_chunks, CG_WAVES) < 1024 ? cn_div_up(n_chunks, CG_WAVES) : 1024);
  double* ws = reinterpret_cast<double*>(workspace);
  double* rec = d_c2w ? ws : nullptr;
  double* recK = d_K ? ws + n_chunks * n_views * 12 : nullptr;
  const CamIntr in = {fx, fy, cx, cy, ndc_ax, ndc_ay, K};
  hipLaunchKernelGGL(camera_rows_bwd_k, dim3((unsigned)blocks), dim3(CG_CHUNK * CG_WAVES), 0, cn_stream(stream), H, W, in, c2w, coords,
                     view, first, B, n_views, use_viewdirs ? 1 : 0, ndc ? 1 : 0, g, n_chunks, rec, recK);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(camera_rows_reduce_k, dim3((unsigned)n_views + 1), dim3(64), 0, cn_stream(stream), rec, recK, n_chunks, n_views,
                     d_c2w, d_K);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}

extern "C" int cnerf_ndc_rays_bwd(const float* g_o, const float* g_d, const float* rays_o, const float* rays_d, int64_t B,
                                  float ndc_ax, float ndc_ay, float* d_rays_o, float* d_rays_d, void* stream) {
  if (!g_o || !g_d || !rays_o || !rays_d || !d_rays_o || !d_rays_d || B <= 0) return CNERF_E_ARG;
  hipLaunchKernelGGL(ndc_rays_bwd_k, dim3((unsigned)cn_div_up(B, 256)), dim3(256), 0, cn_stream(stream), g_o, g_d, rays_o, rays_d, B,
                     ndc_ax, ndc_ay, d_rays_o, d_rays_d);
  CN_CHECK_LAUNCH();
  return CNERF_OK;
}
