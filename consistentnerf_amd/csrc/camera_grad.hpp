// The backward of cn_finish_ray (raygen.hpp): from the gradient of a finished ray row — o, d after the optional NDC warp and the
// view direction of the PRE-NDC ray — to the gradient of the pre-NDC ray (ox, oy, oz, dx, dy, dz) and of the two NDC coefficients.
// The one definition for cnerf_camera_rows_bwd and cnerf_ndc_rays_bwd (camera_grad.hip).  Evaluated in fp64 at the fp32 inputs: the
// forward's intermediates are recomputed, not read, and a result is rounded to fp32 once by its consumer.
//
// Forward (H:188-202, near plane 1), with p = o + t d, t = -(1 + oz) / dz:
//   o' = (ax px / pz, ay py / pz, 1 + 2 / pz)        d' = (ax (dx / dz - px / pz), ay (dy / dz - py / pz), -2 / pz)
// pz = oz + t dz is -1 identically in (o, d): its total derivative w.r.t. every input is zero (d pz / d oz = 1 + dz dt / d oz = 0,
// d pz / d dz = t + dz dt / d dz = 0), so o'_z = 1 + 2 / pz and d'_z = -2 / pz are constants and pz is a constant wherever it divides.
// The derivative is written SIMPLIFIED: no term goes back through pz, and the row gradients of o'_z and d'_z are not read.  (The
// expanded form adds terms that cancel to round-off; float64 autograd of the written formula agrees with either to 1e-16.)
#pragma once
#include "raygen.hpp"

struct CnRayGrad {
  double o[3], d[3];      // gradient of the pre-NDC origin and direction
  double ax, ay;          // gradient of the two coefficients (0 without ndc)
};

// o, d: the pre-NDC ray; g_o, g_d: gradient of the row's o and d columns; g_v: of its view direction (read only when vd)
__device__ __forceinline__ CnRayGrad cn_finish_ray_bwd(const double (&o)[3], const double (&d)[3], int vd, int ndc, double ax,
                                                       double ay, const double (&g_o)[3], const double (&g_d)[3],
                                                       const double (&g_v)[3]) {
  CnRayGrad r;
  r.ax = r.ay = 0.0;
  if (ndc) {
    const double t = -(1.0 + o[2]) / d[2];
    const double px = o[0] + t * d[0], py = o[1] + t * d[1], pz = o[2] + t * d[2];
    const double qx = px / pz, qy = py / pz;                                // o'_x = ax qx, d'_x = ax (dx / dz - qx)
    r.ax = g_o[0] * qx + g_d[0] * (d[0] / d[2] - qx);
    r.ay = g_o[1] * qy + g_d[1] * (d[1] / d[2] - qy);
    const double g_px = ax * (g_o[0] - g_d[0]) / pz, g_py = ay * (g_o[1] - g_d[1]) / pz;
    const double g_t = g_px * d[0] + g_py * d[1];                           // through px, py only (pz is constant)
    r.o[0] = g_px; r.o[1] = g_py; r.o[2] = -g_t / d[2];                     // d t / d oz = -1 / dz
    r.d[0] = g_px * t + g_d[0] * ax / d[2];
    r.d[1] = g_py * t + g_d[1] * ay / d[2];
    // d t / d dz = (1 + oz) / dz^2 = -t / dz
    r.d[2] = -g_t * t / d[2] - (g_d[0] * ax * d[0] + g_d[1] * ay * d[1]) / (d[2] * d[2]);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.o[k] = g_o[k]; r.d[k] = g_d[k]; }
  }
  if (vd) {   // v = d / |d| of the pre-NDC direction, as pack_rays_bwd_k: (g_v - v (v . g_v)) / |d|
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double v[3] = {d[0] / n, d[1] / n, d[2] / n};
    const double dot = v[0] * g_v[0] + v[1] * g_v[1] + v[2] * g_v[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) r.d[k] += (g_v[k] - v[k] * dot) / n;
  }
  return r;
}
