// Host side of the MLP forwards, shared by mlp_fwd.hip (exact fp32) and mlp_fwd_bf.hip (bf16 / fp16 planes).  No device code.
#pragma once
#include "common.hpp"

// Where the points of a forward and their view directions come from, as the kernels take them: explicit points, or ray rows
// (origin, direction, near, far, [view direction] per row of `rs` floats) walked along the depths z.
struct CnFwdSrc {
  const float* pts;    // [M, 3] or nullptr
  const float* rays;   // [B, rs] or nullptr
  int rs;
  const float* dirs;   // [B, 3] or nullptr: the view directions are the last three columns of the ray rows
  const float* z;      // [B, S] (ray rows only)
  bool points_ok() const { return pts || (rays && z && rs >= 8); }
  // (asked of every plane forward, and of an fp32 forward whose network has a view branch)
  bool dirs_ok() const { return dirs || (rays && rs >= 11); }
};
