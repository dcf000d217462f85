// Counter-based uniform streams for the two torch.rand draws of render_rays — the stratified jitter t_rand (R:376) and the
// resampling positions u (H:227) — generated INSIDE coarse_z_k / resample_k instead of by a generator launch whose output
// round-trips HBM.  Philox4x32-10 (Salmon et al., SC'11; the generator behind torch's CUDA streams as well), one block per
// element: key = seed ^ a fixed constant (a stream disjoint from every torch.rand call on the same seed), counter =
// (element index [64 bits], stream offset [64 bits]) with element = (row0 + ray) * cols + col — the index of the value in the
// GLOBAL [total_rays, cols] draw, so a shard of a batch (row0 = its first global row) sees exactly the rows the unsharded call
// sees, for free.  value = (x0 >> 8) * 2^-24: the 24-bit grid on [0, 1) of ATen's CPU torch.rand for float32.
// oracle/philox.py restates this in numpy (pinned on the Random123 known-answer vectors); tests compare bit for bit.
//
// Next to it, a standard-normal stream for the density noise of raw2outputs (R:287-288) and the `--use_noise` label noise
// (V:1633-1638): CnRngDev::normal(row, cols, col) — the same element index e = (row0 + row) * cols + col, the same key
// seed ^ "cnerf_rn", the stream offset in the counter's high half exactly as above — takes words x0 and x1 of that ONE block:
// u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1] (exact in fp32), u2 = (x1 >> 8) * 2^-24 in [0, 1), n = sqrtf(-2 logf(u1)) * cospif(2 u2)
// (Box-Muller; the accurate OCML logf / sqrtf / cospif, no fast forms: the build has no fast-math and -ffp-contract=off).  One block
// per element wastes the sine half of the pair ON PURPOSE: a value then depends on nothing but its own global index, so shards,
// odd column counts and the two levels of a render_rays call need no pairing rule (at B = 4096, 64 + 192 samples the whole draw is
// 2^20 blocks).  |n| <= sqrt(48 ln 2) = 5.7681 (u1 >= 2^-24), never inf or NaN.  A uniform and a normal stream on the same offset
// share x0: callers give each stream an offset of its own (ops.rng_draw).  tests/_noise_ref.py restates it in float64.
#pragma once
#include "common.hpp"

struct CnRngK {
  uint64_t seed, offset;
  const uint64_t* dev;   // non-null: {seed, base offset} live in device memory (hipGraph replays); `offset` is added to the base
  int64_t row0;
};

static inline CnRngK cn_rng_arg(const cnerf_rng* r) {
  CnRngK k;
  k.seed = r->seed; k.offset = r->offset; k.dev = r->state_dev; k.row0 = r->row0;
  return k;
}

// words 0 and 1 of the Philox4x32-10 block of (counter, key)
__device__ __forceinline__ uint2 cn_philox_x01(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint2(c0, c1);
}

__device__ __forceinline__ uint32_t cn_philox_x0(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
  return cn_philox_x01(ctr_lo, ctr_hi, key).x;
}

struct CnRngDev {
  uint64_t key, off;
  int64_t row0;
  __device__ __forceinline__ explicit CnRngDev(const CnRngK& r) {
    const uint64_t seed = r.dev ? r.dev[0] : r.seed;
    key = seed ^ 0x636e6572665f726eull;               // "cnerf_rn"
    off = r.offset + (r.dev ? r.dev[1] : 0ull);
    row0 = r.row0;
  }
  __device__ __forceinline__ float uniform(int64_t row, int cols, int col) const {
    const uint64_t e = (uint64_t)(row0 + row) * (uint64_t)cols + (uint64_t)col;
    return (float)(cn_philox_x0(e, off, key) >> 8) * 5.9604644775390625e-8f;
  }
  // stream `off + add` (cnerf_density_noise_rng: the second level's stream in the same launch)
  __device__ __forceinline__ float normal(int64_t row, int cols, int col, uint64_t add = 0) const {
    const uint64_t e = (uint64_t)(row0 + row) * (uint64_t)cols + (uint64_t)col;
    const uint2 x = cn_philox_x01(e, off + add, key);
    const float u1 = (float)((x.x >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(x.y >> 8) * 5.9604644775390625e-8f;
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
  }
};
