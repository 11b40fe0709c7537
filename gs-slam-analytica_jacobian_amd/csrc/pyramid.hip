// pyramid.hip -- what coarse-to-fine Gauss-Newton tracking needs on the device (include/gsaj.h "image pyramid"):
//   k_pyramid      levels 1..L (L <= 4) of a frame's colour, depth and mask in ONE launch: every level-0 element is read once, every
//                  level element written once, no atomics -- the bits are the same run to run
//   k_gn_relevel   one Levenberg-Marquardt state (pose_jac.hip's gn_state / gn8_state) carried to the next resolution: one wave,
//                  no host read
// Compiled without FMA contraction: tests/pyramid_restated.py restates the pyramid one fp32 rounding at a time.
#include "gsaj_common.h"
#include "gn_state.h"

// ---- the packed pyramid: levels 1..L one after the other, each colour [3,H_l,W_l], depth [H_l,W_l], mask [H_l,W_l], every plane
// at a 256-byte aligned offset (bytes between planes are never written) ----------------------------------------------------------
#define PYR_NONE (~(size_t)0)   // the offset of a plane the pyramid does not have
struct PyrLevel {
  int W, H;
  size_t color, depth, mask;
};
struct PyrLayout {
  PyrLevel lv[GSAJ_PYRAMID_MAX_LEVELS];   // lv[l - 1]: level l
  size_t bytes;
};

static bool pyr_layout(int W, int H, int levels, int has_depth, int has_mask, PyrLayout *out) {
  if (levels < 1 || levels > GSAJ_PYRAMID_MAX_LEVELS || W < 1 || H < 1 || (W >> levels) < 1 || (H >> levels) < 1) return false;
  size_t off = 0;
  for (int l = 1; l <= levels; l++) {
    PyrLevel &v = out->lv[l - 1];
    v.W = W >> l;
    v.H = H >> l;
    const size_t n = (size_t)v.W * v.H;
    v.color = off;
    off += gsaj_align(3 * sizeof(float) * n);
    v.depth = has_depth ? off : PYR_NONE;
    if (has_depth) off += gsaj_align(sizeof(float) * n);
    v.mask = has_mask ? off : PYR_NONE;
    if (has_mask) off += gsaj_align(n);
  }
  for (int l = levels; l < GSAJ_PYRAMID_MAX_LEVELS; l++) out->lv[l] = PyrLevel{0, 0, PYR_NONE, PYR_NONE, PYR_NONE};
  out->bytes = off;
  return true;
}

struct PyrParams {
  int W, H, levels;
  const float *color, *depth;   // level 0; depth may be NULL
  const uint8_t *mask;          // may be NULL
  float edge_ratio;
  char *out;
  int vec;                      // the two pixels of a row pair are one aligned 8-byte (mask: 2-byte) load
  PyrLevel lv[GSAJ_PYRAMID_MAX_LEVELS];
};

// depth of a pixel from its four children in the order p00, p01, p10, p11: the mean of the valid ones (d > 0), 0 if there is none or
// if they straddle a depth discontinuity (dmax - dmin > ratio dmin); the division by n is a multiplication by r[n]
__device__ __forceinline__ float pyr_depth(float d0, float d1, float d2, float d3, float ratio) {
  const float d[4] = {d0, d1, d2, d3};
  float s = 0.f, dmin = 0.f, dmax = 0.f;
  int n = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (d[i] > 0.f) {
      s = n ? s + d[i] : d[i];
      dmin = n ? fminf(dmin, d[i]) : d[i];
      dmax = n ? fmaxf(dmax, d[i]) : d[i];
      n++;
    }
  }
  if (n == 0) return 0.f;
  if (dmax - dmin > ratio * dmin) return 0.f;
  const float r = n == 1 ? 1.f : n == 2 ? 0.5f : n == 3 ? (float)(1.0 / 3.0) : 0.25f;
  return s * r;
}

__device__ __forceinline__ float pyr_color(float p00, float p01, float p10, float p11) { return 0.25f * ((p00 + p01) + (p10 + p11)); }

// bits 0, 2, 4, 6 of t
__device__ __forceinline__ int pyr_even_bits(int t) { return (t & 1) | ((t >> 1) & 2) | ((t >> 2) & 4) | ((t >> 3) & 8); }

// One workgroup: a 32 x 32 block of level 0 = 16 x 16 of level 1, one thread per level-1 pixel.  The threads own the 16 x 16 tile in
// Morton order (x in the even bits of threadIdx.x, y in the odd ones), so the four children of a level l + 1 pixel sit in lanes
// base + {0, 1, 2, 3} 4^(l-1) of ONE wave, in row-major order, and each further level is four lane reads per plane -- no LDS, no
// barrier; a wave is an 8 x 8 block of level 1, which is one pixel of level 4.  A pixel exists only if its whole block of level 0
// lies inside the image, so an existing pixel never reads a lane that loaded nothing.
__global__ __launch_bounds__(256) void k_pyramid(PyrParams p) {
  const int t = threadIdx.x, lane = t & 63;
  const int x1 = blockIdx.x * 16 + pyr_even_bits(t), y1 = blockIdx.y * 16 + pyr_even_bits(t >> 1);
  const bool has_d = p.depth != nullptr, has_m = p.mask != nullptr;
  float c[3] = {0.f, 0.f, 0.f}, d = 0.f;
  uint32_t m = 0u;
  if (x1 < p.lv[0].W && y1 < p.lv[0].H) {
    const size_t N = (size_t)p.W * p.H, r0 = (size_t)(2 * y1) * p.W + 2 * x1, r1 = r0 + p.W;
    float2 a, b;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float *src = p.color + ch * N;
      if (p.vec) {
        a = *reinterpret_cast<const float2 *>(src + r0);
        b = *reinterpret_cast<const float2 *>(src + r1);
      } else {
        a = make_float2(src[r0], src[r0 + 1]);
        b = make_float2(src[r1], src[r1 + 1]);
      }
      c[ch] = pyr_color(a.x, a.y, b.x, b.y);
    }
    if (has_d) {
      if (p.vec) {
        a = *reinterpret_cast<const float2 *>(p.depth + r0);
        b = *reinterpret_cast<const float2 *>(p.depth + r1);
      } else {
        a = make_float2(p.depth[r0], p.depth[r0 + 1]);
        b = make_float2(p.depth[r1], p.depth[r1 + 1]);
      }
      d = pyr_depth(a.x, a.y, b.x, b.y, p.edge_ratio);
    }
    if (has_m) {
      if (p.vec)
        m = (uint32_t)(*reinterpret_cast<const uint16_t *>(p.mask + r0)) | (uint32_t)(*reinterpret_cast<const uint16_t *>(p.mask + r1));
      else
        m = (uint32_t)p.mask[r0] | p.mask[r0 + 1] | p.mask[r1] | p.mask[r1 + 1];
      m = m ? 1u : 0u;
    }
  }
  int xl = x1, yl = y1;
#pragma unroll
  for (int l = 1; l <= GSAJ_PYRAMID_MAX_LEVELS; l++) {
    if (l > p.levels) break;   // (wave-uniform)
    const PyrLevel lv = p.lv[l - 1];
    const int stride = 1 << (2 * (l - 1));   // lanes between the pixels of level l: 1, 4, 16, 64
    if ((lane & (stride - 1)) == 0 && xl < lv.W && yl < lv.H) {
      const size_t n = (size_t)lv.W * lv.H, at = (size_t)yl * lv.W + xl;
      float *oc = reinterpret_cast<float *>(p.out + lv.color);
      oc[at] = c[0];
      oc[n + at] = c[1];
      oc[2 * n + at] = c[2];
      if (has_d) reinterpret_cast<float *>(p.out + lv.depth)[at] = d;
      if (has_m) reinterpret_cast<uint8_t *>(p.out + lv.mask)[at] = (uint8_t)m;
    }
    if (l == p.levels || l == GSAJ_PYRAMID_MAX_LEVELS) break;
    // level l + 1: every lane of a group of 4 * stride reads the group's four pixels (all lanes take part in the lane reads)
    const int base = lane & ~(4 * stride - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      c[ch] = pyr_color(__shfl(c[ch], base), __shfl(c[ch], base + stride), __shfl(c[ch], base + 2 * stride), __shfl(c[ch], base + 3 * stride));
    if (has_d) d = pyr_depth(__shfl(d, base), __shfl(d, base + stride), __shfl(d, base + 2 * stride), __shfl(d, base + 3 * stride), p.edge_ratio);
    if (has_m) m = __shfl(m, base) | __shfl(m, base + stride) | __shfl(m, base + 2 * stride) | __shfl(m, base + 3 * stride);
    xl >>= 1;
    yl >>= 1;
  }
}

// ---- the Levenberg-Marquardt state at the next resolution ---------------------------------------------------------------------------
// gn_state / gn8_state: gn_state.h

// One wave, lane 0 (as the step kernels' tail): back to the accepted pose (and exposure) -- the last proposal was never judged, and
// a loss at another resolution cannot judge it --, the camera matrices from W2C and the NEXT level's projection matrix with the step
// kernels' own update (Exp(0) W2C), lambda back to lambda_init, no accepted loss: the first step at the new level accepts its loss
// as the baseline (the step kernels' first-call rule).  The step counters [83], [84] count over the frame and are kept.
__global__ __launch_bounds__(64) void k_gn_relevel(float *__restrict__ st, int joint, const float *__restrict__ projection, float lambda_init,
                                                   const uint32_t *__restrict__ skip) {
  if (skip && *skip != 0u) return;   // the level just finished was aborted on the device: nothing changes
  if (threadIdx.x != 0) return;
  if (st[GN_HAS] != 0.f) {
    for (int i = 0; i < 16; i++) st[PS_W2C + i] = st[GN_ACC_W2C + i];
    if (joint) {
      st[PS_EXP] = st[GN8_ACC_EXP];
      st[PS_EXP + 1] = st[GN8_ACC_EXP + 1];
    }
  }
  const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  pose_apply_delta(st, zero, projection, 0.f);   // view, full projection, camera centre; tau = 0, |tau| = 0, converged = 0
  if (joint) {
    st[GN8_DEXP] = 0.f;
    st[GN8_DEXP + 1] = 0.f;
  }
  st[GN_LAMBDA] = lambda_init;
  st[GN_ACC_LOSS] = 0.f;
  st[GN_HAS] = 0.f;
  for (int i = 0; i < 3; i++) st[GN_LAST + i] = 0.f;
  for (int i = 0; i < 16; i++) st[GN_ACC_W2C + i] = st[PS_W2C + i];
  const int end = joint ? GN8_ACC_EXP : GSAJ_GN_STATE_FLOATS - 5;   // the accepted H and g: [104:131) / [104:148)
  for (int i = GN_H; i < end; i++) st[i] = 0.f;
  if (joint) {
    st[GN8_ACC_EXP] = st[PS_EXP];
    st[GN8_ACC_EXP + 1] = st[PS_EXP + 1];
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" size_t gsaj_pyramid_bytes(int W, int H, int levels, int has_depth, int has_mask) {
  PyrLayout lay;
  return pyr_layout(W, H, levels, has_depth, has_mask, &lay) ? lay.bytes : 0;
}

extern "C" int gsaj_pyramid_level(int W, int H, int levels, int has_depth, int has_mask, int level, int *W_l, int *H_l, size_t *color_off,
                                  size_t *depth_off, size_t *mask_off) {
  PyrLayout lay;
  if (!pyr_layout(W, H, levels, has_depth, has_mask, &lay) || level < 1 || level > levels) {
    gsaj_set_error("gsaj_pyramid_level: levels must be 1..%d with W >> levels >= 1 and H >> levels >= 1, level 1..levels (W=%d H=%d levels=%d "
                   "level=%d)", GSAJ_PYRAMID_MAX_LEVELS, W, H, levels, level);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const PyrLevel &v = lay.lv[level - 1];
  if (W_l) *W_l = v.W;
  if (H_l) *H_l = v.H;
  if (color_off) *color_off = v.color;
  if (depth_off) *depth_off = v.depth;
  if (mask_off) *mask_off = v.mask;
  return GSAJ_OK;
}

extern "C" int gsaj_pyramid_build(int W, int H, int levels, const float *color, const float *depth, const uint8_t *mask, float depth_edge_ratio,
                                  void *pyramid, void *stream) {
  PyrLayout lay;
  if (!pyr_layout(W, H, levels, depth != nullptr, mask != nullptr, &lay) || !color || !pyramid || !(depth_edge_ratio >= 0.f) ||
      !(depth_edge_ratio < __builtin_inff())) {
    gsaj_set_error("gsaj_pyramid_build: levels must be 1..%d with W >> levels >= 1 and H >> levels >= 1, color and pyramid are required, "
                   "depth_edge_ratio must be finite and >= 0 (W=%d H=%d levels=%d depth_edge_ratio=%g)", GSAJ_PYRAMID_MAX_LEVELS, W, H, levels,
                   (double)depth_edge_ratio);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  PyrParams p;
  p.W = W; p.H = H; p.levels = levels; p.color = color; p.depth = depth; p.mask = mask; p.edge_ratio = depth_edge_ratio;
  p.out = static_cast<char *>(pyramid);
  // an even W keeps every row pair 8-byte (mask: 2-byte) aligned relative to the plane; the planes themselves must be too
  p.vec = (W % 2 == 0) && ((size_t)W * H % 2 == 0) && reinterpret_cast<size_t>(color) % 8 == 0 && (!depth || reinterpret_cast<size_t>(depth) % 8 == 0) &&
          (!mask || reinterpret_cast<size_t>(mask) % 2 == 0);
  for (int l = 0; l < GSAJ_PYRAMID_MAX_LEVELS; l++) p.lv[l] = lay.lv[l];
  const dim3 grid((unsigned)((lay.lv[0].W + 15) / 16), (unsigned)((lay.lv[0].H + 15) / 16));
  hipLaunchKernelGGL(k_pyramid, grid, dim3(256), 0, (hipStream_t)stream, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_pose_gn_relevel(float *gn_state, int state_floats, const float *projection_matrix_next, float lambda_init, const uint32_t *skip,
                                    void *stream) {
  if (!gn_state || !projection_matrix_next || (state_floats != GSAJ_GN_STATE_FLOATS && state_floats != GSAJ_GN8_STATE_FLOATS) ||
      !(lambda_init > 0.f)) {
    gsaj_set_error("gsaj_pose_gn_relevel: gn_state and projection_matrix_next are required, state_floats = GSAJ_GN_STATE_FLOATS or "
                   "GSAJ_GN8_STATE_FLOATS, lambda_init > 0 (state_floats=%d lambda_init=%g)", state_floats, (double)lambda_init);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(k_gn_relevel, dim3(1), dim3(64), 0, (hipStream_t)stream, gn_state, state_floats == GSAJ_GN8_STATE_FLOATS ? 1 : 0,
                     projection_matrix_next, lambda_init, skip);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
