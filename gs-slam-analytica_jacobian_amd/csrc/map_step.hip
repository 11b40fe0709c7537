// map_step.hip -- the step on the Gaussian map in one launch: the chain rule through the activations, Adam on the six raw
// parameters, and the opacity resets (gfx950).  Semantics: include/gsaj.h; the reference does this with autograd through exp /
// sigmoid / normalize / cat, a foreach Adam over six groups and replace_tensor_to_optimizer (gaussian_model.py:438-451, 544-557).
//
// The work is elementwise, P rows x (3 + 3 M + 1 + S + 4) floats x (parameter, two moments, gradient): every tensor is walked along
// its own flat element index, so a wave's loads and stores are consecutive dwords (or consecutive 16-byte pieces where the host
// found the group's three addresses aligned).  A workgroup belongs to exactly one group (the host lays the six groups' workgroups
// out back to back), so the group switch is wave-uniform.  The gradient is always read a dword at a time: the bucket's views are
// only 4-byte aligned for odd P, and an f_rest run of four leaves its g_sh row every 3 (M - 1) elements.
// This file is compiled with -ffp-contract=off: one rounding per operation, which is what tests/map_step_restated.py's bound counts.
#include <limits.h>

#include "gsaj_common.h"

#define MS_BLOCK 256
enum { MS_XYZ = 0, MS_DC, MS_REST, MS_OP, MS_SC, MS_ROT };

struct MapStepParams {
  float *p[GSAJ_MAP_GROUPS], *m[GSAJ_MAP_GROUPS], *v[GSAJ_MAP_GROUPS];
  const float *g_mean, *g_sh, *g_op, *g_sc, *g_rot;
  const int *radii;
  float step_size[GSAJ_MAP_GROUPS], bc2_sqrt[GSAJ_MAP_GROUPS];
  unsigned n[GSAJ_MAP_GROUPS];          // elements of the group
  unsigned block_end[GSAJ_MAP_GROUPS];  // one past the group's last workgroup (a group that does nothing has none)
  unsigned vec4;                        // bit s: group s is walked four elements per lane, 16-byte accesses
  unsigned P, sh_row, rest_row, scale_cols;  // sh_row = 3 M, rest_row = 3 (M - 1)
  int K_vis, flags;
  float b1, c1, b2, c2, eps, reset_value;  // b = (float)beta, c = (float)(1.0 - beta)
};

__device__ __forceinline__ float ms_sigmoid(float o) { return 1.f / (1.f + expf(-o)); }

// dL/d(raw parameter element e of group `seg`), pv = that element's value
__device__ __forceinline__ float ms_grad(const MapStepParams &a, int seg, unsigned e, float pv) {
  switch (seg) {
    case MS_XYZ:
      return a.g_mean[e];
    case MS_DC: {
      const unsigned r = e / 3u;
      return a.g_sh[(size_t)r * a.sh_row + (e - 3u * r)];
    }
    case MS_REST: {
      const unsigned r = e / a.rest_row;
      return a.g_sh[(size_t)r * a.sh_row + 3u + (e - r * a.rest_row)];
    }
    case MS_OP: {
      const float s = ms_sigmoid(pv);
      return a.g_op[e] * s * (1.f - s);
    }
    case MS_SC: {
      const float ex = expf(pv);
      if (a.scale_cols == 3u) return a.g_sc[e] * ex;
      const float *g = a.g_sc + (size_t)e * 3;  // isotropic: the one log-scale drives the three axes
      return (g[0] * ex + g[1] * ex) + g[2] * ex;
    }
    default:
      return 0.f;  // (MS_ROT: ms_rot_grad, a row at a time)
  }
}

// the four gradients of one quaternion row from the row's own values q (already in registers: nothing of the row is read again)
__device__ __forceinline__ void ms_rot_grad(const float *__restrict__ g, const float q[4], float out[4]) {
  const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
  const float n = fmaxf(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), 1e-12f);
  const float h0 = q[0] / n, h1 = q[1] / n, h2 = q[2] / n, h3 = q[3] / n;
  const float dot = ((g0 * h0 + g1 * h1) + g2 * h2) + g3 * h3;
  out[0] = (g0 - h0 * dot) / n;
  out[1] = (g1 - h1 * dot) / n;
  out[2] = (g2 - h2 * dot) / n;
  out[3] = (g3 - h3 * dot) / n;
}

// VEC consecutive elements per lane; WIDE (with VEC == 4): the host found the group's three addresses 16-byte aligned
template <int VEC, bool WIDE>
__device__ __forceinline__ void ms_body(const MapStepParams &a, int seg, unsigned local_block) {
  const unsigned n = a.n[seg];
  const size_t e0 = ((size_t)local_block * MS_BLOCK + threadIdx.x) * VEC;
  if (e0 >= n) return;
  const int cnt = (n - e0 < (size_t)VEC) ? (int)(n - e0) : VEC;
  float *pp = a.p[seg] + e0, *pm = a.m[seg] + e0, *pv = a.v[seg] + e0;
  float p[VEC], m[VEC], v[VEC];
  bool wide = false;
  if constexpr (WIDE) {
    wide = cnt == 4;
    if (wide) {
      const float4 p4 = *reinterpret_cast<const float4 *>(pp), m4 = *reinterpret_cast<const float4 *>(pm),
                   v4 = *reinterpret_cast<const float4 *>(pv);
      p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w;
      m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    }
  }
  if (!wide) {
    for (int k = 0; k < VEC; k++)
      if (k < cnt) { p[k] = pp[k]; m[k] = pm[k]; v[k] = pv[k]; }
  }
  const bool reset = seg == MS_OP && (a.flags & (GSAJ_MAP_RESET_ALL | GSAJ_MAP_RESET_NONVISIBLE));
  if (reset) {
    for (int k = 0; k < VEC; k++) {
      if (k >= cnt) break;
      float np = a.reset_value;
      if (!(a.flags & GSAJ_MAP_RESET_ALL)) {
        bool visible = false;
        for (int kv = 0; kv < a.K_vis; kv++) visible |= a.radii[(size_t)kv * a.P + e0 + k] > 0;
        if (visible) np = (a.flags & GSAJ_MAP_RESET_KEEP_VISIBLE) ? p[k] : ms_sigmoid(p[k]);
      }
      p[k] = np; m[k] = 0.f; v[k] = 0.f;
    }
  } else {
    const float b1 = a.b1, b2 = a.b2, c1 = a.c1, c2 = a.c2;
    const float step_size = a.step_size[seg], bc2_sqrt = a.bc2_sqrt[seg];
    float gr[VEC];
    bool row = false;
    if constexpr (VEC == 4) {
      row = seg == MS_ROT;  // one lane, one row (the group has 4 P elements: cnt == 4)
      if (row) ms_rot_grad(a.g_rot + e0, p, gr);
    }
    if (!row) {
      for (int k = 0; k < VEC; k++)
        if (k < cnt) gr[k] = ms_grad(a, seg, (unsigned)e0 + k, p[k]);
    }
    for (int k = 0; k < VEC; k++) {
      if (k >= cnt) break;
      const float g = gr[k];
      const float mk = b1 * m[k] + c1 * g;
      const float vk = b2 * v[k] + c2 * g * g;
      const float denom = sqrtf(vk) / bc2_sqrt + a.eps;
      p[k] = p[k] + (-step_size * (mk / denom));
      m[k] = mk; v[k] = vk;
    }
  }
  if constexpr (WIDE) {
    if (wide) {
      *reinterpret_cast<float4 *>(pp) = make_float4(p[0], p[1], p[2], p[3]);
      *reinterpret_cast<float4 *>(pm) = make_float4(m[0], m[1], m[2], m[3]);
      *reinterpret_cast<float4 *>(pv) = make_float4(v[0], v[1], v[2], v[3]);
      return;
    }
  }
  for (int k = 0; k < VEC; k++)
    if (k < cnt) { pp[k] = p[k]; pm[k] = m[k]; pv[k] = v[k]; }
}

__global__ void __launch_bounds__(MS_BLOCK) k_map_step(MapStepParams a) {
  int seg = 0;
  unsigned first = 0;
  for (int s = 0; s < GSAJ_MAP_GROUPS - 1; s++)
    if (blockIdx.x >= a.block_end[s]) { seg = s + 1; first = a.block_end[s]; }
  // the rotation group always goes a row per lane, so that a row's gradient comes from the values its own lane holds
  const bool wide = (a.vec4 >> seg) & 1u;
  if (wide)
    ms_body<4, true>(a, seg, blockIdx.x - first);
  else if (seg == MS_ROT)
    ms_body<4, false>(a, seg, blockIdx.x - first);
  else
    ms_body<1, false>(a, seg, blockIdx.x - first);
}

extern "C" int gsaj_map_step(int P, int M, int scale_cols, int K_vis, const GsajMapStepArgs *args, void *stream) {
  if (P < 0 || M < 1 || (scale_cols != 1 && scale_cols != 3) || !args) {
    gsaj_set_error("gsaj_map_step: invalid argument (P >= 0, M >= 1, scale_cols 1 or 3, args are required)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((long long)P * 3 * M > (long long)INT_MAX) {
    gsaj_set_error("gsaj_map_step: invalid argument (P * 3 * M exceeds INT_MAX)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const int all_flags = GSAJ_MAP_RESET_ALL | GSAJ_MAP_RESET_NONVISIBLE | GSAJ_MAP_RESET_KEEP_VISIBLE;
  if (args->flags & ~all_flags) {
    gsaj_set_error("gsaj_map_step: invalid argument (flags has bits outside GSAJ_MAP_RESET_*)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const bool reset = (args->flags & (GSAJ_MAP_RESET_ALL | GSAJ_MAP_RESET_NONVISIBLE)) != 0;
  const bool by_view = reset && !(args->flags & GSAJ_MAP_RESET_ALL);
  if (by_view && (!args->radii || K_vis < 1)) {
    gsaj_set_error("gsaj_map_step: invalid argument (GSAJ_MAP_RESET_NONVISIBLE needs radii [K_vis,P] with K_vis >= 1)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  MapStepParams a;
  const unsigned up = (unsigned)P;
  const unsigned cols[GSAJ_MAP_GROUPS] = {3u, 3u, 3u * (unsigned)(M - 1), 1u, (unsigned)scale_cols, 4u};
  const float *grads[GSAJ_MAP_GROUPS] = {args->g_mean3D, args->g_sh, args->g_sh, args->g_opacity, args->g_scale, args->g_rot};
  static const char *const names[GSAJ_MAP_GROUPS] = {"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"};
  unsigned blocks = 0;
  a.vec4 = 0;
  for (int s = 0; s < GSAJ_MAP_GROUPS; s++) {
    const bool resets = reset && s == MS_OP, steps = !resets && !args->skip[s];
    a.n[s] = (steps || resets) ? up * cols[s] : 0u;
    a.p[s] = args->param[s]; a.m[s] = args->exp_avg[s]; a.v[s] = args->exp_avg_sq[s];
    a.step_size[s] = args->step_size[s]; a.bc2_sqrt[s] = args->bc2_sqrt[s];
    if (a.n[s]) {
      if (!a.p[s] || !a.m[s] || !a.v[s] || (steps && !grads[s])) {
        gsaj_set_error("gsaj_map_step: invalid argument (group %s: parameter, exp_avg, exp_avg_sq%s are required)", names[s],
                       steps ? " and its gradient" : "");
        return GSAJ_ERR_INVALID_ARGUMENT;
      }
      const bool aligned = ((((uintptr_t)a.p[s]) | ((uintptr_t)a.m[s]) | ((uintptr_t)a.v[s])) & 15u) == 0;
      if (aligned) a.vec4 |= 1u << s;
      const unsigned per_block = MS_BLOCK * ((aligned || s == MS_ROT) ? 4u : 1u);
      blocks += (a.n[s] + per_block - 1) / per_block;
    }
    a.block_end[s] = blocks;
  }
  if (P == 0 || blocks == 0) return GSAJ_OK;
  a.g_mean = args->g_mean3D; a.g_sh = args->g_sh; a.g_op = args->g_opacity; a.g_sc = args->g_scale; a.g_rot = args->g_rot;
  a.radii = by_view ? args->radii : nullptr;
  a.P = up; a.sh_row = 3u * (unsigned)M; a.rest_row = 3u * (unsigned)(M - 1); a.scale_cols = (unsigned)scale_cols;
  a.K_vis = by_view ? K_vis : 0; a.flags = args->flags;
  a.b1 = (float)args->beta1; a.c1 = (float)(1.0 - args->beta1); a.b2 = (float)args->beta2; a.c2 = (float)(1.0 - args->beta2);
  a.eps = (float)args->eps; a.reset_value = args->reset_value;
  hipLaunchKernelGGL(k_map_step, dim3(blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, a);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
