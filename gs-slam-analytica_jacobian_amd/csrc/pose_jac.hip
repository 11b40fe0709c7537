// pose_jac.hip -- the per-pixel pose Jacobian d(C, D)/dtau in forward mode, the 6x6 normal equations of the tracking loss
// formed from it, and a Levenberg-Marquardt pose step on the device (gfx950).
//
// tau = [rho(3), theta(3)] is the left increment W2C <- Exp(tau) W2C.  J_p in R^{4x6} (rows r, g, b, depth) is the exact
// transpose of the linear map the backward implements: sum_p sum_ch s[ch, p] J_p[ch, :] == dL_dtau_sum of
// gsaj_rasterize_backward(seeds = s) in real arithmetic, gate for gate (DESIGN.md "Gauss-Newton tracking").
//
//  k_splat_jac     one lane per visible Gaussian: the rows d(mean2D, conic, depth, colour)/dtau -- gaussian_chain_geom /
//                  sh_backward (gaussian_chain.h: the backward's own chain) applied to unit sums, 45 floats in a 48-float row.
//  k_render_jac    the forward-mode compositor: k_render_fwd's work decomposition (one wave64 per 8x8 quadrant, private LDS
//                  staging, no workgroup barrier, tiles in tile_order with the XCD-aware block mapping) over the state of a
//                  FINISHED forward: only the entries the quadrant's forward wave took (BinWS.taken) are staged, each pixel
//                  stops at its n_contrib, and power / G / alpha come from gsaj_power2 / gsaj_load_row -- every gate decides
//                  on the forward's bits.  Per pixel, walking front to back (dalpha, dc, dz are 6-vectors):
//                      J_ch += T (alpha dc[ch] + c[ch] (dalpha - alpha S));   S += dalpha / (1 - alpha);   T *= 1 - alpha
//                  and J_ch -= bg[ch] T_final S_final for the colour rows.  dalpha = o G dpower: the 0.99 cap is no gradient gate.
//                  With seeds s and curvatures h (given as images, or derived from the tracking loss: loss_terms.h) the pixel's
//                  g = sum s J and H = sum h J^T J are reduced over the wave and stored as ONE 32-float row per workgroup
//                  -- no atomics anywhere, so the results are the same bits run to run.
//  k_gn_reduce     the explicit form's tail: the rows summed in slot order (fp64) -> H [21], g [6].
//  k_gn_step       the fused form's tail: the same sum, then accept / reject, damping, a 6x6 Cholesky solve in fp64 and
//                  Exp(tau) W2C with the Adam pose step's own device functions (pose_se3.h).  One launch, no host read.
//  k_render_jac<true, true> / k_gn_step<8>   the joint form: the unknowns are x = [rho, theta, a, b] with the exposure e^a C + b of the
//                  tracking loss.  r_ch = m (e^a C_ch + b - gt_ch), so relative to the rendered colour the exposure parameters are two more
//                  Jacobian columns, J8[ch] = [J[ch][0..5], C_ch, 1 / e^a] (0, 0 in the depth row), under the same seeds and
//                  curvatures: H8 (36, upper triangle by rows) and g8 (8) in ONE 64-float row per workgroup, 8x8 solve, a and b
//                  stepped, saved and restored with the pose.  The same body and the same step, instantiated for 8 unknowns.
//  K views of ONE map are the same kernels with gridDim.y = K (k_splat_jac, the loss-fused k_render_jac) or one workgroup per view
//                  (k_gn_step): every per-view pointer is moved on by the view's index x its stride, for K independent solves in one set
//                  of launches (a keyframe window's poses against a fixed map; K start poses of one frame).  A single view is K = 1 with
//                  zero strides.  Only cov3D is not per view: a batched forward writes it into view 0's geometry block only.
//  k_gn_select     one wave: the view of smallest accepted loss among the active views that have accepted a pose.
#include "gsaj_common.h"
#include "gaussian_chain.h"
#include "loss_terms.h"
#include "gn_state.h"
#include "wave_reduce.h"

#define JROW_F 48      // floats per derivative row: m2x[6] m2y[6] conic a[6] b[6] c[6] depth[6] colour r[3] g[3] b[3], 3 unused
#define JROW_F4 (JROW_F / 4)
#define JAC_CHUNK 32   // list positions examined (and at most that many entries staged) per wave and trip: 1.5 KB of splat rows + 6 KB
                       // of derivative rows + the ids = 7.8 KB of LDS per wave

// ---- per-Gaussian derivative rows ----------------------------------------------------------------------------------------
// The chain is linear in the ten sums the reverse compositor hands it, so its transpose is the chain applied to unit sums:
// row j of d(.)/dtau = the tau the chain returns for sum j = 1, all others 0.  Opacity does not depend on tau.  The colour
// rows are the view-direction term of the SH colour (rho columns only, masked by the clamp flags: sh_backward).
//
// K views of one map (gridDim.y = K; one view: K = 1 and zero strides): view v's camera, radii, clamp flags, abort word and rows come
// from view v's blocks.  p.cov3Ds is NOT moved on: Sigma does not depend on the view, and a batched forward writes it into view 0's
// geometry block only (or the caller gave it) -- as k_chain_window reads it.  projmatrix_raw is shared.
__global__ __launch_bounds__(64) void k_splat_jac(BwdParams p, const uint8_t *__restrict__ clamped, const uint32_t *__restrict__ counters,
                                                  float *__restrict__ rows, ViewStrides vs, size_t rows_stride) {
  const size_t view = blockIdx.y;
  p.viewmatrix += 16 * view;
  p.projmatrix += 16 * view;
  if (p.shs) p.campos += 3 * view;
  p.radii += view * (size_t)p.P;
  clamped = gsaj_shift(clamped, view * vs.geom);
  counters = gsaj_shift(counters, view * vs.image);
  rows = gsaj_shift(rows, view * rows_stride);
  if (counters[4]) return;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= p.P) return;
  const size_t ii = (size_t)idx;
  const int radius = p.radii[ii];
  const float3 mean = make_float3(p.means3D[3 * ii], p.means3D[3 * ii + 1], p.means3D[3 * ii + 2]);
  float c6[6];
#pragma unroll
  for (int k = 0; k < 6; k++) c6[k] = p.cov3Ds[6 * ii + k];
  uint8_t cl[3] = {0, 0, 0};
  if (p.shs) {
    cl[0] = clamped[3 * ii]; cl[1] = clamped[3 * ii + 1]; cl[2] = clamped[3 * ii + 2];
  }
  if (radius <= 0) return;
  float *row = rows + ii * JROW_F;
#pragma unroll 1
  for (int u = 0; u < 6; u++) {
    const float4 s0 = make_float4(u == 0 ? 1.f : 0.f, u == 1 ? 1.f : 0.f, u == 2 ? 1.f : 0.f, u == 3 ? 1.f : 0.f);
    const float4 s1 = make_float4(u == 4 ? 1.f : 0.f, 0.f, 0.f, 0.f);
    const float4 s2 = make_float4(0.f, u == 5 ? 1.f : 0.f, 0.f, 0.f);
    GaussianGrads o;
    float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    gaussian_chain_geom(p, mean, c6, s0, s1, s2, o, tau);
#pragma unroll
    for (int k = 0; k < 6; k++) row[6 * u + k] = tau[k];
  }
  float col[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.shs) {
    const float3 cam = make_float3(p.campos[0], p.campos[1], p.campos[2]);
    const float *sh_row = p.shs + ii * 3 * (size_t)p.M;
    float w_unused[16];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float3 unit = make_float3(ch == 0 ? 1.f : 0.f, ch == 1 ? 1.f : 0.f, ch == 2 ? 1.f : 0.f);
      const float3 dmean = sh_backward<1>(p.D, p.M, mean, cam, sh_row, w_unused, cl, unit);
      col[3 * ch] = -dmean.x; col[3 * ch + 1] = -dmean.y; col[3 * ch + 2] = -dmean.z;
    }
  }
  float4 *row4 = reinterpret_cast<float4 *>(row + 36);
  row4[0] = make_float4(col[0], col[1], col[2], col[3]);
  row4[1] = make_float4(col[4], col[5], col[6], col[7]);
  row4[2] = make_float4(col[8], 0.f, 0.f, 0.f);
}

// ---- forward-mode compositor ----------------------------------------------------------------------------------------------

// JOINT (with LOSS): the exposure columns and the 64-float row of the joint form; the walk is the same code.
template <bool LOSS, bool JOINT>
__device__ __forceinline__ void render_jac_body(
    int W, int H, int gx, int tiles, int P, ImageWS im, const float4 *__restrict__ splat, const float4 *__restrict__ splat16,
    const float *__restrict__ bg, const uint32_t *__restrict__ point_list, const uint32_t *__restrict__ taken,
    const float4 *__restrict__ rows, JacOut jo, FusedLoss fl) {
  static_assert(LOSS || !JOINT, "the joint form is a form of the loss-fused compositor");
  constexpr int ROW = JOINT ? GN8_ROW : GN_ROW;
  __shared__ float4 srow[JAC_CHUNK * 3];         // (x, y, kx, ky) (kz, o, 1-based list position, -) (r, g, b, depth)
  __shared__ float4 drow[JAC_CHUNK * JROW_F4];   // the entries' derivative rows
  __shared__ uint32_t sid[JAC_CHUNK];
  const uint32_t *__restrict__ counters = im.counters;
  if (counters[4]) return;  // aborted async frame: the partial rows stay the previous frame's (k_gn_step is handed the abort word)
  const int lane = threadIdx.x;
  // 32 consecutive workgroups = 8 tiles x 4 quadrants; tile slot = blockIdx.x & 7 (the XCD the workgroup lands on): k_render_fwd's mapping
  const int wave = ((int)blockIdx.x >> 3) & 3;
  const int rank = ((int)blockIdx.x >> 5) * 8 + ((int)blockIdx.x & 7);
  if (rank >= tiles) {
    if (jo.partials && lane < ROW) jo.partials[(size_t)blockIdx.x * ROW + lane] = 0.f;
    return;
  }
  const int tile = (int)min(im.tile_order[rank], (uint32_t)(tiles - 1));
  const int ty = tile / gx, tx = tile - ty * gx;
  const int px = tx * TILE + (wave & 1) * 8 + (lane & 7);
  const int py = ty * TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)py;
  const size_t pid = (size_t)py * W + px, HW = (size_t)H * W;
  const uint2 range = im.ranges[tile];
  const uint32_t last = inside ? im.n_contrib[pid] : 0u;
  // furthest last contributor of the quadrant (a position of the tile's own list: the clamp only keeps a stale workspace inside it)
  const uint32_t wmax = min(wave_max(last), range.y - range.x);
  const bool rec16 = counters[7] != 0u;
  const float half_w = 0.5f * W, half_h = 0.5f * H;

  float T = 1.f;
  float C[4] = {0.f, 0.f, 0.f, 0.f};
  float J[4][6], S[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    S[k] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) J[ch][k] = 0.f;
  }

  for (uint32_t base = 0u; base < wmax; base += JAC_CHUNK) {
    // lane l < 32: did some pixel of this quadrant take list entry base + l?  (the forward's answer: no test of the entry here)
    const uint32_t pos = base + (uint32_t)lane;
    bool rel = false;
    uint32_t id = 0u;
    if (lane < JAC_CHUNK && pos < wmax) {
      rel = ((taken[range.x + pos] >> (8 * wave)) & 0xffu) != 0u;
      if (rel) id = min(point_list[range.x + pos], (uint32_t)(P - 1));  // (clamped: a stale list must not name a row outside the workspace)
    }
    const unsigned long long todo = __builtin_amdgcn_ballot_w64(rel);
    const int nrel = __popcll(todo);
    if (nrel == 0) continue;  // (wave-uniform)
    if (rel) {
      const int slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(todo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)todo, 0u));
      float4 q0, q1, q2;
      gsaj_load_row(splat, splat16, id, rec16, q0, q1, q2);
      const float3 k = gsaj_prescale_conic(q1.x, q1.y, q1.z);
      srow[slot * 3 + 0] = make_float4(q0.x, q0.y, k.x, k.y);
      srow[slot * 3 + 1] = make_float4(k.z, q1.w, __uint_as_float(pos + 1u), 0.f);
      srow[slot * 3 + 2] = make_float4(q2.x, q2.y, q2.z, q0.z);
      sid[slot] = id;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the derivative rows, gathered next to the splat rows: 12 float4 per entry, consecutive lanes take consecutive pieces
    for (int i = lane; i < nrel * JROW_F4; i += 64) {
      const int e = i / JROW_F4, part = i - e * JROW_F4;
      drow[i] = rows[(size_t)sid[e] * JROW_F4 + part];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int s = 0; s < nrel; s++) {
      const float4 a0 = srow[s * 3 + 0], a1 = srow[s * 3 + 1], c = srow[s * 3 + 2];
      const float dx = a0.x - pxf, dy = a0.y - pyf;
      // the forward's own expression (gsaj_common.h): power <= 0 / alpha >= 1/255 are decided on identical bits
      const float p2 = gsaj_power2(dx, dy, a0.z, a0.w, a1.x);
      const float oG = a1.y * __builtin_amdgcn_exp2f(p2);
      const bool valid = __float_as_uint(a1.z) <= last && p2 <= 0.0f && oG >= (1.0f / 255.0f);
      if (__builtin_amdgcn_ballot_w64(valid) == 0ull) continue;
      // a pixel that skips the entry runs the same arithmetic with o G = 0: alpha = 0, dalpha = 0, nothing changes
      const float oGm = valid ? oG : 0.f;
      const float alpha = fminf(0.99f, oGm);
      // d power = sum_j f_j d(sum j)/dtau with the reverse compositor's coefficients of w (render_bwd.hip, v[0..4]); dalpha = o G d power
      const float ca = a0.z * (-2.0f / GSAJ_LOG2E), cb = a0.w * (-1.0f / GSAJ_LOG2E), cc = a1.x * (-2.0f / GSAJ_LOG2E);
      const float f0 = oGm * (-(ca * dx + cb * dy) * half_w);
      const float f1 = oGm * (-(cc * dy + cb * dx) * half_h);
      const float f2 = oGm * (-0.5f * dx * dx);
      const float f3 = oGm * (-0.5f * dx * dy);
      const float f4 = oGm * (-0.5f * dy * dy);
      const float *D = reinterpret_cast<const float *>(drow + s * JROW_F4);
      const float w = alpha * T;  // the forward's weight, from the forward's operations
      const float inv1ma = __builtin_amdgcn_rcpf(1.f - alpha);
      float e[6];
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const float da = f0 * D[k] + f1 * D[6 + k] + f2 * D[12 + k] + f3 * D[18 + k] + f4 * D[24 + k];
        e[k] = T * (da - alpha * S[k]);
        S[k] += da * inv1ma;
      }
      const float cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int ch = 0; ch < 4; ch++) {
#pragma unroll
        for (int k = 0; k < 6; k++) J[ch][k] += cv[ch] * e[k];
      }
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
#pragma unroll
        for (int k = 0; k < 3; k++) J[ch][k] += w * D[36 + 3 * ch + k];
      }
#pragma unroll
      for (int k = 0; k < 6; k++) J[3][k] += w * D[30 + k];
#pragma unroll
      for (int ch = 0; ch < 4; ch++) C[ch] = __builtin_fmaf(cv[ch], w, C[ch]);
      T = __builtin_fmaf(-alpha, T, T);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // background: C += T_final bg, so J_ch -= bg[ch] T_final S_final (colour rows)
  const float bgv[3] = {bg[0], bg[1], bg[2]};
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float tb = T * bgv[ch];
#pragma unroll
    for (int k = 0; k < 6; k++) J[ch][k] -= tb * S[k];
  }
  if (inside) {
    if (jo.jac) {
      float2 *o = reinterpret_cast<float2 *>(jo.jac + pid * 24);
#pragma unroll
      for (int ch = 0; ch < 4; ch++) {
#pragma unroll
        for (int k = 0; k < 6; k += 2) o[ch * 3 + k / 2] = make_float2(J[ch][k], J[ch][k + 1]);
      }
    }
    if (jo.color) {
      jo.color[pid] = __builtin_fmaf(T, bgv[0], C[0]);
      jo.color[HW + pid] = __builtin_fmaf(T, bgv[1], C[1]);
      jo.color[2 * HW + pid] = __builtin_fmaf(T, bgv[2], C[2]);
    }
    if (jo.depth) jo.depth[pid] = C[3];
  }
  if (!jo.partials) return;

  // ---- this pixel's seeds and curvatures, its share of g = sum s J and H = sum h J^T J, and the loss terms ----
  float sv[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
  float ls[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float cx[3] = {0.f, 0.f, 0.f}, iea = 0.f;  // joint form: the exposure columns of the colour rows (a: the forward's colour, b: 1 / e^a)
  bool want_h = true;
  if (LOSS) {
    if (inside) {
      const LossConsts L = loss_consts(fl.flags, fl.alpha, fl.rgb_thr, fl.exp_a, fl.exp_b, HW, 1.f);
      const bool mask = fl.grad_mask ? fl.grad_mask[pid] != 0 : true;
      const float gd = L.mono ? 0.f : fl.gt_depth[pid], d = L.mono ? 0.f : fl.depth[pid];
      const float g0 = fl.gt_color[pid], g1 = fl.gt_color[HW + pid], g2 = fl.gt_color[2 * HW + pid];
      const float c0 = fl.color[pid], c1 = fl.color[HW + pid], c2 = fl.color[2 * HW + pid], op = fl.opacity[pid];
      const LossPixel o = loss_pixel(L, g0, g1, g2, c0, c1, c2, op, mask, gd, d);
      const LossGN q = loss_pixel_gn(L, o, g0, g1, g2, c0, c1, c2, op, mask, gd, d, jo.delta);
#pragma unroll
      for (int ch = 0; ch < 4; ch++) sv[ch] = q.s[ch], hv[ch] = q.h[ch];
      // the pixel's share of loss = k_rgb sum w|r| + k_d sum |r_d| (loss_consts: k_rgb = (alpha | 1) / 3HW, k_d = (1 - alpha) / HW),
      // of L_rgb and L_depth, and the two exposure sums of loss_pixel
      ls[0] = L.k_rgb * o.s_rgb + L.k_d * o.s_d;
      ls[1] = o.s_rgb / (3.f * (float)HW);
      ls[2] = o.s_d / (float)HW;
      ls[3] = o.s_a;
      ls[4] = o.s_b;
      if (JOINT) {
        cx[0] = c0; cx[1] = c1; cx[2] = c2;
        iea = __fdiv_rn(1.f, L.ea);
      }
    }
  } else {
    want_h = jo.curv_c != nullptr;
    if (inside) {
      if (jo.seed_c) {
        sv[0] = jo.seed_c[pid]; sv[1] = jo.seed_c[HW + pid]; sv[2] = jo.seed_c[2 * HW + pid]; sv[3] = jo.seed_d[pid];
      }
      if (want_h) {
        hv[0] = jo.curv_c[pid]; hv[1] = jo.curv_c[HW + pid]; hv[2] = jo.curv_c[2 * HW + pid]; hv[3] = jo.curv_d[pid];
      }
    }
  }
  float *out = jo.partials + (size_t)blockIdx.x * ROW;
  if (JOINT) {
    // 49 sums.  Four at a time go through ONE tree (wave_reduce.h: two half-wave swaps fold lane bits 5 and 4 of four values into one
    // register, four row rotations finish it): 7 cross-lane steps per four values where four butterflies take 24, and row r's first
    // lane stores its own value, so the row's stores are 13 x 4 lanes wide instead of 49 by lane 0.  The tree is fixed -- the same bits
    // run to run -- and adds the pairs wave_sum's butterfly adds (bit 5, bit 4, then 8, 4, 2, 1 within a row): the pose block comes
    // out as the 6-form's bits (measured, not promised).
    float v[52];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
      for (int l = k; l < 8; l++, n++) {
        float t = 0.f;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
          const float jk = k < 6 ? J[ch][k] : (ch == 3 ? 0.f : (k == 6 ? cx[ch] : iea));
          const float jl = l < 6 ? J[ch][l] : (ch == 3 ? 0.f : (l == 6 ? cx[ch] : iea));
          t += (hv[ch] * jk) * jl;
        }
        v[n] = t;
      }
    }
#pragma unroll
    for (int k = 0; k < 8; k++, n++) {
      float t = 0.f;
#pragma unroll
      for (int ch = 0; ch < 4; ch++) t += sv[ch] * (k < 6 ? J[ch][k] : (ch == 3 ? 0.f : (k == 6 ? cx[ch] : iea)));
      v[n] = t;
    }
#pragma unroll
    for (int k = 0; k < 5; k++, n++) v[n] = ls[k];
    v[49] = v[50] = v[51] = 0.f;
#pragma unroll
    for (int q = 0; q < 13; q++) store4(out + 4 * q, lane, reduce4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]));
    if (lane >= 52) out[lane] = 0.f;
    return;
  }
  int n = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
#pragma unroll
    for (int l = k; l < 6; l++, n++) {
      float v = 0.f;
      if (want_h) {
#pragma unroll
        for (int ch = 0; ch < 4; ch++) v += (hv[ch] * J[ch][k]) * J[ch][l];
        v = wave_sum(v);
      }
      if (lane == 0) out[n] = v;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) {
    float v = 0.f;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) v += sv[ch] * J[ch][k];
    v = wave_sum(v);
    if (lane == 0) out[21 + k] = v;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const float v = wave_sum(ls[k]);
    if (lane == 0) out[27 + k] = v;
  }
}

// K views of one map (gridDim.y = K; one view: K = 1 and zero strides), the loss-fused forms: the body on view v's blocks.  Every
// per-view pointer is moved on by blockIdx.y x its stride (workgroup-uniform: scalar adds), as k_render_fwd / k_render_bwd do; view v
// owns gridDim.x partial rows.  The explicit form (LOSS = false) is one view's: launched with gridDim.y = 1 only, it moves nothing.
template <bool LOSS, bool JOINT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_render_jac(
    int W, int H, int gx, int tiles, int P, ImageWS im, const float4 *__restrict__ splat, const float4 *__restrict__ splat16,
    const float *__restrict__ bg, const uint32_t *__restrict__ point_list, const uint32_t *__restrict__ taken,
    const float4 *__restrict__ rows, JacOut jo, FusedLoss fl, ViewStrides vs, size_t rows_stride) {
  if (LOSS) {
    const size_t view = blockIdx.y, HWv = (size_t)H * W;
    im = image_view(im, view * vs.image);
    splat = gsaj_shift(splat, view * vs.geom);
    splat16 = gsaj_shift(splat16, view * vs.geom);
    point_list = gsaj_shift(point_list, view * vs.bin);
    taken = gsaj_shift(taken, view * vs.bin);
    rows = gsaj_shift(rows, view * rows_stride);
    if (jo.jac) jo.jac += view * HWv * 24;
    jo.partials += view * (size_t)gridDim.x * (JOINT ? GN8_ROW : GN_ROW);
    fused_loss_view(fl, view, HWv, 0);  // (no loss partials here: the sums are slots of jo.partials)
  }
  render_jac_body<LOSS, JOINT>(W, H, gx, tiles, P, im, splat, splat16, bg, point_list, taken, rows, jo, fl);
}

// ---- the partial rows summed in slot order, in fp64 (gn_sum_rows: gn_state.h) ----------------------------------------------------
__global__ __launch_bounds__(GN_SUM_THREADS) void k_gn_reduce(const float *__restrict__ partials, int n, const uint32_t *__restrict__ counters,
                                                   float *__restrict__ H_out, float *__restrict__ g_out) {
  __shared__ double red[GN_SUM_THREADS / GN_ROW][GN_ROW], sums[GN_ROW];
  if (counters[4]) return;  // aborted async frame
  gn_sum_rows<GN_ROW>(partials, n, red, sums);
  const int t = threadIdx.x;
  if (H_out && t < 21) H_out[t] = (float)sums[t];
  if (g_out && t >= 21 && t < 27) g_out[t - 21] = (float)sums[t];
}

struct GnStepParams {
  const float *partials;
  int n;
  float lambda_init, nu, lambda_min, lambda_max, threshold;
  const float *projection;
  float *st;
  const uint32_t *skip;
};

// (H + lambda diag(H) + eps I) x = -g by Cholesky in fp64, NX unknowns; eps = 1e-9 x the mean diagonal of H + 1e-30 keeps a direction
// the frame says nothing about (H row == 0) solvable.  Returns false on a non-positive (or non-finite) pivot.
template <int NX>
__device__ bool gn_solve(const float *Hs, const float *gs, double lambda, double *tau) {
  double A[NX][NX], Lc[NX][NX], y[NX];
  int n = 0;
  double tr = 0.0;
  for (int k = 0; k < NX; k++)
    for (int l = k; l < NX; l++, n++) A[k][l] = A[l][k] = (double)Hs[n];
  for (int k = 0; k < NX; k++) tr += A[k][k];
  const double eps = 1e-9 * (tr / (double)NX) + 1e-30;
  for (int k = 0; k < NX; k++) A[k][k] = A[k][k] + lambda * A[k][k] + eps;
  for (int j = 0; j < NX; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d -= Lc[j][k] * Lc[j][k];
    if (!(d > 0.0) || !(d < 1e300)) return false;
    const double ljj = sqrt(d);
    Lc[j][j] = ljj;
    for (int i = j + 1; i < NX; i++) {
      double v = A[i][j];
      for (int k = 0; k < j; k++) v -= Lc[i][k] * Lc[j][k];
      Lc[i][j] = v / ljj;
    }
  }
  for (int i = 0; i < NX; i++) {
    double v = -(double)gs[i];
    for (int k = 0; k < i; k++) v -= Lc[i][k] * y[k];
    y[i] = v / Lc[i][i];
  }
  for (int i = NX - 1; i >= 0; i--) {
    double v = y[i];
    for (int k = i + 1; k < NX; k++) v -= Lc[k][i] * tau[k];
    tau[i] = v / Lc[i][i];
  }
  for (int i = 0; i < NX; i++)
    if (!(fabs(tau[i]) < 1e300)) return false;
  return true;
}

// NX = 6: the pose alone (rows of GN_ROW floats, H [21], g [6]).  NX = 8: the pose and the exposure (rows of GN8_ROW floats, H8 [36],
// g8 [8]); a and b live in the pose state (PS_EXP), are stepped by x[6], x[7], saved on accept and restored on reject with W2C.
template <int NX>
__device__ __forceinline__ void gn_step_body(const GnStepParams &p) {
  constexpr int ROW = NX == 8 ? GN8_ROW : GN_ROW, NH = NX * (NX + 1) / 2, G_AT = NX == 8 ? GN8_G : GN_G;
  __shared__ double red[GN_SUM_THREADS / ROW][ROW], sums[ROW];
  // the frame these rows belong to was aborted on the device (its kernels returned at once: the rows are the PREVIOUS iteration's)
  if (p.skip && *p.skip != 0u) return;
  gn_sum_rows<ROW>(p.partials, p.n, red, sums);
  if (threadIdx.x != 0) return;
  float *st = p.st;
  const float loss = (float)sums[NH + NX];
  st[GN_LAST + 0] = loss;
  st[GN_LAST + 1] = (float)sums[NH + NX + 1];
  st[GN_LAST + 2] = (float)sums[NH + NX + 2];
  const bool has = st[GN_HAS] != 0.f;
  float lambda = has ? st[GN_LAMBDA] : p.lambda_init;
  if (!has || loss <= st[GN_ACC_LOSS]) {  // accept the pose these rows were rendered at
    st[GN_ACC_LOSS] = loss;
    for (int i = 0; i < 16; i++) st[GN_ACC_W2C + i] = st[PS_W2C + i];
    for (int i = 0; i < NH; i++) st[GN_H + i] = (float)sums[i];
    for (int i = 0; i < NX; i++) st[G_AT + i] = (float)sums[NH + i];
    if (NX == 8) {
      st[GN8_ACC_EXP] = st[PS_EXP];
      st[GN8_ACC_EXP + 1] = st[PS_EXP + 1];
    }
    lambda = fmaxf(lambda / p.nu, p.lambda_min);
    st[GN_HAS] = 1.f;
    st[GN_ACCEPTED] += 1.f;
  } else {  // reject: back to the accepted pose and its normal equations, more damping
    for (int i = 0; i < 16; i++) st[PS_W2C + i] = st[GN_ACC_W2C + i];
    if (NX == 8) {
      st[PS_EXP] = st[GN8_ACC_EXP];
      st[PS_EXP + 1] = st[GN8_ACC_EXP + 1];
    }
    lambda = fminf(lambda * p.nu, p.lambda_max);
    st[GN_REJECTED] += 1.f;
  }
  double tau64[NX];
  float delta[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool ok = gn_solve<NX>(st + GN_H, st + G_AT, (double)lambda, tau64);
  if (ok) {
    for (int i = 0; i < NX; i++) delta[i] = (float)tau64[i];
  } else {
    lambda = fminf(lambda * p.nu, p.lambda_max);  // no step from this factorisation: more damping next time
  }
  st[GN_LAMBDA] = lambda;
  // Exp(tau) W2C, the camera matrices, tau, |tau|, converged (tau = 0 on a failed factorisation: the pose comes out unchanged)
  pose_apply_delta(st, delta, p.projection, p.threshold);
  if (NX == 8) {  // (x[6], x[7] = 0 on a failed factorisation: the exposure comes out unchanged)
    st[PS_EXP] += delta[6];
    st[PS_EXP + 1] += delta[7];
    st[GN8_DEXP] = delta[6];
    st[GN8_DEXP + 1] = delta[7];
    if (!(fmaxf(fabsf(delta[6]), fabsf(delta[7])) < p.threshold)) st[PS_CONV] = 0.f;
  }
  if (!ok) st[PS_CONV] = 0.f;
}

// K states in one launch (one state: K = 1): workgroup v steps view v's rows (p.n of them), state and skip word.  active [K] bytes or
// NULL: an inactive view's state is not touched.  The projection matrix and the LM scalars are shared.
// (gn_step_view works on its own copy of the kernel's argument: moved on in place, in the kernel's own text, the state's accepted count
// is fetched by a vector load where this form has a scalar one -- the instructions the batched step always had.)
template <int NX>
__device__ __forceinline__ void gn_step_view(GnStepParams p, const uint8_t *__restrict__ active, size_t skip_stride) {
  constexpr int ROW = NX == 8 ? GN8_ROW : GN_ROW, STATE = NX == 8 ? GSAJ_GN8_STATE_FLOATS : GSAJ_GN_STATE_FLOATS;
  const size_t v = blockIdx.x;
  if (active && !active[v]) return;
  p.partials += v * (size_t)p.n * ROW;
  p.st += v * STATE;
  if (p.skip) p.skip = gsaj_shift(p.skip, v * skip_stride);
  gn_step_body<NX>(p);
}
template <int NX>
__global__ __launch_bounds__(GN_SUM_THREADS) void k_gn_step(GnStepParams p, const uint8_t *__restrict__ active, size_t skip_stride) {
  gn_step_view<NX>(p, active, skip_stride);
}

// One wave: the view of smallest accepted loss among the views that are active, have accepted a pose and whose loss is finite; ties
// go to the lowest index; none: -1 (and +inf).
__global__ __launch_bounds__(64) void k_gn_select(int K, const float *__restrict__ states, int state_floats, const uint8_t *__restrict__ active,
                                                  int *__restrict__ best, float *__restrict__ best_loss) {
  const int lane = threadIdx.x;
  float bl = __builtin_inff();
  int bi = 0x7fffffff;
  for (int v = lane; v < K; v += 64) {  // (ascending v per lane: a strict < keeps the lowest index of a tie)
    const float *st = states + (size_t)v * state_floats;
    const float loss = st[GN_ACC_LOSS];
    const bool ok = (!active || active[v]) && st[GN_HAS] != 0.f && fabsf(loss) < __builtin_inff();
    if (ok && loss < bl) { bl = loss; bi = v; }  // (a finite loss is below the initial +inf)
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ol = __shfl_xor(bl, m);
    const int oi = __shfl_xor(bi, m);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ol < bl || (ol == bl && oi < bi))) { bl = ol; bi = oi; }
  }
  if (lane == 0) {
    *best = bi == 0x7fffffff ? -1 : bi;
    *best_loss = bi == 0x7fffffff ? __builtin_inff() : bl;
  }
}

// ---- launchers (api.hip) ------------------------------------------------------------------------------------------------------
size_t gsaj_jac_rows_bytes(int P) { return gsaj_align(sizeof(float) * JROW_F * (size_t)(P > 0 ? P : 1)); }
int gsaj_jac_slots(int W, int H) { return gsaj_fwd_loss_slots(W, H); }

int launch_splat_jac(const BwdParams &p, int K, const GeomWS &g, const ImageWS &im, float *rows, ViewStrides vs, size_t rows_stride,
                     hipStream_t s) {
  const int nblk = (p.P + 63) / 64;
  hipLaunchKernelGGL(k_splat_jac, dim3(nblk, K), dim3(64), 0, s, p, g.clamped, im.counters, rows, vs, rows_stride);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// fl == NULL: the explicit form (K = 1: its kernel moves no pointer on)
int launch_render_jac(const BwdParams &p, int K, const float *bg, const Carved &c, const float *rows, size_t rows_stride, const JacOut &jo,
                      const FusedLoss *fl, int joint, hipStream_t s) {
  const dim3 grid((unsigned)gsaj_jac_slots(p.W, p.H), (unsigned)K);
  const auto kernel = !fl ? k_render_jac<false, false> : joint ? k_render_jac<true, true> : k_render_jac<true, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(64), 0, s, p.W, p.H, p.grid_x, p.grid_x * p.grid_y, p.P, c.im, c.g.splat, c.g.splat16, bg,
                     c.b.point_list, c.b.taken, reinterpret_cast<const float4 *>(rows), jo, fl ? *fl : FusedLoss{}, c.vs, rows_stride);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

int launch_gn_reduce(const float *partials, int n, const ImageWS &im, float *H_out, float *g_out, hipStream_t s) {
  hipLaunchKernelGGL(k_gn_reduce, dim3(1), dim3(GN_SUM_THREADS), 0, s, partials, n, im.counters, H_out, g_out);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_gn_state_floats(void) { return GSAJ_GN_STATE_FLOATS; }

extern "C" int gsaj_gn8_state_floats(void) { return GSAJ_GN8_STATE_FLOATS; }

// the one launcher of the four step entry points; `required`: the caller's words for what it requires (the K of a batched call included)
static int gn_step_launch(const char *who, const char *required, bool joint, int K, const uint8_t *active, size_t skip_stride,
                          const GnStepParams &p, hipStream_t s) {
  if (K <= 0 || !p.partials || p.n <= 0 || !p.st || !(p.nu > 1.f) || !(p.lambda_min > 0.f) || !(p.lambda_max >= p.lambda_min) ||
      !(p.lambda_init >= p.lambda_min) || !(p.lambda_init <= p.lambda_max)) {
    gsaj_set_error("%s: %s are required; nu > 1, 0 < lambda_min <= lambda_init <= lambda_max", who, required);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (joint)
    hipLaunchKernelGGL(k_gn_step<8>, dim3((unsigned)K), dim3(GN_SUM_THREADS), 0, s, p, active, skip_stride);
  else
    hipLaunchKernelGGL(k_gn_step<6>, dim3((unsigned)K), dim3(GN_SUM_THREADS), 0, s, p, active, skip_stride);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
static const char *const GN_STEP_REQUIRED = "gn_partials, n_partials > 0 and gn_state";
static const char *const GN_STEP_BATCH_REQUIRED = "K > 0, gn_partials, n_partials > 0 and gn_states";

extern "C" int gsaj_pose_gn_step(const float *gn_partials, int n_partials, float lambda_init, float nu, float lambda_min, float lambda_max,
                                 float converged_threshold, const float *projection_matrix, float *gn_state, const uint32_t *skip,
                                 void *stream) {
  const GnStepParams p{gn_partials, n_partials, lambda_init, nu, lambda_min, lambda_max, converged_threshold, projection_matrix, gn_state, skip};
  return gn_step_launch("gsaj_pose_gn_step", GN_STEP_REQUIRED, false, 1, nullptr, 0, p, (hipStream_t)stream);
}

extern "C" int gsaj_pose_gn8_step(const float *gn8_partials, int n_partials, float lambda_init, float nu, float lambda_min, float lambda_max,
                                  float converged_threshold, const float *projection_matrix, float *gn8_state, const uint32_t *skip,
                                  void *stream) {
  const GnStepParams p{gn8_partials, n_partials, lambda_init, nu, lambda_min, lambda_max, converged_threshold, projection_matrix, gn8_state, skip};
  return gn_step_launch("gsaj_pose_gn8_step", GN_STEP_REQUIRED, true, 1, nullptr, 0, p, (hipStream_t)stream);
}

extern "C" int gsaj_pose_gn_step_batch(int K, const float *gn_partials, int n_partials, const uint8_t *active, float lambda_init, float nu,
                                       float lambda_min, float lambda_max, float converged_threshold, const float *projection_matrix,
                                       float *gn_states, const uint32_t *skip, size_t skip_stride_bytes, void *stream) {
  const GnStepParams p{gn_partials, n_partials, lambda_init, nu, lambda_min, lambda_max, converged_threshold, projection_matrix, gn_states, skip};
  return gn_step_launch("gsaj_pose_gn_step_batch", GN_STEP_BATCH_REQUIRED, false, K, active, skip_stride_bytes, p, (hipStream_t)stream);
}

extern "C" int gsaj_pose_gn8_step_batch(int K, const float *gn8_partials, int n_partials, const uint8_t *active, float lambda_init, float nu,
                                        float lambda_min, float lambda_max, float converged_threshold, const float *projection_matrix,
                                        float *gn8_states, const uint32_t *skip, size_t skip_stride_bytes, void *stream) {
  const GnStepParams p{gn8_partials, n_partials, lambda_init, nu, lambda_min, lambda_max, converged_threshold, projection_matrix, gn8_states, skip};
  return gn_step_launch("gsaj_pose_gn8_step_batch", GN_STEP_BATCH_REQUIRED, true, K, active, skip_stride_bytes, p, (hipStream_t)stream);
}

extern "C" int gsaj_pose_gn_select(int K, const float *gn_states, int state_floats, const uint8_t *active, int *best, float *best_loss,
                                   void *stream) {
  if (K <= 0 || !gn_states || (state_floats != GSAJ_GN_STATE_FLOATS && state_floats != GSAJ_GN8_STATE_FLOATS) || !best || !best_loss) {
    gsaj_set_error("gsaj_pose_gn_select: K > 0, gn_states, state_floats = GSAJ_GN_STATE_FLOATS or GSAJ_GN8_STATE_FLOATS, best and best_loss are required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(k_gn_select, dim3(1), dim3(64), 0, (hipStream_t)stream, K, gn_states, state_floats, active, best, best_loss);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
