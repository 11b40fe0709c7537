// align.hip -- frame-to-frame RGB-D alignment (include/gsaj.h "frame-to-frame alignment"): the start pose of a new frame from the
// last tracked frame alone, no map, no binning, no lists.
//   rgbd_align_body<JOINT>   the pixel pass of both forms, one thread per REFERENCE pixel: back-project, transform, project into the
//                       current frame, bilinear sample, photometric and depth residual with their Jacobians, IRLS seed / curvature /
//                       loss; the partials of a 256-thread workgroup (64 x 4 pixels, lane = x) folded in registers (wave_reduce.h) and
//                       across its four waves through LDS in a fixed order: ONE row per workgroup, no atomics
//   k_rgbd_align        the pose-only form (gsaj_rgbd_align): 32 partials per thread (H 21, g 6, three losses, two counts), three
//                       reduce10 and a reduce4 per wave, a row of GSAJ_GN_PARTIAL_FLOATS
//   k_rgbd_align8       the joint form (gsaj_rgbd_align8): the affine brightness change e^a I_r + b of the current frame against the
//                       reference solved with the pose.  Two more Jacobian columns in the photometric term: 49 partials per thread
//                       (H8 36, g8 8, three losses, two counts), five reduce10 per wave, a row of GSAJ_GN8_PARTIAL_FLOATS
//   rgbd_align_fold_body<ROW, VALID>   one workgroup: the rows added in a fixed order in fp64 (gn_sum_rows), normalised by the number of
//                       valid pixels, the overlap gate -> the one row gsaj_pose_gn_step / gsaj_pose_gn8_step takes with n_partials = 1
//                       (k_rgbd_align_fold, k_rgbd_align8_fold)
// Compiled without FMA contraction: tests/align_restated.py and tests/align_joint_restated.py mirror the per-pixel arithmetic one fp32
// rounding at a time, so both forms' floats depend on the expression trees below and on nothing the register allocator decides.
#include "gsaj_common.h"
#include "gn_state.h"
#include "wave_reduce.h"

#define AL_ROW GN_ROW
#define AL_PIX GSAJ_ALIGN_PIXEL_FLOATS
#define AL_MAX_SIDE 16384
#define AL8_ROW GN8_ROW
static_assert(AL_ROW == 32 && AL8_ROW == 64 && AL_PIX == 16, "row / pixel record layout");
static_assert(GN_ROW_VALID == 30 && GN8_ROW_VALID == 47, "the rows' count slots");

struct AlignParams {
  int W, H;
  float fx, fy, cx, cy;
  const float *ref_color, *ref_depth, *ref_w2c, *cur_color, *cur_depth, *state;
  float w_depth, delta_photo, delta_depth, edge_ratio, min_depth, max_depth;
  float *rows, *pix_out;
  uint8_t *valid_out;
  const uint32_t *skip;
};

__device__ __forceinline__ bool al_finite(float x) { return fabsf(x) < __builtin_inff(); }   // (false for a NaN)
__device__ __forceinline__ float al_grey(const float *__restrict__ c, size_t N, size_t at) { return ((c[at] + c[N + at]) + c[2 * N + at]) * (float)(1.0 / 3.0); }

// One IRLS term: seed kappa clamp(r / delta, -1, 1), curvature kappa / max(|r|, delta), loss kappa rho(r)
__device__ __forceinline__ void al_irls(float r, float kappa, float delta, float &s, float &h, float &l) {
  const float ar = fabsf(r);
  s = kappa * fminf(fmaxf(r / delta, -1.f), 1.f);
  h = kappa / fmaxf(ar, delta);
  l = kappa * (ar >= delta ? ar - 0.5f * delta : (r * r) / (2.f * delta));
}

// ---- the pixel pass.  JOINT: the unknowns are [rho, theta, a, b]; r_I = I_c - (e^a I_r + b) with a, b the state's exposure (PS_EXP),
// the photometric row J8 = [J_I, -(e^a I_r), -1], the depth row [J_Z, 0, 0].  gain_out (JOINT only; may be NULL): the e^a the pass used
// -- expf is not correctly rounded, and tests/align_joint_restated.py evaluates its mirror with that very float.
// The warp, the gates, the taps and the depth term are the same text for both forms; what the joint form adds stands under `if (JOINT)`.
// A thread's partials: the upper triangle of H row by row (NH), g (NX), loss / L_photo / L_depth, the valid count, the open depth gates.
template <bool JOINT>
__device__ __forceinline__ void rgbd_align_body(const AlignParams &p, float *__restrict__ gain_out) {
  constexpr int NX = JOINT ? 8 : 6, NH = NX * (NX + 1) / 2, ROW = JOINT ? AL8_ROW : AL_ROW;
  constexpr int LIVE = NH + NX + 5;      // the row's live slots: 32 (all of the row) / 49 ([49:64) zero)
  constexpr int G10 = JOINT ? 5 : 3;     // reduce10 groups per wave; the 6-form's two counts go through a reduce4 instead,
  constexpr int NACC = JOINT ? 10 * G10 : LIVE;   // the joint form's ride in the fifth group, with one zero that fills it
  constexpr int NT = JOINT ? 14 : 12, NPART = JOINT ? 12 * G10 : 12 * G10 + 4;
  static_assert(10 * G10 == (JOINT ? LIVE + 1 : LIVE - 2) && LIVE <= ROW, "the partials and their reduce groups");
  __shared__ float T[NT];             // T_rel = W2C_cur inverse(W2C_ref), rows 0..2; JOINT: e^a, b
  __shared__ float part[4][NPART];    // per wave: G10 store10 slots of 12 floats; 6-form: one store4 slot
  if (p.skip && *p.skip != 0u) return;   // (workgroup-uniform)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (JOINT) {
    if (t == 12) {   // one expf per workgroup; workgroup (0, 0) reports it
      const float ea = expf(p.state[PS_EXP]);
      T[NT - 2] = ea;
      T[NT - 1] = p.state[PS_EXP + 1];
      if (gain_out && blockIdx.x == 0 && blockIdx.y == 0) *gain_out = ea;
    }
  }
  if (t < 12) {
    // the rigid inverse [R^T, -R^T t] of the reference pose and the product, every sum left to right
    const float *c = p.state + PS_W2C, *r = p.ref_w2c;
    const int i = t >> 2, j = t & 3;
    if (j < 3) {
      T[t] = (c[i * 4 + 0] * r[j * 4 + 0] + c[i * 4 + 1] * r[j * 4 + 1]) + c[i * 4 + 2] * r[j * 4 + 2];
    } else {
      float ti[3];
      for (int k = 0; k < 3; k++) ti[k] = -((r[0 + k] * r[3] + r[4 + k] * r[7]) + r[8 + k] * r[11]);
      T[t] = ((c[i * 4 + 0] * ti[0] + c[i * 4 + 1] * ti[1]) + c[i * 4 + 2] * ti[2]) + c[i * 4 + 3];
    }
  }
  __syncthreads();
  const int W = p.W, H = p.H;
  const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + wave;
  const bool inside = x < W && y < H;
  const size_t N = (size_t)W * H, at = inside ? (size_t)y * W + x : 0;

  float acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.f;
  float rec[AL_PIX];
#pragma unroll
  for (int k = 0; k < AL_PIX; k++) rec[k] = 0.f;
  uint32_t flags = 0u;

  bool ok = inside;
  float Ir = 0.f, Zr = 0.f;
  if (ok) {
    Ir = al_grey(p.ref_color, N, at);
    Zr = p.ref_depth[at];
    ok = al_finite(Ir) && al_finite(Zr) && Zr >= p.min_depth && Zr <= p.max_depth;
  }
  float Xc = 0.f, Yc = 0.f, Zc = 0.f;
  if (ok) {
    const float xn = (((float)x + 0.5f) - p.cx) / p.fx, yn = (((float)y + 0.5f) - p.cy) / p.fy;
    const float Xr = xn * Zr, Yr = yn * Zr;
    Xc = ((T[0] * Xr + T[1] * Yr) + T[2] * Zr) + T[3];
    Yc = ((T[4] * Xr + T[5] * Yr) + T[6] * Zr) + T[7];
    Zc = ((T[8] * Xr + T[9] * Yr) + T[10] * Zr) + T[11];
    ok = al_finite(Xc) && al_finite(Yc) && al_finite(Zc) && Zc >= p.min_depth;
  }
  if (ok) {
    const float iz = 1.f / Zc, fxz = p.fx * iz, fyz = p.fy * iz, px = fxz * Xc, py = fyz * Yc;
    const float u = (px + p.cx) - 0.5f, v = (py + p.cy) - 0.5f;
    const float x0f = floorf(u), y0f = floorf(v);
    // 0 <= x0 and x0 + 1 <= W - 1, decided on the floats (a NaN or an inf fails): u = W - 1 exactly is outside
    ok = x0f >= 0.f && x0f <= (float)(W - 2) && y0f >= 0.f && y0f <= (float)(H - 2);
    if (ok) {
      const size_t q = (size_t)(int)y0f * W + (size_t)(int)x0f;
      const float a = u - x0f, b = v - y0f, oma = 1.f - a, omb = 1.f - b;
      const float I00 = al_grey(p.cur_color, N, q), I01 = al_grey(p.cur_color, N, q + 1), I10 = al_grey(p.cur_color, N, q + W),
                  I11 = al_grey(p.cur_color, N, q + W + 1);
      ok = al_finite(I00) && al_finite(I01) && al_finite(I10) && al_finite(I11);
      if (ok) {
        const float Ic = (I00 * oma + I01 * a) * omb + (I10 * oma + I11 * a) * b;
        const float gx = omb * (I01 - I00) + b * (I11 - I10), gy = oma * (I10 - I00) + a * (I11 - I01);
        const float duz = -(px * iz), dvz = -(py * iz);
        float rI, J[NX];
        if (JOINT) {
          const float gI = T[NT - 2] * Ir;   // the reference grey as the current frame would show it, before the offset
          rI = Ic - (gI + T[NT - 1]);
          J[NX - 2] = -gI;
          J[NX - 1] = -1.f;
        } else {
          rI = Ic - Ir;
        }
        J[0] = gx * fxz;
        J[1] = gy * fyz;
        J[2] = gx * duz + gy * dvz;
        J[3] = J[2] * Yc - J[1] * Zc;
        J[4] = J[0] * Zc - J[2] * Xc;
        J[5] = J[1] * Xc - J[0] * Yc;
        float sI, hI, lI;
        al_irls(rI, 1.f, p.delta_photo, sI, hI, lI);
        flags = 1u;
        rec[0] = u; rec[1] = v; rec[2] = Xc; rec[3] = Yc; rec[4] = Zc; rec[5] = Ic; rec[6] = gx; rec[7] = gy; rec[8] = rI; rec[9] = sI;
        rec[10] = hI;
        float sZ = 0.f, hZ = 0.f, lZ = 0.f, JZ[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p.cur_depth) {
          const float D00 = p.cur_depth[q], D01 = p.cur_depth[q + 1], D10 = p.cur_depth[q + W], D11 = p.cur_depth[q + W + 1];
          const float dmin = fminf(fminf(D00, D01), fminf(D10, D11)), dmax = fmaxf(fmaxf(D00, D01), fmaxf(D10, D11));
          const bool open = al_finite(D00) && al_finite(D01) && al_finite(D10) && al_finite(D11) && dmin >= p.min_depth && dmax <= p.max_depth &&
                            dmax - dmin <= p.edge_ratio * dmin;
          if (open) {
            const float Dc = (D00 * oma + D01 * a) * omb + (D10 * oma + D11 * a) * b;
            const float hx = omb * (D01 - D00) + b * (D11 - D10), hy = oma * (D10 - D00) + a * (D11 - D01);
            const float rZ = Dc - Zc;
            const float k0 = hx * fxz, k1 = hy * fyz, k2 = hx * duz + hy * dvz;
            JZ[0] = k0;
            JZ[1] = k1;
            JZ[2] = k2 - 1.f;
            JZ[3] = (k2 * Yc - k1 * Zc) - Yc;
            JZ[4] = (k0 * Zc - k2 * Xc) + Xc;
            JZ[5] = k1 * Xc - k0 * Yc;
            al_irls(rZ, p.w_depth, p.delta_depth, sZ, hZ, lZ);
            flags |= 2u;
            rec[11] = Dc; rec[12] = rZ; rec[13] = sZ; rec[14] = hZ; rec[15] = 1.f;
          }
        }
        // H row by row, then g.  The depth term has no part in the exposure columns (l >= 6): those elements are the photometric
        // product alone
        int n = 0;
#pragma unroll
        for (int k = 0; k < NX; k++) {
          const float a_k = hI * J[k], z_k = k < 6 ? hZ * JZ[k] : 0.f;
#pragma unroll
          for (int l = k; l < NX; l++, n++) acc[n] = l < 6 ? a_k * J[l] + z_k * JZ[l] : a_k * J[l];
        }
#pragma unroll
        for (int k = 0; k < NX; k++) acc[NH + k] = k < 6 ? sI * J[k] + sZ * JZ[k] : sI * J[k];
        acc[NH + NX] = lI + lZ;
        acc[NH + NX + 1] = lI;
        acc[NH + NX + 2] = lZ;
        acc[NH + NX + 3] = 1.f;
        acc[NH + NX + 4] = (flags & 2u) ? 1.f : 0.f;
      }
    }
  }
  if (inside) {
    if (p.pix_out) {
      float *o = p.pix_out + at * AL_PIX;   // (dword stores: pix_out needs no more than 4-byte alignment)
#pragma unroll
      for (int k = 0; k < AL_PIX; k++) o[k] = rec[k];
    }
    if (p.valid_out) p.valid_out[at] = (uint8_t)flags;
  }

  // the workgroup's row: G10 reduce10 (and, 6-form, one reduce4) per wave (every lane takes part), then the four waves in order
#pragma unroll
  for (int g = 0; g < G10; g++) {
    const float v10[10] = {acc[10 * g], acc[10 * g + 1], acc[10 * g + 2], acc[10 * g + 3], acc[10 * g + 4],
                           acc[10 * g + 5], acc[10 * g + 6], acc[10 * g + 7], acc[10 * g + 8], acc[10 * g + 9]};
    float x0, x1, x2;
    reduce10(v10, x0, x1, x2);
    store10(&part[wave][12 * g], lane, x0, x1, x2);
  }
  if (!JOINT) store4(&part[wave][12 * G10], lane, reduce4(acc[LIVE - 2], acc[LIVE - 1], 0.f, 0.f));
  __syncthreads();
  if (t < ROW) {   // (joint form: [LIVE:ROW) zero)
    const int slot = t >= LIVE ? 0 : t < 10 * G10 ? 12 * (t / 10) + t % 10 : 12 * G10 + (t - 10 * G10);
    const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const float sum = ((part[0][slot] + part[1][slot]) + part[2][slot]) + part[3][slot];
    p.rows[row * ROW + t] = t < LIVE ? sum : 0.f;
  }
}
__global__ __launch_bounds__(256) void k_rgbd_align(AlignParams p) { rgbd_align_body<false>(p, nullptr); }
__global__ __launch_bounds__(256) void k_rgbd_align8(AlignParams p, float *__restrict__ gain_out) { rgbd_align_body<true>(p, gain_out); }

// ---- the fold: the step kernels' own gn_sum_rows (gn_state.h: the rows added in a fixed order in fp64), then the normalisation -------
// ROW floats per row, the count of valid pixels in slot VALID: H and g before VALID - 3, the three losses, the two counts (and, in the
// joint form, the zeros behind them, which stay zeros)
template <int ROW, int VALID>
__device__ __forceinline__ void rgbd_align_fold_body(const float *__restrict__ rows, int n, double need, float *__restrict__ out,
                                                     const uint32_t *__restrict__ skip) {
  __shared__ double red[GN_SUM_THREADS / ROW][ROW], sums[ROW];
  if (skip && *skip != 0u) return;
  gn_sum_rows<ROW>(rows, n, red, sums);
  const int c = threadIdx.x & (ROW - 1);
  if (threadIdx.x < ROW) {
    const double cnt = sums[VALID];   // an exact integer: every row's count is, and their sum stays below 2^53
    float o;
    if (c >= VALID)
      o = (float)sums[c];
    else if (cnt < need)   // too little overlap: no step from this frame, and a loss no proposal survives
      o = c < VALID - 3 ? 0.f : __builtin_inff();
    else
      o = (float)(sums[c] / cnt);
    out[c] = o;
  }
}
__global__ __launch_bounds__(GN_SUM_THREADS) void k_rgbd_align_fold(const float *__restrict__ rows, int n, double need, float *__restrict__ out,
                                                                    const uint32_t *__restrict__ skip) {
  rgbd_align_fold_body<AL_ROW, GN_ROW_VALID>(rows, n, need, out, skip);
}
__global__ __launch_bounds__(GN_SUM_THREADS) void k_rgbd_align8_fold(const float *__restrict__ rows, int n, double need, float *__restrict__ out,
                                                                     const uint32_t *__restrict__ skip) {
  rgbd_align_fold_body<AL8_ROW, GN8_ROW_VALID>(rows, n, need, out, skip);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int gsaj_rgbd_align_partial_rows(int W, int H) {
  if (W < 2 || H < 2 || W > AL_MAX_SIDE || H > AL_MAX_SIDE) return 0;
  return ((W + 63) / 64) * ((H + 3) / 4);
}

// both entry points: `joint` names the state (gn_state / gn8_state) and the row (gn_row / gn8_row) in the error text and picks the kernels
static int rgbd_align_launch(bool joint, int W, int H, float fx, float fy, float cx, float cy, const float *ref_color, const float *ref_depth,
                             const float *ref_w2c, const float *cur_color, const float *cur_depth, const float *gn_state, float w_depth,
                             float delta_photo, float delta_depth, float depth_edge_ratio, float min_depth, float max_depth, float min_overlap,
                             float *rows, float *gn_row, float *gain_out, float *pix_out, uint8_t *valid_out, const uint32_t *skip, void *stream) {
  const int n = gsaj_rgbd_align_partial_rows(W, H);
  if (n == 0 || !ref_color || !ref_depth || !ref_w2c || !cur_color || !gn_state || !rows || !gn_row || !(fx > 0.f) || !(fy > 0.f) ||
      !(delta_photo > 0.f) || !(delta_depth > 0.f) || !(w_depth >= 0.f) || !(depth_edge_ratio >= 0.f) || !(min_depth > 0.f) ||
      !(min_depth < max_depth) || !(min_overlap >= 0.f) || !(min_overlap <= 1.f)) {
    gsaj_set_error("gsaj_rgbd_align%s: W and H must be 2..%d; ref_color, ref_depth, ref_w2c, cur_color, %s, rows and %s are required; "
                   "fx, fy, delta_photo, delta_depth > 0; w_depth, depth_edge_ratio >= 0; 0 < min_depth < max_depth; min_overlap in [0, 1] "
                   "(W=%d H=%d fx=%g fy=%g w_depth=%g delta_photo=%g delta_depth=%g depth_edge_ratio=%g min_depth=%g max_depth=%g min_overlap=%g)",
                   joint ? "8" : "", AL_MAX_SIDE, joint ? "gn8_state" : "gn_state", joint ? "gn8_row" : "gn_row", W, H, (double)fx, (double)fy,
                   (double)w_depth, (double)delta_photo, (double)delta_depth, (double)depth_edge_ratio, (double)min_depth, (double)max_depth,
                   (double)min_overlap);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  AlignParams p;
  p.W = W; p.H = H; p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
  p.ref_color = ref_color; p.ref_depth = ref_depth; p.ref_w2c = ref_w2c; p.cur_color = cur_color; p.cur_depth = cur_depth; p.state = gn_state;
  p.w_depth = w_depth; p.delta_photo = delta_photo; p.delta_depth = delta_depth; p.edge_ratio = depth_edge_ratio;
  p.min_depth = min_depth; p.max_depth = max_depth;
  p.rows = rows; p.pix_out = pix_out; p.valid_out = valid_out; p.skip = skip;
  // n >= max(1, ceil(min_overlap W H)) valid pixels or no step
  double need = __builtin_ceil((double)min_overlap * (double)W * (double)H);
  if (need < 1.0) need = 1.0;
  const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4));
  const auto fold = joint ? k_rgbd_align8_fold : k_rgbd_align_fold;
  if (joint)   // (the two pixel kernels differ in their arguments: the joint form's takes gain_out)
    hipLaunchKernelGGL(k_rgbd_align8, grid, dim3(256), 0, (hipStream_t)stream, p, gain_out);
  else
    hipLaunchKernelGGL(k_rgbd_align, grid, dim3(256), 0, (hipStream_t)stream, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold, dim3(1), dim3(GN_SUM_THREADS), 0, (hipStream_t)stream, rows, n, need, gn_row, skip);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_rgbd_align(int W, int H, float fx, float fy, float cx, float cy, const float *ref_color, const float *ref_depth,
                               const float *ref_w2c, const float *cur_color, const float *cur_depth, const float *gn_state, float w_depth,
                               float delta_photo, float delta_depth, float depth_edge_ratio, float min_depth, float max_depth, float min_overlap,
                               float *rows, float *gn_row, float *pix_out, uint8_t *valid_out, const uint32_t *skip, void *stream) {
  return rgbd_align_launch(false, W, H, fx, fy, cx, cy, ref_color, ref_depth, ref_w2c, cur_color, cur_depth, gn_state, w_depth, delta_photo,
                           delta_depth, depth_edge_ratio, min_depth, max_depth, min_overlap, rows, gn_row, nullptr, pix_out, valid_out, skip, stream);
}

extern "C" int gsaj_rgbd_align8(int W, int H, float fx, float fy, float cx, float cy, const float *ref_color, const float *ref_depth,
                                const float *ref_w2c, const float *cur_color, const float *cur_depth, const float *gn8_state, float w_depth,
                                float delta_photo, float delta_depth, float depth_edge_ratio, float min_depth, float max_depth, float min_overlap,
                                float *rows, float *gn8_row, float *gain_out, float *pix_out, uint8_t *valid_out, const uint32_t *skip,
                                void *stream) {
  return rgbd_align_launch(true, W, H, fx, fy, cx, cy, ref_color, ref_depth, ref_w2c, cur_color, cur_depth, gn8_state, w_depth, delta_photo,
                           delta_depth, depth_edge_ratio, min_depth, max_depth, min_overlap, rows, gn8_row, gain_out, pix_out, valid_out, skip,
                           stream);
}
