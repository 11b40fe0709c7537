// sweep.hip -- motion stereo (include/gsaj.h "motion stereo"): the depth of a monocular keyframe from a second frame in general
// relative pose, by a plane sweep over inverse-depth hypotheses and the semi-global aggregation of stereo.hip.  This project's own
// statement (the reference has no counterpart); the device's bits equal tests/sweep_restated.py.
//   k_sweep_grad            both images in one launch: the clipped Sobel bytes Gx | Gy << 8 per pixel (sgm_sobel_bytes)
//   k_sweep_pixel_cost<D>   one lane per (x, d), d innermost: the reference pixel warped into the source frame under hypothesis d
//                           (fp32, one rounding per operation), four taps of the source's gradient bytes blended in sixteenths, the
//                           absolute differences to the reference's own bytes -> pc uint8 [H,W,D], a wave's 64 bytes contiguous
//   k_sweep_box<D>          C uint16 [H,W,D]: pc summed over the clamped window -- k_stereo_cost's walk down a band of rows with its
//                           ring of row sums in LDS (SGM_BOX_WALK), a row sum here 2r + 1 bytes of pc
//   (paths)                 launch_stereo_paths of stereo.hip with the first column 0: S uint32 [H,W,D]
//   k_sweep_winner<D>       a group of min(D, 64) lanes per pixel: argmin, uniqueness, the parabola step (sgm_argmin, sgm_subsample16),
//                           the centre warp of the winner once more (no mask is stored), idx16 and the depth; no LDS
//   k_sweep_grey_u8         float32 [3,H,W] -> the grey byte (the trackers' frames as this matcher's input)
// What is named sgm_* / SGM_* is shared with stereo.hip: sgm.h.  Compiled without FMA contraction: the warp is mirrored one fp32 rounding at a time.
#include "sgm.h"

#define SWEEP_RING 15    // 2 * 7 + 1 row sums
#define SWEEP_MAX_R 7    // 225 * 240 = 54 000 fits C's uint16
#define SWEEP_STAGES (GSAJ_SWEEP_STAGE_COST | GSAJ_SWEEP_STAGE_PATHS | GSAJ_SWEEP_STAGE_WINNER)

struct SweepWS {
  uint16_t *gr, *gs;   // [H,W] gradient bytes of the reference and the source image, Gx | Gy << 8
  uint8_t *pc;         // [H,W,D]
  uint16_t *C;         // [H,W,D]
  uint32_t *S;         // [H,W,D]
};

// (the workspace must be 256-byte aligned as handed over: carved BASE_AS_GIVEN, no base slack in its size)
static size_t sweep_carve(Carver c, int W, int H, int D, SweepWS *w, size_t *pc_off = nullptr, size_t *c_off = nullptr, size_t *s_off = nullptr) {
  const size_t n = (size_t)W * H;
  w->gr = c.take<uint16_t>(n);
  w->gs = c.take<uint16_t>(n);
  if (pc_off) *pc_off = c.used();
  w->pc = c.take<uint8_t>(n * D);
  if (c_off) *c_off = c.used();
  w->C = c.take<uint16_t>(n * D);
  if (s_off) *s_off = c.used();
  w->S = c.take<uint32_t>(n * D);
  return c.used();
}

struct SweepCam {
  int W, H;
  float fx, fy, cx, cy, w_min, step;
  const float *ref_w2c, *src_w2c;
};

// ---- a. gradient bytes ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SGM_BLOCK) void k_sweep_grad(int W, int H, const uint8_t *__restrict__ ref, size_t ref_stride,
                                                          const uint8_t *__restrict__ src, size_t src_stride, uint16_t *__restrict__ gr,
                                                          uint16_t *__restrict__ gs) {
  const size_t i = (size_t)blockIdx.x * SGM_BLOCK + threadIdx.x;
  if (i >= (size_t)W * H) return;
  const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
  (blockIdx.y ? gs : gr)[i] = (uint16_t)sgm_sobel_bytes(blockIdx.y ? src : ref, blockIdx.y ? src_stride : ref_stride, W, H, x, y);
}

// ---- b. element t (row-major, 3 x 4) of T = W2C_src inverse(W2C_ref): the rigid inverse [R^T, -R^T t] and the product, every sum left
// to right -- the lines of rgbd_align_body (align.hip), restated ----------------------------------------------------------------------
__device__ __forceinline__ float sweep_rel_pose(const float *__restrict__ c, const float *__restrict__ r, int t) {
  const int i = t >> 2, j = t & 3;
  if (j < 3) return (c[i * 4 + 0] * r[j * 4 + 0] + c[i * 4 + 1] * r[j * 4 + 1]) + c[i * 4 + 2] * r[j * 4 + 2];
  float ti[3];
  for (int k = 0; k < 3; k++) ti[k] = -((r[0 + k] * r[3] + r[4 + k] * r[7]) + r[8 + k] * r[11]);
  return ((c[i * 4 + 0] * ti[0] + c[i * 4 + 1] * ti[1]) + c[i * 4 + 2] * ti[2]) + c[i * 4 + 3];
}

// ---- d. the warp of reference pixel (x, y) at inverse depth w.  true: inside, q the top-left tap, fa, fb the sixteenths -----------------
__device__ __forceinline__ bool sweep_warp(const SweepCam &p, const float *T, int x, int y, float w, int &q, int &fa, int &fb) {
  const float xn = (((float)x + 0.5f) - p.cx) / p.fx, yn = (((float)y + 0.5f) - p.cy) / p.fy;
  const float ax = (T[0] * xn + T[1] * yn) + T[2], ay = (T[4] * xn + T[5] * yn) + T[6], az = (T[8] * xn + T[9] * yn) + T[10];
  const float px = ax + w * T[3], py = ay + w * T[7], pz = az + w * T[11];
  const float iz = 1.f / pz;
  const float u = ((p.fx * iz) * px + p.cx) - 0.5f, v = ((p.fy * iz) * py + p.cy) - 0.5f;
  const float x0 = floorf(u), y0 = floorf(v);
  // decided on the floats: a NaN or an inf fails, and so does every image narrower or lower than two pixels
  if (!(pz > 0.f && x0 >= 0.f && x0 <= (float)(p.W - 2) && y0 >= 0.f && y0 <= (float)(p.H - 2))) return false;
  fa = (int)floorf((u - x0) * 16.f);
  fb = (int)floorf((v - y0) * 16.f);
  q = (int)y0 * p.W + (int)x0;
  return true;
}

// ---- e. the pixel cost ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_sweep_pixel_cost(SweepCam p, int outside_cost, const uint16_t *__restrict__ gr,
                                                                const uint16_t *__restrict__ gs, uint8_t *__restrict__ pc) {
  __shared__ float T[12];
  if (threadIdx.x < 12) T[threadIdx.x] = sweep_rel_pose(p.src_w2c, p.ref_w2c, threadIdx.x);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * SGM_BLOCK + threadIdx.x, pix = i / D;
  if (pix >= (size_t)p.W * p.H) return;
  const int d = (int)(i % D), x = (int)(pix % (size_t)p.W), y = (int)(pix / (size_t)p.W);
  const float w = p.w_min + (float)d * p.step;
  int cost = outside_cost, q, fa, fb;
  if (sweep_warp(p, T, x, y, w, q, fa, fb)) {
    const int g00 = gs[q], g01 = gs[q + 1], g10 = gs[q + p.W], g11 = gs[q + p.W + 1], g = gr[pix];
    const int w00 = (16 - fa) * (16 - fb), w01 = fa * (16 - fb), w10 = (16 - fa) * fb, w11 = fa * fb;
    const int sx = w00 * (g00 & 255) + w01 * (g01 & 255) + w10 * (g10 & 255) + w11 * (g11 & 255);
    const int sy = w00 * (g00 >> 8) + w01 * (g01 >> 8) + w10 * (g10 >> 8) + w11 * (g11 >> 8);
    cost = (abs(256 * (g & 255) - sx) + abs(256 * (g >> 8) - sy)) >> 6;   // <= 2 * 256 * 30 / 64 = 240
  }
  pc[i] = (uint8_t)cost;
}

// ---- f. the block cost: the walk of sgm.h over every column, a row sum read from pc -------------------------------------------------------
__device__ __forceinline__ int sweep_row_sum(const uint8_t *__restrict__ pc, int W, int D, int y, int x, int d, int r) {
  const uint8_t *a = pc + (size_t)y * W * D + d;
  int s = 0;
  for (int dx = -r; dx <= r; dx++) s += a[(size_t)min(max(x + dx, 0), W - 1) * D];
  return s;
}

// grid: (columns in groups of SGM_BLOCK / D, bands of SGM_BAND rows)
template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_sweep_box(int W, int H, int r, const uint8_t *__restrict__ pc, uint16_t *__restrict__ C) {
  __shared__ uint16_t ring[SWEEP_RING * SGM_BLOCK];   // a row sum is <= 15 * 240
  const int d = threadIdx.x % D;
  const int x = (int)blockIdx.x * (SGM_BLOCK / D) + threadIdx.x / D;
  if (x >= W) return;
#define SWEEP_ROW_SUM(y) sweep_row_sum(pc, W, D, y, x, d, r)
  SGM_BOX_WALK(D, ring, x, d, W, H, r, C, SWEEP_ROW_SUM)   // C <= 225 * 240
}

// ---- h, i. winner, uniqueness, sub-sample step, the centre warp, depth ----------------------------------------------------------------
struct SweepWinner {
  int uniqueness;
  const uint32_t *S;
  int16_t *idx16;
  float *depth;   // or NULL
};

template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_sweep_winner(SweepCam p, SweepWinner q) {
  constexpr int WIDTH = SgmGroup<D>::WIDTH, LPW = SgmGroup<D>::LPW, GROUPS = SgmGroup<D>::GROUPS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (WIDTH - 1), g = wave * LPW + lane / WIDTH;
  const size_t n = (size_t)p.W * p.H, pix = (size_t)blockIdx.x * GROUPS + g;
  const bool active = pix < n;   // (no early return: the reductions below are executed by every lane)
  const uint32_t *s = q.S + (active ? pix : 0) * D;
  const SgmBest w = sgm_argmin<D>(s, sub, q.uniqueness);
  if (!active || sub != 0) return;
  int i16 = -16;
  if (!w.rival) {
    float T[12];
#pragma unroll
    for (int t = 0; t < 12; t++) T[t] = sweep_rel_pose(p.src_w2c, p.ref_w2c, t);
    int tap, fa, fb;
    if (sweep_warp(p, T, (int)(pix % (size_t)p.W), (int)(pix / (size_t)p.W), p.w_min + (float)w.d * p.step, tap, fa, fb))
      i16 = sgm_subsample16<D>(s, w.d, w.S);
  }
  q.idx16[pix] = (int16_t)i16;
  if (q.depth) {
    const double w = (double)p.w_min + ((double)i16 / 16.0) * (double)p.step;   // fp64, rounded to float32 once
    q.depth[pix] = (float)(i16 >= 0 && w > 0.0 ? 1.0 / w : 0.0);
  }
}

// ---- grey bytes of a tracker's colour ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SGM_BLOCK) void k_sweep_grey_u8(int W, int H, const float *__restrict__ c, uint8_t *__restrict__ out, size_t stride) {
  const size_t N = (size_t)W * H, i = (size_t)blockIdx.x * SGM_BLOCK + threadIdx.x;
  if (i >= N) return;
  const float g = ((c[i] + c[N + i]) + c[2 * N + i]) * (float)(1.0 / 3.0);   // al_grey of align.hip
  out[(i / (size_t)W) * stride + (i % (size_t)W)] = (uint8_t)fminf(fmaxf(floorf(g * 255.f + 0.5f), 0.f), 255.f);   // a NaN: fmaxf gives 0
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
static bool sweep_sizes_ok(const char *who, int W, int H, int D, int paths) {
  return sgm_sizes_ok(who, D, paths, [&] {
    if (W >= 1 && H >= 1 && (size_t)W * (size_t)H * (size_t)D <= (size_t)INT32_MAX) return true;
    gsaj_set_error("%s: needs W >= 1, H >= 1 and W * H * D <= INT_MAX (W=%d H=%d D=%d)", who, W, H, D);
    return false;
  });
}

extern "C" int gsaj_motion_stereo_bytes(int W, int H, int D, int paths, size_t *bytes) {
  if (!sweep_sizes_ok("gsaj_motion_stereo_bytes", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (!bytes) {
    gsaj_set_error("gsaj_motion_stereo_bytes: bytes is required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  SweepWS ws;
  *bytes = sweep_carve(Carver(nullptr, BASE_AS_GIVEN), W, H, D, &ws);
  return GSAJ_OK;
}

extern "C" int gsaj_debug_motion_stereo_offsets(int W, int H, int D, int paths, size_t *pc_off, size_t *cost_off, size_t *sum_off) {
  if (!sweep_sizes_ok("gsaj_debug_motion_stereo_offsets", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  SweepWS ws;
  sweep_carve(Carver(nullptr, BASE_AS_GIVEN), W, H, D, &ws, pc_off, cost_off, sum_off);
  return GSAJ_OK;
}

template <int D>
static hipError_t sweep_launch(int stages, const SweepCam &cam, const uint8_t *ref, size_t ref_stride, const uint8_t *src, size_t src_stride, int r,
                               int P1, int P2, int paths, int outside_cost, const SweepWS &ws, const SweepWinner &wp, hipStream_t s) {
  const int W = cam.W, H = cam.H;
  const size_t n = (size_t)W * H;
  if (stages & GSAJ_SWEEP_STAGE_COST) {
    hipLaunchKernelGGL(k_sweep_grad, dim3((unsigned)((n + SGM_BLOCK - 1) / SGM_BLOCK), 2), dim3(SGM_BLOCK), 0, s, W, H, ref, ref_stride, src,
                       src_stride, ws.gr, ws.gs);
    hipLaunchKernelGGL(k_sweep_pixel_cost<D>, dim3((unsigned)((n * D + SGM_BLOCK - 1) / SGM_BLOCK)), dim3(SGM_BLOCK), 0, s, cam, outside_cost,
                       ws.gr, ws.gs, ws.pc);
    constexpr int XB = SGM_BLOCK / D;
    hipLaunchKernelGGL(k_sweep_box<D>, dim3((unsigned)((W + XB - 1) / XB), (unsigned)((H + SGM_BAND - 1) / SGM_BAND)), dim3(SGM_BLOCK), 0, s, W,
                       H, r, ws.pc, ws.C);
  }
  if (stages & GSAJ_SWEEP_STAGE_PATHS) {
    const hipError_t e = launch_stereo_paths(D, W, H, 0, P1, P2, paths, ws.C, ws.S, s);   // zeroes S on the stream first
    if (e != hipSuccess) return e;
  }
  if (stages & GSAJ_SWEEP_STAGE_WINNER) {
    hipLaunchKernelGGL(k_sweep_winner<D>, dim3((unsigned)((n + SgmGroup<D>::GROUPS - 1) / SgmGroup<D>::GROUPS)), dim3(SGM_BLOCK), 0, s, cam, wp);
  }
  return hipGetLastError();
}

static bool sweep_finite(float x) { return x - x == 0.f; }

extern "C" int gsaj_motion_stereo(int W, int H, const uint8_t *ref, size_t ref_stride, const uint8_t *src, size_t src_stride, float fx, float fy,
                                  float cx, float cy, const float *ref_w2c, const float *src_w2c, float w_min, float w_max, int D, int r, int P1,
                                  int P2, int paths, int uniqueness, int outside_cost, int stages, void *workspace, size_t workspace_bytes,
                                  int16_t *idx16, float *out_depth, void *stream) {
  if (!sweep_sizes_ok("gsaj_motion_stereo", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (!sgm_params_ok("gsaj_motion_stereo", r, SWEEP_MAX_R, P1, P2, uniqueness)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (outside_cost < 0 || outside_cost > 240) {
    gsaj_set_error("gsaj_motion_stereo: outside_cost must lie in [0, 240] (outside_cost=%d)", outside_cost);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!(fx > 0.f) || !(fy > 0.f) || !sweep_finite(fx) || !sweep_finite(fy) || !sweep_finite(cx) || !sweep_finite(cy)) {
    gsaj_set_error("gsaj_motion_stereo: fx and fy must be positive and finite, cx and cy finite (fx=%g fy=%g cx=%g cy=%g)", fx, fy, cx, cy);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!sweep_finite(w_min) || !sweep_finite(w_max) || w_min < 0.f || !(w_max > w_min)) {
    gsaj_set_error("gsaj_motion_stereo: needs finite 0 <= w_min < w_max (w_min=%g w_max=%g)", w_min, w_max);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  SweepWS ws;
  const size_t need = sweep_carve(Carver(workspace, BASE_AS_GIVEN), W, H, D, &ws);   // (arithmetic only: a null base is refused below)
  SgmBuffers b;
  b.required = ref && src && ref_w2c && src_w2c && workspace && idx16; b.required_names = "ref, src, ref_w2c, src_w2c, workspace and idx16";
  b.image[0] = "ref"; b.image[1] = "src"; b.stride[0] = ref_stride; b.stride[1] = src_stride;
  b.workspace = workspace; b.workspace_bytes = workspace_bytes; b.need = need; b.size_fn = "gsaj_motion_stereo_bytes";
  b.out16 = idx16; b.out_depth = out_depth; b.aligned_names = "idx16 2-byte, out_depth and the poses 4-byte";
  b.others_aligned = reinterpret_cast<size_t>(ref_w2c) % 4 == 0 && reinterpret_cast<size_t>(src_w2c) % 4 == 0;
  const int rc = sgm_buffers_ok("gsaj_motion_stereo", W, &stages, SWEEP_STAGES, b);
  if (rc != GSAJ_OK) return rc;
  SweepCam cam;
  cam.W = W; cam.H = H; cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.w_min = w_min;
  cam.step = (w_max - w_min) / (float)(D - 1);
  cam.ref_w2c = ref_w2c; cam.src_w2c = src_w2c;
  SweepWinner wp;
  wp.uniqueness = uniqueness; wp.S = ws.S; wp.idx16 = idx16; wp.depth = out_depth;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = sgm_for_d(D, [&](auto d) {
    return sweep_launch<decltype(d)::value>(stages, cam, ref, ref_stride, src, src_stride, r, P1, P2, paths, outside_cost, ws, wp, s);
  });
  GSAJ_HIP_CHECK(e);
  return GSAJ_OK;
}

extern "C" int gsaj_grey_u8(int W, int H, const float *color, uint8_t *out, size_t out_stride, void *stream) {
  if (W < 1 || H < 1 || (size_t)W * (size_t)H > (size_t)INT32_MAX) {
    gsaj_set_error("gsaj_grey_u8: needs W >= 1, H >= 1 and W * H <= INT_MAX (W=%d H=%d)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!color || !out || out_stride < (size_t)W || reinterpret_cast<size_t>(color) % 4 != 0) {
    gsaj_set_error("gsaj_grey_u8: color (4-byte aligned) and out are required, out_stride >= W (out_stride=%zu W=%d)", out_stride, W);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const size_t n = (size_t)W * H;
  hipLaunchKernelGGL(k_sweep_grey_u8, dim3((unsigned)((n + SGM_BLOCK - 1) / SGM_BLOCK)), dim3(SGM_BLOCK), 0, (hipStream_t)stream, W, H, color, out,
                     out_stride);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
