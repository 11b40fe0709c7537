// ssim.hip -- SSIM (11x11 Gaussian window, sigma 1.5, zero padding) and the L1 + D-SSIM loss of colour refinement, forward
// and backward w.r.t. the first image, over [N,C,H,W] fp32 planes (gfx950).
//
// Semantics: reference gaussian_splatting/utils/loss_utils.py:42-101 (ssim / _ssim: five depthwise F.conv2d with
// padding 5, C1 = 0.01^2, C2 = 0.03^2, sigma^2 = blur(x*x) - mu^2 in fp32) and utils/slam_backend.py:320-352 (colour refinement:
// (1 - lambda) * l1_loss + lambda * (1 - ssim)).  The 2-D window is the outer product of the 1-D one, so the blur is done
// separably (horizontal 11 taps, then vertical): it differs from the reference's 2-D conv by rounding only.
//
// Forward (k_ssim_fwd): one workgroup per 32x16 output tile of one plane.  The tile of img and gt plus its 5-pixel halo is
// staged in LDS (zeros outside the image), the five blurred quantities x, y, x^2, y^2, xy are formed, and per pixel
// S = A B / (C D) together with the three partials of S w.r.t. the blurred quantities that depend on img -- dS/dmu1,
// dS/dE[x^2], dS/dE[xy] -- which the backward consumes from the workspace.  Per-workgroup sums of S and |x - y| are reduced
// in a fixed order by the last-arriving workgroup (last_block.h: no float atomics, bit-reproducible).
// Backward (k_ssim_bwd): the same tile geometry blurs the three partial maps (zeros outside: the adjoint of a zero-padded
// correlation with a symmetric window is the same correlation) and forms
//   dL/dx = w_n (blur(dS/dmu1) + 2 x blur(dS/dE[x^2]) + y blur(dS/dE[xy])) + l1_w sign(x - y).
// LDS: lane = column in every pass, so each 32-lane half of a wave reads 32 consecutive dwords of one row: conflict-free
// without padding (ds_read_b32 banks are dword % 32, serviced per 32-lane half).
#include "gsaj_common.h"
#include "last_block.h"
#include "wave_reduce.h"

#define SSIM_TW 32           // output tile width (= the 32 lanes of a wave half)
#define SSIM_TH 16           // output tile height
#define SSIM_R 5             // window radius
#define SSIM_SW (SSIM_TW + 2 * SSIM_R)  // 42 staged columns
#define SSIM_SH (SSIM_TH + 2 * SSIM_R)  // 26 staged rows
#define SSIM_BLOCK 256

// gaussian(11, 1.5) exactly as the reference builds it: exp() in double, stored to a float32 tensor, normalised in float32
constexpr float kSsimWin[11] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
    0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
#define SSIM_C1 (0.01f * 0.01f)
#define SSIM_C2 (0.03f * 0.03f)

struct SsimLayout {  // the workspace: ticket | out area | per-workgroup partials [nblk][4] | partial maps [3][planes*H*W]
  uint32_t *ticket;
  float *partials;
  float *dmu, *dxx, *dxy;
};

static size_t ssim_nblk(int N, int C, int W, int H) {
  return (size_t)((W + SSIM_TW - 1) / SSIM_TW) * (size_t)((H + SSIM_TH - 1) / SSIM_TH) * (size_t)N * (size_t)C;
}

static size_t ssim_carve(Carver c, int N, int C, int W, int H, SsimLayout *L) {
  const size_t plane = (size_t)N * C * W * H;
  L->ticket = c.take<uint32_t>(1);  // the caller zeroes the workspace once, when it allocates it; the last workgroup resets it
  L->partials = c.take<float>(ssim_nblk(N, C, W, H) * 4);
  L->dmu = c.pack<float>(plane);    // (the three maps follow each other unpadded)
  L->dxx = c.pack<float>(plane);
  L->dxy = c.pack<float>(plane);
  return c.used();
}

struct SsimTile {
  int plane, x0, y0;
};

__device__ __forceinline__ SsimTile ssim_tile(int W, int H) {
  const unsigned gx = (W + SSIM_TW - 1) / SSIM_TW, gy = (H + SSIM_TH - 1) / SSIM_TH;
  const unsigned b = blockIdx.x, per = gx * gy, r = b % per;
  SsimTile t;
  t.plane = (int)(b / per);
  t.x0 = (int)(r % gx) * SSIM_TW;
  t.y0 = (int)(r / gx) * SSIM_TH;
  return t;
}

// stage the (SSIM_SH x SSIM_SW) window of K [H,W] planes into LDS, zeros outside the image.  Every load of the window is issued
// before the first LDS write, so a workgroup waits for one global-memory latency, not one per staged row band.
template <int K>
__device__ __forceinline__ void ssim_stage(float (*const dst[K])[SSIM_SW], const float *const src[K], int W, int H, int x0, int y0) {
  constexpr int NIT = (SSIM_SH * SSIM_SW + SSIM_BLOCK - 1) / SSIM_BLOCK;
  float v[K][NIT];
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int i = threadIdx.x + it * SSIM_BLOCK, r = i / SSIM_SW, c = i - r * SSIM_SW;
    const int gx = x0 - SSIM_R + c, gy = y0 - SSIM_R + r;
    const bool in = i < SSIM_SH * SSIM_SW && gx >= 0 && gx < W && gy >= 0 && gy < H;
#pragma unroll
    for (int k = 0; k < K; k++) v[k][it] = in ? src[k][(size_t)gy * W + gx] : 0.f;
  }
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int i = threadIdx.x + it * SSIM_BLOCK, r = i / SSIM_SW, c = i - r * SSIM_SW;
    if (i < SSIM_SH * SSIM_SW) {
#pragma unroll
      for (int k = 0; k < K; k++) dst[k][r][c] = v[k][it];
    }
  }
}

struct SsimFwdParams {
  int N, C, W, H;
  const float *img, *gt;
  float *ssim_map;   // [N,C,H,W] or NULL
  SsimLayout L;
  float *ssim_out;   // [N+1] or NULL: per-image mean of S, then the mean over everything
  float *refine_out; // [3] or NULL: (1 - lambda) L1 + lambda (1 - SSIM), L1, SSIM
  float lambda;
};

__global__ __launch_bounds__(SSIM_BLOCK) void k_ssim_fwd(SsimFwdParams p) {
  __shared__ float sx[SSIM_SH][SSIM_SW], sy[SSIM_SH][SSIM_SW];
  __shared__ float hs[5][SSIM_SH][SSIM_TW];
  __shared__ float red[2][SSIM_BLOCK / 64];
  __shared__ double fin[2][SSIM_BLOCK / 64];
  __shared__ bool is_last;
  const SsimTile t = ssim_tile(p.W, p.H);
  const size_t HW = (size_t)p.W * p.H, off = (size_t)t.plane * HW;
  {
    float(*const dst[2])[SSIM_SW] = {sx, sy};
    const float *const src[2] = {p.img + off, p.gt + off};
    ssim_stage<2>(dst, src, p.W, p.H, t.x0, t.y0);
  }
  __syncthreads();
  // horizontal pass: SSIM_SH rows x SSIM_TW columns, five quantities
  for (int i = threadIdx.x; i < SSIM_SH * SSIM_TW; i += SSIM_BLOCK) {
    const int r = i / SSIM_TW, c = i - r * SSIM_TW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float w = kSsimWin[k], x = sx[r][c + k], y = sy[r][c + k];
      a0 += w * x;
      a1 += w * y;
      a2 += w * (x * x);
      a3 += w * (y * y);
      a4 += w * (x * y);
    }
    hs[0][r][c] = a0; hs[1][r][c] = a1; hs[2][r][c] = a2; hs[3][r][c] = a3; hs[4][r][c] = a4;
  }
  __syncthreads();
  // vertical pass + the per-pixel SSIM terms: SSIM_TH x SSIM_TW outputs, two per thread
  float s[2] = {0.f, 0.f};  // sums of S and of |x - y|
#pragma unroll
  for (int q = 0; q < (SSIM_TH * SSIM_TW) / SSIM_BLOCK; q++) {
    const int i = threadIdx.x + q * SSIM_BLOCK, r = i / SSIM_TW, c = i - r * SSIM_TW;
    const int gx = t.x0 + c, gy = t.y0 + r;
    if (gx >= p.W || gy >= p.H) continue;
    float m1 = 0.f, m2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float w = kSsimWin[k];
      m1 += w * hs[0][r + k][c];
      m2 += w * hs[1][r + k][c];
      exx += w * hs[2][r + k][c];
      eyy += w * hs[3][r + k][c];
      exy += w * hs[4][r + k][c];
    }
    const float m1s = m1 * m1, m2s = m2 * m2, m12 = m1 * m2;
    const float s1 = exx - m1s, s2 = eyy - m2s, s12 = exy - m12;
    const float A = 2.f * m12 + SSIM_C1, B = 2.f * s12 + SSIM_C2;
    const float Cc = m1s + m2s + SSIM_C1, D = s1 + s2 + SSIM_C2;
    const float CD = Cc * D;
    const float S = (A * B) / CD;
    const size_t pix = off + (size_t)gy * p.W + gx;
    if (p.ssim_map) p.ssim_map[pix] = S;
    p.L.dmu[pix] = 2.f * m2 * (B - A) / CD + 2.f * m1 * S * (1.f / D - 1.f / Cc);
    p.L.dxx[pix] = -S / D;
    p.L.dxy[pix] = 2.f * A / CD;
    s[0] += S;
    s[1] += fabsf(sx[r + SSIM_R][c + SSIM_R] - sy[r + SSIM_R][c + SSIM_R]);
  }
  // the workgroup's two partials (in a 4-float slot: one coherent load each), handed to the last workgroup (last_block.h)
  block_fold<SSIM_BLOCK / 64, 2>(s, red, lane_add());
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 2; c++) lb_publish(&p.L.partials[(size_t)blockIdx.x * 4 + c], s[c]);
  }
  if (!lb_arrive(p.L.ticket, &is_last)) return;
  // per image: its C * tiles workgroups are contiguous in blockIdx order; fp64, fixed tree
  const unsigned per_img = gridDim.x / (unsigned)p.N;
  double tot_s = 0.0, tot_l1 = 0.0;
  for (int n = 0; n < p.N; n++) {
    double acc[2] = {0.0, 0.0};
    for (unsigned b = threadIdx.x; b < per_img; b += SSIM_BLOCK) {
      const uint4 u = lb_load_x4(p.L.partials + ((size_t)n * per_img + b) * 4);
      acc[0] += (double)__uint_as_float(u.x);
      acc[1] += (double)__uint_as_float(u.y);
    }
    block_fold<SSIM_BLOCK / 64, 2>(acc, fin, lane_add());
    if (threadIdx.x == 0) {
      if (p.ssim_out) p.ssim_out[n] = (float)(acc[0] / ((double)p.C * (double)HW));
      tot_s += acc[0];
      tot_l1 += acc[1];
    }
    __syncthreads();  // (fin is written again for the next image)
  }
  if (threadIdx.x == 0) {
    const double cnt = (double)p.N * (double)p.C * (double)HW;
    const double ssim = tot_s / cnt, l1 = tot_l1 / cnt;
    if (p.ssim_out) p.ssim_out[p.N] = (float)ssim;
    if (p.refine_out) {
      p.refine_out[0] = (float)((1.0 - (double)p.lambda) * l1 + (double)p.lambda * (1.0 - ssim));
      p.refine_out[1] = (float)l1;
      p.refine_out[2] = (float)ssim;
    }
    lb_reset(p.L.ticket);
  }
}

struct SsimBwdParams {
  int N, C, W, H;
  const float *img, *gt;
  const float *dL_dssim;  // [N+1] (device) or NULL: then every pixel's dL/dS is w_const
  float w_const, l1_w;
  float *dL_dimg;
  SsimLayout L;
};

__global__ __launch_bounds__(SSIM_BLOCK) void k_ssim_bwd(SsimBwdParams p) {
  __shared__ float sm[3][SSIM_SH][SSIM_SW];
  __shared__ float hs[3][SSIM_SH][SSIM_TW];
  const SsimTile t = ssim_tile(p.W, p.H);
  const size_t HW = (size_t)p.W * p.H, off = (size_t)t.plane * HW;
  {
    float(*const dst[3])[SSIM_SW] = {sm[0], sm[1], sm[2]};
    const float *const src[3] = {p.L.dmu + off, p.L.dxx + off, p.L.dxy + off};
    ssim_stage<3>(dst, src, p.W, p.H, t.x0, t.y0);
  }
  float w_n = p.w_const;
  if (p.dL_dssim) {
    const int n = t.plane / p.C;
    const double chw = (double)p.C * (double)HW;
    w_n = (float)((double)p.dL_dssim[n] / chw + (double)p.dL_dssim[p.N] / (chw * (double)p.N));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_SH * SSIM_TW; i += SSIM_BLOCK) {
    const int r = i / SSIM_TW, c = i - r * SSIM_TW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float w = kSsimWin[k];
      a0 += w * sm[0][r][c + k];
      a1 += w * sm[1][r][c + k];
      a2 += w * sm[2][r][c + k];
    }
    hs[0][r][c] = a0; hs[1][r][c] = a1; hs[2][r][c] = a2;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < (SSIM_TH * SSIM_TW) / SSIM_BLOCK; q++) {
    const int i = threadIdx.x + q * SSIM_BLOCK, r = i / SSIM_TW, c = i - r * SSIM_TW;
    const int gx = t.x0 + c, gy = t.y0 + r;
    if (gx >= p.W || gy >= p.H) continue;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
      const float w = kSsimWin[k];
      b0 += w * hs[0][r + k][c];
      b1 += w * hs[1][r + k][c];
      b2 += w * hs[2][r + k][c];
    }
    const size_t pix = off + (size_t)gy * p.W + gx;
    const float x = p.img[pix], y = p.gt[pix], d = x - y;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);  // torch abs backward: sign(0) = 0
    p.dL_dimg[pix] = w_n * (b0 + 2.f * x * b1 + y * b2) + p.l1_w * sg;
  }
}

extern "C" size_t gsaj_ssim_workspace_bytes(int N, int C, int W, int H) {
  if (N <= 0 || C <= 0 || W <= 0 || H <= 0) return 0;
  SsimLayout L;
  return ssim_carve(Carver(nullptr, ALIGN_BASE), N, C, W, H, &L) + 256;
}

static bool ssim_dims_ok(int N, int C, int W, int H) {
  return N >= 1 && C >= 1 && W >= 1 && H >= 1 && ssim_nblk(N, C, W, H) <= 0x7fffffffu &&
         (size_t)N * C * W * H <= ((size_t)1 << 40);
}

static int launch_ssim_fwd(int N, int C, int W, int H, const float *img, const float *gt, float *ssim_out, float *ssim_map,
                           float *refine_out, float lambda, void *ws, hipStream_t s) {
  SsimFwdParams p;
  p.N = N; p.C = C; p.W = W; p.H = H; p.img = img; p.gt = gt; p.ssim_map = ssim_map;
  ssim_carve(Carver(ws, ALIGN_BASE), N, C, W, H, &p.L);
  p.ssim_out = ssim_out; p.refine_out = refine_out; p.lambda = lambda;
  hipLaunchKernelGGL(k_ssim_fwd, dim3((unsigned)ssim_nblk(N, C, W, H)), dim3(SSIM_BLOCK), 0, s, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

static int launch_ssim_bwd(int N, int C, int W, int H, const float *img, const float *gt, const float *dL_dssim, float w_const,
                           float l1_w, float *dL_dimg, void *ws, hipStream_t s) {
  SsimBwdParams p;
  p.N = N; p.C = C; p.W = W; p.H = H; p.img = img; p.gt = gt; p.dL_dssim = dL_dssim; p.w_const = w_const; p.l1_w = l1_w;
  p.dL_dimg = dL_dimg;
  ssim_carve(Carver(ws, ALIGN_BASE), N, C, W, H, &p.L);
  hipLaunchKernelGGL(k_ssim_bwd, dim3((unsigned)ssim_nblk(N, C, W, H)), dim3(SSIM_BLOCK), 0, s, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_ssim_forward(int N, int C, int W, int H, const float *img, const float *gt, float *ssim_out, float *ssim_map,
                                 void *ws, void *stream) {
  if (!ssim_dims_ok(N, C, W, H) || !img || !gt || !ssim_out || !ws) {
    gsaj_set_error("gsaj_ssim_forward: invalid argument (N=%d C=%d W=%d H=%d; img, gt, ssim_out and ws are required)", N, C, W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return launch_ssim_fwd(N, C, W, H, img, gt, ssim_out, ssim_map, nullptr, 0.f, ws, (hipStream_t)stream);
}

extern "C" int gsaj_ssim_backward(int N, int C, int W, int H, const float *img, const float *gt, const float *dL_dssim,
                                  float *dL_dimg, void *ws, void *stream) {
  if (!ssim_dims_ok(N, C, W, H) || !img || !gt || !dL_dssim || !dL_dimg || !ws) {
    gsaj_set_error("gsaj_ssim_backward: invalid argument (N=%d C=%d W=%d H=%d; img, gt, dL_dssim, dL_dimg and ws are required)", N,
                   C, W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return launch_ssim_bwd(N, C, W, H, img, gt, dL_dssim, 0.f, 0.f, dL_dimg, ws, (hipStream_t)stream);
}

extern "C" size_t gsaj_refine_loss_workspace_bytes(int W, int H) { return gsaj_ssim_workspace_bytes(1, 3, W, H); }

extern "C" int gsaj_refine_loss_seeds(int W, int H, float lambda_dssim, const float *image, const float *gt, float *dL_dcolor,
                                      float *out_scalars, void *ws, void *stream) {
  if (!ssim_dims_ok(1, 3, W, H) || !image || !gt || !dL_dcolor || !out_scalars || !ws || !(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) {
    gsaj_set_error("gsaj_refine_loss_seeds: invalid argument (W=%d H=%d lambda_dssim=%g; image, gt, dL_dcolor, out_scalars and ws "
                   "are required, lambda_dssim in [0, 1])", W, H, (double)lambda_dssim);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const hipStream_t s = (hipStream_t)stream;
  const float n = 3.f * (float)W * (float)H;
  const int rc = launch_ssim_fwd(1, 3, W, H, image, gt, nullptr, nullptr, out_scalars, lambda_dssim, ws, s);
  if (rc != GSAJ_OK) return rc;
  // loss = (1 - lambda) mean|x - y| + lambda (1 - mean S): dL/dS = -lambda / n at every pixel, the L1 weight (1 - lambda) / n
  return launch_ssim_bwd(1, 3, W, H, image, gt, nullptr, -lambda_dssim / n, (1.f - lambda_dssim) / n, dL_dcolor, ws, s);
}
