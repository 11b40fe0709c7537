// eval.hip -- rendering quality of one frame on the device: masked, clamped PSNR, SSIM of the clamped image and the 8-bit picture,
// one table row per frame and no host read (gfx950).  Semantics: include/gsaj.h; the reference forms them per frame with two
// boolean-index gathers, a dozen elementwise launches and three .item() calls (utils/eval_utils.py:141-160).
//
// Three launches on the caller's stream:
//   k_eval_pixels    every element once: x = clamp(image, 0, 1) into the workspace (what SSIM then reads), the byte if asked for,
//                    and per workgroup of EV_RUN elements ONE {fp64 sum of masked squared errors, count of masked elements}.
//                    Lanes take 16 bytes of image, gt and x at a time where the host found both inputs 16-byte aligned (the
//                    workspace always is), consecutive dwords otherwise; the choice is made per call.
//   gsaj_ssim_forward  the public entry point, N = 1, on its own slice of the workspace.
//   k_eval_finalize  one workgroup: the partials in block order, 256 at a time, then the scalar tail and the row.
// No float atomics, no ticket of its own; every sum has a fixed order, so a frame gives the same bits every time.
// This file is compiled with -ffp-contract=off: d = x - gt and q = d * d are two roundings, as the reference's two tensor operations.
#include <limits.h>

#include "gsaj_common.h"
#include "wave_reduce.h"

#define EV_BLOCK 256
#define EV_VEC 4
#define EV_RUN (EV_BLOCK * EV_VEC)  // elements per workgroup

struct EvalPartial {  // one per workgroup of k_eval_pixels
  double sse;
  uint32_t n, pad;
};

struct EvalLayout {  // the workspace: clamped image [C,H,W] | partials [nblk] | the SSIM pair | gsaj_ssim_workspace_bytes(1, C, W, H)
  float *clamped;
  EvalPartial *partials;
  float *ssim_out;  // [2]: gsaj_ssim_forward's per-image mean and overall mean (N = 1: the same value twice)
  void *ssim_ws;
};

static size_t eval_nblk(size_t total) { return (total + EV_RUN - 1) / EV_RUN; }

static size_t eval_carve(Carver c, int C, int W, int H, EvalLayout *L) {
  const size_t total = (size_t)C * W * H;
  L->clamped = c.take<float>(total);
  L->partials = c.take<EvalPartial>(eval_nblk(total));
  L->ssim_out = c.take<float>(2);
  L->ssim_ws = c.pack<char>(gsaj_ssim_workspace_bytes(1, C, W, H));  // (last, not rounded)
  return c.used();
}

struct EvalPixelParams {
  const float *image, *gt;
  float *clamped;
  uint8_t *u8;  // [H,W,C] or NULL
  EvalPartial *partials;
  unsigned total, HW, C;
  int reverse;
};

// WIDE: lane t of the workgroup takes elements 4 t .. 4 t + 3 of the run, 16 bytes at a time; otherwise element k * 256 + t in
// round k, a dword at a time.  Either way a wave's accesses are consecutive.
template <bool WIDE>
__global__ __launch_bounds__(EV_BLOCK) void k_eval_pixels(EvalPixelParams p) {
  __shared__ double wsse[EV_BLOCK / 64];
  __shared__ uint32_t wcnt[EV_BLOCK / 64];
  const unsigned base = blockIdx.x * (unsigned)EV_RUN;  // (total <= INT_MAX: no overflow, the last run may pass total by < EV_RUN)
  unsigned e[EV_VEC];
  float v[EV_VEC], g[EV_VEC], x[EV_VEC];
  bool wide = false;
  if constexpr (WIDE) {
    const unsigned e0 = base + threadIdx.x * EV_VEC;
#pragma unroll
    for (int k = 0; k < EV_VEC; k++) e[k] = e0 + k;
    wide = e0 + EV_VEC <= p.total;
    if (wide) {
      const float4 v4 = *reinterpret_cast<const float4 *>(p.image + e0), g4 = *reinterpret_cast<const float4 *>(p.gt + e0);
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
      g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < EV_VEC; k++) e[k] = base + k * EV_BLOCK + threadIdx.x;
  }
  if (!wide) {
#pragma unroll
    for (int k = 0; k < EV_VEC; k++) {
      const bool in = e[k] < p.total;
      v[k] = in ? p.image[e[k]] : 0.f;
      g[k] = in ? p.gt[e[k]] : 0.f;  // (gt = 0: outside the mask)
    }
  }
  double sse = 0.0;
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < EV_VEC; k++) {
    // torch.clamp: a NaN stays a NaN (both comparisons are false)
    x[k] = v[k] < 0.f ? 0.f : (v[k] > 1.f ? 1.f : v[k]);
    const float d = x[k] - g[k];
    const float q = d * d;
    if (g[k] > 0.f) {
      sse += (double)q;
      n++;
    }
  }
  if (wide) {
    *reinterpret_cast<float4 *>(p.clamped + e[0]) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < EV_VEC; k++)
      if (e[k] < p.total) p.clamped[e[k]] = x[k];
  }
  if (p.u8) {
#pragma unroll
    for (int k = 0; k < EV_VEC; k++) {
      if (e[k] >= p.total) continue;
      const unsigned c = e[k] / p.HW, pix = e[k] - c * p.HW;
      const unsigned cb = p.reverse ? p.C - 1u - c : c;
      const float s = x[k] * 255.0f;  // in [0, 255] or NaN; the conversion truncates
      p.u8[(size_t)pix * p.C + cb] = s == s ? (uint8_t)(unsigned)s : (uint8_t)0;
    }
  }
  // workgroup partial: wave butterflies, then the four waves in order
  sse = wave_sum(sse);
  n = wave_sum(n);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { wsse[wave] = sse; wcnt[wave] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wsse[0];
    uint32_t c = wcnt[0];
    for (int w = 1; w < EV_BLOCK / 64; w++) { s += wsse[w]; c += wcnt[w]; }
    EvalPartial out;
    out.sse = s; out.n = c; out.pad = 0u;
    p.partials[blockIdx.x] = out;
  }
}

struct EvalFinalParams {
  const EvalPartial *partials;
  const float *ssim_out;
  float *out_row;
  uint32_t *out_count;
  unsigned nblk, total;
};

__global__ __launch_bounds__(EV_BLOCK) void k_eval_finalize(EvalFinalParams p) {
  __shared__ double wsse[EV_BLOCK / 64];
  __shared__ uint32_t wcnt[EV_BLOCK / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double sse = 0.0;  // (thread 0's are the totals)
  uint32_t n = 0;
  for (unsigned b0 = 0; b0 < p.nblk; b0 += EV_BLOCK) {  // 256 partials at a time, in block order
    const unsigned b = b0 + threadIdx.x;
    double s = 0.0;
    uint32_t c = 0;
    if (b < p.nblk) { s = p.partials[b].sse; c = p.partials[b].n; }
    s = wave_sum(s);
    c = wave_sum(c);
    if (lane == 0) { wsse[wave] = s; wcnt[wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < EV_BLOCK / 64; w++) { sse += wsse[w]; n += wcnt[w]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float mse = (float)(sse / (double)n);  // n = 0: 0 / 0 = NaN
    const float psnr = 20.f * log10f(1.0f / sqrtf(mse));  // mse = 0: +inf
    p.out_row[0] = psnr;
    p.out_row[1] = p.ssim_out[1];
    p.out_row[2] = mse;
    p.out_row[3] = (float)((double)n / (double)p.total);
    *p.out_count = n;
  }
}

static bool eval_dims_ok(int C, int W, int H) {
  return C >= 1 && W >= 1 && H >= 1 && (unsigned long long)C * (unsigned long long)W * (unsigned long long)H <= (unsigned long long)INT_MAX;
}

extern "C" size_t gsaj_eval_workspace_bytes(int C, int W, int H) {
  if (!eval_dims_ok(C, W, H)) return 0;
  EvalLayout L;
  return eval_carve(Carver(nullptr, ALIGN_BASE), C, W, H, &L) + 256;
}

extern "C" int gsaj_eval_frame(int C, int W, int H, int flags, const float *image, const float *gt, float *out_row,
                               uint32_t *out_count, uint8_t *image_u8, void *eval_ws, void *stream) {
  if (!eval_dims_ok(C, W, H) || !image || !gt || !out_row || !out_count || !eval_ws) {
    gsaj_set_error("gsaj_eval_frame: invalid argument (C=%d W=%d H=%d, each >= 1 and C * W * H <= INT_MAX; image, gt, out_row, "
                   "out_count and eval_ws are required)", C, W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (flags & ~GSAJ_EVAL_REVERSE_CHANNELS) {
    gsaj_set_error("gsaj_eval_frame: invalid argument (flags has bits outside GSAJ_EVAL_REVERSE_CHANNELS)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const hipStream_t s = (hipStream_t)stream;
  EvalLayout L;
  eval_carve(Carver(eval_ws, ALIGN_BASE), C, W, H, &L);
  const size_t total = (size_t)C * W * H, nblk = eval_nblk(total);
  EvalPixelParams p;
  p.image = image; p.gt = gt; p.clamped = L.clamped; p.u8 = image_u8; p.partials = L.partials;
  p.total = (unsigned)total; p.HW = (unsigned)W * (unsigned)H; p.C = (unsigned)C;
  p.reverse = (flags & GSAJ_EVAL_REVERSE_CHANNELS) ? 1 : 0;
  const bool aligned = ((((uintptr_t)image) | ((uintptr_t)gt)) & 15u) == 0;
  if (aligned)
    hipLaunchKernelGGL(k_eval_pixels<true>, dim3((unsigned)nblk), dim3(EV_BLOCK), 0, s, p);
  else
    hipLaunchKernelGGL(k_eval_pixels<false>, dim3((unsigned)nblk), dim3(EV_BLOCK), 0, s, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  const int rc = gsaj_ssim_forward(1, C, W, H, L.clamped, gt, L.ssim_out, nullptr, L.ssim_ws, stream);
  if (rc != GSAJ_OK) return rc;
  EvalFinalParams f;
  f.partials = L.partials; f.ssim_out = L.ssim_out; f.out_row = out_row; f.out_count = out_count;
  f.nblk = (unsigned)nblk; f.total = (unsigned)total;
  hipLaunchKernelGGL(k_eval_finalize, dim3(1), dim3(EV_BLOCK), 0, s, f);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
