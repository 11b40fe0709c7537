// frame.hip -- per-frame image operations on the device (gfx950): the tracking gradient mask of an incoming frame.
//
// Semantics: reference utils/slam_utils.py:4-38 (image_gradient: Scharr filter normalised by 32 on the reflect-padded gray image;
// image_gradient_mask: all nine padded neighbours |p| > 0.01) and utils/camera_utils.py:115-144 (Camera.compute_grad_mask:
// intensity = sqrt(gv^2 + gh^2), then either intensity > median * edge_threshold over the whole frame, or -- dataset type
// "replica" -- the same per block of a 32 x 32 grid of int(H/32) x int(W/32) blocks, written back as float 0 / 1 into the
// intensity image, whose leftover rows and columns keep their intensity).  include/gsaj.h states every quirk.
//
// MI355X design: a frame is a few MB, so the work is launch- and latency-bound.
//   * k_gm_intensity: a 64 x 16 tile per workgroup (lane = column, four rows per wave); the gray tile + 1-pixel halo is formed
//     from the three planes on load and staged in LDS, so every gray value is computed once and read nine times from LDS.
//   * whole-frame mode: intensity -> workspace, the rank-(N-1)/2 radix select of seed.hip (launch_select_rank_f32), one threshold
//     kernel that reads the selected key from device memory.  No host read, no synchronisation.
//   * block mode: ONE kernel, one workgroup per block.  Gray tile + halo in LDS, the block's intensities as 32-bit keys in LDS
//     (non-negative floats order as their bit patterns), the exact lower median by a most-significant-digit radix select over
//     those keys -- four passes of 8 bits, an LDS histogram of INTEGER counters (LDS float atomics cost hundreds of cycles, DESIGN
//     section 4; and counts are exact, so the result is bit-reproducible) -- then the threshold and the two outputs.  The
//     workgroups of the last block row / column also write the leftover strips.  35 KB of LDS per workgroup: four workgroups
//     (16 waves) per CU.
//
// Built with -ffp-contract=off (csrc/Makefile): each tensor operation of the reference rounds once in fp32, and so does each
// operator here; division and square root are correctly rounded (hipcc's default for fp32).
#include "gsaj_common.h"
#include "wave_reduce.h"
#include <cmath>

#define GM_THREADS 256
#define GM_TW 64                // intensity kernel: tile width (one wave's lanes)
#define GM_TH 16                // ... and height (four rows per wave)
#define GM_GRID 32              // blocks per image side in block mode
#define GM_KEYS_MAX 4096        // largest block in pixels (1920 x 1080: 33 x 60 = 1980)
#define GM_TILE_MAX 4608        // largest block + halo in pixels
#define GM_EPS 0.01f            // image_gradient_mask's eps

// index of a reflect-padded coordinate (edge pixel not repeated); clamped, so that coordinates of a partial tile's unused halo
// stay inside the image
__device__ __forceinline__ int gm_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// image.mean(dim=0): (r + g) + b, then a true division by 3
__device__ __forceinline__ float gm_gray(const float *__restrict__ image, size_t n, size_t i) {
  return __fdiv_rn(__fadd_rn(__fadd_rn(image[i], image[n + i]), image[2 * n + i]), 3.f);
}

__device__ __forceinline__ float gm_three(float a, float b, float c) {  // (3a + 10b) + 3c
  return __fadd_rn(__fadd_rn(__fmul_rn(3.f, a), __fmul_rn(10.f, b)), __fmul_rn(3.f, c));
}

// the intensity of the pixel whose padded 3 x 3 neighbourhood starts at p (row stride `ld`)
__device__ __forceinline__ float gm_intensity(const float *p, int ld) {
  const float p00 = p[0], p01 = p[1], p02 = p[2];
  const float p10 = p[ld], p11 = p[ld + 1], p12 = p[ld + 2];
  const float p20 = p[2 * ld], p21 = p[2 * ld + 1], p22 = p[2 * ld + 2];
  const bool valid = fabsf(p00) > GM_EPS && fabsf(p01) > GM_EPS && fabsf(p02) > GM_EPS && fabsf(p10) > GM_EPS && fabsf(p11) > GM_EPS &&
                     fabsf(p12) > GM_EPS && fabsf(p20) > GM_EPS && fabsf(p21) > GM_EPS && fabsf(p22) > GM_EPS;
  float gv = __fmul_rn(__fsub_rn(gm_three(p00, p01, p02), gm_three(p20, p21, p22)), 0.03125f);
  float gh = __fmul_rn(__fsub_rn(gm_three(p00, p10, p20), gm_three(p02, p12, p22)), 0.03125f);
  if (!valid) gv = gh = 0.f;
  return sqrtf(__fadd_rn(__fmul_rn(gv, gv), __fmul_rn(gh, gh)));
}

// the same from global memory, for the few pixels of the leftover strips
__device__ float gm_intensity_global(const float *__restrict__ image, int W, int H, int x, int y) {
  const size_t n = (size_t)W * H;
  float p[9];
#pragma unroll
  for (int dy = 0; dy < 3; dy++)
#pragma unroll
    for (int dx = 0; dx < 3; dx++)
      p[3 * dy + dx] = gm_gray(image, n, (size_t)gm_reflect(y - 1 + dy, H) * W + gm_reflect(x - 1 + dx, W));
  return gm_intensity(p, 3);
}

// gray tile [th + 2][tw + 2] whose interior starts at (x0, y0), reflected at the image border
__device__ __forceinline__ void gm_stage_tile(const float *__restrict__ image, int W, int H, int x0, int y0, int tw, int th,
                                              float *tile) {
  const size_t n = (size_t)W * H;
  const int ld = tw + 2, count = ld * (th + 2);
  for (int i = threadIdx.x; i < count; i += GM_THREADS) {
    const int ty = i / ld, tx = i - ty * ld;
    tile[i] = gm_gray(image, n, (size_t)gm_reflect(y0 - 1 + ty, H) * W + gm_reflect(x0 - 1 + tx, W));
  }
}

__global__ __launch_bounds__(GM_THREADS) void k_gm_intensity(int W, int H, const float *__restrict__ image, float *__restrict__ out) {
  __shared__ float tile[(GM_TH + 2) * (GM_TW + 2)];
  const int x0 = blockIdx.x * GM_TW, y0 = blockIdx.y * GM_TH;
  gm_stage_tile(image, W, H, x0, y0, GM_TW, GM_TH, tile);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = x0 + lane;
  if (x >= W) return;
#pragma unroll
  for (int r = 0; r < GM_TH / 4; r++) {
    const int ty = wave * (GM_TH / 4) + r, y = y0 + ty;
    if (y < H) out[(size_t)y * W + x] = gm_intensity(tile + ty * (GM_TW + 2) + lane, GM_TW + 2);
  }
}

// whole-frame mode: mask = I > median * edge_threshold; `key` is the select's key of the median (sign bit set: non-negative)
__global__ __launch_bounds__(GM_THREADS) void k_gm_threshold(int n, const float *__restrict__ I, const uint32_t *__restrict__ key,
                                                             float edge_threshold, uint8_t *__restrict__ out_u8,
                                                             float *__restrict__ out_f32) {
  const int i = blockIdx.x * GM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float t = __fmul_rn(__uint_as_float(*key ^ 0x80000000u), edge_threshold);
  const bool keep = I[i] > t;
  out_u8[i] = keep ? 1 : 0;
  if (out_f32) out_f32[i] = keep ? 1.f : 0.f;
}

__device__ __forceinline__ void gm_write_raw(float v, size_t i, uint8_t *__restrict__ out_u8, float *__restrict__ out_f32) {
  out_u8[i] = (uint8_t)(int)fminf(v, 255.f);  // the byte a .to(torch.uint8) of the float tensor holds: truncated
  if (out_f32) out_f32[i] = v;
}

// block mode: workgroup (bx, by) owns block rows [by bh, (by + 1) bh) x columns [bx bw, (bx + 1) bw)
__global__ __launch_bounds__(GM_THREADS) void k_gm_blocks(int W, int H, int bw, int bh, const float *__restrict__ image,
                                                          float edge_threshold, uint8_t *__restrict__ out_u8,
                                                          float *__restrict__ out_f32) {
  __shared__ float tile[GM_TILE_MAX];
  __shared__ uint32_t keys[GM_KEYS_MAX];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t s_prefix, s_rank;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * bw, y0 = blockIdx.y * bh, n = bw * bh, ld = bw + 2;
  gm_stage_tile(image, W, H, x0, y0, bw, bh, tile);
  if (tid == 0) {
    s_prefix = 0u;
    s_rank = (uint32_t)(n - 1) / 2u;  // torch.median: the LOWER median
  }
  __syncthreads();
  for (int i = tid; i < n; i += GM_THREADS) {
    const int ty = i / bw, tx = i - ty * bw;
    keys[i] = __float_as_uint(gm_intensity(tile + ty * ld + tx, ld));  // >= +0: ordered as unsigned integers
  }
  // most-significant-digit radix select: which digit holds the wanted rank among the keys that match the prefix so far?
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0u;
    __syncthreads();  // (also: keys written, s_prefix / s_rank of the previous pass visible)
    const uint32_t prefix = s_prefix, rank = s_rank;
    for (int i = tid; i < n; i += GM_THREADS) {
      const uint32_t k = keys[i];
      if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = hist[tid];
    const uint32_t excl = block_excl_scan_add<GM_THREADS / 64>(c, wsum);
    if (rank >= excl && rank < excl + c) {  // exactly one thread: the counts add up to more than the rank
      s_prefix = prefix | ((uint32_t)tid << shift);
      s_rank = rank - excl;
    }
    // (the next pass's first barrier orders these writes before their reads; hist is re-zeroed by the thread that read it)
  }
  __syncthreads();
  const float t = __fmul_rn(__uint_as_float(s_prefix), edge_threshold);
  const bool any = t < 1.f;  // the reference writes the ones first and then zeroes everything <= t, the ones included
  for (int i = tid; i < n; i += GM_THREADS) {
    const int ty = i / bw, tx = i - ty * bw;
    const bool keep = any && __uint_as_float(keys[i]) > t;
    const size_t o = (size_t)(y0 + ty) * W + (x0 + tx);
    out_u8[o] = keep ? 1 : 0;
    if (out_f32) out_f32[o] = keep ? 1.f : 0.f;
  }
  // leftover strips: never visited by the reference's block loop, they keep the intensity
  const int xe = GM_GRID * bw, ye = GM_GRID * bh, rw = W - xe, rh = H - ye;
  if (blockIdx.x == GM_GRID - 1 && rw > 0) {  // columns >= xe of this block's rows
    for (int i = tid; i < rw * bh; i += GM_THREADS) {
      const int ty = i / rw, x = xe + (i - ty * rw), y = y0 + ty;
      gm_write_raw(gm_intensity_global(image, W, H, x, y), (size_t)y * W + x, out_u8, out_f32);
    }
  }
  if (blockIdx.y == GM_GRID - 1 && rh > 0) {  // rows >= ye of this block's columns; the last block takes the corner too
    const int cw = blockIdx.x == GM_GRID - 1 ? W - x0 : bw;
    for (int i = tid; i < cw * rh; i += GM_THREADS) {
      const int ty = i / cw, x = x0 + (i - ty * cw), y = ye + ty;
      gm_write_raw(gm_intensity_global(image, W, H, x, y), (size_t)y * W + x, out_u8, out_f32);
    }
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
static bool gm_bad_image(int W, int H) { return W < 2 || H < 2 || (long long)W * H > (1ll << 30); }

struct GradWS {
  uint32_t *key;  // [1] the select's key of the median
  float *I;       // [N]
  void *select;   // gsaj_seed_workspace_bytes(W, H): the radix select's workspace
};

static size_t gm_carve(Carver c, int W, int H, GradWS *w) {
  w->key = c.take<uint32_t>(4);
  w->I = c.take<float>((size_t)W * H + 4);
  w->select = c.take<char>(gsaj_seed_workspace_bytes(W, H));
  return c.used();
}

extern "C" size_t gsaj_grad_mask_workspace_bytes(int W, int H) {
  if (gm_bad_image(W, H)) return 0;
  GradWS w;
  return gm_carve(Carver(nullptr, ALIGN_BASE), W, H, &w) + 256;
}

static void gm_launch_intensity(int W, int H, const float *image, float *out, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_intensity, dim3((W + GM_TW - 1) / GM_TW, (H + GM_TH - 1) / GM_TH), dim3(GM_THREADS), 0, s, W, H, image, out);
}

extern "C" int gsaj_grad_intensity(int W, int H, const float *image, float *out_intensity, void *stream) {
  if (gm_bad_image(W, H) || !image || !out_intensity) {
    gsaj_set_error("gsaj_grad_intensity: invalid argument (W=%d H=%d; both must be at least 2)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  gm_launch_intensity(W, H, image, out_intensity, (hipStream_t)stream);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_grad_mask(int W, int H, const float *image, float edge_threshold, int blocks, uint8_t *out_mask_u8,
                              float *out_mask_f32, void *ws, void *stream) {
  if (gm_bad_image(W, H) || !image || !out_mask_u8 || (!blocks && !ws)) {
    gsaj_set_error("gsaj_grad_mask: invalid argument (W=%d H=%d; both must be at least 2)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  if (blocks) {
    const int bw = W / GM_GRID, bh = H / GM_GRID;
    if (bw < 1 || bh < 1) {
      gsaj_set_error("gsaj_grad_mask: block mode needs W >= %d and H >= %d (got W=%d H=%d): the blocks would be empty", GM_GRID,
                     GM_GRID, W, H);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if ((long long)bw * bh > GM_KEYS_MAX || (long long)(bw + 2) * (bh + 2) > GM_TILE_MAX) {
      gsaj_set_error("gsaj_grad_mask: a block of %d x %d pixels (W=%d H=%d) exceeds the %d pixels (%d with halo) one workgroup holds "
                     "in LDS", bw, bh, W, H, GM_KEYS_MAX, GM_TILE_MAX);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(k_gm_blocks, dim3(GM_GRID, GM_GRID), dim3(GM_THREADS), 0, s, W, H, bw, bh, image, edge_threshold, out_mask_u8,
                       out_mask_f32);
    GSAJ_HIP_CHECK(hipGetLastError());
    return GSAJ_OK;
  }
  GradWS w;
  gm_carve(Carver(ws, ALIGN_BASE), W, H, &w);
  const int n = W * H;
  gm_launch_intensity(W, H, image, w.I, s);
  const int rc = launch_select_rank_f32(W, H, w.I, (uint32_t)((n - 1) / 2), w.key, w.select, s);  // torch.median: the LOWER median
  if (rc != GSAJ_OK) return rc;
  hipLaunchKernelGGL(k_gm_threshold, dim3((n + GM_THREADS - 1) / GM_THREADS), dim3(GM_THREADS), 0, s, n, w.I, w.key, edge_threshold,
                     out_mask_u8, out_mask_f32);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
