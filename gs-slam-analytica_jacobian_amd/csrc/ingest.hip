// ingest.hip -- a camera frame from bytes to what the trackers read (include/gsaj.h "frame ingest"):
//   k_undistort_map  once per camera, fp64: the source coordinate of every output pixel under the Brown-Conrady model
//   k_frame_ingest   once per frame, ONE launch for colour and depth: uint8 [Hs,Ws,C] -> fp32 [3,H,W] in [0, 1], direct or through the
//                    map with an exact fp32 bilinear and a constant 0 border; uint16 depth -> fp32 metres
//   k_rectify_u8     a grey image through the map to BYTES (what a stereo matcher reads), the same bilinear stopped before the division
// Memory-bound with no reuse: no LDS, no barrier, no atomics; every output element is written once, the bits are the same run to run.
// Compiled without FMA contraction: tests/ingest_restated.py restates both kernels one rounding at a time.
#include "gsaj_common.h"

#define INGEST_BLOCK 256
#define INGEST_FLAGS (GSAJ_INGEST_BGR | GSAJ_INGEST_ROUND_U8 | GSAJ_INGEST_DEPTH_MUL)

struct MapParams {
  int W, H;
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
  double iR[9];
  float *map_x, *map_y;
};

// One thread per output pixel.  Every product and sum in the order include/gsaj.h writes it, left to right.
__global__ __launch_bounds__(INGEST_BLOCK) void k_undistort_map(MapParams p) {
  const size_t i = (size_t)blockIdx.x * INGEST_BLOCK + threadIdx.x;
  if (i >= (size_t)p.W * p.H) return;
  const double u = (double)(int)(i % (size_t)p.W), v = (double)(int)(i / (size_t)p.W);
  const double X = p.iR[0] * u + p.iR[1] * v + p.iR[2];
  const double Y = p.iR[3] * u + p.iR[4] * v + p.iR[5];
  const double Wq = p.iR[6] * u + p.iR[7] * v + p.iR[8];
  const double x = X / Wq, y = Y / Wq;
  const double r2 = x * x + y * y;
  const double rad = 1.0 + p.k1 * r2 + p.k2 * (r2 * r2) + p.k3 * ((r2 * r2) * r2);
  const double xd = x * rad + 2.0 * p.p1 * x * y + p.p2 * (r2 + 2.0 * x * x);
  const double yd = y * rad + p.p1 * (r2 + 2.0 * y * y) + 2.0 * p.p2 * x * y;
  p.map_x[i] = (float)(p.fx * xd + p.cx);
  p.map_y[i] = (float)(p.fy * yd + p.cy);
}

struct IngestParams {
  int W, H, Ws, Hs, C, flags;
  size_t src_stride, depth_stride;   // bytes
  const uint8_t *src;
  const float *map_x, *map_y;        // both or neither
  const uint16_t *depth_raw;         // with out_depth, or neither
  double depth_scale;
  float *out_color, *out_depth;
  int src_wide;     // vector path, no map: the four pixels of a thread are one 4-byte aligned read of 4 C bytes
  int depth_wide;   // vector path: the four depths of a thread are one aligned 8-byte read
};

__device__ __forceinline__ float ingest_unit(float val, int flags) {
  if (flags & GSAJ_INGEST_ROUND_U8) val = floorf(val + 0.5f);
  return fminf(fmaxf(val / 255.0f, 0.f), 1.f);
}

// the source channel of output plane c: a grey byte feeds all three planes, a fourth byte is never read
__device__ __forceinline__ int ingest_channel(int c, int C, int flags) { return C == 1 ? 0 : (flags & GSAJ_INGEST_BGR) ? 2 - c : c; }

// exact fp32 bilinear of the three planes at (mx, my); a tap outside the source is 0.0f, a coordinate that is not finite or lies
// outside [-1, Ws] x [-1, Hs] gives 0 -- decided on the floats, before any conversion to an integer.
// BYTES (k_rectify_u8): the value rounded to a byte as GSAJ_INGEST_ROUND_U8 rounds it, left in grey levels
template <bool BYTES = false>
__device__ __forceinline__ void ingest_remap(const IngestParams &p, float mx, float my, float out[3]) {
  out[0] = out[1] = out[2] = 0.f;
  if (!(mx >= -1.f && mx <= (float)p.Ws && my >= -1.f && my <= (float)p.Hs)) return;
  const float fx0 = floorf(mx), fy0 = floorf(my);
  const float ax = mx - fx0, ay = my - fy0, bx = 1.f - ax, by = 1.f - ay;
  const int x0 = (int)fx0, y0 = (int)fy0;
  const bool inx0 = x0 >= 0 && x0 < p.Ws, inx1 = x0 + 1 >= 0 && x0 + 1 < p.Ws;
  const bool iny0 = y0 >= 0 && y0 < p.Hs, iny1 = y0 + 1 >= 0 && y0 + 1 < p.Hs;
  const uint8_t *r0 = p.src + (size_t)(iny0 ? y0 : 0) * p.src_stride, *r1 = p.src + (size_t)(iny1 ? y0 + 1 : 0) * p.src_stride;
  const size_t c0 = (size_t)(inx0 ? x0 : 0) * p.C, c1 = (size_t)(inx1 ? x0 + 1 : 0) * p.C;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c > 0 && p.C == 1) {   // the grey value, computed once
      out[c] = out[0];
      continue;
    }
    const int ch = ingest_channel(c, p.C, p.flags);
    const float p00 = inx0 && iny0 ? (float)r0[c0 + ch] : 0.f, p01 = inx1 && iny0 ? (float)r0[c1 + ch] : 0.f;
    const float p10 = inx0 && iny1 ? (float)r1[c0 + ch] : 0.f, p11 = inx1 && iny1 ? (float)r1[c1 + ch] : 0.f;
    const float top = p00 * bx + p01 * ax, bot = p10 * bx + p11 * ax;
    const float val = top * by + bot * ay;
    out[c] = BYTES ? fminf(floorf(val + 0.5f), 255.f) : ingest_unit(val, p.flags);
  }
}

__device__ __forceinline__ float ingest_depth(uint16_t d, double scale, int flags) {
  return (float)((flags & GSAJ_INGEST_DEPTH_MUL) ? (double)d * scale : (double)d / scale);
}

// 4 C consecutive source bytes as C words: one 4-byte aligned read (global_load_dword / dwordx3 / dwordx4 need no more)
struct IngestWords3 { uint32_t x, y, z; };
struct IngestWords4 { uint32_t x, y, z, w; };
template <int C>
__device__ __forceinline__ void ingest_load_words(const uint8_t *at, uint32_t w[4]) {
  if constexpr (C == 1) {
    w[0] = *reinterpret_cast<const uint32_t *>(at);
  } else if constexpr (C == 3) {
    const IngestWords3 v = *reinterpret_cast<const IngestWords3 *>(at);
    w[0] = v.x; w[1] = v.y; w[2] = v.z;
  } else {
    const IngestWords4 v = *reinterpret_cast<const IngestWords4 *>(at);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
}

// VEC: a thread owns four consecutive pixels of a row (W % 4 == 0, every plane and map 16-byte aligned): one 16-byte store per plane,
// one 16-byte load per map plane.  Otherwise one thread per pixel.  Both give the same bits: the arithmetic is the functions above.
template <bool VEC>
__global__ __launch_bounds__(INGEST_BLOCK) void k_frame_ingest(IngestParams p) {
  constexpr int N = VEC ? 4 : 1;
  const size_t i = (size_t)blockIdx.x * INGEST_BLOCK + threadIdx.x, n = (size_t)p.W * p.H;
  if (i * N >= n) return;
  const int u = (int)((i * N) % (size_t)p.W), v = (int)((i * N) / (size_t)p.W);
  float c[3][4];
  if (p.map_x) {
    float mx[4], my[4];
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4 *>(p.map_x + i * 4), b = *reinterpret_cast<const float4 *>(p.map_y + i * 4);
      mx[0] = a.x; mx[1] = a.y; mx[2] = a.z; mx[3] = a.w;
      my[0] = b.x; my[1] = b.y; my[2] = b.z; my[3] = b.w;
    } else {
      mx[0] = p.map_x[i];
      my[0] = p.map_y[i];
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
      float o[3];
      ingest_remap(p, mx[j], my[j], o);
      c[0][j] = o[0]; c[1][j] = o[1]; c[2][j] = o[2];
    }
  } else {
    const uint8_t *at = p.src + (size_t)v * p.src_stride + (size_t)u * p.C;
    uint32_t w[4] = {0u, 0u, 0u, 0u};   // the 4 C (scalar path: C) bytes of the thread's pixels, little-endian
    if (VEC && p.src_wide) {
      if (p.C == 1) ingest_load_words<1>(at, w);
      else if (p.C == 3) ingest_load_words<3>(at, w);
      else ingest_load_words<4>(at, w);
    } else {
#pragma unroll
      for (int k = 0; k < 4 * N; k++)
        if (k < N * p.C) w[k >> 2] |= (uint32_t)at[k] << (8 * (k & 3));
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
#pragma unroll
      for (int pl = 0; pl < 3; pl++) {
        const int k = j * p.C + ingest_channel(pl, p.C, p.flags);
        const uint32_t word = (k >> 2) == 0 ? w[0] : (k >> 2) == 1 ? w[1] : (k >> 2) == 2 ? w[2] : w[3];
        c[pl][j] = fminf(fmaxf((float)((word >> (8 * (k & 3))) & 255u) / 255.0f, 0.f), 1.f);
      }
    }
  }
#pragma unroll
  for (int pl = 0; pl < 3; pl++) {
    float *o = p.out_color + (size_t)pl * n;
    if (VEC) *reinterpret_cast<float4 *>(o + i * 4) = make_float4(c[pl][0], c[pl][1], c[pl][2], c[pl][3]);
    else o[i] = c[pl][0];
  }
  if (p.depth_raw) {
    const uint16_t *dr = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(p.depth_raw) + (size_t)v * p.depth_stride) + u;
    if (VEC) {
      uint16_t d[4];
      if (p.depth_wide) {
        const uint2 q = *reinterpret_cast<const uint2 *>(dr);
        d[0] = (uint16_t)q.x; d[1] = (uint16_t)(q.x >> 16); d[2] = (uint16_t)q.y; d[3] = (uint16_t)(q.y >> 16);
      } else {
        d[0] = dr[0]; d[1] = dr[1]; d[2] = dr[2]; d[3] = dr[3];
      }
      *reinterpret_cast<float4 *>(p.out_depth + i * 4) =
          make_float4(ingest_depth(d[0], p.depth_scale, p.flags), ingest_depth(d[1], p.depth_scale, p.flags),
                      ingest_depth(d[2], p.depth_scale, p.flags), ingest_depth(d[3], p.depth_scale, p.flags));
    } else {
      p.out_depth[i] = ingest_depth(dr[0], p.depth_scale, p.flags);
    }
  }
}

// One thread per output pixel: the byte, and (out_color != NULL) the byte / 255.0f in all three planes -- bit for bit what
// k_frame_ingest gives a one-channel image with GSAJ_INGEST_ROUND_U8 through the same map.  Without a map the byte is the source's.
__global__ __launch_bounds__(INGEST_BLOCK) void k_rectify_u8(IngestParams p, uint8_t *out, size_t out_stride) {
  const size_t i = (size_t)blockIdx.x * INGEST_BLOCK + threadIdx.x, n = (size_t)p.W * p.H;
  if (i >= n) return;
  const int u = (int)(i % (size_t)p.W), v = (int)(i / (size_t)p.W);
  float b;
  if (p.map_x) {
    float o[3];
    ingest_remap<true>(p, p.map_x[i], p.map_y[i], o);
    b = o[0];
  } else {
    b = (float)p.src[(size_t)v * p.src_stride + u];
  }
  out[(size_t)v * out_stride + u] = (uint8_t)b;
  if (p.out_color) {
    const float c = fminf(fmaxf(b / 255.0f, 0.f), 1.f);
    p.out_color[i] = c;
    p.out_color[n + i] = c;
    p.out_color[2 * n + i] = c;
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
static bool ingest_aligned(const void *ptr, size_t a) { return reinterpret_cast<size_t>(ptr) % a == 0; }

extern "C" int gsaj_undistort_map(int W, int H, const double *K_src, const double *dist, const double *iR, float *map_x, float *map_y,
                                  void *stream) {
  if (W < 1 || H < 1 || (size_t)W * H > (size_t)INT32_MAX) {
    gsaj_set_error("gsaj_undistort_map: W and H must be positive with W * H <= INT_MAX (W=%d H=%d)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!K_src || !dist || !iR || !map_x || !map_y) {
    gsaj_set_error("gsaj_undistort_map: K_src, dist, iR, map_x and map_y are required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  MapParams p;
  p.W = W; p.H = H;
  p.fx = K_src[0]; p.fy = K_src[1]; p.cx = K_src[2]; p.cy = K_src[3];
  p.k1 = dist[0]; p.k2 = dist[1]; p.p1 = dist[2]; p.p2 = dist[3]; p.k3 = dist[4];
  for (int i = 0; i < 9; i++) p.iR[i] = iR[i];
  p.map_x = map_x; p.map_y = map_y;
  const size_t n = (size_t)W * H;
  hipLaunchKernelGGL(k_undistort_map, dim3((unsigned)((n + INGEST_BLOCK - 1) / INGEST_BLOCK)), dim3(INGEST_BLOCK), 0, (hipStream_t)stream, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_frame_ingest(int W, int H, int Ws, int Hs, int channels, size_t src_stride, const uint8_t *src, const float *map_x,
                                 const float *map_y, const uint16_t *depth_raw, size_t depth_stride, double depth_scale, int flags,
                                 float *out_color, float *out_depth, void *stream) {
  if (W < 1 || H < 1 || Ws < 1 || Hs < 1 || (size_t)W * H > (size_t)INT32_MAX || (size_t)Ws * Hs > (size_t)INT32_MAX) {
    gsaj_set_error("gsaj_frame_ingest: W, H, Ws and Hs must be positive with W * H and Ws * Hs <= INT_MAX (W=%d H=%d Ws=%d Hs=%d)", W, H, Ws, Hs);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (channels != 1 && channels != 3 && channels != 4) {
    gsaj_set_error("gsaj_frame_ingest: channels must be 1, 3 or 4 (channels=%d)", channels);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (flags & ~INGEST_FLAGS) {
    gsaj_set_error("gsaj_frame_ingest: unknown flag bits (flags=0x%x)", (unsigned)flags);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!src || !out_color) {
    gsaj_set_error("gsaj_frame_ingest: src and out_color are required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (src_stride < (size_t)Ws * channels) {
    gsaj_set_error("gsaj_frame_ingest: src_stride %zu is less than Ws * channels = %zu", src_stride, (size_t)Ws * channels);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((map_x == nullptr) != (map_y == nullptr)) {
    gsaj_set_error("gsaj_frame_ingest: map_x and map_y must be given together or not at all");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!map_x && (Ws != W || Hs != H)) {
    gsaj_set_error("gsaj_frame_ingest: without a map the source must have the output's size (W=%d H=%d Ws=%d Hs=%d)", W, H, Ws, Hs);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((depth_raw == nullptr) != (out_depth == nullptr)) {
    gsaj_set_error("gsaj_frame_ingest: depth_raw and out_depth must be given together or not at all");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (depth_raw) {
    if (depth_stride < 2 * (size_t)W) {
      gsaj_set_error("gsaj_frame_ingest: depth_stride %zu is less than 2 * W = %zu", depth_stride, 2 * (size_t)W);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if (depth_stride % 2 != 0 || !ingest_aligned(depth_raw, 2)) {
      gsaj_set_error("gsaj_frame_ingest: depth_raw and depth_stride must be 2-byte aligned (depth_stride=%zu)", depth_stride);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if (!(depth_scale != 0.0) || !(__builtin_fabs(depth_scale) < __builtin_inf())) {
      gsaj_set_error("gsaj_frame_ingest: depth_scale must be finite and not zero (depth_scale=%g)", depth_scale);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
  }
  if (!ingest_aligned(out_color, 4) || (out_depth && !ingest_aligned(out_depth, 4)) || (map_x && (!ingest_aligned(map_x, 4) || !ingest_aligned(map_y, 4)))) {
    gsaj_set_error("gsaj_frame_ingest: out_color, out_depth, map_x and map_y must be 4-byte aligned");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  IngestParams p;
  p.W = W; p.H = H; p.Ws = Ws; p.Hs = Hs; p.C = channels; p.flags = flags;
  p.src_stride = src_stride; p.depth_stride = depth_raw ? depth_stride : 0;
  p.src = src; p.map_x = map_x; p.map_y = map_y; p.depth_raw = depth_raw; p.depth_scale = depth_raw ? depth_scale : 1.0;
  p.out_color = out_color; p.out_depth = out_depth;
  // W % 4 == 0 keeps every row, hence every plane, 16-byte aligned relative to its base; the bases themselves must be too
  const bool vec = W % 4 == 0 && ingest_aligned(out_color, 16) && (!out_depth || ingest_aligned(out_depth, 16)) &&
                   (!map_x || (ingest_aligned(map_x, 16) && ingest_aligned(map_y, 16)));
  p.src_wide = vec && !map_x && ingest_aligned(src, 4) && src_stride % 4 == 0;
  p.depth_wide = vec && depth_raw && ingest_aligned(depth_raw, 8) && depth_stride % 8 == 0;
  const size_t threads = ((size_t)W * H) / (vec ? 4 : 1);
  const dim3 grid((unsigned)((threads + INGEST_BLOCK - 1) / INGEST_BLOCK));
  if (vec) hipLaunchKernelGGL(k_frame_ingest<true>, grid, dim3(INGEST_BLOCK), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(k_frame_ingest<false>, grid, dim3(INGEST_BLOCK), 0, (hipStream_t)stream, p);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_rectify_u8(int W, int H, int Ws, int Hs, size_t src_stride, const uint8_t *src, const float *map_x, const float *map_y,
                               uint8_t *out, size_t out_stride, float *out_color, void *stream) {
  if (W < 1 || H < 1 || Ws < 1 || Hs < 1 || (size_t)W * H > (size_t)INT32_MAX || (size_t)Ws * Hs > (size_t)INT32_MAX) {
    gsaj_set_error("gsaj_rectify_u8: W, H, Ws and Hs must be positive with W * H and Ws * Hs <= INT_MAX (W=%d H=%d Ws=%d Hs=%d)", W, H, Ws, Hs);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!src || !out) {
    gsaj_set_error("gsaj_rectify_u8: src and out are required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (src_stride < (size_t)Ws || out_stride < (size_t)W) {
    gsaj_set_error("gsaj_rectify_u8: a row stride is less than its row (src_stride=%zu Ws=%d out_stride=%zu W=%d)", src_stride, Ws, out_stride, W);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((map_x == nullptr) != (map_y == nullptr)) {
    gsaj_set_error("gsaj_rectify_u8: map_x and map_y must be given together or not at all");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!map_x && (Ws != W || Hs != H)) {
    gsaj_set_error("gsaj_rectify_u8: without a map the source must have the output's size (W=%d H=%d Ws=%d Hs=%d)", W, H, Ws, Hs);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((out_color && !ingest_aligned(out_color, 4)) || (map_x && (!ingest_aligned(map_x, 4) || !ingest_aligned(map_y, 4)))) {
    gsaj_set_error("gsaj_rectify_u8: out_color, map_x and map_y must be 4-byte aligned");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  IngestParams p;
  p.W = W; p.H = H; p.Ws = Ws; p.Hs = Hs; p.C = 1; p.flags = GSAJ_INGEST_ROUND_U8;
  p.src_stride = src_stride; p.depth_stride = 0;
  p.src = src; p.map_x = map_x; p.map_y = map_y; p.depth_raw = nullptr; p.depth_scale = 1.0;
  p.out_color = out_color; p.out_depth = nullptr;
  p.src_wide = 0; p.depth_wide = 0;
  const size_t n = (size_t)W * H;
  hipLaunchKernelGGL(k_rectify_u8, dim3((unsigned)((n + INGEST_BLOCK - 1) / INGEST_BLOCK)), dim3(INGEST_BLOCK), 0, (hipStream_t)stream, p, out, out_stride);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
