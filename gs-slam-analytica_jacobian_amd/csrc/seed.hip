// seed.hip -- new Gaussians from a keyframe, on the device (gfx950): depth statistics (median / std), the monocular depth
// prior, a reproducible uniform down-sample of the valid pixels, back-projection and parameter initialisation.
//
// Semantics: reference utils/slam_utils.py:131-142 (get_median_depth), utils/slam_frontend.py:89-108 (add_new_keyframe, the
// depth the new keyframe is seeded from) and gaussian_splatting/scene/gaussian_model.py:183-279 (create_pcd_from_image /
// create_pcd_from_image_and_depth: Open3D RGBD image -> point cloud -> random_down_sample -> RGB2SH, distCUDA2 scales, unit
// rotations, opacity 0.5).  The reference takes that path through the host (GPU -> NumPy -> Open3D -> NumPy -> GPU).
//
// MI355X design: everything is a few MB per image, i.e. launch- and bandwidth-bound, so the work is a short chain of small
// kernels on one stream with NO host read between them.
//   * Rank selection (median, down-sample threshold) is a most-significant-digit radix SELECT over 32-bit keys: four passes of
//     8 bits, each "histogram of the digit among the keys that still match the prefix" (one LDS histogram per workgroup, then
//     one integer atomic per non-empty bucket) + "one workgroup picks the digit that holds the wanted rank" and leaves the
//     narrowed prefix and the remaining rank in the workspace.  Counts are integers: exact and bit-reproducible.
//   * The fp64 sums of the standard deviation ride along: pass 0 sums the valid depths (-> mean, in its pick), pass 1 the squared
//     deviations (-> std, in its pick).  Per-thread sums in index order, a fixed tree over the workgroup, partials per workgroup
//     summed in index order by the pick: no float atomics anywhere.
//   * The down-sample keeps the m valid pixels with the smallest key(i) = mix32(i ^ mix32(seed)); mix32 is a bijection of the
//     32-bit integers, so keys never tie.  The select gives the m-th smallest key, a count / scan / compact (wave ballot, one wave
//     per 2048 pixels walking them in order) lists the chosen pixels IN PIXEL ORDER.
//
// Built with -ffp-contract=off (csrc/Makefile): where the reference is a chain of fp32 tensor operations (the depth prior, the
// colour quantisation, the scales) each operation here rounds once, like its tensor counterpart; a fused multiply-add would not.
#include "gsaj_common.h"
#include "wave_reduce.h"
#include <cfloat>
#include <cmath>

#define SD_THREADS 256
#define SD_PER 16                      // keys per thread of the histogram kernels: four 16-byte loads
#define SD_TILE (SD_THREADS * SD_PER)  // keys per workgroup
#define SD_CTILE 2048                  // pixels per wave of the compaction kernels
#define SD_SH_C0 0.28209479177387814f  // sh_utils.py C0

enum { SD_KIND_STATS = 0, SD_KIND_SEED = 1, SD_KIND_ALL = 2 };     // what pass 0 takes for key and validity
enum { SD_RANK_MEDIAN = 0, SD_RANK_SAMPLE = 1, SD_RANK_FIXED = 2 };  // how the wanted rank follows from n_valid
enum { ST_PREFIX = 0, ST_RANK = 1, ST_NVALID = 2, ST_NONE = 3, ST_M = 4 };  // SeedWS.st
enum { RES_NVALID = 0, RES_M = 1, RES_THRESHOLD = 2, RES_MED_LO = 3, RES_MED_HI = 4 };  // SeedWS.res

struct SeedWS {
  uint32_t *res;     // [16] what outlives a call: n_valid, m, threshold key of the last gsaj_seed_select; the two middle keys of
                     //   the adaptive point size.  FIRST, so that gsaj_seed_count finds it without knowing W, H
  uint32_t *hist;    // [4][256] digit counts of the four passes           -+
  uint32_t *st;      // [16] select state (ST_*)                            | zeroed by ONE memset per select
  double *dstat;     // [4] mean, std                                      -+
  double *part;      // [ntile] per-workgroup fp64 partial sums of the pass under way
  uint32_t *keys;    // [N]
  uint8_t *flags;    // [N] 1 = valid
  uint32_t *tcount;  // [ctile] chosen pixels per compaction tile, then their exclusive offsets
  uint32_t *sel;     // [N] the chosen pixels, ascending
  float *dist2;      // [N] gsaj_dist2 of the new points
  size_t zero_bytes;
};

static size_t seed_carve(Carver c, int W, int H, SeedWS *w) {
  const size_t N = (size_t)W * H, ntile = (N + SD_TILE - 1) / SD_TILE, ctile = (N + SD_CTILE - 1) / SD_CTILE;
  w->res = c.take<uint32_t>(16);
  const size_t z0 = c.used();
  w->hist = c.take<uint32_t>(4 * 256);
  w->st = c.take<uint32_t>(16);
  w->dstat = c.take<double>(4);
  w->zero_bytes = c.used() - z0;
  w->part = c.take<double>(ntile + 1);
  w->keys = c.take<uint32_t>(N + 4);
  w->flags = c.take<uint8_t>(N + 4);
  w->tcount = c.take<uint32_t>(ctile + 1);
  w->sel = c.take<uint32_t>(N + 4);
  w->dist2 = c.take<float>(N + 4);
  return c.used();
}

// ---- keys -------------------------------------------------------------------------------------------------------------
// floats -> unsigned keys of the same order (negative: all bits flipped; non-negative: sign bit set), and back
__device__ __forceinline__ uint32_t sd_float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float sd_key_float(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
// a bijection of the 32-bit integers (xor-shifts and odd multipliers are each invertible): include/gsaj.h states it in words
__host__ __device__ __forceinline__ uint32_t sd_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 16 bytes from a 4-byte aligned address (planes of a [3,H,W] image start wherever H*W puts them); scalar loads at the end
typedef float sd_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t sd_u4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void sd_load4(const float *__restrict__ p, size_t i, size_t n, float (&v)[4]) {
  if (i + 3 < n) {
    const sd_f4 t = *reinterpret_cast<const sd_f4 *>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = i + c < n ? p[i + c] : 0.f;
  }
}

__device__ __forceinline__ double sd_block_sum(double v, double *red /*[4] LDS*/) {  // fixed tree; the total in every thread
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

struct SdSrc {
  int n, kind;
  const float *depth, *opacity, *gt;  // [n], [n] or NULL, [3,n] or NULL
  const uint8_t *mask;                // [n] bytes or NULL
  float opacity_min, rgb_thr, trunc;
  uint32_t seedmix;
  uint8_t *out_valid;                 // [n] bytes or NULL
};

// pass 0: validity + key of every pixel (kept for the later passes), the histogram of the top digit, the sum of the valid depths
__global__ __launch_bounds__(SD_THREADS) void k_sd_keys(SdSrc a, SeedWS w) {
  __shared__ uint32_t cnt[256];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  cnt[tid] = 0u;
  __syncthreads();
  const size_t n = (size_t)a.n;
  double sum = 0.0;
  for (int j = 0; j < SD_PER / 4; j++) {
    const size_t i = (size_t)blockIdx.x * SD_TILE + ((size_t)j * SD_THREADS + tid) * 4;
    if (i >= n) continue;
    float d[4];
    sd_load4(a.depth, i, n, d);
    bool ok[4];
#pragma unroll
    for (int c = 0; c < 4; c++)
      ok[c] = i + c < n && (a.kind == SD_KIND_ALL || (d[c] > 0.f && (a.kind != SD_KIND_SEED || d[c] < a.trunc)));
    if (a.opacity) {
      float o[4];
      sd_load4(a.opacity, i, n, o);
#pragma unroll
      for (int c = 0; c < 4; c++) ok[c] = ok[c] && o[c] > a.opacity_min;
    }
    if (a.gt) {  // gt_image.sum(dim=0) > threshold, summed (r + g) + b in fp32 like the tensor reduction
      float r[4], g[4], b[4];
      sd_load4(a.gt, i, n, r);
      sd_load4(a.gt + n, i, n, g);
      sd_load4(a.gt + 2 * n, i, n, b);
#pragma unroll
      for (int c = 0; c < 4; c++) ok[c] = ok[c] && __fadd_rn(__fadd_rn(r[c], g[c]), b[c]) > a.rgb_thr;
    }
    if (a.mask) {
#pragma unroll
      for (int c = 0; c < 4; c++) ok[c] = ok[c] && (i + c < n ? a.mask[i + c] != 0 : false);
    }
    uint32_t k[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      k[c] = a.kind == SD_KIND_SEED ? sd_mix32((uint32_t)(i + c) ^ a.seedmix) : sd_float_key(d[c]);
      if (ok[c]) {
        atomicAdd(&cnt[k[c] >> 24], 1u);
        sum += (double)d[c];
      }
    }
    if (i + 3 < n) {
      sd_u4 kv;
      kv.x = k[0]; kv.y = k[1]; kv.z = k[2]; kv.w = k[3];
      *reinterpret_cast<sd_u4 *>(w.keys + i) = kv;
      *reinterpret_cast<uint32_t *>(w.flags + i) =
          (uint32_t)ok[0] | ((uint32_t)ok[1] << 8) | ((uint32_t)ok[2] << 16) | ((uint32_t)ok[3] << 24);
    } else {
      for (int c = 0; c < 4 && i + c < n; c++) {
        w.keys[i + c] = k[c];
        w.flags[i + c] = ok[c] ? 1 : 0;
      }
    }
    if (a.out_valid)
      for (int c = 0; c < 4 && i + c < n; c++) a.out_valid[i + c] = ok[c] ? 1 : 0;
  }
  __syncthreads();
  if (cnt[tid]) atomicAdd(&w.hist[tid], cnt[tid]);
  sum = sd_block_sum(sum, red);
  if (tid == 0) w.part[blockIdx.x] = sum;
}

// passes 1-3: histogram of the pass's digit among the valid keys that match the prefix found so far; with want_var the sum of
// the squared deviations of ALL valid depths from the mean pass 0 left
__global__ __launch_bounds__(SD_THREADS) void k_sd_hist(int n_, int pass, int want_var, const float *__restrict__ depth, SeedWS w) {
  __shared__ uint32_t cnt[256];
  __shared__ double red[4];
  if (w.st[ST_NONE]) return;  // (the same word for every thread: no barrier is split)
  const int tid = threadIdx.x;
  cnt[tid] = 0u;
  __syncthreads();
  const size_t n = (size_t)n_;
  const int shift = 24 - 8 * pass;
  const uint32_t want = w.st[ST_PREFIX] >> (shift + 8);
  const double mean = w.dstat[0];
  double ss = 0.0;
  for (int j = 0; j < SD_PER / 4; j++) {
    const size_t i = (size_t)blockIdx.x * SD_TILE + ((size_t)j * SD_THREADS + tid) * 4;
    if (i >= n) continue;
    uint32_t k[4], f;
    if (i + 3 < n) {
      const sd_u4 kv = *reinterpret_cast<const sd_u4 *>(w.keys + i);
      k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
      f = *reinterpret_cast<const uint32_t *>(w.flags + i);
    } else {
      f = 0u;
      for (int c = 0; c < 4; c++) {
        k[c] = i + c < n ? w.keys[i + c] : 0u;
        f |= i + c < n ? (uint32_t)w.flags[i + c] << (8 * c) : 0u;
      }
    }
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (want_var) sd_load4(depth, i, n, d);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (!((f >> (8 * c)) & 0xffu)) continue;
      if (want_var) {
        const double dd = (double)d[c] - mean;
        ss += dd * dd;
      }
      if ((k[c] >> (shift + 8)) == want) atomicAdd(&cnt[(k[c] >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  if (cnt[tid]) atomicAdd(&w.hist[pass * 256 + tid], cnt[tid]);
  if (want_var) {
    ss = sd_block_sum(ss, red);
    if (tid == 0) w.part[blockIdx.x] = ss;
  }
}

struct SdPick {
  int pass, rank_mode, ntile, stats;
  uint32_t k_fixed;
  double inv_factor;
  uint32_t *out_key;     // pass 3: the key of the wanted rank (0 if there is none)
  uint32_t *out_counts;  // pass 3: n_valid, m (may be NULL)
  float *out_stats;      // pass 3, stats: median, std, n_valid, 0 (may be NULL)
};

// one workgroup: which digit holds the wanted rank?  Leaves prefix | digit and the rank inside that digit's keys.
__global__ __launch_bounds__(256) void k_sd_pick(SdPick a, SeedWS w) {
  __shared__ uint32_t wsum[4];
  __shared__ double red[4];
  __shared__ uint32_t s_rank, s_none, s_prefix, s_final;
  const int tid = threadIdx.x;
  const int shift = 24 - 8 * a.pass;
  double psum = 0.0;
  if (a.stats && a.pass < 2) {
    for (int b = tid; b < a.ntile; b += 256) psum += w.part[b];
    psum = sd_block_sum(psum, red);
  }
  const uint32_t c = w.hist[a.pass * 256 + tid];
  const uint32_t excl = block_excl_scan_add<4>(c, wsum);
  if (tid == 0) {
    uint32_t none, rank;
    if (a.pass == 0) {
      const uint32_t nv = block_scan_total<4>(wsum);  // pass 0's histogram counts every valid pixel
      uint32_t m = 0u;
      none = nv == 0u;
      rank = 0u;
      if (a.rank_mode == SD_RANK_MEDIAN) {
        rank = none ? 0u : (nv - 1u) / 2u;  // torch.median: the LOWER median
      } else if (a.rank_mode == SD_RANK_SAMPLE) {
        size_t mm = (size_t)((double)nv * a.inv_factor);  // Open3D random_down_sample(1 / factor): size_t(n * ratio)
        if (mm > nv) mm = nv;
        m = (uint32_t)mm;
        none = m == 0u;
        rank = none ? 0u : m - 1u;
      } else {
        none = a.k_fixed >= nv;
        rank = none ? 0u : a.k_fixed;
      }
      w.st[ST_NVALID] = nv;
      w.st[ST_M] = m;
      w.st[ST_NONE] = none;
      if (a.stats) w.dstat[0] = nv ? psum / (double)nv : 0.0;
    } else {
      none = w.st[ST_NONE];
      rank = w.st[ST_RANK];
      // torch.std: unbiased; one valid pixel gives 0 / 0 = NaN there and here
      if (a.stats && a.pass == 1 && !none) w.dstat[1] = sqrt(psum / ((double)w.st[ST_NVALID] - 1.0));
    }
    s_none = none;
    s_rank = rank;
    s_prefix = w.st[ST_PREFIX];
    s_final = 0u;
  }
  __syncthreads();
  if (!s_none) {
    if (s_rank >= excl && s_rank < excl + c) {  // exactly one thread: the counts of the matching keys add up to more than the rank
      const uint32_t np = s_prefix | ((uint32_t)tid << shift);
      w.st[ST_PREFIX] = np;
      w.st[ST_RANK] = s_rank - excl;
      s_final = np;
    }
  }
  __syncthreads();
  if (a.pass == 3 && tid == 0) {
    if (a.out_key) *a.out_key = s_none ? 0u : s_final;
    if (a.out_counts) {
      a.out_counts[0] = w.st[ST_NVALID];
      a.out_counts[1] = w.st[ST_M];
    }
    if (a.out_stats) {
      a.out_stats[0] = s_none ? 0.f : sd_key_float(s_final);
      a.out_stats[1] = s_none ? 0.f : (float)w.dstat[1];
      a.out_stats[2] = (float)w.st[ST_NVALID];
      a.out_stats[3] = 0.f;
    }
  }
}

static int sd_run_select(const SdSrc &src, int rank_mode, uint32_t k_fixed, double inv_factor, int stats, uint32_t *out_key,
                         uint32_t *out_counts, float *out_stats, SeedWS &w, hipStream_t s) {
  const int ntile = (src.n + SD_TILE - 1) / SD_TILE;
  GSAJ_HIP_CHECK(hipMemsetAsync(w.hist, 0, w.zero_bytes, s));
  SdPick pk;
  pk.rank_mode = rank_mode; pk.ntile = ntile; pk.stats = stats; pk.k_fixed = k_fixed; pk.inv_factor = inv_factor;
  pk.out_key = out_key; pk.out_counts = out_counts; pk.out_stats = out_stats;
  for (int pass = 0; pass < 4; pass++) {
    if (pass == 0)
      hipLaunchKernelGGL(k_sd_keys, dim3(ntile), dim3(SD_THREADS), 0, s, src, w);
    else
      hipLaunchKernelGGL(k_sd_hist, dim3(ntile), dim3(SD_THREADS), 0, s, src.n, pass, (stats && pass == 1) ? 1 : 0, src.depth, w);
    pk.pass = pass;
    hipLaunchKernelGGL(k_sd_pick, dim3(1), dim3(256), 0, s, pk, w);
  }
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// ---- the chosen pixels in pixel order ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sd_count(int n, SeedWS w) {
  const int lane = threadIdx.x, beg = blockIdx.x * SD_CTILE, end = min(n, beg + SD_CTILE);
  const bool any = w.res[RES_M] != 0u;
  const uint32_t thr = w.res[RES_THRESHOLD];
  uint32_t cnt = 0u;
  for (int i = beg + lane; i < end; i += 64) cnt += (any && w.flags[i] && w.keys[i] <= thr) ? 1u : 0u;
  cnt = wave_sum(cnt);
  if (lane == 0) w.tcount[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(64) void k_sd_compact(int n, SeedWS w) {
  const int lane = threadIdx.x, beg = blockIdx.x * SD_CTILE, end = min(n, beg + SD_CTILE);
  const bool any = w.res[RES_M] != 0u;
  const uint32_t thr = w.res[RES_THRESHOLD];
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t base = w.tcount[blockIdx.x];
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int i = i0 + lane;
    const bool pick = i < end && any && w.flags[i] && w.keys[i] <= thr;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(pick);
    const uint32_t dst = base + (uint32_t)__popcll(bal & below);
    if (pick && dst < (uint32_t)n) w.sel[dst] = (uint32_t)i;
    base += (uint32_t)__popcll(bal);
  }
}

// ---- the monocular depth prior ----------------------------------------------------------------------------------------------
// slam_frontend.py:92-103 with the statistics gsaj_depth_stats left on the device; one fp32 rounding per tensor operation of the
// reference (no contraction), so the result is the reference's bit for bit wherever the comparisons agree
__global__ __launch_bounds__(256) void k_sd_prior(int n_, const float *__restrict__ depth, const float *__restrict__ gt, float rgb_thr,
                                                  const float *__restrict__ noise, const float *__restrict__ stats,
                                                  const uint8_t *__restrict__ valid, float *__restrict__ out) {
  const size_t n = (size_t)n_, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const float med = stats[0], sd = stats[1];
  const float hi = __fadd_rn(med, sd), lo = __fsub_rn(med, sd);
  const float s_bad = __fmul_rn(sd, 0.5f), s_good = __fmul_rn(sd, 0.2f);
  float d[4], r[4], g[4], b[4], z[4] = {0.f, 0.f, 0.f, 0.f};
  sd_load4(depth, i, n, d);
  sd_load4(gt, i, n, r);
  sd_load4(gt + n, i, n, g);
  sd_load4(gt + 2 * n, i, n, b);
  if (noise) sd_load4(noise, i, n, z);
  float o[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const bool v = i + c < n ? valid[i + c] != 0 : false;
    const bool bad = d[c] > hi || d[c] < lo || !v;
    const float base = bad ? med : d[c];
    const float val = noise ? __fadd_rn(base, __fmul_rn(z[c], bad ? s_bad : s_good)) : base;
    o[c] = __fadd_rn(__fadd_rn(r[c], g[c]), b[c]) > rgb_thr ? val : 0.f;
  }
  if (i + 3 < n) {
    sd_f4 t;
    t.x = o[0]; t.y = o[1]; t.z = o[2]; t.w = o[3];
    *reinterpret_cast<sd_f4 *>(out + i) = t;
  } else {
    for (int c = 0; c < 4 && i + c < n; c++) out[i + c] = o[c];
  }
}

// ---- back-projection + initial parameters -----------------------------------------------------------------------------------
struct SdInit {
  int m, W, H, rest;  // rest = (sh_coeffs - 1) * 3 floats of f_rest per point
  const float *depth, *image, *exposure_ab, *w2c;
  double fx, fy, cx, cy;
  float *xyz, *f_dc, *rotation, *opacity;
};

__global__ __launch_bounds__(256) void k_sd_points(SdInit a, SeedWS w) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.m) return;
  const size_t n = (size_t)a.W * a.H;
  const uint32_t i = min(w.sel[j], (uint32_t)(n - 1));
  const int u = (int)(i % (uint32_t)a.W), v = (int)(i / (uint32_t)a.W);
  // Open3D works in double on the float image (z = d, x = (u - cx) z / fx, y = (v - cy) z / fy), the reference rounds the world
  // point to fp32 once (.float()).  W2C: 16 row-major floats, inverted as a general affine map (it may be a similarity transform)
  const double z = (double)a.depth[i];
  const double x = ((double)u - a.cx) * z / a.fx, y = ((double)v - a.cy) * z / a.fy;
  double A[3][3], t[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) A[r][c] = (double)a.w2c[4 * r + c];
    t[r] = (double)a.w2c[4 * r + 3];
  }
  const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
               c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  const double idet = 1.0 / (A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02);
  const double qx = x - t[0], qy = y - t[1], qz = z - t[2];
  // inverse = adjugate / det; adjugate[r][c] = cofactor[c][r]
  const double wx = (c00 * qx + (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * qy + (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * qz) * idet;
  const double wy = (c01 * qx + (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * qy + (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * qz) * idet;
  const double wz = (c02 * qx + (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * qy + (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * qz) * idet;
  a.xyz[3 * (size_t)j] = (float)wx;
  a.xyz[3 * (size_t)j + 1] = (float)wy;
  a.xyz[3 * (size_t)j + 2] = (float)wz;
  // colour: q = (uint8)(clamp(exp(a) img + b, 0, 1) * 255), truncated (gaussian_model.py:185-187); Open3D keeps q / 255 in double,
  // the reference rounds it to fp32; RGB2SH = (rgb - 0.5) / C0
  const float ea = a.exposure_ab ? expf(a.exposure_ab[0]) : 1.f, eb = a.exposure_ab ? a.exposure_ab[1] : 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float ab = __fadd_rn(__fmul_rn(ea, a.image[(size_t)c * n + i]), eb);
    const float cl = fminf(fmaxf(ab, 0.f), 1.f);
    const int q = (int)__fmul_rn(cl, 255.f);
    const float rgb = (float)((double)q / 255.0);
    a.f_dc[3 * (size_t)j + c] = __fdiv_rn(__fsub_rn(rgb, 0.5f), SD_SH_C0);
  }
  a.rotation[4 * (size_t)j] = 1.f;
  a.rotation[4 * (size_t)j + 1] = 0.f;
  a.rotation[4 * (size_t)j + 2] = 0.f;
  a.rotation[4 * (size_t)j + 3] = 0.f;
  a.opacity[j] = 0.f;  // inverse_sigmoid(0.5)
}

// scales = log(sqrt(max(dist2, 1e-7) * point_size)), one fp32 rounding per operation (gaussian_model.py:259-268)
__global__ __launch_bounds__(256) void k_sd_scales(int m, int cols, float point_size, int adaptive, SeedWS w, float *__restrict__ scaling) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  float ps = point_size;
  if (adaptive) {
    // np.median of the whole depth image: the mean of the two middle order statistics, in the image's fp32; then
    // min(0.05, point_size * median) in double (a Python float times a NumPy scalar), rounded when it meets the fp32 tensor
    const float med = __fmul_rn(__fadd_rn(sd_key_float(w.res[RES_MED_LO]), sd_key_float(w.res[RES_MED_HI])), 0.5f);
    ps = (float)fmin(0.05, (double)point_size * (double)med);
  }
  const float s = logf(sqrtf(__fmul_rn(fmaxf(w.dist2[j], 1e-7f), ps)));
  for (int c = 0; c < cols; c++) scaling[(size_t)j * cols + c] = s;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
static bool sd_bad_image(int W, int H) { return W <= 0 || H <= 0 || (long long)W * H > (1ll << 30); }

extern "C" size_t gsaj_seed_workspace_bytes(int W, int H) {
  if (sd_bad_image(W, H)) return 0;
  SeedWS w;
  return seed_carve(Carver(nullptr, ALIGN_BASE), W, H, &w) + 256;
}

extern "C" int gsaj_depth_stats(int W, int H, const float *depth, const float *opacity, float opacity_min, const uint8_t *mask,
                                const float *gt_image, float rgb_threshold, float *out_stats, uint8_t *out_valid, void *seed_ws,
                                void *stream) {
  if (sd_bad_image(W, H) || !depth || !out_stats || !seed_ws) {
    gsaj_set_error("gsaj_depth_stats: invalid argument (W=%d H=%d)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  SdSrc src;
  src.n = W * H; src.kind = SD_KIND_STATS; src.depth = depth; src.opacity = opacity; src.gt = gt_image; src.mask = mask;
  src.opacity_min = opacity_min; src.rgb_thr = rgb_threshold; src.trunc = 0.f; src.seedmix = 0u; src.out_valid = out_valid;
  return sd_run_select(src, SD_RANK_MEDIAN, 0u, 0.0, 1, nullptr, nullptr, out_stats, w, (hipStream_t)stream);
}

extern "C" int gsaj_keyframe_depth_prior(int W, int H, const float *depth, const float *opacity, const float *gt_image,
                                         float rgb_threshold, const float *noise, float *out_depth, float *out_stats, void *seed_ws,
                                         void *stream) {
  if (sd_bad_image(W, H) || !depth || !opacity || !gt_image || !out_depth || !out_stats || !seed_ws) {
    gsaj_set_error("gsaj_keyframe_depth_prior: invalid argument (W=%d H=%d)", W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const int rc = gsaj_depth_stats(W, H, depth, opacity, 0.95f, nullptr, gt_image, rgb_threshold, out_stats, nullptr, seed_ws, stream);
  if (rc != GSAJ_OK) return rc;
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  const int n = W * H;
  hipLaunchKernelGGL(k_sd_prior, dim3((n + 1023) / 1024), dim3(256), 0, (hipStream_t)stream, n, depth, gt_image, rgb_threshold, noise,
                     out_stats, w.flags, out_depth);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_seed_select(int W, int H, const float *depth, const float *gt_image, float rgb_threshold, float depth_trunc,
                                double downsample_factor, uint32_t seed, void *seed_ws, void *stream) {
  if (sd_bad_image(W, H) || !depth || !seed_ws || !(downsample_factor >= 1.0) || !(depth_trunc > 0.f)) {
    gsaj_set_error("gsaj_seed_select: invalid argument (W=%d H=%d downsample_factor=%g depth_trunc=%g)", W, H, downsample_factor,
                   (double)depth_trunc);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  const int n = W * H, ctile = (n + SD_CTILE - 1) / SD_CTILE;
  SdSrc src;
  src.n = n; src.kind = SD_KIND_SEED; src.depth = depth; src.opacity = nullptr; src.gt = gt_image; src.mask = nullptr;
  src.opacity_min = 0.f; src.rgb_thr = rgb_threshold; src.trunc = depth_trunc; src.seedmix = sd_mix32(seed); src.out_valid = nullptr;
  const int rc = sd_run_select(src, SD_RANK_SAMPLE, 0u, 1.0 / downsample_factor, 0, w.res + RES_THRESHOLD, w.res + RES_NVALID, nullptr, w, s);
  if (rc != GSAJ_OK) return rc;
  hipLaunchKernelGGL(k_sd_count, dim3(ctile), dim3(64), 0, s, n, w);
  launch_exclusive_scan_u32(ctile, w.tcount, s);  // (knn.hip: the radix sort's one-workgroup scan)
  hipLaunchKernelGGL(k_sd_compact, dim3(ctile), dim3(64), 0, s, n, w);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// the key (sd_float_key) of the order statistic `rank` of ALL W * H floats of `values`; for frame.hip, through gsaj_common.h
int launch_select_rank_f32(int W, int H, const float *values, uint32_t rank, uint32_t *out_key, void *seed_ws, hipStream_t s) {
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  SdSrc src;
  src.n = W * H; src.kind = SD_KIND_ALL; src.depth = values; src.opacity = nullptr; src.gt = nullptr; src.mask = nullptr;
  src.opacity_min = 0.f; src.rgb_thr = 0.f; src.trunc = 0.f; src.seedmix = 0u; src.out_valid = nullptr;
  return sd_run_select(src, SD_RANK_FIXED, rank, 0.0, 0, out_key, nullptr, nullptr, w, s);
}

extern "C" int gsaj_seed_count(const void *seed_ws, void *stream, int *n_valid, int *m) {
  if (!seed_ws || !n_valid || !m) {
    gsaj_set_error("gsaj_seed_count: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), 1, 1, &w);  // (res comes first: its place does not depend on the image size)
  uint32_t host[2] = {0u, 0u};
  GSAJ_HIP_CHECK(hipMemcpyAsync(host, w.res + RES_NVALID, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *n_valid = (int)host[0];
  *m = (int)host[1];
  return GSAJ_OK;
}

extern "C" int gsaj_debug_seed_pixels(int W, int H, int m, const void *seed_ws, uint32_t *pixels, void *stream) {
  if (sd_bad_image(W, H) || m < 0 || (long long)m > (long long)W * H || !seed_ws || (m > 0 && !pixels)) {
    gsaj_set_error("gsaj_debug_seed_pixels: invalid argument (W=%d H=%d m=%d)", W, H, m);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (m == 0) return GSAJ_OK;
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  GSAJ_HIP_CHECK(hipMemcpyAsync(pixels, w.sel, (size_t)m * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GSAJ_OK;
}

extern "C" int gsaj_seed_gaussians(int m, int W, int H, const float *depth, const float *image, const float *exposure_ab,
                                   const float *w2c, double fx, double fy, double cx, double cy, float point_size, int adaptive,
                                   int sh_coeffs, int isotropic, float *xyz, float *f_dc, float *f_rest, float *scaling,
                                   float *rotation, float *opacity, void *seed_ws, void *knn_ws, void *stream) {
  if (m < 0 || sd_bad_image(W, H) || (long long)m > (long long)W * H || sh_coeffs < 1 || !(fx != 0.0) || !(fy != 0.0) ||
      (m > 0 && (!depth || !image || !w2c || !xyz || !f_dc || (sh_coeffs > 1 && !f_rest) || !scaling || !rotation || !opacity ||
                 !seed_ws || !knn_ws))) {
    gsaj_set_error("gsaj_seed_gaussians: invalid argument (m=%d W=%d H=%d sh_coeffs=%d)", m, W, H, sh_coeffs);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (m == 0) return GSAJ_OK;
  hipStream_t s = (hipStream_t)stream;
  SeedWS w;
  seed_carve(Carver(seed_ws, ALIGN_BASE), W, H, &w);
  const int n = W * H;
  if (adaptive) {  // the two middle order statistics of the whole depth image, zeros included (np.median)
    int rc = launch_select_rank_f32(W, H, depth, (uint32_t)((n - 1) / 2), w.res + RES_MED_LO, seed_ws, s);
    if (rc != GSAJ_OK) return rc;
    rc = launch_select_rank_f32(W, H, depth, (uint32_t)(n / 2), w.res + RES_MED_HI, seed_ws, s);
    if (rc != GSAJ_OK) return rc;
  }
  SdInit a;
  a.m = m; a.W = W; a.H = H; a.rest = (sh_coeffs - 1) * 3;
  a.depth = depth; a.image = image; a.exposure_ab = exposure_ab; a.w2c = w2c;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.xyz = xyz; a.f_dc = f_dc; a.rotation = rotation; a.opacity = opacity;
  if (a.rest) GSAJ_HIP_CHECK(hipMemsetAsync(f_rest, 0, (size_t)m * a.rest * sizeof(float), s));
  hipLaunchKernelGGL(k_sd_points, dim3((m + 255) / 256), dim3(256), 0, s, a, w);
  GSAJ_HIP_CHECK(hipGetLastError());
  const int rc = gsaj_dist2(m, xyz, w.dist2, knn_ws, stream);
  if (rc != GSAJ_OK) return rc;
  hipLaunchKernelGGL(k_sd_scales, dim3((m + 255) / 256), dim3(256), 0, s, m, isotropic ? 1 : 3, point_size, adaptive ? 1 : 0, w, scaling);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
