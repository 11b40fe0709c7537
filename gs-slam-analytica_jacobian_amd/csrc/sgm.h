// sgm.h -- the stages the two semi-global matchers share, each written once: stereo.hip (a rectified pair) and sweep.hip (motion
// stereo) are the same pipeline -- gradient bytes, block cost, path aggregation, winner -- over different pixel costs.  Here: the
// clipped Sobel bytes (sgm_sobel_bytes), the walk down a band of rows with a ring of row sums in LDS (SGM_BOX_WALK), the winner of a
// pixel's D sums and its sub-sample step (sgm_argmin, sgm_subsample16), the path aggregation's launcher (k_stereo_paths is compiled
// once, in stereo.hip), the entry points' argument checks, their texts taking `who`, and the dispatch over D (sgm_for_d).
#pragma once
#include <type_traits>
#include "gsaj_common.h"
#include "wave_reduce.h"

#define SGM_BLOCK 256
#define SGM_BAND 64   // rows a thread of a block-cost kernel walks: the 2r + 1 row sums of its start are shared by this many outputs

// stereo.hip's path aggregation over the columns [first_col, W) of a cost volume C [H,W,D] (D 16, 32, 64 or 128; paths 4 or 8): S [H,W,D]
// is zeroed on the stream, then ONE launch adds every line's L into it.  first_col: D for the rectified pair, 0 for motion stereo.
hipError_t launch_stereo_paths(int D, int W, int H, int first_col, int P1, int P2, int paths, const uint16_t *C, uint32_t *S, hipStream_t s);

// ---- host: the entry points' checks, in the order they have always been made (sizes: D, the file's range line with its own message, paths)
static inline bool sgm_d_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128; }

template <class RangeOk>
static bool sgm_sizes_ok(const char *who, int D, int paths, RangeOk range_ok) {
  if (!sgm_d_ok(D)) {
    gsaj_set_error("%s: D must be 16, 32, 64 or 128 (D=%d)", who, D);
    return false;
  }
  if (!range_ok()) return false;
  if (paths != 4 && paths != 8) {
    gsaj_set_error("%s: paths must be 4 or 8 (paths=%d)", who, paths);
    return false;
  }
  return true;
}

static bool sgm_params_ok(const char *who, int r, int r_max, int P1, int P2, int uniqueness) {
  if (r < 0 || r > r_max) {
    gsaj_set_error("%s: the block radius must lie in [0, %d] (r=%d)", who, r_max, r);
    return false;
  }
  if (P1 < 0 || P1 >= P2 || P2 > 1024) {
    gsaj_set_error("%s: needs 0 <= P1 < P2 <= 1024 (P1=%d P2=%d)", who, P1, P2);
    return false;
  }
  if (uniqueness < 0 || uniqueness > 99) {
    gsaj_set_error("%s: uniqueness must lie in [0, 99] (uniqueness=%d)", who, uniqueness);
    return false;
  }
  return true;
}

struct SgmBuffers {   // what a match entry point was handed, with the words its messages name them by
  bool required; const char *required_names;   // every required pointer is there; "left, right, workspace and disp16"
  const char *image[2]; size_t stride[2];      // "left", "right"
  const void *workspace; size_t workspace_bytes, need; const char *size_fn;   // need: what the size function says
  const void *out16, *out_depth; bool others_aligned; const char *aligned_names;   // others: the entry point's further 4-byte pointers
};

// stage bits (0 becomes `all`), required pointers, row strides, the workspace's size, the alignments -> GSAJ_OK or the error code
static int sgm_buffers_ok(const char *who, int W, int *stages, int all, const SgmBuffers &b) {
  if (*stages & ~all) {
    gsaj_set_error("%s: unknown stage bits (stages=0x%x)", who, (unsigned)*stages);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (*stages == 0) *stages = all;
  if (!b.required) {
    gsaj_set_error("%s: %s are required", who, b.required_names);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (b.stride[0] < (size_t)W || b.stride[1] < (size_t)W) {
    gsaj_set_error("%s: a row stride is less than W (%s_stride=%zu %s_stride=%zu W=%d)", who, b.image[0], b.stride[0], b.image[1], b.stride[1], W);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (b.workspace_bytes < b.need) {
    gsaj_set_error("%s: the workspace has %zu bytes, %s says %zu", who, b.workspace_bytes, b.size_fn, b.need);
    return GSAJ_ERR_WORKSPACE_TOO_SMALL;
  }
  if (reinterpret_cast<size_t>(b.workspace) % 256 != 0 || reinterpret_cast<size_t>(b.out16) % 2 != 0 ||
      reinterpret_cast<size_t>(b.out_depth) % 4 != 0 || !b.others_aligned) {
    gsaj_set_error("%s: workspace must be 256-byte, %s aligned", who, b.aligned_names);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

// f(std::integral_constant<int, D>) for the D that sgm_d_ok has passed: the one place the four instantiations are chosen
template <class F>
static auto sgm_for_d(int D, F &&f) {
  switch (D) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return f(std::integral_constant<int, 128>{});
  }
}

#ifdef __HIPCC__
// ---- a. the clipped Sobel bytes Gx | Gy << 8 of pixel (x, y), neighbour rows and columns clamped to the image --------------------------------
__device__ __forceinline__ int sgm_sobel_bytes(const uint8_t *__restrict__ img, size_t stride, int W, int H, int x, int y) {
  const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
  const uint8_t *r0 = img + (size_t)max(y - 1, 0) * stride, *r1 = img + (size_t)y * stride, *r2 = img + (size_t)min(y + 1, H - 1) * stride;
  const int gx = ((int)r0[xp] - (int)r0[xm]) + 2 * ((int)r1[xp] - (int)r1[xm]) + ((int)r2[xp] - (int)r2[xm]);
  const int gy = ((int)r2[xm] - (int)r0[xm]) + 2 * ((int)r2[x] - (int)r0[x]) + ((int)r2[xp] - (int)r0[xp]);
  const int bx = min(max(gx, -15), 15) + 15, by = min(max(gy, -15), 15) + 15;
  return bx | (by << 8);
}

// ---- the block cost of column x, entry d over the band of rows blockIdx.y: C = the sum of ROW_SUM(y') over the clamped window
// |y' - y| <= r.  The 2r + 1 row sums stay in LDS, a ring of slots private to the thread (slot-major: a wave's reads and writes of one
// slot are contiguous, no barrier is needed), so that a step computes ONE row sum, the entering row's, and takes the leaving row's from
// the ring.  The kernel declares `ring` (>= 2 r_max + 1 slots: its LDS), maps its threads to (x, d), returns where x >= W and ends with
// this.  A macro, ROW_SUM(y) a function-like macro of the kernel's: as an inline function taking a callable the same loops come out laid
// out differently, and k_stereo_cost<16> measured 1.2 % slower at 160 x 120; expanded in place both kernels keep their instructions.
#define SGM_BOX_WALK(D, ring, x, d, W, H, r, C, ROW_SUM)                                                          \
  const int y0 = (int)blockIdx.y * SGM_BAND, y1 = min(y0 + SGM_BAND, H), n = 2 * r + 1;                           \
  uint16_t *mine = ring + threadIdx.x;                                                                            \
  int v = 0;                                                                                                      \
  for (int k = 0; k < n; k++) { /* slot k: row y0 - r + k */                                                      \
    const int s = ROW_SUM(min(max(y0 - r + k, 0), H - 1));                                                        \
    mine[k * SGM_BLOCK] = (uint16_t)s;                                                                            \
    v += s;                                                                                                       \
  }                                                                                                               \
  int slot = 0; /* the slot of row y - r, the one that leaves next */                                             \
  for (int y = y0; y < y1; y++) {                                                                                 \
    C[((size_t)y * W + x) * D + d] = (uint16_t)v;                                                                 \
    if (y + 1 < y1) {                                                                                             \
      const int in = ROW_SUM(min(y + 1 + r, H - 1));                                                              \
      v += in - (int)mine[slot * SGM_BLOCK];                                                                      \
      mine[slot * SGM_BLOCK] = (uint16_t)in;                                                                      \
      slot = slot + 1 == n ? 0 : slot + 1;                                                                        \
    }                                                                                                             \
  }

// ---- the winner of a pixel's D sums s[0 .. D), by a group of min(D, 64) lanes, D / 64 entries a lane: `sub` is the lane's place in its
// group.  Executed by EVERY lane of the wave (reductions).  d* by a packed (S << 7 | d) key, S < 2^25: the lowest d wins a tie; rival:
// an entry further than 1 from d* within the uniqueness margin of the best.
template <int D>
struct SgmGroup {   // lanes per pixel, pixels per wave, entries per lane, pixels per workgroup
  static constexpr int WIDTH = D < 64 ? D : 64, LPW = 64 / WIDTH, NV = D / WIDTH, GROUPS = (SGM_BLOCK / 64) * LPW;
};

struct SgmBest { int d; uint32_t S; bool rival; };
template <int D>
__device__ __forceinline__ SgmBest sgm_argmin(const uint32_t *__restrict__ s, int sub, int uniqueness) {
  constexpr int WIDTH = SgmGroup<D>::WIDTH, NV = SgmGroup<D>::NV;
  uint32_t v[NV], key = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < NV; j++) {
    v[j] = s[sub * NV + j];
    key = min(key, (v[j] << 7) | (uint32_t)(sub * NV + j));
  }
  key = wave_min<WIDTH>(key);
  const int dstar = (int)(key & 127u);
  const uint32_t best = key >> 7, margin = (uint32_t)(100 - uniqueness);
  uint32_t vote = 0u;
#pragma unroll
  for (int j = 0; j < NV; j++)
    if (abs(sub * NV + j - dstar) > 1 && v[j] * margin < best * 100u) vote = 1u;
  return {dstar, best, wave_max<WIDTH>(vote) != 0u};
}

// 16 d* plus the parabola's step through S(d* - 1), S(d*), S(d* + 1), rounded by C division (towards zero); none at either end
template <int D>
__device__ __forceinline__ int sgm_subsample16(const uint32_t *__restrict__ s, int dstar, uint32_t best) {
  int d16 = 16 * dstar;
  if (dstar > 0 && dstar < D - 1) {
    const int sm = (int)s[dstar - 1], sp = (int)s[dstar + 1];
    const int den = max(sm + sp - 2 * (int)best, 1);
    d16 += ((sm - sp) * 16 + den) / (2 * den);
  }
  return d16;
}
#endif
