// stereo.hip -- a rectified stereo pair to a disparity and a depth map (include/gsaj.h "stereo frames"): semi-global matching in integer
// arithmetic, the device's bits equal to tests/stereo_restated.py.  What is named sgm_* / SGM_* is shared with sweep.hip: sgm.h.
//   k_stereo_prefilter  both images: the clipped horizontal Sobel, one byte per pixel (sgm_sobel_bytes)
//   k_stereo_cost       C [H,W,D] uint16, d innermost: |P_L - P_R| summed over the clamped window -- a thread owns one (x, d) and walks
//                       down a band of rows with a ring of row sums in LDS (SGM_BOX_WALK); pc is never stored
//   k_stereo_paths      ONE launch for every line of every direction: a group of min(D, 64) lanes walks one line, a lane per disparity
//                       (two per lane at D = 128, 64 / D lines per wave below 64); L(d +- 1) by lane shifts, m(q) by wave_min; the next
//                       step's row of C is requested before this step's arithmetic; L is added into S [H,W,D] uint32 with atomics
//                       (integer adds: exact in any order)
//   k_stereo_winner     a workgroup per row: argmin, uniqueness, sub-pixel (sgm_argmin, sgm_subsample16); disp2 by a packed-key atomic
//                       min in LDS, so no result depends on which lane came first; then the left-right check, disp16 and the depth
// Only the depth line is floating point (fp64, nothing there to contract); the file is compiled without FMA contraction all the same.
#include "sgm.h"

#define STEREO_RING 31        // 2 * 15 + 1 row sums
#define STEREO_MAX_R 15       // 961 * 30 fits C's uint16
#define STEREO_MAX_W 4096     // k_stereo_winner keeps 12 bytes of LDS per column
#define STEREO_STAGES (GSAJ_STEREO_STAGE_COST | GSAJ_STEREO_STAGE_PATHS | GSAJ_STEREO_STAGE_WINNER)

struct StereoWS {
  uint8_t *pl, *pr;   // [H,W] prefiltered left, right
  uint16_t *C;        // [H,W,D]
  uint32_t *S;        // [H,W,D]
};

// (the workspace must be 256-byte aligned as handed over: carved BASE_AS_GIVEN, no base slack in its size)
static size_t stereo_carve(Carver c, int W, int H, int D, StereoWS *w, size_t *c_off = nullptr, size_t *s_off = nullptr) {
  const size_t n = (size_t)W * H;
  w->pl = c.take<uint8_t>(n);
  w->pr = c.take<uint8_t>(n);
  if (c_off) *c_off = c.used();
  w->C = c.take<uint16_t>(n * D);
  if (s_off) *s_off = c.used();
  w->S = c.take<uint32_t>(n * D);
  return c.used();
}

// ---- a. prefilter ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SGM_BLOCK) void k_stereo_prefilter(int W, int H, const uint8_t *__restrict__ left, size_t left_stride,
                                                                const uint8_t *__restrict__ right, size_t right_stride,
                                                                uint8_t *__restrict__ pl, uint8_t *__restrict__ pr) {
  const size_t i = (size_t)blockIdx.x * SGM_BLOCK + threadIdx.x;
  if (i >= (size_t)W * H) return;
  const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
  const int b = sgm_sobel_bytes(blockIdx.y ? right : left, blockIdx.y ? right_stride : left_stride, W, H, x, y);
  (blockIdx.y ? pr : pl)[i] = (uint8_t)(b & 255);   // the horizontal byte alone
}

// ---- b, c. the block cost --------------------------------------------------------------------------------------------------------------
// the row sum of pc over |x' - x| <= r at row y
__device__ __forceinline__ int stereo_row_sum(const uint8_t *__restrict__ pl, const uint8_t *__restrict__ pr, int W, int y, int x, int d, int r) {
  const uint8_t *a = pl + (size_t)y * W, *b = pr + (size_t)y * W;
  int s = 0;
  for (int dx = -r; dx <= r; dx++) {
    const int xc = min(max(x + dx, 0), W - 1);
    s += abs((int)a[xc] - (int)b[max(xc - d, 0)]);
  }
  return s;
}

// grid: (columns of the valid region in groups of SGM_BLOCK / D, bands of SGM_BAND rows); the walk and its ring of row sums: sgm.h
template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_stereo_cost(int W, int H, int r, const uint8_t *__restrict__ pl, const uint8_t *__restrict__ pr,
                                                           uint16_t *__restrict__ C) {
  __shared__ uint16_t ring[STEREO_RING * SGM_BLOCK];   // a row sum is <= 31 * 30
  const int d = threadIdx.x % D;
  const int x = D + (int)blockIdx.x * (SGM_BLOCK / D) + threadIdx.x / D;
  if (x >= W) return;
#define STEREO_ROW_SUM(y) stereo_row_sum(pl, pr, W, y, x, d, r)
  SGM_BOX_WALK(D, ring, x, d, W, H, r, C, STEREO_ROW_SUM)   // C <= 961 * 30
}

// ---- e. the paths ------------------------------------------------------------------------------------------------------------------------
struct StereoPaths {
  int W, H, P1, P2, paths;
  int xf;   // the first valid column: D for the rectified pair, 0 for a volume that is valid everywhere (sweep.hip)
  const uint16_t *C;
  uint32_t *S;
};

// The lines of direction (dx, dy) over the valid region x in [xf, W): every pixel whose predecessor lies outside starts one.
//   dy == 0: H lines; dx == 0: W - xf lines; a diagonal: the W - xf pixels of its first row, then the H - 1 others of its first column
__device__ __forceinline__ int stereo_line_count(int dx, int dy, int Wv, int H) { return dy == 0 ? H : dx == 0 ? Wv : Wv + H - 1; }

template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_stereo_paths(StereoPaths p) {
  constexpr int WIDTH = D < 64 ? D : 64, LPW = 64 / WIDTH, NV = D / WIDTH;   // lanes per line, lines per wave, disparities per lane
  const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (WIDTH - 1);
  const int Wv = p.W - p.xf;
  int rem = ((int)blockIdx.x * (SGM_BLOCK / 64) + wave) * LPW + lane / WIDTH;
  int dx = 0, dy = 0, x0 = 0, y0 = 0, len = 0;
  bool found = false;
  for (int k = 0; k < p.paths; k++) {
    const int n = stereo_line_count(DX[k], DY[k], Wv, p.H);
    if (!found && rem < n) {
      found = true;
      dx = DX[k];
      dy = DY[k];
    } else if (!found) {
      rem -= n;
    }
  }
  if (found) {
    if (dy == 0) {
      y0 = rem;
      x0 = dx > 0 ? p.xf : p.W - 1;
    } else if (dx == 0 || rem < Wv) {
      x0 = p.xf + rem;
      y0 = dy > 0 ? 0 : p.H - 1;
    } else {
      const int j = rem - Wv + 1;   // 1 .. H - 1
      x0 = dx > 0 ? p.xf : p.W - 1;
      y0 = dy > 0 ? j : p.H - 1 - j;
    }
    const int lx = dx > 0 ? p.W - x0 : dx < 0 ? x0 - p.xf + 1 : INT32_MAX;
    const int ly = dy > 0 ? p.H - y0 : dy < 0 ? y0 + 1 : INT32_MAX;
    len = min(lx, ly);
  }
  const int steps = wave_max(len);   // the lines of a wave differ in length: every lane runs the longest, a finished line idles
  const ptrdiff_t at0 = ((ptrdiff_t)y0 * p.W + x0) * D + sub * NV, stride = ((ptrdiff_t)dy * p.W + dx) * D;
  // this lane's disparities of C at step i: d = sub (NV = 1), or d = 2 sub and 2 sub + 1 as one 4-byte read (NV = 2)
  auto load = [&](int i) -> uint32_t {
    if (i >= len) return 0u;
    const uint16_t *c = p.C + (at0 + (ptrdiff_t)i * stride);
    return NV == 1 ? (uint32_t)*c : *reinterpret_cast<const uint32_t *>(c);
  };
  uint32_t c = load(0);
  int L0 = 0, L1 = 0;
  for (int i = 0; i < steps; i++) {
    const uint32_t cn = load(i + 1);   // requested before this step's chain of shuffles: the walk is a serial dependency
    const int c0 = (int)(c & 0xffffu), c1 = (int)(c >> 16);
    if (i == 0) {
      L0 = c0;
      L1 = c1;
    } else {
      const int m = wave_min<WIDTH>(NV == 1 ? L0 : min(L0, L1));
      const int up = __shfl_up(NV == 1 ? L0 : L1, 1, WIDTH), dn = __shfl_down(L0, 1, WIDTH);
      int a0 = min(L0, m + p.P2), a1 = min(L1, m + p.P2);
      if (sub > 0) a0 = min(a0, up + p.P1);
      if (NV == 1) {
        if (sub < WIDTH - 1) a0 = min(a0, dn + p.P1);
      } else {
        a0 = min(a0, L1 + p.P1);
        a1 = min(a1, L0 + p.P1);
        if (sub < WIDTH - 1) a1 = min(a1, dn + p.P1);
      }
      L0 = c0 + a0 - m;
      L1 = c1 + a1 - m;
    }
    if (i < len) {
      uint32_t *s = p.S + (at0 + (ptrdiff_t)i * stride);
      atomicAdd(s, (uint32_t)L0);
      if (NV == 2) atomicAdd(s + 1, (uint32_t)L1);
    }
    c = cn;
  }
}

// One launch for every line of every direction over the columns [first_col, W) of C, after S has been zeroed on the stream (S is summed
// into).  Shared with sweep.hip (sgm.h); sizes are the caller's to have checked.
template <int D>
static void stereo_paths_launch(const StereoPaths &pp, hipStream_t s) {
  const int Wv = pp.W - pp.xf;
  const int lines = (pp.paths == 8 ? 4 : 0) * (Wv + pp.H - 1) + 2 * pp.H + 2 * Wv;
  constexpr int per_block = (SGM_BLOCK / 64) * (D < 64 ? 64 / D : 1);
  hipLaunchKernelGGL(k_stereo_paths<D>, dim3((unsigned)((lines + per_block - 1) / per_block)), dim3(SGM_BLOCK), 0, s, pp);
}

hipError_t launch_stereo_paths(int D, int W, int H, int first_col, int P1, int P2, int paths, const uint16_t *C, uint32_t *S, hipStream_t s) {
  if (!sgm_d_ok(D) || first_col < 0 || first_col >= W || H < 1 || (paths != 4 && paths != 8)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(S, 0, (size_t)W * H * D * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  StereoPaths pp;
  pp.W = W; pp.H = H; pp.P1 = P1; pp.P2 = P2; pp.paths = paths; pp.xf = first_col; pp.C = C; pp.S = S;
  sgm_for_d(D, [&](auto d) { stereo_paths_launch<decltype(d)::value>(pp, s); });
  return hipGetLastError();
}

// ---- f-i. winner, uniqueness, sub-pixel, left-right check, depth -------------------------------------------------------------------------
struct StereoWinner {
  int W, H, uniqueness, lr_max_diff;
  const uint32_t *S;
  int16_t *disp16;
  float *depth;   // or NULL
  double bf;
};

#define STEREO_NO_KEY 0xffffffffffffffffull

// One workgroup per row.  LDS: disp2 [W] as packed keys S << 32 | (W - 1 - x) << 8 | d*, so that an integer min is the rule "smallest
// S, then the largest x"; d16 [W] as int.
template <int D>
__global__ __launch_bounds__(SGM_BLOCK) void k_stereo_winner(StereoWinner p) {
  constexpr int WIDTH = SgmGroup<D>::WIDTH, LPW = SgmGroup<D>::LPW, GROUPS = SgmGroup<D>::GROUPS;
  extern __shared__ unsigned long long stereo_lds[];
  unsigned long long *disp2 = stereo_lds;
  int *d16s = reinterpret_cast<int *>(stereo_lds + p.W);
  const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (WIDTH - 1), g = wave * LPW + lane / WIDTH;
  for (int x = threadIdx.x; x < p.W; x += SGM_BLOCK) {
    disp2[x] = STEREO_NO_KEY;
    d16s[x] = -16;
  }
  __syncthreads();
  const uint32_t *row = p.S + (size_t)y * p.W * D;
  for (int xb = D; xb < p.W; xb += GROUPS) {   // (uniform: the reductions below are executed by every lane)
    const int x = xb + g;
    const bool active = x < p.W;
    const uint32_t *s = row + (size_t)(active ? x : D) * D;
    const SgmBest w = sgm_argmin<D>(s, sub, p.uniqueness);
    if (active && sub == 0 && !w.rival) {
      d16s[x] = sgm_subsample16<D>(s, w.d, w.S);
      atomicMin(&disp2[x - w.d], ((unsigned long long)w.S << 32) | ((unsigned long long)(uint32_t)(p.W - 1 - x) << 8) | (unsigned long long)w.d);
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < p.W; x += SGM_BLOCK) {
    int v = d16s[x];
    if (v >= 0 && p.lr_max_diff >= 0) {
      int fails = 0;
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int delta = (v + 15 * k) >> 4, x2 = x - delta;
        if (x2 >= 0) {
          const unsigned long long key = disp2[x2];
          if (key != STEREO_NO_KEY && abs((int)(key & 255ull) - delta) > p.lr_max_diff) fails++;
        }
      }
      if (fails == 2) v = -16;
    }
    p.disp16[(size_t)y * p.W + x] = (int16_t)v;
    if (p.depth) {
      double delta = (double)v / 16.0;   // the reference's lines in its float64, rounded to float32 once
      if (delta == 0.0) delta = 1e10;
      double z = p.bf / delta;
      if (z < 0.0) z = 0.0;
      p.depth[(size_t)y * p.W + x] = (float)z;
    }
  }
}

// k_stereo_winner's LDS: disp2 [W] 8-byte keys + d16 [W] ints of dynamic LDS, no __shared__ of its own.  W <= STEREO_MAX_W keeps the
// request under LDS_DEFAULT_LIMIT (stereo_sizes_ok refuses a wider image before anything is launched).
constexpr size_t STEREO_WINNER_STATIC_LDS = 0;
static_assert(STEREO_WINNER_STATIC_LDS + (size_t)STEREO_MAX_W * (sizeof(unsigned long long) + sizeof(int)) <= LDS_DEFAULT_LIMIT,
              "k_stereo_winner: STEREO_MAX_W columns no longer fit the LDS of a workgroup");
bool lds_stereo_winner(int W, int D, LdsRequest *out) {
  if (!sgm_d_ok(D) || W <= D || W > STEREO_MAX_W) return false;
  out->dynamic_bytes = (size_t)W * (sizeof(unsigned long long) + sizeof(int));
  out->static_bytes = STEREO_WINNER_STATIC_LDS;
  out->limit_bytes = LDS_DEFAULT_LIMIT;
  out->variant = D;
  return true;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
static bool stereo_sizes_ok(const char *who, int W, int H, int D, int paths) {
  return sgm_sizes_ok(who, D, paths, [&] {
    if (H >= 1 && W > D && W <= STEREO_MAX_W && (size_t)W * H * D <= (size_t)INT32_MAX) return true;
    gsaj_set_error("%s: needs D < W <= %d, H >= 1 and W * H * D <= INT_MAX (W=%d H=%d D=%d)", who, STEREO_MAX_W, W, H, D);
    return false;
  });
}

extern "C" int gsaj_stereo_workspace_bytes(int W, int H, int D, int paths, size_t *bytes) {
  if (!stereo_sizes_ok("gsaj_stereo_workspace_bytes", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (!bytes) {
    gsaj_set_error("gsaj_stereo_workspace_bytes: bytes is required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  StereoWS ws;
  *bytes = stereo_carve(Carver(nullptr, BASE_AS_GIVEN), W, H, D, &ws);
  return GSAJ_OK;
}

extern "C" int gsaj_debug_stereo_offsets(int W, int H, int D, int paths, size_t *cost_off, size_t *sum_off) {
  if (!stereo_sizes_ok("gsaj_debug_stereo_offsets", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  StereoWS ws;
  stereo_carve(Carver(nullptr, BASE_AS_GIVEN), W, H, D, &ws, cost_off, sum_off);
  return GSAJ_OK;
}

template <int D>
static hipError_t stereo_launch(int stages, int W, int H, const uint8_t *left, size_t left_stride, const uint8_t *right, size_t right_stride, int r,
                                int P1, int P2, int paths, const StereoWS &ws, const StereoWinner &wp, hipStream_t s) {
  const int Wv = W - D;
  if (stages & GSAJ_STEREO_STAGE_COST) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(k_stereo_prefilter, dim3((unsigned)((n + SGM_BLOCK - 1) / SGM_BLOCK), 2), dim3(SGM_BLOCK), 0, s, W, H, left,
                       left_stride, right, right_stride, ws.pl, ws.pr);
    constexpr int XB = SGM_BLOCK / D;
    hipLaunchKernelGGL(k_stereo_cost<D>, dim3((unsigned)((Wv + XB - 1) / XB), (unsigned)((H + SGM_BAND - 1) / SGM_BAND)), dim3(SGM_BLOCK),
                       0, s, W, H, r, ws.pl, ws.pr, ws.C);
  }
  if (stages & GSAJ_STEREO_STAGE_PATHS) {
    const hipError_t e = launch_stereo_paths(D, W, H, D, P1, P2, paths, ws.C, ws.S, s);   // S is summed into: zeroed there, on the stream
    if (e != hipSuccess) return e;
  }
  if (stages & GSAJ_STEREO_STAGE_WINNER) {
    LdsRequest lds;
    if (!lds_stereo_winner(W, D, &lds)) return hipErrorInvalidValue;  // (cannot happen: stereo_sizes_ok has passed)
    hipLaunchKernelGGL(k_stereo_winner<D>, dim3((unsigned)H), dim3(SGM_BLOCK), lds.dynamic_bytes, s, wp);
  }
  return hipGetLastError();
}

extern "C" int gsaj_stereo_match(int W, int H, const uint8_t *left, size_t left_stride, const uint8_t *right, size_t right_stride, int D, int r,
                                 int P1, int P2, int paths, int uniqueness, int lr_max_diff, int stages, void *workspace,
                                 size_t workspace_bytes, int16_t *disp16, float *out_depth, double bf, void *stream) {
  if (!stereo_sizes_ok("gsaj_stereo_match", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (!sgm_params_ok("gsaj_stereo_match", r, STEREO_MAX_R, P1, P2, uniqueness)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (lr_max_diff < -1) {
    gsaj_set_error("gsaj_stereo_match: lr_max_diff must be >= -1 (lr_max_diff=%d)", lr_max_diff);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  StereoWS ws;
  const size_t need = stereo_carve(Carver(workspace, BASE_AS_GIVEN), W, H, D, &ws);   // (arithmetic only: a null base is refused below)
  SgmBuffers b;
  b.required = left && right && workspace && disp16; b.required_names = "left, right, workspace and disp16";
  b.image[0] = "left"; b.image[1] = "right"; b.stride[0] = left_stride; b.stride[1] = right_stride;
  b.workspace = workspace; b.workspace_bytes = workspace_bytes; b.need = need; b.size_fn = "gsaj_stereo_workspace_bytes";
  b.out16 = disp16; b.out_depth = out_depth; b.others_aligned = true; b.aligned_names = "disp16 2-byte and out_depth 4-byte";
  const int rc = sgm_buffers_ok("gsaj_stereo_match", W, &stages, STEREO_STAGES, b);
  if (rc != GSAJ_OK) return rc;
  if (out_depth && (!(bf > 0.0) || !(bf < __builtin_inf()))) {
    gsaj_set_error("gsaj_stereo_match: with out_depth, bf must be positive and finite (bf=%g)", bf);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  StereoWinner wp;
  wp.W = W; wp.H = H; wp.uniqueness = uniqueness; wp.lr_max_diff = lr_max_diff; wp.S = ws.S; wp.disp16 = disp16; wp.depth = out_depth;
  wp.bf = out_depth ? bf : 1.0;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = sgm_for_d(D, [&](auto d) {
    return stereo_launch<decltype(d)::value>(stages, W, H, left, left_stride, right, right_stride, r, P1, P2, paths, ws, wp, s);
  });
  GSAJ_HIP_CHECK(e);
  return GSAJ_OK;
}
