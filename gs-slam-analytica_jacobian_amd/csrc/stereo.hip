// stereo.hip -- a rectified stereo pair to a disparity and a depth map (include/gsaj.h "stereo frames"): semi-global matching in integer
// arithmetic, the device's bits equal to tests/stereo_restated.py.
//   k_stereo_prefilter  both images: the clipped horizontal Sobel, one byte per pixel
//   k_stereo_cost       C [H,W,D] uint16, d innermost: |P_L - P_R| summed over the clamped window -- a thread owns one (x, d) and walks
//                       down a band of rows with a running column sum: the entering row's sum is computed, the leaving row's comes
//                       from a ring in LDS; pc is never stored
//   k_stereo_paths      ONE launch for every line of every direction: a group of min(D, 64) lanes walks one line, a lane per disparity
//                       (two per lane at D = 128, 64 / D lines per wave below 64); L(d +- 1) by lane shifts, m(q) by wave_min; the next
//                       step's row of C is requested before this step's arithmetic; L is added into S [H,W,D] uint32 with atomics
//                       (integer adds: exact in any order)
//   k_stereo_winner     a workgroup per row: argmin by a packed (S, d) key, uniqueness, sub-pixel; disp2 by a packed-key atomic min in
//                       LDS, so no result depends on which lane came first; then the left-right check, disp16 and the depth
// Only the depth line is floating point (fp64, nothing there to contract); the file is compiled without FMA contraction all the same.
#include "gsaj_common.h"
#include "wave_reduce.h"

#define STEREO_BLOCK 256
#define STEREO_BAND 64        // rows a thread of k_stereo_cost walks: the 2r + 1 row sums of its start are shared by this many outputs
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
__global__ __launch_bounds__(STEREO_BLOCK) void k_stereo_prefilter(int W, int H, const uint8_t *__restrict__ left, size_t left_stride,
                                                                   const uint8_t *__restrict__ right, size_t right_stride,
                                                                   uint8_t *__restrict__ pl, uint8_t *__restrict__ pr) {
  const size_t i = (size_t)blockIdx.x * STEREO_BLOCK + threadIdx.x;
  if (i >= (size_t)W * H) return;
  const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
  const uint8_t *img = blockIdx.y ? right : left;
  const size_t stride = blockIdx.y ? right_stride : left_stride;
  const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
  const uint8_t *r0 = img + (size_t)max(y - 1, 0) * stride, *r1 = img + (size_t)y * stride, *r2 = img + (size_t)min(y + 1, H - 1) * stride;
  const int gx = ((int)r0[xp] - (int)r0[xm]) + 2 * ((int)r1[xp] - (int)r1[xm]) + ((int)r2[xp] - (int)r2[xm]);
  (blockIdx.y ? pr : pl)[i] = (uint8_t)(min(max(gx, -15), 15) + 15);
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

// grid: (columns of the valid region in groups of STEREO_BLOCK / D, bands of STEREO_BAND rows).  The 2r + 1 row sums of the window stay
// in LDS, a ring of slots private to the thread (slot-major: a wave's reads and writes of one slot are contiguous, no barrier is
// needed), so that a step computes ONE row sum, the entering row's, and takes the leaving row's from the ring.
#define STEREO_RING 31   // 2 * 15 + 1
template <int D>
__global__ __launch_bounds__(STEREO_BLOCK) void k_stereo_cost(int W, int H, int r, const uint8_t *__restrict__ pl, const uint8_t *__restrict__ pr,
                                                              uint16_t *__restrict__ C) {
  __shared__ uint16_t ring[STEREO_RING * STEREO_BLOCK];   // a row sum is <= 31 * 30
  const int d = threadIdx.x % D;
  const int x = D + (int)blockIdx.x * (STEREO_BLOCK / D) + threadIdx.x / D;
  if (x >= W) return;
  const int y0 = (int)blockIdx.y * STEREO_BAND, y1 = min(y0 + STEREO_BAND, H), n = 2 * r + 1;
  uint16_t *mine = ring + threadIdx.x;
  int v = 0;
  for (int k = 0; k < n; k++) {   // slot k: row y0 - r + k
    const int s = stereo_row_sum(pl, pr, W, min(max(y0 - r + k, 0), H - 1), x, d, r);
    mine[k * STEREO_BLOCK] = (uint16_t)s;
    v += s;
  }
  int slot = 0;   // the slot of row y - r, the one that leaves next
  for (int y = y0; y < y1; y++) {
    C[((size_t)y * W + x) * D + d] = (uint16_t)v;   // <= 961 * 30
    if (y + 1 < y1) {
      const int in = stereo_row_sum(pl, pr, W, min(y + 1 + r, H - 1), x, d, r);
      v += in - (int)mine[slot * STEREO_BLOCK];
      mine[slot * STEREO_BLOCK] = (uint16_t)in;
      slot = slot + 1 == n ? 0 : slot + 1;
    }
  }
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
__global__ __launch_bounds__(STEREO_BLOCK) void k_stereo_paths(StereoPaths p) {
  constexpr int WIDTH = D < 64 ? D : 64, LPW = 64 / WIDTH, NV = D / WIDTH;   // lanes per line, lines per wave, disparities per lane
  const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (WIDTH - 1);
  const int Wv = p.W - p.xf;
  int rem = ((int)blockIdx.x * (STEREO_BLOCK / 64) + wave) * LPW + lane / WIDTH;
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
// into).  Shared with sweep.hip (gsaj_common.h); sizes are the caller's to have checked.
template <int D>
static void stereo_paths_launch(const StereoPaths &pp, hipStream_t s) {
  const int Wv = pp.W - pp.xf;
  const int lines = (pp.paths == 8 ? 4 : 0) * (Wv + pp.H - 1) + 2 * pp.H + 2 * Wv;
  constexpr int per_block = (STEREO_BLOCK / 64) * (D < 64 ? 64 / D : 1);
  hipLaunchKernelGGL(k_stereo_paths<D>, dim3((unsigned)((lines + per_block - 1) / per_block)), dim3(STEREO_BLOCK), 0, s, pp);
}

hipError_t launch_stereo_paths(int D, int W, int H, int first_col, int P1, int P2, int paths, const uint16_t *C, uint32_t *S, hipStream_t s) {
  if ((D != 16 && D != 32 && D != 64 && D != 128) || first_col < 0 || first_col >= W || H < 1 || (paths != 4 && paths != 8)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(S, 0, (size_t)W * H * D * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  StereoPaths pp;
  pp.W = W; pp.H = H; pp.P1 = P1; pp.P2 = P2; pp.paths = paths; pp.xf = first_col; pp.C = C; pp.S = S;
  switch (D) {
    case 16: stereo_paths_launch<16>(pp, s); break;
    case 32: stereo_paths_launch<32>(pp, s); break;
    case 64: stereo_paths_launch<64>(pp, s); break;
    default: stereo_paths_launch<128>(pp, s); break;
  }
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
__global__ __launch_bounds__(STEREO_BLOCK) void k_stereo_winner(StereoWinner p) {
  constexpr int WIDTH = D < 64 ? D : 64, LPW = 64 / WIDTH, NV = D / WIDTH, GROUPS = (STEREO_BLOCK / 64) * LPW;
  extern __shared__ unsigned long long stereo_lds[];
  unsigned long long *disp2 = stereo_lds;
  int *d16s = reinterpret_cast<int *>(stereo_lds + p.W);
  const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (WIDTH - 1), g = wave * LPW + lane / WIDTH;
  for (int x = threadIdx.x; x < p.W; x += STEREO_BLOCK) {
    disp2[x] = STEREO_NO_KEY;
    d16s[x] = -16;
  }
  __syncthreads();
  const uint32_t *row = p.S + (size_t)y * p.W * D;
  for (int xb = D; xb < p.W; xb += GROUPS) {   // (uniform: the reductions below are executed by every lane)
    const int x = xb + g;
    const bool active = x < p.W;
    const uint32_t *s = row + (size_t)(active ? x : D) * D;
    uint32_t v[NV], key = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < NV; j++) {
      v[j] = s[sub * NV + j];
      key = min(key, (v[j] << 7) | (uint32_t)(sub * NV + j));   // S < 2^25: the lowest d wins a tie
    }
    key = wave_min<WIDTH>(key);
    const int dstar = (int)(key & 127u);
    const uint32_t best = key >> 7;
    uint32_t rival = 0u;
#pragma unroll
    for (int j = 0; j < NV; j++)
      if (abs(sub * NV + j - dstar) > 1 && v[j] * (uint32_t)(100 - p.uniqueness) < best * 100u) rival = 1u;
    rival = wave_max<WIDTH>(rival);
    if (active && sub == 0 && !rival) {
      int d16 = 16 * dstar;
      if (dstar > 0 && dstar < D - 1) {
        const int sm = (int)s[dstar - 1], sp = (int)s[dstar + 1];
        const int den = max(sm + sp - 2 * (int)best, 1);
        d16 += ((sm - sp) * 16 + den) / (2 * den);   // C division: towards zero
      }
      d16s[x] = d16;
      atomicMin(&disp2[x - dstar], ((unsigned long long)best << 32) | ((unsigned long long)(uint32_t)(p.W - 1 - x) << 8) | (unsigned long long)dstar);
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < p.W; x += STEREO_BLOCK) {
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
  if ((D != 16 && D != 32 && D != 64 && D != 128) || W <= D || W > STEREO_MAX_W) return false;
  out->dynamic_bytes = (size_t)W * (sizeof(unsigned long long) + sizeof(int));
  out->static_bytes = STEREO_WINNER_STATIC_LDS;
  out->limit_bytes = LDS_DEFAULT_LIMIT;
  out->variant = D;
  return true;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
static bool stereo_sizes_ok(const char *who, int W, int H, int D, int paths) {
  if (D != 16 && D != 32 && D != 64 && D != 128) {
    gsaj_set_error("%s: D must be 16, 32, 64 or 128 (D=%d)", who, D);
    return false;
  }
  if (H < 1 || W <= D || W > STEREO_MAX_W || (size_t)W * H * D > (size_t)INT32_MAX) {
    gsaj_set_error("%s: needs D < W <= %d, H >= 1 and W * H * D <= INT_MAX (W=%d H=%d D=%d)", who, STEREO_MAX_W, W, H, D);
    return false;
  }
  if (paths != 4 && paths != 8) {
    gsaj_set_error("%s: paths must be 4 or 8 (paths=%d)", who, paths);
    return false;
  }
  return true;
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
                          const StereoWS &ws, const StereoPaths &pp, const StereoWinner &wp, hipStream_t s) {
  const int Wv = W - D;
  if (stages & GSAJ_STEREO_STAGE_COST) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(k_stereo_prefilter, dim3((unsigned)((n + STEREO_BLOCK - 1) / STEREO_BLOCK), 2), dim3(STEREO_BLOCK), 0, s, W, H, left,
                       left_stride, right, right_stride, ws.pl, ws.pr);
    constexpr int XB = STEREO_BLOCK / D;
    hipLaunchKernelGGL(k_stereo_cost<D>, dim3((unsigned)((Wv + XB - 1) / XB), (unsigned)((H + STEREO_BAND - 1) / STEREO_BAND)), dim3(STEREO_BLOCK),
                       0, s, W, H, r, ws.pl, ws.pr, ws.C);
  }
  if (stages & GSAJ_STEREO_STAGE_PATHS) {
    const hipError_t e = launch_stereo_paths(D, W, H, D, pp.P1, pp.P2, pp.paths, pp.C, pp.S, s);   // S is summed into: zeroed there, on the stream
    if (e != hipSuccess) return e;
  }
  if (stages & GSAJ_STEREO_STAGE_WINNER) {
    LdsRequest lds;
    if (!lds_stereo_winner(W, D, &lds)) return hipErrorInvalidValue;  // (cannot happen: stereo_sizes_ok has passed)
    hipLaunchKernelGGL(k_stereo_winner<D>, dim3((unsigned)H), dim3(STEREO_BLOCK), lds.dynamic_bytes, s, wp);
  }
  return hipGetLastError();
}

extern "C" int gsaj_stereo_match(int W, int H, const uint8_t *left, size_t left_stride, const uint8_t *right, size_t right_stride, int D, int r,
                                 int P1, int P2, int paths, int uniqueness, int lr_max_diff, int stages, void *workspace,
                                 size_t workspace_bytes, int16_t *disp16, float *out_depth, double bf, void *stream) {
  if (!stereo_sizes_ok("gsaj_stereo_match", W, H, D, paths)) return GSAJ_ERR_INVALID_ARGUMENT;
  if (r < 0 || r > 15) {
    gsaj_set_error("gsaj_stereo_match: the block radius must lie in [0, 15] (r=%d)", r);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (P1 < 0 || P1 >= P2 || P2 > 1024) {
    gsaj_set_error("gsaj_stereo_match: needs 0 <= P1 < P2 <= 1024 (P1=%d P2=%d)", P1, P2);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (uniqueness < 0 || uniqueness > 99) {
    gsaj_set_error("gsaj_stereo_match: uniqueness must lie in [0, 99] (uniqueness=%d)", uniqueness);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (lr_max_diff < -1) {
    gsaj_set_error("gsaj_stereo_match: lr_max_diff must be >= -1 (lr_max_diff=%d)", lr_max_diff);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (stages & ~STEREO_STAGES) {
    gsaj_set_error("gsaj_stereo_match: unknown stage bits (stages=0x%x)", (unsigned)stages);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (stages == 0) stages = STEREO_STAGES;
  if (!left || !right || !workspace || !disp16) {
    gsaj_set_error("gsaj_stereo_match: left, right, workspace and disp16 are required");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (left_stride < (size_t)W || right_stride < (size_t)W) {
    gsaj_set_error("gsaj_stereo_match: a row stride is less than W (left_stride=%zu right_stride=%zu W=%d)", left_stride, right_stride, W);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  StereoWS ws;
  const size_t need = stereo_carve(Carver(workspace, BASE_AS_GIVEN), W, H, D, &ws);
  if (workspace_bytes < need) {
    gsaj_set_error("gsaj_stereo_match: the workspace has %zu bytes, gsaj_stereo_workspace_bytes says %zu", workspace_bytes, need);
    return GSAJ_ERR_WORKSPACE_TOO_SMALL;
  }
  if (reinterpret_cast<size_t>(workspace) % 256 != 0 || reinterpret_cast<size_t>(disp16) % 2 != 0 ||
      (out_depth && reinterpret_cast<size_t>(out_depth) % 4 != 0)) {
    gsaj_set_error("gsaj_stereo_match: workspace must be 256-byte, disp16 2-byte and out_depth 4-byte aligned");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (out_depth && (!(bf > 0.0) || !(bf < __builtin_inf()))) {
    gsaj_set_error("gsaj_stereo_match: with out_depth, bf must be positive and finite (bf=%g)", bf);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  StereoPaths pp;
  pp.W = W; pp.H = H; pp.P1 = P1; pp.P2 = P2; pp.paths = paths; pp.xf = D; pp.C = ws.C; pp.S = ws.S;
  StereoWinner wp;
  wp.W = W; wp.H = H; wp.uniqueness = uniqueness; wp.lr_max_diff = lr_max_diff; wp.S = ws.S; wp.disp16 = disp16; wp.depth = out_depth;
  wp.bf = out_depth ? bf : 1.0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  switch (D) {
    case 16: e = stereo_launch<16>(stages, W, H, left, left_stride, right, right_stride, r, ws, pp, wp, s); break;
    case 32: e = stereo_launch<32>(stages, W, H, left, left_stride, right, right_stride, r, ws, pp, wp, s); break;
    case 64: e = stereo_launch<64>(stages, W, H, left, left_stride, right, right_stride, r, ws, pp, wp, s); break;
    default: e = stereo_launch<128>(stages, W, H, left, left_stride, right, right_stride, r, ws, pp, wp, s); break;
  }
  GSAJ_HIP_CHECK(e);
  return GSAJ_OK;
}
