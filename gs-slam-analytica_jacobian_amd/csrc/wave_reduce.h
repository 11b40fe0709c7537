// wave_reduce.h -- the only home of lane scans and reductions: every kernel's __shfl_xor butterfly and __shfl_up ladder is one of these.
//
// All of it is register-only and force-inlined; nothing here owns LDS.  Where a workgroup form needs one slot per wave the
// caller passes the array (as row_rank() in row_move.h does), so a kernel's LDS is what the kernel declares.  Workgroups are
// one-dimensional and a multiple of 64 lanes wide: lane = threadIdx.x & 63, wave = threadIdx.x >> 6.
//
//   wave_sum / wave_min / wave_max   xor butterfly over WIDTH lanes (64, or a half-wave), steps WIDTH/2 ... 1, the result in
//                                    every lane.  Floating-point sums are compared bit for bit elsewhere: this tree is fixed.
//   wave_incl_scan_add / _max        the __shfl_up ladder (steps 1 ... WIDTH/2) over uint32_t
//   block_excl_scan_add              workgroup exclusive scan: wave scans + one LDS hop for the wave totals, ONE barrier;
//   block_scan_total                 the workgroup's total from the same LDS words
//   block_excl_scan_runs             the same over n items, a contiguous run per lane, with the largest item
//   block_fold (_put / _get)         workgroup reduction: butterflies + one LDS hop, ONE barrier, the waves folded in wave order
//   reduce4 / store4                 four per-lane partials through one tree (7 cross-lane steps where four butterflies take 24)
//   reduce10 / store10               ten per-lane partials at once, register-only:
//
// v_permlane32_swap / v_permlane16_swap exchange half-waves / odd-even rows between two
// registers, so ONE swap + ONE add both halves the number of live registers and folds one
// lane bit: 10 -> 5 -> 3 registers.  Four DPP row rotations then finish each 16-lane row.
// After reduce10():  row r = lane>>4 holds  x0 -> v[{0,2,1,3}[r]],  x1 -> v[{4,6,5,7}[r]],
//                    x2 -> v[{8,8,9,9}[r]]   in every lane of the row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The value parameter of every wave primitive, as the __shfl_* it is handed to declare theirs: the compiler then treats the argument
// exactly as it treats the operand of a shuffle written at the call site (a plain by-value parameter is `noundef`, which changes
// the code around the call: up to 10 VGPRs in k_chain_window).
#define WAVE_MAYBE_UNDEF __attribute__((maybe_undef))

// ---- xor butterfly: all-reduce over each aligned group of WIDTH lanes -------------------------------------------------------
struct lane_add {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct lane_min {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); }
};
struct lane_max {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); }
};
template <int WIDTH = 64, typename T, typename Op>
__device__ __forceinline__ T wave_allreduce(WAVE_MAYBE_UNDEF T v, Op op) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_sum(WAVE_MAYBE_UNDEF T v) {
  return wave_allreduce<WIDTH>(v, lane_add());
}
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_min(WAVE_MAYBE_UNDEF T v) {
  return wave_allreduce<WIDTH>(v, lane_min());
}
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_max(WAVE_MAYBE_UNDEF T v) {
  return wave_allreduce<WIDTH>(v, lane_max());
}

// ---- __shfl_up ladder: inclusive scan over each aligned group of WIDTH lanes ------------------------------------------------
template <int WIDTH = 64, typename Op>
__device__ __forceinline__ uint32_t wave_incl_scan(WAVE_MAYBE_UNDEF uint32_t x, Op op) {
  const int lane = threadIdx.x & (WIDTH - 1);
#pragma unroll
  for (int o = 1; o < WIDTH; o <<= 1) {
    const uint32_t up = __shfl_up(x, o, WIDTH);
    if (lane >= o) x = op(x, up);
  }
  return x;
}
template <int WIDTH = 64>
__device__ __forceinline__ uint32_t wave_incl_scan_add(WAVE_MAYBE_UNDEF uint32_t x) {
  return wave_incl_scan<WIDTH>(x, lane_add());
}
template <int WIDTH = 64>
__device__ __forceinline__ uint32_t wave_incl_scan_max(WAVE_MAYBE_UNDEF uint32_t x) {
  return wave_incl_scan<WIDTH>(x, lane_max());
}

// ---- workgroup exclusive scan of one value per lane, NWAVES waves (every lane must call) ------------------------------------
// wsum: NWAVES words of the caller's LDS; they hold the wave totals until the caller reuses them, and block_scan_total is
// their sum, the workgroup's total (as row_total() in row_move.h).  A running offset across several calls stays with the caller
// (k_scatter_instances, k_rs_scan): this has ONE barrier.
template <int NWAVES>
__device__ __forceinline__ uint32_t block_excl_scan_add(uint32_t x, uint32_t *wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan_add(x);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0u;
#pragma unroll 4  // (four totals in flight at a time: the sixteen of a 1024-lane workgroup at once cost k_rs_scan 5 VGPRs)
  for (int w = 0; w < NWAVES; w++) {
    const uint32_t v = wsum[w];
    if (w < wave) before += v;
  }
  // the same in every lane of a wave: a scalar register, formed HERE (left as a vector value the compiler moved the sum behind
  // k_sd_pick's bookkeeping branch and kept the wave totals alive across it: 4 VGPRs)
  before = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
  return before + incl - x;
}
template <int NWAVES>
__device__ __forceinline__ uint32_t block_scan_total(const uint32_t *wsum) {
  uint32_t total = 0u;
#pragma unroll
  for (int w = 0; w < NWAVES; w++) total += wsum[w];
  return total;
}

// ---- workgroup exclusive scan of n items: each lane sums a contiguous run, the run totals go through block_excl_scan_add, then
// each lane rewrites its run (out may be in).  Returns the total; largest = the largest item.  wsum, wmax: NWAVES words each of
// the caller's LDS.  In: the input's pointer type -- force-inlined, so an LDS array is still read as LDS.
template <int NWAVES, typename In>
__device__ __forceinline__ uint32_t block_excl_scan_runs(In in, uint32_t *out, int n, uint32_t *wsum, uint32_t *wmax, uint32_t &largest) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n + NWAVES * 64 - 1) / (NWAVES * 64);
  const int b0 = min(n, tid * per), b1 = min(n, b0 + per);
  uint32_t s = 0, mx = 0;
  for (int i = b0; i < b1; i++) {
    const uint32_t v = in[i];
    s += v;
    mx = max(mx, v);
  }
  mx = wave_max(mx);
  if (lane == 0) wmax[wave] = mx;
  uint32_t run = block_excl_scan_add<NWAVES>(s, wsum);
  const uint32_t total = block_scan_total<NWAVES>(wsum);
  largest = 0u;
#pragma unroll
  for (int w = 0; w < NWAVES; w++) largest = max(largest, wmax[w]);
  for (int i = b0; i < b1; i++) {
    const uint32_t v = in[i];
    out[i] = run;
    run += v;
  }
  return total;
}

// ---- ordered workgroup fold of N values per lane, NWAVES waves (every lane must call) ----------------------------------------
// slots: N rows of NWAVES words of the caller's LDS.  block_fold_put: the butterfly of each value, then lane 0 of each wave
// writes its wave's N results; block_fold_get, behind a barrier: row by row, the waves folded in order 0, 1, 2, ... -- a fixed
// tree, whatever the value type.  block_fold is the two around ONE barrier, the result in thread 0 only.  A caller whose values
// do not share one operation (a bounding box: three minima, three maxima) puts each group, has its own barrier, and gets.
template <int NWAVES, int N, typename T, typename Op>
__device__ __forceinline__ void block_fold_put(T *v, T (*slots)[NWAVES], Op op) {
#pragma unroll
  for (int c = 0; c < N; c++) v[c] = wave_allreduce(v[c], op);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < N; c++) slots[c][threadIdx.x >> 6] = v[c];
  }
}
template <int NWAVES, typename T, typename Op>
__device__ __forceinline__ T block_fold_get(const T *row, Op op) {
  T s = row[0];
  for (int w = 1; w < NWAVES; w++) s = op(s, row[w]);
  return s;
}
template <int NWAVES, int N, typename T, typename Op>
__device__ __forceinline__ void block_fold(T *v, T (*slots)[NWAVES], Op op) {
  block_fold_put<NWAVES, N>(v, slots, op);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < N; c++) v[c] = block_fold_get<NWAVES>(slots[c], op);
  }
}

// ---- ten values at once -----------------------------------------------------------------------------------------------------

typedef unsigned gsaj_u32x2 __attribute__((ext_vector_type(2)));

// (A, B) -> lanes 0-31: A_lo + A_hi, lanes 32-63: B_lo + B_hi   (sum across lane bit 5)
__device__ __forceinline__ float merge32(float a, float b) {
  gsaj_u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// (A, B) -> even rows: A_r + A_{r+1}, odd rows: B_{r-1} + B_r      (sum across lane bit 4)
__device__ __forceinline__ float merge16(float a, float b) {
  gsaj_u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_allreduce(float v) {  // sum over the 16 lanes of each row
  v = dpp_add<0x128>(v);  // row_ror:8
  v = dpp_add<0x124>(v);  // row_ror:4
  v = dpp_add<0x122>(v);  // row_ror:2
  v = dpp_add<0x121>(v);  // row_ror:1
  return v;
}
// Four values at once: after reduce4() every lane of row r = lane>>4 holds the wave's sum of v{0,2,1,3}[r]; store4: the first lane of
// each row stores it, a[0..3] = the sums of v0..v3.  A fixed tree of depth 6, like wave_sum's, in another order.
__device__ __forceinline__ float reduce4(float v0, float v1, float v2, float v3) {
  return row_allreduce(merge16(merge32(v0, v1), merge32(v2, v3)));
}
__device__ __forceinline__ void store4(float *a, int lane, float x) {
  if ((lane & 15) == 0) {
    const int r = lane >> 4;
    a[((r & 1) << 1) | (r >> 1)] = x;
  }
}
__device__ __forceinline__ void reduce10(const float (&v)[10], float &x0, float &x1, float &x2) {
  const float w0 = merge32(v[0], v[1]), w1 = merge32(v[2], v[3]), w2 = merge32(v[4], v[5]), w3 = merge32(v[6], v[7]),
              w4 = merge32(v[8], v[9]);
  x0 = row_allreduce(merge16(w0, w1));
  x1 = row_allreduce(merge16(w2, w3));
  x2 = row_allreduce(merge16(w4, w4));
}
// Lane 0 of each row stores its three totals into a 12-float slot (a[0..9] = v[0..9]).
__device__ __forceinline__ void store10(float *a, int lane, float x0, float x1, float x2) {
  if ((lane & 15) == 0) {
    const int r = lane >> 4;
    const int k = ((r & 1) << 1) | (r >> 1);
    a[k] = x0;
    a[4 + k] = x1;
    if ((r & 1) == 0) a[8 + (r >> 1)] = x2;
  }
}
