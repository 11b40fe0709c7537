// gn_state.h -- the Levenberg-Marquardt state behind the pose state (include/gsaj.h "gn_state" / "gn8_state"; pose_se3.h keeps the
// pose state's own PS_* offsets) and the fp64 fold of the partial rows that the step kernels (pose_jac.hip), the relevel
// (pyramid.hip) and the frame-to-frame alignment (align.hip) share.  The only place in csrc/ that defines these offsets;
// gsaj/_gn_state.py holds the same table for the host and tests/test_cpu_gn_state.py compares the two name for name.
#pragma once
#include "gsaj_common.h"
#include "pose_se3.h"

#define GN_ROW GSAJ_GN_PARTIAL_FLOATS  // H (21, upper triangle by rows), g (6), loss, L_rgb, L_depth, d/da, d/db partials
#define GN8_ROW GSAJ_GN8_PARTIAL_FLOATS  // joint form: H8 (36), g8 (8), loss, L_rgb, L_depth, d/da, d/db partials, 15 zeros

// gn_state fields behind the pose state (include/gsaj.h)
#define GN_LAMBDA 80
#define GN_ACC_LOSS 81
#define GN_HAS 82
#define GN_ACCEPTED 83
#define GN_REJECTED 84
#define GN_LAST 85      // loss, L_rgb, L_depth of the last call
#define GN_ACC_W2C 88
#define GN_H 104
#define GN_G 125
static_assert(GN_G + 6 <= GSAJ_GN_STATE_FLOATS && GSAJ_GN_STATE_FLOATS == 136 && GN_ROW == 32, "gn_state layout");
// joint form: [0:104) as above, then H8, g8 and the accepted exposure; the exposure step x[6], x[7] of the last call goes into the
// two floats the pose state leaves unused behind `converged`
#define GN8_G (GN_H + 36)
#define GN8_ACC_EXP (GN8_G + 8)
#define GN8_DEXP 78
static_assert(GN8_ACC_EXP + 2 <= GSAJ_GN8_STATE_FLOATS && GSAJ_GN8_STATE_FLOATS == 152 && GN8_ROW == 64, "gn8_state layout");
// A row's slots behind H and g: loss, L_rgb, L_depth, then the two floats the step does not read.  The frame-to-frame alignment
// (align.hip) keeps the number of valid pixels in the first of them (gsaj/_gn_state.py: ROW_VALID, Layout.row_valid).  Constants of
// the ROW, not offsets of the state: the #defines of this file are the state's table.
constexpr int GN_ROW_VALID = 21 + 6 + 3, GN8_ROW_VALID = 36 + 8 + 3;
static_assert(GN_ROW_VALID + 2 == GN_ROW && GN8_ROW_VALID + 2 <= GN8_ROW, "the rows' count slots");

// ---- the partial rows summed in slot order, in fp64 ------------------------------------------------------------------------
// GN_SUM_THREADS threads = GROUPS row groups x ROW columns (32 groups of the 32-float row, 16 of the joint form's 64-float row): thread
// (r, c) adds rows r, r + GROUPS, ... of column c, four loads in flight at a time and added in row order, then the groups are added in
// order.  (A frame of 640x480 has 4800 rows: eight groups with one dependent load after the other took 158 us, as long as the
// compositor.)  sums: [ROW] doubles in LDS, complete after the call's barrier.
#define GN_SUM_THREADS 1024
template <int ROW>
__device__ __forceinline__ void gn_sum_rows(const float *__restrict__ partials, int n, double (*red)[ROW], double *sums) {
  constexpr int GROUPS = GN_SUM_THREADS / ROW;
  const int c = threadIdx.x & (ROW - 1), r = threadIdx.x / ROW;
  double acc = 0.0;
  for (int i0 = r; i0 < n; i0 += 4 * GROUPS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * GROUPS;
      v[u] = i < n ? partials[(size_t)i * ROW + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) acc += (double)v[u];
  }
  red[r][c] = acc;
  __syncthreads();
  if (r == 0) {
    double t = red[0][c];
    for (int q = 1; q < GROUPS; q++) t += red[q][c];
    sums[c] = t;
  }
  __syncthreads();
}
