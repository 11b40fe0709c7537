// gaussian_chain.h -- one Gaussian's chain from the reverse compositor's ten sums to dL/d{mean3D, cov3D, scale, rotation, SH}
// and the six pose components (gaussian_chain_geom, gaussian_chain, sh_backward, cov3d_backward): shared by the per-Gaussian
// backward kernels (gaussian_bwd.hip) and by the forward-mode pose Jacobian rows (pose_jac.hip: the chain applied to unit sums).
#pragma once
#include "gsaj_common.h"

// The SH basis constants of the chain, one copy per translation unit that includes this.  The linkage is the includer's choice, because
// it is part of the arithmetic: a `static` table is folded into the instructions as literals (signs and all: other multiplies,
// other contractions), one with external linkage may be written by the host and is loaded from constant memory.  pose_jac.hip was
// built with the first, gaussian_bwd.hip (which defines GSAJ_SH_LINKAGE_EXTERN) with the second; each keeps its instruction stream.
#ifdef GSAJ_SH_LINKAGE_EXTERN
#define GSAJ_SH_LINKAGE
#else
#define GSAJ_SH_LINKAGE static
#endif
GSAJ_SH_LINKAGE __constant__ float bSH_C0 = 0.28209479177387814f;
GSAJ_SH_LINKAGE __constant__ float bSH_C1 = 0.4886025119029199f;
GSAJ_SH_LINKAGE __constant__ float bSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f,
                                0.5462742152960396f};
GSAJ_SH_LINKAGE __constant__ float bSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

__device__ __forceinline__ float3 dnormvdv(float3 v, float3 dv) {
  const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
  const float inv = 1.0f / sqrtf(sum2 * sum2 * sum2);
  float3 o;
  o.x = ((+sum2 - v.x * v.x) * dv.x - v.y * v.x * dv.y - v.z * v.x * dv.z) * inv;
  o.y = (-v.x * v.y * dv.x + (sum2 - v.y * v.y) * dv.y - v.z * v.y * dv.z) * inv;
  o.z = (-v.x * v.z * dv.x - v.y * v.z * dv.y + (sum2 - v.z * v.z) * dv.z) * inv;
  return o;
}

// SH backward.  `sh` holds this Gaussian's coefficients [M][3]; dL/dsh goes to `dL_dsh` (zeros above the active degree).
// dL_dsh may alias sh (the single-view kernel works in place): within a band every coefficient is read before the band's
// gradients overwrite it.  Returns dL/dmean through the view direction.
// MODE 0: dL_dsh[k][ch] = w_k g[ch] (w_k = the basis weights of this view direction, g = the colour gradient masked by the clamp
// flags); MODE 1: dL_dsh[k] = w_k only (the batched path sums w_k g[ch] over views itself; nothing is written above the active
// degree); MODE 2: dL_dsh[k][ch] += w_k g[ch].
template <int MODE>
__device__ __forceinline__ float3 sh_backward(int deg, int M, float3 pos, float3 campos, const float *sh, float *dL_dsh,
                                              const uint8_t *__restrict__ clamped, float3 gcol) {
  const float3 dorig = make_float3(pos.x - campos.x, pos.y - campos.y, pos.z - campos.z);
  const float len = sqrtf(dorig.x * dorig.x + dorig.y * dorig.y + dorig.z * dorig.z);
  const float x = dorig.x / len, y = dorig.y / len, z = dorig.z / len;
  const float g[3] = {gcol.x * (clamped[0] ? 0.f : 1.f), gcol.y * (clamped[1] ? 0.f : 1.f), gcol.z * (clamped[2] ? 0.f : 1.f)};
  float dx[3] = {0.f, 0.f, 0.f}, dy[3] = {0.f, 0.f, 0.f}, dz[3] = {0.f, 0.f, 0.f};
#define SH(k, ch) sh[(k) * 3 + (ch)]
#define OUT(k, w)                                                                  \
  {                                                                                \
    const float _w = (w);                                                          \
    if (MODE == 1) {                                                               \
      dL_dsh[(k)] = _w;                                                            \
    } else if (MODE == 2) {                                                        \
      dL_dsh[(k) * 3 + 0] += _w * g[0];                                            \
      dL_dsh[(k) * 3 + 1] += _w * g[1];                                            \
      dL_dsh[(k) * 3 + 2] += _w * g[2];                                            \
    } else {                                                                       \
      dL_dsh[(k) * 3 + 0] = _w * g[0];                                             \
      dL_dsh[(k) * 3 + 1] = _w * g[1];                                             \
      dL_dsh[(k) * 3 + 2] = _w * g[2];                                             \
    }                                                                              \
  }
  OUT(0, bSH_C0)
  if (deg > 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      dx[ch] = -bSH_C1 * SH(3, ch);
      dy[ch] = -bSH_C1 * SH(1, ch);
      dz[ch] = bSH_C1 * SH(2, ch);
    }
    OUT(1, -bSH_C1 * y) OUT(2, bSH_C1 * z) OUT(3, -bSH_C1 * x)
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        dx[ch] += bSH_C2[0] * y * SH(4, ch) + bSH_C2[2] * 2.f * -x * SH(6, ch) + bSH_C2[3] * z * SH(7, ch) + bSH_C2[4] * 2.f * x * SH(8, ch);
        dy[ch] += bSH_C2[0] * x * SH(4, ch) + bSH_C2[1] * z * SH(5, ch) + bSH_C2[2] * 2.f * -y * SH(6, ch) + bSH_C2[4] * 2.f * -y * SH(8, ch);
        dz[ch] += bSH_C2[1] * y * SH(5, ch) + bSH_C2[2] * 2.f * 2.f * z * SH(6, ch) + bSH_C2[3] * x * SH(7, ch);
      }
      OUT(4, bSH_C2[0] * xy) OUT(5, bSH_C2[1] * yz) OUT(6, bSH_C2[2] * (2.f * zz - xx - yy))
      OUT(7, bSH_C2[3] * xz) OUT(8, bSH_C2[4] * (xx - yy))
      if (deg > 2) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          dx[ch] += (bSH_C3[0] * SH(9, ch) * 3.f * 2.f * xy + bSH_C3[1] * SH(10, ch) * yz + bSH_C3[2] * SH(11, ch) * -2.f * xy +
                     bSH_C3[3] * SH(12, ch) * -3.f * 2.f * xz + bSH_C3[4] * SH(13, ch) * (-3.f * xx + 4.f * zz - yy) +
                     bSH_C3[5] * SH(14, ch) * 2.f * xz + bSH_C3[6] * SH(15, ch) * 3.f * (xx - yy));
          dy[ch] += (bSH_C3[0] * SH(9, ch) * 3.f * (xx - yy) + bSH_C3[1] * SH(10, ch) * xz +
                     bSH_C3[2] * SH(11, ch) * (-3.f * yy + 4.f * zz - xx) + bSH_C3[3] * SH(12, ch) * -3.f * 2.f * yz +
                     bSH_C3[4] * SH(13, ch) * -2.f * xy + bSH_C3[5] * SH(14, ch) * -2.f * yz + bSH_C3[6] * SH(15, ch) * -3.f * 2.f * xy);
          dz[ch] += (bSH_C3[1] * SH(10, ch) * xy + bSH_C3[2] * SH(11, ch) * 4.f * 2.f * yz +
                     bSH_C3[3] * SH(12, ch) * 3.f * (2.f * zz - xx - yy) + bSH_C3[4] * SH(13, ch) * 4.f * 2.f * xz +
                     bSH_C3[5] * SH(14, ch) * (xx - yy));
        }
        OUT(9, bSH_C3[0] * y * (3.f * xx - yy)) OUT(10, bSH_C3[1] * xy * z) OUT(11, bSH_C3[2] * y * (4.f * zz - xx - yy))
        OUT(12, bSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)) OUT(13, bSH_C3[4] * x * (4.f * zz - xx - yy))
        OUT(14, bSH_C3[5] * z * (xx - yy)) OUT(15, bSH_C3[6] * x * (xx - 3.f * yy))
      }
    }
  }
#undef SH
#undef OUT
  if (MODE == 0)
    for (int k = (deg + 1) * (deg + 1) * 3; k < 3 * M; k++) dL_dsh[k] = 0.f;  // coefficients above the active degree
  const float3 ddir = make_float3(dx[0] * g[0] + dx[1] * g[1] + dx[2] * g[2], dy[0] * g[0] + dy[1] * g[1] + dy[2] * g[2],
                                  dz[0] * g[0] + dz[1] * g[1] + dz[2] * g[2]);
  return dnormvdv(dorig, ddir);
}

// dL/dSigma (6-vector, off-diagonals doubled) -> dL/dscale, dL/drot  (backward.cu:426-489): Sigma = R S^2 R^T.
__device__ __forceinline__ void cov3d_backward(const float (&gcov)[6], float3 sc, float4 q, float scale_modifier, float3 &o_scale,
                                               float4 &o_rot) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                         {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                         {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
  const float s[3] = {scale_modifier * sc.x, scale_modifier * sc.y, scale_modifier * sc.z};
  const float dS[3][3] = {{gcov[0], 0.5f * gcov[1], 0.5f * gcov[2]},
                          {0.5f * gcov[1], gcov[3], 0.5f * gcov[4]},
                          {0.5f * gcov[2], 0.5f * gcov[4], gcov[5]}};
  float dA[3][3];  // A = S R^T, dL/dA = 2 A dSigma
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int cc = 0; cc < 3; cc++)
      dA[i][cc] = 2.0f * ((s[i] * R[0][i]) * dS[0][cc] + (s[i] * R[1][i]) * dS[1][cc] + (s[i] * R[2][i]) * dS[2][cc]);
  o_scale.x = R[0][0] * dA[0][0] + R[1][0] * dA[0][1] + R[2][0] * dA[0][2];
  o_scale.y = R[0][1] * dA[1][0] + R[1][1] * dA[1][1] + R[2][1] * dA[1][2];
  o_scale.z = R[0][2] * dA[2][0] + R[1][2] * dA[2][1] + R[2][2] * dA[2][2];
  float gR[3][3];  // dL/dR[j][i] = s_i dA[i][j]
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) gR[j][i] = s[i] * dA[i][j];
  float4 dq;
  dq.x = 2 * z * (gR[1][0] - gR[0][1]) + 2 * y * (gR[0][2] - gR[2][0]) + 2 * x * (gR[2][1] - gR[1][2]);
  dq.y = 2 * y * (gR[0][1] + gR[1][0]) + 2 * z * (gR[0][2] + gR[2][0]) + 2 * r * (gR[2][1] - gR[1][2]) - 4 * x * (gR[2][2] + gR[1][1]);
  dq.z = 2 * x * (gR[0][1] + gR[1][0]) + 2 * r * (gR[0][2] - gR[2][0]) + 2 * z * (gR[2][1] + gR[1][2]) - 4 * y * (gR[2][2] + gR[0][0]);
  dq.w = 2 * r * (gR[1][0] - gR[0][1]) + 2 * x * (gR[0][2] + gR[2][0]) + 2 * y * (gR[2][1] + gR[1][2]) - 4 * z * (gR[1][1] + gR[0][0]);
  o_rot = dq;
}

// Everything one Gaussian contributes for ONE view, from the reverse compositor's sums (s0, s1, s2 = the 10 partials) to
// dL/d{mean3D, cov3D, scale, rotation, SH} and the 6 pose components -- shared by the single-view and the batched kernel so
// that both produce the same bits per view.  p.viewmatrix / projmatrix / campos are that view's.
struct GaussianGrads {
  float m2x, m2y, ca, cb, cc, op, dz;
  float3 col, gm, scale;
  float4 rot;
  float cov[6];
};
// gaussian_chain_geom: everything but the colour -> SH / view-direction part and cov3D -> (scale, rotation): o.gm and tau
// lack the view-direction term (sh_backward's return value: gm += d, tau[0..2] -= d), o.scale / o.rot are not set.
__device__ __forceinline__ void gaussian_chain_geom(const BwdParams &p, float3 mean, const float (&c6)[6], float4 s0, float4 s1, float4 s2,
                                                    GaussianGrads &o, float (&tau)[6]) {
  const float g2x = s0.x, g2y = s0.y;           // dL/dmean2D (NDC-scaled)
  const float gcx = s0.z, gcy = s0.w, gcz = s1.x;  // dL/dconic a, b, c
  const float gop = s1.y;
  const float3 gcol = make_float3(s1.z, s1.w, s2.x);
  const float gz = s2.y;
  // ---- 2. conic -> cov2D -> cov3D, M = J Rcw, t ----
  const float *vm = p.viewmatrix;
  const float fx = p.focal_x, fy = p.focal_y;
  float3 t = xform4x3(vm, mean);
  const float3 pC = t;  // un-clamped camera-space point
  const float limx = 1.3f * p.tanfovx, limy = 1.3f * p.tanfovy;
  const float txtz = t.x / t.z, tytz = t.y / t.z;
  t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
  t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
  const float xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
  const float ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
  const float J00 = fx / t.z, J02 = -(fx * t.x) / (t.z * t.z);
  const float J11 = fy / t.z, J12 = -(fy * t.y) / (t.z * t.z);
  float Rc[3][3], M[2][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Rc[r][c] = vm[4 * c + r];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    M[0][k] = Rc[0][k] * J00 + Rc[2][k] * J02;
    M[1][k] = Rc[1][k] * J11 + Rc[2][k] * J12;
  }
  const float V[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  float MV[2][3];
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) MV[r][k] = M[r][0] * V[k][0] + M[r][1] * V[k][1] + M[r][2] * V[k][2];
  const float a = (MV[0][0] * M[0][0] + MV[0][1] * M[0][1] + MV[0][2] * M[0][2]) + 0.3f;
  const float b = MV[1][0] * M[0][0] + MV[1][1] * M[0][1] + MV[1][2] * M[0][2];
  const float c = (MV[1][0] * M[1][0] + MV[1][1] * M[1][1] + MV[1][2] * M[1][2]) + 0.3f;
  const float denom = a * c - b * b;
  float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
  const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
  float gcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (denom2inv != 0.f) {
    dL_da = denom2inv * (-c * c * gcx + 2 * b * c * gcy + (denom - a * c) * gcz);
    dL_dc = denom2inv * (-a * a * gcz + 2 * a * b * gcy + (denom - a * c) * gcx);
    dL_db = denom2inv * 2 * (b * c * gcx - (denom + 2 * b * b) * gcy + a * b * gcz);
    gcov[0] = (M[0][0] * M[0][0] * dL_da + M[0][0] * M[1][0] * dL_db + M[1][0] * M[1][0] * dL_dc);
    gcov[3] = (M[0][1] * M[0][1] * dL_da + M[0][1] * M[1][1] * dL_db + M[1][1] * M[1][1] * dL_dc);
    gcov[5] = (M[0][2] * M[0][2] * dL_da + M[0][2] * M[1][2] * dL_db + M[1][2] * M[1][2] * dL_dc);
    gcov[1] = 2 * M[0][0] * M[0][1] * dL_da + (M[0][0] * M[1][1] + M[0][1] * M[1][0]) * dL_db + 2 * M[1][0] * M[1][1] * dL_dc;
    gcov[2] = 2 * M[0][0] * M[0][2] * dL_da + (M[0][0] * M[1][2] + M[0][2] * M[1][0]) * dL_db + 2 * M[1][0] * M[1][2] * dL_dc;
    gcov[4] = 2 * M[0][2] * M[0][1] * dL_da + (M[0][1] * M[1][2] + M[0][2] * M[1][1]) * dL_db + 2 * M[1][1] * M[1][2] * dL_dc;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) o.cov[k] = gcov[k];
  float dM[2][3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    dM[0][k] = 2 * MV[0][k] * dL_da + MV[1][k] * dL_db;
    dM[1][k] = 2 * MV[1][k] * dL_dc + MV[0][k] * dL_db;
  }
  const float dJ00 = Rc[0][0] * dM[0][0] + Rc[0][1] * dM[0][1] + Rc[0][2] * dM[0][2];
  const float dJ02 = Rc[2][0] * dM[0][0] + Rc[2][1] * dM[0][1] + Rc[2][2] * dM[0][2];
  const float dJ11 = Rc[1][0] * dM[1][0] + Rc[1][1] * dM[1][1] + Rc[1][2] * dM[1][2];
  const float dJ12 = Rc[2][0] * dM[1][0] + Rc[2][1] * dM[1][1] + Rc[2][2] * dM[1][2];
  const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
  float3 gt;
  gt.x = xmul * -fx * tz2 * dJ02;
  gt.y = ymul * -fy * tz2 * dJ12;
  gt.z = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2 * fx * t.x) * tz3 * dJ02 + (2 * fy * t.y) * tz3 * dJ12;
  // tau: rho += g, theta += t x g (clamped t) + sum_k col_k(Rcw) x dL/dcol_k(Rcw)
  const float3 txg = cross3(t, gt);
  tau[0] += gt.x; tau[1] += gt.y; tau[2] += gt.z;
  tau[3] += txg.x; tau[4] += txg.y; tau[5] += txg.z;
  float3 gm = make_float3(Rc[0][0] * gt.x + Rc[1][0] * gt.y + Rc[2][0] * gt.z,
                          Rc[0][1] * gt.x + Rc[1][1] * gt.y + Rc[2][1] * gt.z,
                          Rc[0][2] * gt.x + Rc[1][2] * gt.y + Rc[2][2] * gt.z);
  {
    float3 th = make_float3(0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float3 ck = make_float3(Rc[0][k], Rc[1][k], Rc[2][k]);
      const float3 gk = make_float3(J00 * dM[0][k], J11 * dM[1][k], J02 * dM[0][k] + J12 * dM[1][k]);
      const float3 cr = cross3(ck, gk);
      th.x += cr.x; th.y += cr.y; th.z += cr.z;
    }
    tau[3] += th.x; tau[4] += th.y; tau[5] += th.z;
  }

  // ---- 3. mean2D -> mean3D, tau ----
  const float *pj = p.projmatrix;
  const float4 mh = xform4x4(pj, mean);
  const float mw = 1.0f / (mh.w + 0.0000001f);
  const float mul1 = (pj[0] * mean.x + pj[4] * mean.y + pj[8] * mean.z + pj[12]) * mw * mw;
  const float mul2 = (pj[1] * mean.x + pj[5] * mean.y + pj[9] * mean.z + pj[13]) * mw * mw;
  gm.x += (pj[0] * mw - pj[3] * mul1) * g2x + (pj[1] * mw - pj[3] * mul2) * g2y;
  gm.y += (pj[4] * mw - pj[7] * mul1) * g2x + (pj[5] * mw - pj[7] * mul2) * g2y;
  gm.z += (pj[8] * mw - pj[11] * mul1) * g2x + (pj[9] * mw - pj[11] * mul2) * g2y;
  {
    const float alpha_ = 1.0f * mw, beta_ = -mh.x * mw * mw, gamma_ = -mh.y * mw * mw;
    const float pa = p.projmatrix_raw[0], pb = p.projmatrix_raw[5], pe = p.projmatrix_raw[11];
    const float3 d1 = make_float3(alpha_ * pa, 0.f, beta_ * pe), d2 = make_float3(0.f, alpha_ * pb, gamma_ * pe);
    const float3 c1 = cross3(pC, d1), c2 = cross3(pC, d2);
    tau[0] += g2x * d1.x + g2y * d2.x; tau[1] += g2x * d1.y + g2y * d2.y; tau[2] += g2x * d1.z + g2y * d2.z;
    tau[3] += g2x * c1.x + g2y * c2.x; tau[4] += g2x * c1.y + g2y * c2.y; tau[5] += g2x * c1.z + g2y * c2.z;
  }
  // ---- 4. depth -> mean3D, tau: dz/dtau = [0,0,1, y, -x, 0] ----
  gm.x += gz * vm[2]; gm.y += gz * vm[6]; gm.z += gz * vm[10];
  tau[2] += gz;
  tau[3] += gz * pC.y;
  tau[4] += gz * -pC.x;
  o.m2x = g2x; o.m2y = g2y; o.ca = gcx; o.cb = gcy; o.cc = gcz; o.op = gop; o.col = gcol; o.dz = gz; o.gm = gm;
}
__device__ __forceinline__ void gaussian_chain(const BwdParams &p, float3 mean, const float (&c6)[6], float3 sc, float4 q,
                                               const uint8_t (&cl)[3], float4 s0, float4 s1, float4 s2, const float *sh_row,
                                               float *dsh_row, bool want_scale_rot, GaussianGrads &o, float (&tau)[6]) {
  gaussian_chain_geom(p, mean, c6, s0, s1, s2, o, tau);
  // ---- 5. colour -> SH, view direction -> mean3D, tau ----
  if (p.shs) {
    const float3 cam = make_float3(p.campos[0], p.campos[1], p.campos[2]);
    const float3 dmean = sh_backward<0>(p.D, p.M, mean, cam, sh_row, dsh_row, cl, o.col);
    o.gm.x += dmean.x; o.gm.y += dmean.y; o.gm.z += dmean.z;
    tau[0] -= dmean.x; tau[1] -= dmean.y; tau[2] -= dmean.z;
  }
  // ---- 6. cov3D -> scale, rotation ----
  if (p.scales && want_scale_rot) cov3d_backward(o.cov, sc, q, p.scale_modifier, o.scale, o.rot);
}
