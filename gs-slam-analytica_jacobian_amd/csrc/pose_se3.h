// pose_se3.h -- W2C <- Exp(tau) * W2C and the camera matrices the next render needs (reference utils/pose_utils.py:61-93,
// camera_utils.py:95-109): the pose-state layout and SO(3) exponential of the Adam pose step (pose.hip), and the same update as a
// function for the Levenberg-Marquardt pose step (pose_jac.hip).  k_pose_adam_step keeps its own in-line copy of the update:
// called through this function the compiler contracted one of its products differently, and that kernel's bits stay as they are.
#pragma once
#include "gsaj_common.h"

// pose_state layout (floats): see include/gsaj.h
#define PS_W2C 0
#define PS_M 16
#define PS_V 24
#define PS_STEP 32
#define PS_EXP 33
#define PS_VIEW 35
#define PS_PROJ 51
#define PS_CAMPOS 67
#define PS_TAU 70
#define PS_NORM 76
#define PS_CONV 77

__device__ void so3_exp_and_v(const float *th, float R[9], float V[9]) {
  const float W[9] = {0.f, -th[2], th[1], th[2], 0.f, -th[0], -th[1], th[0], 0.f};
  float W2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) W2[i * 3 + j] = W[i * 3 + 0] * W[0 * 3 + j] + W[i * 3 + 1] * W[1 * 3 + j] + W[i * 3 + 2] * W[2 * 3 + j];
  const float angle = sqrtf(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
  float a, b, c, d;  // R = I + a W + b W2;  V = I + c W + d W2
  if (angle < 1e-5f) {
    a = 1.f; b = 0.5f; c = 0.5f; d = 1.0f / 6.0f;
  } else {
    const float s = sinf(angle), co = cosf(angle), a2 = angle * angle;
    a = s / angle;
    b = (1.f - co) / a2;
    c = b;
    d = (angle - s) / (a2 * angle);
  }
  for (int i = 0; i < 9; i++) {
    const float id = (i % 4 == 0) ? 1.f : 0.f;
    R[i] = id + a * W[i] + b * W2[i];
    V[i] = id + c * W[i] + d * W2[i];
  }
}

// st: a pose state (include/gsaj.h); delta = [rho, theta]; p_projection may be NULL.  The statements of k_pose_adam_step, one for one.
static __device__ void pose_apply_delta(float *st, const float *delta, const float *p_projection, float p_threshold) {
  float R[9], V[9];
  so3_exp_and_v(delta + 3, R, V);
  const float tr[3] = {V[0] * delta[0] + V[1] * delta[1] + V[2] * delta[2], V[3] * delta[0] + V[4] * delta[1] + V[5] * delta[2],
                       V[6] * delta[0] + V[7] * delta[1] + V[8] * delta[2]};
  float w[16], nw[16];
  for (int i = 0; i < 16; i++) w[i] = st[PS_W2C + i];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++)
      nw[i * 4 + j] = R[i * 3 + 0] * w[0 * 4 + j] + R[i * 3 + 1] * w[1 * 4 + j] + R[i * 3 + 2] * w[2 * 4 + j] + tr[i] * w[3 * 4 + j];
  }
  nw[12] = 0.f; nw[13] = 0.f; nw[14] = 0.f; nw[15] = 1.f;
  for (int i = 0; i < 16; i++) st[PS_W2C + i] = nw[i];
  // world_view_transform = W2C^T (row-major), full_proj_transform = W2C^T * projection_matrix, camera centre = -R^T t
  float vw[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) vw[i * 4 + j] = nw[j * 4 + i];
  for (int i = 0; i < 16; i++) st[PS_VIEW + i] = vw[i];
  if (p_projection) {
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        float s = 0.f;
        for (int k = 0; k < 4; k++) s += vw[i * 4 + k] * p_projection[k * 4 + j];
        st[PS_PROJ + i * 4 + j] = s;
      }
  }
  {  // camera_center = inverse(world_view_transform)[3, :3] = -R^-1 t (general 3x3 inverse: W2C may carry a scale)
    const float a = nw[0], b = nw[1], c = nw[2], d = nw[4], e = nw[5], f = nw[6], g = nw[8], h = nw[9], i = nw[10];
    const float A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const float idet = 1.f / (a * A + b * B + c * C);
    const float inv[9] = {A * idet, -(b * i - c * h) * idet, (b * f - c * e) * idet, B * idet, (a * i - c * g) * idet, -(a * f - c * d) * idet,
                          C * idet, -(a * h - b * g) * idet, (a * e - b * d) * idet};
    for (int j = 0; j < 3; j++) st[PS_CAMPOS + j] = -(inv[j * 3 + 0] * nw[3] + inv[j * 3 + 1] * nw[7] + inv[j * 3 + 2] * nw[11]);
  }
  float n2 = 0.f;
  for (int i = 0; i < 6; i++) {
    st[PS_TAU + i] = delta[i];
    n2 += delta[i] * delta[i];
  }
  const float nrm = sqrtf(n2);
  st[PS_NORM] = nrm;
  st[PS_CONV] = (nrm < p_threshold) ? 1.f : 0.f;
}
