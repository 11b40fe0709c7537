// densify_prune.hip -- clone, split and prune of the Gaussian map from one plan: gsaj_densify_plan, gsaj_densify_counts,
// gsaj_densify_rows, gsaj_densify_children, gsaj_densify_noise (include/gsaj.h states the semantics).  What the reference does
// with densify_and_clone, densify_and_split and the final prune_points (gaussian_splatting/scene/gaussian_model.py:599-765: about
// twenty boolean-mask gathers and three torch.cat reallocations of the six parameters and their twelve Adam moments) is one pass
// over the rows that classifies each (a code byte and three block counts), one exclusive scan that turns the counts into the
// destination offsets of the 2 + N output segments, one launch that writes every segment of a whole table of tensors, and one
// launch that overwrites the children's positions and log-scales.  Structure as compact.hip, the block counts and the row mover
// from the header the two share (row_move.h): no atomics, no tickets, the result does not depend on the launch geometry.  Built
// with -ffp-contract=off: the decisions and the child values restate fp32 tensor operations one rounding at a time.
#include "row_move.h"

#define DN_HDR 8       // words in front of the counters: [0] kept originals [1] clones [2] children per copy [3] P'' [4] P [5] N

#define DN_ORIGINAL 1u  // code bits: what a source row emits
#define DN_CLONE 2u
#define DN_CHILDREN 4u

struct DensifyRule {  // every threshold already rounded to fp32 on the host
  float grad_threshold, t_dense, t_big, min_opacity, divisor;
  int size_rule, size_all, stages, S, N;
};

__device__ __forceinline__ float dn_max(float m, float e) { return (e > m || e != e) ? e : m; }  // torch.max: a NaN wins

// The code byte of row i and the block's three counts.  counters: [nb] originals, [nb] clones, N x [nb] children, one zero.
__global__ void __launch_bounds__(ROW_BLOCK) k_dn_plan(int P, DensifyRule r, const float *__restrict__ accum, const float *__restrict__ denom,
                                                       int n_grads, const float *__restrict__ scaling, const float *__restrict__ opacity,
                                                       uint8_t *__restrict__ code, uint32_t *__restrict__ ws) {
  __shared__ uint32_t wcnt[3][ROW_BLOCK / GSAJ_WAVE];
  const size_t i = (size_t)blockIdx.x * ROW_BLOCK + threadIdx.x;
  uint32_t c = 0u;
  if (i < (size_t)P) {
    float g;
    if (denom) {
      g = accum[i] / denom[i];
      if (g != g) g = 0.f;
    } else {
      g = i < (size_t)n_grads ? accum[i] : 0.f;
    }
    float m, mc;  // the largest activated scale of the row, and of a child of the row
    {
      const float e = expf(scaling[i * (size_t)r.S]);
      m = e;
      mc = expf(logf(e / r.divisor));
    }
    for (int j = 1; j < r.S; ++j) {
      const float e = expf(scaling[i * (size_t)r.S + j]);
      m = dn_max(m, e);
      mc = dn_max(mc, expf(logf(e / r.divisor)));
    }
    const bool clone = (r.stages & GSAJ_DENSIFY_CLONE) && fabsf(g) >= r.grad_threshold && m <= r.t_dense;
    const bool split = (r.stages & GSAJ_DENSIFY_SPLIT) && g >= r.grad_threshold && m > r.t_dense;
    bool gone = false, child_gone = false;
    if (r.stages & GSAJ_DENSIFY_PRUNE) {
      const float o = 1.f / (1.f + expf(-opacity[i]));
      const bool faint = o < r.min_opacity;
      gone = faint || (r.size_rule && (r.size_all || m > r.t_big));
      child_gone = faint || (r.size_rule && (r.size_all || mc > r.t_big));
    }
    if (!split && !gone) c |= DN_ORIGINAL;
    if (clone && !gone) c |= DN_CLONE;
    if (split && !child_gone) c |= DN_CHILDREN;
    code[i] = (uint8_t)c;
  }
  row_post((c & DN_ORIGINAL) != 0u, wcnt[0]);
  row_post((c & DN_CLONE) != 0u, wcnt[1]);
  row_post((c & DN_CHILDREN) != 0u, wcnt[2]);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t *counts = gsaj_shift(ws, sizeof(uint32_t) * DN_HDR);
    const size_t nb = gridDim.x;
    const uint32_t k2 = row_total(wcnt[2]);
    counts[blockIdx.x] = row_total(wcnt[0]);
    counts[nb + blockIdx.x] = row_total(wcnt[1]);
    for (int n = 0; n < r.N; ++n) counts[(size_t)(2 + n) * nb + blockIdx.x] = k2;
    if (blockIdx.x == 0) {
      counts[(size_t)(2 + r.N) * nb] = 0u;
      ws[4] = (uint32_t)P; ws[5] = (uint32_t)r.N; ws[6] = 0u; ws[7] = 0u;
    }
  }
}

// the small second kernel: the four counts from the scanned offsets to the fixed words gsaj_densify_counts reads
__global__ void __launch_bounds__(GSAJ_WAVE) k_dn_totals(uint32_t nb, uint32_t N, uint32_t *__restrict__ ws) {
  if (threadIdx.x == 0) {
    const uint32_t *offs = gsaj_shift(ws, sizeof(uint32_t) * DN_HDR);
    ws[0] = offs[nb];
    ws[1] = offs[2 * (size_t)nb] - offs[nb];
    ws[2] = offs[3 * (size_t)nb] - offs[2 * (size_t)nb];
    ws[3] = offs[(size_t)(2 + N) * nb];
  }
}

// Workgroup (b, t, seg) writes rows [offs[seg][b], offs[seg][b + 1]) of tensor t: the rows source block b emits into segment seg
// (0 originals, 1 clones, 2 + n the children of copy n), in order.
__global__ void __launch_bounds__(ROW_BLOCK) k_dn_rows(int P, int N, RowTable tb, const uint8_t *__restrict__ code_,
                                                       const uint32_t *__restrict__ ws) {
  if (ws[4] != (uint32_t)P || ws[5] != (uint32_t)N) return;  // not the plan of these tensors: nothing is read or written
  const uint32_t *offs = gsaj_shift(ws, sizeof(uint32_t) * DN_HDR);
  const uint32_t seg = blockIdx.z;
  const size_t slot = (size_t)seg * gridDim.x + blockIdx.x;
  const uint32_t off = offs[slot], count = offs[slot + 1] - off;
  if (!row_count_ok(count)) return;  // (the mover refuses the same; here for the zero fill below, and before the table is read)
  const uint32_t w = tb.w[blockIdx.y];
  const size_t row0 = (size_t)blockIdx.x * ROW_BLOCK;
  const row_src32 s32 = (row_src32)((unsigned long long)tb.src[blockIdx.y]) + row0 * w;
  const row_dst32 d32 = (row_dst32)((unsigned long long)tb.dst[blockIdx.y]) + (size_t)off * w;

  if (seg != 0u && ((tb.zero_new >> blockIdx.y) & 1u)) {  // new rows of an Adam moment
    for (uint32_t j = threadIdx.x; j < count * w; j += ROW_BLOCK) d32[j] = 0u;
    return;
  }
  const row_bytes_t code = (row_bytes_t)((unsigned long long)code_);
  const uint32_t bit = seg == 0u ? DN_ORIGINAL : seg == 1u ? DN_CLONE : DN_CHILDREN;
  row_move_segment(s32, d32, w, tb.magic[blockIdx.y], count,
                   [=](uint32_t r) { return row0 + r < (size_t)P && ((uint32_t)code[row0 + r] & bit) != 0u; });
}

// ---- Philox4x32-10 and the normal draws of (row i, copy n) -------------------------------------------------------------------
struct dn_z3 { float x, y, z; };

__host__ __device__ __forceinline__ void dn_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ dn_z3 dn_draw(uint32_t i, uint32_t n, uint32_t k0, uint32_t k1) {
  uint32_t x[4];
  dn_philox(i, n, 0u, 0u, k0, k1, x);
  const float two_pi = 6.28318530717958647692f;
  const float u1a = ((float)(x[0] >> 9) + 0.5f) * 1.1920928955078125e-07f, u2a = (float)(x[1] >> 8) * 5.9604644775390625e-08f;
  const float u1b = ((float)(x[2] >> 9) + 0.5f) * 1.1920928955078125e-07f, u2b = (float)(x[3] >> 8) * 5.9604644775390625e-08f;
  const float ra = sqrtf(-2.f * logf(u1a)), rb = sqrtf(-2.f * logf(u1b));
  const float ta = two_pi * u2a, tb = two_pi * u2b;
  dn_z3 z;
  z.x = ra * cosf(ta);
  z.y = ra * sinf(ta);
  z.z = rb * cosf(tb);
  return z;
}

__global__ void __launch_bounds__(ROW_BLOCK) k_dn_noise(int P, uint32_t k0, uint32_t k1, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * ROW_BLOCK + threadIdx.x;
  if (i >= (size_t)P) return;
  const dn_z3 z = dn_draw((uint32_t)i, blockIdx.y, k0, k1);
  float *o = out + ((size_t)blockIdx.y * (size_t)P + i) * 3;
  o[0] = z.x; o[1] = z.y; o[2] = z.z;
}

// Lane (i, n) with children emitted: xyz = R(q_i) (exp(s_i) o z_{i,n}) + xyz_i and log(exp(s_i) / d) into the child's row.
__global__ void __launch_bounds__(ROW_BLOCK) k_dn_children(int P, int S, int N, float divisor, const float *__restrict__ xyz,
                                                           const float *__restrict__ scaling, const float *__restrict__ rotation,
                                                           const float *__restrict__ noise, uint32_t k0, uint32_t k1,
                                                           const uint8_t *__restrict__ code, const uint32_t *__restrict__ ws,
                                                           float *__restrict__ dst_xyz, float *__restrict__ dst_scaling) {
  __shared__ uint32_t wcnt[ROW_BLOCK / GSAJ_WAVE];
  if (ws[4] != (uint32_t)P || ws[5] != (uint32_t)N) return;
  const uint32_t *offs = gsaj_shift(ws, sizeof(uint32_t) * DN_HDR);
  const uint32_t n = blockIdx.y;
  const size_t slot = (size_t)(2u + n) * gridDim.x + blockIdx.x;
  const uint32_t off = offs[slot], count = offs[slot + 1] - off;
  if (!row_count_ok(count)) return;
  const size_t i = (size_t)blockIdx.x * ROW_BLOCK + threadIdx.x;
  const bool emit = i < (size_t)P && (code[i] & DN_CHILDREN) != 0u;
  const uint32_t rank = row_rank(emit, wcnt);
  if (!emit || rank >= count) return;
  const size_t row = (size_t)off + rank;

  dn_z3 z;
  if (noise) {
    const float *zp = noise + ((size_t)n * (size_t)P + i) * 3;
    z.x = zp[0]; z.y = zp[1]; z.z = zp[2];
  } else {
    z = dn_draw((uint32_t)i, n, k0, k1);
  }
  float e[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j < S) {
      e[j] = expf(scaling[i * (size_t)S + j]);
      dst_scaling[row * (size_t)S + j] = logf(e[j] / divisor);
    } else {
      e[j] = e[0];  // isotropic: the one scale multiplies the three components
    }
  }
  const float v0 = e[0] * z.x, v1 = e[1] * z.y, v2 = e[2] * z.z;  // torch.normal(0, std): 0 + std z

  const float *q = rotation + i * 4;
  const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  const float r = q0 / norm, x = q1 / norm, y = q2 / norm, w = q3 / norm;  // (w: the reference's z)
  const float R00 = 1.f - 2.f * (y * y + w * w), R01 = 2.f * (x * y - r * w), R02 = 2.f * (x * w + r * y);
  const float R10 = 2.f * (x * y + r * w), R11 = 1.f - 2.f * (x * x + w * w), R12 = 2.f * (y * w - r * x);
  const float R20 = 2.f * (x * w - r * y), R21 = 2.f * (y * w + r * x), R22 = 1.f - 2.f * (x * x + y * y);
  const float *mu = xyz + i * 3;
  float *o = dst_xyz + row * 3;
  o[0] = ((R00 * v0 + R01 * v1) + R02 * v2) + mu[0];
  o[1] = ((R10 * v0 + R11 * v1) + R12 * v2) + mu[1];
  o[2] = ((R20 * v0 + R21 * v1) + R22 * v2) + mu[2];
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
static bool dn_bad_pn(int P, int N) { return P <= 0 || N < 1 || N > GSAJ_DENSIFY_MAX_SPLIT || (size_t)P * (size_t)(N + 1) > 0x7fffffffull; }

extern "C" size_t gsaj_densify_workspace_bytes(int P, int N) {
  if (dn_bad_pn(P, N)) return 0;
  return gsaj_align(sizeof(uint32_t) * (DN_HDR + (size_t)(2 + N) * row_blocks(P) + 1));
}

extern "C" int gsaj_densify_plan(int P, int S, int N, int stages, const float *accum, const float *denom, int n_grads, const float *scaling,
                                 const float *opacity, float grad_threshold, float t_dense, float t_big, float min_opacity,
                                 int size_rule, int size_all, uint8_t *code, void *densify_ws, void *stream) {
  if (dn_bad_pn(P, N) || (S != 1 && S != 3) || !accum || !scaling || !opacity || !code || !densify_ws || !(grad_threshold > 0.f) ||
      stages < 0 || stages > (GSAJ_DENSIFY_CLONE | GSAJ_DENSIFY_SPLIT | GSAJ_DENSIFY_PRUNE) || (!denom && (n_grads < 0 || n_grads > P))) {
    gsaj_set_error("gsaj_densify_plan: invalid argument (P=%d S=%d N=%d stages=%d grad_threshold=%g n_grads=%d; P must be positive, S 1 or 3, "
                   "N 1..%d, the threshold greater than 0, n_grads 0..P without denom, no null pointer)", P, S, N, stages,
                   (double)grad_threshold, n_grads, GSAJ_DENSIFY_MAX_SPLIT);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ws = static_cast<uint32_t *>(densify_ws);
  const size_t nb = row_blocks(P);
  DensifyRule r;
  r.grad_threshold = grad_threshold; r.t_dense = t_dense; r.t_big = t_big; r.min_opacity = min_opacity;
  r.divisor = (float)(0.8 * N);
  r.size_rule = size_rule ? 1 : 0; r.size_all = size_all ? 1 : 0; r.stages = stages; r.S = S; r.N = N;
  hipLaunchKernelGGL(k_dn_plan, dim3((unsigned)nb), dim3(ROW_BLOCK), 0, s, P, r, accum, denom, n_grads, scaling, opacity, code, ws);
  launch_exclusive_scan_u32((int)((size_t)(2 + N) * nb + 1), ws + DN_HDR, s);
  hipLaunchKernelGGL(k_dn_totals, dim3(1), dim3(GSAJ_WAVE), 0, s, (uint32_t)nb, (uint32_t)N, ws);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_densify_counts(const void *densify_ws, void *stream, int *counts) {
  if (!densify_ws || !counts) {
    gsaj_set_error("gsaj_densify_counts: invalid argument (no null pointer)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  uint32_t host[4] = {0u, 0u, 0u, 0u};
  GSAJ_HIP_CHECK(hipMemcpyAsync(host, densify_ws, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  for (int k = 0; k < 4; ++k) counts[k] = (int)host[k];
  return GSAJ_OK;
}

extern "C" int gsaj_densify_rows(int P, int N, int n_tensors, const void *const *src, void *const *dst, const int *row_bytes,
                                 const int *zero_new, const uint8_t *code, const void *densify_ws, void *stream) {
  if (dn_bad_pn(P, N) || n_tensors < 1 || n_tensors > GSAJ_DENSIFY_MAX_TENSORS || !src || !dst || !row_bytes || !zero_new || !code ||
      !densify_ws) {
    gsaj_set_error("gsaj_densify_rows: invalid argument (P=%d N=%d n_tensors=%d; P must be positive, N 1..%d, n_tensors 1..%d, no null pointer)",
                   P, N, n_tensors, GSAJ_DENSIFY_MAX_SPLIT, GSAJ_DENSIFY_MAX_TENSORS);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  RowTable tb;
  if (int rc = row_table_fill("gsaj_densify_rows", &tb, n_tensors, src, dst, row_bytes, zero_new)) return rc;
  hipLaunchKernelGGL(k_dn_rows, dim3((unsigned)row_blocks(P), (unsigned)n_tensors, (unsigned)(2 + N)), dim3(ROW_BLOCK), 0, (hipStream_t)stream,
                     P, N, tb, code, static_cast<const uint32_t *>(densify_ws));
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_densify_children(int P, int S, int N, const float *xyz, const float *scaling, const float *rotation, const float *noise,
                                     uint64_t seed, const uint8_t *code, const void *densify_ws, float *dst_xyz, float *dst_scaling,
                                     void *stream) {
  if (dn_bad_pn(P, N) || (S != 1 && S != 3) || !xyz || !scaling || !rotation || !code || !densify_ws || !dst_xyz || !dst_scaling ||
      dst_xyz == xyz || dst_scaling == scaling) {
    gsaj_set_error("gsaj_densify_children: invalid argument (P=%d S=%d N=%d; P must be positive, S 1 or 3, N 1..%d, no null pointer but noise, "
                   "destinations different from the sources)", P, S, N, GSAJ_DENSIFY_MAX_SPLIT);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(k_dn_children, dim3((unsigned)row_blocks(P), (unsigned)N), dim3(ROW_BLOCK), 0, (hipStream_t)stream, P, S, N,
                     (float)(0.8 * N), xyz, scaling, rotation, noise, (uint32_t)seed, (uint32_t)(seed >> 32), code,
                     static_cast<const uint32_t *>(densify_ws), dst_xyz, dst_scaling);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_densify_noise(int P, int N, uint64_t seed, float *out, void *stream) {
  if (dn_bad_pn(P, N) || !out) {
    gsaj_set_error("gsaj_densify_noise: invalid argument (P=%d N=%d; P must be positive, N 1..%d, no null pointer)", P, N, GSAJ_DENSIFY_MAX_SPLIT);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipLaunchKernelGGL(k_dn_noise, dim3((unsigned)row_blocks(P), (unsigned)N), dim3(ROW_BLOCK), 0, (hipStream_t)stream, P, (uint32_t)seed,
                     (uint32_t)(seed >> 32), out);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
