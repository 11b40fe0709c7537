// compact.hip -- removing rows of the Gaussian map under a mask: gsaj_compact_plan, gsaj_compact_count, gsaj_compact_rows
// (include/gsaj.h states the semantics).  What the reference does with one boolean index per tensor -- six parameters, their twelve
// Adam moments and the bookkeeping vectors, gaussian_splatting/scene/gaussian_model.py:559-597, each t[mask] a nonzero with a host
// read and a gather -- is one pass over the mask (block counts -> exclusive block offsets) and one launch that moves the kept rows
// of a whole table of tensors (the mover of row_move.h, which densify_prune.hip calls too).  Pure data movement: the result is
// t[keep] bit for bit, in the stable order, whatever the launch geometry; no atomics, no floating point.
#include "row_move.h"

#define CP_HDR 8  // words in front of the block offsets: [0] P' [1] P [2] mask_is_remove [4..5] the mask's address

__device__ __forceinline__ bool cp_keep(const uint8_t *mask, size_t i, size_t P, uint32_t rem) {
  return i < P && ((mask[i] != 0) != (rem != 0u));
}

// counts[b] = kept rows of block b; counts[nb] = 0, the slot the scan leaves P' in.  The header remembers what the rows step needs.
__global__ void __launch_bounds__(ROW_BLOCK) k_cp_count(int P, const uint8_t *__restrict__ mask, int rem, uint32_t *__restrict__ ws) {
  __shared__ uint32_t wcnt[ROW_BLOCK / GSAJ_WAVE];
  const size_t i = (size_t)blockIdx.x * ROW_BLOCK + threadIdx.x;
  row_post(cp_keep(mask, i, (size_t)P, (uint32_t)rem), wcnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t *counts = gsaj_shift(ws, sizeof(uint32_t) * CP_HDR);
    counts[blockIdx.x] = row_total(wcnt);
    if (blockIdx.x == 0) {
      counts[gridDim.x] = 0u;
      const unsigned long long a = (unsigned long long)mask;
      ws[1] = (uint32_t)P; ws[2] = (uint32_t)rem; ws[3] = 0u; ws[4] = (uint32_t)a; ws[5] = (uint32_t)(a >> 32);
    }
  }
}

// the small second kernel: P' from the scan's last slot to the fixed place gsaj_compact_count reads
__global__ void __launch_bounds__(GSAJ_WAVE) k_cp_total(uint32_t nb, uint32_t *__restrict__ ws) {
  if (threadIdx.x == 0) ws[0] = gsaj_shift(ws, sizeof(uint32_t) * CP_HDR)[nb];
}

// Workgroup (b, t) writes rows [offs[b], offs[b + 1]) of tensor t: the kept rows of source block b, in order.
__global__ void __launch_bounds__(ROW_BLOCK) k_cp_rows(int P, RowTable tb, const uint32_t *__restrict__ ws) {
  if (ws[1] != (uint32_t)P) return;  // not the plan of these tensors: nothing is read or written
  const uint32_t *offs = gsaj_shift(ws, sizeof(uint32_t) * CP_HDR);
  const uint32_t off = offs[blockIdx.x], count = offs[blockIdx.x + 1] - off;
  const uint32_t w = tb.w[blockIdx.y];
  const size_t row0 = (size_t)blockIdx.x * ROW_BLOCK;
  const row_src32 s32 = (row_src32)((unsigned long long)tb.src[blockIdx.y]) + row0 * w;
  const row_dst32 d32 = (row_dst32)((unsigned long long)tb.dst[blockIdx.y]) + (size_t)off * w;
  row_move_segment(s32, d32, w, tb.magic[blockIdx.y], count, [=](uint32_t r) {  // (the header has the mask's address and polarity)
    const row_bytes_t mask = (row_bytes_t)((unsigned long long)ws[4] | ((unsigned long long)ws[5] << 32));
    return row0 + r < (size_t)P && ((mask[row0 + r] != 0) != (ws[2] != 0u));
  });
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
extern "C" size_t gsaj_compact_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return gsaj_align(sizeof(uint32_t) * (CP_HDR + row_blocks(P) + 1));
}

extern "C" int gsaj_compact_plan(int P, const uint8_t *mask, int mask_is_remove, void *compact_ws, void *stream) {
  if (P <= 0 || !mask || !compact_ws) {
    gsaj_set_error("gsaj_compact_plan: invalid argument (P=%d; P must be positive, no null pointer)", P);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ws = static_cast<uint32_t *>(compact_ws);
  const size_t nb = row_blocks(P);
  hipLaunchKernelGGL(k_cp_count, dim3((unsigned)nb), dim3(ROW_BLOCK), 0, s, P, mask, mask_is_remove ? 1 : 0, ws);
  launch_exclusive_scan_u32((int)(nb + 1), ws + CP_HDR, s);  // (knn.hip: the one-workgroup scan seed.hip's compaction uses too)
  hipLaunchKernelGGL(k_cp_total, dim3(1), dim3(GSAJ_WAVE), 0, s, (uint32_t)nb, ws);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_compact_count(const void *compact_ws, void *stream, int *n_kept) {
  if (!compact_ws || !n_kept) {
    gsaj_set_error("gsaj_compact_count: invalid argument (no null pointer)");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  uint32_t host = 0u;
  GSAJ_HIP_CHECK(hipMemcpyAsync(&host, compact_ws, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *n_kept = (int)host;
  return GSAJ_OK;
}

extern "C" int gsaj_compact_rows(int P, int n_tensors, const void *const *src, void *const *dst, const int *row_bytes,
                                 const void *compact_ws, void *stream) {
  if (P <= 0 || n_tensors < 1 || n_tensors > GSAJ_COMPACT_MAX_TENSORS || !src || !dst || !row_bytes || !compact_ws) {
    gsaj_set_error("gsaj_compact_rows: invalid argument (P=%d n_tensors=%d; P must be positive, n_tensors 1..%d, no null pointer)", P,
                   n_tensors, GSAJ_COMPACT_MAX_TENSORS);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  RowTable tb;
  if (int rc = row_table_fill("gsaj_compact_rows", &tb, n_tensors, src, dst, row_bytes, nullptr)) return rc;
  hipLaunchKernelGGL(k_cp_rows, dim3((unsigned)row_blocks(P), (unsigned)n_tensors), dim3(ROW_BLOCK), 0, (hipStream_t)stream, P, tb,
                     static_cast<const uint32_t *>(compact_ws));
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
