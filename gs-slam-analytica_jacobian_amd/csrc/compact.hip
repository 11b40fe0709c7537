// compact.hip -- removing rows of the Gaussian map under a mask: gsaj_compact_plan, gsaj_compact_count, gsaj_compact_rows
// (include/gsaj.h states the semantics).  What the reference does with one boolean index per tensor -- six parameters, their twelve
// Adam moments and the bookkeeping vectors, gaussian_splatting/scene/gaussian_model.py:559-597, each t[mask] a nonzero with a host
// read and a gather -- is one pass over the mask (block counts -> exclusive block offsets) and one launch that moves the kept rows
// of a whole table of tensors.  Pure data movement: the result is t[keep] bit for bit, in the stable order, whatever the launch
// geometry; no atomics, no floating point.
#include "gsaj_common.h"

#define CP_BLOCK 256   // rows per workgroup, one lane per row: the unit of the block counts and of a destination segment
#define CP_HDR 8       // words in front of the block offsets: [0] P' [1] P [2] mask_is_remove [4..5] the mask's address
#define CP_UNROLL 8    // dwords a lane has in flight in the gather loop (all loads of a pass are issued before the first store)
#define CP_SHIFT 30    // row = (j * ceil(2^30 / w)) >> 30 is exact for j < 2^18 (256 rows of at most 1024 dwords), w <= 1024:
                       // the error term j * (m w - 2^30) stays below 2^18 * 2^10 < 2^30

struct CompactTable {
  const void *src[GSAJ_COMPACT_MAX_TENSORS];
  void *dst[GSAJ_COMPACT_MAX_TENSORS];
  uint32_t w[GSAJ_COMPACT_MAX_TENSORS];      // row size in dwords
  uint32_t magic[GSAJ_COMPACT_MAX_TENSORS];  // ceil(2^30 / w)
};

typedef const __attribute__((address_space(1))) uint32_t *cp_src32;
typedef __attribute__((address_space(1))) uint32_t *cp_dst32;
typedef uint32_t cp_u4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) cp_u4 *cp_src128;
typedef __attribute__((address_space(1))) cp_u4 *cp_dst128;

static inline size_t cp_blocks(int P) { return ((size_t)P + CP_BLOCK - 1) / CP_BLOCK; }

__device__ __forceinline__ bool cp_keep(const uint8_t *mask, size_t i, size_t P, uint32_t rem) {
  return i < P && ((mask[i] != 0) != (rem != 0u));
}

// counts[b] = kept rows of block b; counts[nb] = 0, the slot the scan leaves P' in.  The header remembers what the rows step needs.
__global__ void __launch_bounds__(CP_BLOCK) k_cp_count(int P, const uint8_t *__restrict__ mask, int rem, uint32_t *__restrict__ ws) {
  __shared__ uint32_t wcnt[CP_BLOCK / GSAJ_WAVE];
  const size_t i = (size_t)blockIdx.x * CP_BLOCK + threadIdx.x;
  const unsigned long long kept = __ballot(cp_keep(mask, i, (size_t)P, (uint32_t)rem));
  if ((threadIdx.x & (GSAJ_WAVE - 1)) == 0) wcnt[threadIdx.x / GSAJ_WAVE] = (uint32_t)__popcll(kept);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t *counts = gsaj_shift(ws, sizeof(uint32_t) * CP_HDR);
    counts[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
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
__global__ void __launch_bounds__(CP_BLOCK) k_cp_rows(int P, CompactTable tb, const uint32_t *__restrict__ ws) {
  __shared__ uint8_t list[CP_BLOCK];  // the kept local rows, ascending
  __shared__ uint32_t wcnt[CP_BLOCK / GSAJ_WAVE];
  if (ws[1] != (uint32_t)P) return;  // not the plan of these tensors: nothing is read or written
  const uint32_t *offs = gsaj_shift(ws, sizeof(uint32_t) * CP_HDR);
  const uint32_t off = offs[blockIdx.x], count = offs[blockIdx.x + 1] - off;
  if (count == 0u) return;

  const uint32_t w = tb.w[blockIdx.y], magic = tb.magic[blockIdx.y];
  const size_t row0 = (size_t)blockIdx.x * CP_BLOCK;
  const cp_src32 s32 = (cp_src32)((unsigned long long)tb.src[blockIdx.y]) + row0 * w;
  const cp_dst32 d32 = (cp_dst32)((unsigned long long)tb.dst[blockIdx.y]) + (size_t)off * w;
  const uint32_t n = count * w;  // dwords of the segment, at most 2^18

  if (count == CP_BLOCK) {  // every row of the block is kept: a straight copy, 16 bytes per lane where both addresses allow
    if ((((unsigned long long)s32 | (unsigned long long)d32) & 15ull) == 0ull) {
      const cp_src128 s128 = (cp_src128)s32;
      const cp_dst128 d128 = (cp_dst128)d32;
      const uint32_t n4 = n / 4u;  // (256 w dwords: a multiple of 4)
      for (uint32_t j0 = threadIdx.x; j0 < n4; j0 += CP_BLOCK * 4) {
        cp_u4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = j0 + u * CP_BLOCK < n4 ? s128[j0 + u * CP_BLOCK] : cp_u4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u * CP_BLOCK < n4) d128[j0 + u * CP_BLOCK] = v[u];
      }
    } else {
      for (uint32_t j0 = threadIdx.x; j0 < n; j0 += CP_BLOCK * CP_UNROLL) {
        uint32_t v[CP_UNROLL];
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) v[u] = j0 + u * CP_BLOCK < n ? s32[j0 + u * CP_BLOCK] : 0u;
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u)
          if (j0 + u * CP_BLOCK < n) d32[j0 + u * CP_BLOCK] = v[u];
      }
    }
    return;
  }

  // the list of kept rows: ballot, position among the wave's kept lanes, prefix over the four waves
  const unsigned long long a = (unsigned long long)ws[4] | ((unsigned long long)ws[5] << 32);
  const __attribute__((address_space(1))) uint8_t *mask = (const __attribute__((address_space(1))) uint8_t *)a;
  const size_t i = row0 + threadIdx.x;
  const bool keep = i < (size_t)P && ((mask[i] != 0) != (ws[2] != 0u));
  const unsigned long long kept = __ballot(keep);
  const int lane = threadIdx.x & (GSAJ_WAVE - 1), wave = threadIdx.x / GSAJ_WAVE;
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(kept);
  list[threadIdx.x] = 0;  // (a mask changed since the plan leaves slots unwritten: they name the block's first row, which exists)
  __syncthreads();
  uint32_t before = 0u;
  for (int k = 0; k < wave; ++k) before += wcnt[k];
  if (keep) list[before + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull))] = (uint8_t)threadIdx.x;
  __syncthreads();

  // consecutive lanes write consecutive dwords of the segment; dword j is column j % w of the (j / w)-th kept row
  for (uint32_t j0 = threadIdx.x; j0 < n; j0 += CP_BLOCK * CP_UNROLL) {
    uint32_t v[CP_UNROLL];
#pragma unroll
    for (int u = 0; u < CP_UNROLL; ++u) {
      const uint32_t j = j0 + u * CP_BLOCK;
      v[u] = 0u;
      if (j < n) {
        const uint32_t r = (uint32_t)(((unsigned long long)j * magic) >> CP_SHIFT);
        v[u] = s32[(uint32_t)list[r] * w + (j - r * w)];
      }
    }
#pragma unroll
    for (int u = 0; u < CP_UNROLL; ++u)
      if (j0 + u * CP_BLOCK < n) d32[j0 + u * CP_BLOCK] = v[u];
  }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
extern "C" size_t gsaj_compact_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return gsaj_align(sizeof(uint32_t) * (CP_HDR + cp_blocks(P) + 1));
}

extern "C" int gsaj_compact_plan(int P, const uint8_t *mask, int mask_is_remove, void *compact_ws, void *stream) {
  if (P <= 0 || !mask || !compact_ws) {
    gsaj_set_error("gsaj_compact_plan: invalid argument (P=%d; P must be positive, no null pointer)", P);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ws = static_cast<uint32_t *>(compact_ws);
  const size_t nb = cp_blocks(P);
  hipLaunchKernelGGL(k_cp_count, dim3((unsigned)nb), dim3(CP_BLOCK), 0, s, P, mask, mask_is_remove ? 1 : 0, ws);
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
  CompactTable tb = {};
  for (int t = 0; t < n_tensors; ++t) {
    if (!src[t] || !dst[t] || src[t] == dst[t]) {
      gsaj_set_error("gsaj_compact_rows: tensor %d: src and dst must be two different non-null pointers (no in-place form)", t);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if (row_bytes[t] <= 0 || row_bytes[t] % 4 != 0 || row_bytes[t] > 4096) {
      gsaj_set_error("gsaj_compact_rows: tensor %d: row size %d is not a positive multiple of 4 bytes of at most 4096", t, row_bytes[t]);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    tb.src[t] = src[t];
    tb.dst[t] = dst[t];
    tb.w[t] = (uint32_t)row_bytes[t] / 4u;
    tb.magic[t] = (uint32_t)(((1ull << CP_SHIFT) + tb.w[t] - 1u) / tb.w[t]);
  }
  hipLaunchKernelGGL(k_cp_rows, dim3((unsigned)cp_blocks(P), (unsigned)n_tensors), dim3(CP_BLOCK), 0, (hipStream_t)stream, P, tb,
                     static_cast<const uint32_t *>(compact_ws));
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
