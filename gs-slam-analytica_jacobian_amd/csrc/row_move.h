// row_move.h -- the one row mover of compact.hip (prune) and densify_prune.hip (clone / split / prune): a table of up to 32 tensors
// whose selected rows go, block of 256 source rows by block, into contiguous destination segments.  Both files count the selected
// rows of a block with ballots, scan the counts into segment offsets and then call row_move_segment once per (block, tensor
// [, segment]).  Integers and data movement only: the result is the selected rows bit for bit, in source order, whatever the launch
// geometry and whatever FMA contraction the including file is built with.
#pragma once
#include "gsaj_common.h"

#define ROW_BLOCK 256       // rows per workgroup, one lane per row: the unit of the block counts and of a destination segment
#define ROW_UNROLL 8        // dwords a lane has in flight in the copy and gather loops (all loads of a pass are issued before the first store)
#define ROW_SHIFT 30        // row = (j * ceil(2^30 / w)) >> 30 is exact for j < 2^18 (256 rows of at most 1024 dwords), w <= 1024:
                            // the error term j * (m w - 2^30) stays below 2^18 * 2^10 < 2^30
#define ROW_MAX_TENSORS 32  // entries of a table, passed to the kernel by value
#define ROW_MAX_BYTES 4096  // largest row

static_assert(GSAJ_COMPACT_MAX_TENSORS == ROW_MAX_TENSORS && GSAJ_DENSIFY_MAX_TENSORS == ROW_MAX_TENSORS,
              "include/gsaj.h promises tables of the mover's size");

struct RowTable {
  const void *src[ROW_MAX_TENSORS];
  void *dst[ROW_MAX_TENSORS];
  uint32_t w[ROW_MAX_TENSORS];      // row size in dwords
  uint32_t magic[ROW_MAX_TENSORS];  // ceil(2^30 / w)
  uint32_t zero_new;                // bit t: new rows (clones, children) of tensor t are zeros, not the parent's row (densify only)
};

typedef const __attribute__((address_space(1))) uint32_t *row_src32;
typedef __attribute__((address_space(1))) uint32_t *row_dst32;
typedef uint32_t row_u4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) row_u4 *row_src128;
typedef __attribute__((address_space(1))) row_u4 *row_dst128;
typedef const __attribute__((address_space(1))) uint8_t *row_bytes_t;  // a mask or a code byte per source row

static inline size_t row_blocks(int P) { return ((size_t)P + ROW_BLOCK - 1) / ROW_BLOCK; }

// Checks and fills a table; `who` is the entry point the messages name.  zero_new == NULL: no tensor has zero rows.
static inline int row_table_fill(const char *who, RowTable *tb, int n_tensors, const void *const *src, void *const *dst,
                                 const int *row_bytes, const int *zero_new) {
  *tb = RowTable{};
  for (int t = 0; t < n_tensors; ++t) {
    if (!src[t] || !dst[t] || src[t] == dst[t]) {
      gsaj_set_error("%s: tensor %d: src and dst must be two different non-null pointers (no in-place form)", who, t);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if (row_bytes[t] <= 0 || row_bytes[t] % 4 != 0 || row_bytes[t] > ROW_MAX_BYTES) {
      gsaj_set_error("%s: tensor %d: row size %d is not a positive multiple of 4 bytes of at most %d", who, t, row_bytes[t], ROW_MAX_BYTES);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    tb->src[t] = src[t];
    tb->dst[t] = dst[t];
    tb->w[t] = (uint32_t)row_bytes[t] / 4u;
    tb->magic[t] = (uint32_t)(((1ull << ROW_SHIFT) + tb->w[t] - 1u) / tb->w[t]);
    if (zero_new && zero_new[t]) tb->zero_new |= 1u << t;
  }
  return GSAJ_OK;
}

// The workgroup's lanes with `has` set, through four wave counts in LDS (every lane must call): row_post leaves each wave's count
// in wcnt and returns the wave's ballot; after a barrier row_total is the block count and row_rank the lane's rank among them.
__device__ __forceinline__ unsigned long long row_post(bool has, uint32_t *wcnt) {
  const unsigned long long set = __ballot(has);
  if ((threadIdx.x & (GSAJ_WAVE - 1)) == 0) wcnt[threadIdx.x / GSAJ_WAVE] = (uint32_t)__popcll(set);
  return set;
}
__device__ __forceinline__ uint32_t row_total(const uint32_t *wcnt) { return wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]; }
__device__ __forceinline__ uint32_t row_rank(bool has, uint32_t *wcnt) {
  const unsigned long long set = row_post(has, wcnt);
  const int lane = threadIdx.x & (GSAJ_WAVE - 1), wave = threadIdx.x / GSAJ_WAVE;
  __syncthreads();
  uint32_t before = 0u;
  for (int k = 0; k < wave; ++k) before += wcnt[k];
  return before + (uint32_t)__popcll(set & ((1ull << lane) - 1ull));
}

// The rows a block sends to a segment: the difference of two neighbouring offsets.  0: nothing to do; more than a block has: the
// offsets are not this plan's, and nothing may be indexed or written with them.
__device__ __forceinline__ bool row_count_ok(uint32_t count) { return count != 0u && count <= ROW_BLOCK; }

// One workgroup writes one destination segment of one tensor: the `count` rows of w dwords that its block of ROW_BLOCK source
// rows (s32: the block's first row) emits, in order, to d32.  emit(r): local row r is one of them -- asked only where the block
// is partial, so whatever it reads (a mask, a code byte) is not touched on the straight-copy path.  A count that is not row_count_ok
// moves nothing, which keeps every index inside list[].
template <typename Emit>
__device__ __forceinline__ void row_move_segment(row_src32 s32, row_dst32 d32, uint32_t w, uint32_t magic, uint32_t count, Emit emit) {
  __shared__ uint8_t list[ROW_BLOCK];  // the emitted local rows, ascending
  __shared__ uint32_t wcnt[ROW_BLOCK / GSAJ_WAVE];
  if (!row_count_ok(count)) return;
  const uint32_t n = count * w;  // dwords of the segment, at most 2^18

  if (count == ROW_BLOCK) {  // every row of the block is emitted: a straight copy, 16 bytes per lane where both addresses allow
    if ((((unsigned long long)s32 | (unsigned long long)d32) & 15ull) == 0ull) {
      const row_src128 s128 = (row_src128)s32;
      const row_dst128 d128 = (row_dst128)d32;
      const uint32_t n4 = n / 4u;  // (256 w dwords: a multiple of 4)
      for (uint32_t j0 = threadIdx.x; j0 < n4; j0 += ROW_BLOCK * 4) {
        row_u4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = j0 + u * ROW_BLOCK < n4 ? s128[j0 + u * ROW_BLOCK] : row_u4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u * ROW_BLOCK < n4) d128[j0 + u * ROW_BLOCK] = v[u];
      }
    } else {
      for (uint32_t j0 = threadIdx.x; j0 < n; j0 += ROW_BLOCK * ROW_UNROLL) {
        uint32_t v[ROW_UNROLL];
#pragma unroll
        for (int u = 0; u < ROW_UNROLL; ++u) v[u] = j0 + u * ROW_BLOCK < n ? s32[j0 + u * ROW_BLOCK] : 0u;
#pragma unroll
        for (int u = 0; u < ROW_UNROLL; ++u)
          if (j0 + u * ROW_BLOCK < n) d32[j0 + u * ROW_BLOCK] = v[u];
      }
    }
    return;
  }

  // the list of emitted rows: ballot, position among the wave's emitting lanes, prefix over the four waves
  const bool has = emit((uint32_t)threadIdx.x);
  list[threadIdx.x] = 0;  // (a mask or codes changed since the plan leave slots unwritten: they name the block's first row, which exists)
  const uint32_t rank = row_rank(has, wcnt);  // (the barrier inside orders the line above before the writes below)
  if (has) list[rank] = (uint8_t)threadIdx.x;
  __syncthreads();

  // consecutive lanes write consecutive dwords of the segment; dword j is column j % w of the (j / w)-th emitted row
  for (uint32_t j0 = threadIdx.x; j0 < n; j0 += ROW_BLOCK * ROW_UNROLL) {
    uint32_t v[ROW_UNROLL];
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u) {
      const uint32_t j = j0 + u * ROW_BLOCK;
      v[u] = 0u;
      if (j < n) {
        const uint32_t r = (uint32_t)(((unsigned long long)j * magic) >> ROW_SHIFT);
        v[u] = s32[(uint32_t)list[r] * w + (j - r * w)];
      }
    }
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u)
      if (j0 + u * ROW_BLOCK < n) d32[j0 + u * ROW_BLOCK] = v[u];
  }
}
