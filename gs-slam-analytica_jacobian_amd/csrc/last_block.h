// last_block.h -- the cross-workgroup hand-off "every workgroup leaves a partial, the last one to arrive folds them all", without
// fences: the only place where this library relies on memory ordering the compiler does not check.  Five kernels end with it:
// k_gaussian_bwd (dL/dtau), k_loss_seeds, k_isotropic, k_ssim_fwd and k_knn_bbox ("Cross-workgroup hand-off").
//
// The rule.  A workgroup writes its partials with lb_publish (write-through stores), then EVERY thread calls lb_arrive: thread 0
// drains its stores, draws a ticket from one word with a relaxed agent-scope add, and a barrier hands the answer to the others.
// The workgroup whose add returned gridDim.x - 1 is the last: it reads every workgroup's partials with the lb_load* functions and
// nothing else, folds them in a fixed order (so the result does not depend on who came last), writes the result and calls lb_reset.
//
// Why it holds.  It is the first row of the table "hand-offs measured with sc1 loads in place of the acquire" of
// MI355X_MICROARCH.md (visibility section): one lane of each storing workgroup signals, for all that workgroup's stores, with an
// agent-scope add to ONE unsharded counter, and the consumer is the workgroup told by the value its add returned.  Measured on
// gfx950, not an architectural guarantee, and only under that row's conditions -- break one and a partial is stale a few percent
// of the time, under uneven load only, with plausible numbers:
//   (1) every handed-off byte is stored sc1: lb_publish, 4 or 8 bytes, by the thread that will draw the ticket (a partial stored
//       by another wave would need that wave's own drain and a barrier in front of lb_arrive);
//   (2) the storing wave drains (s_waitcnt vmcnt(0)) before the ONE add: lb_arrive;
//   (3) the adding wave loads only after its add has returned, the other waves behind a barrier that wave joins: lb_arrive's
//       barrier, and the loads come after the call;
//   (4) every load of those bytes is an sc1 load: lb_load, lb_load_x4, lb_load_partials4 -- never a plain read of a partial.
//
// What the fenced form costs.  A __threadfence() in front of the ticket is a buffer_wbl2 of everything the kernel has dirtied, once
// per workgroup: k_loss_seeds' 5 MB of seed rows made it 78 us instead of 6, and k_gaussian_bwd would write back ~25 MB of
// per-Gaussian output each time.
//
// Why the loads are wide and few.  A coherent load costs ~100 ns and coherent loads do not overlap (tools/chain_trace.py: 6 dword
// loads per partial made the last workgroup's sum 20 us of the batched backward's 80; two dwordx4 loads: 8 us).  So a partial slot
// is read by as few and as wide loads as the ISA allows, strided over the whole workgroup.
//
// The ticket word.  One uint32_t per hand-off, on a line no partial shares, ZERO when the kernel starts: whoever owns the workspace
// zeroes it once (or per call), and lb_reset leaves it zero for the next launch on the same stream.  Two launches that share a
// ticket must not overlap.  A launch that does not run to the end (an aborted frame returns before drawing) draws no ticket at all.
//
// Not this: the s_waitcnt vmcnt(0) of preprocess.hip and render_bwd.hip and gsaj_load_u64_device order a workgroup's OWN stores.
//
// Like wave_reduce.h this header owns no LDS: the flag word is the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One partial value, write-through.
template <typename T>
__device__ __forceinline__ void lb_publish(T *slot, T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a partial is stored 4 or 8 bytes at a time");
  __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every thread of the workgroup calls it, after thread 0 has published.  True in the workgroup that arrived last.
__device__ __forceinline__ bool lb_arrive(uint32_t *ticket, bool *s_last) {
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  return *s_last;
}

// By one thread of the last workgroup, when the partials have been read.
__device__ __forceinline__ void lb_reset(uint32_t *ticket) { *ticket = 0u; }

// ---- the last workgroup's loads ----------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T lb_load(const T *slot) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4 or 8 bytes; wider: lb_load_x4");
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 16 bytes that bypass this CU's L1 and this XCD's L2 (sc0 sc1).  The wait is inside the statement: the compiler takes an asm's
// outputs for ready when the statement ends and may copy them at once.
__device__ __forceinline__ uint4 lb_load_x4(const void *src) {
  uint4 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(src) : "memory");
  return v;
}
// Four 32-byte slots (8 floats each) as one batch of eight such loads behind ONE wait, inside the statement for the same reason.
__device__ __forceinline__ void lb_load_partials4(const float *p0, const float *p1, const float *p2, const float *p3,
                                                  float4 (&lo)[4], float4 (&hi)[4]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc0 sc1\n\tglobal_load_dwordx4 %1, %8, off offset:16 sc0 sc1\n\t"
      "global_load_dwordx4 %2, %9, off sc0 sc1\n\tglobal_load_dwordx4 %3, %9, off offset:16 sc0 sc1\n\t"
      "global_load_dwordx4 %4, %10, off sc0 sc1\n\tglobal_load_dwordx4 %5, %10, off offset:16 sc0 sc1\n\t"
      "global_load_dwordx4 %6, %11, off sc0 sc1\n\tglobal_load_dwordx4 %7, %11, off offset:16 sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]), "=&v"(hi[2]), "=&v"(lo[3]), "=&v"(hi[3])
      : "v"(p0), "v"(p1), "v"(p2), "v"(p3)
      : "memory");
}
// One wave: the sum over the 8-float slots i = lane, lane + 64, ... < nblk of their first 6 components, in that order, in fp64.
__device__ __forceinline__ void lb_sum_partials(const float *partials, int nblk, int lane, double (&acc)[6]) {
  for (int i0 = lane; i0 < nblk; i0 += 4 * 64) {
    float4 lo[4], hi[4];
    const float *src[4];
#pragma unroll
    for (int u = 0; u < 4; u++) src[u] = partials + (size_t)min(i0 + u * 64, nblk - 1) * 8;  // unconditional loads, masked below
    lb_load_partials4(src[0], src[1], src[2], src[3], lo, hi);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const bool in = i0 + u * 64 < nblk;
      const float t6[6] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y};
#pragma unroll
      for (int k = 0; k < 6; k++) acc[k] += in ? (double)t6[k] : 0.0;
    }
  }
}
