// covis.hip -- covisibility of the keyframe window as one bit per (Gaussian, window slot): gsaj_covis_pack, gsaj_covis_query,
// gsaj_covis_prune_mask (include/gsaj.h states the semantics).  What the reference keeps as a dict of int64 [P] vectors
// (occ_aware_visibility, utils/slam_backend.py:236-240) and consults with logical_and / logical_or / count_nonzero per keyframe
// (utils/slam_frontend.py:218-224, 239-246, 422-428; n_obs: utils/slam_backend.py:248-263) is one uint32 word per Gaussian here.
// Everything is an integer: results are exact and do not depend on the launch geometry.
#include "gsaj_common.h"

#define CV_THREADS 256   // pack / prune mask: one lane per Gaussian, grid-stride
#define CV_MAX_BLOCKS 2048
#ifndef CQ_THREADS
#define CQ_THREADS 512   // query: 8 waves per workgroup, each lane CQ_UNROLL Gaussians per pass (loads issued before any is used)
#endif
#ifndef CQ_UNROLL
#define CQ_UNROLL 4
#endif
#ifndef CQ_MAX_BLOCKS
#define CQ_MAX_BLOCKS 256  // one workgroup per CU: every workgroup ends with one atomic per live output word on the same 260 bytes, and
                           // the kernel's time grew with their number (P = 10^6, K = 8, kernel trace on an MI355X: 7.6 / 8.9 us
                           // with 256 / 489 workgroups of 512 threads, 14 / 24 us with 977 / 1954 of 256), so few, fat ones
#endif
#define CQ_OUT (2 * GSAJ_COVIS_MAX_SLOTS + 1)

struct CovisSlots {
  uint8_t s[GSAJ_COVIS_MAX_SLOTS];
};

static inline unsigned cv_grid(long long n, int per_block, int cap) {
  const long long b = (n + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// words[i] = (words[i] & keep) | bits of the K rows; keep = ~(clear_mask | the K slot bits).  keep == 0: the old word is not read.
__global__ void __launch_bounds__(CV_THREADS) k_covis_pack(int K, int P, const int *__restrict__ n_touched, CovisSlots slots,
                                                           uint32_t keep, uint32_t *__restrict__ words) {
  const size_t stride = (size_t)gridDim.x * CV_THREADS;
  for (size_t i = (size_t)blockIdx.x * CV_THREADS + threadIdx.x; i < (size_t)P; i += stride) {
    uint32_t w = keep ? (words[i] & keep) : 0u;
    for (int k = 0; k < K; ++k) w |= (uint32_t)(n_touched[(size_t)k * P + i] > 0) << slots.s[k];
    words[i] = w;
  }
}

// Lane s of every wave keeps the two counters of slot s.  Per pass a wave holds CQ_UNROLL x 64 Gaussians; for every live slot
// (a scalar loop over the set bits of slot_mask) the ballots of the slot bit give 64-bit masks, whose popcounts -- alone and ANDed
// with the ballot of the query predicate -- are wave-uniform (scalar ALU) and are added in the one lane that owns the slot.
__global__ void __launch_bounds__(CQ_THREADS) k_covis_query(int P, const uint32_t *__restrict__ words, const int *__restrict__ cur,
                                                            int query_slot, uint32_t slot_mask, int *__restrict__ out) {
  __shared__ int sh[CQ_OUT];
  const int lane = threadIdx.x & (GSAJ_WAVE - 1);
  int inter = 0, count = 0, nq = 0;  // inter / count: of slot `lane` (lanes 0..31); nq: the same in every lane
  if (threadIdx.x < CQ_OUT) sh[threadIdx.x] = 0;
  __syncthreads();

  const size_t chunk = (size_t)CQ_THREADS * CQ_UNROLL, stride = (size_t)gridDim.x * chunk;
  // (every lane of a workgroup makes the same number of passes: the ballots need whole waves; lanes past P carry zeros)
  for (size_t base = (size_t)blockIdx.x * chunk; base < (size_t)P; base += stride) {
    uint32_t w[CQ_UNROLL];
    int c[CQ_UNROLL];
#pragma unroll
    for (int u = 0; u < CQ_UNROLL; ++u) {  // all loads of the pass are issued before the first is used
      const size_t i = base + (size_t)u * CQ_THREADS + threadIdx.x;
      const bool in = i < (size_t)P;
      w[u] = in ? words[i] : 0u;
      c[u] = (in && cur) ? cur[i] : 0;
    }
    unsigned long long bq[CQ_UNROLL];
#pragma unroll
    for (int u = 0; u < CQ_UNROLL; ++u) {
      bq[u] = __ballot(cur ? c[u] > 0 : (bool)((w[u] >> query_slot) & 1u));
      nq += __popcll(bq[u]);
    }
    for (uint32_t m = slot_mask; m; m &= m - 1) {
      const int s = __ffs(m) - 1;
      int cs = 0, is = 0;
#pragma unroll
      for (int u = 0; u < CQ_UNROLL; ++u) {
        const unsigned long long bs = __ballot((w[u] >> s) & 1u);
        cs += __popcll(bs);
        is += __popcll(bs & bq[u]);
      }
      if (lane == s) {
        count += cs;
        inter += is;
      }
    }
  }

  if (lane < GSAJ_COVIS_MAX_SLOTS) {
    if (inter) atomicAdd(&sh[lane], inter);
    if (count) atomicAdd(&sh[GSAJ_COVIS_MAX_SLOTS + lane], count);
  }
  if (lane == 0 && nq) atomicAdd(&sh[2 * GSAJ_COVIS_MAX_SLOTS], nq);
  __syncthreads();
  if (threadIdx.x < CQ_OUT) {
    const int v = sh[threadIdx.x];
    if (v) atomicAdd(&out[threadIdx.x], v);  // (out was zeroed on the stream before this launch)
  }
}

__global__ void __launch_bounds__(CV_THREADS) k_covis_prune(int P, const uint32_t *__restrict__ words, uint32_t window_mask,
                                                            const int *__restrict__ kf_ids, int kf_id_min, int max_obs,
                                                            uint8_t *__restrict__ to_prune, int *__restrict__ n_obs,
                                                            int *__restrict__ n_pruned) {
  __shared__ int sh;
  if (threadIdx.x == 0) sh = 0;
  __syncthreads();
  int mine = 0;
  const size_t stride = (size_t)gridDim.x * CV_THREADS;
  for (size_t i = (size_t)blockIdx.x * CV_THREADS + threadIdx.x; i < (size_t)P; i += stride) {
    const int obs = __popc(words[i] & window_mask);
    const bool prune = obs <= max_obs && (!kf_ids || kf_ids[i] >= kf_id_min);
    to_prune[i] = prune ? 1 : 0;
    if (n_obs) n_obs[i] = obs;
    mine += prune ? 1 : 0;
  }
  if (mine) atomicAdd(&sh, mine);
  __syncthreads();
  if (threadIdx.x == 0 && sh) atomicAdd(n_pruned, sh);  // (zeroed on the stream before this launch)
}

extern "C" int gsaj_covis_pack(int K, int P, const int *n_touched, const int *slots, uint32_t clear_mask, uint32_t *words,
                               void *stream) {
  if (P <= 0 || K < 1 || K > GSAJ_COVIS_MAX_SLOTS || !n_touched || !slots || !words) {
    gsaj_set_error("gsaj_covis_pack: invalid argument (K=%d P=%d; K must be 1..%d, P positive, no null pointer)", K, P,
                   GSAJ_COVIS_MAX_SLOTS);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  CovisSlots cs = {};
  uint32_t bits = 0;
  for (int k = 0; k < K; ++k) {
    if (slots[k] < 0 || slots[k] >= GSAJ_COVIS_MAX_SLOTS || ((bits >> slots[k]) & 1u)) {
      gsaj_set_error("gsaj_covis_pack: slots[%d] = %d is outside 0..%d or repeated", k, slots[k], GSAJ_COVIS_MAX_SLOTS - 1);
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    bits |= 1u << slots[k];
    cs.s[k] = (uint8_t)slots[k];
  }
  hipLaunchKernelGGL(k_covis_pack, dim3(cv_grid(P, CV_THREADS, CV_MAX_BLOCKS)), dim3(CV_THREADS), 0, (hipStream_t)stream, K, P,
                     n_touched, cs, ~(clear_mask | bits), words);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_covis_query(int P, const uint32_t *words, const int *cur_n_touched, int query_slot, uint32_t slot_mask, int *out,
                                void *stream) {
  if (P <= 0 || !words || !out || (!cur_n_touched && (query_slot < 0 || query_slot >= GSAJ_COVIS_MAX_SLOTS))) {
    gsaj_set_error("gsaj_covis_query: invalid argument (P=%d query_slot=%d; P must be positive, the slot 0..%d when no "
                   "cur_n_touched is given, no null pointer)", P, query_slot, GSAJ_COVIS_MAX_SLOTS - 1);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  GSAJ_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(int) * CQ_OUT, s));
  hipLaunchKernelGGL(k_covis_query, dim3(cv_grid(P, CQ_THREADS * CQ_UNROLL, CQ_MAX_BLOCKS)), dim3(CQ_THREADS), 0, s, P, words,
                     cur_n_touched, cur_n_touched ? 0 : query_slot, slot_mask, out);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_covis_prune_mask(int P, const uint32_t *words, uint32_t window_mask, const int *unique_kfIDs, int kf_id_min,
                                     int max_obs, uint8_t *to_prune, int *n_obs, int *n_pruned, void *stream) {
  if (P <= 0 || !words || !to_prune || !n_pruned) {
    gsaj_set_error("gsaj_covis_prune_mask: invalid argument (P=%d; P must be positive, no null pointer)", P);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  GSAJ_HIP_CHECK(hipMemsetAsync(n_pruned, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_covis_prune, dim3(cv_grid(P, CV_THREADS, CV_MAX_BLOCKS)), dim3(CV_THREADS), 0, s, P, words, window_mask,
                     unique_kfIDs, kf_id_min, max_obs, to_prune, n_obs, n_pruned);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
