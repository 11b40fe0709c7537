// knn.hip -- distCUDA2: mean squared distance of every point to its 3 nearest neighbours (gfx950).  SURVEY 8(f)-3.
//
// Semantics: reference submodules/simple-knn/simple_knn.cu:45-220 (SimpleKNN::knn) behind simple_knn._C.distCUDA2
// (spatial.cu): Morton-order the points (10 bits per axis over the bounding box that -- reference quirk, cub init
// {0,0,0} -- also contains the origin), cut the sorted sequence into boxes, and for every point scan the boxes that can
// hold one of its 3 nearest neighbours (bound: the 3rd best among its 3 Morton neighbours on either side).  The search
// is exact, so the result is the 3-NN mean squared distance whatever the box size; points without 3 neighbours keep
// FLT_MAX terms (-> inf), as in the reference.
//
// MI355X design: no host round trips (the reference copies the bounding box to the host twice); one workspace;
// points gathered into Morton order once so the scans are contiguous; 256-point boxes; a wave (64 consecutive Morton
// points = spatial neighbours) scans the UNION of the boxes its lanes accept, so a box's points are fetched once per
// wave through LDS and every lane tests them (a superset of candidates keeps the result exact).
#include "gsaj_common.h"
#include "last_block.h"
#include "wave_reduce.h"
#include <cfloat>
#include <cstring>

#define KNN_BOX 256
#define RS_TILE 2048   // keys per workgroup of the radix passes (one wave64: a tile is walked in list order, 64 keys at a time)
#define RS_BITS 8
#define RS_BUCKETS (1 << RS_BITS)

struct KnnWS {
  float *bbox;         // [6] min xyz, max xyz
  uint32_t *ticket;    // [1]
  float *bpart;        // [nblk][6]
  uint32_t *codes, *codes_sorted, *idx, *idx_sorted;
  float4 *sorted;      // [P] points in Morton order (w unused)
  float *boxes;        // [nbox][6]
  uint32_t *hist;      // [RS_BUCKETS][ntile] digit counts of the radix pass under way, bucket-major; exclusive offsets after the scan
};

static size_t knn_carve(Carver c, int P, KnnWS *w) {
  const size_t Pz = (size_t)P, nblk = (Pz + 255) / 256, nbox = (Pz + KNN_BOX - 1) / KNN_BOX;
  w->bbox = c.take<float>(6);
  w->ticket = c.take<uint32_t>(1);
  w->bpart = c.take<float>(nblk * 6);
  w->codes = c.take<uint32_t>(Pz);
  w->codes_sorted = c.take<uint32_t>(Pz);
  w->idx = c.take<uint32_t>(Pz);
  w->idx_sorted = c.take<uint32_t>(Pz);
  w->sorted = c.take<float4>(Pz);
  w->boxes = c.take<float>(nbox * 6);
  w->hist = c.take<uint32_t>((size_t)RS_BUCKETS * ((Pz + RS_TILE - 1) / RS_TILE));
  return c.used();
}

// A box {min xyz, max xyz} of a workgroup through the ordered fold of wave_reduce.h: three minima and three maxima put into the six
// rows of red, the caller's ONE barrier, then component c folded over the waves in order.
template <int NWAVES>
__device__ __forceinline__ void knn_box_put(float *v, float (*red)[NWAVES]) {
  block_fold_put<NWAVES, 3>(v, red, lane_min());
  block_fold_put<NWAVES, 3>(v + 3, red + 3, lane_max());
}
template <int NWAVES>
__device__ __forceinline__ float knn_box_get(const float (*red)[NWAVES], int c) {
  return c < 3 ? block_fold_get<NWAVES>(red[c], lane_min()) : block_fold_get<NWAVES>(red[c], lane_max());
}

// bounding box incl. the origin (simple_knn.cu:194-203: Reduce with init {0,0,0}); last workgroup combines the partials
__global__ __launch_bounds__(256) void k_knn_bbox(int P, const float *__restrict__ pts, KnnWS w) {
  __shared__ float red[6][4];
  __shared__ bool is_last;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < P) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    v[0] = fminf(0.f, x); v[1] = fminf(0.f, y); v[2] = fminf(0.f, z);
    v[3] = fmaxf(0.f, x); v[4] = fmaxf(0.f, y); v[5] = fmaxf(0.f, z);
  }
  knn_box_put<4>(v, red);
  __syncthreads();
  if (threadIdx.x == 0) {  // the workgroup's box, handed to the last workgroup (last_block.h)
#pragma unroll
    for (int c = 0; c < 6; c++) lb_publish(&w.bpart[(size_t)blockIdx.x * 6 + c], knn_box_get<4>(red, c));
  }
  if (!lb_arrive(w.ticket, &is_last)) return;
  float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (unsigned b = threadIdx.x; b < gridDim.x; b += 256)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const float t = lb_load(&w.bpart[(size_t)b * 6 + c]);
      a[c] = c < 3 ? fminf(a[c], t) : fmaxf(a[c], t);
    }
  __syncthreads();  // (red is written again)
  knn_box_put<4>(a, red);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 6; c++) w.bbox[c] = knn_box_get<4>(red, c);
    lb_reset(w.ticket);
  }
}

__device__ __forceinline__ uint32_t prep_morton(uint32_t x) {  // spread 10 bits to every third position (simple_knn.cu:45-52)
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

__global__ __launch_bounds__(256) void k_knn_morton(int P, const float *__restrict__ pts, KnnWS w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float mnx = w.bbox[0], mny = w.bbox[1], mnz = w.bbox[2], mxx = w.bbox[3], mxy = w.bbox[4], mxz = w.bbox[5];
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  const uint32_t cx = prep_morton((uint32_t)(((x - mnx) / (mxx - mnx)) * 1023.f));
  const uint32_t cy = prep_morton((uint32_t)(((y - mny) / (mxy - mny)) * 1023.f));
  const uint32_t cz = prep_morton((uint32_t)(((z - mnz) / (mxz - mnz)) * 1023.f));
  w.codes[i] = cx | (cy << 1) | (cz << 2);
  w.idx[i] = (uint32_t)i;
}

// ---- the Morton sort: least-significant-digit radix sort of (code, index) pairs, 8 bits per pass (thrust::sort_by_key in the
// reference, simple_knn.cu:211; a library radix sort up to round 2).  Three kernels per pass: per-tile digit counts, one
// exclusive scan over (bucket, tile) -- bucket-major, so a key's offset is "keys of smaller digits anywhere + keys of its digit in
// earlier tiles" --, and a scatter in which ONE wave walks its tile in list order, 64 keys at a time: the lanes holding the
// same digit find each other with eight ballots, rank = the tile's running count of the digit + the peers on lower lanes.  Every
// pass is therefore STABLE (ties keep their order, as a radix sort's must for the next digit to be meaningful), and the result
// is the one any stable sort by code gives.  Map initialisation / densification path: throughput is not the point (10^6 points:
// 4 passes x 3 short launches), having no library in the rasteriser's shared object is.
__device__ __forceinline__ unsigned long long rs_peers(uint32_t digit, bool valid) {
  unsigned long long m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
  for (int b = 0; b < RS_BITS; b++) {
    const unsigned long long bal = __builtin_amdgcn_ballot_w64((digit >> b) & 1u);
    m &= ((digit >> b) & 1u) ? bal : ~bal;
  }
  return m;
}

__global__ __launch_bounds__(64) void k_rs_hist(int P, int ntile, int shift, const uint32_t *__restrict__ keys, uint32_t *__restrict__ hist) {
  __shared__ uint32_t cnt[RS_BUCKETS];
  const int lane = threadIdx.x, tile = blockIdx.x;
  for (int d = lane; d < RS_BUCKETS; d += 64) cnt[d] = 0u;
  __syncthreads();
  const int beg = tile * RS_TILE, end = min(P, beg + RS_TILE);
  for (int i = beg + lane; i < end; i += 64) atomicAdd(&cnt[(keys[i] >> shift) & (RS_BUCKETS - 1)], 1u);
  __syncthreads();
  for (int d = lane; d < RS_BUCKETS; d += 64) hist[(size_t)d * ntile + tile] = cnt[d];
}

__global__ __launch_bounds__(1024) void k_rs_scan(int n, uint32_t *__restrict__ hist) {  // exclusive scan, one workgroup
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0u;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const uint32_t v = i < n ? hist[i] : 0u;
    const uint32_t excl = block_excl_scan_add<16>(v, wsum) + carry;  // (carry: read behind the scan's barrier)
    if (i < n) hist[i] = excl;
    __syncthreads();
    if (tid == 1023) carry = excl + v;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_rs_scatter(int P, int ntile, int shift, const uint32_t *__restrict__ keys,
                                                   const uint32_t *__restrict__ vals, uint32_t *__restrict__ keys_out,
                                                   uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ hist) {
  __shared__ uint32_t run[RS_BUCKETS];  // where the tile's next key of each digit goes
  const int lane = threadIdx.x, tile = blockIdx.x;
  for (int d = lane; d < RS_BUCKETS; d += 64) run[d] = hist[(size_t)d * ntile + tile];
  __syncthreads();
  const int beg = tile * RS_TILE, end = min(P, beg + RS_TILE);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i0 = beg; i0 < end; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < end;
    const uint32_t k = valid ? keys[i] : 0u, v = valid ? vals[i] : 0u;
    const uint32_t d = (k >> shift) & (RS_BUCKETS - 1);
    const unsigned long long peers = rs_peers(d, valid);
    if (valid) {
      const uint32_t dst = run[d] + (uint32_t)__popcll(peers & below);
      keys_out[dst] = k;
      vals_out[dst] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers & below) == 0ull) run[d] += (uint32_t)__popcll(peers);  // the digit's lowest lane
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

void launch_exclusive_scan_u32(int n, uint32_t *v, hipStream_t s) { hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, n, v); }

// Sorts the (codes, idx) pairs; the passes alternate between the two pairs of arrays, and w.codes_sorted / w.idx_sorted are
// pointed at whichever pair holds the result.
static int knn_radix_sort(int P, KnnWS &w, hipStream_t s) {
  const int ntile = (P + RS_TILE - 1) / RS_TILE;
  uint32_t *ka = w.codes, *va = w.idx, *kb = w.codes_sorted, *vb = w.idx_sorted;
  for (int shift = 0; shift < 30; shift += RS_BITS) {
    hipLaunchKernelGGL(k_rs_hist, dim3(ntile), dim3(64), 0, s, P, ntile, shift, ka, w.hist);
    launch_exclusive_scan_u32(RS_BUCKETS * ntile, w.hist, s);
    hipLaunchKernelGGL(k_rs_scatter, dim3(ntile), dim3(64), 0, s, P, ntile, shift, ka, va, kb, vb, w.hist);
    uint32_t *t = ka; ka = kb; kb = t;
    t = va; va = vb; vb = t;
  }
  w.codes_sorted = ka;  // (an even number of passes: the result is back in the first pair of arrays)
  w.idx_sorted = va;
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// gather into Morton order + per-box bounds (simple_knn.cu:76-117, 256-point boxes)
__global__ __launch_bounds__(KNN_BOX) void k_knn_boxes(int P, const float *__restrict__ pts, KnnWS w) {
  __shared__ float red[6][KNN_BOX / 64];
  const int i = blockIdx.x * KNN_BOX + threadIdx.x;
  float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  if (i < P) {
    const size_t src = w.idx_sorted[i];
    const float x = pts[3 * src], y = pts[3 * src + 1], z = pts[3 * src + 2];
    w.sorted[i] = make_float4(x, y, z, 0.f);
    v[0] = x; v[1] = y; v[2] = z; v[3] = x; v[4] = y; v[5] = z;
  }
  knn_box_put<KNN_BOX / 64>(v, red);
  __syncthreads();
  if (threadIdx.x < 6) w.boxes[(size_t)blockIdx.x * 6 + threadIdx.x] = knn_box_get<KNN_BOX / 64>(red, (int)threadIdx.x);
}

__device__ __forceinline__ void k_best3(float d, float &b0, float &b1, float &b2) {  // simple_knn.cu:134-147
  if (b0 > d) { const float t = b0; b0 = d; d = t; }
  if (b1 > d) { const float t = b1; b1 = d; d = t; }
  if (b2 > d) { b2 = d; }
}

__global__ __launch_bounds__(64) void k_knn_mean_dist(int P, KnnWS w, float *__restrict__ out) {
  __shared__ float4 stage[KNN_BOX];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < P;
  const float4 me = live ? w.sorted[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
  if (live) {
    for (int j = max(0, i - 3); j <= min(P - 1, i + 3); j++) {
      if (j == i) continue;
      const float4 q = w.sorted[j];
      const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
      k_best3(dx * dx + dy * dy + dz * dz, b0, b1, b2);
    }
  }
  // an upper bound of the true 3rd-nearest distance (simple_knn.cu:165) -- with head room for rounding: the best three are
  // found AGAIN below, and the neighbour that defines the bound may be a box of its own (the last, partial box: one point),
  // whose box distance IS this bound up to the contraction of the two sums of squares; one ulp above it the box was skipped
  // and the neighbour lost (tools/fuzz_knn.py, 2049 points)
  const float reject = b2 * 1.000002f;
  b0 = FLT_MAX; b1 = FLT_MAX; b2 = FLT_MAX;
  const int nbox = (P + KNN_BOX - 1) / KNN_BOX;
  for (int b = 0; b < nbox; b++) {
    const float *bx = w.boxes + (size_t)b * 6;
    float ddx = 0.f, ddy = 0.f, ddz = 0.f;  // distBoxPoint, simple_knn.cu:119-130
    if (me.x < bx[0] || me.x > bx[3]) ddx = fminf(fabsf(me.x - bx[0]), fabsf(me.x - bx[3]));
    if (me.y < bx[1] || me.y > bx[4]) ddy = fminf(fabsf(me.y - bx[1]), fabsf(me.y - bx[4]));
    if (me.z < bx[2] || me.z > bx[5]) ddz = fminf(fabsf(me.z - bx[2]), fabsf(me.z - bx[5]));
    const float dist = ddx * ddx + ddy * ddy + ddz * ddz;
    const bool want = live && !(dist > reject || dist > b2);
    if (__builtin_amdgcn_ballot_w64(want) == 0ull) continue;  // wave-uniform: scan the union of the lanes' boxes
    const int base = b * KNN_BOX, cnt = min(KNN_BOX, P - base);
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < cnt; t += 64) stage[t] = w.sorted[base + t];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int t = 0; t < cnt; t++) {
      const float4 q = stage[t];
      const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
      const float d = dx * dx + dy * dy + dz * dz;
      if (base + t != i) k_best3(d, b0, b1, b2);
    }
  }
  if (live) out[w.idx_sorted[i]] = (b0 + b1 + b2) / 3.0f;
}

extern "C" size_t gsaj_dist2_workspace_bytes(int P) {
  if (P <= 0) return 512;
  KnnWS w;
  return knn_carve(Carver(nullptr, ALIGN_BASE), P, &w) + 256;
}

extern "C" int gsaj_dist2(int P, const float *points, float *mean_dists, void *knn_ws, void *stream) {
  if (P < 0 || (P > 0 && (!points || !mean_dists || !knn_ws))) {
    gsaj_set_error("gsaj_dist2: invalid argument (P=%d)", P);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (P == 0) return GSAJ_OK;
  hipStream_t s = (hipStream_t)stream;
  KnnWS w;
  knn_carve(Carver(knn_ws, ALIGN_BASE), P, &w);
  GSAJ_HIP_CHECK(hipMemsetAsync(w.ticket, 0, sizeof(uint32_t), s));
  const unsigned nblk = (unsigned)((P + 255) / 256), nbox = (unsigned)((P + KNN_BOX - 1) / KNN_BOX);
  hipLaunchKernelGGL(k_knn_bbox, dim3(nblk), dim3(256), 0, s, P, points, w);
  hipLaunchKernelGGL(k_knn_morton, dim3(nblk), dim3(256), 0, s, P, points, w);
  {
    const int rc = knn_radix_sort(P, w, s);
    if (rc != GSAJ_OK) return rc;
  }
  hipLaunchKernelGGL(k_knn_boxes, dim3(nbox), dim3(KNN_BOX), 0, s, P, points, w);
  hipLaunchKernelGGL(k_knn_mean_dist, dim3((P + 63) / 64), dim3(64), 0, s, P, w, mean_dists);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

extern "C" int gsaj_debug_dist2_order(int P, void *knn_ws, uint32_t *codes_sorted, uint32_t *idx_sorted, void *stream) {
  if (P <= 0 || !knn_ws || !codes_sorted || !idx_sorted) {
    gsaj_set_error("gsaj_debug_dist2_order: invalid argument (P=%d)", P);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  KnnWS w;
  knn_carve(Carver(knn_ws, ALIGN_BASE), P, &w);
  // (where knn_radix_sort leaves the result: passes alternate between the two pairs of arrays)
  int passes = 0;
  for (int shift = 0; shift < 30; shift += RS_BITS) passes++;
  const uint32_t *k = (passes & 1) ? w.codes_sorted : w.codes, *v = (passes & 1) ? w.idx_sorted : w.idx;
  GSAJ_HIP_CHECK(hipMemcpyAsync(codes_sorted, k, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
  GSAJ_HIP_CHECK(hipMemcpyAsync(idx_sorted, v, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
  GSAJ_HIP_CHECK(hipStreamSynchronize(s));
  return GSAJ_OK;
}
