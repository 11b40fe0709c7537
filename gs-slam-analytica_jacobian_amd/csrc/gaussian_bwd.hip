// gaussian_bwd.hip -- fused per-Gaussian backward (gfx950): instance-gradient gather,
// conic -> cov2D -> (cov3D, mean3D, tau), mean2D -> (mean3D, tau), depth -> (mean3D, tau),
// colour -> (SH, mean3D, tau), cov3D -> (scale, rotation), and the reduction of dL/dtau.
//
// The reference runs computeCov2DCUDA (backward.cu:150-422), preprocessCUDA (:494-624, with
// computeColorFromSH :21-145 and computeCov3D :426-489) as two kernels that `+=` into
// dL_dmean3D / dL_dtau through global memory, then torch.sum over [P,6]
// (diff_gaussian_rasterization/__init__.py:162).  Here one lane owns one Gaussian end to end:
// it first sums the partial gradients of its (tile, Gaussian) instances in emission order
// (deterministic -- replaces the float atomics of backward.cu:852-869), keeps every
// intermediate in registers, writes each output once, and the 6 pose components are reduced
// wave -> (last-arriving workgroup) fixed-order final pass.  HBM-bound streaming stage: one wave per
// workgroup (P/64 groups spread over the 256 CUs), the instance partials of a Gaussian are one
// contiguous run (emission-slot order), and the [64][M*3] SH blocks are staged through LDS so that the
// global loads / stores of dL_dsh are fully coalesced (padded LDS rows, conflict-free per-lane reads).
#include "gsaj_common.h"
#include "last_block.h"
#include "wave_reduce.h"
#define GSAJ_SH_LINKAGE_EXTERN  // the SH constants have external linkage here and are loaded from constant memory (gaussian_chain.h)
#include "gaussian_chain.h"
#include <type_traits>

// SHW = 3*M as a compile-time constant (0: runtime) -- the staging loops divide by it per element
GSAJ_TRACE_DEFINE(gbwd)

template <int SHW>
__global__ __launch_bounds__(GB_BLOCK) void k_gaussian_bwd(BwdParams p, GeomWS g, uint32_t *__restrict__ counters,
                                                           const float4 *__restrict__ inst_grad,
                                                           const uint8_t *__restrict__ reached) {
  extern __shared__ float sh_lds[];  // [GB_BLOCK][3M+1]: SH coefficients in, overwritten in place by dL/dSH (padded rows)
  __shared__ bool s_last;
  if (counters[4]) return;  // aborted async frame
  GSAJ_TRACE_BEGIN(gbwd)
#ifdef GSAJ_BLOCK_TRACE
  unsigned long long tr_[5] = {0, 0, 0, 0, 0}, tr_t = wall_clock64();
#define TRM(i) { const unsigned long long n_ = wall_clock64(); tr_[i] += n_ - tr_t; tr_t = n_; }
#else
#define TRM(i)
#endif
  const int tid = threadIdx.x;
  const int idx = blockIdx.x * GB_BLOCK + tid;
  const int shw = SHW > 0 ? SHW : 3 * p.M, shs_stride = shw + 1;
  float *sh_io = sh_lds;
  // ---- 0. every input of this Gaussian is requested up front (this stage is latency-bound: one wave
  //         per SIMD, so the loads must be in flight together, not one s_waitcnt apart) ----
  const int radius = idx < p.P ? p.radii[idx] : 0;
  const bool vis = radius > 0;
  const size_t ii = (size_t)(idx < p.P ? idx : 0);
  // emission slots: Gaussian idx owns rows [first, first + cnt) of inst_grad; consecutive Gaussians
  // own consecutive runs, so the rows of this wave's 64 Gaussians are ONE contiguous block
  const uint32_t cnt = idx < p.P ? g.tiles_touched[ii] : 0u;
  // (point_offsets counts inside the Gaussian's block of PRE_BLOCK; block_sums holds the blocks' exclusive offsets)
  const uint32_t endi = idx < p.P ? g.block_sums[ii / PRE_BLOCK] + g.point_offsets[ii] : 0u;
  const uint32_t first = endi - cnt;
  // The wave's rows [F, E) of inst_grad are gathered in trips of 256; the first trip's flag and row loads (two dependent
  // round trips) are issued NOW, so that they overlap the input loads and the SH staging below.
  const uint32_t F = (uint32_t)__shfl((int)first, 0);
  const uint32_t E = wave_max(endi);
  float4 a[4][3];
  auto load_trip = [&](uint32_t lo, uint32_t hi) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const uint32_t r = lo + (uint32_t)(w * GB_BLOCK + tid);
      a[w][0] = a[w][1] = a[w][2] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < hi && reached[r]) {  // rows the reverse compositor never wrote are zero by definition
        const float4 *src = inst_grad + (size_t)r * REC_F4;
        a[w][0] = src[0]; a[w][1] = src[1]; a[w][2] = src[2];
      }
    }
  };
  load_trip(F, min(F + 256u, E));
  const float3 mean = make_float3(p.means3D[3 * ii], p.means3D[3 * ii + 1], p.means3D[3 * ii + 2]);
  float c6[6];
#pragma unroll
  for (int k = 0; k < 6; k++) c6[k] = p.cov3Ds[6 * ii + k];
  float3 sc = make_float3(0.f, 0.f, 0.f);
  float4 q = make_float4(1.f, 0.f, 0.f, 0.f);
  if (p.scales) {
    sc = make_float3(p.scales[3 * ii], p.scales[3 * ii + 1], p.scales[3 * ii + 2]);
    q = reinterpret_cast<const float4 *>(p.rotations)[ii];
  }
  uint8_t cl[3] = {0, 0, 0};
  if (p.shs) {
    cl[0] = g.clamped[3 * ii]; cl[1] = g.clamped[3 * ii + 1]; cl[2] = g.clamped[3 * ii + 2];
    // coalesced load of this workgroup's contiguous [GB_BLOCK][M*3] SH block, 24 loads in flight per batch
    const size_t base = (size_t)blockIdx.x * GB_BLOCK * shw;
    const int count = min(GB_BLOCK, p.P - blockIdx.x * GB_BLOCK) * shw;
    for (int e0 = 0; e0 < count; e0 += 24 * GB_BLOCK) {
      float v[24];
#pragma unroll
      for (int b = 0; b < 24; b++) {
        const int e = e0 + b * GB_BLOCK + tid;
        v[b] = e < count ? p.shs[base + e] : 0.f;
      }
#pragma unroll
      for (int b = 0; b < 24; b++) {
        const int e = e0 + b * GB_BLOCK + tid;
        if (e < count) {
          const int gi = e / shw, k = e - gi * shw;
          sh_io[gi * shs_stride + k] = v[b];
        }
      }
    }
    __syncthreads();
  }
  TRM(0)
  float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // ---- 1. gather the instance partials.  Tiles-per-Gaussian is heavy-tailed (mean ~8, max > 100), so a
  //         per-lane loop over global memory makes the whole wave wait for its largest Gaussian.
  //         Instead the wave streams its contiguous block of rows through LDS with fully coalesced
  //         loads (256 rows = 12 KB per trip, 12 loads per lane in flight) and each lane then sums its
  //         own rows from LDS in emission order (bit-reproducible). ----
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0;
  {
    __shared__ float4 rows[256 * REC_F4];
    for (uint32_t lo = F; lo < E; lo += 256) {
      const uint32_t hi = min(lo + 256u, E);
      if (lo != F) load_trip(lo, hi);
#pragma unroll
      for (int w = 0; w < 4; w++) {
        rows[(w * GB_BLOCK + tid) * REC_F4 + 0] = a[w][0];
        rows[(w * GB_BLOCK + tid) * REC_F4 + 1] = a[w][1];
        rows[(w * GB_BLOCK + tid) * REC_F4 + 2] = a[w][2];
      }
      __syncthreads();
      const uint32_t ub = max(first, lo), ue = min(first + cnt, hi);
      for (uint32_t u = ub; u < ue; u++) {
        const float4 a0 = rows[(u - lo) * REC_F4 + 0], a1 = rows[(u - lo) * REC_F4 + 1], a2 = rows[(u - lo) * REC_F4 + 2];
        s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
        s1.x += a1.x; s1.y += a1.y; s1.z += a1.z; s1.w += a1.w;
        s2.x += a2.x; s2.y += a2.y;
      }
      __syncthreads();
    }
  }
  TRM(1)
  // every output of this Gaussian stays in registers until the dL/dtau hand-off below has been made:
  // the hand-off drains this wave's outstanding stores (s_waitcnt vmcnt(0)), so the bulk stores come last
  GaussianGrads o;
  o.m2x = o.m2y = o.ca = o.cb = o.cc = o.op = o.dz = 0.f;
  o.col = o.gm = o.scale = make_float3(0.f, 0.f, 0.f);
  o.rot = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 6; k++) o.cov[k] = 0.f;
  if (vis)
    gaussian_chain(p, mean, c6, sc, q, cl, s0, s1, s2, sh_io + tid * shs_stride, sh_io + tid * shs_stride,
                   p.dL_dscale != nullptr, o, tau);
  TRM(2)
  // ---- 7. wave partial of dL/dtau (fixed butterfly) ----
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float v = wave_sum(tau[k]);
    if (tid == 0) lb_publish(&g.tau_partials[(size_t)blockIdx.x * 8 + k], v);  // (6 floats in an 8-float slot: two 16-byte loads)
  }
  // ---- 8. the last workgroup to arrive sums the partials in workgroup order (fp64): deterministic, no extra launch (replaces
  // torch.sum over [P,6], diff_gaussian_rasterization/__init__.py:162).  The hand-off is last_block.h's, the ticket counters[3].
  if (p.dL_dtau_sum && lb_arrive(&counters[3], &s_last)) {
    double acc6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    lb_sum_partials(g.tau_partials, (int)gridDim.x, tid, acc6);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double v = wave_sum(acc6[k]);
      if (tid == 0) p.dL_dtau_sum[k] = (float)v;
    }
    if (tid == 0) lb_reset(&counters[3]);  // ready for the next backward over this workspace
  }
  TRM(3)
  // ---- 9. outputs: one row per Gaussian, zeros for culled ones (the reference's binding memsets first) ----
  if (idx < p.P && p.dL_dmean2D) {  // pose-only mode (all per-Gaussian outputs NULL) stores nothing per Gaussian
    const size_t i = (size_t)idx;
    p.dL_dmean2D[3 * i] = o.m2x; p.dL_dmean2D[3 * i + 1] = o.m2y; p.dL_dmean2D[3 * i + 2] = 0.f;
    reinterpret_cast<float4 *>(p.dL_dconic)[i] = make_float4(o.ca, o.cb, 0.f, o.cc);
    p.dL_dopacity[i] = o.op;
    p.dL_dcolor[3 * i] = o.col.x; p.dL_dcolor[3 * i + 1] = o.col.y; p.dL_dcolor[3 * i + 2] = o.col.z;
    p.dL_ddepth[i] = o.dz;
    p.dL_dmean3D[3 * i] = o.gm.x; p.dL_dmean3D[3 * i + 1] = o.gm.y; p.dL_dmean3D[3 * i + 2] = o.gm.z;
#pragma unroll
    for (int k = 0; k < 6; k++) p.dL_dcov3D[6 * i + k] = o.cov[k];
    if (p.scales) {
      p.dL_dscale[3 * i] = o.scale.x; p.dL_dscale[3 * i + 1] = o.scale.y; p.dL_dscale[3 * i + 2] = o.scale.z;
      reinterpret_cast<float4 *>(p.dL_drot)[i] = o.rot;
    }
  }
  if (idx < p.P && p.dL_dtau) {
#pragma unroll
    for (int k = 0; k < 6; k++) p.dL_dtau[6 * (size_t)idx + k] = tau[k];
  }
  // dL/dSH block: coalesced store (rows of culled Gaussians and coefficients above the active degree are zero)
  if (p.shs && p.dL_dsh) {
    if (!vis) {
      for (int k = 0; k < shw; k++) sh_io[tid * shs_stride + k] = 0.f;
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * GB_BLOCK * shw;
    const int count = min(GB_BLOCK, p.P - blockIdx.x * GB_BLOCK) * shw;
    for (int e = tid; e < count; e += GB_BLOCK) {
      const int gi = e / shw, k = e - gi * shw;
      p.dL_dsh[base + e] = sh_io[gi * shs_stride + k];
    }
  }
  TRM(4)
  GSAJ_TRACE_END(gbwd)
#ifdef GSAJ_BLOCK_TRACE
  if (tid == 0 && blockIdx.x < GSAJ_TRACE_MAX) {
    unsigned long long *t = g_trace_gbwd + 4 * blockIdx.x;
    t[2] = (tr_[0] << 42) | (tr_[1] << 21) | tr_[2];
    t[3] = (tr_[3] << 21) | tr_[4];
  }
#endif
}

// k_gaussian_bwd's LDS: rows[] (one trip of 256 instance rows) and s_last as __shared__; with SH coefficients, GB_BLOCK padded rows of
// 3 M + 1 floats of dynamic LDS (M <= 16: 12.25 KB at the most)
constexpr size_t GAUSSIAN_BWD_STATIC_LDS = lds_static_round(sizeof(float4[256 * REC_F4]) + sizeof(bool));
LdsRequest lds_gaussian_bwd(int M, bool has_shs) {
  LdsRequest r;
  r.dynamic_bytes = has_shs ? sizeof(float) * GB_BLOCK * (3 * (size_t)M + 1) : 0;
  r.static_bytes = GAUSSIAN_BWD_STATIC_LDS;
  r.limit_bytes = LDS_DEFAULT_LIMIT;
  r.variant = has_shs && (M == 1 || M == 4 || M == 9 || M == 16) ? 3 * M : 0;
  return r;
}

// The SH storage widths the per-Gaussian kernels are instantiated at: f(std::integral_constant<int, 3 M>) for M = 0 (no SH), 1, 4, 9 or
// 16 coefficients; any other M: f is not called, false
template <typename F>
static bool sh_for_m(int M, F &&f) {
  switch (M) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case 1: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 12>{}); return true;
    case 9: f(std::integral_constant<int, 27>{}); return true;
    case 16: f(std::integral_constant<int, 48>{}); return true;
    default: return false;
  }
}

int launch_gaussian_backward(const BwdParams &p, const GeomWS &g, const BinWS &b, const ImageWS &im, hipStream_t s) {
  const int nblk = (p.P + GB_BLOCK - 1) / GB_BLOCK;
  {
    GsajProfScope ps(ST_GAUSSIAN_BWD, s);
    const size_t lds = lds_gaussian_bwd(p.M, p.shs != nullptr).dynamic_bytes;
    auto launch = [&](auto shw) {
      hipLaunchKernelGGL(k_gaussian_bwd<decltype(shw)::value>, dim3(nblk), dim3(GB_BLOCK), lds, s, p, g, im.counters, b.inst_grad, b.reached);
    };
    if (!sh_for_m(p.shs ? p.M : 0, launch)) launch(std::integral_constant<int, 0>{});  // (any other M: the runtime-width instantiation)
  }
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// ---- batched: K views of one map, per-Gaussian parameter gradients summed over the views IN-KERNEL --------------------
// A mapping window renders every keyframe against the same Gaussians and back-propagates once, so the per-Gaussian
// gradients accumulate over keyframes while every keyframe keeps its own dL/dtau (reference utils/slam_backend.py:168-232).
// A whole window (gsaj_rasterize_backward_batch without GSAJ_BWD_ONLY_*): one launch per 8 views and one for dL/dtau,
//  k_chain_window<SHW, true> + k_tau_sum: the chain kernel sums a Gaussian's per-instance partial-gradient rows ITSELF (RowWalk,
//    one wave per two views of 32 Gaussians) and runs the chain on the totals; gsum is neither written nor read.
// The two halves of a window called separately (GSAJ_BWD_ONLY_COMPOSITE, then GSAJ_BWD_ONLY_CHAIN: two streams, tile bands):
//  k_gather_sums (grid x K, HBM-streaming, many waves in flight): the same walk, one wave per 64 Gaussians of a view, the same
//    bits; 48 bytes per Gaussian and view out (gsum).
//  k_chain_window<SHW, false> + k_tau_sum: below; reads gsum.
// one step of the keyed wave scan: lanes that receive a value through the DPP pattern CTRL (row mask ROWS) add it iff it comes from
// the same owner; lanes the pattern does not reach see the key -1 and add nothing
// Each value and step is ONE v_fmac_f32 with a DPP operand: v += dpp(v) * same, same = 1.0 where the incoming value is the lane's own
// owner's, else 0.0 (sums are finite, so x * 0 = 0 and x * 1 + v is the add, bit for bit); a lane the pattern does not reach is not
// written (bound_ctrl off).  As "v += same ? dpp(v) : 0" every value and step cost a zero initialisation, a DPP move, a select and an
// add, and the kernel was as VALU-bound (0.71) as it was HBM-bound.  (Masking the adds with EXEC instead does not work: a DPP read
// of a lane that EXEC disables is an invalid read, and the lanes to be skipped are other lanes' sources.)
#define GSAJ_SCAN_STEP(DPPSTR)                                                                                          \
  asm volatile("v_fmac_f32_dpp %[v0], %[v0], %[m] " DPPSTR "\n\tv_fmac_f32_dpp %[v1], %[v1], %[m] " DPPSTR "\n\t"           \
               "v_fmac_f32_dpp %[v2], %[v2], %[m] " DPPSTR "\n\tv_fmac_f32_dpp %[v3], %[v3], %[m] " DPPSTR "\n\t"           \
               "v_fmac_f32_dpp %[v4], %[v4], %[m] " DPPSTR "\n\tv_fmac_f32_dpp %[v5], %[v5], %[m] " DPPSTR "\n\t"           \
               "v_fmac_f32_dpp %[v6], %[v6], %[m] " DPPSTR "\n\tv_fmac_f32_dpp %[v7], %[v7], %[m] " DPPSTR "\n\t"           \
               "v_fmac_f32_dpp %[v8], %[v8], %[m] " DPPSTR "\n\tv_fmac_f32_dpp %[v9], %[v9], %[m] " DPPSTR                   \
               : [v0] "+v"(v[0]), [v1] "+v"(v[1]), [v2] "+v"(v[2]), [v3] "+v"(v[3]), [v4] "+v"(v[4]), [v5] "+v"(v[5]),       \
                 [v6] "+v"(v[6]), [v7] "+v"(v[7]), [v8] "+v"(v[8]), [v9] "+v"(v[9])                                          \
               : [m] "v"(same))
template <int CTRL, int ROWS>
__device__ __forceinline__ void scan_by_key_step(int own, float (&v)[10]) {
  const int own_in = __builtin_amdgcn_update_dpp(-1, own, CTRL, ROWS, 0xF, false);
  const float same = own_in == own ? 1.0f : 0.0f;
  static_assert(CTRL == 0x111 || CTRL == 0x112 || CTRL == 0x114 || CTRL == 0x118 || CTRL == 0x142 || CTRL == 0x143, "the six steps of the wave scan");
  if constexpr (CTRL == 0x111) GSAJ_SCAN_STEP("row_shr:1 row_mask:0xf bank_mask:0xf");
  else if constexpr (CTRL == 0x112) GSAJ_SCAN_STEP("row_shr:2 row_mask:0xf bank_mask:0xf");
  else if constexpr (CTRL == 0x114) GSAJ_SCAN_STEP("row_shr:4 row_mask:0xf bank_mask:0xf");
  else if constexpr (CTRL == 0x118) GSAJ_SCAN_STEP("row_shr:8 row_mask:0xf bank_mask:0xf");
  else if constexpr (CTRL == 0x142) GSAJ_SCAN_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf");
  else GSAJ_SCAN_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf");
}
#undef GSAJ_SCAN_STEP

// The per-lane preamble of a RowWalk (below): lane = owner, N consecutive owners per wave (64) or half-wave (32)
struct OwnerRows {
  uint32_t cnt, first, endi;  // the lane's own run; its end slot, non-decreasing over the N lanes
  uint32_t F, E;              // rows of the N owners (F = ~0u: none)
  uint32_t block_off;         // rows before the owner's PRE_BLOCK block (the chain kernel derives its grid origin from it)
};
// live: the lane has a Gaussian whose frame was not aborted (an aborted async frame has no rows)
template <int N>
__device__ __forceinline__ OwnerRows owner_rows(bool live, const GeomWS &g, size_t ii) {
  OwnerRows o;
  o.cnt = live ? g.tiles_touched[ii] : 0u;
  o.block_off = live ? g.block_sums[ii / PRE_BLOCK] : 0u;
  const uint32_t endi_raw = live ? o.block_off + g.point_offsets[ii] : 0u;  // (block-local scan + the block's offset)
  o.endi = wave_incl_scan_max<N>(endi_raw);  // (culled / out-of-range owners repeat their predecessor's end)
  o.first = live ? endi_raw - o.cnt : o.endi;
  o.F = wave_min<N>((o.cnt > 0) ? o.first : 0xffffffffu);
  o.E = (uint32_t)__shfl((int)o.endi, N - 1, N);
  return o;
}

// ---- RowWalk: the per-instance gradient rows of OWNERS consecutive Gaussians, summed per Gaussian ------------------------------
// Gaussian i owns rows [first, first + cnt) of inst_grad by emission slot and consecutive Gaussians own consecutive runs, so the
// rows of OWNERS consecutive Gaussians are ONE contiguous block [F, E) ordered by owner.  A wave walks it with lane = ROW, 64 rows
// (a group) at a time with fully coalesced loads: every row finds its owner by a binary search over the owners' end slots (lane
// shuffles), a scan-by-key runs over the 64 rows (Hillis-Steele, add when the owner of lane l equals the owner of lane l - d: exact
// for contiguous segments; DPP, no LDS) and each owner picks up its run's total at its run's last row of the group.  No LDS staging
// and no per-lane loop over a heavy-tailed run length (that loop kept ~20 % of the lanes busy and its scattered ds_read_b128
// conflicted 4-way: 100 us; this form: see profiles/).
//  The grid.  The additions follow a fixed tree per group and the groups in order, so a run's total depends on where the group
//   boundaries fall inside it.  There is ONE grid per block of 64 Gaussians: groups start at G + 64 k, G = the block's first row.
//   64 owners (k_gather_sums) are that block: the walk starts at F = G.  32 owners (k_chain_window, a half-block) start at the group
//   of the same grid that holds their first row, G + ((F - G) & ~63): the same additions in the same order as the walk over all 64,
//   the same bits.
//  Foreign rows.  The first and the last group of 32 owners may hold rows of the other half-block: never fetched, value 0, owner key
//   -2.  A segment's scan result depends on its own lanes only, and what the keyed fmac adds from another owner is x * 0 = +-0,
//   which no non-zero value and no final sum -- sums start at +0 and +0 + -0 = +0 -- can tell apart.  (64 owners have none: rows
//   past E are 0 and no owner's run reaches them.)
//  Prefetch.  Rows the reverse compositor never wrote (`reached` = 0: no pixel of the tile got that far -- most of an opaque scene's
//   instances) are not fetched: the one-byte flags run TWO groups ahead of the rows they admit, the rows ONE group ahead of their
//   use; only the first group is fetched without waiting for its flags.  A group none of whose rows was reached adds nothing and
//   is skipped.
// The caller hands start() F, E and G as scalars (readfirstlane: the group loop and its bounds then run on the scalar unit; DESIGN.md has the figures);
// endi (the owners' end slots, non-decreasing inside each group of OWNERS lanes), first and cnt (the lane's own run) are owner_rows'
// above.
template <int OWNERS>
struct RowWalk {
  static_assert(OWNERS == 32 || OWNERS == 64, "a wave or a half-wave of owners");
  const float4 *__restrict__ inst_grad;
  const uint8_t *__restrict__ reached;
  uint32_t F, E, base;  // the owners' rows [F, E); first row of the current group
  int src;              // first lane of the owners
  float4 a0, a1, a2;
  uint8_t fl, fl_a, fl_b;  // flags of the group in (a0, a1, a2), of the next group, of the one after

  __device__ __forceinline__ bool active() const { return base < E; }  // a group is left to walk
  __device__ __forceinline__ bool inside(uint32_t r) const { return (OWNERS == 64 || r >= F) && r < E; }
  __device__ __forceinline__ uint8_t flags_of(uint32_t b, int lane) const { return inside(b + (uint32_t)lane) ? reached[b + lane] : (uint8_t)0; }
  __device__ __forceinline__ void rows_of(uint32_t b, int lane) {
    const float4 *rp = inst_grad + (size_t)(b + lane) * REC_F4;
    a0 = rp[0]; a1 = rp[1]; a2 = rp[2];
  }
  // requests the first group's flags and rows (the rows without waiting for their flags) and the flags of the next two groups
  __device__ __forceinline__ void start(bool on, int first_lane, int lane, uint32_t F_, uint32_t E_, uint32_t G, const float4 *ig,
                                        const uint8_t *rc) {
    inst_grad = ig; reached = rc;
    src = first_lane; F = F_;
    E = on && F != 0xffffffffu && F < E_ ? E_ : 0u;  // (no rows, no walk: nothing is inside)
    base = OWNERS == 64 ? F : G + ((F - G) & ~63u);
    fl = flags_of(base, lane);
    if (inside(base + (uint32_t)lane)) rows_of(base, lane);
    fl_a = flags_of(base + 64, lane);
    fl_b = flags_of(base + 128, lane);
  }
  // one group of 64 rows: requests the next group's rows, reduces the current one, owners take their runs' totals
  __device__ __forceinline__ void step(int lane, uint32_t endi, uint32_t first, uint32_t cnt, float (&sum)[10]) {
    const uint32_t r = base + (uint32_t)lane;
    const bool ok = fl != 0;
    float v[10] = {ok ? a0.x : 0.f, ok ? a0.y : 0.f, ok ? a0.z : 0.f, ok ? a0.w : 0.f, ok ? a1.x : 0.f,
                   ok ? a1.y : 0.f, ok ? a1.z : 0.f, ok ? a1.w : 0.f, ok ? a2.x : 0.f, ok ? a2.y : 0.f};
    if (base + 64 < E) {
      fl = fl_a;
      if (fl) rows_of(base + 64, lane);
      fl_a = fl_b;
      fl_b = flags_of(base + 192, lane);
    }
    if (__builtin_amdgcn_ballot_w64(ok) != 0ull) {
      // owner of row r = number of owners whose end slot is <= r (end slots are non-decreasing): binary search by shuffles
      int own = 0;
#pragma unroll
      for (int st = OWNERS / 2; st > 0; st >>= 1) {
        const uint32_t e = (uint32_t)__shfl((int)endi, src + own + st - 1);
        if (e <= r) own += st;
      }
      if (OWNERS < 64 && !inside(r)) own = -2;
      // scan by key: after the last step lane l holds the sum of the rows of its owner in [max(run start, base), r].  All in the
      // VALU (DPP): four row_shr steps inside each 16-lane row, then row_bcast:15 (rows 1, 3 take lane 15 / 47) and row_bcast:31
      // (rows 2, 3 take lane 31, which by then carries rows 0-1) -- the keyed form of the classic wave scan
      scan_by_key_step<0x111, 0xF>(own, v);  // row_shr:1
      scan_by_key_step<0x112, 0xF>(own, v);  // row_shr:2
      scan_by_key_step<0x114, 0xF>(own, v);  // row_shr:4
      scan_by_key_step<0x118, 0xF>(own, v);  // row_shr:8
      scan_by_key_step<0x142, 0xA>(own, v);  // row_bcast:15 -> rows 1, 3
      scan_by_key_step<0x143, 0xC>(own, v);  // row_bcast:31 -> rows 2, 3
      // every owner whose run meets this group takes the total at its run's last row inside the group
      const uint32_t run_lo = max(first, base), run_hi = min(first + cnt, min(base + 64u, E));
      const bool mine = (OWNERS == 64 || (lane & OWNERS) == src) && cnt > 0 && run_lo < run_hi;
      const int q = mine ? (int)(run_hi - 1u - base) : 0;
#pragma unroll
      for (int c = 0; c < 10; c++) {
        const float t = __shfl(v[c], q);
        sum[c] += mine ? t : 0.f;
      }
    }
    base += 64;
  }
};

// k_gather_sums: one wave = one block of 64 Gaussians of one view, one RowWalk<64>; 48 bytes per Gaussian and view out (gsum)
GSAJ_TRACE_DEFINE(gath)
__global__ __launch_bounds__(256) void k_gather_sums(int P, const int *__restrict__ radii0, GeomWS g0, ImageWS im0,
                                                     const float4 *__restrict__ inst_grad0, const uint8_t *__restrict__ reached0,
                                                     ViewStrides vs) {
  GSAJ_TRACE_BEGIN(gath)
  const size_t view = blockIdx.y;
  const GeomWS g = geom_view(g0, view * vs.geom);
  const uint32_t *counters = gsaj_shift(im0.counters, view * vs.image);
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const size_t ii = (size_t)(idx < P ? idx : 0);
  const OwnerRows o = owner_rows<64>(idx < P && counters[4] == 0u, g, ii);
  float sum[10];
#pragma unroll
  for (int c = 0; c < 10; c++) sum[c] = 0.f;
  RowWalk<64> w;
  const uint32_t F = (uint32_t)__builtin_amdgcn_readfirstlane((int)o.F), E = (uint32_t)__builtin_amdgcn_readfirstlane((int)o.E);
  w.start(true, 0, lane, F, E, F, gsaj_shift(inst_grad0, view * vs.bin), gsaj_shift(reached0, view * vs.bin));
  while (w.active()) w.step(lane, o.endi, o.first, o.cnt, sum);
  if (idx < P) {
    g.gsum[3 * ii + 0] = make_float4(sum[0], sum[1], sum[2], sum[3]);
    g.gsum[3 * ii + 1] = make_float4(sum[4], sum[5], sum[6], sum[7]);
    g.gsum[3 * ii + 2] = make_float4(sum[8], sum[9], 0.f, 0.f);
  }
  (void)radii0;
  GSAJ_TRACE_END(gath)
}

// ---- the batched per-Gaussian backward ------------------------------------------------------------------------------
// (round 2 ran it as 64 Gaussians x 4 waves, wave w taking views w, w + 4 one after the other with the SH backward inside:
// 213 VGPRs, two waves per SIMD, a wave alive for 27 us of which 5 us issued instructions -- 70 us per cfg2 window.)
//
//  k_chain_window  one workgroup = 32 Gaussians x 8 views, lane = (view, Gaussian): every lane runs the whole per-view chain on
//                  that view's sums (gaussian_chain_geom + the view-direction term of the SH colour) -- K x P independent lanes
//                  fill the chip -- writes the view's own outputs (dL/dmean2D, ..., a dL/dtau partial per 32 Gaussians), and
//                  leaves what the sums over views need in LDS: (dL/dopacity, dL/dmean3D, dL/dcov3D, the colour gradient
//                  masked by the clamp flags, the SH basis weights of the view direction).  After a barrier the workgroup adds
//                  the views IN VIEW ORDER (fixed order: bit-reproducible): thread t owns up to 8 of the 32 x (10 + 3 M)
//                  elements -- component c of a Gaussian, or dL/dSH[k][ch] = sum_v w_k(view) g_v[ch] -- through every group
//                  launch of 8 views (K > 8: further launches ADD to the outputs, in view order); dL/dscale, dL/drot are formed ONCE from the summed dL/dcov3D (they are linear in it with
//                  view-independent coefficients); the block's outputs go out transposed through LDS, contiguous rows.
//                  Nothing per (view, Gaussian) goes through memory except what the caller asked for.
//  k_tau_sum       one workgroup per view adds that view's dL/dtau partials up in slot order (fp64).  No tickets: 31 256
//                  workgroups (cfg5 window) drawing tickets from ONE word per view run at the ~88 returning atomics per us a
//                  single address sustains (MI355X_MICROARCH.md, dequeue) -- 0.36 ms of a 1.2 ms kernel when tried.
#define CW_G 32   // Gaussians per workgroup
#define CW_V 8    // views per pass
GSAJ_TRACE_DEFINE(gbb)

// k_chain_window<., GATHER = true>: the ten sums of a (view, Gaussian) lane formed in the kernel.  The 32 lanes of a half-wave are the
// 32 Gaussians of one view, a half-block of k_gather_sums' 64: the WHOLE wave walks their rows with a RowWalk<CW_G> on that block's
// grid, so every sum is bit-identical to what k_gather_sums leaves in gsum.  A wave runs its two views' walks side by side (start,
// then step by turns), so that two groups of rows are on their way at any time.
template <int SHW, bool GATHER>
__global__ __launch_bounds__(CW_G * CW_V, 4) void k_chain_window(BwdParams p, int v0, int K, GeomWS g0, ImageWS im0, ViewStrides vs,
                                                              const float4 *__restrict__ inst_grad0, const uint8_t *__restrict__ reached0,
                                                              float *__restrict__ pv_mean2D, float *__restrict__ pv_conic,
                                                              float *__restrict__ pv_color, float *__restrict__ pv_depth,
                                                              float *__restrict__ pv_tau, int accumulate) {
  constexpr int MC = SHW / 3;           // SH coefficients stored
  constexpr int NV = 13 + MC;           // values a (view, Gaussian) lane leaves for the sums
  constexpr int NE = 10 + SHW;          // summed outputs per Gaussian
  constexpr int EPT = (NE * CW_G + CW_G * CW_V - 1) / (CW_G * CW_V);  // elements per thread
  __shared__ __attribute__((aligned(16))) float rowv[CW_V * NV * CW_G];  // [view lane][value][Gaussian]
  __shared__ float outv[NE * CW_G];         // [element][Gaussian]: the sums, for the transposed store
  GSAJ_TRACE_BEGIN(gbb)
  const int tid = threadIdx.x, gl = tid & (CW_G - 1), vl = tid / CW_G;
  const int idx = blockIdx.x * CW_G + gl;
  const size_t ii = (size_t)(idx < p.P ? idx : 0);
  // inputs that do not depend on the view: once
  const float3 mean = make_float3(p.means3D[3 * ii], p.means3D[3 * ii + 1], p.means3D[3 * ii + 2]);
  float c6[6];
  if constexpr (!GATHER) {
#pragma unroll
    for (int k = 0; k < 6; k++) c6[k] = p.cov3Ds[6 * ii + k];  // (view 0's copy: Sigma = R S^2 R^T does not depend on the view)
  }
  const float *vm0 = p.viewmatrix, *pj0 = p.projmatrix;
  float acc[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) acc[j] = 0.f;
  // views [v0, min(v0 + 8, K)) of the window.  (A loop over the groups of 8 views INSIDE the kernel cost 70 VGPRs: 201 instead of
  // 132 -- the compiler kept view-independent values alive across it, whatever was hidden from it.)
  {
    const int v = v0 + vl;
    GaussianGrads o;
    o.m2x = o.m2y = o.ca = o.cb = o.cc = o.op = o.dz = 0.f;
    o.col = o.gm = make_float3(0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; k++) o.cov[k] = 0.f;
    float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float w[MC > 0 ? MC : 1];  // SH basis weights of this view's direction
#pragma unroll
    for (int k = 0; k < MC; k++) w[k] = 0.f;
    float3 gmask = make_float3(0.f, 0.f, 0.f);
    bool sh_left = false;
    // GATHER: this lane's ten sums, formed here (the wave walks the instance rows of its two views' 32 Gaussians)
    uint32_t aborted_w = 0u;
    int rad_w = 0;
    uint8_t cl_w[3] = {0, 0, 0};
    if constexpr (GATHER) {
      float sum[10];
      const int lane = tid & 63;
      const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's views: v0 + 2 wv (lanes 0-31), v0 + 2 wv + 1 (lanes 32-63)
      const size_t vc = (size_t)(v < K ? v : v0);  // (a lane past the window's last view reads view v0's and uses nothing of it)
      const GeomWS gw = geom_view(g0, vc * vs.geom);
      aborted_w = gsaj_shift(im0.counters, vc * vs.image)[4];
      rad_w = p.radii[vc * p.P + ii];
      if (SHW > 0) { cl_w[0] = gw.clamped[3 * ii]; cl_w[1] = gw.clamped[3 * ii + 1]; cl_w[2] = gw.clamped[3 * ii + 2]; }
      const bool live = v < K && idx < p.P && aborted_w == 0u;
      const OwnerRows o = owner_rows<CW_G>(live, gw, ii);
      // the grid's origin: first row of the enclosing block of 64 Gaussians = end slot of the Gaussian before it (same PRE_BLOCK)
      const int i64 = ((int)blockIdx.x & ~1) * CW_G;
      const uint32_t G32 = live ? o.block_off + ((i64 % PRE_BLOCK) ? gw.point_offsets[i64 - 1] : 0u) : 0u;
#pragma unroll
      for (int c = 0; c < 10; c++) sum[c] = 0.f;
      // the wave's two views side by side: two independent row streams in flight (one after the other, a wave had one group of rows
      // on its way at a time and the walk was bound by that round trip).  Each stream's F, E, G: its half-wave's, made scalars.
      // (G from lane 0 of the half, which is in range whenever the workgroup exists)
      auto of_half = [&](uint32_t x, int half) { return (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)x, half * CW_G)); };
      const int vA = v0 + 2 * wv;
      RowWalk<CW_G> sa, sb;
      sa.start(vA < K, 0, lane, of_half(o.F, 0), of_half(o.E, 0), of_half(G32, 0), gsaj_shift(inst_grad0, (size_t)min(vA, K - 1) * vs.bin),
               gsaj_shift(reached0, (size_t)min(vA, K - 1) * vs.bin));
      sb.start(vA + 1 < K, CW_G, lane, of_half(o.F, 1), of_half(o.E, 1), of_half(G32, 1), gsaj_shift(inst_grad0, (size_t)min(vA + 1, K - 1) * vs.bin),
               gsaj_shift(reached0, (size_t)min(vA + 1, K - 1) * vs.bin));
      while (sa.active() || sb.active()) {
        if (sa.active()) sa.step(lane, o.endi, o.first, o.cnt, sum);
        if (sb.active()) sb.step(lane, o.endi, o.first, o.cnt, sum);
      }
      // handed to the chain through LDS, in slots 0-9 of this view lane's part of rowv (320 floats: [32] float4 | [32] float4 | [32]
      // float2; the chain writes those slots last, after every read; a lane reads what it wrote itself: no barrier).  The chain below
      // then starts from 16-byte loads as it does on gsum and compiles to the same arithmetic -- contracting a * b + c into an fma
      // is the compiler's choice and follows the form of the inputs: fed from scalar registers, dL/dtau came out 1 ulp different.
      float *stage = rowv + vl * NV * CW_G;
      reinterpret_cast<float4 *>(stage)[gl] = make_float4(sum[0], sum[1], sum[2], sum[3]);
      reinterpret_cast<float4 *>(stage + 4 * CW_G)[gl] = make_float4(sum[4], sum[5], sum[6], sum[7]);
      reinterpret_cast<float2 *>(stage + 8 * CW_G)[gl] = make_float2(sum[8], sum[9]);
      asm volatile("" ::: "memory");  // (no store-to-load forwarding)
    }
    if (v < K) {
      const GeomWS g = geom_view(g0, (size_t)v * vs.geom);
      const size_t iv = ii;
      const float3 mean_v = mean;
      const float (&c6v)[6] = c6;
      // every input of this (view, Gaussian) requested up front and unconditionally
      const uint32_t aborted = GATHER ? aborted_w : gsaj_shift(im0.counters, (size_t)v * vs.image)[4];  // aborted async frame: contributes nothing
      const int rad = GATHER ? rad_w : p.radii[(size_t)v * p.P + ii];
      float4 s0, s1, s2;
      if constexpr (GATHER) {
        const float *stage = rowv + vl * NV * CW_G;
        s0 = reinterpret_cast<const float4 *>(stage)[gl];
        s1 = reinterpret_cast<const float4 *>(stage + 4 * CW_G)[gl];
        const float2 s2h = reinterpret_cast<const float2 *>(stage + 8 * CW_G)[gl];
        s2 = make_float4(s2h.x, s2h.y, 0.f, 0.f);
      } else {
        s0 = g.gsum[3 * ii + 0]; s1 = g.gsum[3 * ii + 1]; s2 = g.gsum[3 * ii + 2];
      }
      uint8_t cl[3] = {0, 0, 0};
      if (SHW > 0 && GATHER) { cl[0] = cl_w[0]; cl[1] = cl_w[1]; cl[2] = cl_w[2]; }
      else if (SHW > 0) { cl[0] = g.clamped[3 * ii]; cl[1] = g.clamped[3 * ii + 1]; cl[2] = g.clamped[3 * ii + 2]; }
      p.viewmatrix = vm0 + 16 * v;
      p.projmatrix = pj0 + 16 * v;
      const bool vis = idx < p.P && !aborted && rad > 0;
      if (vis) {
        // the view-direction term first: its 3 M coefficient loads are consumed (and their registers free) before the geometric
        // chain's own peak
        float3 dmean = make_float3(0.f, 0.f, 0.f);
        if (SHW > 0) {
          const float *cam = p.campos + 3 * v;
          constexpr int DEG_MAX = MC >= 16 ? 3 : (MC >= 9 ? 2 : (MC >= 4 ? 1 : 0));  // (the storage bounds the degree: dead bands compile away)
          const float3 gcol = make_float3(s1.z, s1.w, s2.x);
          dmean = sh_backward<1>(min(p.D, DEG_MAX), p.M, mean_v, make_float3(cam[0], cam[1], cam[2]), p.shs + iv * SHW, w, cl, gcol);
          gmask = make_float3(cl[0] ? 0.f : gcol.x, cl[1] ? 0.f : gcol.y, cl[2] ? 0.f : gcol.z);
          if constexpr (GATHER) {
            // left in LDS at once, not carried through the geometric chain: 3 + M registers less at the kernel's register peak
            // (slots 10 and up: clear of the staged sums in slots 0-9, which are read once more below)
            float *mine = rowv + vl * NV * CW_G + gl;
            mine[10 * CW_G] = gmask.x; mine[11 * CW_G] = gmask.y; mine[12 * CW_G] = gmask.z;
#pragma unroll
            for (int k = 0; k < MC; k++) mine[(13 + k) * CW_G] = w[k];
            sh_left = true;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (GATHER) {
          // requested here, behind the view-direction term's register peak (the row walk is no place to hold them); the sums, of which
          // that term needed the colour part only, are read from LDS again rather than carried through it
#pragma unroll
          for (int k = 0; k < 6; k++) c6[k] = p.cov3Ds[6 * ii + k];
          if (SHW > 0) {
            asm volatile("" ::: "memory");
            const float *stage = rowv + vl * NV * CW_G;
            s0 = reinterpret_cast<const float4 *>(stage)[gl];
            s1 = reinterpret_cast<const float4 *>(stage + 4 * CW_G)[gl];
            const float2 s2h = reinterpret_cast<const float2 *>(stage + 8 * CW_G)[gl];
            s2 = make_float4(s2h.x, s2h.y, 0.f, 0.f);
          }
        }
        gaussian_chain_geom(p, mean_v, c6v, s0, s1, s2, o, tau);
        if (SHW > 0) {
          o.gm.x += dmean.x; o.gm.y += dmean.y; o.gm.z += dmean.z;
          tau[0] -= dmean.x; tau[1] -= dmean.y; tau[2] -= dmean.z;
        }
      }
      // the view's own outputs
      if (idx < p.P) {
        const size_t row = (size_t)v * p.P + ii;
        if (pv_mean2D) { pv_mean2D[3 * row] = o.m2x; pv_mean2D[3 * row + 1] = o.m2y; pv_mean2D[3 * row + 2] = 0.f; }
        if (pv_conic) reinterpret_cast<float4 *>(pv_conic)[row] = make_float4(o.ca, o.cb, 0.f, o.cc);
        if (pv_color) { pv_color[3 * row] = o.col.x; pv_color[3 * row + 1] = o.col.y; pv_color[3 * row + 2] = o.col.z; }
        if (pv_depth) pv_depth[row] = o.dz;
        if (pv_tau) {
#pragma unroll
          for (int k = 0; k < 6; k++) pv_tau[6 * row + k] = tau[k];
        }
      }
      // this view's dL/dtau: partial over the 32 Gaussians (the lanes of one half-wave), one slot per (view, workgroup); k_tau_sum
      // adds the slots up
      float t6[6];
#pragma unroll
      for (int k = 0; k < 6; k++) {
        t6[k] = wave_sum<CW_G>(tau[k]);
      }
      if (gl == 0) {
        float4 *tp = reinterpret_cast<float4 *>(g.tau_partials + (size_t)blockIdx.x * 8);
        tp[0] = make_float4(t6[0], t6[1], t6[2], t6[3]);
        tp[1] = make_float4(t6[4], t6[5], 0.f, 0.f);
      }
    }
    // ---- what the sums over views need, through LDS ----
    float *mine = rowv + vl * NV * CW_G + gl;
    mine[0 * CW_G] = o.op; mine[1 * CW_G] = o.gm.x; mine[2 * CW_G] = o.gm.y; mine[3 * CW_G] = o.gm.z;
#pragma unroll
    for (int k = 0; k < 6; k++) mine[(4 + k) * CW_G] = o.cov[k];
    if constexpr (GATHER && SHW > 0) {
      if (!sh_left) {  // (a lane that ran the view-direction term has left these already; the others leave zeros)
        mine[10 * CW_G] = 0.f; mine[11 * CW_G] = 0.f; mine[12 * CW_G] = 0.f;
#pragma unroll
        for (int k = 0; k < MC; k++) mine[(13 + k) * CW_G] = 0.f;
      }
    } else {
      mine[10 * CW_G] = gmask.x; mine[11 * CW_G] = gmask.y; mine[12 * CW_G] = gmask.z;
#pragma unroll
      for (int k = 0; k < MC; k++) mine[(13 + k) * CW_G] = w[k];
    }
    __syncthreads();
    const int nv = min(CW_V, K - v0);
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      const int e = tid + j * (CW_G * CW_V);  // element e = c * 32 + Gaussian: this thread's Gaussian is always gl
      const int c = e / CW_G;
      if (c < NE) {
        float sacc = acc[j];
        if (c < 10) {
#pragma unroll 2
          for (int u = 0; u < nv; u++) sacc += rowv[u * NV * CW_G + c * CW_G + gl];
        } else {
          const int kk = (c - 10) / 3, ch = (c - 10) - 3 * kk;
#pragma unroll 2
          for (int u = 0; u < nv; u++) sacc += rowv[u * NV * CW_G + (13 + kk) * CW_G + gl] * rowv[u * NV * CW_G + (10 + ch) * CW_G + gl];
        }
        acc[j] = sacc;
      }
    }
    __syncthreads();
  }
  // ---- the sums, transposed through LDS: [element][Gaussian] -> rows of the outputs ----
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const int e = tid + j * (CW_G * CW_V);
    if (e < NE * CW_G) outv[e] = acc[j];
  }
  __syncthreads();
  // accumulate: this call's sums are ADDED to what the buffers hold (a window processed in several calls, or keyframes of several
  // windows accumulated on one rank before the optimiser step: callers add in a fixed order, so the result stays reproducible)
#define OUT(dst, x) dst = accumulate ? dst + (x) : (x)
  const int nG = min(CW_G, p.P - (int)blockIdx.x * CW_G);  // Gaussians of this workgroup
  const size_t b0 = (size_t)blockIdx.x * CW_G;
  for (int e = tid; e < nG; e += CW_G * CW_V) OUT(p.dL_dopacity[b0 + e], outv[0 * CW_G + e]);
  for (int e = tid; e < 3 * nG; e += CW_G * CW_V) OUT(p.dL_dmean3D[3 * b0 + e], outv[(1 + e % 3) * CW_G + e / 3]);
  for (int e = tid; e < 6 * nG; e += CW_G * CW_V) OUT(p.dL_dcov3D[6 * b0 + e], outv[(4 + e % 6) * CW_G + e / 6]);
  if (SHW > 0 && p.dL_dsh) {  // (coefficients above the active degree have zero weights: their gradients come out zero)
    for (int e = tid; e < SHW * nG; e += CW_G * CW_V) OUT(p.dL_dsh[(size_t)SHW * b0 + e], outv[(10 + e % SHW) * CW_G + e / SHW]);
  }
  if (p.scales && tid < nG) {  // dL/dscale, dL/drot from the summed dL/dcov3D (this call's part: both are linear in it)
    const size_t i = b0 + tid;
    float gcov[6];
#pragma unroll
    for (int k = 0; k < 6; k++) gcov[k] = outv[(4 + k) * CW_G + tid];
    const float3 sc = make_float3(p.scales[3 * i], p.scales[3 * i + 1], p.scales[3 * i + 2]);
    const float4 q = reinterpret_cast<const float4 *>(p.rotations)[i];
    float3 dscale;
    float4 drot;
    cov3d_backward(gcov, sc, q, p.scale_modifier, dscale, drot);
    OUT(p.dL_dscale[3 * i], dscale.x); OUT(p.dL_dscale[3 * i + 1], dscale.y); OUT(p.dL_dscale[3 * i + 2], dscale.z);
    float4 *dr = reinterpret_cast<float4 *>(p.dL_drot) + i;
    if (accumulate) { const float4 o4 = *dr; drot.x += o4.x; drot.y += o4.y; drot.z += o4.z; drot.w += o4.w; }
    *dr = drot;
  }
#undef OUT
  GSAJ_TRACE_END(gbb)
}

// workgroup `view`: dL_dtau_sum[view] = sum of the view's partials (one per 32 Gaussians) in slot order, fp64
__global__ __launch_bounds__(256) void k_tau_sum(BwdParams p, GeomWS g0, ViewStrides vs) {
  __shared__ double red[256 * 6];
  const int tid = threadIdx.x, view = blockIdx.x, nslot = (p.P + CW_G - 1) / CW_G;
  const float4 *tp = reinterpret_cast<const float4 *>(gsaj_shift(g0.tau_partials, (size_t)view * vs.geom));
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < nslot; i += 256) {
    const float4 lo = tp[2 * i], hi = tp[2 * i + 1];
    a[0] += (double)lo.x; a[1] += (double)lo.y; a[2] += (double)lo.z; a[3] += (double)lo.w; a[4] += (double)hi.x; a[5] += (double)hi.y;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) red[k * 256 + tid] = a[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // fixed tree
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[k * 256 + tid] += red[k * 256 + tid + o];
    }
    __syncthreads();
  }
  if (tid < 6 && p.dL_dtau_sum) p.dL_dtau_sum[6 * view + tid] = (float)red[tid * 256];
}

template <int SHW, bool GATHER>
static void launch_chain(const BwdParams &p, int K, const GeomWS &g, const BinWS &b, const ImageWS &im, ViewStrides vs, int accumulate,
                         hipStream_t s) {
  for (int v0 = 0; v0 < K; v0 += CW_V)  // 8 views per launch; later launches add to the first one's sums (same stream: in view order)
    hipLaunchKernelGGL((k_chain_window<SHW, GATHER>), dim3((p.P + CW_G - 1) / CW_G), dim3(CW_G * CW_V), 0, s, p, v0, K, g, im, vs,
                       b.inst_grad, b.reached, p.dL_dmean2D, p.dL_dconic, p.dL_dcolor, p.dL_ddepth, p.dL_dtau,
                       (accumulate || v0 > 0) ? 1 : 0);
  hipLaunchKernelGGL(k_tau_sum, dim3(K), dim3(256), 0, s, p, g, vs);
}

int launch_gather_sums(int P, int K, const int *radii, const GeomWS &g, const BinWS &b, const ImageWS &im, ViewStrides vs, hipStream_t s) {
  GsajProfScope ps(ST_GATHER_SUMS, s);
  hipLaunchKernelGGL(k_gather_sums, dim3((P + 255) / 256, K), dim3(256), 0, s, P, radii, g, im, b.inst_grad, b.reached, vs);
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}

// gather != 0: the chain kernel sums the reverse compositor's instance rows itself (k_gather_sums has not run, gsum is not touched);
// gather == 0: it reads the sums k_gather_sums left in gsum
int launch_gaussian_backward_batch(const BwdParams &p, int K, const GeomWS &g, const BinWS &b, const ImageWS &im, ViewStrides vs,
                                   int accumulate, int gather, hipStream_t s) {
  GsajProfScope ps(ST_GAUSSIAN_BWD, s);
  const bool known = sh_for_m(p.shs ? p.M : 0, [&](auto shw) {
    if (gather) launch_chain<decltype(shw)::value, true>(p, K, g, b, im, vs, accumulate, s);
    else launch_chain<decltype(shw)::value, false>(p, K, g, b, im, vs, accumulate, s);
  });
  if (!known) {
    gsaj_set_error("batched backward: SH storage of %d coefficients is not supported (1, 4, 9 or 16)", p.M);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  GSAJ_HIP_CHECK(hipGetLastError());
  return GSAJ_OK;
}
