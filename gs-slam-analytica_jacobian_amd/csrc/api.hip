// api.hip -- extern "C" entry points of libgsaj_hip.so (see include/gsaj.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "gsaj_common.h"
#include "loss_terms.h"

static thread_local char g_err[512] = "";

void gsaj_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- event-based per-stage profiler ------------------------------------------------------------
// Shared by every thread / stream of the process: the record table is guarded by a mutex, a record is claimed with an
// atomic index, and the record a launch scope has open is thread-local (a scope opens and closes on one thread), so
// concurrent launches from a tracking and a mapping thread each time their own kernels.
struct ProfRec { int stage; hipEvent_t a, b; };
static std::mutex g_prof_mu;
static ProfRec *g_prof = nullptr;
static std::atomic<bool> g_prof_on{false};
static int g_prof_cap = 0;
static std::atomic<int> g_prof_n{0};
static thread_local int t_prof_open = -1;

void gsaj_prof_mark(int stage, int is_stop, hipStream_t s) {
  if (!g_prof_on.load(std::memory_order_acquire)) return;  // the common case: one relaxed-cost load, no lock
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof) return;
  if (!is_stop) {
    const int i = g_prof_n.fetch_add(1);
    if (i >= g_prof_cap) { g_prof_n.store(g_prof_cap); t_prof_open = -1; return; }
    t_prof_open = i;
    g_prof[i].stage = stage;
    (void)hipEventRecord(g_prof[i].a, s);
  } else if (t_prof_open >= 0 && t_prof_open < g_prof_cap) {
    (void)hipEventRecord(g_prof[t_prof_open].b, s);
    t_prof_open = -1;
  }
}

extern "C" {

int gsaj_profile_begin(int max_records) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof || max_records <= 0) {
    gsaj_set_error("gsaj_profile_begin: already active or bad size");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  g_prof = new ProfRec[max_records];
  for (int i = 0; i < max_records; i++) {
    GSAJ_HIP_CHECK(hipEventCreate(&g_prof[i].a));
    GSAJ_HIP_CHECK(hipEventCreate(&g_prof[i].b));
  }
  g_prof_cap = max_records;
  g_prof_n.store(0);
  g_prof_on.store(true, std::memory_order_release);
  return GSAJ_OK;
}

int gsaj_profile_end(float *stage_ms, int *stage_launches) {
  if (!stage_ms || !stage_launches) {
    gsaj_set_error("gsaj_profile_end: null output");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  g_prof_on.store(false, std::memory_order_release);  // no new records; launches in flight finish under the lock
  GSAJ_HIP_CHECK(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof) {
    gsaj_set_error("gsaj_profile_end: not active");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < ST_COUNT; i++) { stage_ms[i] = 0.f; stage_launches[i] = 0; }
  const int nrec = g_prof_n.load() < g_prof_cap ? g_prof_n.load() : g_prof_cap;
  for (int i = 0; i < nrec; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof[i].a, g_prof[i].b) == hipSuccess) {
      stage_ms[g_prof[i].stage] += ms;
      stage_launches[g_prof[i].stage] += 1;
    }
  }
  for (int i = 0; i < g_prof_cap; i++) { (void)hipEventDestroy(g_prof[i].a); (void)hipEventDestroy(g_prof[i].b); }
  delete[] g_prof;
  g_prof = nullptr;
  g_prof_cap = 0;
  g_prof_n.store(0);
  return GSAJ_OK;
}

const char *gsaj_last_error(void) { return g_err; }
int gsaj_version(void) { return 114; }

// (+ 256: the base slack of a workspace carved from its next 256-byte boundary, workspace.h)
size_t gsaj_geom_workspace_bytes(int P) { GeomWS g; return geom_carve(Carver(nullptr, ALIGN_BASE), (size_t)(P > 0 ? P : 0), &g) + 256; }
size_t gsaj_image_workspace_bytes(int W, int H) { ImageWS im; return image_carve(Carver(nullptr, ALIGN_BASE), W, H, &im) + 256; }
size_t gsaj_binning_workspace_bytes(int R) { BinWS b; return bin_carve(Carver(nullptr, ALIGN_BASE), (size_t)(R > 0 ? R : 0), &b) + 256; }

// ---- argument groups of the rasteriser entry points (host only; DESIGN.md "Argument groups") --------------------------------
// Every extern "C" rasteriser function fills these once from its own parameters -- members in the order of the ABI, so that an
// initialiser reads like the signature -- and the functions behind them take the groups.  Where a launcher's struct already is the
// group it is filled directly: BwdParams holds the twelve gradient outputs and radii, FusedLoss the loss arguments, JacOut the
// Jacobian walk's outputs.
struct Scene {  // the Gaussian map (colors_precomp is in the splat rows once the forward has run: later calls do not read it)
  int P, D, M;
  const float *means3D, *shs, *colors_precomp, *opacities, *scales;
  float scale_modifier;
  const float *rotations, *cov3D_precomp;
};
struct Views {  // K views of it: viewmatrix / projmatrix [K,16], campos [K,3]; the single-frame entry points have K = 1
  int K;
  const float *bg;
  int W, H;
  const float *viewmatrix, *projmatrix, *projmatrix_raw, *campos;
  float tanfovx, tanfovy;
};
struct Arenas {  // the workspaces as the caller handed them over (per view of a batched call: K consecutive blocks each)
  void *geom, *binning;
  size_t binning_bytes;     // what the caller says the binning arena holds (a backward takes no size: the forward checked it)
  int instances;            // what the binning arena is carved for: R (synchronous forms), the capacity (asynchronous and batched)
  int tile_list_capacity;   // asynchronous forms: the tile list the LDS sort is sized for (0: SORT_CAP)
  void *image;
};
struct FwdOut {  // what a forward writes: images [K,3,H,W] / [K,1,H,W], radii / n_touched [K,P]; fused forms: scalars [K,5], dexposure [K,2]
  float *color, *depth, *opacity;
  int *radii, *n_touched;
  float *scalars, *dexposure;
};
struct PixelSeeds {  // where the reverse compositor's dL/dpixel comes from: two images, or (fl != NULL) the loss, derived per pixel
  const float *dL_dpix, *dL_dpix_depth;
  const FusedLoss *fl;
};
struct GnSums {  // what becomes of the Jacobian walk's partial rows: the explicit form sums them into H_out / g_out; the fused form
  float *H_out, *g_out;  // (fl != NULL) leaves them in JacOut.partials for gsaj_pose_gn_step / gsaj_pose_gn8_step (joint)
  FusedLoss *fl;
  bool joint;
};
static const size_t SIZE_NOT_GIVEN = SIZE_MAX;  // Arenas.binning_bytes of the calls that take no size: carve()'s size check always passes

// The one place the three workspaces are carved.  batch_K == 0, the single-frame calls: from the aligned base of whatever the caller
// gave, zero strides.  batch_K > 0, the batched calls: the caller's blocks must be aligned themselves (view v's block is v strides on)
// and K binning blocks must fit.
static int carve(const Arenas &a, int P, int W, int H, int batch_K, Carved *c) {
  c->vs = ViewStrides{0, 0, 0};
  if (batch_K > 0) {
    c->vs.geom = gsaj_geom_workspace_bytes(P);
    c->vs.image = gsaj_image_workspace_bytes(W, H);
    c->vs.bin = gsaj_binning_workspace_bytes(a.instances);
    if (((uintptr_t)a.geom | (uintptr_t)a.binning | (uintptr_t)a.image) & 255) {
      gsaj_set_error("batched entry points need 256-byte aligned workspaces");
      return GSAJ_ERR_INVALID_ARGUMENT;
    }
    if (a.binning_bytes < c->vs.bin * (size_t)batch_K) {
      gsaj_set_error("binning workspace smaller than K x gsaj_binning_workspace_bytes(capacity=%d)", a.instances);
      return GSAJ_ERR_WORKSPACE_TOO_SMALL;
    }
  }
  geom_carve(Carver(a.geom, ALIGN_BASE), (size_t)P, &c->g);
  image_carve(Carver(a.image, ALIGN_BASE), W, H, &c->im);
  bin_carve(Carver(a.binning, ALIGN_BASE), (size_t)a.instances, &c->b);
  return GSAJ_OK;
}

// what every forward asks of the map after its own required pointers
static int check_scene(const char *who, const Scene &sc, const float *campos) {
  if ((sc.shs == nullptr) == (sc.colors_precomp == nullptr)) {
    gsaj_set_error("Please provide excatly one of either SHs or precomputed colors!");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (((sc.scales == nullptr || sc.rotations == nullptr) && sc.cov3D_precomp == nullptr) ||
      ((sc.scales != nullptr || sc.rotations != nullptr) && sc.cov3D_precomp != nullptr)) {
    gsaj_set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (sc.shs && (!campos || sc.M <= 0 || sc.D < 0 || (sc.D + 1) * (sc.D + 1) > sc.M || sc.D > 3)) {
    gsaj_set_error("%s: SH degree %d needs %d coefficients, got M=%d", who, sc.D, (sc.D + 1) * (sc.D + 1), sc.M);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

static int sort_cap_of(int tile_list_capacity) {
  return (tile_list_capacity > 0 && tile_list_capacity < SORT_CAP) ? tile_list_capacity : SORT_CAP;
}

static FwdParams fwd_params(const Scene &sc, const Views &v, int prefiltered, const Arenas &a) {
  FwdParams p;
  p.P = sc.P; p.D = sc.D; p.M = sc.M; p.W = v.W; p.H = v.H;
  p.means3D = sc.means3D; p.shs = sc.shs; p.colors_precomp = sc.colors_precomp; p.opacities = sc.opacities;
  p.scales = sc.scales; p.rotations = sc.rotations; p.cov3D_precomp = sc.cov3D_precomp;
  p.viewmatrix = v.viewmatrix; p.projmatrix = v.projmatrix; p.campos = v.campos;
  p.scale_modifier = sc.scale_modifier; p.tanfovx = v.tanfovx; p.tanfovy = v.tanfovy;
  p.focal_y = v.H / (2.0f * v.tanfovy);
  p.focal_x = v.W / (2.0f * v.tanfovx);
  p.prefiltered = prefiltered;
  p.grid_x = (v.W + TILE - 1) / TILE; p.grid_y = (v.H + TILE - 1) / TILE;
  p.capacity = a.instances;
  p.sort_cap = sort_cap_of(a.tile_list_capacity);
  p.views = v.K;
  return p;
}

// what a backward's caller gives BwdParams directly, in the order of the ABI: radii and the twelve gradient outputs
static BwdParams grad_outputs(const int *radii, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_ddepth,
                              float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot, float *dL_dtau,
                              float *dL_dtau_sum) {
  BwdParams p{};
  p.radii = radii;
  p.dL_dmean2D = dL_dmean2D; p.dL_dconic = dL_dconic; p.dL_dopacity = dL_dopacity; p.dL_dcolor = dL_dcolor;
  p.dL_ddepth = dL_ddepth; p.dL_dmean3D = dL_dmean3D; p.dL_dcov3D = dL_dcov3D; p.dL_dsh = dL_dsh;
  p.dL_dscale = dL_dscale; p.dL_drot = dL_drot; p.dL_dtau = dL_dtau; p.dL_dtau_sum = dL_dtau_sum;
  return p;
}

// p arrives with what the caller gave it directly: the twelve gradient outputs (none for the Jacobian walk) and radii
static void bwd_params(BwdParams *p, const Scene &sc, const Views &v, const GeomWS &g) {
  p->P = sc.P; p->D = sc.D; p->M = sc.M; p->W = v.W; p->H = v.H;
  p->means3D = sc.means3D; p->shs = sc.shs; p->scales = sc.scales; p->rotations = sc.rotations;
  p->cov3Ds = sc.cov3D_precomp ? sc.cov3D_precomp : g.cov3D;
  p->viewmatrix = v.viewmatrix; p->projmatrix = v.projmatrix; p->projmatrix_raw = v.projmatrix_raw; p->campos = v.campos;
  p->scale_modifier = sc.scale_modifier; p->tanfovx = v.tanfovx; p->tanfovy = v.tanfovy;
  p->focal_y = v.H / (2.0f * v.tanfovy);
  p->focal_x = v.W / (2.0f * v.tanfovx);
  p->grid_x = (v.W + TILE - 1) / TILE; p->grid_y = (v.H + TILE - 1) / TILE;
  if (!p->radii) p->radii = g.internal_radii;
}

// the loss arguments as the entry points name them (the backward forms add the forward's images themselves)
static FusedLoss loss_args(int loss_flags, float alpha, float rgb_boundary_threshold, const float *gt_color, const float *gt_depth,
                           const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, int exposure_stride = 1) {
  FusedLoss fl{};
  fl.flags = loss_flags; fl.alpha = alpha; fl.rgb_thr = rgb_boundary_threshold;
  fl.gt_color = gt_color; fl.gt_depth = gt_depth; fl.grad_mask = grad_mask; fl.exp_a = exposure_a; fl.exp_b = exposure_b;
  fl.exp_stride = exposure_stride;
  return fl;
}

// fl arrives with the caller's loss arguments as given (K: the views of a batched call).  They are checked, before anything is
// launched; then the pointers the flags rule out are nulled, so that the kernels' per-view shifts (fused_loss_view) leave them alone.
// No kernel reads them in those cases: gt_depth and depth are read behind `L.mono ? 0.f : ...` only, and exp_a / exp_b in
// loss_consts behind GSAJ_LOSS_NO_EXPOSURE only (loss_terms.h).
static int fused_loss(const char *who, FusedLoss *fl, int K = 1) {
  if (K <= 0) {
    gsaj_set_error("%s: invalid argument (K=%d)", who, K);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const bool mono = fl->flags & GSAJ_LOSS_MONOCULAR, noexp = fl->flags & GSAJ_LOSS_NO_EXPOSURE;
  if ((fl->flags & GSAJ_LOSS_COMPUTE_LOSS) || !fl->gt_color || (!mono && !fl->gt_depth) || (!noexp && (!fl->exp_a || !fl->exp_b)) ||
      fl->exp_stride < 1) {
    gsaj_set_error("%s: invalid loss arguments (flags=%d, exposure stride %d; GSAJ_LOSS_COMPUTE_LOSS has no fused form)", who, fl->flags,
                   fl->exp_stride);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (mono) fl->gt_depth = fl->depth = nullptr;
  if (noexp) fl->exp_a = fl->exp_b = nullptr;
  return GSAJ_OK;
}

// the backward forms of the fused loss read the images the forward wrote
static int check_loss_images(const char *who, const FusedLoss &fl) {
  if (!fl.color || !fl.opacity || (!(fl.flags & GSAJ_LOSS_MONOCULAR) && !fl.depth)) {
    gsaj_set_error("%s: the forward's color / depth / opacity images are required", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

// the forward forms of the fused loss write these
static int check_loss_outputs(const char *who, const FwdOut &o, const void *loss_ws) {
  if (!o.scalars || !loss_ws) {
    gsaj_set_error("%s: out_scalars and loss_ws are required", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// checks, carve (all three workspaces, for whoever goes on) and the per-Gaussian kernels of one frame
static int preprocess_frame(const Scene &sc, const Views &v, int prefiltered, const FwdOut &o, const Arenas &a, Carved *c,
                            hipStream_t s) {
  if (sc.P <= 0 || v.W <= 0 || v.H <= 0 || !sc.means3D || !sc.opacities || !v.viewmatrix || !v.projmatrix || !a.geom || !a.image ||
      !o.n_touched) {
    gsaj_set_error("gsaj_forward_preprocess: invalid argument (P=%d W=%d H=%d)", sc.P, v.W, v.H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  int rc = check_scene("gsaj_forward_preprocess", sc, v.campos);
  if (rc != GSAJ_OK) return rc;
  carve(a, sc.P, v.W, v.H, 0, c);
  return launch_preprocess(fwd_params(sc, v, prefiltered, a), o.radii ? o.radii : c->g.internal_radii, o.n_touched, c->g, c->im, c->vs, s);
}

// tile binning, the compositor and (fl != NULL) the loss sums of v.K carved frames
static int composite(int P, const Views &v, int sort_cap, int flags, const FwdOut &o, const Carved &c, const FusedLoss *fl, hipStream_t s) {
  const int gx = (v.W + TILE - 1) / TILE, gy = (v.H + TILE - 1) / TILE;
  int rc = launch_tile_binning(P, sort_cap, (flags & GSAJ_FWD_RECORDS_FP16) ? 1 : 0, gx, gy, c.g, c.b, c.im, v.K, c.vs, s);
  if (rc != GSAJ_OK) return rc;
  rc = launch_render_forward(P, v.W, v.H, gx, gy, v.bg, c.g, c.b, c.im, o.color, o.depth, o.opacity, o.n_touched, v.K, c.vs, s, fl);
  if (rc != GSAJ_OK || !fl) return rc;
  return launch_loss_finalize(*fl, gsaj_fwd_loss_slots(v.W, v.H), v.W, v.H, c.im.counters + 4, o.scalars, s, v.K, c.vs.image, o.dexposure);
}

int gsaj_forward_preprocess(int P, int D, int M, int W, int H, const float *means3D, const float *shs,
                            const float *colors_precomp, const float *opacities, const float *scales,
                            float scale_modifier, const float *rotations, const float *cov3D_precomp,
                            const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                            float tanfovy, int prefiltered, int *radii, int *n_touched, void *geom_ws, void *image_ws,
                            void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, nullptr, W, H, viewmatrix, projmatrix, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{nullptr, nullptr, nullptr, radii, n_touched, nullptr, nullptr};
  Carved c;
  return preprocess_frame(sc, v, prefiltered, o, Arenas{geom_ws, nullptr, 0, 0, 0, image_ws}, &c, (hipStream_t)stream);
}

int gsaj_forward_preprocess_cap(int P, int D, int M, int W, int H, const float *means3D, const float *shs,
                                const float *colors_precomp, const float *opacities, const float *scales,
                                float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                                float tanfovy, int prefiltered, int *radii, int *n_touched, void *geom_ws, void *image_ws,
                                int capacity, int tile_list_capacity, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, nullptr, W, H, viewmatrix, projmatrix, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{nullptr, nullptr, nullptr, radii, n_touched, nullptr, nullptr};
  Carved c;
  return preprocess_frame(sc, v, prefiltered, o, Arenas{geom_ws, nullptr, 0, capacity, tile_list_capacity, image_ws}, &c,
                          (hipStream_t)stream);
}

int gsaj_forward_num_rendered(int W, int H, const void *image_ws, void *stream, int *num_rendered, int *max_tile_list) {
  if (W <= 0 || H <= 0 || !image_ws || !num_rendered) {
    gsaj_set_error("gsaj_forward_num_rendered: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  ImageWS im;
  image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
  uint32_t host[4] = {0, 0, 0, 0};
  GSAJ_HIP_CHECK(hipMemcpyAsync(host, im.counters, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *num_rendered = (int)host[0];
  if (max_tile_list) *max_tile_list = (int)host[2];
  if (host[1] & ERR_PREFILTERED) {
    gsaj_set_error("Point is filtered although prefiltered is set. This shouldn't happen!");
    return GSAJ_ERR_PREFILTERED_CULLED;
  }
  if (host[1] & ERR_INTERNAL) {
    gsaj_set_error("internal error: tile histogram total != instance total");
    return GSAJ_ERR_HIP;
  }
  if (host[1] & ERR_CAPACITY) {
    gsaj_set_error("async forward aborted: binning arena too small (R=%u, longest tile list=%u)", host[0], host[2]);
    return GSAJ_ERR_WORKSPACE_TOO_SMALL;
  }
  return GSAJ_OK;
}

int gsaj_forward_aborted_count(int W, int H, void *image_ws, void *stream, int *count) {
  if (W <= 0 || H <= 0 || !image_ws || !count) {
    gsaj_set_error("gsaj_forward_aborted_count: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  ImageWS im;
  image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
  uint32_t host = 0;
  GSAJ_HIP_CHECK(hipMemcpyAsync(&host, im.sticky, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *count = (int)host;
  // read and clear: the next call reports the aborts since this one (a caller that re-sized its arena starts from zero)
  if (host) GSAJ_HIP_CHECK(hipMemsetAsync(im.sticky, 0, sizeof(uint32_t), (hipStream_t)stream));
  return GSAJ_OK;
}

const uint32_t *gsaj_forward_abort_flag(int W, int H, void *image_ws) {
  if (W <= 0 || H <= 0 || !image_ws) {
    gsaj_set_error("gsaj_forward_abort_flag: invalid argument");
    return nullptr;
  }
  ImageWS im;
  image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
  return im.counters + 4;
}

int gsaj_set_tile_band(int W, int H, void *image_ws, int tile_row_begin, int tile_row_end, void *stream) {
  const int gy = (H + TILE - 1) / TILE;
  if (W <= 0 || H <= 0 || !image_ws || tile_row_begin < 0 || tile_row_end < tile_row_begin || tile_row_end > gy || gy > 0xffff) {
    gsaj_set_error("gsaj_set_tile_band: rows [%d, %d) are not a band of the %d tile rows of a %dx%d frame", tile_row_begin,
                   tile_row_end, gy, W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  ImageWS im;
  image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
  // 0 = the whole frame; an empty band [b, b) with b > 0 is kept as such (the rank renders nothing); [0, 0) cannot be
  // told from "whole frame" and is refused
  const bool whole = tile_row_begin == 0 && tile_row_end == gy;
  if (!whole && tile_row_end == 0) {
    gsaj_set_error("gsaj_set_tile_band: the empty band [0, 0) cannot be expressed; give an empty band as [b, b) with b > 0");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const uint32_t band = whole ? 0u : ((uint32_t)tile_row_begin | ((uint32_t)tile_row_end << 16));
  GSAJ_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(im.sticky + 1), (int)band, 1, (hipStream_t)stream));
  GSAJ_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(im.sticky + 2), (int)~band, 1, (hipStream_t)stream));
  return GSAJ_OK;
}

// the synchronous second half: the arena is carved for the R the caller read back
static int render_frame(int P, const Views &v, int max_tile_list, int flags, const FwdOut &o, const Arenas &a, hipStream_t s) {
  const int R = a.instances;
  if (P <= 0 || R < 0 || v.W <= 0 || v.H <= 0 || !v.bg || !a.geom || !a.binning || !a.image || !o.color || !o.depth ||
      !o.opacity || !o.n_touched) {
    gsaj_set_error("gsaj_forward_render: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const size_t need = gsaj_binning_workspace_bytes(R);
  if (a.binning_bytes < need) {
    gsaj_set_error("binning workspace too small: have %zu bytes, need %zu for R=%d", a.binning_bytes, need, R);
    return GSAJ_ERR_WORKSPACE_TOO_SMALL;
  }
  Carved c;
  carve(a, P, v.W, v.H, 0, &c);
  // per-tile lists sorted by the tile's workgroup: in one LDS pass when the list fits the capacity sized from max_tile_list,
  // in LDS-sized chunks + merge passes when it does not (max_tile_list < 0 forces that path with the smallest capacity)
  const int sort_cap = max_tile_list < 0 ? 128 : (max_tile_list > SORT_CAP ? SORT_CAP : max_tile_list);
  return composite(P, v, sort_cap, flags, o, c, nullptr, s);
}

int gsaj_forward_render(int P, int R, int max_tile_list, int W, int H, const float *bg, const float *colors_precomp,
                        const int *radii,
                        void *geom_ws, void *binning_ws, size_t binning_ws_bytes, void *image_ws, float *out_color,
                        float *out_depth, float *out_opacity, int *n_touched, int flags, void *stream) {
  (void)colors_precomp;  // (already in the splat rows: gsaj_forward_preprocess)
  (void)radii;
  const Views v{1, bg, W, H, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f};
  const FwdOut o{out_color, out_depth, out_opacity, nullptr, n_touched, nullptr, nullptr};
  return render_frame(P, v, max_tile_list, flags, o, Arenas{geom_ws, binning_ws, binning_ws_bytes, R, 0, image_ws}, (hipStream_t)stream);
}

int gsaj_rasterize_forward(int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                           const float *colors_precomp, const float *opacities, const float *scales,
                           float scale_modifier, const float *rotations, const float *cov3D_precomp,
                           const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                           float tanfovy, int prefiltered, float *out_color, float *out_depth, float *out_opacity,
                           int *radii, int *n_touched, void *geom_ws, void *binning_ws, size_t binning_ws_bytes,
                           void *image_ws, int *num_rendered_out, int flags, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{out_color, out_depth, out_opacity, radii, n_touched, nullptr, nullptr};
  Arenas a{geom_ws, binning_ws, binning_ws_bytes, 0, 0, image_ws};
  Carved c;
  int rc = preprocess_frame(sc, v, prefiltered, o, a, &c, (hipStream_t)stream);
  if (rc != GSAJ_OK) return rc;
  int max_tile = 0;
  rc = gsaj_forward_num_rendered(W, H, image_ws, stream, &a.instances, &max_tile);
  if (num_rendered_out) *num_rendered_out = a.instances;
  if (rc != GSAJ_OK) return rc;
  rc = render_frame(P, v, max_tile, flags, o, a, (hipStream_t)stream);
  return rc == GSAJ_OK ? a.instances : rc;
}

// fl != NULL: the loss-fused form (partials = the aligned loss workspace)
static int forward_async(const Scene &sc, const Views &v, int prefiltered, int flags, const FwdOut &o, const Arenas &a,
                         const FusedLoss *fl, hipStream_t s) {
  if (a.instances <= 0 || !a.binning || !v.bg || !o.color || !o.depth || !o.opacity || !o.n_touched) {
    gsaj_set_error("gsaj_rasterize_forward_async: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (a.binning_bytes < gsaj_binning_workspace_bytes(a.instances)) {
    gsaj_set_error("binning workspace smaller than gsaj_binning_workspace_bytes(capacity=%d)", a.instances);
    return GSAJ_ERR_WORKSPACE_TOO_SMALL;
  }
  Carved c;
  int rc = preprocess_frame(sc, v, prefiltered, o, a, &c, s);
  if (rc != GSAJ_OK) return rc;
  // No host round trip: grids do not depend on R, the arena is carved for `capacity` instances, and
  // k_scan aborts the frame on the device if R or a tile list does not fit (gsaj_forward_num_rendered
  // reports it whenever the caller chooses to look).
  return composite(sc.P, v, sort_cap_of(a.tile_list_capacity), flags, o, c, fl, s);
}

int gsaj_rasterize_forward_async(int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *opacities, const float *scales,
                                 float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                 const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                                 float tanfovy, int prefiltered, float *out_color, float *out_depth, float *out_opacity,
                                 int *radii, int *n_touched, void *geom_ws, void *binning_ws, size_t binning_ws_bytes,
                                 int capacity, int tile_list_capacity, void *image_ws, int flags, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{out_color, out_depth, out_opacity, radii, n_touched, nullptr, nullptr};
  const Arenas a{geom_ws, binning_ws, binning_ws_bytes, capacity, tile_list_capacity, image_ws};
  return forward_async(sc, v, prefiltered, flags, o, a, nullptr, (hipStream_t)stream);
}

// (one array at the aligned base, the forward's partial slots [slots][4], not rounded)
size_t gsaj_fused_loss_workspace_bytes(int W, int H) { return (size_t)gsaj_fwd_loss_slots(W, H) * 4 * sizeof(float) + 256; }

int gsaj_rasterize_forward_loss(int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                                const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                const float *projmatrix, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                                float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched, void *geom_ws,
                                void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity, void *image_ws,
                                int flags, int loss_flags, float alpha, float rgb_boundary_threshold, const float *gt_color,
                                const float *gt_depth, const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                float *out_scalars, void *loss_ws, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{out_color, out_depth, out_opacity, radii, n_touched, out_scalars, nullptr};
  const Arenas a{geom_ws, binning_ws, binning_ws_bytes, capacity, tile_list_capacity, image_ws};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b);
  int rc = fused_loss("gsaj_rasterize_forward_loss", &fl);
  if (rc != GSAJ_OK) return rc;
  if ((rc = check_loss_outputs("gsaj_rasterize_forward_loss", o, loss_ws)) != GSAJ_OK) return rc;
  fl.partials = reinterpret_cast<float *>(align_base(loss_ws));
  return forward_async(sc, v, prefiltered, flags, o, a, &fl, (hipStream_t)stream);
}

// ---- batched multi-view entry points: K views of ONE Gaussian map (a mapping window) --------------------------------
// fl != NULL: the loss-fused form (view 0's pointers; partials = the aligned loss workspace)
static int forward_batch(const Scene &sc, const Views &v, int prefiltered, int flags, const FwdOut &o, const Arenas &a,
                         const FusedLoss *fl, hipStream_t s) {
  if (v.K <= 0 || sc.P <= 0 || v.W <= 0 || v.H <= 0 || a.instances <= 0 || !sc.means3D || !sc.opacities || !v.viewmatrix ||
      !v.projmatrix || !v.bg || !o.color || !o.depth || !o.opacity || !o.radii || !o.n_touched || !a.geom || !a.binning || !a.image) {
    gsaj_set_error("gsaj_rasterize_forward_batch: invalid argument (K=%d P=%d W=%d H=%d capacity=%d)", v.K, sc.P, v.W, v.H, a.instances);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  int rc = check_scene("gsaj_rasterize_forward_batch", sc, v.campos);
  if (rc != GSAJ_OK) return rc;
  Carved c;
  if ((rc = carve(a, sc.P, v.W, v.H, v.K, &c)) != GSAJ_OK) return rc;
  if ((rc = launch_preprocess(fwd_params(sc, v, prefiltered, a), o.radii, o.n_touched, c.g, c.im, c.vs, s)) != GSAJ_OK) return rc;
  return composite(sc.P, v, sort_cap_of(a.tile_list_capacity), flags, o, c, fl, s);
}

int gsaj_rasterize_forward_batch(int K, int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                                 const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                 const float *projmatrices, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                                 float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched, void *geom_ws,
                                 void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity, void *image_ws,
                                 int flags, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{out_color, out_depth, out_opacity, radii, n_touched, nullptr, nullptr};
  const Arenas a{geom_ws, binning_ws, binning_ws_bytes, capacity, tile_list_capacity, image_ws};
  return forward_batch(sc, v, prefiltered, flags, o, a, nullptr, (hipStream_t)stream);
}

size_t gsaj_fused_loss_batch_workspace_bytes(int K, int W, int H) {
  return (size_t)(K > 0 ? K : 0) * view_stride(gsaj_fused_loss_workspace_bytes(W, H));
}

int gsaj_rasterize_forward_loss_batch(int K, int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                                      const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                      const float *projmatrices, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                                      float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched, void *geom_ws,
                                      void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity, void *image_ws,
                                      int flags, int loss_flags, float alpha, float rgb_boundary_threshold, const float *gt_color,
                                      const float *gt_depth, const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                      int exposure_stride, float *out_scalars, float *out_dexposure, void *loss_ws, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, nullptr, campos, tanfovx, tanfovy};
  const FwdOut o{out_color, out_depth, out_opacity, radii, n_touched, out_scalars, out_dexposure};
  const Arenas a{geom_ws, binning_ws, binning_ws_bytes, capacity, tile_list_capacity, image_ws};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b, exposure_stride);
  int rc = fused_loss("gsaj_rasterize_forward_loss_batch", &fl, K);
  if (rc != GSAJ_OK) return rc;
  if ((rc = check_loss_outputs("gsaj_rasterize_forward_loss_batch", o, loss_ws)) != GSAJ_OK) return rc;
  fl.partials = reinterpret_cast<float *>(align_base(loss_ws));  // [K][slots][4], dense: K x 255 bytes of the workspace are slack
  return forward_batch(sc, v, prefiltered, flags, o, a, &fl, (hipStream_t)stream);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// k_render_bwd finds an instance's gradient row from the Gaussian's tile rectangle as k_preprocess packed it: 10 bits for x0, 10 for
// y0.  Beyond 1024 tiles a side x0 spills into y0 and the row lands elsewhere, past the arena at worst: such a call is refused here,
// behind the argument checks of the backward at hand and before it carves or launches anything.
static int check_rect_range(const Views &v) {
  if (v.W > GSAJ_BWD_MAX_SIDE || v.H > GSAJ_BWD_MAX_SIDE) {
    gsaj_set_error("backward: W=%d H=%d is above the %d pixels (%d tiles) a side that the packed tile rectangle's 10-bit fields hold",
                   v.W, v.H, GSAJ_BWD_MAX_SIDE, GSAJ_BWD_MAX_SIDE / TILE);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

static int backward_batch(BwdParams *p, const Scene &sc, const Views &v, const Arenas &a, const PixelSeeds &seeds, int flags,
                          hipStream_t s) {
  if (v.K <= 0 || sc.P <= 0 || a.instances <= 0 || v.W <= 0 || v.H <= 0 || !v.bg || !sc.means3D || !v.viewmatrix || !v.projmatrix ||
      !v.projmatrix_raw || !p->radii || !a.geom || !a.binning || !a.image || (!seeds.fl && (!seeds.dL_dpix || !seeds.dL_dpix_depth)) ||
      !p->dL_dopacity || !p->dL_dmean3D || !p->dL_dcov3D || !p->dL_dtau_sum) {
    gsaj_set_error("gsaj_rasterize_backward_batch: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((sc.shs && (!p->dL_dsh || !v.campos)) || (sc.scales && (!sc.rotations || !p->dL_dscale || !p->dL_drot)) ||
      (!sc.scales && !sc.cov3D_precomp)) {
    gsaj_set_error("gsaj_rasterize_backward_batch: missing gradient buffer for a provided input");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  int rc = check_rect_range(v);
  if (rc != GSAJ_OK) return rc;
  Carved c;
  if ((rc = carve(a, sc.P, v.W, v.H, v.K, &c)) != GSAJ_OK) return rc;
  bwd_params(p, sc, v, c.g);
  // the whole window in one call: the chain kernel sums the reverse compositor's instance rows itself (no gather launch, no gsum
  // round trip); the two halves called separately go through gsum as before
  const int fused = (flags & (GSAJ_BWD_ONLY_COMPOSITE | GSAJ_BWD_ONLY_CHAIN)) ? 0 : 1;
  if (!(flags & GSAJ_BWD_ONLY_CHAIN)) {
    rc = launch_render_backward(a.instances, v.W, v.H, p->grid_x, p->grid_y, v.bg, c.g, c.b, c.im, seeds.dL_dpix, seeds.dL_dpix_depth,
                                v.K, c.vs, s, seeds.fl);
    if (rc != GSAJ_OK) return rc;
    if (!fused && (rc = launch_gather_sums(sc.P, v.K, p->radii, c.g, c.b, c.im, c.vs, s)) != GSAJ_OK) return rc;
  }
  if (flags & GSAJ_BWD_ONLY_COMPOSITE) return GSAJ_OK;
  return launch_gaussian_backward_batch(*p, v.K, c.g, c.b, c.im, c.vs, (flags & GSAJ_BWD_ACCUMULATE) ? 1 : 0, fused, s);
}

int gsaj_rasterize_backward_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                  const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                  const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                  const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                  float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                  const float *dL_dpix, const float *dL_dpix_depth, float *dL_dmean2D, float *dL_dconic,
                                  float *dL_dopacity, float *dL_dcolor, float *dL_ddepth, float *dL_dmean3D, float *dL_dcov3D,
                                  float *dL_dsh, float *dL_dscale, float *dL_drot, float *dL_dtau, float *dL_dtau_sum, int flags,
                                  void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, capacity, 0, image_ws};
  BwdParams p = grad_outputs(radii, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                             dL_dtau, dL_dtau_sum);
  return backward_batch(&p, sc, v, a, PixelSeeds{dL_dpix, dL_dpix_depth, nullptr}, flags, (hipStream_t)stream);
}

int gsaj_rasterize_backward_loss_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                       const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                       const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                       const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                       float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws, int loss_flags,
                                       float alpha, float rgb_boundary_threshold, const float *color, const float *depth,
                                       const float *opacity, const float *gt_color, const float *gt_depth, const uint8_t *grad_mask,
                                       const float *exposure_a, const float *exposure_b, int exposure_stride, float *dL_dmean2D,
                                       float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_ddepth, float *dL_dmean3D,
                                       float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot, float *dL_dtau,
                                       float *dL_dtau_sum, int flags, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, capacity, 0, image_ws};
  FusedLoss fl{};
  if (!(flags & GSAJ_BWD_ONLY_CHAIN)) {  // (the chain half reads no image: its loss arguments are ignored)
    fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b, exposure_stride);
    fl.color = color; fl.depth = depth; fl.opacity = opacity;
    int rc = fused_loss("gsaj_rasterize_backward_loss_batch", &fl, K);
    if (rc != GSAJ_OK) return rc;
    if ((rc = check_loss_images("gsaj_rasterize_backward_loss_batch", fl)) != GSAJ_OK) return rc;
  }
  BwdParams p = grad_outputs(radii, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                             dL_dtau, dL_dtau_sum);
  return backward_batch(&p, sc, v, a, PixelSeeds{nullptr, nullptr, &fl}, flags, (hipStream_t)stream);
}

static int backward_frame(BwdParams *p, const Scene &sc, const Views &v, const Arenas &a, const PixelSeeds &seeds, hipStream_t s) {
  // pose-only mode (tracking: only the camera is optimised): every per-Gaussian output pointer NULL, dL_dtau_sum given
  const bool pose_only = !p->dL_dmean2D && !p->dL_dconic && !p->dL_dopacity && !p->dL_dcolor && !p->dL_ddepth && !p->dL_dmean3D &&
                         !p->dL_dcov3D && !p->dL_dsh && !p->dL_dscale && !p->dL_drot && p->dL_dtau_sum;
  if (sc.P <= 0 || a.instances < 0 || v.W <= 0 || v.H <= 0 || !v.bg || !sc.means3D || !v.viewmatrix || !v.projmatrix ||
      !v.projmatrix_raw || !a.geom || !a.binning || !a.image || (!seeds.fl && (!seeds.dL_dpix || !seeds.dL_dpix_depth)) ||
      (!pose_only && (!p->dL_dmean2D || !p->dL_dconic || !p->dL_dopacity || !p->dL_dcolor || !p->dL_ddepth || !p->dL_dmean3D ||
                      !p->dL_dcov3D))) {
    gsaj_set_error("gsaj_rasterize_backward: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if ((sc.shs && ((!pose_only && !p->dL_dsh) || !v.campos)) ||
      (sc.scales && (!sc.rotations || (!pose_only && (!p->dL_dscale || !p->dL_drot)))) || (!sc.scales && !sc.cov3D_precomp)) {
    gsaj_set_error("gsaj_rasterize_backward: missing gradient buffer for a provided input");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  int rc = check_rect_range(v);
  if (rc != GSAJ_OK) return rc;
  Carved c;
  carve(a, sc.P, v.W, v.H, 0, &c);
  bwd_params(p, sc, v, c.g);
  // every output row is written by the kernels (zeros for culled Gaussians): no memsets
  rc = launch_render_backward(a.instances, v.W, v.H, p->grid_x, p->grid_y, v.bg, c.g, c.b, c.im, seeds.dL_dpix, seeds.dL_dpix_depth,
                                  1, c.vs, s, seeds.fl);
  if (rc != GSAJ_OK) return rc;
  return launch_gaussian_backward(*p, c.g, c.b, c.im, s);
}

int gsaj_rasterize_backward(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                            const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                            const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                            const float *projmatrix, const float *projmatrix_raw, const float *campos, float tanfovx,
                            float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                            const float *dL_dpix, const float *dL_dpix_depth, float *dL_dmean2D, float *dL_dconic,
                            float *dL_dopacity, float *dL_dcolor, float *dL_ddepth, float *dL_dmean3D,
                            float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot, float *dL_dtau,
                            float *dL_dtau_sum, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, R, 0, image_ws};
  BwdParams p = grad_outputs(radii, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                             dL_dtau, dL_dtau_sum);
  return backward_frame(&p, sc, v, a, PixelSeeds{dL_dpix, dL_dpix_depth, nullptr}, (hipStream_t)stream);
}

int gsaj_rasterize_backward_loss(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                                 const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                 const float *projmatrix_raw, const float *campos, float tanfovx, float tanfovy, const int *radii,
                                 void *geom_ws, void *binning_ws, void *image_ws, int loss_flags, float alpha,
                                 float rgb_boundary_threshold, const float *color, const float *depth, const float *opacity,
                                 const float *gt_color, const float *gt_depth, const uint8_t *grad_mask, const float *exposure_a,
                                 const float *exposure_b, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor,
                                 float *dL_ddepth, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale,
                                 float *dL_drot, float *dL_dtau, float *dL_dtau_sum, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, R, 0, image_ws};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b);
  fl.color = color; fl.depth = depth; fl.opacity = opacity;
  int rc = fused_loss("gsaj_rasterize_backward_loss", &fl);
  if (rc != GSAJ_OK) return rc;
  if ((rc = check_loss_images("gsaj_rasterize_backward_loss", fl)) != GSAJ_OK) return rc;
  BwdParams p = grad_outputs(radii, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_ddepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
                             dL_dtau, dL_dtau_sum);
  return backward_frame(&p, sc, v, a, PixelSeeds{nullptr, nullptr, &fl}, (hipStream_t)stream);
}

// ---- Gauss-Newton tracking: per-pixel pose Jacobians and normal equations (pose_jac.hip) ------------------------------------
struct JacWS { float *rows, *partials; };  // the derivative rows | the explicit form's partial rows (the fused forms: the caller's)
static size_t jac_carve(Carver c, int P, int W, int H, JacWS *w) {
  w->rows = reinterpret_cast<float *>(c.take<char>(gsaj_jac_rows_bytes(P)));
  w->partials = c.take<float>((size_t)gsaj_jac_slots(W, H) * GSAJ_GN_PARTIAL_FLOATS);
  return c.used();
}
size_t gsaj_pose_jac_workspace_bytes(int P, int W, int H) { JacWS w; return jac_carve(Carver(nullptr, ALIGN_BASE), P, W, H, &w) + 256; }
int gsaj_pose_jac_partial_rows(int W, int H) { return gsaj_jac_slots(W, H); }

// (the batched forms keep no partial rows of their own -- the caller owns gn_partials -- so W and H do not count)
size_t gsaj_pose_jac_batch_workspace_bytes(int K, int P, int W, int H) {
  (void)W; (void)H;
  return (size_t)(K > 0 ? K : 0) * view_stride(gsaj_jac_rows_bytes(P));  // (view v's rows are v strides on: pose_jac.hip)
}

// the fused form's loss arguments (fl arrives as the caller gave them), in the order a caller is told about them
static int pose_jac_loss_args(const char *who, bool joint, FusedLoss *fl, const float *gn_partials, float irls_delta, int K) {
  int rc = fused_loss(who, fl, K);
  if (rc != GSAJ_OK) return rc;
  if (joint && ((fl->flags & GSAJ_LOSS_NO_EXPOSURE) || !fl->exp_a || !fl->exp_b)) {
    gsaj_set_error("%s: the joint form solves for the exposure: exposure_a / exposure_b are required, GSAJ_LOSS_NO_EXPOSURE is not allowed", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!fl->color || !fl->opacity || (!(fl->flags & GSAJ_LOSS_MONOCULAR) && !fl->depth) || !gn_partials || !(irls_delta >= 0.f)) {
    gsaj_set_error("%s: the forward's color / depth / opacity images, gn_partials and irls_delta >= 0 are required", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return GSAJ_OK;
}

// The five Jacobian entry points: v.K views of one map (the single forms: K = 1).  p: radii only (no gradient output).  jo: the walk's
// outputs as the caller named them; the explicit form's seed / curvature images are dropped where their sum was not asked for, and its
// partial rows live in the Jacobian workspace behind the derivative rows.  What differs between the single and the batched forms:
//   single   run behind a synchronous forward: R may be 0 and radii may be the workspace's own; every workspace is carved from the
//            aligned base of whatever the caller gave; jac_ws holds the rows, then the explicit form's partial rows (jac_carve)
//   batched  (the loss-fused forms only) a capacity > 0 and the caller's radii [K,P]; K blocks of every workspace, 256-byte aligned
//            themselves; jac_ws is K row blocks view_stride apart and nothing else (gsaj_pose_jac_batch_workspace_bytes)
static int pose_jac(const char *who, BwdParams *p, const Scene &sc, const Views &v, const Arenas &a, void *jac_ws, JacOut jo,
                    const GnSums &gn, bool batched, hipStream_t s) {
  int rc = gn.fl ? pose_jac_loss_args(who, gn.joint, gn.fl, jo.partials, jo.delta, v.K) : GSAJ_OK;
  if (rc != GSAJ_OK) return rc;
  if (sc.P <= 0 || (batched ? a.instances <= 0 || !p->radii : a.instances < 0) || v.W <= 0 || v.H <= 0 || !v.bg || !sc.means3D ||
      !v.viewmatrix || !v.projmatrix || !v.projmatrix_raw || !a.geom || !a.binning || !a.image || !jac_ws || (sc.shs && !v.campos) ||
      (sc.scales && !sc.rotations) || (!sc.scales && !sc.cov3D_precomp)) {
    gsaj_set_error("%s: invalid argument", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  if (!gn.fl && ((gn.g_out && (!jo.seed_c || !jo.seed_d)) || (gn.H_out && (!jo.curv_c || !jo.curv_d)))) {
    gsaj_set_error("%s: g_out needs both seed images, H_out both curvature images", who);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  Carved c;
  if ((rc = carve(a, sc.P, v.W, v.H, batched ? v.K : 0, &c)) != GSAJ_OK) return rc;
  if (batched && ((uintptr_t)jac_ws & 255)) {
    gsaj_set_error("batched entry points need 256-byte aligned workspaces");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  bwd_params(p, sc, v, c.g);  // (cov3Ds: the caller's, or view 0's geometry block -- the only one a batched forward writes)
  JacWS w;  // (batched: jac_ws is aligned, so w.rows is the first of the K row blocks; w.partials is not used)
  jac_carve(Carver(jac_ws, ALIGN_BASE), sc.P, v.W, v.H, &w);
  const size_t rows_stride = view_stride(gsaj_jac_rows_bytes(sc.P));
  rc = launch_splat_jac(*p, v.K, c.g, c.im, w.rows, c.vs, rows_stride, s);
  if (rc != GSAJ_OK) return rc;
  const bool sums = gn.fl || gn.H_out || gn.g_out;
  if (!gn.g_out) jo.seed_c = jo.seed_d = nullptr;
  if (!gn.H_out) jo.curv_c = jo.curv_d = nullptr;
  if (!gn.fl) jo.partials = sums ? w.partials : nullptr;
  rc = launch_render_jac(*p, v.K, v.bg, c, w.rows, rows_stride, jo, gn.fl, gn.joint ? 1 : 0, s);
  if (rc != GSAJ_OK || gn.fl || !sums) return rc;
  return launch_gn_reduce(jo.partials, gsaj_jac_slots(v.W, v.H), c.im, gn.H_out, gn.g_out, s);
}

int gsaj_rasterize_pose_jacobian(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                                 const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                 const float *projmatrix_raw, const float *campos, float tanfovx, float tanfovy, const int *radii,
                                 void *geom_ws, void *binning_ws, void *image_ws, void *jac_ws, float *jac_out, float *out_color,
                                 float *out_depth, float *H_out, float *g_out, const float *seed_color, const float *seed_depth,
                                 const float *curv_color, const float *curv_depth, void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, R, 0, image_ws};
  const JacOut jo{jac_out, out_color, out_depth, seed_color, seed_depth, curv_color, curv_depth, nullptr, 0.f};
  BwdParams p{};
  p.radii = radii;
  return pose_jac("gsaj_rasterize_pose_jacobian", &p, sc, v, a, jac_ws, jo, GnSums{H_out, g_out, nullptr, false}, false, (hipStream_t)stream);
}

int gsaj_rasterize_pose_jacobian_loss(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                                      const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                      const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                      const float *projmatrix, const float *projmatrix_raw, const float *campos, float tanfovx,
                                      float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                      void *jac_ws, int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                      const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                      const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float irls_delta,
                                      float *gn_partials, float *jac_out, void *stream) {
  const char *who = "gsaj_rasterize_pose_jacobian_loss";
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, R, 0, image_ws};
  const JacOut jo{jac_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gn_partials, irls_delta};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b);
  fl.color = color; fl.depth = depth; fl.opacity = opacity;
  BwdParams p{};
  p.radii = radii;
  return pose_jac(who, &p, sc, v, a, jac_ws, jo, GnSums{nullptr, nullptr, &fl, false}, false, (hipStream_t)stream);
}

int gsaj_rasterize_pose_jacobian_loss8(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                                       const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                       const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                       const float *projmatrix, const float *projmatrix_raw, const float *campos, float tanfovx,
                                       float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                       void *jac_ws, int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                       const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                       const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float irls_delta,
                                       float *gn8_partials, float *jac_out, void *stream) {
  const char *who = "gsaj_rasterize_pose_jacobian_loss8";
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{1, bg, W, H, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, R, 0, image_ws};
  const JacOut jo{jac_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gn8_partials, irls_delta};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b);
  fl.color = color; fl.depth = depth; fl.opacity = opacity;
  BwdParams p{};
  p.radii = radii;
  return pose_jac(who, &p, sc, v, a, jac_ws, jo, GnSums{nullptr, nullptr, &fl, true}, false, (hipStream_t)stream);
}

// ---- the same for K views of one map: gridDim.y = K, K consecutive blocks of every workspace (the loss-fused forms only) ----------
int gsaj_rasterize_pose_jacobian_loss_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                            const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                            const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                            const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                            float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                            int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                            const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                            const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                            int exposure_stride, void *jac_ws, float irls_delta, float *gn_partials, float *jac_out,
                                            void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, capacity, 0, image_ws};
  const JacOut jo{jac_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gn_partials, irls_delta};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b, exposure_stride);
  fl.color = color; fl.depth = depth; fl.opacity = opacity;
  BwdParams p{};
  p.radii = radii;
  return pose_jac("gsaj_rasterize_pose_jacobian_loss_batch", &p, sc, v, a, jac_ws, jo, GnSums{nullptr, nullptr, &fl, false}, true,
                  (hipStream_t)stream);
}

int gsaj_rasterize_pose_jacobian_loss8_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                             const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                             const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                             const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                             float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                             int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                             const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                             const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                             int exposure_stride, void *jac_ws, float irls_delta, float *gn8_partials, float *jac_out,
                                             void *stream) {
  const Scene sc{P, D, M, means3D, shs, colors_precomp, nullptr, scales, scale_modifier, rotations, cov3D_precomp};
  const Views v{K, bg, W, H, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy};
  const Arenas a{geom_ws, binning_ws, SIZE_NOT_GIVEN, capacity, 0, image_ws};
  const JacOut jo{jac_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gn8_partials, irls_delta};
  FusedLoss fl = loss_args(loss_flags, alpha, rgb_boundary_threshold, gt_color, gt_depth, grad_mask, exposure_a, exposure_b, exposure_stride);
  fl.color = color; fl.depth = depth; fl.opacity = opacity;
  BwdParams p{};
  p.radii = radii;
  return pose_jac("gsaj_rasterize_pose_jacobian_loss8_batch", &p, sc, v, a, jac_ws, jo, GnSums{nullptr, nullptr, &fl, true}, true,
                  (hipStream_t)stream);
}

int gsaj_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present,
                      void *stream) {
  (void)projmatrix;  // the reference's test only uses the view-space depth (auxiliary.h:154)
  if (P <= 0 || !means3D || !viewmatrix || !present) {
    gsaj_set_error("gsaj_mark_visible: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  return launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
}

int gsaj_debug_export(int P, int R, int W, int H, const void *geom_ws, const void *binning_ws, const void *image_ws,
                      float *means2D, float *depths, float *cov3D, float *conic_opacity, float *rgb, uint8_t *clamped,
                      uint32_t *tiles_touched, uint32_t *point_list, uint32_t *ranges, float *final_T,
                      uint32_t *n_contrib, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const size_t Pz = (size_t)P, N = (size_t)W * H;
  const size_t tiles = (size_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
#define CP(dst, src, bytes) \
  if (dst) GSAJ_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s))
  if (geom_ws) {
    GeomWS g;
    geom_carve(Carver(geom_ws, ALIGN_BASE), Pz, &g);
    // means2D, conic_opacity, rgb live in the 48-byte splat rows only: strided copies
#define CP2D(dst, src, width) \
  if (dst) GSAJ_HIP_CHECK(hipMemcpy2DAsync(dst, width, src, sizeof(float4) * REC_F4, width, Pz, hipMemcpyDeviceToDevice, s))
    CP2D(means2D, g.splat, sizeof(float2));
    CP2D(conic_opacity, g.splat + 1, sizeof(float4));
    CP2D(rgb, g.splat + 2, sizeof(float) * 3);
#undef CP2D
    CP(depths, g.depths, sizeof(float) * Pz);
    CP(cov3D, g.cov3D, sizeof(float) * 6 * Pz);
    CP(clamped, g.clamped, 3 * Pz);
    CP(tiles_touched, g.tiles_touched, sizeof(uint32_t) * Pz);
  }
  if (binning_ws && R > 0) {
    BinWS b;
    bin_carve(Carver(binning_ws, ALIGN_BASE), (size_t)R, &b);
    CP(point_list, b.point_list, sizeof(uint32_t) * (size_t)R);
  }
  if (image_ws) {
    ImageWS im;
    image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
    CP(ranges, im.ranges, sizeof(uint2) * tiles);
    CP(final_T, im.final_T, sizeof(float) * N);
    CP(n_contrib, im.n_contrib, sizeof(uint32_t) * N);
  }
#undef CP
  return GSAJ_OK;
}

int gsaj_debug_launch_plan(int P, int views, int W, int H, int *plan) {
  if (P <= 0 || views <= 0 || W <= 0 || H <= 0 || !plan) {
    gsaj_set_error("gsaj_debug_launch_plan: invalid argument (P=%d views=%d W=%d H=%d)", P, views, W, H);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;  // (as fwd_params and composite form them)
  const PreprocessPlan pre = plan_preprocess(P, views, gx, gy);
  const ScatterPlan sc = plan_scatter(P, views, gx, gy);
  plan[GSAJ_PLAN_BPW] = pre.bpw;
  plan[GSAJ_PLAN_PRE_WORKGROUPS] = pre.workgroups;
  plan[GSAJ_PLAN_HIST_LDS] = pre.hist_lds ? 1 : 0;
  plan[GSAJ_PLAN_GPT] = sc.gpt;
  plan[GSAJ_PLAN_SCAT_WORKGROUPS] = sc.workgroups;
  plan[GSAJ_PLAN_SCAT_LDS] = sc.counters_lds ? 1 : 0;
  return GSAJ_OK;
}

int gsaj_debug_lds_budget(int P, int views, int W, int H, int M, int tile_list_capacity, int stereo_W, int stereo_D, int *budget) {
  LdsRequest stereo;
  if (P <= 0 || views <= 0 || W <= 0 || H <= 0 || M < 0 || tile_list_capacity < 0 || !budget ||
      !lds_stereo_winner(stereo_W, stereo_D, &stereo)) {
    gsaj_set_error("gsaj_debug_lds_budget: invalid argument (P=%d views=%d W=%d H=%d M=%d tile_list_capacity=%d stereo_W=%d stereo_D=%d)",
                   P, views, W, H, M, tile_list_capacity, stereo_W, stereo_D);
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;  // (as fwd_params and composite form them)
  const PreprocessPlan pre = plan_preprocess(P, views, gx, gy);
  const ScatterPlan sc = plan_scatter(P, views, gx, gy);
  const SortPlan sp = plan_tile_sort(sort_cap_of(tile_list_capacity));  // (as the asynchronous forwards: 0 is SORT_CAP keys)
  auto put = [&](int launch, const LdsRequest &r) {
    int *row = budget + launch * GSAJ_LDS_FIELDS;
    row[GSAJ_LDS_DYNAMIC] = (int)r.dynamic_bytes;
    row[GSAJ_LDS_STATIC] = (int)r.static_bytes;
    row[GSAJ_LDS_LIMIT] = (int)r.limit_bytes;
    row[GSAJ_LDS_VARIANT] = r.variant;
  };
  put(GSAJ_LDS_PREPROCESS, lds_preprocess(pre, gx, gy, M == 16));
  put(GSAJ_LDS_FRAME_SCAN, lds_frame_scan(pre, gx, gy));
  put(GSAJ_LDS_SCATTER, lds_scatter(sc, gx, gy));
  put(GSAJ_LDS_TILE_SORT, sp.lds[0]);
  put(GSAJ_LDS_TILE_SORT_2, sp.lds[1]);
  put(GSAJ_LDS_GAUSSIAN_BWD, lds_gaussian_bwd(M, M > 0));
  put(GSAJ_LDS_STEREO_WINNER, stereo);
  return GSAJ_OK;
}

int gsaj_debug_export_taken(int R, int W, int H, const void *binning_ws, const void *image_ws, uint32_t *taken, uint8_t *reached,
                            void *stream) {
  if (R <= 0 || W <= 0 || H <= 0 || !binning_ws || !image_ws) {
    gsaj_set_error("gsaj_debug_export_taken: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  hipStream_t s = (hipStream_t)stream;
  BinWS b;
  bin_carve(Carver(binning_ws, ALIGN_BASE), (size_t)R, &b);
  ImageWS im;
  image_carve(Carver(image_ws, ALIGN_BASE), W, H, &im);
  if (reached) GSAJ_HIP_CHECK(hipMemcpyAsync(reached, b.reached, (size_t)R, hipMemcpyDeviceToDevice, s));
  if (taken) return launch_export_taken(W, H, (W + TILE - 1) / TILE, (H + TILE - 1) / TILE, b, im, taken, s);
  return GSAJ_OK;
}

// (valid only while gsum holds the view's sums: after a GSAJ_BWD_ONLY_COMPOSITE call; a whole-window backward does not write gsum)
int gsaj_debug_export_view_sums(int P, const void *geom_ws, float *sums, void *stream) {
  if (P <= 0 || !geom_ws || !sums) {
    gsaj_set_error("gsaj_debug_export_view_sums: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  GeomWS g;
  geom_carve(Carver(geom_ws, ALIGN_BASE), (size_t)P, &g);
  GSAJ_HIP_CHECK(hipMemcpyAsync(sums, g.gsum, sizeof(float4) * 3 * (size_t)P, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GSAJ_OK;
}

int gsaj_debug_export_view_sums_gather(int P, int capacity, int W, int H, void *geom_ws, void *binning_ws, void *image_ws, float *sums,
                                       void *stream) {
  if (P <= 0 || capacity <= 0 || W <= 0 || H <= 0 || !geom_ws || !binning_ws || !image_ws || !sums) {
    gsaj_set_error("gsaj_debug_export_view_sums_gather: invalid argument");
    return GSAJ_ERR_INVALID_ARGUMENT;
  }
  Carved c;
  int rc = carve(Arenas{geom_ws, binning_ws, SIZE_NOT_GIVEN, capacity, 0, image_ws}, P, W, H, 1, &c);
  if (rc != GSAJ_OK) return rc;
  if ((rc = launch_gather_sums(P, 1, nullptr, c.g, c.b, c.im, c.vs, (hipStream_t)stream)) != GSAJ_OK) return rc;
  GSAJ_HIP_CHECK(hipMemcpyAsync(sums, c.g.gsum, sizeof(float4) * 3 * (size_t)P, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GSAJ_OK;
}

}  // extern "C"
