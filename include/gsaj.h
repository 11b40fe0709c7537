/*
 * gsaj.h -- C ABI of libgsaj_hip.so: MI355X (gfx950) Gaussian-splat rasteriser with
 * analytical pose Jacobians.
 *
 * These entry points are what the reference's Python binding for this path would bind in
 * place of its pybind/CUDA layer (paths relative to the reference repository):
 *
 *   gsaj_rasterize_forward  / gsaj_forward_*   <- CudaRasterizer::Rasterizer::forward
 *        submodules/diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:33-58,
 *        called from rasterize_points.cu:36-130 (RasterizeGaussiansCUDA)
 *   gsaj_rasterize_backward                    <- CudaRasterizer::Rasterizer::backward
 *        rasterizer.h:60-91, called from rasterize_points.cu:132-223
 *   gsaj_mark_visible                          <- CudaRasterizer::Rasterizer::markVisible
 *        rasterizer.h:24-31, rasterize_points.cu:225-246
 *   gsaj_*_workspace_bytes                     <- required<GeometryState/ImageState/BinningState>()
 *        rasterizer_impl.h:21-72 (the std::function<char*(size_t)> resize callbacks of
 *        rasterize_points.cu:27-33 become size queries + caller-owned buffers)
 *   gsaj_dense_* / gsaj_pose_jacobians         <- the CPU/NumPy analytic path
 *        Loss_Derivative_script_compare.py:1173-1351 (compute_gradients_2D_vectorized_chunked),
 *        :633-760 (GetAnalyticalJcobian, compute_analytical_jacobians_all_gaussians),
 *        :1587-1695 (dL/dtau assembly)
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer; fp32, contiguous, caller-owned.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  All work is
 *     enqueued asynchronously on it; the only host synchronisation is the 4-byte read of
 *     the instance count in gsaj_forward_num_rendered / gsaj_rasterize_forward
 *     (the reference has the same one, rasterizer_impl.cu:331).
 *   - viewmatrix / projmatrix / projmatrix_raw are 16 floats = the transposed 4x4 tensors
 *     the reference hands over (W2C^T, (P W2C)^T, P^T), i.e. column-major W2C / P W2C / P.
 *   - return value: >= 0 on success (gsaj_rasterize_forward returns num_rendered),
 *     a negative GSAJ_ERR_* on failure; gsaj_last_error() describes the last failure of
 *     the calling thread.
 *   - the caller need not zero anything: every output row is written by the kernels (zeros for
 *     culled Gaussians), where the reference's binding zero-fills first (rasterize_points.cu:84-88,175-185).
 */
#ifndef GSAJ_H_INCLUDED
#define GSAJ_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSAJ_OK 0
#define GSAJ_ERR_INVALID_ARGUMENT (-1)   /* bad shape / null pointer / bad combination */
#define GSAJ_ERR_HIP (-2)                /* a HIP runtime call failed */
#define GSAJ_ERR_WORKSPACE_TOO_SMALL (-3) /* binning workspace smaller than gsaj_binning_workspace_bytes(R) */
#define GSAJ_ERR_PREFILTERED_CULLED (-4) /* prefiltered=1 but a point failed the frustum test (auxiliary.h:156-160) */

#define GSAJ_TILE 16         /* BLOCK_X = BLOCK_Y of config.h:15-17 */
#define GSAJ_NUM_CHANNELS 3  /* NUM_CHANNELS of config.h */

const char *gsaj_last_error(void);
int gsaj_version(void);

/* ---- workspace sizes (bytes) -------------------------------------------------------- */
/* The memory contract of every workspace (tests/test_gpu_memory_contracts.py runs each entry point on poisoned memory behind guard
 * bands and holds it to these lines): a call writes nothing outside its outputs and the stated number of workspace bytes, and a
 * workspace is either "no initialisation needed" -- it may hold any bytes, a smaller problem may follow a larger one in it -- or
 * "zeroed once" by the caller when allocated and from then on only handed back to the same entry point at the same size: the words
 * that need the zero (tickets, sticky counters) are put back by the call that used them.
 * geom_ws: gsaj_geom_workspace_bytes(P) bytes, no initialisation needed. */
size_t gsaj_geom_workspace_bytes(int P);
/* image_ws: gsaj_image_workspace_bytes(W, H) bytes, zeroed once (the sticky abort counter, the frame counters and the tile band). */
size_t gsaj_image_workspace_bytes(int W, int H);
/* The binning workspace holds, per instance (one Gaussian in one tile's list): two 8-byte sort keys, the 4-byte list entry, a
 * 48-byte partial-gradient row with its one-byte `reached` flag, and a 4-byte `taken` word -- one byte per 8x8 pixel quadrant of
 * the tile, set by the forward compositor when some pixel of the quadrant composited the entry.  The reverse compositor stages only
 * entries taken by some quadrant, and keeps their compacted list in the (by then idle) first sort-key buffer.
 * binning_ws: gsaj_binning_workspace_bytes(R) bytes, no initialisation needed (every forward clears the flags it reads). */
size_t gsaj_binning_workspace_bytes(int R);

/* ---- per-call flags of the forward entry points (the library keeps NO process-wide mode: two threads may render
 * frames of different formats on different streams at the same time) ---------------------------------------------
 * GSAJ_FWD_RECORDS_FP16: the compositors of THIS frame read 32-byte per-Gaussian splat rows with conic, opacity and colour
 * rounded to half once (positions, depth, every accumulation and every gradient stay fp32) -- BASELINE config 5,
 * "fp16 splat with fp32 Jacobian accumulation"; integer outputs (radii, lists, ranges) are unchanged, images /
 * gradients move by ~1e-3 relative.  Default: 48-byte fp32 rows.  The format is latched in the frame's image
 * workspace, where the matching backward reads it.  (The name is historical: up to round 2 the rows were per-instance
 * records; since the compositors gather per-Gaussian rows the mode saves 16 of 48 bytes per GAUSSIAN, which no longer
 * buys time on MI355X -- see DESIGN.md section 5.) */
#define GSAJ_FWD_RECORDS_FP16 1

/* ---- forward, two-phase form --------------------------------------------------------- */
/* Phase A: per-Gaussian projection (cov3D, EWA cov2D + 0.3, conic, radius, tile rect,
 * SH -> RGB) and the prefix sum of tiles touched.  Writes radii[P] (int32, may be NULL). */
int gsaj_forward_preprocess(int P, int D, int M, int W, int H,
                            const float *means3D /*dev [P,3]*/, const float *shs /*dev [P,M,3] or NULL*/,
                            const float *colors_precomp /*dev [P,3] or NULL*/, const float *opacities /*dev [P]*/,
                            const float *scales /*dev [P,3] or NULL*/, float scale_modifier,
                            const float *rotations /*dev [P,4] or NULL*/, const float *cov3D_precomp /*dev [P,6] or NULL*/,
                            const float *viewmatrix /*dev [16]*/, const float *projmatrix /*dev [16]*/,
                            const float *campos /*dev [3]*/, float tanfovx, float tanfovy, int prefiltered,
                            int *radii /*dev [P] or NULL*/, int *n_touched /*dev [P], zeroed here*/,
                            void *geom_ws /*dev*/, void *image_ws /*dev*/, void *stream);
/* Blocking: number of (Gaussian, tile) instances produced by phase A. */
int gsaj_forward_num_rendered(int W, int H, const void *image_ws, void *stream, int *num_rendered /*host*/,
                              int *max_tile_list /*host, may be NULL: longest per-tile list*/);
/* Phase B: instance scatter into per-tile id lists, per-tile (depth, id) sort in LDS (a list longer than the LDS capacity
 * is sorted in LDS-sized chunks and merged in place by the same workgroup: no list length is refused), front-to-back
 * compositing straight from the sorted id list (the compositor gathers the per-Gaussian 48-byte rows of phase A).
 * out_color [3,H,W], out_depth [1,H,W], out_opacity [1,H,W], n_touched [P] int32.  R must be the value phase A produced. */
int gsaj_forward_render(int P, int R, int max_tile_list /* from phase A: sizes the LDS sort; < 0 forces the chunk + merge path
                                                           (128-key chunks) for every list longer than 128 -- for tests */, int W, int H,
                        const float *bg /*dev [3]*/,
                        const float *colors_precomp /*dev [P,3] or NULL*/, const int *radii /*dev [P] or NULL*/,
                        void *geom_ws, void *binning_ws, size_t binning_ws_bytes, void *image_ws,
                        float *out_color, float *out_depth, float *out_opacity, int *n_touched,
                        int flags /* GSAJ_FWD_*: takes the place of the reference's `bool debug` */, void *stream);

/* ---- forward, one call (phase A, sync, phase B).  The caller supplies a binning
 * workspace of any capacity; if it is too small the call fails with
 * GSAJ_ERR_WORKSPACE_TOO_SMALL and *num_rendered_out holds the R to size it for. */
int gsaj_rasterize_forward(int P, int D, int M, const float *bg, int W, int H,
                           const float *means3D, const float *shs, const float *colors_precomp,
                           const float *opacities, const float *scales, float scale_modifier,
                           const float *rotations, const float *cov3D_precomp,
                           const float *viewmatrix, const float *projmatrix, const float *campos,
                           float tanfovx, float tanfovy, int prefiltered,
                           float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched,
                           void *geom_ws, void *binning_ws, size_t binning_ws_bytes, void *image_ws,
                           int *num_rendered_out /*host, may be NULL*/, int flags /* GSAJ_FWD_* */, void *stream);

/* ---- forward without any host synchronisation (tracking / mapping inner loops) -----------------
 * The caller provides a binning workspace sized for `capacity` instances
 * (gsaj_binning_workspace_bytes(capacity)) and passes the SAME capacity as `R` to
 * gsaj_rasterize_backward.  If the frame needs more instances than that, the frame is aborted on the
 * device (every later kernel of the frame returns at once: outputs are the previous frame's) and
 * gsaj_forward_num_rendered -- which may be called at any later time -- returns
 * GSAJ_ERR_WORKSPACE_TOO_SMALL together with the R to size the arena for; the caller then repeats
 * the frame with a larger arena.  tile_list_capacity (0 = the maximum, 16384): the tile-list length the
 * per-tile LDS sort is sized for (rounded up to a power of two >= 128); the sort is given exactly that much
 * shared memory, so scenes with short lists keep more workgroups resident.  It is a performance hint only:
 * a longer list is sorted in chunks of that size and merged (slower, same result) -- never an abort. */
int gsaj_rasterize_forward_async(int P, int D, int M, const float *bg, int W, int H,
                                 const float *means3D, const float *shs, const float *colors_precomp,
                                 const float *opacities, const float *scales, float scale_modifier,
                                 const float *rotations, const float *cov3D_precomp,
                                 const float *viewmatrix, const float *projmatrix, const float *campos,
                                 float tanfovx, float tanfovy, int prefiltered,
                                 float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched,
                                 void *geom_ws, void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity,
                                 void *image_ws, int flags /* GSAJ_FWD_* */, void *stream);
/* Blocking: number of async forwards aborted on the device since the previous call (read and clear; the first call counts
 * from when the caller zero-filled the image workspace, which it does once, when it allocates it). */
int gsaj_forward_aborted_count(int W, int H, void *image_ws, void *stream, int *count /*host*/);

/* Device address of the frame's abort word inside the image workspace: non-zero after an asynchronous forward that did not fit
 * its arena (every later kernel of that frame returned at once: images, dL/dtau and per-Gaussian outputs are the previous
 * frame's); cleared by the next forward.  Stream-ordered consumers on the device read it without a host round trip:
 * gsaj_pose_adam_step(skip = this) leaves the pose alone after an aborted frame.  NULL on invalid arguments. */
const uint32_t *gsaj_forward_abort_flag(int W, int H, void *image_ws);

/* Tile-band sharding of ONE frame (tracking on several GPUs; no counterpart in the reference, whose rasteriser is
 * single-device: cuda_rasterizer/rasterizer_impl.cu:224-352 binds every tile of the frame).  Every later forward that uses
 * this image workspace renders only tile rows [tile_row_begin, tile_row_end) of the (H + 15) / 16 rows: a Gaussian's tile
 * rectangle (auxiliary.h:46-58 getRect) is clipped to the band, pixels outside it come out as background / zero depth /
 * zero opacity, Gaussians with no tile inside get radii = 0, and the backward returns the band's share of every gradient
 * and of dL/dtau -- the shares of disjoint bands covering the frame add up to the whole-frame result (every gradient is a
 * sum over pixels).  The setting is kept in the image workspace (stream-ordered) until changed; [0, rows) restores the
 * whole frame.  In a batched workspace set it on each view's block.  A workspace this call never touched renders the whole
 * frame whatever its bytes are (the band word is stored with its complement and ignored unless both agree). */
int gsaj_set_tile_band(int W, int H, void *image_ws, int tile_row_begin, int tile_row_end, void *stream);
/* gsaj_forward_preprocess with the arena capacity check armed (capacity = 0: unchecked). */
int gsaj_forward_preprocess_cap(int P, int D, int M, int W, int H,
                                const float *means3D, const float *shs, const float *colors_precomp,
                                const float *opacities, const float *scales, float scale_modifier,
                                const float *rotations, const float *cov3D_precomp,
                                const float *viewmatrix, const float *projmatrix, const float *campos,
                                float tanfovx, float tanfovy, int prefiltered, int *radii, int *n_touched,
                                void *geom_ws, void *image_ws, int capacity, int tile_list_capacity, void *stream);

/* ---- backward ------------------------------------------------------------------------ */
/* dL_dpix [3,H,W], dL_dpix_depth [1,H,W] -> dL_dmean2D [P,3] (NDC-scaled, z unused),
 * dL_dconic [P,2,2] (slots 0,1,3), dL_dopacity [P], dL_dcolor [P,3], dL_ddepth [P],
 * dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscale [P,3], dL_drot [P,4],
 * dL_dtau [P,6] (may be NULL) and dL_dtau_sum [6] = sum over Gaussians, tau = [rho, theta]
 * (may be NULL; replaces torch.sum in diff_gaussian_rasterization/__init__.py:162).
 * Pose-only mode (tracking, where only the camera is optimised): pass NULL for ALL ten per-Gaussian outputs
 * dL_dmean2D .. dL_drot and a dL_dtau_sum; the per-Gaussian parameter gradients are then neither finished nor stored.
 * The three workspaces must be the ones the forward filled.  W, H <= GSAJ_BWD_MAX_SIDE = 16384 ("image size of a backward", below). */
int gsaj_rasterize_backward(int P, int D, int M, int R, const float *bg, int W, int H,
                            const float *means3D, const float *shs, const float *colors_precomp,
                            const float *scales, float scale_modifier, const float *rotations,
                            const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                            const float *projmatrix_raw, const float *campos, float tanfovx, float tanfovy,
                            const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                            const float *dL_dpix, const float *dL_dpix_depth,
                            float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor,
                            float *dL_ddepth, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh,
                            float *dL_dscale, float *dL_drot, float *dL_dtau, float *dL_dtau_sum, void *stream);

/* ---- batched multi-view entry points: K views of ONE Gaussian map ------------------------------------------------
 * The mapping step of the reference renders every keyframe of the window against the same Gaussians, sums the losses and
 * back-propagates once: per-Gaussian gradients ACCUMULATE over the keyframes, every keyframe keeps its own dL/dtau
 * (utils/slam_backend.py:168-232).  These two calls do that for K views in one set of launches (grids x K): the Gaussians
 * are read once per kernel where the view does not matter, the per-Gaussian parameter gradients are summed over the K views
 * inside the kernel in view order (deterministic) and written once, and K rows of dL/dtau come out.
 *
 * Per-view arrays are K consecutive blocks: viewmatrices / projmatrices [K,16], campos [K,3], out_color [K,3,H,W], out_depth
 * / out_opacity [K,1,H,W], radii / n_touched [K,P], dL_dpix [K,3,H,W], dL_dpix_depth [K,1,H,W].  All K views share W, H,
 * tanfov (one camera model) and projmatrix_raw.  Workspaces are K consecutive blocks of gsaj_geom_workspace_bytes(P),
 * gsaj_image_workspace_bytes(W, H) and gsaj_binning_workspace_bytes(capacity) bytes, 256-byte aligned, the image workspaces
 * zeroed once by the caller; view v's block can be handed to gsaj_forward_num_rendered / gsaj_forward_aborted_count /
 * gsaj_debug_export on its own.  Like gsaj_rasterize_forward_async there is NO host synchronisation: `capacity` instances
 * per view, a view that needs more is aborted on the device, contributes nothing to the sums, and is reported by
 * gsaj_forward_num_rendered(view block); tile_list_capacity as in gsaj_rasterize_forward_async (a hint, never an abort).
 *
 * Backward outputs.  Summed over the views: dL_dopacity [P], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscale
 * [P,3], dL_drot [P,4].  Per view (each may be NULL): dL_dmean2D [K,P,3] (what densification reads as
 * viewspace_points.grad, gaussian_model.py:767-771), dL_dconic [K,P,2,2], dL_dcolor [K,P,3], dL_ddepth [K,P], dL_dtau [K,P,6];
 * and dL_dtau_sum [K,6].  SH storage of 1, 4, 9 or 16 coefficients.  Backward: W, H <= GSAJ_BWD_MAX_SIDE; forward: any size. */
int gsaj_rasterize_forward_batch(int K, int P, int D, int M, const float *bg, int W, int H, const float *means3D,
                                 const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                                 float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                 const float *viewmatrices, const float *projmatrices, const float *campos, float tanfovx,
                                 float tanfovy, int prefiltered, float *out_color, float *out_depth, float *out_opacity,
                                 int *radii, int *n_touched, void *geom_ws, void *binning_ws, size_t binning_ws_bytes,
                                 int capacity, int tile_list_capacity, void *image_ws, int flags /* GSAJ_FWD_* */, void *stream);
int gsaj_rasterize_backward_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H,
                                  const float *means3D, const float *shs, const float *colors_precomp, const float *scales,
                                  float scale_modifier, const float *rotations, const float *cov3D_precomp,
                                  const float *viewmatrices, const float *projmatrices, const float *projmatrix_raw,
                                  const float *campos, float tanfovx, float tanfovy, const int *radii, void *geom_ws,
                                  void *binning_ws, void *image_ws, const float *dL_dpix, const float *dL_dpix_depth,
                                  float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor, float *dL_ddepth,
                                  float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale, float *dL_drot,
                                  float *dL_dtau, float *dL_dtau_sum, int flags /* GSAJ_BWD_* */, void *stream);
/* flags of gsaj_rasterize_backward_batch:
 * GSAJ_BWD_ACCUMULATE      the summed per-Gaussian outputs are ADDED to what their buffers hold instead of overwriting them:
 *                          a window processed in several calls (views [0,K0) then [K0,K)), or the keyframes of several windows
 *                          accumulated on one rank before the optimiser step (utils/slam_backend.py:168-232: current window +
 *                          2 random older keyframes, ONE backward).  Calls add in the caller's order: reproducible.
 * GSAJ_BWD_ONLY_COMPOSITE  run only the per-view half (reverse compositor + per-Gaussian gather of its partial sums);
 * GSAJ_BWD_ONLY_CHAIN      run only the per-Gaussian chain on views whose per-view half has already run.
 *                          Together they let a caller put the per-view halves of two view groups on two HIP streams (they are
 *                          independent) and serialise only the accumulating chains (gsaj.rasterizer.BatchContext(streams=2)). */
#define GSAJ_BWD_ACCUMULATE 1
#define GSAJ_BWD_ONLY_COMPOSITE 2
#define GSAJ_BWD_ONLY_CHAIN 4

/* ---- frustum test -------------------------------------------------------------------- */
int gsaj_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                      uint8_t *present /*dev [P]*/, void *stream);

/* ---- introspection of the forward state (parity tests, debugging) -------------------- */
/* Copies internal arrays to caller-provided DEVICE buffers; any pointer may be NULL.
 * means2D [P,2], depths [P], cov3D [P,6], conic_opacity [P,4], rgb [P,3], clamped [P,3] u8,
 * tiles_touched [P] u32, point_list [R] u32, ranges [tiles,2] u32, final_T [H,W], n_contrib [H,W] u32. */
int gsaj_debug_export(int P, int R, int W, int H, const void *geom_ws, const void *binning_ws, const void *image_ws,
                      float *means2D, float *depths, float *cov3D, float *conic_opacity, float *rgb, uint8_t *clamped,
                      uint32_t *tiles_touched, uint32_t *point_list, uint32_t *ranges, float *final_T,
                      uint32_t *n_contrib, void *stream);

/* What the forward compositor took, and what the reverse compositor wrote, of one view (its blocks of the binning and image
 * workspaces; R = the capacity the binning workspace was carved for).  taken [R] u32, by position in point_list: byte q = 1 if
 * some pixel of quadrant q (8x8 pixels; q = 2 * (lower half) + (right half)) of the position's tile composited that entry, as the
 * reverse compositor reads it: bytes at or beyond the quadrant's furthest last contributor are cleared (they may be stale in the
 * workspace); positions outside every tile list are left as the caller initialised them.  reached [R] u8, by emission slot: 1 = the
 * last backward wrote that instance's row.  Either may be NULL. */
int gsaj_debug_export_taken(int R, int W, int H, const void *binning_ws, const void *image_ws, uint32_t *taken /*dev [R]*/,
                            uint8_t *reached /*dev [R]*/, void *stream);

/* After gsaj_rasterize_backward_batch: the reverse compositor's 10 sums per Gaussian of ONE view of the window (that view's block
 * of the geometry workspace), sums [P,12] = (dL/dmean2D x, y | dL/dconic a, b, c | dL/dopacity | dL/dcolor r, g, b | dL/ddepth | 2
 * pads) -- the per-view quantities the batched backward does not return (it returns their sums over the views), for parity tests. */
/* gsaj_debug_export_view_sums copies what the geometry workspace holds: valid only after a GSAJ_BWD_ONLY_COMPOSITE call, which
 * leaves the sums there for the GSAJ_BWD_ONLY_CHAIN call.  A whole-window call (neither flag) forms the sums inside its chain kernel
 * and never stores them: after it use gsaj_debug_export_view_sums_gather, which takes that view's blocks of all three workspaces
 * (256-byte aligned, as the batched entry points take them), sums the view's instance rows again -- they and their `reached` flags
 * survive until the next forward -- into the geometry workspace, and copies the result.  Same additions, same bits, either way. */
int gsaj_debug_export_view_sums(int P, const void *geom_ws, float *sums /*dev [P,12]*/, void *stream);
int gsaj_debug_export_view_sums_gather(int P, int capacity, int W, int H, void *geom_ws, void *binning_ws, void *image_ws,
                                       float *sums /*dev [P,12]*/, void *stream);

/* ---- per-kernel timing (bench.py's roofline leg) ----------------------------------------
 * Between gsaj_profile_begin and gsaj_profile_end every kernel launch of the library is
 * bracketed by HIP events on the stream it is launched on.  gsaj_profile_end synchronises,
 * and returns per stage the summed duration in ms and the number of launches.
 * Stage order: GSAJ_STAGE_NAMES.  (scan_blocks, emit_keys, sort, ranges_records and tau_finalize belong to kernels that no
 * longer exist; the slots are kept so that the indices of the others do not move, and report 0 launches.  tile_sort_records
 * is k_tile_sort -- it sorts ids now, there are no per-instance records.) */
#define GSAJ_NUM_STAGES 14
#define GSAJ_STAGE_NAMES "preprocess,scan_blocks,emit_keys,sort,ranges_records,render_fwd,render_bwd,gaussian_bwd,tau_finalize,dense_bwd,dense_reduce,scatter_instances,tile_sort_records,gather_sums"
int gsaj_profile_begin(int max_records);
int gsaj_profile_end(float *stage_ms /*host [GSAJ_NUM_STAGES]*/, int *stage_launches /*host [GSAJ_NUM_STAGES]*/);

/* ---- losses + pixel-gradient seeds ---------------------------------------------
 * Replaces the ~15 full-frame torch kernels + autograd of get_loss_tracking / get_loss_mapping
 * (reference utils/slam_utils.py:56-128) by one pass: reads color [3,H,W], depth [1,H,W], opacity [1,H,W], the
 * ground truth gt_color [3,H,W], gt_depth [H,W] (RGB-D only) and the optional tracking grad_mask [H,W] (bytes,
 * non-zero = keep; slam_utils.py:69), the exposure scalars a, b on the device (ignored with NO_EXPOSURE, i.e.
 * get_loss_mapping(initialization=True)), and writes dL/dcolor [3,H,W], dL/ddepth [1,H,W] -- the two inputs of
 * gsaj_rasterize_backward -- optionally dL/dopacity [1,H,W] (the reference's rasteriser ignores it), and
 * out_scalars[5] = {loss, L_rgb, L_depth, dL/da, dL/db} on the device.  Deterministic (no float atomics).
 * loss_ws: gsaj_loss_workspace_bytes(W, H) bytes, ZEROED ONCE by the caller when allocated. */
#define GSAJ_LOSS_TRACKING 1    /* opacity weight, grad_mask, opacity > 0.95 depth gate (get_loss_tracking*) */
#define GSAJ_LOSS_MONOCULAR 2   /* config["Training"]["monocular"]: colour term only */
#define GSAJ_LOSS_NO_EXPOSURE 4 /* image_ab = image (get_loss_mapping(initialization=True)) */
#define GSAJ_LOSS_COMPUTE_LOSS 8 /* compute_loss of the verification harness (Jacobian_test.py:155-196, compare.py:144-185):
                                  * grad_mask = the per-pixel mask; colour = mean over 3HW of |color*mask - gt*mask|; depth = mean
                                  * over the pixels with gt_depth > 0 inside the mask of |depth - gt|; loss = their plain sum
                                  * (alpha, rgb_boundary_threshold, exposure ignored; with MONOCULAR: colour term only).  The
                                  * 10 x isotropic term of compute_loss is per Gaussian: gsaj_isotropic_loss. */
size_t gsaj_loss_workspace_bytes(int W, int H);
int gsaj_loss_seeds(int W, int H, int flags, float alpha, float rgb_boundary_threshold, const float *color,
                    const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                    const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float *dL_dcolor,
                    float *dL_ddepth, float *dL_dopacity, float *out_scalars, void *loss_ws, void *stream);

/* ---- the same losses FUSED into the compositors (SURVEY 8(f)-1 as written): no seed image, no pass over the frame ------------
 * The reference evaluates get_loss_tracking / get_loss_mapping between render() and backward() (utils/slam_frontend.py:164-176,
 * utils/slam_utils.py:56-128).  gsaj_rasterize_forward_loss = gsaj_rasterize_forward_async whose compositor epilogue also sums the
 * loss terms of its pixels against the ground truth; out_scalars[5] = {loss, L_rgb, L_depth, dL/da, dL/db} (device) are there when
 * the call's work has run.  gsaj_rasterize_backward_loss = gsaj_rasterize_backward whose reverse compositor derives each pixel's
 * seeds dL/dC, dL/dD from the images the forward wrote (color, depth, opacity: pass them back), the ground truth and the exposure
 * scalars, with the arithmetic of gsaj_loss_seeds bit for bit -- the gradients equal those of forward -> gsaj_loss_seeds ->
 * backward exactly; the loss scalars differ from gsaj_loss_seeds' only by the order of their sums.  loss_flags: GSAJ_LOSS_TRACKING,
 * _MONOCULAR, _NO_EXPOSURE (GSAJ_LOSS_COMPUTE_LOSS has no fused form).  loss_ws: gsaj_fused_loss_workspace_bytes(W, H) bytes, no
 * initialisation needed.  An aborted frame leaves out_scalars as they were.  Backward forms: W, H <= GSAJ_BWD_MAX_SIDE. */
size_t gsaj_fused_loss_workspace_bytes(int W, int H);
int gsaj_rasterize_forward_loss(int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                                const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                const float *projmatrix, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                                float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched, void *geom_ws,
                                void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity, void *image_ws,
                                int flags /* GSAJ_FWD_* */, int loss_flags /* GSAJ_LOSS_* */, float alpha,
                                float rgb_boundary_threshold, const float *gt_color /*dev [3,H,W]*/,
                                const float *gt_depth /*dev [H,W] or NULL (monocular)*/, const uint8_t *grad_mask /*dev [H,W] or NULL*/,
                                const float *exposure_a, const float *exposure_b /*dev scalars; NULL with NO_EXPOSURE*/,
                                float *out_scalars /*dev [5]*/, void *loss_ws, void *stream);
int gsaj_rasterize_backward_loss(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                                 const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                 const float *projmatrix_raw, const float *campos, float tanfovx, float tanfovy, const int *radii,
                                 void *geom_ws, void *binning_ws, void *image_ws, int loss_flags, float alpha,
                                 float rgb_boundary_threshold, const float *color, const float *depth, const float *opacity,
                                 const float *gt_color, const float *gt_depth, const uint8_t *grad_mask, const float *exposure_a,
                                 const float *exposure_b, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dcolor,
                                 float *dL_ddepth, float *dL_dmean3D, float *dL_dcov3D, float *dL_dsh, float *dL_dscale,
                                 float *dL_drot, float *dL_dtau, float *dL_dtau_sum, void *stream);

/* ---- the fused losses for the K views of a mapping window ---------------------------------------------------------------------
 * gsaj_rasterize_forward_loss_batch = gsaj_rasterize_forward_batch whose compositor also sums each view's loss terms, followed by
 * one finalize workgroup per view: out_scalars [K,5] row k = {loss, L_rgb, L_depth, dL/da, dL/db} of view k, and, if
 * out_dexposure is given, out_dexposure [K,2] row k = {dL/da, dL/db} (the contiguous form gsaj_pose_adam_step_batch reads).
 * gsaj_rasterize_backward_loss_batch = gsaj_rasterize_backward_batch whose reverse compositor derives the pixel seeds of view k from
 * color / depth / opacity [K,.,H,W] as the forward wrote them; no [K,3,H,W] / [K,1,H,W] seed images exist.  gt_color [K,3,H,W],
 * gt_depth / grad_mask [K,H,W]; exposure_a / exposure_b point at view 0's scalars, view k's are exposure_stride floats further on
 * (1: contiguous [K]; 80: columns 33 and 34 of the gsaj_pose_adam_step_batch state, read in place).
 * Bit for bit: every image, n_touched and every gradient equals gsaj_rasterize_forward_batch -> gsaj_loss_seeds_batch ->
 * gsaj_rasterize_backward_batch on the same inputs, and row k of out_scalars equals what gsaj_rasterize_forward_loss gives for view
 * k alone (same partial grid, same summation order); with K = 1 both calls are the single-view pair above.  The scalars differ
 * from gsaj_loss_seeds_batch's only by the order of their sums.  A view aborted on the device (binning arena too small) leaves its
 * rows of out_scalars / out_dexposure as they were and contributes nothing to any gradient.
 * loss_ws: gsaj_fused_loss_batch_workspace_bytes(K, W, H) = K blocks of gsaj_fused_loss_workspace_bytes(W, H) rounded up to 256
 * bytes; no initialisation needed.  The GSAJ_BWD_* flags keep their meaning (GSAJ_BWD_ONLY_CHAIN reads no image and ignores the loss
 * arguments).  Invalid arguments are reported before anything is launched. */
size_t gsaj_fused_loss_batch_workspace_bytes(int K, int W, int H);
int gsaj_rasterize_forward_loss_batch(int K, int P, int D, int M, const float *bg, int W, int H, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales, float scale_modifier,
                                      const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                      const float *projmatrices, const float *campos, float tanfovx, float tanfovy, int prefiltered,
                                      float *out_color, float *out_depth, float *out_opacity, int *radii, int *n_touched, void *geom_ws,
                                      void *binning_ws, size_t binning_ws_bytes, int capacity, int tile_list_capacity, void *image_ws,
                                      int flags /* GSAJ_FWD_* */, int loss_flags /* GSAJ_LOSS_* */, float alpha,
                                      float rgb_boundary_threshold, const float *gt_color /*dev [K,3,H,W]*/,
                                      const float *gt_depth /*dev [K,H,W] or NULL (monocular)*/,
                                      const uint8_t *grad_mask /*dev [K,H,W] or NULL*/, const float *exposure_a, const float *exposure_b,
                                      int exposure_stride /*floats between views, >= 1; pointers NULL with NO_EXPOSURE*/,
                                      float *out_scalars /*dev [K,5]*/, float *out_dexposure /*dev [K,2] or NULL*/, void *loss_ws,
                                      void *stream);
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
                                       float *dL_dtau_sum, int flags /* GSAJ_BWD_* */, void *stream);

/* The same for the K views of a mapping window in ONE launch (utils/slam_backend.py:168-232 sums get_loss_mapping over the
 * keyframes of the window): color / gt_color / dL_dcolor [K,3,H,W], depth / opacity / dL_ddepth / dL_dopacity [K,1,H,W], gt_depth /
 * grad_mask [K,H,W], exposure_a / exposure_b [K] (one pair per keyframe, camera_utils.py:43-48), out_scalars [K,5]; view k gets
 * exactly what gsaj_loss_seeds gives for its slices.  loss_ws: K blocks of gsaj_loss_workspace_bytes(W, H) rounded up to 256 bytes,
 * 256-byte aligned, zeroed once.  GSAJ_LOSS_COMPUTE_LOSS has no batched form. */
int gsaj_loss_seeds_batch(int K, int W, int H, int flags, float alpha, float rgb_boundary_threshold, const float *color,
                          const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                          const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float *dL_dcolor,
                          float *dL_ddepth, float *dL_dopacity, float *out_scalars, void *loss_ws, void *stream);

/* weight * mean |s_ij - mean_j(s_i.)| over scales [P,C] (C = 1..3) -> out_loss[0] (device), and its gradient into dL_dscales
 * [P,C] (may be NULL; accumulate != 0: added to what is there): the isotropic regulariser of compute_loss (weight 10,
 * Jacobian_test.py:169-171) and of the mapping loss (slam_backend.py:229-231).  iso_ws: gsaj_isotropic_workspace_bytes(P),
 * ZEROED ONCE by the caller when allocated.  Deterministic. */
size_t gsaj_isotropic_workspace_bytes(int P);
int gsaj_isotropic_loss(int P, int C, float weight, const float *scales, float *dL_dscales, int accumulate, float *out_loss,
                        void *iso_ws, void *stream);

/* ---- SSIM and the L1 + D-SSIM loss of colour refinement -------------------------------------------------------------
 * ssim (gaussian_splatting/utils/loss_utils.py:42-101): 11x11 Gaussian window (sigma 1.5), zero padding 5, C1 = 0.01^2,
 * C2 = 0.03^2, over img / gt [N,C,H,W] fp32 (contiguous, planes independent; any N, C, W, H >= 1).  Deterministic: workgroup
 * partials are summed in a fixed order by the last workgroup.  ssim_ws: gsaj_ssim_workspace_bytes(N, C, W, H) bytes, ZEROED
 * ONCE by the caller when allocated (it holds the ticket, reset by the last workgroup). */
size_t gsaj_ssim_workspace_bytes(int N, int C, int W, int H);
/* ssim_out [N+1] (dev): per-image mean of the SSIM map (size_average=False), then the mean over all N*C*H*W (size_average=True).
 * ssim_map [N,C,H,W] (dev) may be NULL.  Leaves the partial maps the backward needs in ssim_ws. */
int gsaj_ssim_forward(int N, int C, int W, int H, const float *img, const float *gt, float *ssim_out, float *ssim_map,
                      void *ssim_ws, void *stream);
/* dL_dssim [N+1] (dev): upstream gradient of each entry of ssim_out -> dL_dimg [N,C,H,W] (dev), the gradient w.r.t. img only.
 * Uses the partial maps the last gsaj_ssim_forward on the same inputs left in ssim_ws. */
int gsaj_ssim_backward(int N, int C, int W, int H, const float *img, const float *gt, const float *dL_dssim, float *dL_dimg,
                       void *ssim_ws, void *stream);
/* Colour refinement, one view (utils/slam_backend.py:320-352): image, gt [3,H,W] -> dL_dcolor [3,H,W] (the input of
 * gsaj_rasterize_backward) and out_scalars [3] (dev) = {loss, L1, SSIM}, loss = (1 - lambda) L1 + lambda (1 - SSIM).
 * Two launches, no host synchronisation.  ws: gsaj_refine_loss_workspace_bytes(W, H) bytes, zeroed once. */
size_t gsaj_refine_loss_workspace_bytes(int W, int H);
int gsaj_refine_loss_seeds(int W, int H, float lambda_dssim, const float *image, const float *gt, float *dL_dcolor,
                           float *out_scalars, void *ws, void *stream);

/* ---- densification / pruning bookkeeping ----------------------------------------------------------
 * What the reference's mapping loop does per rendered view after the backward (utils/slam_backend.py:113-121, 276-285):
 *   vis = radii > 0;  max_radii2D[vis] = max(max_radii2D[vis], radii[vis]);
 *   xyz_gradient_accum[vis] += ||viewspace_points.grad[vis, :2]||;  denom[vis] += 1        (gaussian_model.py:767-771)
 * and, for pruning, n_obs = number of views that touched the Gaussian (n_touched > 0; slam_backend.py:236-250), for the K
 * views of a window in ONE launch (K = 1: one view).  dL_dmean2D [K,P,3] (the backward's per-view output), radii [K,P],
 * n_touched [K,P] (may be NULL); xyz_gradient_accum [P], denom [P], max_radii2D [P] are updated in place (each may be NULL),
 * n_obs [P] int32 is written (may be NULL). */
int gsaj_densification_stats(int K, int P, const float *dL_dmean2D, const int *radii, const int *n_touched,
                             float *xyz_gradient_accum, float *denom, float *max_radii2D, int *n_obs, void *stream);

/* ---- tracking pose step on the device -------------------------------------------
 * One launch = torch.optim.Adam.step() on (cam_trans_delta, cam_rot_delta, exposure_a, exposure_b) as set up in
 * slam_frontend.py:135-160 + update_pose (reference utils/pose_utils.py:76-93) + the camera matrices of
 * camera_utils.py:95-109, with no host read-back.  dL_dtau = [rho(3), theta(3)] is the dL_dtau_sum of
 * gsaj_rasterize_backward; dL_dexposure = {dL/da, dL/db} (out_scalars + 3 of gsaj_loss_seeds) or NULL.
 * projection_matrix = the camera's projection_matrix (P^T, row-major [16]) or NULL.
 * pose_state: GSAJ_POSE_STATE_FLOATS device floats owned by the caller:
 *   [0:16)  W2C row-major (in: current pose; out: Exp(tau) * W2C)      [16:24) Adam m   [24:32) Adam v
 *   [32]    step count    [33:35) exposure a, b (updated in place)
 *   [35:51) out world_view_transform = W2C^T     [51:67) out full_proj_transform    [67:70) out camera_center
 *   [70:76) out tau = [rho, theta] applied       [76] out |tau|     [77] out converged (1.0 / 0.0: |tau| < threshold)
 * Initialise [0:16) with the pose and zero the rest.
 * skip (device, may be NULL): if the 32-bit word it points to is non-zero the call changes NOTHING (no Adam moment, no step
 * count, no pose): pass gsaj_forward_abort_flag() of the frame the gradients come from -- an aborted asynchronous frame leaves
 * the previous iteration's dL/dtau in place -- or, with the frame sharded over ranks, a word of the all-reduced buffer that is
 * non-zero when ANY rank's share was aborted (any non-zero bit pattern counts, e.g. a positive float). */
#define GSAJ_POSE_STATE_FLOATS 80
int gsaj_pose_state_floats(void);
int gsaj_pose_adam_step(const float *dL_dtau, const float *dL_dexposure, float lr_rot, float lr_trans, float lr_exp_a,
                        float lr_exp_b, float beta1, float beta2, float eps, float converged_threshold,
                        const float *projection_matrix, float *pose_state, const uint32_t *skip, void *stream);

/* The same step for K poses in one launch (the keyframe poses of a mapping window, each with its own Adam state:
 * utils/slam_backend.py:255-262 steps the keyframe optimiser and calls update_pose per keyframe, skipping uid 0):
 * dL_dtau [K,6] (the dL_dtau_sum rows of gsaj_rasterize_backward_batch), dL_dexposure [K,2] or NULL, active [K] bytes or NULL
 * (0: the pose and its Adam state are left untouched), pose_states [K, GSAJ_POSE_STATE_FLOATS]; the learning rates are shared.
 * skip (may be NULL) / skip_stride_bytes: pose k is left untouched if the word at skip + k * skip_stride_bytes is non-zero -- with
 * skip = gsaj_forward_abort_flag(view 0's image workspace) and skip_stride_bytes = gsaj_image_workspace_bytes(W, H), the views of a
 * batched window that were aborted on the device. */
int gsaj_pose_adam_step_batch(int K, const float *dL_dtau, const float *dL_dexposure, const uint8_t *active, float lr_rot,
                              float lr_trans, float lr_exp_a, float lr_exp_b, float beta1, float beta2, float eps,
                              float converged_threshold, const float *projection_matrix, float *pose_states, const uint32_t *skip,
                              size_t skip_stride_bytes, void *stream);

/* ---- Gauss-Newton tracking: per-pixel pose Jacobians, normal equations, Levenberg-Marquardt step -----------------
 * tau = [rho(3), theta(3)] is the left increment W2C <- Exp(tau) W2C.  The pose Jacobian of a pixel, J_p [4,6] (rows r, g, b,
 * depth of what gsaj_rasterize_forward writes), is the exact transpose of the map the backward implements: for any seed images
 * s, sum_p sum_ch s[ch,p] J_p[ch,:] == dL_dtau_sum of gsaj_rasterize_backward(seeds = s) in real arithmetic -- the 0.99 alpha cap
 * is no gradient gate, power > 0 / alpha < 1/255 entries and entries behind a pixel's last contributor add nothing, the
 * background term -T_final S bg is included, radii and tile rectangles are constants.
 *
 * Both entry points take the geometry arguments of gsaj_rasterize_backward and the geom / binning / image workspaces of a
 * FINISHED forward of the same frame (synchronous, asynchronous or loss-fused; R = what the backward would be given; a tile band
 * is not supported), and a scratch workspace jac_ws of gsaj_pose_jac_workspace_bytes(P, W, H) bytes (no initialisation needed).
 * No float atomics: results are the same bits run to run.  An aborted asynchronous frame leaves every output as it was.
 *
 * gsaj_rasterize_pose_jacobian -- the explicit form.  Outputs, each may be NULL: jac_out [H,W,4,6]; out_color [3,H,W] and
 *   out_depth [H,W], the images re-derived by the walk (the forward's bits); g_out [6] = sum s J from the seed images seed_color
 *   [3,H,W], seed_depth [H,W]; H_out [21] = the upper triangle, by rows, of sum h J^T J from the curvature images curv_color
 *   [3,H,W], curv_depth [H,W].  g_out needs both seed images, H_out both curvature images (GSAJ_ERR_INVALID_ARGUMENT otherwise,
 *   and for the argument errors of gsaj_rasterize_backward).
 * gsaj_rasterize_pose_jacobian_loss -- the fused form, for the tracking loss of gsaj_rasterize_backward_loss (same loss arguments;
 *   exposure enters as the fixed affine e^a C + b, it is not solved for: the joint form below does).  With the residuals r of csrc/loss_terms.h, kappa_rgb =
 *   k_rgb w_rgb, kappa_d = k_d and irls_delta >= 0 (iteratively reweighted least squares for the L1 terms):
 *     seed s = kappa (dr/dC) clamp(r / delta, -1, 1)   (delta == 0: the backward's own seed, bit for bit)
 *     curvature h = kappa (dr/dC)^2 / max(|r|, delta)  (0 where the gate is closed, or r == 0 with delta == 0)
 *   gn_partials [gsaj_pose_jac_partial_rows(W, H)][GSAJ_GN_PARTIAL_FLOATS]: one row per workgroup, fixed slots --
 *   [0:21) H, [21:27) g, [27] loss, [28] L_rgb, [29] L_depth, [30:32) the exposure sums of the fused forward -- which
 *   gsaj_pose_gn_step (or any reader) adds up in slot order.  jac_out may be NULL.
 *
 * gsaj_pose_gn_step -- one Levenberg-Marquardt step on the device, one launch, no host read.  gn_state: GSAJ_GN_STATE_FLOATS
 *   floats owned by the caller; [0:80) have the layout of the pose state above (W2C, exposure at 33 / 34, the camera matrices,
 *   tau, |tau|, converged; the Adam slots are unused), then
 *     [80] lambda   [81] accepted loss   [82] 1.0 once a pose has been accepted   [83] accepted steps   [84] rejected steps
 *     [85:88) loss, L_rgb, L_depth of the last call   [88:104) accepted W2C   [104:125) accepted H   [125:131) accepted g
 *   Initialise [0:16) with the pose (and [33:35) with the exposure) and zero the rest.  The call sums the rows; on the first
 *   call, or if loss <= accepted loss, it accepts -- saves (loss, W2C, H, g), lambda <- max(lambda / nu, lambda_min), lambda
 *   starting from lambda_init -- otherwise it rejects: restores the accepted W2C, H, g, lambda <- min(lambda nu, lambda_max).
 *   Then (H + lambda diag(H) + eps I) tau = -g is solved by Cholesky in fp64 (eps = 1e-9 x the mean of diag(H) + 1e-30) and
 *   W2C <- Exp(tau) W2C is applied with the operations of gsaj_pose_adam_step, the camera matrices are refreshed, tau, |tau| and
 *   converged = |tau| < converged_threshold written.  A non-positive pivot raises lambda and leaves the pose unchanged for the
 *   call (tau = 0, converged = 0).  skip: as in gsaj_pose_adam_step -- a non-zero word (aborted frame) changes nothing.
 *   GSAJ_ERR_INVALID_ARGUMENT unless nu > 1 and 0 < lambda_min <= lambda_init <= lambda_max.
 *
 * The joint form -- the exposure solved together with the pose.  The unknowns are x = [rho(3), theta(3), a, b]; with the residual
 * r_ch = m (e^a C_ch + b - gt_ch), dr_ch = m e^a (dC_ch + C_ch da + db / e^a): relative to the rendered colour the exposure
 * parameters are two more Jacobian columns, J8[ch] = [J[ch][0..5], C_ch, 1 / e^a] (C: the forward's image; both 0 in the depth
 * row), under the SAME seeds s and curvatures h as above (the derivative of the opacity weight is neglected, as there).
 * gsaj_rasterize_pose_jacobian_loss8 -- the arguments of gsaj_rasterize_pose_jacobian_loss;
 *   gn8_partials [gsaj_pose_jac_partial_rows(W, H)][GSAJ_GN8_PARTIAL_FLOATS]: [0:36) H8 = sum h J8^T J8, the upper triangle by
 *   rows, [36:44) g8 = sum s J8, [44] loss, [45] L_rgb, [46] L_depth, [47:49) the exposure sums of the fused forward, [49:64) zero.
 *   GSAJ_LOSS_NO_EXPOSURE or a NULL exposure pointer is GSAJ_ERR_INVALID_ARGUMENT, as are the argument errors of the 6-form.
 * gsaj_pose_gn8_step -- gsaj_pose_gn_step on 8 unknowns.  gn8_state: GSAJ_GN8_STATE_FLOATS floats; [0:104) as gn_state, then
 *     [104:140) accepted H8   [140:148) accepted g8   [148:150) accepted exposure a, b   (and [78:80) the exposure step x[6], x[7])
 *   Initialise as gn_state.  Accept saves the exposure [33:35) with the pose, reject restores it with the pose.  The 8x8 system
 *   (H8 + lambda diag(H8) + eps I) x = -g8 (eps from the mean of the 8 diagonal elements) is solved by Cholesky in fp64; W2C <-
 *   Exp(x[0:6]) W2C, a <- a + x[6], b <- b + x[7]; converged = |tau| < converged_threshold and max(|x[6]|, |x[7]|) <
 *   converged_threshold.  A non-positive pivot raises lambda and changes neither pose nor exposure; a non-zero skip word changes
 *   nothing. */
#define GSAJ_GN_PARTIAL_FLOATS 32
#define GSAJ_GN_STATE_FLOATS 136
#define GSAJ_GN8_PARTIAL_FLOATS 64
#define GSAJ_GN8_STATE_FLOATS 152
size_t gsaj_pose_jac_workspace_bytes(int P, int W, int H);
int gsaj_pose_jac_partial_rows(int W, int H);
int gsaj_rasterize_pose_jacobian(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D, const float *shs,
                                 const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                                 const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
                                 const float *projmatrix_raw, const float *campos, float tanfovx, float tanfovy, const int *radii,
                                 void *geom_ws, void *binning_ws, void *image_ws, void *jac_ws, float *jac_out /*NULL ok*/,
                                 float *out_color /*NULL ok*/, float *out_depth /*NULL ok*/, float *H_out /*[21] NULL ok*/,
                                 float *g_out /*[6] NULL ok*/, const float *seed_color, const float *seed_depth,
                                 const float *curv_color, const float *curv_depth, void *stream);
int gsaj_rasterize_pose_jacobian_loss(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                                      const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                      const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                      const float *projmatrix, const float *projmatrix_raw, const float *campos, float tanfovx,
                                      float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                      void *jac_ws, int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                      const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                      const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float irls_delta,
                                      float *gn_partials, float *jac_out /*NULL ok*/, void *stream);
int gsaj_gn_state_floats(void);
int gsaj_pose_gn_step(const float *gn_partials, int n_partials, float lambda_init, float nu, float lambda_min, float lambda_max,
                      float converged_threshold, const float *projection_matrix, float *gn_state, const uint32_t *skip,
                      void *stream);
int gsaj_rasterize_pose_jacobian_loss8(int P, int D, int M, int R, const float *bg, int W, int H, const float *means3D,
                                       const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                       const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                       const float *projmatrix, const float *projmatrix_raw, const float *campos, float tanfovx,
                                       float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                       void *jac_ws, int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                       const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                       const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b, float irls_delta,
                                       float *gn8_partials, float *jac_out /*NULL ok*/, void *stream);
int gsaj_gn8_state_floats(void);
int gsaj_pose_gn8_step(const float *gn8_partials, int n_partials, float lambda_init, float nu, float lambda_min, float lambda_max,
                       float converged_threshold, const float *projection_matrix, float *gn8_state, const uint32_t *skip,
                       void *stream);

/* The same for K views of ONE map in one set of launches (gridDim.y = K): K independent solves -- the keyframe poses of a window
 * against a fixed map, or K start poses of one frame.  The loss-fused forms only; a tile band on any view is not supported.
 * gsaj_rasterize_pose_jacobian_loss_batch / _loss8_batch -- the arguments of gsaj_rasterize_backward_loss_batch up to the loss
 *   group (on a FINISHED gsaj_rasterize_forward[_loss]_batch of the same K views: 256-byte aligned blocks, `capacity` as there),
 *   then jac_ws (gsaj_pose_jac_batch_workspace_bytes(K, P, W, H) bytes, 256-byte aligned, no initialisation needed), irls_delta, gn_partials
 *   [K][gsaj_pose_jac_partial_rows(W, H)][GSAJ_GN_PARTIAL_FLOATS | GSAJ_GN8_PARTIAL_FLOATS] and jac_out [K,H,W,4,6] or NULL.
 *   View v's rows are the bits of the single-view entry point on view v's blocks.  cov3D is read from the caller's cov3D_precomp
 *   or from view 0's geometry block, the only one a batched forward writes.  A view aborted on the device keeps its rows.
 *   K <= 0, misaligned blocks and, in the joint form, GSAJ_LOSS_NO_EXPOSURE or a NULL exposure: GSAJ_ERR_INVALID_ARGUMENT.
 * gsaj_pose_gn_step_batch / gsaj_pose_gn8_step_batch -- K workgroups, each gsaj_pose_gn_step / gsaj_pose_gn8_step on view v's
 *   n_partials rows, state v of gn_states [K, GSAJ_GN_STATE_FLOATS | GSAJ_GN8_STATE_FLOATS] and the skip word at skip + v *
 *   skip_stride_bytes; active [K] bytes or NULL (0: that state is not touched), as gsaj_pose_adam_step_batch.  The projection
 *   matrix and the LM scalars are shared.
 * gsaj_pose_gn_select -- *best (device int32) = the view of smallest accepted loss [81] among the views that are active, have
 *   accepted a pose ([82] != 0) and have a finite loss, ties to the lowest index, -1 if there is none; *best_loss (device) its
 *   loss (+inf if none).  state_floats: GSAJ_GN_STATE_FLOATS or GSAJ_GN8_STATE_FLOATS. */
size_t gsaj_pose_jac_batch_workspace_bytes(int K, int P, int W, int H);
int gsaj_rasterize_pose_jacobian_loss_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                            const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                            const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                            const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                            float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                            int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                            const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                            const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                            int exposure_stride, void *jac_ws, float irls_delta, float *gn_partials,
                                            float *jac_out /*NULL ok*/, void *stream);
int gsaj_rasterize_pose_jacobian_loss8_batch(int K, int P, int D, int M, int capacity, const float *bg, int W, int H, const float *means3D,
                                             const float *shs, const float *colors_precomp, const float *scales, float scale_modifier,
                                             const float *rotations, const float *cov3D_precomp, const float *viewmatrices,
                                             const float *projmatrices, const float *projmatrix_raw, const float *campos, float tanfovx,
                                             float tanfovy, const int *radii, void *geom_ws, void *binning_ws, void *image_ws,
                                             int loss_flags, float alpha, float rgb_boundary_threshold, const float *color,
                                             const float *depth, const float *opacity, const float *gt_color, const float *gt_depth,
                                             const uint8_t *grad_mask, const float *exposure_a, const float *exposure_b,
                                             int exposure_stride, void *jac_ws, float irls_delta, float *gn8_partials,
                                             float *jac_out /*NULL ok*/, void *stream);
int gsaj_pose_gn_step_batch(int K, const float *gn_partials, int n_partials, const uint8_t *active, float lambda_init, float nu,
                            float lambda_min, float lambda_max, float converged_threshold, const float *projection_matrix,
                            float *gn_states, const uint32_t *skip, size_t skip_stride_bytes, void *stream);
int gsaj_pose_gn8_step_batch(int K, const float *gn8_partials, int n_partials, const uint8_t *active, float lambda_init, float nu,
                             float lambda_min, float lambda_max, float converged_threshold, const float *projection_matrix,
                             float *gn8_states, const uint32_t *skip, size_t skip_stride_bytes, void *stream);
int gsaj_pose_gn_select(int K, const float *gn_states, int state_floats, const uint8_t *active, int *best, float *best_loss,
                        void *stream);

/* Coarse-to-fine: the image pyramid of a frame and the Levenberg-Marquardt state carried from one resolution to the next
 * (csrc/pyramid.hip).  Level 0 is the frame: colour [3,H,W] fp32, depth [H,W] fp32 or NULL, mask [H,W] bytes or NULL.  Level l of
 * 1..levels (levels <= GSAJ_PYRAMID_MAX_LEVELS) is W_l = W >> l by H_l = H >> l: a level-l pixel exists only where its whole
 * 2^l x 2^l block of level-0 pixels lies inside the image -- an odd last column or row is dropped, never partially averaged.
 * Level l from level l - 1, children p00 p01 / p10 p11 in row-major order, fp32, one rounding per operation:
 *   colour  0.25f * ((p00 + p01) + (p10 + p11))
 *   depth   a child is valid iff d > 0.0f (NaN and negatives are not).  No valid child: 0.  Otherwise dmin, dmax over the valid
 *           children; dmax - dmin > depth_edge_ratio * dmin: 0 (the pixel straddles a depth discontinuity and must not pull the
 *           pose); otherwise s * r[n], s = the valid children added in the order p00, p01, p10, p11, n their number,
 *           r = {1, 0.5f, (float)(1.0 / 3.0), 0.25f}.  A 0 is an invalid child of the next level.
 *   mask    the OR of the four children, non-zero written as 1
 * The packed pyramid holds levels 1..levels one after the other, each colour [3,H_l,W_l], then depth [H_l,W_l], then mask
 * [H_l,W_l] (the planes the frame has), every plane at a 256-byte aligned offset; the bytes between planes are never written.
 * gsaj_pyramid_bytes -- its size (0 for arguments gsaj_pyramid_build would refuse).
 * gsaj_pyramid_level -- host only: the size of level `level` (1..levels) and the byte offsets of its planes ((size_t)-1 for a plane
 *   the pyramid does not have); every output pointer may be NULL.
 * gsaj_pyramid_build -- all levels in ONE launch on `stream`, no host read, no atomics: every input element is read once, every
 *   output element written once, the bits are the same run to run.  `pyramid`: gsaj_pyramid_bytes(W, H, levels, depth != NULL,
 *   mask != NULL) bytes, 256-byte aligned, no initialisation needed.
 * gsaj_pose_gn_relevel -- a gn_state / gn8_state (above) taken to the next resolution: one launch of one wave, no host read.  If a
 *   pose has been accepted ([82] != 0), W2C [0:16) <- the accepted W2C [88:104) and, in the joint form, the exposure [33:35) <-
 *   [148:150): the last proposed pose, which no step has judged, is discarded -- a loss at another resolution cannot judge it;
 *   otherwise the pose stays.  The camera matrices [35:70) are refreshed from W2C and projection_matrix_next with the operations
 *   of gsaj_pose_gn_step; [80] <- lambda_init; zeroed: [81], [82], tau, |tau| and converged [70:78) (and [78:80) in the joint
 *   form), [85:88), the accepted H and g; [88:104) <- W2C and, in the joint form, [148:150) <- the exposure.  The step counters
 *   [83], [84] are kept: they count over the frame.  With [82] = 0 the next gsaj_pose_gn_step accepts its loss as the new
 *   baseline.  skip: as in gsaj_pose_gn_step -- a non-zero word (the level just finished was aborted) changes nothing.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: levels outside 1..GSAJ_PYRAMID_MAX_LEVELS, W >> levels < 1 or
 * H >> levels < 1, a NULL colour or pyramid, depth_edge_ratio < 0 or not finite; a NULL gn_state or projection_matrix_next, a
 * state_floats that is neither GSAJ_GN_STATE_FLOATS nor GSAJ_GN8_STATE_FLOATS, lambda_init <= 0. */
#define GSAJ_PYRAMID_MAX_LEVELS 4
size_t gsaj_pyramid_bytes(int W, int H, int levels, int has_depth, int has_mask);
int gsaj_pyramid_level(int W, int H, int levels, int has_depth, int has_mask, int level, int *W_l, int *H_l, size_t *color_off,
                       size_t *depth_off, size_t *mask_off);
int gsaj_pyramid_build(int W, int H, int levels, const float *color, const float *depth /*NULL ok*/, const uint8_t *mask /*NULL ok*/,
                       float depth_edge_ratio, void *pyramid /*dev*/, void *stream);
int gsaj_pose_gn_relevel(float *gn_state, int state_floats /*GSAJ_GN_STATE_FLOATS | GSAJ_GN8_STATE_FLOATS*/,
                         const float *projection_matrix_next, float lambda_init, const uint32_t *skip, void *stream);

/* ---- frame ingest: a camera frame from bytes to the tensors the trackers read (csrc/ingest.hip) ----------------------------------
 * What the reference's datasets do per frame on the host (utils/dataset.py:257-278, :370-386, :499-513: cv2.remap of a distorted
 * image, image / 255.0, clamp, permute, the float32 upload; depth / depth_scale), on the device: the bytes are uploaded as bytes.
 *
 * gsaj_undistort_map -- once per camera, fp64, what cv2.initUndistortRectifyMap(K, dist, R, newK, (W, H), CV_32FC1) is documented
 *   to compute.  K_src = host {fx, fy, cx, cy} of the distorted camera, dist = host {k1, k2, p1, p2, k3}, iR = host, the 3 x 3
 *   inverse of newK R, row-major (an input: the caller inverts).  For output pixel (u, v), every operation in fp64, one rounding
 *   each, no fused multiply-add, every product and sum evaluated left to right as written:
 *     X = iR[0] u + iR[1] v + iR[2];  Y = iR[3] u + iR[4] v + iR[5];  Wq = iR[6] u + iR[7] v + iR[8]
 *     x = X / Wq;  y = Y / Wq;  r2 = x x + y y
 *     rad = 1 + k1 r2 + k2 (r2 r2) + k3 ((r2 r2) r2)
 *     xd = x rad + 2 p1 x y + p2 (r2 + 2 x x)            (2 p1 x y is ((2 p1) x) y, 2 x x is (2 x) x)
 *     yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y
 *     map_x[v][u] = (float)(fx xd + cx);  map_y[v][u] = (float)(fy yd + cy)
 * gsaj_frame_ingest -- once per frame, ONE launch for colour and depth.  src: bytes [Hs][Ws][channels], rows src_stride bytes
 *   apart; channels 1 (the grey byte goes to all three planes, cvtColor GRAY2BGR), 3, or 4 (the fourth byte is ignored).  Plane c of
 *   out_color [3,H,W] reads channel c, with GSAJ_INGEST_BGR channel 2 - c (a grey image has one channel: the flag changes nothing).
 *   fp32, one rounding per operation, no fused multiply-add:
 *   without a map (Ws = W, Hs = H):  out = min(max((float)byte / 255.0f, 0), 1) -- a true division: (float)k / 255.0f equals
 *     (float)(k / 255.0) for all 256 bytes, which a multiplication by a reciprocal does not.
 *   with map_x, map_y [H,W] (pixel coordinates in the source), an exact bilinear with a constant border of 0:
 *     a coordinate pair that is not finite or lies outside [-1, Ws] x [-1, Hs] gives 0 (decided on the floats); otherwise
 *     x0 = floorf(mx), ax = mx - x0, bx = 1.0f - ax, and y0, ay, by likewise; the taps p00 p01 / p10 p11 at (x0, y0), (x0 + 1, y0),
 *     (x0, y0 + 1), (x0 + 1, y0 + 1) as floats, a tap outside 0 <= x < Ws, 0 <= y < Hs being 0.0f;
 *     top = p00 bx + p01 ax;  bot = p10 bx + p11 ax;  val = top by + bot ay;  with GSAJ_INGEST_ROUND_U8 val = floorf(val + 0.5f),
 *     the k / 255 lattice a uint8 remap output lives on;  out = min(max(val / 255.0f, 0), 1).
 *   depth_raw (may be NULL, then out_depth is NULL too): uint16 [H][W], rows depth_stride bytes apart, never remapped (the reference
 *     does not remap it either): out_depth [H,W] = (float)((double)d / depth_scale), with GSAJ_INGEST_DEPTH_MUL (float)((double)d *
 *     depth_scale) (a RealSense's depth unit) -- NumPy's float64 result rounded to float32 once.
 *   Where W % 4 == 0 and out_color, out_depth, map_x, map_y are 16-byte aligned a thread owns four consecutive pixels of a row (16-byte
 *   stores and map loads; the source as one 4-byte aligned read where src and src_stride allow it, the depths as one 8-byte read
 *   where depth_raw and depth_stride allow it); otherwise one thread per pixel.  Both give the same bits.  No atomics: every output
 *   element is written once, the bits are the same run to run; nothing outside out_color and out_depth is written.
 * Bit parity with cv2.remap is NOT claimed: its uint8 path quantises the map to 1/32 pixel and interpolates with 15-bit integer
 * weights, so it differs from the exact bilinear by up to the local gradient x 1/64 pixel, plus rounding.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: a non-positive size (or W H, Ws Hs above INT_MAX); channels not 1, 3 or 4;
 * unknown flag bits; a NULL src, out_color, K_src, dist, iR, map_x or map_y of gsaj_undistort_map; src_stride < Ws channels; exactly
 * one of the two maps; no map and (Ws, Hs) != (W, H); depth_raw without out_depth or the reverse; with depth: depth_stride < 2 W or
 * odd, a depth_scale that is zero or not finite; an output or map pointer that is not 4-byte aligned. */
#define GSAJ_INGEST_BGR 1
#define GSAJ_INGEST_ROUND_U8 2
#define GSAJ_INGEST_DEPTH_MUL 4
int gsaj_undistort_map(int W, int H, const double *K_src /*host: fx fy cx cy*/, const double *dist /*host: k1 k2 p1 p2 k3*/,
                       const double *iR /*host, 9*/, float *map_x /*dev [H,W]*/, float *map_y /*dev [H,W]*/, void *stream);
int gsaj_frame_ingest(int W, int H, int Ws, int Hs, int channels, size_t src_stride, const uint8_t *src /*dev*/,
                      const float *map_x /*dev or NULL*/, const float *map_y /*dev or NULL*/,
                      const uint16_t *depth_raw /*dev or NULL*/, size_t depth_stride, double depth_scale, int flags,
                      float *out_color /*dev [3,H,W]*/, float *out_depth /*dev [H,W] or NULL*/, void *stream);

/* ---- stereo frames: rectify, semi-global matching, depth (csrc/stereo.hip; the byte remap in csrc/ingest.hip) -----------------------
 * What the reference's StereoDataset does per frame on the host (utils/dataset.py:365-393): cv2.remap of both grey images,
 * cv2.StereoSGBM (minDisparity 0, numDisparities 64, blockSize 20, uniquenessRatio 40), depth = bf / disparity.  The matcher below is
 * this library's OWN statement of semi-global matching in integer arithmetic, parametrised the way StereoSGBM is; bit parity with
 * OpenCV is NOT claimed (its pixel cost, its defaults and its path set are not restated here).  tests/stereo_restated.py restates it
 * in NumPy; all of it but the depth line is integer, so the device equals the restatement bit for bit.
 *
 * gsaj_rectify_u8 -- grey bytes [Hs][Ws] (rows src_stride apart) through map_x, map_y [H,W] to bytes out [H][W] (rows out_stride
 *   apart): exactly gsaj_frame_ingest's bilinear of a one-channel image with GSAJ_INGEST_ROUND_U8, stopped before the division:
 *   out = (uint8)min(floorf(val + 0.5f), 255).  Without maps (Ws = W, Hs = H) the byte is copied.  out_color (may be NULL): fp32
 *   [3,H,W], min(max((float)out / 255.0f, 0), 1) in all three planes -- the bits gsaj_frame_ingest gives the same image.
 *
 * gsaj_stereo_match -- left, right: rectified grey bytes [H][W].  D in {16, 32, 64, 128} disparities, D < W <= 4096; block radius r in
 *   [0, 15] (a (2r+1)^2 window); penalties 0 <= P1 < P2 <= 1024; paths 4 or 8; uniqueness u in [0, 99]; lr_max_diff >= -1 (-1: no
 *   left-right check).  (StereoSGBM's blockSize 20 is r = 10; 2 and 5 are what OpenCV is understood to substitute for unset
 *   penalties -- unverified, hence parameters.)  All integers:
 *   a. prefilter   P(x,y) = clamp(gx, -15, 15) + 15,  gx = (I(x+1,y-1) - I(x-1,y-1)) + 2 (I(x+1,y) - I(x-1,y)) + (I(x+1,y+1) -
 *                  I(x-1,y+1)), coordinates clamped to the image
 *   b. pixel cost  pc(x,y,d) = |P_L(x,y) - P_R(max(x-d, 0), y)|                                              (0..30)
 *   c. block cost  C(x,y,d) = sum of pc(x',y',d) over |x'-x| <= r, |y'-y| <= r, x' and y' clamped to the image   (<= 28 830)
 *   d. valid       only x in [D, W-1] carries a result; every x < D is invalid
 *   e. paths       over the valid region, per direction rho -- paths = 4: (1,0) (-1,0) (0,1) (0,-1); paths = 8: also (1,1) (-1,1)
 *                  (1,-1) (-1,-1).  With q = p - rho and m(q) = min_k L(q,k):
 *                    L(p,d) = C(p,d) + min(L(q,d), L(q,d-1) + P1, L(q,d+1) + P1, m(q) + P2) - m(q)
 *                  terms with d-1 or d+1 outside [0, D-1] are absent; L(p,.) = C(p,.) where q lies outside the valid region.
 *                  S = the sum of L over the directions, in 32 bits (it exceeds 65 535)
 *   f. winner      d* = argmin_d S(p,d), the lowest d among equals.  p is invalid if some d with |d - d*| > 1 has
 *                  S(p,d) (100 - u) < S(p,d*) 100
 *   g. sub-pixel   for 0 < d* < D-1: den = max(S(d*-1) + S(d*+1) - 2 S(d*), 1), d16 = 16 d* + ((S(d*-1) - S(d*+1)) 16 + den) / (2 den),
 *                  C integer division (towards zero); otherwise d16 = 16 d*
 *   h. left-right  (lr_max_diff >= 0) disp2(x2) of a row = the d* of the left pixel that passed f, has x - d* = x2 and the smallest
 *                  S(x,d*), the largest x among equals; absent if there is none.  A candidate delta of a left pixel FAILS when
 *                  x - delta >= 0, disp2(x - delta) is present and |disp2(x - delta) - delta| > lr_max_diff; the pixel is invalid if
 *                  both delta = d16 >> 4 and delta = (d16 + 15) >> 4 fail.  No result depends on the order threads run in
 *   i. output      disp16 int16 [H,W], -16 at every invalid pixel.  out_depth (may be NULL) fp32 [H,W], the reference's lines in its
 *                  float64: delta = d16 / 16.0; delta == 0 -> 1e10; z = bf / delta; z < 0 -> 0; one rounding to fp32.  So an
 *                  invalid pixel gives 0 and d16 = 0 gives (float)(bf 1e-10).  bf: baseline x focal length, positive and finite
 *   No speckle filter (the reference leaves it at 0), minDisparity 0 only.
 *   workspace: gsaj_stereo_workspace_bytes(W, H, D, paths, &bytes) bytes, 256-byte aligned; it holds the prefiltered images, C as
 *   uint16 [H,W,D] and S as uint32 [H,W,D] (d innermost), and S is zeroed on the stream inside the call: no allocation, no host
 *   synchronisation.  stages: 0 = everything; otherwise the GSAJ_STEREO_STAGE_* to run, each on what the workspace already holds
 *   (measurement and tests: tools/stereo_bench.py times the stages one by one, a test may plant S and run the winner alone).
 * gsaj_debug_stereo_offsets -- tests and tools only, host only: the byte offsets of C and S in the workspace; both stay there
 *   after a call.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: any parameter outside the ranges above, W * H * D above INT_MAX, unknown
 * stage bits, a NULL image, workspace, disp16 or bytes, a row stride below its row, a misaligned workspace (256), disp16 (2) or float
 * pointer (4), out_depth with a bf that is not positive and finite; for gsaj_rectify_u8 the errors of gsaj_frame_ingest's remap.
 * GSAJ_ERR_WORKSPACE_TOO_SMALL: workspace_bytes below gsaj_stereo_workspace_bytes. */
#define GSAJ_STEREO_STAGE_COST 1
#define GSAJ_STEREO_STAGE_PATHS 2
#define GSAJ_STEREO_STAGE_WINNER 4
int gsaj_stereo_workspace_bytes(int W, int H, int D, int paths, size_t *bytes);
int gsaj_debug_stereo_offsets(int W, int H, int D, int paths, size_t *cost_off, size_t *sum_off);
int gsaj_rectify_u8(int W, int H, int Ws, int Hs, size_t src_stride, const uint8_t *src /*dev*/, const float *map_x /*dev or NULL*/,
                    const float *map_y /*dev or NULL*/, uint8_t *out /*dev*/, size_t out_stride, float *out_color /*dev [3,H,W] or NULL*/,
                    void *stream);
int gsaj_stereo_match(int W, int H, const uint8_t *left /*dev*/, size_t left_stride, const uint8_t *right /*dev*/, size_t right_stride,
                      int D, int r, int P1, int P2, int paths, int uniqueness, int lr_max_diff, int stages, void *workspace /*dev*/,
                      size_t workspace_bytes, int16_t *disp16 /*dev [H,W]*/, float *out_depth /*dev [H,W] or NULL*/, double bf,
                      void *stream);

/* ---- distCUDA2 -------------------------------------------------------------------
 * simple_knn._C.distCUDA2 (reference submodules/simple-knn/simple_knn.cu:45-220, spatial.cu): for P points
 * [P,3] the mean of the squared distances to the 3 nearest other points -> mean_dists [P].  Exact search;
 * fewer than 3 neighbours leaves FLT_MAX terms (-> inf) as in the reference.  No host synchronisation.
 * knn_ws: gsaj_dist2_workspace_bytes(P) bytes, no initialisation needed (the call zeroes its ticket on the stream). */
size_t gsaj_dist2_workspace_bytes(int P);
int gsaj_dist2(int P, const float *points, float *mean_dists, void *knn_ws, void *stream);
/* Tests only: the Morton order gsaj_dist2 left in its workspace -- the 30-bit codes in sorted order and the point index of every
 * position (device arrays [P]; blocking).  The sort is this library's own stable radix sort (thrust::sort_by_key in the reference,
 * simple_knn.cu:211): ascending codes, equal codes in ascending index order. */
int gsaj_debug_dist2_order(int P, void *knn_ws, uint32_t *codes_sorted, uint32_t *idx_sorted, void *stream);

/* ---- new Gaussians from a keyframe (csrc/seed.hip) -------------------------------------------------------------------
 * The reference grows its map from every keyframe through the host: slam_frontend.py:57-108 (add_new_keyframe: the depth to seed
 * from), slam_utils.py:131-142 (get_median_depth), gaussian_model.py:183-279 (create_pcd_from_image[_and_depth]: Open3D RGBD image
 * -> point cloud -> random_down_sample -> RGB2SH, distCUDA2 scales, unit rotations, opacity 0.5).  Here the same steps stay on the
 * device; the only host read is the 8-byte gsaj_seed_count, which sizes the new tensors.  Images are [H,W] fp32 (depth, opacity,
 * noise), [3,H,W] fp32 (gt_image / image), masks [H,W] bytes (non-zero = keep).  No float atomics: every result is bit-reproducible.
 * seed_ws: gsaj_seed_workspace_bytes(W, H) bytes, no initialisation needed; it carries state from gsaj_seed_select to
 * gsaj_seed_count / gsaj_seed_gaussians.
 *
 * gsaj_depth_stats = get_median_depth: valid = depth > 0 [and opacity > opacity_min] [and mask] [and (r + g) + b > rgb_threshold,
 *   with gt_image]; out_stats (dev float[4]) = {median, std, n_valid, 0}; out_valid (dev bytes [H,W], may be NULL) = the valid mask.
 *   median = torch.median = the LOWER median, order statistic (n_valid - 1) / 2, exact (integer radix select over order-preserving
 *   keys); std = torch.std (unbiased, n - 1), summed in fp64 in a fixed order and rounded once.  n_valid == 0 (the reference
 *   raises): median = std = 0.  n_valid == 1: std = NaN, as torch.std.
 * gsaj_keyframe_depth_prior = the monocular branch of add_new_keyframe (:89-103): statistics as above with opacity > 0.95 and the
 *   colour mask; invalid = depth > med + std or depth < med - std or not valid; out = (invalid ? med : depth) + noise * (invalid ?
 *   0.5 std : 0.2 std); out = 0 where the colour mask fails.  noise: the caller's N(0,1) image or NULL for none.
 * gsaj_seed_select: valid = 0 < depth < depth_trunc [and (r + g) + b > rgb_threshold] (Open3D create_from_color_and_depth(depth_scale
 *   1, depth_trunc) + project_valid_depth_only); m = (size_t)(n_valid * (1.0 / downsample_factor)) in double (random_down_sample);
 *   the chosen set is the m valid pixels with the smallest key, where, for pixel index i = v * W + u,
 *       key(i) = mix(i XOR mix(seed)),   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   in 32-bit unsigned arithmetic.  mix is a bijection, so no two pixels share a key and there is no tie-break rule.  The set is a
 *   uniform m-subset of the valid pixels, reproducible from `seed`; it is NOT Open3D's subset (an unseeded mt19937 shuffle).  The
 *   pixels are listed in ascending pixel order.  downsample_factor >= 1.
 * gsaj_seed_count: blocking; n_valid and m of the last gsaj_seed_select on this workspace.
 * gsaj_seed_gaussians: for the m chosen pixels, in pixel order: xyz [m,3] = inverse(W2C) (x, y, z, 1) with z = depth, x = (u - cx) z /
 *   fx, y = (v - cy) z / fy, evaluated in fp64 on the fp32 inputs and rounded once (w2c: dev, 16 row-major floats, inverted as a general
 *   affine map; the first 16 floats of a pose_state qualify); f_dc [m,3] = (q / 255 - 0.5) / C0 with q = (uint8)(clamp(exp(a) image + b, 0,
 *   1) * 255), truncated (exposure_ab: dev {a, b} or NULL = {0, 0}; pose_state + 33 qualifies); f_rest [m, (sh_coeffs - 1) * 3] = 0;
 *   scaling [m, isotropic ? 1 : 3] = log(sqrt(max(dist2, 1e-7) * point_size)), dist2 = gsaj_dist2 of the new points (knn_ws:
 *   gsaj_dist2_workspace_bytes(m)); with adaptive != 0 point_size becomes min(0.05, point_size * median of ALL pixels of `depth`, zeros
 *   included, the mean of the two middle values: np.median), found on the device; rotation [m,4] = (1, 0, 0, 0); opacity [m] = 0 =
 *   inverse_sigmoid(0.5).  m must be the m of gsaj_seed_count; depth must be the image given to gsaj_seed_select.  m < 4 leaves
 *   FLT_MAX terms in dist2 (see gsaj_dist2), hence huge or infinite scales, as in the reference; m == 0 is a successful no-op. */
size_t gsaj_seed_workspace_bytes(int W, int H);
int gsaj_depth_stats(int W, int H, const float *depth, const float *opacity /*or NULL*/, float opacity_min,
                     const uint8_t *mask /*or NULL*/, const float *gt_image /*or NULL*/, float rgb_threshold,
                     float *out_stats /*dev [4]*/, uint8_t *out_valid /*dev [H,W] or NULL*/, void *seed_ws, void *stream);
int gsaj_keyframe_depth_prior(int W, int H, const float *depth, const float *opacity, const float *gt_image, float rgb_threshold,
                              const float *noise /*or NULL*/, float *out_depth /*dev [H,W]*/, float *out_stats /*dev [4]*/,
                              void *seed_ws, void *stream);
int gsaj_seed_select(int W, int H, const float *depth, const float *gt_image /*or NULL*/, float rgb_threshold, float depth_trunc,
                     double downsample_factor, uint32_t seed, void *seed_ws, void *stream);
int gsaj_seed_count(const void *seed_ws, void *stream, int *n_valid /*host*/, int *m /*host*/);
int gsaj_seed_gaussians(int m, int W, int H, const float *depth, const float *image, const float *exposure_ab /*dev [2] or NULL*/,
                        const float *w2c /*dev [16]*/, double fx, double fy, double cx, double cy, float point_size, int adaptive,
                        int sh_coeffs, int isotropic, float *xyz, float *f_dc, float *f_rest, float *scaling, float *rotation,
                        float *opacity, void *seed_ws, void *knn_ws, void *stream);
/* Tests only: the first m pixel indices (v * W + u, ascending) the last gsaj_seed_select left in the workspace -> pixels (dev [m]). */
int gsaj_debug_seed_pixels(int W, int H, int m, const void *seed_ws, uint32_t *pixels, void *stream);

/* ---- the tracking gradient mask of a frame (frame.hip) -------------------------------------------------------------------------
 * The per-pixel grad_mask the tracking loss reads, computed from the frame's colour image on the device (reference
 * utils/camera_utils.py:115-144 Camera.compute_grad_mask on utils/slam_utils.py:4-38 image_gradient / image_gradient_mask).
 * image: dev [3,H,W] fp32, W, H >= 2.  One fp32 rounding per operation, no fused multiply-add:
 *   gray = ((r + g) + b) / 3 (a true division); p = gray reflect-padded by one pixel (the edge pixel is not repeated);
 *   gv = ((3 p[-1,-1] + 10 p[-1,0]) + 3 p[-1,+1]) - ((3 p[+1,-1] + 10 p[+1,0]) + 3 p[+1,+1])) / 32  (p[row, column]),
 *   gh = ((3 p[-1,-1] + 10 p[0,-1]) + 3 p[+1,-1]) - ((3 p[-1,+1] + 10 p[0,+1]) + 3 p[+1,+1])) / 32;
 *   a pixel is valid iff all nine padded neighbours have |p| > 0.01, otherwise gv = gh = 0;
 *   intensity I = sqrt(gv gv + gh gh), correctly rounded.  (The reference's conv2d sums the nine taps in an order of its own; any
 *   order is within 16 * 2^-24 * max|gray| of this one.)
 * gsaj_grad_intensity: out_intensity [H,W] = I.
 * gsaj_grad_mask, blocks == 0 (every dataset type but "replica"): t = med * edge_threshold with med the LOWER median of all H W
 *   intensities, zeros included (order statistic (H W - 1) / 2, torch.median); mask = I > t.  out_mask_u8 [H,W] = 0 / 1;
 *   out_mask_f32 [H,W] (may be NULL) = 0.0 / 1.0.  An intensity pass, a radix select and one threshold kernel that reads the
 *   selected value from device memory: no host read, no synchronisation.  ws: gsaj_grad_mask_workspace_bytes(W, H) bytes, no
 *   initialisation needed.
 * blocks != 0 ("replica"): a 32 x 32 grid of blocks of bh = H / 32 rows and bw = W / 32 columns (integer division) anchored at
 *   (0, 0); per block t = med * edge_threshold with med the lower median of the block's bh bw intensities; out_mask_f32 is what the
 *   reference leaves in Camera.grad_mask, a FLOAT image: 1 where I > t and t < 1 (the reference writes the ones first and then
 *   zeroes everything <= t, the ones included), else 0; rows >= 32 bh and columns >= 32 bw are never visited and keep I.
 *   out_mask_u8 = (uint8)out_mask_f32, truncated: the byte the loss kernels read when handed that float image.  One kernel, one
 *   workgroup per block; ws may be NULL.  W < 32 or H < 32 (empty blocks: the reference raises) and blocks of more than 4096 pixels,
 *   or 4608 with their one-pixel halo (what a workgroup holds in LDS; 1920 x 1080 has 1980), return GSAJ_ERR_INVALID_ARGUMENT
 *   before anything is launched.
 * Integer counters only: results are bit-reproducible. */
size_t gsaj_grad_mask_workspace_bytes(int W, int H);
int gsaj_grad_intensity(int W, int H, const float *image, float *out_intensity /*dev [H,W]*/, void *stream);
int gsaj_grad_mask(int W, int H, const float *image, float edge_threshold, int blocks, uint8_t *out_mask_u8 /*dev [H,W]*/,
                   float *out_mask_f32 /*dev [H,W] or NULL*/, void *ws, void *stream);

/* ---- covisibility of the keyframe window (csrc/covis.hip) ------------------------------
 * What the reference keeps as occ_aware_visibility[kf] = (n_touched > 0).long(), one int64 [P] vector per keyframe
 * (utils/slam_backend.py:236-240), is ONE uint32 word per Gaussian here: bit s of words[i] = "Gaussian i was touched
 * (n_touched > 0) in the view held in slot s".  At most GSAJ_COVIS_MAX_SLOTS views; which keyframe sits in which slot is
 * the caller's book-keeping.  All results are exact integers, independent of the launch geometry; nothing below
 * synchronises with the host.
 *
 * gsaj_covis_pack: K rows n_touched [K,P] (device int32) go to the K DISTINCT slots `slots` (host [K], each 0..31):
 *   words[i] = (words[i] & ~(clear_mask | bits of slots)) | (bit slots[k] where n_touched[k][i] > 0).
 *   clear_mask = 0xFFFFFFFF rebuilds every word from the rows (the old words are not read); K = 1 updates one slot;
 *   a clear_mask bit also wipes a slot that is not written (a dropped keyframe).
 * gsaj_covis_query: one pass over the P words.  The query set is {i : cur_n_touched[i] > 0} when cur_n_touched is given
 *   (device int32 [P]; query_slot is ignored), else {i : bit query_slot of words[i]}.  out (device int32 [65]), for
 *   every slot s in slot_mask:  out[s] = |query & slot s|,  out[32 + s] = |slot s|;  out[64] = |query|;  entries of
 *   slots outside slot_mask are 0.  out is overwritten whatever it held.  A union is |a| + |b| - |a & b|.
 * gsaj_covis_prune_mask: n_obs[i] = popcount(words[i] & window_mask) (written when n_obs is given);
 *   to_prune[i] = n_obs[i] <= max_obs && (unique_kfIDs == NULL || unique_kfIDs[i] >= kf_id_min); *n_pruned = number of
 *   ones in to_prune.  The reference's two modes (utils/slam_backend.py:252-263): "odometry" max_obs = 2, no ids
 *   (n_obs < 3); "slam" max_obs = 3, kf_id_min = the third-newest keyframe of the window, or 0 while not initialised.
 *   Only the mask and its count are produced; no row of the map is removed.
 * GSAJ_ERR_INVALID_ARGUMENT: P <= 0, K outside 1..32, a slot outside 0..31 or repeated, a null pointer (cur_n_touched,
 *   unique_kfIDs and n_obs may be NULL). */
#define GSAJ_COVIS_MAX_SLOTS 32
int gsaj_covis_pack(int K, int P, const int *n_touched /*dev [K,P]*/, const int *slots /*host [K]*/, uint32_t clear_mask,
                    uint32_t *words /*dev [P]*/, void *stream);
int gsaj_covis_query(int P, const uint32_t *words, const int *cur_n_touched /*dev [P] or NULL*/, int query_slot,
                     uint32_t slot_mask, int *out /*dev int32 [65]*/, void *stream);
int gsaj_covis_prune_mask(int P, const uint32_t *words, uint32_t window_mask, const int *unique_kfIDs /*dev [P] or NULL*/,
                          int kf_id_min, int max_obs, uint8_t *to_prune /*dev [P]*/, int *n_obs /*dev [P] or NULL*/,
                          int *n_pruned /*dev [1]*/, void *stream);

/* ---- removing rows of the map under a mask (csrc/compact.hip) ---------------------------
 * The rows are moved by the one mover of csrc/row_move.h, which gsaj_densify_rows below calls too.
 * The reference's prune_points (gaussian_splatting/scene/gaussian_model.py:559-597) indexes every parameter, Adam moment and
 * bookkeeping vector with one boolean mask, t[mask] each.  Here ONE pass over the mask plans the move and ONE launch moves the
 * kept rows of up to GSAJ_COMPACT_MAX_TENSORS tensors.  keep(i) = (mask[i] != 0) != (mask_is_remove != 0) -- any non-zero byte
 * is set; P' = number of kept rows.
 *
 * gsaj_compact_plan: counts the kept rows per block of 256 and scans the counts into block offsets.  No host read.
 *   compact_ws: gsaj_compact_workspace_bytes(P) bytes, P / 256 + O(1) words, no initialisation needed.  The plan remembers the mask's ADDRESS: the mask
 *   must stay where it is, unchanged, until the last gsaj_compact_rows of the plan has run.
 * gsaj_compact_count: *n_kept = P' (host).  The one blocking read, 4 bytes; a caller who knows P' already need not call it.
 * gsaj_compact_rows: for every t < n_tensors, dst[t] = the kept rows of src[t], row_bytes[t] bytes each, in the STABLE order
 *   (what t[keep] gives, bit for bit).  dst[t] holds P' rows; nothing outside those rows is written; src and mask are not
 *   modified.  P is the plan's P: with any other value nothing is read or written.  With P' = 0 nothing is written either
 *   (every workgroup returns at once); a caller who knows P' = 0 launches nothing, as gsaj.pruning does.  A plan stays valid
 *   until its workspace is reused; several gsaj_compact_rows calls may follow one plan.  src[t] and dst[t] must not overlap:
 *   destinations precede sources in a stable compaction, so an in-place form would race between workgroups.  A workspace
 *   that is no plan's is harmless as far as the mover goes: a block whose offsets differ by more than 256 rows, which no plan
 *   produces, moves nothing (as in gsaj_densify_rows; not observable with a valid plan).
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: P <= 0, a null pointer (in src / dst too), n_tensors outside
 *   1..GSAJ_COMPACT_MAX_TENSORS, a row size that is not a positive multiple of 4 or exceeds 4096, src[t] == dst[t]. */
#define GSAJ_COMPACT_MAX_TENSORS 32
size_t gsaj_compact_workspace_bytes(int P);
int gsaj_compact_plan(int P, const uint8_t *mask /*dev [P]*/, int mask_is_remove, void *compact_ws, void *stream);
int gsaj_compact_count(const void *compact_ws, void *stream, int *n_kept /*host*/);
int gsaj_compact_rows(int P, int n_tensors, const void *const *src /*host [n] of dev*/, void *const *dst /*host [n] of dev*/,
                      const int *row_bytes /*host [n]*/, const void *compact_ws, void *stream);

/* ---- map densification: clone, split and prune from one plan (csrc/densify_prune.hip) --------------------------------------------
 * The rows are moved by the one mover of csrc/row_move.h, as in gsaj_compact_rows above: the two tables have one size and one set of limits.
 * The reference's densify_and_prune (gaussian_splatting/scene/gaussian_model.py:599-765: densify_and_clone, densify_and_split with
 * its prune of the parents, and the final prune_points) as one classification of the P source rows and one move of every tensor.
 * All comparisons are fp32; the caller rounds every threshold to fp32 once: t_dense = fl32(percent_dense * extent),
 * t_big = fl32(0.1 * extent), grad_threshold, min_opacity.  Per row i: g = accum[i] / denom[i] with NaN -> 0 (denom == NULL:
 * g = accum[i] for i < n_grads, else 0 -- the padded_grad of densify_and_split), m = max_j exp(scaling[i][j]), o = sigmoid(opacity[i]).
 *   clone  (stage GSAJ_DENSIFY_CLONE):  |g| >= grad_threshold and m <= t_dense
 *   split  (stage GSAJ_DENSIFY_SPLIT):  g >= grad_threshold and m > t_dense; the parent leaves, N children enter
 *   prune  (stage GSAJ_DENSIFY_PRUNE):  a row goes if o < min_opacity, or if size_rule and (size_all or m > t_big); a clone
 *          stands or falls with its original; a child uses its parent's opacity and its own m = max_j exp(log(exp(s_ij) / d)),
 *          d = fl32(0.8 N), and the N children of a parent stand or fall together.
 * Kept quirks of the reference: size_rule is bool(max_screen_size), so None and 0 switch the size terms off; size_all is
 * 0 > max_screen_size, the reference's max_radii2D > max_screen_size evaluated on the zeros densification_postfix has just
 * written (true only for a negative size); the clone test takes |g| and the split test g; a zero quaternion gives NaN children.
 * grad_threshold must be greater than 0 (at or below 0 the reference would split the clones it has just appended).
 * code [P]: bit 0 the original is emitted, bit 1 a clone, bit 2 the children.  Output order (the reference's cat, prune, prune):
 * kept originals not split, kept clones, then the kept children of copy 0, copy 1, ... copy N - 1, each in source-row order.
 * gsaj_densify_counts: the one blocking read, 16 bytes: {originals, clones, children per copy, P''}, P'' = originals + clones +
 *   N children.
 * gsaj_densify_rows: dst[t] [P'', row_bytes[t]] from src[t] [P, row_bytes[t]]: an original keeps its row; a new row (clone,
 *   child) gets its parent's row, or zeros where zero_new[t] is set (Adam moments).  src[t] != dst[t].  Several calls may follow one plan.
 * gsaj_densify_children: overwrites the child rows of dst_xyz [P'',3] and dst_scaling [P'',S] with
 *   R(q_i) (exp(s_i) o z_{i,n}) + xyz_i (R: the reference's build_rotation, normalised by the fp32 norm; S = 1: the one scale
 *   multiplies the three components) and log(exp(s_i) / d).  noise [N,P,3] is indexed by SOURCE row; NULL: Philox4x32-10 with
 *   key (seed low, seed high) and counter (i, n, 0, 0): u1 = ((x0 >> 9) + 0.5) 2^-23, u2 = (x1 >> 8) 2^-24, r = sqrt(-2 ln u1),
 *   z0 = r cos(2 pi u2), z1 = r sin(2 pi u2), z2 from (x2, x3) the same way, cosine branch.  gsaj_densify_noise writes exactly
 *   those draws for every (n, i).  They depend on (seed, i, n) only.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: P <= 0 or P (N + 1) > INT_MAX, S not 1 or 3, N outside
 *   1..GSAJ_DENSIFY_MAX_SPLIT, grad_threshold not greater than 0, stages outside the mask, n_grads outside 0..P without denom,
 *   a null pointer (noise and denom excepted), n_tensors outside 1..GSAJ_DENSIFY_MAX_TENSORS, a row size that is not a positive
 *   multiple of 4 or exceeds 4096, a source equal to its destination. */
#define GSAJ_DENSIFY_MAX_TENSORS 32
#define GSAJ_DENSIFY_MAX_SPLIT 4
#define GSAJ_DENSIFY_CLONE 1
#define GSAJ_DENSIFY_SPLIT 2
#define GSAJ_DENSIFY_PRUNE 4
/* densify_ws: gsaj_densify_workspace_bytes(P, N) bytes, no initialisation needed; gsaj_densify_plan writes it and `code`, the other calls read both. */
size_t gsaj_densify_workspace_bytes(int P, int N);
int gsaj_densify_plan(int P, int S, int N, int stages, const float *accum /*dev [P]*/, const float *denom /*dev [P] or NULL*/,
                      int n_grads, const float *scaling /*dev [P,S]*/, const float *opacity /*dev [P]*/, float grad_threshold,
                      float t_dense, float t_big, float min_opacity, int size_rule, int size_all, uint8_t *code /*dev [P]*/,
                      void *densify_ws, void *stream);
int gsaj_densify_counts(const void *densify_ws, void *stream, int *counts /*host [4]*/);
int gsaj_densify_rows(int P, int N, int n_tensors, const void *const *src /*host [n] of dev*/, void *const *dst /*host [n] of dev*/,
                      const int *row_bytes /*host [n]*/, const int *zero_new /*host [n]*/, const uint8_t *code, const void *densify_ws,
                      void *stream);
int gsaj_densify_children(int P, int S, int N, const float *xyz, const float *scaling, const float *rotation,
                          const float *noise /*dev [N,P,3] or NULL*/, uint64_t seed, const uint8_t *code, const void *densify_ws,
                          float *dst_xyz /*dev [P'',3]*/, float *dst_scaling /*dev [P'',S]*/, void *stream);
int gsaj_densify_noise(int P, int N, uint64_t seed, float *out /*dev [N,P,3]*/, void *stream);

/* ---- map step: activation gradients, Adam and the opacity resets in one launch (csrc/map_step.hip) ------------------------------
 * The step of a mapping iteration on the Gaussian map (utils/slam_backend.py:299-311: the opacity reset, optimizer.step) over the six
 * raw parameters of gaussian_model.py, groups in the order xyz [P,3], f_dc [P,1,3], f_rest [P,M-1,3] (empty for M = 1), opacity [P,1],
 * scaling [P,scale_cols], rotation [P,4], each with exp_avg / exp_avg_sq of its shape, all updated IN PLACE.  One launch; every
 * element of every tensor is read once and written once; fp32 throughout, one rounding per operation (no contraction).
 * (a) The gradients arrive w.r.t. the ACTIVATED quantities, as the backwards leave them in the bucket: g_mean3D [P,3], g_sh [P,M,3],
 *   g_opacity [P], g_scale [P,3], g_rot [P,4].  The chain rule through the activations is closed form: xyz and SH identity (coefficient
 *   0 of a g_sh row is f_dc's, the rest f_rest's); opacity g s (1 - s), s = 1 / (1 + expf(-o)); scaling g_j expf(s_j), with
 *   scale_cols = 1 the three products summed, ((0 + 1) + 2), into the one column; rotation (g - qh (g . qh)) / n, n = max(|q|, 1e-12),
 *   qh = q / n, the dot product summed ((0 + 1) + 2) + 3.
 * (b) Per group with skip == 0, torch.optim.Adam without weight decay / amsgrad / maximize, eps outside the root:
 *   m = b1 m + c1 g;  v = b2 v + (c2 g) g;  p = p + (-step_size (m / (sqrtf(v) / bc2_sqrt + eps))),
 *   with b = (float)beta and c = (float)(1.0 - beta) formed from the doubles, the factors torch's fp32 kernels get from its Python
 *   floats ((float)(1.0 - 0.999) is not 1.0f - 0.999f), and step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) computed by
 *   the caller, who also owns t.  A zero gradient with non-zero moments moves the parameter; zero gradient and zero moments leave
 *   all three bit-identical.
 * (c) flags & (GSAJ_MAP_RESET_ALL | GSAJ_MAP_RESET_NONVISIBLE): the opacity group is NOT stepped whatever its skip says (the caller
 *   must not advance its t either), its moments become zeros and its raw values are rewritten -- what the reference's
 *   replace_tensor_to_optimizer leaves behind when the reset precedes optimizer.step (gaussian_model.py:438-451, 544-557):
 *   GSAJ_MAP_RESET_ALL: reset_value everywhere (the caller passes inverse_sigmoid(0.01)); it wins over the other two bits.
 *   GSAJ_MAP_RESET_NONVISIBLE: reset_value (inverse_sigmoid(0.4)) where radii[k][i] <= 0 for every k < K_vis.  A row visible in any
 *     view gets s = sigmoid(o), the ACTIVATED value, as its raw value.  Kept quirk of the reference (opacities_new[filter] =
 *     self.get_opacity[filter]): every such reset squashes the visible opacities once more.
 *   GSAJ_MAP_RESET_KEEP_VISIBLE (with _NONVISIBLE): visible rows keep their raw value instead; their moments are zeroed all the same.
 *   A reset bit with every skip set is the stand-alone reset.  Without a reset bit radii, K_vis and reset_value are not read.
 * Pointers of a group that is neither stepped nor reset, and gradients no stepped group reads, may be NULL.  No pointer needs more
 * than 4-byte alignment (the bucket's field views have no more when P is odd): gradients are always read a dword at a time, and
 * a group's parameter and moments 16 bytes at a time only where the three addresses allow it, checked per launch.
 * P = 0: GSAJ_OK, nothing launched.  GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: P < 0, M < 1, P * 3 * M > INT_MAX,
 * scale_cols not 1 or 3, args NULL, a NULL pointer that the launch would read or write, flags outside the three bits,
 * GSAJ_MAP_RESET_NONVISIBLE (without _ALL) with radii NULL or K_vis < 1. */
#define GSAJ_MAP_GROUPS 6
#define GSAJ_MAP_RESET_ALL 1
#define GSAJ_MAP_RESET_NONVISIBLE 2
#define GSAJ_MAP_RESET_KEEP_VISIBLE 4
typedef struct GsajMapStepArgs {
  float *param[GSAJ_MAP_GROUPS];      /* dev, in place; xyz, f_dc, f_rest, opacity, scaling, rotation */
  float *exp_avg[GSAJ_MAP_GROUPS];    /* dev, in place */
  float *exp_avg_sq[GSAJ_MAP_GROUPS]; /* dev, in place */
  const float *g_mean3D, *g_sh, *g_opacity, *g_scale, *g_rot; /* dev */
  float step_size[GSAJ_MAP_GROUPS];
  float bc2_sqrt[GSAJ_MAP_GROUPS];
  int skip[GSAJ_MAP_GROUPS];
  double beta1, beta2, eps; /* as the optimizer holds them: the kernel's four factors are (float)beta, (float)(1.0 - beta) */
  int flags;
  const int *radii; /* dev [K_vis,P] or NULL */
  float reset_value;
} GsajMapStepArgs;
int gsaj_map_step(int P, int M, int scale_cols /*3 or 1*/, int K_vis, const GsajMapStepArgs *args /*host*/, void *stream);

/* ---- rendering quality of one frame: masked PSNR, SSIM, the 8-bit picture (csrc/eval.hip) ----------------------------------------
 * What eval_rendering forms per frame (utils/eval_utils.py:141-160) from image (the render) and gt, both [C,H,W] fp32, contiguous,
 * 4-byte aligned (16 bytes at a time where both are 16-byte aligned, checked per call).  One fp32 rounding per tensor operation
 * of the reference (no contraction):
 *   x = clamp(image, 0, 1)                      a NaN stays a NaN, as torch.clamp leaves it
 *   m = gt > 0                                  per ELEMENT (per channel value), not per pixel: image[mask] gathers elements
 *   d = x - gt;  q = d * d                      fp32, two roundings
 *   n = sum m, an exact integer;  sse = sum over m of q, in fp64 in a fixed order (the reference sums the gathered q in fp32)
 *   mse = (float)(sse / n);  psnr = 20 * log10f(1.0f / sqrtf(mse))        (gaussian_splatting/utils/image_utils.py:19-21)
 *   ssim = the size_average=True value of gsaj_ssim_forward(1, C, W, H, x, gt, ...): of the CLAMPED image and NOT masked (:155)
 *   out_row [4] (dev) = {psnr, ssim, mse, n / (C * H * W)};  out_count [1] (dev) = n.
 * Kept as the reference has them: n = 0 (a black gt) gives mse = psnr = NaN; mse = 0 gives psnr = +inf; a NaN in image gives a NaN
 * psnr (and SSIM), and the byte of that element is 0.
 * image_u8 [H,W,C] (dev, may be NULL): the picture the reference appends to img_pred (:144-148), byte (h, w, c) =
 *   (uint8)(x[c', h, w] * 255.0f), one fp32 multiply and then truncation; c' = C - 1 - c with GSAJ_EVAL_REVERSE_CHANNELS (what
 *   cv2.COLOR_BGR2RGB does to the three channels), else c' = c.
 * Three launches on `stream` (the element pass, gsaj_ssim_forward, a one-workgroup tail), no host read, no float atomics:
 * bit-reproducible.  Nothing but out_row, out_count, image_u8 and eval_ws is written.
 * eval_ws: gsaj_eval_workspace_bytes(C, W, H) bytes, ZEROED ONCE by the caller when allocated (its SSIM slice holds a ticket).  From
 *   its first 256-byte-aligned address it holds x [C,H,W] (readable after the call: what a perceptual metric wants), then the
 *   per-workgroup partials and the SSIM workspace.  gsaj_eval_workspace_bytes returns 0 for dimensions the call would refuse.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: C, W or H < 1, C * W * H > INT_MAX, a NULL image / gt / out_row /
 * out_count / eval_ws, flags outside GSAJ_EVAL_REVERSE_CHANNELS. */
#define GSAJ_EVAL_REVERSE_CHANNELS 1
size_t gsaj_eval_workspace_bytes(int C, int W, int H);
int gsaj_eval_frame(int C, int W, int H, int flags, const float *image, const float *gt, float *out_row /*[4] dev*/,
                    uint32_t *out_count /*[1] dev*/, uint8_t *image_u8 /*[H,W,C] dev or NULL*/, void *eval_ws, void *stream);

/* ---- dense analytic path (NumPy-path semantics) ------------------ */
/* dense_ws: gsaj_dense_workspace_bytes(N, W, H) bytes (the per-workgroup partials of gsaj_dense_backward), no initialisation needed. */
size_t gsaj_dense_workspace_bytes(int N, int W, int H);
/* N depth-sorted Gaussians: means2D [N,2] (pixels), covs2D [N,2,2], colors [N,3], depths [N], opac [N];
 * per-pixel seeds seed_color [H,W,3], seed_depth [H,W]  ->
 * grad_mu [N,2], grad_Sigma [N,2,2], grad_depth [N], grad_color [N,3]. */
/* flags: GSAJ_DENSE_NAIVE_GUARDS selects the edge semantics of the naive per-pixel loop
 * (Loss_Derivative_wrt_mu_and_cov.py:3-118 = compare.py:1050-1169) instead of the vectorised golden producer's (:1311): where
 * alpha_i >= 0.999 the suffix term is dropped rather than divided by 1.0, and an entry with abs(alpha_i) < 1e-8 adds nothing to
 * grad_mu / grad_Sigma. */
#define GSAJ_DENSE_NAIVE_GUARDS 1
/* GSAJ_DENSE_NORMALISED_COORDS: the variant of Loss_Derivative_script.py:820-979 -- means2D / covs2D are in NORMALISED image
 * coordinates and pixel (col, row) sits at ((col - cx) / fx, (row - cy) / fy) (float64 arithmetic rounded to float32 as in
 * :873-877, where the reference reads the module globals cx, fx, cy, fy); `intrinsics` = host {fx, fy, cx, cy}, read only
 * with this flag (NULL otherwise).  Same arithmetic; the gradients come out in normalised units. */
#define GSAJ_DENSE_NORMALISED_COORDS 2
int gsaj_dense_backward(int N, int W, int H, const float *means2D, const float *covs2D, const float *colors,
                        const float *depths, const float *opac, const float *seed_color, const float *seed_depth,
                        float *grad_mu, float *grad_Sigma, float *grad_depth, float *grad_color,
                        void *dense_ws, int flags, const double *intrinsics /*host [4] or NULL*/, void *stream);
/* Front end of the NumPy path (GetImagePlaneMeanAndCovs + compute_cov2d + ndc2Pix + compute_colors_from_sh +
 * OrderGaussiansByDepth, compare.py:854-971, 772-852, 535-588, 764-769), fp64 arithmetic on the fp32 inputs like the
 * reference's Python floats, Appendix A.4 semantics: no z <= 0.2 cull, no tile test, colours clamped below at 0 only, one
 * global STABLE order by view-space z.  means3D [N,3], cov3D [N,6] (xx,xy,xz,yy,yz,zz), shs [N,sh_coeffs,3]; viewmatrix /
 * projmatrix as for the rasteriser (W2C^T, (P W2C)^T); campos [3].  Outputs (device): order [N] int32 (order[i] = original
 * index of sorted position i) and, IN SORTED ORDER, mean2D [N,2] pixels, cov2D [N,2,2] pixels^2 (+0.3 dilation), color [N,3],
 * color_raw [N,3] (before the clamp; may be NULL), depth [N].  project_ws: gsaj_dense_project_workspace_bytes(N) bytes, no
 * initialisation needed. */
size_t gsaj_dense_project_workspace_bytes(int N);
int gsaj_dense_project(int N, int sh_coeffs, int sh_degree, int W, int H, const float *means3D, const float *cov3D,
                       const float *shs, const float *viewmatrix, const float *projmatrix, const float *campos, double fx,
                       double fy, int *order, double *mean2D, double *cov2D, double *color, double *color_raw, double *depth,
                       void *project_ws, void *stream);
/* Dense forward compositor: out_color [H,W,3], out_depth [H,W]. */
int gsaj_dense_render(int N, int W, int H, const float *means2D, const float *covs2D, const float *colors,
                      const float *depths, const float *opac, float *out_color, float *out_depth, void *stream);
/* Closed-form d(mu_I)/d(tau) [N,2,6] and d(vec Sigma_I)/d(tau) [N,4,6] (fp64), already
 * scaled to NDC / pixel^2 units like compute_analytical_jacobians_all_gaussians.
 * T_cw: 16 doubles row-major; mu_w [N,3] doubles; cov3D [N,6] doubles. */
int gsaj_pose_jacobians(int N, const double *T_cw /*dev*/, const double *mu_w, const double *cov3D, double fx,
                        double fy, int W, int H, double *dmu_dtau, double *dcov_dtau, void *stream);
/* dL/dtau (6 doubles, dev) of the NumPy path: chain rule over sorted Gaussians
 * (order[i] = original index of sorted position i) including depth and SH view-direction terms. */
int gsaj_dense_tau(int N, int sh_coeffs, int sh_degree, const int *order, const float *grad_mu,
                   const float *grad_Sigma, const float *grad_depth, const float *grad_color,
                   const double *dmu_dtau, const double *dcov_dtau, const double *mu_w, const double *T_cw,
                   const double *campos, const double *shs /*[N,sh_coeffs,3]*/, double *dL_dtau /*dev [6]*/,
                   double *parts /*dev [4,6] mu,cov,depth,sh or NULL*/, void *stream);

/* ---- image size of a backward ------------------------------------------------------------------------------------------
 * W and H up to GSAJ_BWD_MAX_SIDE (16384 pixels = 1024 tiles a side).  The reverse compositor finds the row an instance's
 * partial gradients go to from the Gaussian's tile rectangle, which the forward packs with 10 bits for each of its first column
 * and first row.  A larger W or H is GSAJ_ERR_INVALID_ARGUMENT, before anything is launched, in all four backward entry points
 * (gsaj_rasterize_backward, _backward_loss, _backward_batch, _backward_loss_batch); the forward entry points and the Jacobian
 * walk do not read the packed rectangle and take wider images. */
#define GSAJ_BWD_MAX_SIDE 16384

/* ---- the launch variants of the binning front end (tests, debugging) ------------------------------------------------------
 * Host only, touches no device: the variants the binning front end selects by the size of a launch, for `views` views of P
 * Gaussians at W x H in ONE call (a single-frame entry point: views = 1; a batched one: its K) -- computed by the functions the
 * launchers themselves call.  plan [GSAJ_PLAN_COUNT] (host memory):
 *   GSAJ_PLAN_BPW               blocks of 256 Gaussians per per-Gaussian forward workgroup (1, 2, 4 or 8)
 *   GSAJ_PLAN_PRE_WORKGROUPS    workgroups of that kernel per view: ceil(ceil(P / 256) / bpw)
 *   GSAJ_PLAN_HIST_LDS          1: its tile histogram is kept in LDS (at most 8192 tiles), 0: global atomics
 *   GSAJ_PLAN_GPT               blocks of 256 Gaussians per instance-scatter workgroup (4, 8, 9 or 10)
 *   GSAJ_PLAN_SCAT_WORKGROUPS   scatter workgroups per view: 8 row classes x ceil(P / (256 gpt))
 *   GSAJ_PLAN_SCAT_LDS          1: the scatter's tile counters are in LDS (ceil(tile rows / 8) x tile columns <= 3411)
 * GSAJ_ERR_INVALID_ARGUMENT: P, views, W or H <= 0, or plan NULL. */
#define GSAJ_PLAN_BPW 0
#define GSAJ_PLAN_PRE_WORKGROUPS 1
#define GSAJ_PLAN_HIST_LDS 2
#define GSAJ_PLAN_GPT 3
#define GSAJ_PLAN_SCAT_WORKGROUPS 4
#define GSAJ_PLAN_SCAT_LDS 5
#define GSAJ_PLAN_COUNT 6
int gsaj_debug_launch_plan(int P, int views, int W, int H, int *plan /*host [GSAJ_PLAN_COUNT]*/);

/* The LDS of every launch that passes dynamic LDS (tests, debugging).  Host only, touches no device: for `views` views of P Gaussians
 * with M SH coefficients per channel (0: precomputed colours) at W x H, sorted with tile_list_capacity keys of LDS (0: the default,
 * 16384), and for the disparity winner of a stereo_W pixel wide pair at stereo_D disparities -- computed by the functions the launchers
 * themselves take their byte counts from.  budget [GSAJ_LDS_LAUNCHES][GSAJ_LDS_FIELDS] (host memory), one row per launch:
 *   GSAJ_LDS_PREPROCESS      the per-Gaussian forward: 4 bytes per tile, up to 8192 tiles          variant: 2 (M = 16) + 1 (bpw > 1)
 *   GSAJ_LDS_FRAME_SCAN      the frame scan: the same
 *   GSAJ_LDS_SCATTER         the instance scatter: 12 bytes per class-local tile while GSAJ_PLAN_SCAT_LDS
 *   GSAJ_LDS_TILE_SORT       the tile sort's first (or only) launch: 8 bytes per key (+ 1028 below 4096 keys)    variant: threads per tile
 *   GSAJ_LDS_TILE_SORT_2     its second launch, half the keys (from 4096 keys on; else a row of zeros)           variant: threads per tile
 *   GSAJ_LDS_GAUSSIAN_BWD    the per-Gaussian backward: 64 rows of 3 M + 1 floats                                variant: 3 M, or 0
 *   GSAJ_LDS_STEREO_WINNER   the disparity winner: 12 bytes per column                                           variant: stereo_D
 * and per row:
 *   GSAJ_LDS_DYNAMIC   bytes of dynamic LDS the launcher passes
 *   GSAJ_LDS_STATIC    bytes of LDS the kernel itself declares
 *   GSAJ_LDS_LIMIT     bytes a workgroup of that kernel may hold, static + dynamic, as the launcher has secured it: 65536, or what it
 *                      raises the function's limit to (the tile sort above 8192 keys)
 *   GSAJ_LDS_VARIANT   which instantiation of the kernel runs
 * The instance scatter counts in LDS only while GSAJ_LDS_STATIC + GSAJ_LDS_DYNAMIC <= 65536: with 24 596 bytes declared, up to
 * 3411 class-local tiles; a larger grid (3840 x 2160: 4080) requests none and counts with global atomics.
 * GSAJ_ERR_INVALID_ARGUMENT: P, views, W or H <= 0, M or tile_list_capacity < 0, budget NULL, or a stereo size gsaj_stereo_match
 * refuses (stereo_D not 16, 32, 64 or 128, stereo_W <= stereo_D or > 4096). */
#define GSAJ_LDS_PREPROCESS 0
#define GSAJ_LDS_FRAME_SCAN 1
#define GSAJ_LDS_SCATTER 2
#define GSAJ_LDS_TILE_SORT 3
#define GSAJ_LDS_TILE_SORT_2 4
#define GSAJ_LDS_GAUSSIAN_BWD 5
#define GSAJ_LDS_STEREO_WINNER 6
#define GSAJ_LDS_LAUNCHES 7
#define GSAJ_LDS_DYNAMIC 0
#define GSAJ_LDS_STATIC 1
#define GSAJ_LDS_LIMIT 2
#define GSAJ_LDS_VARIANT 3
#define GSAJ_LDS_FIELDS 4
int gsaj_debug_lds_budget(int P, int views, int W, int H, int M, int tile_list_capacity, int stereo_W, int stereo_D,
                          int *budget /*host [GSAJ_LDS_LAUNCHES][GSAJ_LDS_FIELDS]*/);

/* ---- frame-to-frame RGB-D alignment: the start pose of a new frame (csrc/align.hip) --------------------------------------------
 * The reference starts a new frame's tracking at the previous frame's pose (utils/slam_frontend.py:129-130) and has NO counterpart of
 * what follows: direct image alignment of the last tracked frame (colour, depth, known pose) against the new frame (colour, optionally
 * depth).  No map, no binning, no lists: one iteration is one pass over the pixels, and it ends in the normal equations
 * gsaj_pose_gn_step solves.  tau = [rho, theta] is that step's left increment, W2C_cur <- Exp(tau) W2C_cur.
 *
 * gsaj_rgbd_align -- two launches on `stream` (the pixel pass, a one-workgroup fold), no host read, no float atomics: the same bits
 *   run to run and on any stream.  Colour [3,H,W], depth [H,W], fp32, contiguous.  Per REFERENCE pixel (i, j) = (column, row), all
 *   fp32, one rounding per operation (no contraction), every sum left to right as written:
 *   0. T = W2C_cur inverse(W2C_ref), W2C_cur = gn_state[0:16) read on the device, the inverse the rigid one [R^T, -R^T t]:
 *        T[a][b] = (C[a][0] R[b][0] + C[a][1] R[b][1]) + C[a][2] R[b][2]                       (C: W2C_cur, R: W2C_ref, 3 x 3 blocks)
 *        ti[k] = -((R[0][k] t[0] + R[1][k] t[1]) + R[2][k] t[2]);   T[a][3] = ((C[a][0] ti[0] + C[a][1] ti[1]) + C[a][2] ti[2]) + C[a][3]
 *   1. I_r = ((r + g) + b) (float)(1.0 / 3.0), Z_r = ref_depth.  Invalid unless both are finite and min_depth <= Z_r <= max_depth.
 *      This project's pixel convention (gsaj/pyramid.py level_camera): pixel index = fx X / Z + cx - 0.5, so
 *        xn = (((float)i + 0.5f) - cx) / fx,  yn likewise;   X_r = xn Z_r,  Y_r = yn Z_r
 *   2. X_c = ((T[0][0] X_r + T[0][1] Y_r) + T[0][2] Z_r) + T[0][3], Y_c, Z_c likewise.  Invalid unless all three are finite and
 *      Z_c >= min_depth.
 *   3. iz = 1.0f / Z_c;  fxz = fx iz;  px = fxz X_c;  u = (px + cx) - 0.5f;  v likewise;  x0 = floorf(u), y0 = floorf(v).
 *      Valid iff 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1 (u = W - 1 exactly is invalid).  a = u - x0, b = v - y0; the taps
 *      p00 p01 / p10 p11 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), each the grey of line 1; invalid unless all four
 *      are finite.  With oma = 1.0f - a, omb = 1.0f - b:
 *        I_c = (p00 oma + p01 a) omb + (p10 oma + p11 a) b
 *        gx = omb (p01 - p00) + b (p11 - p10);   gy = oma (p10 - p00) + a (p11 - p01)
 *      -- the exact derivative of that interpolant; there is no gradient image.
 *   4. r_I = I_c - I_r.  With duz = -(px iz), dvz = -(py iz):  j0 = gx fxz, j1 = gy fyz, j2 = gx duz + gy dvz and
 *        J_I = [j0, j1, j2, j2 Y_c - j1 Z_c, j0 Z_c - j2 X_c, j1 X_c - j0 Y_c]                      (= [j0 j1 j2] [I, -[X_c]x])
 *   5. With cur_depth: the gate is open iff the four depth taps are finite, in [min_depth, max_depth], and
 *      dmax - dmin <= depth_edge_ratio dmin.  D_c and its gradient (hx, hy) as I_c and (gx, gy); r_Z = D_c - Z_c;
 *      k0 = hx fxz, k1 = hy fyz, k2 = hx duz + hy dvz and
 *        J_Z = [k0, k1, k2 - 1, (k2 Y_c - k1 Z_c) - Y_c, (k0 Z_c - k2 X_c) + X_c, k1 X_c - k0 Y_c]
 *   6. Per term, kappa = 1 (photometric) or w_depth, delta = delta_photo or delta_depth (iteratively reweighted least squares, as
 *      gsaj_rasterize_pose_jacobian_loss):  s = kappa min(max(r / delta, -1), 1);  h = kappa / max(|r|, delta);
 *      l = kappa (|r| >= delta ? |r| - 0.5f delta : (r r) / (2.0f delta)).
 *      The pixel's terms:  H_kl = (h_I J_I[k]) J_I[l] + (h_Z J_Z[k]) J_Z[l]  (k <= l),  g_k = s_I J_I[k] + s_Z J_Z[k],  l_I + l_Z, l_I,
 *      l_Z, 1, and 1 if the depth gate is open (a closed gate: s_Z = h_Z = l_Z = 0, J_Z = 0).
 *   7. A NaN or an inf anywhere in an input makes that pixel (colour, reference depth, pose) or that term (current depth) invalid; it
 *      never reaches a sum.
 *   rows [gsaj_rgbd_align_partial_rows(W, H)][GSAJ_GN_PARTIAL_FLOATS]: scratch, one row per workgroup of 64 x 4 pixels, no
 *   initialisation needed.  gn_row [GSAJ_GN_PARTIAL_FLOATS]: the rows added in a fixed order in fp64, then with n = the number of
 *   valid pixels:  [0:21) H / n, [21:27) g / n, [27] loss / n, [28] L_photo / n, [29] L_depth / n, [30] n, [31] the number of open
 *   depth gates -- the ONE row gsaj_pose_gn_step is given, n_partials = 1.  If n < max(1, ceil(min_overlap W H)): H and g are zero and
 *   the three losses +inf, so the step rejects the proposal, or on a first call leaves the pose where it is.
 *   pix_out (may be NULL) [H,W,GSAJ_ALIGN_PIXEL_FLOATS]: u, v, X_c, Y_c, Z_c, I_c, gx, gy, r_I, s_I, h_I, then D_c, r_Z, s_Z, h_Z, 1.0
 *   (zeros with a closed gate); all zeros at an invalid pixel.  valid_out (may be NULL) [H,W]: bit 0 valid, bit 1 depth gate open.
 *   skip: as in gsaj_pose_gn_step -- a non-zero word changes nothing (neither launch writes).
 * gsaj_rgbd_align_partial_rows -- ceil(W / 64) ceil(H / 4); 0 for sizes the call refuses.
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: W or H < 2 or > 16384; a NULL ref_color, ref_depth, ref_w2c, cur_color,
 * gn_state, rows or gn_row; fx or fy not positive; delta_photo or delta_depth <= 0; w_depth < 0; depth_edge_ratio < 0; min_depth <= 0
 * or >= max_depth; min_overlap outside [0, 1]. */
#define GSAJ_ALIGN_PIXEL_FLOATS 16
int gsaj_rgbd_align_partial_rows(int W, int H);      /* 0 for sizes the call refuses */
int gsaj_rgbd_align(int W, int H, float fx, float fy, float cx, float cy,
                    const float *ref_color /*[3,H,W]*/, const float *ref_depth /*[H,W]*/,
                    const float *ref_w2c   /*[16] device, row-major*/,
                    const float *cur_color /*[3,H,W]*/, const float *cur_depth /*[H,W], NULL: photometric only*/,
                    const float *gn_state  /*device; only W2C [0:16) is read*/,
                    float w_depth, float delta_photo, float delta_depth, float depth_edge_ratio,
                    float min_depth, float max_depth, float min_overlap,
                    float *rows      /*[partial_rows][GSAJ_GN_PARTIAL_FLOATS], no initialisation needed*/,
                    float *gn_row    /*[GSAJ_GN_PARTIAL_FLOATS]: the ONE row gsaj_pose_gn_step is given, n_partials = 1*/,
                    float *pix_out   /*[H,W,GSAJ_ALIGN_PIXEL_FLOATS] NULL ok*/, uint8_t *valid_out /*[H,W] NULL ok*/,
                    const uint32_t *skip /*NULL ok, as in gsaj_pose_gn_step*/, void *stream);

/* The joint form -- the affine brightness change of the current frame solved with the pose (auto-exposure between two frames).
 * The unknowns are x = [rho(3), theta(3), a, b], a and b additive as in gsaj_pose_gn8_step; the model is I_c = e^a I_r + b:
 * (a, b) is the current frame's brightness RELATIVE TO THE REFERENCE FRAME, not an absolute camera exposure.
 *
 * gsaj_rgbd_align8 -- gsaj_rgbd_align with a gn8_state (a, b = gn8_state[33], [34], read on the device) and rows of
 *   GSAJ_GN8_PARTIAL_FLOATS; the same two launches, no atomics, the same bits run to run.  Lines 0-3, 5 and 7 above are unchanged.
 *   What differs, fp32, one rounding per operation:
 *   4'. ea = expf(a), evaluated ONCE per workgroup (expf is not correctly rounded: gain_out, if not NULL, receives the float the
 *       pass used; a = 0 gives exactly 1.0f);   g_I = ea I_r;   r_I = I_c - (g_I + b);   J_I as in line 4 and
 *         J8 = [J_I[0..5], -g_I, -1.0f]          (the depth row has no exposure columns: [J_Z[0..5], 0, 0])
 *   6'. s, h, l of both terms as in line 6, from the r_I of line 4'.  The pixel's terms, k <= l:
 *         H8_kl = (h_I J8[k]) J8[l] + (h_Z J_Z[k]) J_Z[l]   for l < 6;      H8_kl = (h_I J8[k]) J8[l]   for l >= 6
 *         g8_k  = s_I J8[k] + s_Z J_Z[k]                     for k < 6;      g8_k  = s_I J8[k]           for k >= 6
 *       then l_I + l_Z, l_I, l_Z, 1, and 1 if the depth gate is open.
 *   rows [gsaj_rgbd_align_partial_rows(W, H)][GSAJ_GN8_PARTIAL_FLOATS]: scratch as above.  gn8_row [GSAJ_GN8_PARTIAL_FLOATS], with
 *   n = the number of valid pixels:  [0:36) H8 / n, the upper triangle by rows, [36:44) g8 / n, [44] loss / n, [45] L_photo / n,
 *   [46] L_depth / n, [47] n, [48] the number of open depth gates, [49:64) zero -- the ONE row gsaj_pose_gn8_step is given,
 *   n_partials = 1 (it reads [0:47)).  The overlap gate as above: H8 and g8 zero, the three losses +inf.
 *   pix_out, valid_out: as above, r_I, s_I, h_I those of line 4'.  skip: a non-zero word changes nothing, gain_out included.
 * GSAJ_ERR_INVALID_ARGUMENT: as gsaj_rgbd_align, with gn8_state and gn8_row in place of gn_state and gn_row. */
int gsaj_rgbd_align8(int W, int H, float fx, float fy, float cx, float cy,
                     const float *ref_color /*[3,H,W]*/, const float *ref_depth /*[H,W]*/,
                     const float *ref_w2c   /*[16] device, row-major*/,
                     const float *cur_color /*[3,H,W]*/, const float *cur_depth /*[H,W], NULL: photometric only*/,
                     const float *gn8_state /*device; only W2C [0:16) and the exposure [33:35) are read*/,
                     float w_depth, float delta_photo, float delta_depth, float depth_edge_ratio,
                     float min_depth, float max_depth, float min_overlap,
                     float *rows      /*[partial_rows][GSAJ_GN8_PARTIAL_FLOATS], no initialisation needed*/,
                     float *gn8_row   /*[GSAJ_GN8_PARTIAL_FLOATS]: the ONE row gsaj_pose_gn8_step is given, n_partials = 1*/,
                     float *gain_out  /*[1] NULL ok: the e^a the pass used*/,
                     float *pix_out   /*[H,W,GSAJ_ALIGN_PIXEL_FLOATS] NULL ok*/, uint8_t *valid_out /*[H,W] NULL ok*/,
                     const uint32_t *skip /*NULL ok, as in gsaj_pose_gn_step*/, void *stream);

/* ---- motion stereo: the depth of a monocular keyframe from a second frame (csrc/sweep.hip) --------------------------------------
 * A monocular keyframe has no measured depth; the reference seeds its new Gaussians at the map's rendered depth or at a constant with
 * noise (utils/slam_frontend.py:63-104) and has NO counterpart of what follows: a plane sweep of the keyframe (`ref`) against another
 * frame (`src`) in general relative pose over D inverse-depth hypotheses, the semi-global aggregation of "stereo frames" above and a
 * winner stage without a left-right check.  This library's own statement, equal bit for bit to tests/sweep_restated.py; nothing is
 * pinned against OpenCV.
 *
 * gsaj_motion_stereo -- on `stream`, no host read, integer atomics only: the same bits run to run and on any stream.  ref, src: grey
 *   uint8 [H,W] with row strides in bytes.  ref_w2c, src_w2c: device float[16], row-major (the first 16 floats of a pose state serve).
 *   a. Gradient bytes of both images, coordinates clamped to the image:  Gx = clamp(gx, -15, 15) + 15, gx the horizontal Sobel of
 *      line 1a of "stereo frames";  Gy the same with the transposed kernel, bottom rows minus top rows.
 *   b. T = W2C_src inverse(W2C_ref): line 0 of "frame-to-frame alignment" with C = W2C_src, R = W2C_ref, fp32, every sum left to right.
 *   c. step = (w_max - w_min) / (float)(D - 1);   w_d = w_min + (float)d step, fp32.  d = 0 is the farthest hypothesis; w = 0 is a point
 *      at infinity.
 *   d. The warp of reference pixel (x, y) under hypothesis d, fp32, one rounding per operation (no contraction):
 *        xn = (((float)x + 0.5f) - cx) / fx,  yn likewise;        a_k = (T[k][0] xn + T[k][1] yn) + T[k][2]
 *        p_k = a_k + w_d T[k][3]         (the source-camera point scaled by w: finite at w = 0)
 *        iz = 1.0f / p_z;   u = ((fx iz) p_x + cx) - 0.5f,  v likewise;   x0 = floorf(u), y0 = floorf(v)
 *      Inside iff, on the floats, p_z > 0, 0 <= x0 <= W - 2 and 0 <= y0 <= H - 2 (a NaN fails).
 *        fa = (int)floorf((u - x0) 16.0f),  fb likewise: both in 0..15.
 *   e. Integers.  For a gradient plane G of the source, taps G00 G01 / G10 G11 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1):
 *        s(G) = (16 - fa)(16 - fb) G00 + fa (16 - fb) G01 + (16 - fa) fb G10 + fa fb G11                       (in [0, 256 * 30])
 *        inside:  pc = (|256 Gx_ref(x, y) - s(Gx_src)| + |256 Gy_ref(x, y) - s(Gy_src)|) >> 6   (<= 240);     outside:  pc = outside_cost
 *   f. C(x, y, d) = the sum of pc over |dx|, |dy| <= r, window coordinates clamped to the image, each window pixel warped on its own
 *      under the same d.  uint16: 225 * 240 = 54 000, hence r <= 7.
 *   g. S = the sum over the 4 or 8 directions of L_rho, line 1e of "stereo frames", over ALL columns (the first column is 0).
 *   h. Per pixel: d* = argmin S, the lowest d on ties; invalid if some d with |d - d*| > 1 has S(d) (100 - uniqueness) < 100 S(d*);
 *      idx16 = 16 d* + ((S(d* - 1) - S(d* + 1)) 16 + den) / (2 den) for 0 < d* < D - 1, den = max(S(d* - 1) + S(d* + 1) - 2 S(d*), 1),
 *      C division (lines 1f-1h of "stereo frames").  No disp2, no left-right check.  Invalid too if the pixel's OWN warp at d* (line d,
 *      recomputed) is outside.  idx16 int16 [H,W]: the hypothesis index in sixteenths, -16 where invalid.
 *   i. out_depth (may be NULL) float32 [H,W], fp64 rounded to float32 once:  w = (double)w_min + ((double)idx16 / 16.0) (double)step;
 *      z = 1 / w if idx16 >= 0 and w > 0, else 0.
 *   stages: GSAJ_SWEEP_STAGE_* to run on what the workspace holds; 0 = all three.
 *   workspace: gsaj_motion_stereo_bytes(W, H, D, paths) bytes, 256-byte aligned, no initialisation needed (S is zeroed on the stream
 *   inside the call): both images' gradient bytes (2 bytes per pixel each), pc uint8, C uint16 and S uint32 [H,W,D] --
 *   gsaj_debug_motion_stereo_offsets gives the byte offsets of the last three (tests, tools).
 * GSAJ_ERR_INVALID_ARGUMENT, before anything is launched: D not 16, 32, 64 or 128; W < 1, H < 1 or W H D > INT_MAX; paths not 4 or 8;
 * r outside [0, 7]; not 0 <= P1 < P2 <= 1024; uniqueness outside [0, 99]; outside_cost outside [0, 240]; fx or fy not positive and
 * finite, cx or cy not finite; w_min or w_max not finite, w_min < 0 or w_max <= w_min; unknown stage bits; a NULL ref, src, ref_w2c,
 * src_w2c, workspace or idx16; a stride below W; a workspace not 256-byte, idx16 not 2-byte, out_depth or a pose not 4-byte aligned.
 * GSAJ_ERR_WORKSPACE_TOO_SMALL: workspace_bytes below gsaj_motion_stereo_bytes.
 *
 * gsaj_grey_u8 -- a tracker's colour float32 [3,H,W] to grey bytes (rows out_stride bytes apart), one launch:
 *   g = ((c0 + c1) + c2) (float)(1.0 / 3.0)   (the grey of "frame-to-frame alignment");   byte = min(max(floorf(g 255.0f + 0.5f), 0), 255);
 *   a NaN gives 0.  GSAJ_ERR_INVALID_ARGUMENT: W or H < 1, W H > INT_MAX, a NULL color or out, out_stride < W. */
#define GSAJ_SWEEP_STAGE_COST 1
#define GSAJ_SWEEP_STAGE_PATHS 2
#define GSAJ_SWEEP_STAGE_WINNER 4
int gsaj_motion_stereo_bytes(int W, int H, int D, int paths, size_t *bytes);
int gsaj_debug_motion_stereo_offsets(int W, int H, int D, int paths, size_t *pc_off, size_t *cost_off, size_t *sum_off);
int gsaj_motion_stereo(int W, int H, const uint8_t *ref /*[H,W]*/, size_t ref_stride, const uint8_t *src /*[H,W]*/, size_t src_stride,
                       float fx, float fy, float cx, float cy,
                       const float *ref_w2c /*[16] device, row-major*/, const float *src_w2c /*[16] device, row-major*/,
                       float w_min, float w_max, int D, int r, int P1, int P2, int paths, int uniqueness, int outside_cost, int stages,
                       void *workspace, size_t workspace_bytes, int16_t *idx16 /*[H,W]*/, float *out_depth /*[H,W] NULL ok*/, void *stream);
int gsaj_grey_u8(int W, int H, const float *color /*[3,H,W]*/, uint8_t *out /*[H,W]*/, size_t out_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSAJ_H_INCLUDED */
