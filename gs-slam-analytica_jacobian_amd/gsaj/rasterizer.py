"""Torch-tensor front end of the C ABI: the three functions the reference's pybind module
exports (submodules/diff-gaussian-rasterization/ext.cpp:15-19) with the same argument
order and return tuples (rasterize_points.cu:36-246), backed by libgsaj_hip.so.

PyTorch only provides device memory and the current HIP stream here; every computation
happens in the hand-written kernels.
"""
import ctypes
import os

import torch

from . import _lib
from ._loop import stream as _stream

_F32 = torch.float32
# tests flip this (or set the variable) to push every tile list longer than 128 entries through the chunk + merge path of the
# tile sort (the path a list longer than the LDS capacity takes)
FORCE_CHUNKED_SORT = bool(int(__import__("os").environ.get("GSAJ_FORCE_CHUNKED_SORT", "0")))
SORT_CAP = 16384  # longest tile list the per-tile sort handles in ONE LDS pass (csrc/gsaj_common.h); longer: chunks + merge passes


def _ptr(t):
    """Device pointer of a tensor, NULL for None / empty tensors (the reference passes empty
    tensors for absent optionals, diff_gaussian_rasterization/__init__.py:229-243)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _prep(t, device, name):
    if t is None or t.numel() == 0:
        return None
    if t.device != device:
        t = t.to(device)
    if t.dtype != _F32:
        t = t.to(_F32)
    return t.contiguous()


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (HIP device): libgsaj_hip has no CPU path" % what)


# ---- the argument groups of the rasteriser entry points (include/gsaj.h), each built in ONE place as a tuple in ABI order; a call is
# a concatenation of groups (DESIGN.md "Argument groups").  The groups that depend on a context's buffers are methods of _Context.
_ABSENT = object()  # an argument the entry point at hand does not have (the backward family takes no opacities, the forward no raw projection)


def _off(t, nbytes):
    """_ptr(t) moved on by nbytes (a view group's first view); NULL stays NULL."""
    return None if t is None or t.numel() == 0 else t.data_ptr() + nbytes


def _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, opacities=_ABSENT):
    """means3D .. cov3D_precomp; the forward family has opacities after colors_precomp."""
    if opacities is _ABSENT:
        return _ptr(means3D), _ptr(shs), _ptr(colors_precomp), _ptr(scales), float(scale_modifier), _ptr(rotations), _ptr(cov3D_precomp)
    return (_ptr(means3D), _ptr(shs), _ptr(colors_precomp), _ptr(opacities), _ptr(scales), float(scale_modifier), _ptr(rotations),
            _ptr(cov3D_precomp))


def _view(viewmatrix, projmatrix, campos, tanfovx, tanfovy, projmatrix_raw=_ABSENT, v0=None):
    """viewmatrix .. tanfovy; the backward family has projmatrix_raw (one for all views) after projmatrix.  v0 given: the views from v0
    on of a batched call, whose [K,4,4] stacks must be tensors (only campos [K,3] may be absent)."""
    if v0 is None:
        vm, pm, cp = _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos)
    else:
        vm, pm, cp = viewmatrix.data_ptr() + 64 * v0, projmatrix.data_ptr() + 64 * v0, _off(campos, 12 * v0)
    if projmatrix_raw is _ABSENT:
        return vm, pm, cp, float(tanfovx), float(tanfovy)
    return vm, pm, _ptr(projmatrix_raw), cp, float(tanfovx), float(tanfovy)


def _grad_out(g, pose_only=False, v0=0, P=0):
    """The twelve gradient outputs from a slot dict: ten per-Gaussian ones (all NULL: the pose-only form; a BatchContext's slot has no
    conic / color / depth), then dL_dtau and dL_dtau_sum.  v0: the per-view ones ([K,P,.], [K,6]) from that view on."""
    per = (None,) * 10 if pose_only else (
        g["mean2D"].data_ptr() + 12 * P * v0, _ptr(g.get("conic")), g["opacity"].data_ptr(), _ptr(g.get("color")), _ptr(g.get("depth")),
        g["mean3D"].data_ptr(), g["cov3D"].data_ptr(), _ptr(g["sh"]), _ptr(g["scale"]), _ptr(g["rot"]))
    tau_sum = g["tau_sum"] if "tau_sum" in g else g["tau_all"]
    return per + (_off(g["tau"], 24 * P * v0), tau_sum.data_ptr() + 24 * v0)


class _Context:
    """What FrameContext (one view: K = 1, v0 = 0) and BatchContext (views [v0, v0 + kv) of K) hand the entry points from their own
    buffers.  Both have P, W, H, M, flags, the output images, radii / n_touched, the three workspaces, capacity, tile_list_capacity and
    the byte strides between two views' workspace blocks."""

    def _head(self, sh_degree, bg, count=None, K=None):
        """[K,] P, D, M, [count = R or capacity,] bg, W, H"""
        head = (self.P, int(sh_degree), self.M) if count is None else (self.P, int(sh_degree), self.M, count)
        return (head if K is None else (K,) + head) + (_ptr(bg), self.W, self.H)

    def _bind(self):
        """Once the buffers exist.  A context owns its images, radii / n_touched and the geometry and image workspaces for its whole
        life, so their addresses are read once and not per call (the host time of a short tracking iteration is mostly such reads);
        the binning arena is re-allocated as the map grows and is read per call.  (These attributes are not to be re-assigned: the
        asynchronous forwards, the backwards and the Jacobian walk would go on using the buffers bound here.)"""
        self._own = tuple(t.data_ptr() for t in (self.color, self.depth, self.opacity, self.radii, self.n_touched, self.geom, self.img))

    def _images(self, v0=0):
        """color, depth, opacity of view v0"""
        HW = 4 * self.H * self.W * v0
        return self._own[0] + 3 * HW, self._own[1] + HW, self._own[2] + HW

    def _fwd_state(self, v0=0, kv=None):
        """What the asynchronous forwards write and work in: color .. n_touched, geom_ws .. image_ws, flags (kv None: the one view of a
        FrameContext, whose arena is as large as its tensor says)."""
        nbytes, HW = self.binning.numel() if kv is None else self.bin_stride * kv, 4 * self.H * self.W * v0
        color, depth, opacity, radii, n_touched, geom, img = self._own
        return (color + 3 * HW, depth + HW, opacity + HW, radii + 4 * self.P * v0, n_touched + 4 * self.P * v0, geom + self.geom_stride * v0,
                self.binning.data_ptr() + self.bin_stride * v0, nbytes, self.capacity, self.tile_list_capacity, img + self.img_stride * v0,
                self.flags)

    def _bwd_state(self, v0=0):
        """What every pass over a finished forward reads: radii, geom_ws, binning_ws, image_ws"""
        return (self._own[3] + 4 * self.P * v0, self._own[5] + self.geom_stride * v0, self.binning.data_ptr() + self.bin_stride * v0,
                self._own[6] + self.img_stride * v0)

    def _loss(self, L, v0=0, images=False, batched=False):
        """The loss arguments of the fused entry points from the dict forward_loss describes: flags, alpha, threshold, [the forward's
        images: the backward forms,] the ground truth and the exposure pair moved on to view v0 [, exposure_stride: the batched forms]."""
        HW, es = self.H * self.W * v0, int(L.get("exposure_stride", 1)) if batched else 1
        if batched:
            K, HW1 = self.K, self.H * self.W
            for name, n in (("gt_color", 3 * K * HW1), ("gt_depth", K * HW1), ("grad_mask", K * HW1)):
                t = L.get(name)
                if t is not None and (t.device.type != "cuda" or not t.is_contiguous() or t.numel() != n or
                                      t.dtype != (torch.uint8 if name == "grad_mask" else _F32)):
                    raise _lib.GsajError("forward_loss / backward_loss: %s must be a contiguous device tensor of %d elements" % (name, n))
            for name in ("exposure_a", "exposure_b"):
                t = L.get(name)
                if t is not None and (t.device.type != "cuda" or t.dtype != _F32 or t.dim() != 1 or t.shape[0] != K or
                                      (K > 1 and t.stride(0) != es)):
                    raise _lib.GsajError("forward_loss / backward_loss: %s must be a float32 device tensor [K] whose stride is "
                                         "exposure_stride = %d floats" % (name, es))
        head = (int(L["flags"]), float(L["alpha"]), float(L["rgb_boundary_threshold"]))
        gt = (_off(L["gt_color"], 12 * HW), _off(L.get("gt_depth"), 4 * HW), _off(L.get("grad_mask"), HW),
              _off(L.get("exposure_a"), 4 * es * v0), _off(L.get("exposure_b"), 4 * es * v0))
        return (head + self._images(v0) if images else head) + (gt + (es,) if batched else gt)


_SYM6 = [(k, l) for k in range(6) for l in range(k, 6)]  # the 21 stored elements of a symmetric 6x6: upper triangle by rows


def unpack_sym6(h21):
    """[..., 21] (upper triangle by rows, as the normal-equation kernels store H) -> symmetric [..., 6, 6]."""
    out = h21.new_zeros(tuple(h21.shape[:-1]) + (6, 6))
    for n, (k, l) in enumerate(_SYM6):
        out[..., k, l] = h21[..., n]
        out[..., l, k] = h21[..., n]
    return out


def unpack_sym8(h36):
    """[..., 36] (upper triangle by rows, as the joint form stores H8) -> symmetric [..., 8, 8]."""
    out = h36.new_zeros(tuple(h36.shape[:-1]) + (8, 8))
    n = 0
    for k in range(8):
        for l in range(k, 8):
            out[..., k, l] = h36[..., n]
            out[..., l, k] = h36[..., n]
            n += 1
    return out


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, image_height, image_width, sh,
                        degree, campos, prefiltered, debug, record_bits=32):
    """-> (num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, depth, opacity, n_touched)
    (RasterizeGaussiansCUDA, rasterize_points.cu:36-130).  record_bits=16: this frame's sorted instance records store
    conic / opacity / colour as halves (GSAJ_FWD_RECORDS_FP16; a per-call flag, nothing process-wide)."""
    lib = _lib.load()
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _require_cuda(means3D, "means3D")
    dev = means3D.device
    P, H, W = means3D.shape[0], int(image_height), int(image_width)
    f = dict(device=dev, dtype=_F32)
    out_color = torch.zeros((3, H, W), **f)
    out_depth = torch.zeros((1, H, W), **f)
    out_opacity = torch.zeros((1, H, W), **f)
    radii = torch.zeros((P,), device=dev, dtype=torch.int32)
    n_touched = torch.zeros((P,), device=dev, dtype=torch.int32)
    byte = dict(device=dev, dtype=torch.uint8)
    if P == 0:
        e = torch.empty(0, **byte)
        return 0, out_color, radii, e, e.clone(), e.clone(), out_depth, out_opacity, n_touched

    means3D = _prep(means3D, dev, "means3D")
    colors = _prep(colors, dev, "colors")
    opacity = _prep(opacity, dev, "opacity")
    scales = _prep(scales, dev, "scales")
    rotations = _prep(rotations, dev, "rotations")
    cov3D_precomp = _prep(cov3D_precomp, dev, "cov3D")
    sh = _prep(sh, dev, "sh")
    background = _prep(background, dev, "bg")
    viewmatrix = _prep(viewmatrix, dev, "viewmatrix")
    projmatrix = _prep(projmatrix, dev, "projmatrix")
    campos = _prep(campos, dev, "campos")
    M = 0 if sh is None else sh.shape[1]

    geom = torch.empty(lib.gsaj_geom_workspace_bytes(P), **byte)
    # zeroed, as the contexts' are: a block the allocator hands back may be a freed context's image workspace of the same size, with
    # its tile band and the complement that validates it still in place, and this frame would then render that band only
    img = torch.zeros(lib.gsaj_image_workspace_bytes(W, H), **byte)
    st = _stream(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_forward_preprocess(
            P, int(degree), M, W, H, *_scene(means3D, sh, colors, scales, scale_modifier, rotations, cov3D_precomp, opacities=opacity),
            *_view(viewmatrix, projmatrix, campos, tan_fovx, tan_fovy), int(bool(prefiltered)), radii.data_ptr(),
            n_touched.data_ptr(), geom.data_ptr(), img.data_ptr(), st), "gsaj_forward_preprocess")
        R, mt = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.gsaj_forward_num_rendered(W, H, img.data_ptr(), st, ctypes.byref(R), ctypes.byref(mt)),
                   "gsaj_forward_num_rendered")
        R = R.value
        nbytes = lib.gsaj_binning_workspace_bytes(R)
        binning = torch.empty(nbytes, **byte)
        _lib.check(lib.gsaj_forward_render(
            P, R, -1 if FORCE_CHUNKED_SORT else mt.value, W, H, _ptr(background), _ptr(colors), radii.data_ptr(), geom.data_ptr(), binning.data_ptr(), nbytes,
            img.data_ptr(), out_color.data_ptr(), out_depth.data_ptr(), out_opacity.data_ptr(), n_touched.data_ptr(),
            _fwd_flags(record_bits), st), "gsaj_forward_render")
        if debug:
            torch.cuda.synchronize(dev)
    return R, out_color, radii, geom, binning, img, out_depth, out_opacity, n_touched


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, projmatrix_raw, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_depths, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug,
                                 per_gaussian_tau=True):
    """-> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dtau)
    (RasterizeGaussiansBackwardCUDA, rasterize_points.cu:132-223) followed by three extras: dL_dtau_sum [6]
    (= torch.sum(grad_tau.view(-1, 6), dim=0) of diff_gaussian_rasterization/__init__.py:162, reduced in-kernel),
    dL_dconic [P,2,2] and dL_ddepths [P,1] (internal to the reference's binding; exposed for parity tests)."""
    lib = _lib.load()
    _require_cuda(means3D, "means3D")
    dev = means3D.device
    P = means3D.shape[0]
    H, W = dL_dout_color.shape[1], dL_dout_color.shape[2]
    sh = _prep(sh, dev, "sh")
    M = 0 if sh is None else sh.shape[1]
    f = dict(device=dev, dtype=_F32)
    dL_dmeans3D = torch.empty((P, 3), **f)
    dL_dmeans2D = torch.empty((P, 3), **f)
    dL_dcolors = torch.empty((P, 3), **f)
    dL_ddepths = torch.empty((P, 1), **f)
    dL_dconic = torch.empty((P, 2, 2), **f)
    dL_dopacity = torch.empty((P, 1), **f)
    dL_dcov3D = torch.empty((P, 6), **f)
    dL_dsh = torch.empty((P, M, 3), **f)
    dL_dscales = torch.empty((P, 3), **f)
    dL_drotations = torch.empty((P, 4), **f)
    dL_dtau = torch.empty((P, 6), **f) if per_gaussian_tau else None
    dL_dtau_sum = torch.zeros((6,), **f)
    if P == 0:
        return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations,
                dL_dtau, dL_dtau_sum, dL_dconic, dL_ddepths)
    means3D = _prep(means3D, dev, "means3D")
    colors = _prep(colors, dev, "colors")
    scales = _prep(scales, dev, "scales")
    rotations = _prep(rotations, dev, "rotations")
    cov3D_precomp = _prep(cov3D_precomp, dev, "cov3D")
    background = _prep(background, dev, "bg")
    viewmatrix = _prep(viewmatrix, dev, "viewmatrix")
    projmatrix = _prep(projmatrix, dev, "projmatrix")
    projmatrix_raw = _prep(projmatrix_raw, dev, "projmatrix_raw")
    campos = _prep(campos, dev, "campos")
    dL_dout_color = _prep(dL_dout_color, dev, "dL_dout_color")
    dL_dout_depths = _prep(dL_dout_depths, dev, "dL_dout_depths")
    g = dict(mean2D=dL_dmeans2D, conic=dL_dconic, opacity=dL_dopacity, color=dL_dcolors, depth=dL_ddepths, mean3D=dL_dmeans3D,
             cov3D=dL_dcov3D, sh=dL_dsh, scale=dL_dscales if scales is not None else None,
             rot=dL_drotations if rotations is not None else None, tau=dL_dtau, tau_sum=dL_dtau_sum)
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_rasterize_backward(
            P, int(degree), M, int(R), _ptr(background), W, H, *_scene(means3D, sh, colors, scales, scale_modifier, rotations, cov3D_precomp),
            *_view(viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, projmatrix_raw=projmatrix_raw), radii.data_ptr(),
            geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr(), _ptr(dL_dout_color), _ptr(dL_dout_depths),
            *_grad_out(g), _stream(dev)), "gsaj_rasterize_backward")
        if debug:
            torch.cuda.synchronize(dev)
    if scales is None:
        dL_dscales.zero_()
        dL_drotations.zero_()
    return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_dtau,
            dL_dtau_sum, dL_dconic, dL_ddepths)


def mark_visible(means3D, viewmatrix, projmatrix):
    """-> bool [P] (markVisible, rasterize_points.cu:225-246)."""
    lib = _lib.load()
    _require_cuda(means3D, "means3D")
    dev = means3D.device
    P = means3D.shape[0]
    present = torch.zeros((P,), device=dev, dtype=torch.bool)
    if P != 0:
        means3D = _prep(means3D, dev, "means3D")
        viewmatrix = _prep(viewmatrix, dev, "viewmatrix")
        projmatrix = _prep(projmatrix, dev, "projmatrix")
        with torch.cuda.device(dev):
            _lib.check(lib.gsaj_mark_visible(P, _ptr(means3D), _ptr(viewmatrix), _ptr(projmatrix), present.data_ptr(),
                                             _stream(dev)), "gsaj_mark_visible")
    return present


def debug_export(P, R, W, H, geomBuffer, binningBuffer, imageBuffer):
    """Internal forward state as tensors (parity tests)."""
    lib = _lib.load()
    dev = geomBuffer.device
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    f = dict(device=dev, dtype=_F32)
    out = dict(
        means2D=torch.zeros((P, 2), **f), depths=torch.zeros((P,), **f), cov3D=torch.zeros((P, 6), **f),
        conic_opacity=torch.zeros((P, 4), **f), rgb=torch.zeros((P, 3), **f),
        clamped=torch.zeros((P, 3), device=dev, dtype=torch.uint8),
        tiles_touched=torch.zeros((P,), device=dev, dtype=torch.int32),
        point_list=torch.zeros((max(R, 1),), device=dev, dtype=torch.int32),
        ranges=torch.zeros((tiles, 2), device=dev, dtype=torch.int32), final_T=torch.zeros((H, W), **f),
        n_contrib=torch.zeros((H, W), device=dev, dtype=torch.int32))
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_debug_export(
            P, R, W, H, geomBuffer.data_ptr(), binningBuffer.data_ptr(), imageBuffer.data_ptr(),
            out["means2D"].data_ptr(), out["depths"].data_ptr(), out["cov3D"].data_ptr(),
            out["conic_opacity"].data_ptr(), out["rgb"].data_ptr(), out["clamped"].data_ptr(),
            out["tiles_touched"].data_ptr(), out["point_list"].data_ptr(), out["ranges"].data_ptr(),
            out["final_T"].data_ptr(), out["n_contrib"].data_ptr(), _stream(dev)), "gsaj_debug_export")
    out["point_list"] = out["point_list"][:R]
    return out


PLAN_FIELDS = ("bpw", "pre_workgroups", "hist_lds", "gpt", "scat_workgroups", "scat_lds")  # GSAJ_PLAN_* of include/gsaj.h, in order


def launch_plan(P, views, W, H):
    """The variants the binning front end selects for ONE call with `views` views of P Gaussians at W x H, as the launchers
    themselves compute them (gsaj_debug_launch_plan; host only, no device needed): dict of PLAN_FIELDS."""
    plan = (ctypes.c_int * len(PLAN_FIELDS))()
    _lib.check(_lib.load().gsaj_debug_launch_plan(int(P), int(views), int(W), int(H), plan), "gsaj_debug_launch_plan")
    return dict(zip(PLAN_FIELDS, (int(x) for x in plan)))


LDS_LAUNCHES = ("preprocess", "frame_scan", "scatter", "tile_sort", "tile_sort_2", "gaussian_bwd", "stereo_winner")  # GSAJ_LDS_* rows
LDS_FIELDS = ("dynamic", "static", "limit", "variant")  # GSAJ_LDS_* fields of include/gsaj.h, in order


def lds_budget(P, views, W, H, M=1, tile_list_capacity=0, stereo_W=4096, stereo_D=64):
    """The LDS of every launch that passes dynamic LDS, for ONE call with `views` views of P Gaussians (M SH coefficients per channel)
    at W x H sorted with tile_list_capacity keys, and of the disparity winner of a stereo_W wide pair at stereo_D disparities, from
    the functions the launchers take their byte counts from (gsaj_debug_lds_budget; host only, no device needed):
    {launch: dict of LDS_FIELDS} over LDS_LAUNCHES."""
    out = (ctypes.c_int * (len(LDS_LAUNCHES) * len(LDS_FIELDS)))()
    _lib.check(_lib.load().gsaj_debug_lds_budget(int(P), int(views), int(W), int(H), int(M), int(tile_list_capacity), int(stereo_W),
                                                 int(stereo_D), out), "gsaj_debug_lds_budget")
    n = len(LDS_FIELDS)
    return {name: dict(zip(LDS_FIELDS, (int(x) for x in out[i * n:(i + 1) * n]))) for i, name in enumerate(LDS_LAUNCHES)}


def debug_export_taken(R, W, H, binningBuffer, imageBuffer):
    """(taken [R] int32 by list position, reached [R] uint8 by emission slot) of one view: which entries the forward compositor
    took per quadrant (byte q of a word), cleared beyond each quadrant's furthest last contributor as the reverse compositor
    reads them, and which instance rows the last backward wrote.  binningBuffer / imageBuffer: the view's own blocks."""
    lib = _lib.load()
    dev = binningBuffer.device
    taken = torch.zeros((max(R, 1),), device=dev, dtype=torch.int32)
    reached = torch.zeros((max(R, 1),), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_debug_export_taken(R, W, H, binningBuffer.data_ptr(), imageBuffer.data_ptr(), taken.data_ptr(),
                                               reached.data_ptr(), _stream(dev)), "gsaj_debug_export_taken")
    return taken[:R], reached[:R]


STAGE_NAMES = ("preprocess,scan_blocks,emit_keys,sort,ranges_records,render_fwd,render_bwd,gaussian_bwd,tau_finalize,"
               "dense_bwd,dense_reduce,scatter_instances,tile_sort_records,gather_sums").split(",")


class profile_stages:
    """Context manager around gsaj_profile_begin/_end: per-stage kernel time (ms) and launch
    counts measured with HIP events on the launch stream."""

    def __init__(self, max_records=4096):
        self.max_records = max_records
        self.ms, self.launches = {}, {}

    def __enter__(self):
        _lib.check(_lib.load().gsaj_profile_begin(self.max_records), "gsaj_profile_begin")
        return self

    def __exit__(self, *exc):
        n = len(STAGE_NAMES)
        ms = (ctypes.c_float * n)()
        cnt = (ctypes.c_int * n)()
        _lib.check(_lib.load().gsaj_profile_end(ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(cnt, ctypes.c_void_p)),
                   "gsaj_profile_end")
        self.ms = {k: float(ms[i]) for i, k in enumerate(STAGE_NAMES)}
        self.launches = {k: int(cnt[i]) for i, k in enumerate(STAGE_NAMES)}
        return False


FWD_RECORDS_FP16 = 1  # GSAJ_FWD_RECORDS_FP16 (include/gsaj.h)


def _fwd_flags(record_bits):
    """16: the sorted instance records store conic / opacity / colour as halves (32-byte records; positions, depth and all
    accumulation stay fp32).  32: the default fp32 records."""
    if record_bits not in (16, 32):
        raise ValueError("record_bits must be 16 or 32, got %r" % (record_bits,))
    return FWD_RECORDS_FP16 if record_bits == 16 else 0


class ArenaWatch:
    """Growing the binning arena BEFORE a frame overflows it, without a host synchronisation.

    An asynchronous forward that needs more instances than the arena holds is aborted on the device and repeated after a
    blocking re-size -- and a SLAM map grows by construction.  After every `every`-th asynchronous forward the K views' frame
    counters (instances R, error flags, longest tile list: 16 bytes per view) are copied to pinned host memory on the stream
    (non-blocking) and an event is recorded; a later call that finds the event complete looks at them -- a query, never a wait --
    and re-allocates the arena (x1.5 of the largest R) once R passes `grow_at` of the capacity.  The figures are a few frames old
    by then: the head room covers a map that grows a few per cent per frame; a jump beyond it still takes the abort path.
    Not used inside a stream capture (a captured graph holds the arena's address)."""

    def __init__(self, img, K, img_stride, counters_offset, every=4, grow_at=0.75):
        self.K, self.every, self.grow_at = int(K), int(every), float(grow_at)
        i32 = img.view(torch.int32)
        self.dev_counters = torch.as_strided(i32, (self.K, 4), (img_stride // 4, 1), counters_offset // 4)
        self.host = torch.zeros((self.K, 4), dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.pending, self.calls = False, 0
        self.grown = 0  # how many times the arena was re-allocated ahead of an overflow
        # the very first strided device-to-pinned-host copy costs tens of milliseconds (the copy kernel's code object is loaded
        # lazily): paid here, where blocking is allowed, not in the middle of somebody's loop
        with torch.cuda.device(img.device):
            self.host.copy_(self.dev_counters, non_blocking=True)
            self.event.record()
            self.event.synchronize()

    def post(self):
        """After an asynchronous forward was enqueued."""
        self.calls += 1
        if self.pending or self.calls % self.every or torch.cuda.is_current_stream_capturing():
            return
        self.host.copy_(self.dev_counters, non_blocking=True)
        self.event.record()
        self.pending = True

    def poll(self):
        """Before an asynchronous forward: (largest R, longest tile list) of a frame a few calls back, or None."""
        if not self.pending or torch.cuda.is_current_stream_capturing() or not self.event.query():
            return None
        self.pending = False
        return int(self.host[:, 0].max()), int(self.host[:, 2].max())


class FrameContext(_Context):
    """Pre-allocated outputs and workspaces for repeated forward+backward passes over one scene
    size (the tracking / mapping inner loop): no allocation and two C-ABI calls per step.
    The binning workspace grows geometrically when a frame produces more instances."""
    geom_stride = img_stride = bin_stride = 0  # one view: nothing is ever moved on to a later view's block

    def __init__(self, P, W, H, M, device, has_scales=True, per_gaussian_tau=False, grad_slots=1, n_keyframes=0,
                 keyframe=0, record_bits=32):
        lib = _lib.load()
        self.flags = _fwd_flags(record_bits)  # per context (= per view), handed to every forward call
        self.lib, self.P, self.W, self.H, self.M, self.dev = lib, P, W, H, M, torch.device(device)
        f = dict(device=self.dev, dtype=_F32)
        byte = dict(device=self.dev, dtype=torch.uint8)
        self.color = torch.zeros((3, H, W), **f)
        self.depth = torch.zeros((1, H, W), **f)
        self.opacity = torch.zeros((1, H, W), **f)
        self.radii = torch.zeros((P,), device=self.dev, dtype=torch.int32)
        self.n_touched = torch.zeros((P,), device=self.dev, dtype=torch.int32)
        self.geom = torch.empty(lib.gsaj_geom_workspace_bytes(P), **byte)
        self.img = torch.zeros(lib.gsaj_image_workspace_bytes(W, H), **byte)  # zeroed: holds the sticky abort counter
        self.binning = torch.empty(0, **byte)
        self.R = 0
        self.capacity = 0  # > 0 once an arena has been sized: enables forward(sync=False)
        self.tile_list_capacity = 0  # tile-list length the LDS sort of asynchronous frames is sized for (0: the maximum, 16384);
                                     # a longer list is sorted in chunks + merge passes (slower, never wrong)
        self.watch = ArenaWatch(self.img, 1, self.img.numel(), self.abort_flag_ptr() - 16 - self.img.data_ptr())  # (counters[4] = the abort word)
        self.auto_grow = os.environ.get("GSAJ_ARENA_WATCH", "1") != "0"  # asynchronous frames: grow the arena ahead of an overflow (ArenaWatch)
        # per-Gaussian parameter gradients live in ONE flat bucket (field-major) so that a multi-GPU
        # mapping step can all-reduce it with a single collective (gsaj.keyframe_shard); `grad_slots`
        # buckets let the collective of step i overlap the kernels of step i+1
        from .keyframe_shard import bucket_numel, bucket_views
        self.buckets, self.slots = [], []
        for _ in range(max(1, grad_slots)):
            bucket = torch.zeros(bucket_numel(P, M, has_scales, n_keyframes), **f)
            v = bucket_views(bucket, P, M, has_scales, n_keyframes)
            self.buckets.append(bucket)
            self.slots.append(dict(
                mean2D=torch.zeros((P, 3), **f), conic=torch.zeros((P, 2, 2), **f), opacity=v["opacity"],
                color=torch.zeros((P, 3), **f), depth=torch.zeros((P, 1), **f), mean3D=v["mean3D"],
                cov3D=v["cov3D"] if not has_scales else torch.zeros((P, 6), **f), sh=v["sh"].view(P, M, 3),
                scale=v.get("scale"), rot=v.get("rot"),
                tau=torch.zeros((P, 6), **f) if per_gaussian_tau else None,
                # with keyframes the 6 pose gradients land in this rank's row of the shared tau block
                tau_sum=v["tau_all"][keyframe] if n_keyframes else torch.zeros((6,), **f),
                tau_all=v.get("tau_all")))
        self.bucket, self.g = self.buckets[0], self.slots[0]
        self._bind()

    def set_tile_band(self, tile_row_begin, tile_row_end):
        """Render only tile rows [begin, end) from now on (gsaj_set_tile_band; gsaj.tile_band_shard): the frame's other
        pixels come out as background, every gradient is the band's share.  (0, rows) restores the whole frame."""
        _lib.check(self.lib.gsaj_set_tile_band(self.W, self.H, self.img.data_ptr(), int(tile_row_begin), int(tile_row_end),
                                               _stream(self.dev)), "gsaj_set_tile_band")
        self.band = (int(tile_row_begin), int(tile_row_end))

    def abort_flag_ptr(self):
        """Device address of this context's abort word (gsaj_forward_abort_flag): non-zero after an asynchronous forward that did
        not fit the arena.  For PoseTracker.step(skip=...)."""
        return self.lib.gsaj_forward_abort_flag(self.W, self.H, self.img.data_ptr())

    def abort_flag_tensor(self):
        """The same word as a one-element int32 view of the image workspace (for folding it into a collective)."""
        off = self.abort_flag_ptr() - self.img.data_ptr()
        return self.img[off:off + 4].view(torch.int32)

    def _grow_ahead(self):
        """(asynchronous frames) re-allocate the arena if a recent frame came close to filling it; no host synchronisation."""
        seen = self.watch.poll() if self.auto_grow else None
        if seen is None:
            return
        R, longest = seen
        if R > self.watch.grow_at * self.capacity:
            self.capacity = int(R * 1.5) + 1024
            self.binning = torch.empty(self.lib.gsaj_binning_workspace_bytes(self.capacity), device=self.dev, dtype=torch.uint8)
            self.watch.grown += 1
        if longest > self.tile_list_capacity:
            self.tile_list_capacity = min(SORT_CAP, int(1.1 * longest) + 1)

    def _ensure_binning(self, R):
        need = self.lib.gsaj_binning_workspace_bytes(R)
        if self.binning.numel() < need:
            self.capacity = int(R * 1.5) + 1024
            self.binning = torch.empty(self.lib.gsaj_binning_workspace_bytes(self.capacity), device=self.dev,
                                       dtype=torch.uint8)

    def status(self):
        """Blocking: (num_rendered, longest tile list) of the last forward; raises if it, or any asynchronous forward since the
        previous status(), was aborted on the device.  The abort counter is read AND cleared first, so that a caller which
        re-sizes after the exception starts from a clean slate."""
        n = ctypes.c_int(0)
        _lib.check(self.lib.gsaj_forward_aborted_count(self.W, self.H, self.img.data_ptr(), _stream(self.dev),
                                                       ctypes.byref(n)), "gsaj_forward_aborted_count")
        R, mt = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self.lib.gsaj_forward_num_rendered(self.W, self.H, self.img.data_ptr(), _stream(self.dev),
                                                      ctypes.byref(R), ctypes.byref(mt)), "gsaj_forward_num_rendered")
        self.true_R = R.value
        if n.value:
            raise _lib.GsajError("%d asynchronous forward(s) were aborted on the device (binning arena too small for the frame's "
                                 "instances); run forward(sync=True) to re-size" % n.value)
        return R.value, mt.value

    def forward(self, bg, means3D, opacities, viewmatrix, projmatrix, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0, sync=True):
        """sync=True: read R back (16-byte D2H, the reference's only sync) and size the arena exactly.
        sync=False: no host round trip at all -- the arena sized by an earlier synchronous frame (x1.5)
        is reused and an overflowing frame aborts on the device; call status() when convenient."""
        lib, st = self.lib, _stream(self.dev)
        scene = _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, opacities=opacities)
        view = _view(viewmatrix, projmatrix, campos, tanfovx, tanfovy)
        with torch.cuda.device(self.dev):
            if not sync and self.capacity > 0:
                self._grow_ahead()
                _lib.check(lib.gsaj_rasterize_forward_async(*self._head(sh_degree, bg), *scene, *view, 0, *self._fwd_state(), st),
                           "gsaj_rasterize_forward_async")
                self.R = self.capacity  # what the backward must be given (arena carving)
                if self.auto_grow:
                    self.watch.post()
                return self.R
            _lib.check(lib.gsaj_forward_preprocess(
                self.P, int(sh_degree), self.M, self.W, self.H, *scene, *view, 0, self.radii.data_ptr(),
                self.n_touched.data_ptr(), self.geom.data_ptr(), self.img.data_ptr(), st), "gsaj_forward_preprocess")
            R, mt = ctypes.c_int(0), ctypes.c_int(0)
            _lib.check(lib.gsaj_forward_num_rendered(self.W, self.H, self.img.data_ptr(), st, ctypes.byref(R), ctypes.byref(mt)),
                       "gsaj_forward_num_rendered")
            self.R, self.max_tile_list = R.value, mt.value
            # asynchronous frames get an LDS sort sized for the longest tile list seen so far + 10 % (the launcher rounds up to a power
            # of two, which is what the bitonic network pads to anyway; more LDS than that only costs resident workgroups: 2x the
            # longest list made cfg5's sort 2.2x slower).  A longer list is still sorted -- in LDS-sized chunks and merge passes
            self.tile_list_capacity = min(SORT_CAP, max(self.tile_list_capacity, int(1.1 * self.max_tile_list) + 1, 256))
            self._ensure_binning(self.R)
            self.true_R = self.R
            _lib.check(lib.gsaj_forward_render(
                self.P, self.R, -1 if FORCE_CHUNKED_SORT else self.max_tile_list, self.W, self.H, _ptr(bg), _ptr(colors_precomp),
                self.radii.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(), self.binning.numel(), self.img.data_ptr(),
                *self._images(), self.n_touched.data_ptr(), self.flags, st), "gsaj_forward_render")
        return self.R

    # ---- the loss fused into the compositors (gsaj_rasterize_forward_loss / _backward_loss) -----------------
    def forward_loss(self, loss, bg, means3D, opacities, viewmatrix, projmatrix, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                     colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
        """Asynchronous forward (the arena must have been sized by a synchronous forward()) whose compositor also sums the loss:
        loss = dict(flags, alpha, rgb_boundary_threshold, gt_color [3,H,W], gt_depth [H,W] or None, grad_mask (uint8 [H*W]) or None,
        exposure_a, exposure_b (device scalars or None), scalars (float32 [5] device: loss, L_rgb, L_depth, dL/da, dL/db))."""
        if self.capacity <= 0:
            raise _lib.GsajError("forward_loss: size the arena with one synchronous forward() first")
        if not hasattr(self, "loss_ws"):
            self.loss_ws = torch.empty(self.lib.gsaj_fused_loss_workspace_bytes(self.W, self.H), device=self.dev, dtype=torch.uint8)
        with torch.cuda.device(self.dev):
            self._grow_ahead()
            _lib.check(self.lib.gsaj_rasterize_forward_loss(
                *self._head(sh_degree, bg),
                *_scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, opacities=opacities),
                *_view(viewmatrix, projmatrix, campos, tanfovx, tanfovy), 0, *self._fwd_state(), *self._loss(loss),
                loss["scalars"].data_ptr(), self.loss_ws.data_ptr(), _stream(self.dev)), "gsaj_rasterize_forward_loss")
            if self.auto_grow:
                self.watch.post()
        self.R = self.capacity
        return self.R

    def backward_loss(self, loss, bg, means3D, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                      colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0, slot=0,
                      pose_only=False):
        """backward() with the pixel seeds derived inside the reverse compositor from this context's color / depth / opacity and the
        ground truth of `loss` (same dict as forward_loss): no dL/dcolor, dL/ddepth images exist."""
        g = self._slot(slot)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_rasterize_backward_loss(
                *self._head(sh_degree, bg, self.R), *_scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp),
                *_view(viewmatrix, projmatrix, campos, tanfovx, tanfovy, projmatrix_raw=projmatrix_raw), *self._bwd_state(),
                *self._loss(loss, images=True), *_grad_out(g, pose_only), _stream(self.dev)), "gsaj_rasterize_backward_loss")
        return g

    def backward(self, bg, means3D, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy, dL_dcolor, dL_ddepth,
                 sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                 scale_modifier=1.0, slot=0, pose_only=False):
        """pose_only=True (tracking: only the camera is optimised): the per-Gaussian parameter gradients are neither
        computed to the end nor stored; only g["tau_sum"] (and g["tau"] if allocated) are valid afterwards."""
        g = self._slot(slot)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_rasterize_backward(
                *self._head(sh_degree, bg, self.R), *_scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp),
                *_view(viewmatrix, projmatrix, campos, tanfovx, tanfovy, projmatrix_raw=projmatrix_raw), *self._bwd_state(),
                _ptr(dL_dcolor), _ptr(dL_ddepth), *_grad_out(g, pose_only), _stream(self.dev)), "gsaj_rasterize_backward")
        return g

    def _slot(self, slot):
        g = self.slots[slot]
        if g["tau_all"] is not None:
            g["tau_all"].zero_()  # rows of the other ranks' keyframes must be zero before the sum all-reduce
        return g

    # ---- per-pixel pose Jacobians and normal equations (gsaj_rasterize_pose_jacobian / _loss; DESIGN "Gauss-Newton tracking") ----
    def _jac_ready(self, what):
        if self.dev.type != "cuda":
            raise _lib.GsajError("%s needs a HIP device (there is no CPU path)" % what)
        if self.binning.numel() == 0:
            raise _lib.GsajError("%s: run a forward of this context first (it walks the finished forward's state)" % what)
        band = getattr(self, "band", None)
        if band is not None and band != (0, (self.H + 15) // 16):
            raise _lib.GsajError("%s: a tile band is set on this context (band sharding of the Jacobian is not supported)" % what)
        if not hasattr(self, "jac_ws"):
            byte = dict(device=self.dev, dtype=torch.uint8)
            self.jac_ws = torch.empty(self.lib.gsaj_pose_jac_workspace_bytes(self.P, self.W, self.H), **byte)
            self.gn_rows = self.lib.gsaj_pose_jac_partial_rows(self.W, self.H)

    def pose_jacobian(self, bg, means3D, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy, seeds=None, curvature=None,
                      want_jacobian=False, want_images=False, sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None,
                      cov3D_precomp=None, scale_modifier=1.0):
        """The per-pixel pose Jacobian d(colour, depth)/dtau of the last forward of this context and, from it, the normal equations
        of a weighted least-squares problem.  seeds = (s_color [3,H,W], s_depth [1,H,W] or [H,W]): g = sum s J; curvature = (h_color,
        h_depth), same shapes: H = sum h J^T J.  -> dict(H [6,6] or None, g [6] or None, jacobian [H,W,4,6] or None; with
        want_images also color [3,H,W], depth [1,H,W] as the walk re-derives them: the forward's bits).  Tensors are new each call."""
        self._jac_ready("pose_jacobian")
        f = dict(device=self.dev, dtype=_F32)
        jac = torch.empty((self.H, self.W, 4, 6), **f) if want_jacobian else None
        col = torch.empty((3, self.H, self.W), **f) if want_images else None
        dep = torch.empty((1, self.H, self.W), **f) if want_images else None
        H21 = torch.zeros(21, **f) if curvature is not None else None
        g6 = torch.zeros(6, **f) if seeds is not None else None
        sc, sd = (None, None) if seeds is None else [_prep(t, self.dev, "seeds") for t in seeds]
        cc, cd = (None, None) if curvature is None else [_prep(t, self.dev, "curvature") for t in curvature]
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_rasterize_pose_jacobian(
                *self._head(sh_degree, bg, self.R), *_scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp),
                *_view(viewmatrix, projmatrix, campos, tanfovx, tanfovy, projmatrix_raw=projmatrix_raw), *self._bwd_state(),
                self.jac_ws.data_ptr(), _ptr(jac), _ptr(col), _ptr(dep), _ptr(H21), _ptr(g6), _ptr(sc), _ptr(sd), _ptr(cc), _ptr(cd),
                _stream(self.dev)), "gsaj_rasterize_pose_jacobian")
        out = dict(H=None if H21 is None else unpack_sym6(H21), g=g6, jacobian=jac)
        if want_images:
            out.update(color=col, depth=dep)
        return out

    def pose_jacobian_loss(self, loss, bg, means3D, viewmatrix, projmatrix, projmatrix_raw, campos, tanfovx, tanfovy, irls_delta=0.0,
                           partials=None, want_jacobian=False, sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None,
                           cov3D_precomp=None, scale_modifier=1.0, solve_exposure=False):
        """The fused form: seeds and curvatures of the tracking loss (`loss`: the dict of forward_loss / backward_loss) derived per
        pixel from this context's color / depth / opacity, with IRLS delta.  Fills `partials` (float32 [gn_rows, 32], made on the
        first call if None: one fixed-slot row per workgroup -- H (21), g (6), loss, L_rgb, L_depth, two exposure sums) for
        gsaj_pose_gn_step.  solve_exposure: the joint form over [rho, theta, a, b] (gsaj_rasterize_pose_jacobian_loss8) -- rows of
        64 floats: H8 (36), g8 (8), loss, L_rgb, L_depth, two exposure sums, zeros -- for gsaj_pose_gn8_step; the loss must carry
        exposure_a / exposure_b.  -> dict(partials, jacobian or None)."""
        self._jac_ready("pose_jacobian_loss")
        width, own, name = (64, "gn8_partials", "gsaj_rasterize_pose_jacobian_loss8") if solve_exposure else (
            32, "gn_partials", "gsaj_rasterize_pose_jacobian_loss")
        if partials is None:  # (the context's own rows: made right here, nothing to check)
            if not hasattr(self, own):
                setattr(self, own, torch.zeros((self.gn_rows, width), device=self.dev, dtype=_F32))
            partials = getattr(self, own)
        elif tuple(partials.shape) != (self.gn_rows, width) or partials.dtype != _F32 or not partials.is_contiguous() or partials.device != self.dev:
            raise _lib.GsajError("pose_jacobian_loss: partials must be a contiguous float32 [%d, %d] tensor on %s" % (self.gn_rows, width, self.dev))
        jac = torch.empty((self.H, self.W, 4, 6), device=self.dev, dtype=_F32) if want_jacobian else None
        with torch.cuda.device(self.dev):
            _lib.check(getattr(self.lib, name)(
                *self._head(sh_degree, bg, self.R), *_scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp),
                *_view(viewmatrix, projmatrix, campos, tanfovx, tanfovy, projmatrix_raw=projmatrix_raw), *self._bwd_state(),
                self.jac_ws.data_ptr(), *self._loss(loss, images=True), float(irls_delta), partials.data_ptr(), _ptr(jac),
                _stream(self.dev)), name)
        return dict(partials=partials, jacobian=jac)

    def interactions(self):
        """sum over pixels of n_contrib = Gaussian-pixel interactions of the last forward."""
        dbg = debug_export(self.P, self.R, self.W, self.H, self.geom, self.binning, self.img)  # only n_contrib is used
        return int(dbg["n_contrib"].to(torch.int64).sum().item())


def _launch_groups(ctx, name, calls):  # (the one place pose_jacobian_loss needs the device: host-logic tests replace it)
    """One call of entry point `name` per view group of a BatchContext, each on its stream: calls = [(stream or None, arguments up to
    the stream)]."""
    cur = ctx._fork()
    for st, args in calls:
        _lib.check(getattr(ctx.lib, name)(*args, (cur if st is None else st).cuda_stream), name)
    ctx._join(cur)


class BatchContext(_Context):
    """K views of ONE Gaussian map through the batched C-ABI entry points (gsaj_rasterize_forward_batch / _backward_batch): the
    mapping window of the reference (utils/slam_backend.py:168-232) in one set of launches.  Per-view outputs: color / depth /
    opacity [K,.,H,W], radii / n_touched [K,P], g["mean2D"] [K,P,3] (densification reads it per view), g["tau_all"] [K,6];
    per-Gaussian parameter gradients summed over the K views in-kernel, in the flat bucket of gsaj.keyframe_shard (one
    all-reduce ships it, tail = the K pose-gradient rows)."""

    def __init__(self, K, P, W, H, M, device, has_scales=True, record_bits=32, per_gaussian_tau=False, grad_slots=1,
                 n_windows=1, window=0, streams=1):
        """n_windows > 1 (multi-GPU: one window per rank): the bucket's tail has a dL/dtau row for every keyframe of every
        window; this context writes the rows of window `window` and keeps the others zero, so that the ONE sum all-reduce of
        the bucket also gathers the pose gradients of all ranks.
        streams = 2: the window is processed as two groups of views on two HIP streams -- the per-Gaussian / binning kernels of
        one group (latency-bound, few workgroups) overlap the compositors of the other; only the two accumulating per-Gaussian
        chain launches are ordered (GSAJ_BWD_ONLY_COMPOSITE / _ONLY_CHAIN / _ACCUMULATE).  Results are identical to streams = 1
        up to the order of the final fp32 additions (group 0's sum + group 1's sum)."""
        from .keyframe_shard import bucket_numel, bucket_views
        lib = _lib.load()
        self.lib, self.K, self.P, self.W, self.H, self.M, self.dev = lib, int(K), int(P), int(W), int(H), int(M), torch.device(device)
        self.flags = _fwd_flags(record_bits)
        f = dict(device=self.dev, dtype=_F32)
        byte = dict(device=self.dev, dtype=torch.uint8)
        self.color = torch.zeros((K, 3, H, W), **f)
        self.depth = torch.zeros((K, 1, H, W), **f)
        self.opacity = torch.zeros((K, 1, H, W), **f)
        self.radii = torch.zeros((K, P), device=self.dev, dtype=torch.int32)
        self.n_touched = torch.zeros((K, P), device=self.dev, dtype=torch.int32)
        self.geom_stride = lib.gsaj_geom_workspace_bytes(P)
        self.img_stride = lib.gsaj_image_workspace_bytes(W, H)
        self.geom = torch.empty(K * self.geom_stride, **byte)
        self.img = torch.zeros(K * self.img_stride, **byte)  # zeroed once: holds the sticky abort counters
        self.binning = torch.empty(0, **byte)
        self.capacity, self.tile_list_capacity, self.bin_stride = 0, 0, 0
        self.bands = {}  # view -> the tile band set on it (set_tile_band); the Jacobian walk refuses a window with one
        self.watch = ArenaWatch(self.img, self.K, self.img_stride, lib.gsaj_forward_abort_flag(W, H, self.img.data_ptr()) - 16 - self.img.data_ptr())
        self.auto_grow = os.environ.get("GSAJ_ARENA_WATCH", "1") != "0"  # sync=False windows: grow the arena ahead of an overflow (ArenaWatch)
        self.buckets, self.slots = [], []
        for _ in range(max(1, grad_slots)):
            bucket = torch.zeros(bucket_numel(P, M, has_scales, K * n_windows), **f)
            v = bucket_views(bucket, P, M, has_scales, K * n_windows)
            self.buckets.append(bucket)
            self.slots.append(dict(mean2D=torch.zeros((K, P, 3), **f), opacity=v["opacity"], mean3D=v["mean3D"],
                                   cov3D=v["cov3D"] if not has_scales else torch.zeros((P, 6), **f), sh=v["sh"].view(P, M, 3),
                                   scale=v.get("scale"), rot=v.get("rot"), tau=torch.zeros((K, P, 6), **f) if per_gaussian_tau else None,
                                   tau_all=v["tau_all"][window * K:(window + 1) * K], tau_every_window=v["tau_all"] if n_windows > 1 else None))
        self.bucket, self.g = self.buckets[0], self.slots[0]
        # view groups: [(first view, number of views, stream or None = the caller's current stream)]
        if streams >= 2 and K >= 2:
            k0 = (K + 1) // 2
            self.groups = [(0, k0, None), (k0, K - k0, torch.cuda.Stream(self.dev))]
        else:
            self.groups = [(0, K, None)]
        self._bind()

    def _size(self, capacity):
        self.capacity = int(capacity)
        self.bin_stride = self.lib.gsaj_binning_workspace_bytes(self.capacity)
        self.binning = torch.empty(self.K * self.bin_stride, device=self.dev, dtype=torch.uint8)

    def set_tile_band(self, tile_row_begin, tile_row_end, views=None):
        """Render only tile rows [begin, end) of the given views (default: all K) from now on -- gsaj_set_tile_band on each view's
        block of the image workspace.  (0, rows) restores whole frames."""
        for v in (range(self.K) if views is None else views):
            _lib.check(self.lib.gsaj_set_tile_band(self.W, self.H, self.img.data_ptr() + int(v) * self.img_stride, int(tile_row_begin),
                                                   int(tile_row_end), _stream(self.dev)), "gsaj_set_tile_band")
            self.bands[int(v)] = (int(tile_row_begin), int(tile_row_end))

    def status(self):
        """Blocking: per view (num_rendered, longest tile list, aborted)."""
        out, st = [], _stream(self.dev)
        for v in range(self.K):
            R, mt = ctypes.c_int(0), ctypes.c_int(0)
            rc = self.lib.gsaj_forward_num_rendered(self.W, self.H, self.img.data_ptr() + v * self.img_stride, st, ctypes.byref(R), ctypes.byref(mt))
            if rc not in (0, -3):
                _lib.check(rc, "gsaj_forward_num_rendered")
            out.append((R.value, mt.value, rc == -3))
        return out

    def abort_flags(self):
        """(address of view 0's abort word, byte stride between the views' words) for PoseTrackerBatch.step(skip=..., skip_stride=...)."""
        return self.lib.gsaj_forward_abort_flag(self.W, self.H, self.img.data_ptr()), self.img_stride

    def clear_aborts(self):
        """Blocking: read and clear every view's count of aborted asynchronous forwards; returns their sum."""
        total, st = 0, _stream(self.dev)
        for v in range(self.K):
            n = ctypes.c_int(0)
            _lib.check(self.lib.gsaj_forward_aborted_count(self.W, self.H, self.img.data_ptr() + v * self.img_stride, st, ctypes.byref(n)),
                       "gsaj_forward_aborted_count")
            total += n.value
        return total

    def _fork(self):
        """side streams wait for everything the caller's stream has enqueued so far (inputs, the previous step's results)"""
        cur = torch.cuda.current_stream(self.dev)
        for _, _, st in self.groups:
            if st is not None:
                st.wait_stream(cur)
        return cur

    def _join(self, cur):
        for _, _, st in self.groups:
            if st is not None:
                cur.wait_stream(st)

    def _grow_ahead(self):
        """(asynchronous windows) re-allocate the arena if a recent window came close to filling it; no host synchronisation."""
        seen = self.watch.poll() if self.auto_grow else None
        if seen is None:
            return
        if seen[0] > self.watch.grow_at * self.capacity:
            self._size(int(1.5 * seen[0]) + 1024)
            self.watch.grown += 1
        if seen[1] > self.tile_list_capacity > 0:
            self.tile_list_capacity = min(SORT_CAP, int(1.1 * seen[1]) + 1)

    def _launch(self, name, map_args, view_args, tail=lambda v0: ()):
        """One forward call per view group, each on its stream: map_args = (sh_degree, bg, scene), view_args what _view takes,
        tail(v0) what the entry point `name` takes between flags and stream."""
        sh_degree, bg, scene = map_args
        cur = self._fork()
        for v0, kv, st in self.groups:
            _lib.check(getattr(self.lib, name)(
                *self._head(sh_degree, bg, K=kv), *scene, *_view(*view_args, v0=v0), 0, *self._fwd_state(v0, kv), *tail(v0),
                (cur if st is None else st).cuda_stream), name)
        self._join(cur)

    def forward(self, bg, means3D, opacities, viewmatrices, projmatrices, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0, sync=True):
        """viewmatrices / projmatrices [K,4,4] (the rasteriser's transposed matrices), campos [K,3].
        sync=False: no host round trip (arena from an earlier synchronous call; overflowing views abort on the device).
        sync=True: the K instance counts are read back; if a view did not fit, the arena grows and the batch is re-run (tile bands
    set with set_tile_band stay in force: only the abort counters are cleared)."""
        a = ("gsaj_rasterize_forward_batch",
             (sh_degree, bg, _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, opacities=opacities)),
             (viewmatrices, projmatrices, campos, tanfovx, tanfovy))
        if self.capacity == 0:
            self._size(max(4096, 12 * self.P))
        elif not sync:
            self._grow_ahead()
        self._launch(*a)
        if not sync:
            if self.auto_grow:
                self.watch.post()
            return None
        st = self.status()
        if any(ab for _, _, ab in st):
            self._size(int(1.5 * max(r for r, _, _ in st)) + 1024)
            self.tile_list_capacity = 0  # the maximum (16384) until the lists are known
            self.clear_aborts()          # (NOT img.zero_(): the image workspaces also hold the views' tile bands)
            self._launch(*a)
            st = self.status()
            if any(ab for _, _, ab in st):
                raise _lib.GsajError("the batch was aborted again after re-sizing the arena to %d instances per view: %r" % (self.capacity, st))
        if self.auto_grow and max(r for r, _, _ in st) > self.watch.grow_at * self.capacity:
            # the window fits, but with less head room than the arena watch keeps: re-size HERE, where blocking is allowed, rather than
            # a few asynchronous windows later (an allocation of gigabytes in the middle of a loop)
            self._size(int(1.5 * max(r for r, _, _ in st)) + 1024)
            self._launch(*a)
            st = self.status()
        self.tile_list_capacity = min(SORT_CAP, max(self.tile_list_capacity, int(1.1 * max(m for _, m, _ in st)) + 1, 256))
        return st

    def _backward(self, name, slot, split, map_args, view_args, seeds):
        """The one schedule of both backward forms.  A single group: the whole window in one call, or (split) its two halves,
        GSAJ_BWD_ONLY_COMPOSITE then GSAJ_BWD_ONLY_CHAIN.  View groups: the composite halves on their streams, join, then the
        accumulating chains in group order on the caller's stream.  seeds(v0): where dL/dpixel of the views from v0 on comes from."""
        g = self.slots[slot]
        if g["tau_every_window"] is not None:
            g["tau_every_window"].zero_()  # rows of the other ranks' windows must be zero before the sum all-reduce
        sh_degree, bg, scene = map_args

        def call(v0, kv, stream, flags):
            _lib.check(getattr(self.lib, name)(
                *self._head(sh_degree, bg, self.capacity, K=kv), *scene, *_view(*view_args, v0=v0), *self._bwd_state(v0), *seeds(v0),
                *_grad_out(g, v0=v0, P=self.P), flags, stream.cuda_stream), name)

        cur = self._fork()
        if len(self.groups) == 1:
            if split:
                call(0, self.K, cur, 2)
                call(0, self.K, cur, 4)
            else:
                call(0, self.K, cur, 0)
            return g
        for v0, kv, st in self.groups:      # per-view halves: independent, one stream each
            call(v0, kv, cur if st is None else st, 2)
        self._join(cur)                      # the accumulating per-Gaussian chains: in group order on the caller's stream
        for i, (v0, kv, st) in enumerate(self.groups):
            call(v0, kv, cur, 4 | (1 if i > 0 else 0))
        return g

    def backward(self, bg, means3D, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy, dL_dcolor, dL_ddepth,
                 sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0, slot=0,
                 split=False):
        """split=True (one stream): the window's two halves as two calls, GSAJ_BWD_ONLY_COMPOSITE then GSAJ_BWD_ONLY_CHAIN -- the
        per-view sums go through the geometry workspace (k_gather_sums) instead of being formed inside the chain kernel; the
        results are the same bits."""
        HW = self.H * self.W
        return self._backward(
            "gsaj_rasterize_backward_batch", slot, split,
            (sh_degree, bg, _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp)),
            (viewmatrices, projmatrices, campos, tanfovx, tanfovy, projmatrix_raw),
            lambda v0: (dL_dcolor.data_ptr() + 12 * HW * v0, dL_ddepth.data_ptr() + 4 * HW * v0))

    # ---- the loss fused into the batched compositors (gsaj_rasterize_forward_loss_batch / _backward_loss_batch) ---------------
    def forward_loss(self, L, bg, means3D, opacities, viewmatrices, projmatrices, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                     colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
        """forward(sync=False) whose compositor also sums every view's loss: L is the dict FrameContext.forward_loss takes with
        [K,...] tensors -- flags, alpha, rgb_boundary_threshold, gt_color [K,3,H,W], gt_depth [K,H,W] or None, grad_mask (uint8
        [K*H*W]) or None, exposure_a / exposure_b ([K] views with stride exposure_stride floats, default 1; e.g. columns 33 / 34 of
        PoseTrackerBatch.state with exposure_stride=80, read in place) or None, scalars (float32 [K,5]: loss, L_rgb, L_depth,
        dL/da, dL/db per view) and optionally dexposure (float32 [K,2]: the last two again, contiguous, what PoseTrackerBatch.step
        takes).  Asynchronous only: the arena must have been sized by an earlier forward(sync=True).  An aborted view leaves its
        rows of scalars / dexposure as they were."""
        if self.capacity <= 0:
            raise _lib.GsajError("forward_loss: size the arena with one synchronous forward() first")
        K = self.K
        sc, dx = L["scalars"], L.get("dexposure")
        for t, shape in ((sc, (K, 5)), (dx, (K, 2))):
            if t is not None and (t.device.type != "cuda" or t.dtype != _F32 or not t.is_contiguous() or tuple(t.shape) != shape):
                raise _lib.GsajError("forward_loss: scalars / dexposure must be contiguous float32 device tensors [K,5] / [K,2]")
        if not hasattr(self, "loss_ws"):
            self.loss_ws_stride = self.lib.gsaj_fused_loss_batch_workspace_bytes(1, self.W, self.H)
            self.loss_ws = torch.empty(self.lib.gsaj_fused_loss_batch_workspace_bytes(K, self.W, self.H), device=self.dev, dtype=torch.uint8)
        self._grow_ahead()
        self._launch(
            "gsaj_rasterize_forward_loss_batch",
            (sh_degree, bg, _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp, opacities=opacities)),
            (viewmatrices, projmatrices, campos, tanfovx, tanfovy),
            lambda v0: self._loss(L, v0, batched=True) + (sc.data_ptr() + 20 * v0, _off(dx, 8 * v0),
                                                          self.loss_ws.data_ptr() + self.loss_ws_stride * v0))
        if self.auto_grow:
            self.watch.post()

    def backward_loss(self, L, bg, means3D, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy, sh_degree=0, shs=None,
                      colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0, slot=0, split=False):
        """backward() with every view's pixel seeds derived inside the reverse compositor from this context's color / depth / opacity
        and the ground truth of L (same dict as forward_loss): no [K,3,H,W] / [K,1,H,W] seed images exist.  The gradients are those
        of forward -> LossSeedsBatch -> backward bit for bit; split and the view groups work as in backward()."""
        return self._backward(
            "gsaj_rasterize_backward_loss_batch", slot, split,
            (sh_degree, bg, _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp)),
            (viewmatrices, projmatrices, campos, tanfovx, tanfovy, projmatrix_raw),
            lambda v0: self._loss(L, v0, images=True, batched=True))

    # ---- the pose Jacobians and normal equations of the K views (gsaj_rasterize_pose_jacobian_loss_batch / _loss8_batch) ----------
    def pose_jacobian_loss(self, L, bg, means3D, viewmatrices, projmatrices, projmatrix_raw, campos, tanfovx, tanfovy, irls_delta=0.0,
                           partials=None, want_jacobian=False, solve_exposure=False, sh_degree=0, shs=None, colors_precomp=None,
                           scales=None, rotations=None, cov3D_precomp=None, scale_modifier=1.0):
        """FrameContext.pose_jacobian_loss for the K views of the last forward of this context, in one set of launches: L is the
        dict forward_loss / backward_loss take ([K,...] tensors; the exposure pair may be read in place with exposure_stride).  Fills
        `partials` (float32 [K, gn_rows, 32], or [K, gn_rows, 64] with solve_exposure; made on the first call if None): view v's rows
        are what the single-view entry point writes for view v -- for gsaj_pose_gn_step_batch / gsaj_pose_gn8_step_batch.  A view
        aborted on the device keeps its rows.  -> dict(partials, jacobian [K,H,W,4,6] or None)."""
        what = "pose_jacobian_loss"
        if self.binning.numel() == 0:
            raise _lib.GsajError("%s: run a forward of this context first (it walks the finished forward's state)" % what)
        if any(b != (0, (self.H + 15) // 16) for b in self.bands.values()):
            raise _lib.GsajError("%s: a tile band is set on a view of this context (band sharding of the Jacobian is not supported)" % what)
        if not hasattr(self, "jac_ws"):
            self.jac_stride = self.lib.gsaj_pose_jac_batch_workspace_bytes(1, self.P, self.W, self.H)
            self.jac_ws = torch.empty(self.K * self.jac_stride, device=self.dev, dtype=torch.uint8)
            self.gn_rows = self.lib.gsaj_pose_jac_partial_rows(self.W, self.H)
        width, own, name = (64, "gn8_partials", "gsaj_rasterize_pose_jacobian_loss8_batch") if solve_exposure else (
            32, "gn_partials", "gsaj_rasterize_pose_jacobian_loss_batch")
        shape = (self.K, self.gn_rows, width)
        if partials is None:
            if not hasattr(self, own):
                setattr(self, own, torch.zeros(shape, device=self.dev, dtype=_F32))
            partials = getattr(self, own)
        elif tuple(partials.shape) != shape or partials.dtype != _F32 or not partials.is_contiguous() or partials.device != self.dev:
            raise _lib.GsajError("%s: partials must be a contiguous float32 [%d, %d, %d] tensor on %s" % ((what,) + shape + (self.dev,)))
        for t in (means3D, viewmatrices, projmatrices, projmatrix_raw):
            if not torch.is_tensor(t) or t.device.type != "cuda":
                raise _lib.GsajError("%s: means3D and the camera matrices must be device tensors (there is no CPU path)" % what)
        jac = torch.empty((self.K, self.H, self.W, 4, 6), device=self.dev, dtype=_F32) if want_jacobian else None
        scene = _scene(means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp)
        view_args = (viewmatrices, projmatrices, campos, tanfovx, tanfovy, projmatrix_raw)
        calls = [(st, self._head(sh_degree, bg, self.capacity, K=kv) + scene + _view(*view_args, v0=v0) + self._bwd_state(v0) +
                  self._loss(L, v0, images=True, batched=True) +
                  (self.jac_ws.data_ptr() + self.jac_stride * v0, float(irls_delta), partials.data_ptr() + 4 * self.gn_rows * width * v0,
                   _off(jac, 96 * self.H * self.W * v0))) for v0, kv, st in self.groups]
        _launch_groups(self, name, calls)
        return dict(partials=partials, jacobian=jac)

    def view_sums(self, v, stored=False):
        """[P,12]: the reverse compositor's 10 sums per Gaussian of view v of the last backward (gsaj_debug_export_view_sums_gather:
        the whole-window backward never stores them, so they are summed again from the view's instance rows, which survive
        until the next forward): dL/dmean2D x, y | dL/dconic a, b, c | dL/dopacity | dL/dcolor r, g, b | dL/ddepth | 2 pads.
        stored=True: what the geometry workspace holds (gsaj_debug_export_view_sums) -- the sums a split or two-stream backward
        left there for its chain.  For parity tests."""
        out = torch.zeros((self.P, 12), device=self.dev, dtype=_F32)
        v = int(v)
        if stored:
            _lib.check(self.lib.gsaj_debug_export_view_sums(self.P, self.geom.data_ptr() + v * self.geom_stride, out.data_ptr(),
                                                            _stream(self.dev)), "gsaj_debug_export_view_sums")
            return out
        _lib.check(self.lib.gsaj_debug_export_view_sums_gather(
            self.P, self.capacity, self.W, self.H, self.geom.data_ptr() + v * self.geom_stride, self.binning.data_ptr() + v * self.bin_stride,
            self.img.data_ptr() + v * self.img_stride, out.data_ptr(), _stream(self.dev)), "gsaj_debug_export_view_sums_gather")
        return out

    def interactions(self):
        """sum over views and pixels of n_contrib (Gaussian-pixel interactions of the last forward)."""
        total = 0
        for v in range(self.K):
            n = torch.zeros((self.H, self.W), device=self.dev, dtype=torch.int32)
            _lib.check(self.lib.gsaj_debug_export(self.P, 0, self.W, self.H, None, None, self.img.data_ptr() + v * self.img_stride,
                                                  None, None, None, None, None, None, None, None, None, None, n.data_ptr(),
                                                  _stream(self.dev)), "gsaj_debug_export")
            total += int(n.to(torch.int64).sum().item())
        return total
