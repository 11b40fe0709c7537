"""The scene and the calls of tests/test_gpu_gn_single_view.py and tools/gn_same_bits.py: the single-frame Gauss-Newton entry points
are the batched kernels of csrc/pose_jac.hip launched with one view, so what is exercised here is the host code that tells the two
forms apart (csrc/api.hip: pose_jac) -- where a workspace starts, what the Jacobian workspace holds, which kernel is launched.

200 Gaussians on a 40 x 24 frame: 3 x 2 tiles with a partial tile column and a partial tile row, 24 workgroups in one granule of 32
(gsaj_pose_jac_partial_rows = 32), so the eight workgroups of tile slots 6 and 7 find no tile and write zero rows."""
import math

import numpy as np

import loss_restated as lr

W, H, P, K = 40, 24, 200, 3
ROWS = 32
PADDING = (6, 7, 14, 15, 22, 23, 30, 31)   # the workgroups whose rank (blockIdx >> 5) * 8 + (blockIdx & 7) is beyond the 6 tiles
BIN_CAPACITY = 4096                        # instances the unaligned binning arena is made for (the scene has under 1200)
LM = (1e-3, 4.0, 1e-7, 1e7, 1e-4)          # lambda_init, nu, lambda_min, lambda_max, converged_threshold
SENTINEL = -7.0
COLOURS = ("sh", "precomp")


class World:
    """The map, K cameras on an arc, and per view a ground truth, a mask and an exposure pair (random: any will do for equal bits)."""

    def __init__(self, colours):
        import torch
        from gsaj import synthetic as syn

        self.dev = torch.device("cuda:0")
        self.t = t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.dev)  # noqa: E731
        self.cams = cams = syn.keyframe_cameras(K, radius=0.25, W=W, H=H, fx=35.0, fy=35.0, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
        sc = syn.make_scene(P, 11, cams[1], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
        rng = np.random.default_rng(17)
        self.bg, self.means, self.opac = t((0.1, 0.2, 0.3)), t(sc["means3D"]), t(sc["opacities"])
        self.kw = dict(scales=t(sc["scales"]), rotations=t(sc["rotations"]))
        if colours == "sh":
            self.kw.update(sh_degree=3, shs=t(sc["shs"]))
        else:
            self.kw.update(colors_precomp=t(rng.uniform(0.0, 1.0, size=(P, 3))))
        self.views = tuple(t(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
        self.w2cs = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float32) for c in cams]
        self.praw = t(cams[0]["projmatrix_raw"])
        self.tan = (cams[0]["tanfovx"], cams[0]["tanfovy"])
        self.gt_c = t(rng.uniform(0.0, 1.0, size=(K, 3, H, W)))
        self.gt_d = t(rng.uniform(1.0, 4.0, size=(K, H, W)))
        self.mask = torch.as_tensor((rng.uniform(size=(K, H * W)) < 0.7).astype(np.uint8), device=self.dev)
        self.E = t(rng.uniform(-0.1, 0.1, size=(K, 2)))
        self.seeds = (t(rng.normal(size=(3, H, W)) / (3 * H * W)), t(rng.normal(size=(1, H, W)) / (H * W)))
        self.curv = (t(rng.uniform(0.0, 1.0, size=(3, H, W))), t(rng.uniform(0.0, 1.0, size=(1, H, W))))

    def loss(self, v):
        """the tracking loss of view v, as the single-frame entry points take it"""
        return dict(flags=lr.TRACKING, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=self.gt_c[v], gt_depth=self.gt_d[v],
                    grad_mask=self.mask[v], exposure_a=self.E[v, 0:1], exposure_b=self.E[v, 1:2])

    def loss_batch(self, k):
        """... of views [0, k), as the batched entry points take it (the exposure pairs read in place)"""
        return dict(flags=lr.TRACKING, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=self.gt_c[:k].contiguous(),
                    gt_depth=self.gt_d[:k].contiguous(), grad_mask=self.mask[:k].reshape(-1).contiguous(), exposure_a=self.E[:k, 0],
                    exposure_b=self.E[:k, 1], exposure_stride=2)


def off_boundary(nbytes, dev, zero=False):
    """nbytes of device memory that start 16 bytes past a 256-byte boundary"""
    import torch

    buf = (torch.zeros if zero else torch.empty)(nbytes + 512, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256 + 16
    return buf[off:off + nbytes]


class Frame:
    """View v through the single-frame entry points (FrameContext); unaligned: every workspace 16 bytes past a 256-byte boundary."""

    def __init__(self, w, v, unaligned=False):
        from gsaj.rasterizer import FrameContext

        self.w, self.v = w, v
        self.ctx = c = FrameContext(P, W, H, 16, w.dev)
        if unaligned:
            lib = c.lib
            c.geom = off_boundary(lib.gsaj_geom_workspace_bytes(P), w.dev)
            c.img = off_boundary(lib.gsaj_image_workspace_bytes(W, H), w.dev, zero=True)
            c.binning = off_boundary(lib.gsaj_binning_workspace_bytes(BIN_CAPACITY), w.dev)
            c.jac_ws = off_boundary(lib.gsaj_pose_jac_workspace_bytes(P, W, H), w.dev)
            c.gn_rows = lib.gsaj_pose_jac_partial_rows(W, H)
            c.auto_grow = False
            c._bind()
        self.view = tuple(m[v] for m in w.views)
        R = c.forward(w.bg, w.means, w.opac, *self.view, *w.tan, **w.kw)
        assert 0 < R <= BIN_CAPACITY
        if unaligned:
            assert all(b.data_ptr() % 256 == 16 for b in (c.geom, c.img, c.binning, c.jac_ws)), "the forward replaced a workspace"

    def jac(self, **kw):
        w = self.w
        return self.ctx.pose_jacobian(w.bg, w.means, self.view[0], self.view[1], w.praw, self.view[2], *w.tan, **kw, **w.kw)

    def jac_loss(self, joint):
        import torch

        w = self.w
        rows = torch.full((ROWS, 64 if joint else 32), SENTINEL, device=w.dev)
        return self.ctx.pose_jacobian_loss(w.loss(self.v), w.bg, w.means, self.view[0], self.view[1], w.praw, self.view[2], *w.tan,
                                           irls_delta=0.03, partials=rows, want_jacobian=True, solve_exposure=joint, **w.kw)


class Window:
    """Views [0, k) through the batched entry points (BatchContext)."""

    def __init__(self, w, k):
        from gsaj.rasterizer import BatchContext

        self.w, self.k = w, k
        self.views = tuple(m[:k].contiguous() for m in w.views)
        self.ctx = BatchContext(k, P, W, H, 16, w.dev)
        st = self.ctx.forward(w.bg, w.means, w.opac, *self.views, *w.tan, sync=True, **w.kw)
        assert not any(ab for _, _, ab in st)

    def jac_loss(self, joint):
        import torch

        w = self.w
        rows = torch.full((self.k, ROWS, 64 if joint else 32), SENTINEL, device=w.dev)
        return self.ctx.pose_jacobian_loss(w.loss_batch(self.k), w.bg, w.means, self.views[0], self.views[1], w.praw, self.views[2], *w.tan,
                                           irls_delta=0.03, partials=rows, want_jacobian=True, solve_exposure=joint, **w.kw)


def new_states(w, k, joint):
    """k fresh Gauss-Newton states [k, n] at the cameras' poses with the views' exposure pairs"""
    import torch
    from gsaj._gn_state import init_state, layout

    lay = layout("gn8" if joint else "gn")
    s = torch.zeros((k, lay.floats), device=w.dev)
    for v in range(k):
        init_state(s[v], lay, w.w2cs[v], w.praw.reshape(4, 4), tuple(float(x) for x in w.E[v].cpu()), LM[0])
    return s


def step(w, joint, rows, state, skip=None):
    """gsaj_pose_gn_step / gsaj_pose_gn8_step on one state, in place; skip: a device uint32 tensor or None"""
    import torch
    from gsaj import _lib

    lib = _lib.load()
    name = "gsaj_pose_gn8_step" if joint else "gsaj_pose_gn_step"
    _lib.check(getattr(lib, name)(rows.data_ptr(), rows.shape[0], *LM, w.praw.data_ptr(), state.data_ptr(),
                                  None if skip is None else skip.data_ptr(), torch.cuda.current_stream(w.dev).cuda_stream), name)


def step_batch(w, joint, rows, states, active=None, skip=None, skip_stride=0):
    """gsaj_pose_gn_step_batch / gsaj_pose_gn8_step_batch on states [k, n], in place"""
    import torch
    from gsaj import _lib

    lib = _lib.load()
    name = "gsaj_pose_gn8_step_batch" if joint else "gsaj_pose_gn_step_batch"
    _lib.check(getattr(lib, name)(states.shape[0], rows.data_ptr(), rows.shape[1], None if active is None else active.data_ptr(), *LM,
                                  w.praw.data_ptr(), states.data_ptr(), None if skip is None else skip.data_ptr(), int(skip_stride),
                                  torch.cuda.current_stream(w.dev).cuda_stream), name)
