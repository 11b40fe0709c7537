"""The pose state and the Levenberg-Marquardt state behind it, for the host: the one place in gsaj/ where the layout's numbers are
typed.  include/gsaj.h states the layout ("pose_state", "gn_state", "gn8_state"); csrc/pose_se3.h and csrc/gn_state.h hold it for the
kernels under the names in the tables below, and tests/test_cpu_gn_state.py compares the two name for name.

layout(kind)        the checked table of "pose" | "gn" | "gn8": field -> [a, b), the state's size and the partial rows' length
StateViews / GnViews   the read-only views of `self.state` every tracker hands out, for any leading shape ([n], [K, n])
init_state          a state from a pose: the four resets
matrices            the camera matrices of K states, gathered for a batched render
check_schedule      the coarse-to-fine iteration counts"""
import functools
import re

import torch

from . import _lib

# field: (the kernels' name, offset, floats)
_POSE = dict(w2c=("PS_W2C", 0, 16), m=("PS_M", 16, 8), v=("PS_V", 24, 8), step=("PS_STEP", 32, 1), exposure=("PS_EXP", 33, 2),
             view=("PS_VIEW", 35, 16), proj=("PS_PROJ", 51, 16), campos=("PS_CAMPOS", 67, 3), tau=("PS_TAU", 70, 6), norm=("PS_NORM", 76, 1),
             conv=("PS_CONV", 77, 1))
# gn_state: [0:80) the pose state, then the Levenberg-Marquardt fields
_GN = dict(_POSE, lam=("GN_LAMBDA", 80, 1), acc_loss=("GN_ACC_LOSS", 81, 1), has=("GN_HAS", 82, 1), accepted=("GN_ACCEPTED", 83, 1),
           rejected=("GN_REJECTED", 84, 1), last=("GN_LAST", 85, 3), acc_w2c=("GN_ACC_W2C", 88, 16), H=("GN_H", 104, 21), g=("GN_G", 125, 6))
# the joint form: [0:104) as above, then the accepted H8, g8 and exposure; the last exposure step behind `converged`
_GN8 = dict(_GN, H=("GN_H", 104, 36), g=("GN8_G", 140, 8), acc_exposure=("GN8_ACC_EXP", 148, 2), dexposure=("GN8_DEXP", 78, 2))
FIELDS = dict(pose=_POSE, gn=_GN, gn8=_GN8)
SPANS = {kind: {k: (a, a + n) for k, (_, a, n) in fields.items()} for kind, fields in FIELDS.items()}   # kind: field -> (a, b)
ROW_VALID = 30   # gsaj_rgbd_align's gn_row: the slot that holds the number of valid pixels (gsaj_rgbd_align8's: Layout.row_valid)


class Layout:
    """o: field -> (a, b), sl: field -> slice(a, b), at: field -> a; floats: the state's size, from the library; row: the floats of
    one partial row, from include/gsaj.h (None for the pose state); joint: the 8-unknown form."""

    def __init__(self, kind):
        lib, fields = _lib.load(), FIELDS[kind]
        self.kind, self.joint = kind, kind == "gn8"
        self.o = SPANS[kind]
        self.sl = {k: slice(a, b) for k, (a, b) in self.o.items()}
        self.at = {k: a for k, (a, _) in self.o.items()}
        self.sl.update(exposure_a=slice(self.at["exposure"], self.at["exposure"] + 1), exposure_b=slice(self.at["exposure"] + 1, self.o["exposure"][1]))
        self.floats = getattr(lib, "gsaj_%s_state_floats" % kind)()
        spans = sorted(self.o.values())
        if any(a1 < b0 for (_, b0), (a1, _) in zip(spans, spans[1:])) or -(-spans[-1][1] // 8) * 8 != self.floats:
            raise _lib.GsajError("gsaj._gn_state: the %s table does not fit the library's %d floats" % (kind, self.floats))
        self.row = None
        if kind != "pose":   # the header defines the row lengths: H, g, three loss terms and two exposure sums, padded
            with open(_lib.HEADER) as fh:
                self.row = int(re.search(r"#define GSAJ_%s_PARTIAL_FLOATS (\d+)" % kind.upper(), fh.read()).group(1))
            if self.row < fields["H"][2] + fields["g"][2] + 5:
                raise _lib.GsajError("gsaj._gn_state: a %s row of %d floats does not hold H, g and the five sums" % (kind, self.row))
            # gsaj_rgbd_align / gsaj_rgbd_align8: the slot of the row that holds the number of valid pixels (csrc/gn_state.h
            # GN_ROW_VALID, GN8_ROW_VALID) -- behind H, g and the three losses
            self.row_valid = fields["H"][2] + fields["g"][2] + 3


_LAYOUTS = {}


def layout(kind):
    if kind not in _LAYOUTS:
        _LAYOUTS[kind] = Layout(kind)
    return _LAYOUTS[kind]


class StateViews:
    """Views of self.state [..., n] under self._layout: [..., 4, 4] matrices, [..., k] vectors, [...] scalars -- all on the device."""

    def _v(self, name, shape=None):
        t = self.state[..., self._layout.sl[name]]
        return t.view(*t.shape[:-1], *shape) if shape else t

    def _f(self, name):
        return self.state[..., self._layout.at[name]]

    w2c = property(lambda s: s._v("w2c", (4, 4)))
    viewmatrix = property(lambda s: s._v("view", (4, 4)))        # world_view_transform = W2C^T
    projmatrix = property(lambda s: s._v("proj", (4, 4)))        # full_proj_transform
    campos = property(lambda s: s._v("campos"))
    exposure = property(lambda s: s._v("exposure"))
    exposure_a = property(lambda s: s._v("exposure_a"))
    exposure_b = property(lambda s: s._v("exposure_b"))
    tau = property(lambda s: s._v("tau"))
    converged = property(lambda s: s._f("conv"))                 # 1.0 when |tau| < threshold


class GnViews(StateViews):
    """The layout follows self.solve_exposure (False unless the host sets it), looked up at the first view and kept: a host needs no
    attribute beyond its state."""
    solve_exposure = False
    _layout = functools.cached_property(lambda s: layout("gn8" if s.solve_exposure else "gn"))
    accepted_w2c = property(lambda s: s._v("acc_w2c", (4, 4)))

    @property
    def accepted_exposure(self):
        """[..., 2]: a, b of the last accepted step.  Without the joint form the exposure never moves: the state's own [a, b]."""
        return self._v("acc_exposure" if self._layout.joint else "exposure")

    @property
    def loss_terms(self):
        """[..., 3]: loss, L_rgb (L_photo), L_depth of the last iteration."""
        return self._v("last")

    @property
    def lm(self):
        """dict(lam, accepted, rejected, accepted_loss: [...]; H [..., 6, 6], g [..., 6]: the accepted normal equations -- [..., 8, 8],
        [..., 8] over [rho, theta, a, b] in the joint form)."""
        from .rasterizer import unpack_sym6, unpack_sym8
        return dict(lam=self._f("lam"), accepted=self._f("accepted"), rejected=self._f("rejected"), accepted_loss=self._f("acc_loss"),
                    H=(unpack_sym8 if self._layout.joint else unpack_sym6)(self._v("H")), g=self._v("g"))


def init_state(s, lay, w2c, projection, exposure=None, lambda_init=None, rigid=False):
    """One state s [lay.floats] from a pose, in place: the camera matrices of the first render, no accepted step, lambda_init.
    rigid=False: the camera centre by a general 3x3 inverse in fp64 on the host (W2C may carry a scale: one host read);
    rigid=True: -(R^T t) on the device, no host read."""
    sl, at = lay.sl, lay.at
    s.zero_()
    s[sl["w2c"]] = torch.as_tensor(w2c, dtype=torch.float32).reshape(16).to(s.device)
    if exposure is not None:
        s[at["exposure"]] = float(exposure[0])
        s[at["exposure"] + 1] = float(exposure[1])
    w = s[sl["w2c"]].view(4, 4)
    s[sl["view"]] = w.t().reshape(16)
    s[sl["proj"]] = (w.t() @ projection).reshape(16)
    if rigid:
        s[sl["campos"]] = -(w[:3, :3].t() @ w[:3, 3])
    else:
        s[sl["campos"]] = -(torch.linalg.inv(w[:3, :3].double().cpu()) @ w[:3, 3].double().cpu()).float().to(s.device)
    if "lam" in at:
        s[at["lam"]] = lambda_init
        s[sl["acc_w2c"]] = s[sl["w2c"]]
    if lay.joint:
        s[sl["acc_exposure"]] = s[sl["exposure"]]


def matrices(state):
    """(viewmatrices [K,4,4], projmatrices [K,4,4], campos [K,3]) of states [K, n] as contiguous tensors: the poses the next batched
    render is at."""
    K = state.shape[0]
    view, proj, campos = (state[:, a:a + n] for _, a, n in (_POSE["view"], _POSE["proj"], _POSE["campos"]))
    return view.reshape(K, 4, 4).contiguous(), proj.reshape(K, 4, 4).contiguous(), campos.contiguous()


def check_schedule(schedule, levels, who):
    """The iteration counts from the coarsest level to level 0 as ints; `who` names the caller in the error."""
    schedule = [int(n) for n in schedule]
    if len(schedule) != levels + 1 or min(schedule) < 0:
        raise _lib.GsajError("%s: schedule must hold %d non-negative counts, coarsest level first (got %r)" % (who, levels + 1, schedule))
    return schedule
