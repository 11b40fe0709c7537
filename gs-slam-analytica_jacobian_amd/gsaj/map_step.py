"""The step on the Gaussian map in one launch (gsaj_map_step, csrc/map_step.hip; semantics in include/gsaj.h): the chain rule
through the activations, torch.optim.Adam's update on the six raw parameters and the reference's opacity resets
(gaussian_model.py:438-451 with replace_tensor_to_optimizer :544-557), in place on the parameters and on the exp_avg / exp_avg_sq
of the attached torch.optim.Adam, which stays the owner of the state: map growth and pruning go on reading optimizer.state, and
optimizer.step() and map_step may alternate.  The step counts live on the host, one per group as torch keeps them; step_size and
bc2_sqrt are formed from them in Python floats exactly as torch/optim/adam.py::_single_tensor_adam does, and rounded to fp32 once."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import GsajError

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
OPACITY = NAMES.index("opacity")
RESET_ALL, RESET_NONVISIBLE, RESET_KEEP_VISIBLE = 1, 2, 4
RESETS = {None: 0, "all": RESET_ALL, "nonvisible": RESET_NONVISIBLE, "nonvisible_keep": RESET_NONVISIBLE | RESET_KEEP_VISIBLE}
_f6, _i6, _p6 = ctypes.c_float * 6, ctypes.c_int * 6, ctypes.c_void_p * 6


class MapStepArgs(ctypes.Structure):  # GsajMapStepArgs
    _fields_ = [("param", _p6), ("exp_avg", _p6), ("exp_avg_sq", _p6),
                ("g_mean3D", ctypes.c_void_p), ("g_sh", ctypes.c_void_p), ("g_opacity", ctypes.c_void_p),
                ("g_scale", ctypes.c_void_p), ("g_rot", ctypes.c_void_p),
                ("step_size", _f6), ("bc2_sqrt", _f6), ("skip", _i6),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("flags", ctypes.c_int), ("radii", ctypes.c_void_p), ("reset_value", ctypes.c_float)]


def reset_value(opacity):
    """inverse_sigmoid(opacity) as the reference's fp32 tensor expression log(x / (1 - x)): the quotient in fp32, its logarithm
    correctly rounded to fp32 (a library's fp32 log may differ from it in the last place)."""
    x = np.float32(opacity)
    return float(np.float32(math.log(float(x / (np.float32(1.0) - x)))))


def adam_scalars(lr, beta1, beta2, step):
    """(step_size, bc2_sqrt) of _single_tensor_adam for a host step count: Python floats."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return lr / bias_correction1, math.sqrt(bias_correction2)


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(P, M, scale_cols, params, exp_avg, exp_avg_sq, grads, step_size, bc2_sqrt, skip, beta1, beta2, eps, flags=0,
           radii=None, reset=0.0, stream=None):
    """gsaj_map_step on tensors: params / exp_avg / exp_avg_sq are six fp32 device tensors (or None) in NAMES order, grads the
    five of the bucket (mean3D, sh, opacity, scale, rot; or None); no copies are made, so every tensor must be laid out as the
    header says (views at any 4-byte offset are fine)."""
    a = MapStepArgs()
    for i in range(6):
        a.param[i], a.exp_avg[i], a.exp_avg_sq[i] = _ptr(params[i]), _ptr(exp_avg[i]), _ptr(exp_avg_sq[i])
        a.step_size[i], a.bc2_sqrt[i], a.skip[i] = step_size[i], bc2_sqrt[i], int(bool(skip[i]))
    a.g_mean3D, a.g_sh, a.g_opacity, a.g_scale, a.g_rot = (_ptr(g) for g in grads)
    a.beta1, a.beta2, a.eps, a.flags, a.radii, a.reset_value = beta1, beta2, eps, int(flags), _ptr(radii), reset
    K_vis = 0 if radii is None else int(radii.shape[0])
    dev = next(t for t in list(params) + [radii] if t is not None).device
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.load().gsaj_map_step(int(P), int(M), int(scale_cols), K_vis, ctypes.byref(a), s), "gsaj_map_step")


def _flat(t, what, numel, dev, dtype=torch.float32):
    if t is None:
        raise GsajError("map_step: %s is missing" % what)
    if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.numel() != numel:
        raise GsajError("map_step: %s must be a contiguous %s tensor of %d elements on %s, got %s %s on %s%s"
                        % (what, dtype, numel, dev, t.dtype, list(t.shape), t.device, "" if t.is_contiguous() else ", strided"))
    return t


def check_optimizer(model):
    """The attached optimizer must be one whose step the kernel reproduces: GsajError names the reason otherwise."""
    opt = model.optimizer
    if opt is None:
        raise GsajError("map_step: no optimizer attached (training_setup)")
    if not isinstance(opt, torch.optim.Adam) or isinstance(opt, torch.optim.AdamW):
        raise GsajError("map_step: the optimizer must be torch.optim.Adam, got %s" % type(opt).__name__)
    params = dict(zip(NAMES, model.parameters()))
    groups = {}
    for group in opt.param_groups:
        name = group.get("name")
        if len(group["params"]) != 1:
            raise GsajError("map_step: group %r holds %d parameters; one per group is supported" % (name, len(group["params"])))
        if name not in params or name in groups:
            raise GsajError("map_step: optimizer group %r is not one of %s, each once" % (name, list(NAMES)))
        if group["params"][0] is not params[name]:
            raise GsajError("map_step: optimizer group %r does not hold the model's parameter of that name" % name)
        for key, why in (("amsgrad", "amsgrad"), ("maximize", "maximize"), ("capturable", "a capturable (device-resident) step"),
                         ("differentiable", "a differentiable step"), ("fused", "the fused implementation (device-resident step)")):
            if group.get(key):
                raise GsajError("map_step: group %r asks for %s, which the kernel does not reproduce" % (name, why))
        if group.get("weight_decay", 0) != 0:
            raise GsajError("map_step: group %r has weight decay %r, which the kernel does not reproduce" % (name, group["weight_decay"]))
        if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise GsajError("map_step: group %r keeps lr or betas in a tensor; host numbers are needed" % name)
        step = opt.state.get(params[name], {}).get("step")
        if step is not None and isinstance(step, torch.Tensor) and step.device.type != "cpu":
            raise GsajError("map_step: group %r keeps its step on %s; a host step is needed" % (name, step.device))
        groups[name] = group
    if len(groups) != 6:
        raise GsajError("map_step: the optimizer lacks the groups %s" % sorted(set(NAMES) - set(groups)))
    betas, eps = {tuple(g["betas"]) for g in groups.values()}, {g["eps"] for g in groups.values()}
    if len(betas) != 1 or len(eps) != 1:
        raise GsajError("map_step: betas and eps must be the same in every group (they are passed once), got %s, %s" % (sorted(betas), sorted(eps)))
    return params, groups


def _state(opt, prm):
    """A group's state, created where absent as Adam._init_group creates it."""
    state = opt.state[prm]
    if len(state) == 0:
        state["step"] = torch.tensor(0.0, dtype=torch.float32)
        state["exp_avg"] = torch.zeros_like(prm, memory_format=torch.preserve_format)
        state["exp_avg_sq"] = torch.zeros_like(prm, memory_format=torch.preserve_format)
    return state


def map_step(model, g=None, reset=None, radii=None, freeze=()):
    """See GaussianModel.map_step."""
    flags = RESETS[reset] if reset in RESETS else int(reset)
    resets = bool(flags & (RESET_ALL | RESET_NONVISIBLE))
    params, groups = check_optimizer(model)
    unknown = set(freeze) - set(NAMES)
    if unknown:
        raise GsajError("map_step: freeze names %s are not among %s" % (sorted(unknown), list(NAMES)))
    skip = [g is None or n in freeze for n in NAMES]
    if all(skip) and not resets:
        return
    opt = model.optimizer
    dev = params["xyz"].device
    P = params["xyz"].shape[0]
    M = params["f_rest"].shape[1] + 1
    S = params["scaling"].shape[1]
    widths = dict(xyz=3, f_dc=3, f_rest=3 * (M - 1), opacity=1, scaling=S, rotation=4)
    prm, m, v = [None] * 6, [None] * 6, [None] * 6
    step_size, bc2_sqrt = [0.0] * 6, [1.0] * 6
    beta1, beta2 = groups["xyz"]["betas"]
    eps = groups["xyz"]["eps"]
    for i, n in enumerate(NAMES):
        reset_here = resets and i == OPACITY
        if skip[i] and not reset_here:
            continue
        state = _state(opt, params[n])
        prm[i] = _flat(params[n].detach(), "parameter " + n, P * widths[n], dev)
        m[i] = _flat(state["exp_avg"], "exp_avg of " + n, P * widths[n], dev)
        v[i] = _flat(state["exp_avg_sq"], "exp_avg_sq of " + n, P * widths[n], dev)
        if not reset_here:  # (a reset group is not stepped: its step count stays, gaussian_model.py:544-557)
            state["step"] += 1
            step_size[i], bc2_sqrt[i] = adam_scalars(groups[n]["lr"], beta1, beta2, float(state["step"]))
    grads = [None] * 5
    if g is not None:
        need = dict(mean3D=not skip[0], sh=not (skip[1] and skip[2]), opacity=not skip[3] and not resets, scale=not skip[4], rot=not skip[5])
        width = dict(mean3D=3, sh=3 * M, opacity=1, scale=3, rot=4)
        grads = [_flat(g[k], "gradient " + k, P * width[k], dev) if need[k] else None for k in ("mean3D", "sh", "opacity", "scale", "rot")]
    rad = None
    if flags & RESET_NONVISIBLE and not flags & RESET_ALL:
        if radii is None:
            raise GsajError("map_step: a reset of the non-visible Gaussians needs radii [K,P]")
        rad = radii_of(radii, P, dev)
    value = reset_value(0.01 if flags & RESET_ALL else 0.4) if resets else 0.0
    _launch(P, M, S, prm, m, v, grads, step_size, bc2_sqrt, skip, beta1, beta2, eps, flags, rad, value)
    if resets:  # a new leaf over the same storage takes the old one's place in the model, its group and its state's key
        new = dict(params)
        new["opacity"] = params["opacity"].detach()
        model._install(new, {})


def radii_of(visibility, P, dev):
    """[K,P] int32 on the device from what reset_opacity_nonvisible is given: a list of bool [P] filters (radii > 0), stacked and
    converted once, or one int32 [K,P] radii tensor as it is."""
    if isinstance(visibility, (list, tuple)):
        if len(visibility) == 0:
            return torch.zeros((1, P), dtype=torch.int32, device=dev)
        visibility = torch.stack([f.to(dev) for f in visibility])
    r = visibility if visibility.dim() == 2 else visibility[None]
    r = r.to(device=dev, dtype=torch.int32).contiguous()
    if r.shape[1] != P:
        raise GsajError("map_step: visibility has %d columns for %d Gaussians" % (r.shape[1], P))
    return r


def _launch(*a):  # (the one call that needs the device: host-logic tests replace it)
    launch(*a)
