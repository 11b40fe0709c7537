"""The C ABI as include/gsaj.h declares it, for the CPU tests: every declaration parsed into (return type, [(type, parameter name)]),
the ctypes type each C type must be bound as, and calls of the rasteriser entry points built BY PARAMETER NAME from one set of named
argument groups, so that a test states only what it changes (no test spells a 40-argument list)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsaj.h")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def declarations():
    """name -> (return type, [(type, name), ...]) of every function the header declares; types as written, comments and
    redundant blanks removed ("const float *", "int", ...)."""
    with open(HEADER) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(gsaj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p in ("void", ""):
                continue
            m = re.fullmatch(r"(.*?[\s\*])(\w+)", p)
            plist.append((" ".join(m.group(1).split()), m.group(2)))
        out[name] = (" ".join(ret.split()), plist)
    return out


def binds_as(ctype, bound):
    """Is `bound` (a ctypes type) how the C type `ctype` must travel?  Scalars map one to one; anything with a * is void* or a
    typed ctypes pointer (const char * may also be c_char_p, which is what makes gsaj_last_error() return bytes)."""
    if "*" in ctype:
        if bound is ctypes.c_void_p or (isinstance(bound, type) and issubclass(bound, ctypes._Pointer)):
            return True
        return bound is ctypes.c_char_p and ctype.replace(" ", "") == "constchar*"
    return _SCALARS.get(ctype) is bound


def signature_mismatches(signatures, decls=None):
    """[(function, position, C type, bound type)]: position -1 is the return type, -2 a wrong argument count, "missing" / "undeclared"
    a function only one side has."""
    decls = declarations() if decls is None else decls
    bad = [(n, "missing", None, None) for n in decls if n not in signatures]
    bad += [(n, "undeclared", None, None) for n in signatures if n not in decls]
    for name, (ret, params) in decls.items():
        if name not in signatures:
            continue
        res, args = signatures[name]
        if not binds_as(ret, res):
            bad.append((name, -1, ret, res))
        if len(args) != len(params):
            bad.append((name, -2, len(params), len(args)))
            continue
        bad += [(name, i, ct, a) for i, ((ct, _), a) in enumerate(zip(params, args)) if not binds_as(ct, a)]
    return bad


# ---- calls that are rejected before any launch ------------------------------------------------------------------------------------
X = 0x1000  # a non-NULL, 256-byte aligned pointer nothing reads: every call made with it must return before any launch
COMPUTE_LOSS, MONOCULAR, NO_EXPOSURE = 8, 2, 4   # GSAJ_LOSS_*
ONLY_COMPOSITE, ONLY_CHAIN = 2, 4                # GSAJ_BWD_*

# one value per parameter NAME of the rasteriser entry points: a well-formed call of a 300-Gaussian SH-degree-3 map with scales and
# rotations, at 37 x 29 -- which no test makes: each row overrides the names that carry its defect
SCENE = dict(P=300, D=3, M=16, means3D=X, shs=X, colors_precomp=None, opacities=X, scales=X, scale_modifier=1.0, rotations=X,
             cov3D_precomp=None)
VIEW = dict(K=3, W=37, H=29, bg=X, viewmatrix=X, projmatrix=X, viewmatrices=X, projmatrices=X, projmatrix_raw=X, campos=X, tanfovx=0.5,
            tanfovy=0.5, prefiltered=0)
WORKSPACES = dict(geom_ws=X, binning_ws=X, binning_ws_bytes=1 << 20, image_ws=X, jac_ws=X, R=4096, capacity=4096, tile_list_capacity=0,
                  max_tile_list=64, stream=None)
FORWARD_OUT = dict(out_color=X, out_depth=X, out_opacity=X, radii=X, n_touched=X, num_rendered_out=None, flags=0)
LOSS = dict(loss_flags=0, alpha=0.9, rgb_boundary_threshold=0.01, color=X, depth=X, opacity=X, gt_color=X, gt_depth=X, grad_mask=None,
            exposure_a=X, exposure_b=X, exposure_stride=1, out_scalars=X, out_dexposure=None, loss_ws=X)
GRADS = dict(dL_dpix=X, dL_dpix_depth=X, dL_dmean2D=X, dL_dconic=X, dL_dopacity=X, dL_dcolor=X, dL_ddepth=X, dL_dmean3D=X, dL_dcov3D=X,
             dL_dsh=X, dL_dscale=X, dL_drot=X, dL_dtau=X, dL_dtau_sum=X)
JACOBIAN = dict(jac_out=X, H_out=X, g_out=X, seed_color=X, seed_depth=X, curv_color=X, curv_depth=X, irls_delta=0.0, gn_partials=X,
                gn8_partials=X)
DEFAULTS = {}
for _g in (SCENE, VIEW, WORKSPACES, FORWARD_OUT, LOSS, GRADS, JACOBIAN):
    DEFAULTS.update(_g)
_DECLS = None


def call(lib, name, **overrides):
    """lib.<name>(...) with every parameter the header names taken from `overrides`, else from the groups above."""
    global _DECLS
    if _DECLS is None:
        _DECLS = declarations()
    names = [p for _, p in _DECLS[name][1]]
    unknown = set(overrides) - set(names)
    assert not unknown, "%s has no parameter %s" % (name, sorted(unknown))
    return getattr(lib, name)(*[overrides[p] if p in overrides else DEFAULTS[p] for p in names])
