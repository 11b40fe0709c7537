"""CPU: gsaj/_lib.py binds every function include/gsaj.h declares with the ctypes type each C type must have -- position by position,
return type included -- not merely with the right number of arguments.  A c_int where the header says float would otherwise pass
every count-based check and hand the library garbage."""
import ctypes

from abi import declarations, signature_mismatches


def _signatures():
    from gsaj import _lib

    return _lib.SIGNATURES


def test_the_header_parses_into_every_declared_function():
    decls = declarations()
    assert len(decls) >= 89 and "gsaj_version" in decls and decls["gsaj_version"] == ("int", [])
    ret, params = decls["gsaj_forward_render"]
    assert ret == "int" and len(params) == 18 and params[0] == ("int", "P") and params[10] == ("size_t", "binning_ws_bytes")
    assert params[5] == ("const float *", "bg") and params[-1] == ("void *", "stream")
    assert decls["gsaj_densify_noise"][1][2] == ("uint64_t", "seed") and decls["gsaj_last_error"][0] == "const char *"


def test_every_binding_has_the_type_the_header_declares():
    assert signature_mismatches(_signatures()) == []


def test_canary_a_swapped_scalar_type_is_reported_with_its_function_and_position():
    table = {k: (res, list(args)) for k, (res, args) in _signatures().items()}
    name = "gsaj_rasterize_backward_loss"
    pos = table[name][1].index(ctypes.c_float)  # scale_modifier
    assert declarations()[name][1][pos] == ("float", "scale_modifier")
    table[name][1][pos] = ctypes.c_int
    assert signature_mismatches(table) == [(name, pos, "float", ctypes.c_int)]
    # a pointer bound as a scalar, a wrong return type and a dropped argument are reported as well
    table = {k: (res, list(args)) for k, (res, args) in _signatures().items()}
    table["gsaj_dist2"][1][1] = ctypes.c_int
    table["gsaj_geom_workspace_bytes"] = (ctypes.c_int, table["gsaj_geom_workspace_bytes"][1])
    table["gsaj_mark_visible"][1].pop()
    assert sorted(signature_mismatches(table), key=lambda m: m[0]) == [
        ("gsaj_dist2", 1, "const float *", ctypes.c_int), ("gsaj_geom_workspace_bytes", -1, "size_t", ctypes.c_int),
        ("gsaj_mark_visible", -2, 6, 5)]
