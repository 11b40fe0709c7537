"""GPU: the drop-in forward must render the whole frame whatever the allocator hands it.

rasterize_gaussians takes its image workspace from torch's caching allocator for every call.  A FrameContext of the same frame size
that rendered a tile band (gsaj.tile_band_shard) leaves the band word and the complement that validates it in ITS image workspace;
once the context is freed, the next allocation of that size is the same block.  An un-zeroed workspace then rendered the stale band
only: with the empty band [rows, rows) of an idle rank, nothing at all (num_rendered = 0).  Which test met such a block depended on
the allocations of the tests before it."""
import numpy as np
import pytest

import helpers as hp

pytestmark = pytest.mark.gpu


def test_a_freed_banded_workspace_does_not_band_the_next_drop_in_frame():
    import torch
    from gsaj import _lib
    from gsaj import tile_band_shard as tbs

    lib = _lib.load()
    cam, sc, deg = hp.make("p2000_160x120")
    W, H = cam["W"], cam["H"]
    rows = tbs.tile_rows(H)
    mod = hp.scale_modifier("p2000_160x120")
    (ref, _), kw = hp.oracle_forward(cam, sc, deg, bg=hp.PARITY_BG, precomp=False, scale_modifier=mod)
    assert ref["num_rendered"] > 0
    nbytes = lib.gsaj_image_workspace_bytes(W, H)
    for band in ((rows, rows), (0, 1)):  # an idle rank's empty band; the first tile row only
        # what a freed banded context leaves behind: a workspace of this size with the band set, returned to the allocator
        stale = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        _lib.check(lib.gsaj_set_tile_band(W, H, stale.data_ptr(), band[0], band[1], torch.cuda.current_stream().cuda_stream), "band")
        torch.cuda.synchronize()
        where = stale.data_ptr()
        del stale
        probe = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        print("band %s: the allocator handed the freed block back: %s, its bytes still non-zero: %s"
              % (band, probe.data_ptr() == where, bool(probe.any())))
        del probe
        out, _ = hp.gpu_forward(cam, sc, deg, bg=hp.PARITY_BG, kw=kw, scale_modifier=mod)
        assert out[0] == ref["num_rendered"], (band, out[0], ref["num_rendered"])
        assert np.array_equal(out[2].cpu().numpy(), ref["radii"])
