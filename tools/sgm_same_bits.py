#!/usr/bin/env python3
"""Every output of the two semi-global matchers (csrc/stereo.hip, csrc/sweep.hip, csrc/sgm.h) at their benchmarks' sizes, as SHA-256:
StereoMatcher on tools/stereo_bench.py's pair at 752x480, D = 64, r = 10, paths 4 and 8 -- disp16, depth, C, S -- and MotionStereo on
tools/motion_stereo_bench.py's frames at its three sizes -- idx16, depth, the gradient bytes, pc, C, S.  (The restatements of tests/ are
too slow at these sizes; they pin the small ones.)  Run once per library (GSAJ_LIB_PATH names the one to load), one process each, the
same package; the calls and their arguments are the same, so the two outputs must be equal hash for hash.

    GSAJ_LIB_PATH=<parent's library> python tools/sgm_same_bits.py PARENT.json
    python tools/sgm_same_bits.py CHANGE.json
    python tools/sgm_same_bits.py --compare PARENT.json CHANGE.json OUT.json
"""
import numpy as np

from same_bits import main, sha


def run(torch):
    import motion_stereo_bench as mb
    import stereo_bench as sb
    from gsaj import MotionStereo
    from gsaj.stereo import StereoMatcher

    dev, out = torch.device("cuda:0"), {}
    left, right = (torch.as_tensor(x, device=dev) for x in sb.pair(np.random.default_rng(0)))
    for paths in (4, 8):
        m = StereoMatcher(sb.W, sb.H, dev, num_disparities=sb.D, block_radius=sb.R, paths=paths)
        disp16, depth = m(left, right, bf=sb.BF)
        out["stereo/%dx%d/D%d/r%d/paths%d" % (sb.W, sb.H, sb.D, sb.R, paths)] = dict(
            disp16=sha(disp16), depth=sha(depth), C=sha(m.cost_volume()[:, sb.D:]), S=sha(m.sums()))   # (C carries a result at x >= D only)
    for W, H, D, r, paths in mb.SIZES:
        ref, src, K, ref_w2c, src_w2c = mb.frames(W, H, np.random.default_rng(0))
        m = MotionStereo(W, H, dev, *K, num_hypotheses=D, block_radius=r, paths=paths)
        idx16, depth = m(*[torch.as_tensor(x, device=dev) for x in (ref, src, ref_w2c, src_w2c)], *mb.W_RANGE)
        out["sweep/%dx%d/D%d/r%d/paths%d" % (W, H, D, r, paths)] = dict(
            idx16=sha(idx16), depth=sha(depth), grad=sha(m.gradient_bytes()), pc=sha(m.pixel_costs()), C=sha(m.cost_volume()), S=sha(m.sums()))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    main("sgm_same_bits", run, "tools/sgm_same_bits.py on the parent's library and on this change's, one process each, the same package: SHA-256 of "
         "disp16, depth, C and S of StereoMatcher and of idx16, depth, the gradient bytes, pc, C and S of MotionStereo at the "
         "sizes of tools/stereo_bench.py and tools/motion_stereo_bench.py")
