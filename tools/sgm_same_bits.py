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
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


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


def main():
    if sys.argv[1] == "--compare":
        a, b = (json.load(open(p)) for p in sys.argv[2:4])
        differing = sorted(k for k in set(a["hashes"]) | set(b["hashes"]) if a["hashes"].get(k) != b["hashes"].get(k))
        doc = dict(what="tools/sgm_same_bits.py on the parent's library and on this change's, one process each, the same package: SHA-256 of "
                        "disp16, depth, C and S of StereoMatcher and of idx16, depth, the gradient bytes, pc, C and S of MotionStereo at the "
                        "sizes of tools/stereo_bench.py and tools/motion_stereo_bench.py", cases=len(a["hashes"]),
                   buffers=sum(len(v) for v in a["hashes"].values()), libraries_differ=a["library_sha256"] != b["library_sha256"],
                   differing=differing, equal=not differing, parent=a, change=b)
        with open(sys.argv[4], "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print("sgm_same_bits: %d cases, %d buffers, %d cases differ %s" % (doc["cases"], doc["buffers"], len(differing), differing))
        sys.exit(1 if differing else 0)
    import torch

    if not torch.cuda.is_available():
        sys.exit("sgm_same_bits: no GPU")
    from gsaj import _lib
    doc = dict(device=torch.cuda.get_device_name(0), library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), hashes=run(torch))
    with open(sys.argv[1], "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("sgm_same_bits: %d cases written to %s" % (len(doc["hashes"]), sys.argv[1]))


if __name__ == "__main__":
    main()
