#!/usr/bin/env python3
"""Every output of the frame-to-frame alignment's entry points (csrc/align.hip), as SHA-256: gsaj_rgbd_align and gsaj_rgbd_align8 on
tests/align_restated.py's parity scene at 2x2, 65x4, 97x61 and the long-fold 70x260, in the three modes (depth, photometric, w_depth = 0),
the joint form at each of align_joint_restated.EXPOSURES -- rows, row, pix_out, valid_out and the joint form's gain_out -- and the state
and the row of RgbdAligner and JointRgbdAligner after the default schedule on the 80x60 behaviour scene (m = 1, 2; levels = 2; with and
without depth; the joint form's current frame at e^0.1 I + 0.03).  Run once per library (GSAJ_LIB_PATH names the one to load), one
process each, the same package; the calls and their arguments are the same, so the two outputs must be equal hash for hash.

    GSAJ_LIB_PATH=<parent's library> python tools/align_same_bits.py PARENT.json
    python tools/align_same_bits.py CHANGE.json
    python tools/align_same_bits.py --compare PARENT.json CHANGE.json OUT.json
"""
from same_bits import main, sha

SIZES = ((2, 2), (65, 4), (97, 61), (70, 260))
BRIGHT = (0.1, 0.03)


def run(torch):
    import align_calls
    import align_joint_restated as aj
    import align_restated as ar

    out = {}
    for joint in (False, True):
        calls = align_calls.Calls(joint)
        form = "align8" if joint else "align"
        buffers = ("rows", "row", "pix", "valid") + (("gain",) if joint else ())
        for W, H in SIZES:
            for mode in ar.MODES:
                for e in aj.EXPOSURES if joint else (None,):
                    case = aj.parity_case8(W, H, mode, *e) if joint else ar.parity_case(W, H, mode)
                    _, t = calls.run(case)
                    out["%s/%dx%d/%s%s" % (form, W, H, mode, "/a%g_b%g" % e if joint else "")] = {k: sha(t[k]) for k in buffers}
        for m in (1.0, 2.0):
            for depth in (True, False):
                case = aj.behaviour_case8(m, depth, *BRIGHT) if joint else ar.behaviour_case(m, depth)
                al = calls.aligner()
                al.set_reference(align_calls.dev(case, "ref_color"), align_calls.dev(case, "ref_depth"), case["ref_w2c"])
                al.align(align_calls.dev(case, "cur_color"), align_calls.dev(case, "cur_depth"))
                out["%s/aligner/m%g/%s" % (form, m, "depth" if depth else "photometric")] = dict(state=sha(al.state), row=sha(al.row))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    main("align_same_bits", run, "tools/align_same_bits.py on the parent's library and on this change's, one process each, the same package: SHA-256 "
         "of every output of gsaj_rgbd_align and gsaj_rgbd_align8 on the parity cases and of the state and the row of both "
         "aligners after the default schedule")
