#!/usr/bin/env python3
"""Every output of the batched backward on the windows of tests/fused_chain_cases.py, as SHA-256: the small parametrisations, the
scene with planted runs across the row walk's group boundaries and the bench's cfg2 window in both record formats, each whole-window
(k_chain_window sums the instance rows itself) and split (k_gather_sums, gsum, then the chain) -- every array of OUTPUTS and every
view_sums(v).  Run once per library (GSAJ_LIB_PATH names the one to load), one process each, the same package; the calls and their
arguments are the same, so the two outputs must be equal hash for hash.

    GSAJ_LIB_PATH=<parent's library> python tools/backward_same_bits.py PARENT.json
    python tools/backward_same_bits.py CHANGE.json
    python tools/backward_same_bits.py --compare PARENT.json CHANGE.json OUT.json
"""
from same_bits import main, sha


def run(torch):
    import fused_chain_cases as cs

    cases = [("small/K%d_P%d_M%d_bits%d_blind%s" % c, cs.small_case(*c), cs.BG) for c in cs.SMALL]
    cases.append(("planted", cs.planted_case(), cs.BG))
    cases += [("cfg2/bits%d" % bits, cs.bench_case(bits), (0.0, 0.0, 0.0)) for bits in (32, 16)]
    out = {}
    for name, args, bg in cases:
        for split in (False, True):
            _, grads, sums = cs.window(*args, split, bg)
            out["%s/%s" % (name, "split" if split else "fused")] = dict(
                {n: sha(grads[n]) for n in cs.OUTPUTS}, **{"view_sums%d" % v: sha(s) for v, s in enumerate(sums)})
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    main("backward_same_bits", run, "tools/backward_same_bits.py on the parent's library and on this change's, one process each, the same package: "
         "SHA-256 of every gradient array and of every view's ten sums of the batched backward, whole-window and split, on the windows of "
         "tests/fused_chain_cases.py")
