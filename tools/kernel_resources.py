#!/usr/bin/env python3
"""Registers, LDS, scratch and occupancy of every kernel of csrc/ as the compiler reports them (hipcc --offload-arch=gfx950
-Rpass-analysis=kernel-resource-usage; no GPU needed), for this tree and for another tree's csrc/ (the parent's), side by side
in the form of profiles/r11_scan_refactor_resources.json.

    git archive HEAD gs-slam-analytica_jacobian_amd/csrc include | tar -x -C /tmp/parent
    python tools/kernel_resources.py --parent /tmp/parent/gs-slam-analytica_jacobian_amd/csrc --changed k_loss_finalize \\
        --loss-forms "k_render_fwd<true>" "k_render_bwd<true>" --out profiles/r14_fused_batch_resources.json

--changed: kernels allowed to differ at all; --loss-forms: kernels that may differ in registers but must keep LDS, have no scratch
and not lose occupancy; every other kernel must be identical in VGPRs, SGPRs, LDS, scratch and occupancy."""
import argparse
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOCONTRACT = {"preprocess.hip", "seed.hip", "frame.hip", "densify_prune.hip", "map_step.hip", "eval.hip", "pyramid.hip", "ingest.hip", "stereo.hip", "align.hip", "sweep.hip"}  # csrc/Makefile
KEYS = (("sgprs", r"^(?:Total)?SGPRs: (\d+)"), ("vgprs", r"^VGPRs: (\d+)"), ("agprs", r"^AGPRs: (\d+)"),
        ("scratch_bytes", r"^ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"^Occupancy \[waves/SIMD\]: (\d+)"),
        ("lds_bytes", r"^LDS Size \[bytes/block\]: (\d+)"))


def one(csrc, f):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    if f in NOCONTRACT:
        cmd.append("-ffp-contract=off")
    cmd += ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", f, "-o", os.devnull]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f + "\n" + r.stderr[-3000:])
    ks, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", line)
        if not m:
            continue
        t = m.group(1).strip()
        m2 = re.match(r"Function Name: (\S+)", t)
        if m2:
            name = subprocess.run(["c++filt", m2.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void ", "", name).split("(")[0]
            cur = {"file": f, "kernel": name, "res": {}}
            ks.append(cur)
            continue
        for key, pat in KEYS:
            m3 = re.match(pat, t)
            if m3 and cur is not None:
                cur["res"][key] = int(m3.group(1))
    return ks


def tree(csrc):
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(8) as ex:
        return {(k["file"], k["kernel"]): k["res"] for ks in ex.map(lambda f: one(csrc, f), files) for k in ks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="csrc/ of the tree to compare against")
    ap.add_argument("--changed", nargs="*", default=[])
    ap.add_argument("--loss-forms", nargs="*", default=[])
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    par, br = tree(a.parent), tree(os.path.join(ROOT, "gs-slam-analytica_jacobian_amd", "csrc"))
    violations, kernels = [], []
    for key in sorted(set(par) | set(br)):
        p, b = par.get(key), br.get(key)
        kernels.append({"file": key[0], "kernel": key[1], "parent": p, "branch": b})
        if key[1] in a.changed:
            continue
        if p is None or b is None:
            violations.append("%s %s exists in one tree only" % key)
        elif key[1] in a.loss_forms:
            if b["scratch_bytes"] or b["lds_bytes"] != p["lds_bytes"] or b["occupancy"] < p["occupancy"]:
                violations.append("%s %s: %r -> %r" % (key + (p, b)))
        elif p != b:
            violations.append("%s %s: %r -> %r" % (key + (p, b)))
    doc = {"method": "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC (+ -ffp-contract=off on %s) -Rpass-analysis=kernel-resource-usage "
                     "--cuda-device-only, every .hip of csrc/, the parent against this change" % ", ".join(sorted(NOCONTRACT)),
           "requirement": "every kernel%s identical in VGPRs, SGPRs, AGPRs, LDS, scratch and occupancy%s" % (
               " except " + ", ".join(a.changed + a.loss_forms) if a.changed or a.loss_forms else "",
               "; %s: no scratch, LDS unchanged, occupancy not below the parent's" % ", ".join(a.loss_forms) if a.loss_forms else ""),
           "violations": violations, "kernels": kernels}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("%d kernels, %d violations -> %s" % (len(kernels), len(violations), a.out))
    for v in violations:
        print("  " + v)
    return 1 if violations else 0


if __name__ == "__main__":
    sys.exit(main())
