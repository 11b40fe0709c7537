#!/usr/bin/env python3
"""The instruction streams of the kernels of some csrc/ files, this tree against another tree's csrc/ (the parent's), without a GPU: each
file compiled device-only to assembly with the Makefile's flags (hipcc --offload-arch=gfx950 --cuda-device-only -S), and per kernel the
instruction lines from the kernel's label to its end label compared with comments and directives dropped and register names,
basic-block labels, s_waitcnt counts and rel32 symbol references replaced by placeholders.  Writes, as the `assembly` block of a
tools/kernel_resources.py record (--into) or on its own (--out): per kernel the two instruction counts, whether the streams are
identical, and the v_writelane_b32 (SGPR spill) and scratch instruction counts of both trees.

    python tools/kernel_streams.py --parent /tmp/parent/gs-slam-analytica_jacobian_amd/csrc gaussian_bwd.hip pose_jac.hip \\
        --into profiles/r33_row_walk_resources.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

from kernel_resources import NOCONTRACT, ROOT


def kernels(csrc, f):
    """{mangled name: [instruction lines]} of one file's device code"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
        cmd += ["-ffp-contract=off"] if f in NOCONTRACT else []
        r = subprocess.run(cmd + ["--cuda-device-only", "-S", f, "-o", out], cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(f + "\n" + r.stderr[-3000:])
        text = open(out).read().splitlines()
    ks, cur = {}, None
    for line in text:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = ks.setdefault(m.group(1), [])
        elif re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
        elif cur is not None:
            t = line.split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                cur.append(t)
    return {k: v for k, v in ks.items() if v}


def norm(t):
    t = re.sub(r"\b[vsa]\[\d+:\d+\]", "R", t)
    t = re.sub(r"\b[vsa]\d+\b", "R", t)
    t = re.sub(r"\.LBB\d+_\d+", "L", t)
    t = re.sub(r"\b\w+@rel32@(lo|hi)\+\d+", "SYM", t)
    return re.sub(r"^s_waitcnt.*", "s_waitcnt", t)


def count(lines, pat):
    return sum(1 for t in lines if re.match(pat, t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="csrc/ of the tree to compare against")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--into", help="a kernel_resources.py record that gets the result as its `assembly` block")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for f in a.files:
        par, br = kernels(a.parent, f), kernels(os.path.join(ROOT, "gs-slam-analytica_jacobian_amd", "csrc"), f)
        names = sorted(set(par) | set(br))
        plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
        for k, d in zip(names, plain):
            p, b = par.get(k), br.get(k)
            row = {"file": f, "kernel": re.sub(r"^void ", "", d).split("(")[0]}
            for tag, lines in (("parent", p), ("branch", b)):
                row[tag] = None if lines is None else {"instructions": len(lines), "sgpr_spills_v_writelane": count(lines, r"v_writelane_b32"),
                                                       "scratch_instructions": count(lines, r"scratch_(load|store)")}
            row["stream_identical"] = p is not None and b is not None and [norm(t) for t in p] == [norm(t) for t in b]
            rows.append(row)
            print("%-14s %-34s %5s -> %5s  %s" % (f, row["kernel"], p and len(p), b and len(b), "identical" if row["stream_identical"] else "DIFFERS"))
    block = {"method": __doc__.split("\n\n")[0].replace("\n", " "), "files": a.files,
             "identical": sum(r["stream_identical"] for r in rows), "differing": [r["kernel"] for r in rows if not r["stream_identical"]], "kernels": rows}
    if a.into:
        doc = json.load(open(a.into))
        doc["assembly"] = block
    else:
        doc = block
    with open(a.into or a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
