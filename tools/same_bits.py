"""The harness of the *_same_bits.py tools: each names its cases and hashes their outputs (run), this writes and compares the records.

    GSAJ_LIB_PATH=<parent's library> python tools/X_same_bits.py PARENT.json
    python tools/X_same_bits.py CHANGE.json
    python tools/X_same_bits.py --compare PARENT.json CHANGE.json OUT.json     (exit status 1 if any case differs)

A record: the device, the SHA-256 of the library that was loaded and {case: {buffer: SHA-256}}."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _dump(doc, path):
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main(name, run, what, unit="cases", one_library=False):
    """name: the tool's; run(torch) -> {case: {buffer: hash}}; what: the comparison's description; unit: what a case is called in the
    comparison; one_library: the two records come from two trees on ONE library, not from two libraries"""
    if sys.argv[1] == "--compare":
        a, b = (json.load(open(p)) for p in sys.argv[2:4])
        differing = sorted(k for k in set(a["hashes"]) | set(b["hashes"]) if a["hashes"].get(k) != b["hashes"].get(k))
        doc = {"what": what, unit: len(a["hashes"]), "buffers": sum(len(v) for v in a["hashes"].values())}
        if not one_library:
            doc["libraries_differ"] = a["library_sha256"] != b["library_sha256"]
        doc.update(differing=differing, equal=not differing, parent=a, change=b)
        _dump(doc, sys.argv[4])
        if one_library:
            print("%s: %d %s, %d differ %s" % (name, doc[unit], unit, len(differing), differing))
        else:
            print("%s: %d %s, %d buffers, %d %s differ %s" % (name, doc[unit], unit, doc["buffers"], len(differing), unit, differing))
        sys.exit(1 if differing else 0)
    import torch

    if not torch.cuda.is_available():
        sys.exit("%s: no GPU" % name)
    from gsaj import _lib
    doc = dict(device=torch.cuda.get_device_name(0), library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), hashes=run(torch))
    _dump(doc, sys.argv[1])
    print("%s: %d %s written to %s" % (name, len(doc["hashes"]), unit, sys.argv[1]))
