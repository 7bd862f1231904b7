#!/usr/bin/env python3
"""tests/golden/reference_configs.json: the MODEL / PROBABILISTIC_INFERENCE values of every model x inference YAML pair of the
REFERENCE's configs/ tree, read by pod_compare_amd.config.setup_config (the `eval` tag of Base-RetinaNet.yaml is replaced by literal
sizes, never evaluated).  Values only: the files themselves are not stored."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refimport import REFERENCE_SRC  # noqa: E402
from pod_compare_amd import config  # noqa: E402

SECTIONS = ("MODEL", "PROBABILISTIC_INFERENCE")


def flat(d, p=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, p + k + "."))
        else:
            out[p + k] = [list(x) if isinstance(x, (list, tuple)) else x for x in v] if isinstance(v, (list, tuple)) else v
    return out


def pair_values(cfg_root, model_rel, inference_rel):
    cfg = config.setup_config(os.path.join(cfg_root, model_rel), os.path.join(cfg_root, inference_rel))
    return {sect: flat(cfg[sect]) for sect in SECTIONS}


def main():
    ref_cfg = os.path.join(REFERENCE_SRC, "configs")
    out = {}
    for m in sorted(glob.glob(ref_cfg + "/BDD-Detection/retinanet/retinanet*.yaml")):
        for i in sorted(glob.glob(ref_cfg + "/Inference/*.yaml")):
            mr, ir = os.path.relpath(m, ref_cfg), os.path.relpath(i, ref_cfg)
            out[mr + " + " + ir] = dict(model=mr, inference=ir, **pair_values(ref_cfg, mr, ir))
    path = os.path.join(ROOT, "tests", "golden", "reference_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(out), "pairs ->", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
