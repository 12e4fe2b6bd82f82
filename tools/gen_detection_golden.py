"""Record the golden vectors of the detection path from the REFERENCE's own loops (authoring machine only: needs the reference
checkout; never runs where the tests run).

    python tools/gen_detection_golden.py /path/to/reference

detection/patch_utils.py does not import (nibabel, nilearn, nipype, numba) and detection/model_utils.py is not valid Python
(notebook magics, one mis-indented method), so neither is imported: `get_all_patches_and_labels` and `get_only_patches` are taken
out of the first with `ast` — they are pure numpy — and the two model classes out of the text between `class PatchModel` and
`def train` of the second.

Writes tests/golden/detection_patches.npz (per case: template, volume, mask, h, w, the reference's patches of both functions and
its labels) and tests/golden/detection_state_keys.json (state_dict keys and shapes of PatchModel).  Data only.

The cases (Y a multiple of h in all of them: only then do the reference's shifted strips stay whole):
  a  20 x 12 x 3, h = w = 4
  b  21 x 12 x 3, h = w = 4          odd X: pins X // 2 and the mirror
  c  80 x 48 x 5, h = 16, w = 32     an empty strip, a strip with start >= mid (no side patches), strips with start + w > mid
                                     (side / middle overlap), and a mask that touches one side and one middle patch of the base
                                     grid and nothing else
"""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_functions(ref_root):
    src = open(os.path.join(ref_root, "detection", "patch_utils.py")).read()
    wanted = ("get_all_patches_and_labels", "get_only_patches")
    tree = ast.parse(src)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    ns = {"np": np}
    exec(compile(tree, "patch_utils.py", "exec"), ns)
    return ns[wanted[0]], ns[wanted[1]]


def reference_model(ref_root):
    import torch
    import torch.nn as nn
    lines = open(os.path.join(ref_root, "detection", "model_utils.py")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("class PatchModel"))
    last = next(i for i, l in enumerate(lines) if l.startswith("def train"))
    ns = {"torch": torch, "nn": nn}
    exec(compile("\n".join(lines[first:last]), "model_utils.py", "exec"), ns)
    return ns["PatchModel"]


def template(rng, shape, h, starts):
    """A template whose base strip j of slice z starts in column starts[z][j] (None: an empty strip) and ends at its mirror."""
    x, y, z = shape
    gm = np.zeros(shape, np.float32)
    for i in range(z):
        for j, s in enumerate(starts[i]):
            if s is None:
                continue
            block = (rng.random((x - 2 * s, h)) < 0.5) * rng.random((x - 2 * s, h))
            block[0, rng.integers(h)] = 0.5            # the start column itself holds a value
            gm[s:x - s, y - (j + 1) * h:y - j * h, i] = block
    return gm


def cases():
    rng = np.random.default_rng(20260101)
    out = {}
    for name, shape in (("a", (20, 12, 3)), ("b", (21, 12, 3))):
        h = w = 4
        starts = [[1, 3, None], [2, 6, 7], [None, 5, 1]]            # mid = 6: sides, no sides (6, 7), empty strips
        gm = template(rng, shape, h, starts)
        vol = rng.standard_normal(shape).astype(np.float32)
        mask = (rng.random(shape) < 0.02).astype(np.uint8)
        out[name] = (gm, vol, mask, h, w)
    shape, h, w = (80, 48, 5), 16, 32
    starts = [[3, 9, None], [1, 7, 5], [None, None, 12], [8, 2, 6], [4, None, 3]]   # mid = 8
    gm = template(rng, shape, h, starts)
    vol = rng.standard_normal(shape).astype(np.float32)
    mask = np.zeros(shape, np.uint8)
    # slice 1, strip 1 (rows 16..31, y = 16..31), start 7: column 20 lies under the side patch (7..38) and the middle patch (8..39)
    mask[20, 24, 1] = 1
    out["c"] = (gm, vol, mask, h, w)
    return out


def main(ref_root):
    get_all, get_only = reference_functions(ref_root)
    arrays = {}
    for name, (gm, vol, mask, h, w) in cases().items():
        only = get_only(vol, gm, h=h, w=w)
        both, labels = get_all(vol, gm, mask.astype(bool), h=h, w=w)
        for arr in (only, both):
            assert np.array_equal(arr.astype(np.float32).astype(arr.dtype), arr)      # a pure copy of float32 values
        arrays.update({name + "_gm": gm, name + "_vol": vol, name + "_mask": mask, name + "_hw": np.array([h, w], np.int32),
                       name + "_only": only.astype(np.float32), name + "_all": both.astype(np.float32),
                       name + "_labels": labels.astype(np.uint8)})
        print("case %s: %d base patches, %d with upsampling, %d positive" % (name, len(only), len(both), int(labels.sum())))
    np.savez_compressed(os.path.join(GOLDEN, "detection_patches.npz"), **arrays)
    model = reference_model(ref_root)()
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    with open(os.path.join(GOLDEN, "detection_state_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
    print("wrote", len(arrays), "arrays and", len(keys), "state_dict keys")


if __name__ == "__main__":
    main(sys.argv[1])
