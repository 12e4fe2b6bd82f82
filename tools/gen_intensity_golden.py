"""Record the golden vectors of the intensity statistics from the REFERENCE's own function and from scipy (authoring machine only:
needs the reference checkout and scipy; never runs where the tests run).

    python tools/gen_intensity_golden.py /path/to/reference

`_get_average_mapping` lives in a notebook cell (classification/train_ENC_CLF.ipynb cell 9); it is taken out of the cell's source
with `ast`, together with the cell's STANDARD_RANGE, and run on a seeded 5 x 13 percentile database.  The densities are what
`plot_histogram` (classification/transfer/full_sample_classification.ipynb cell 9) asks of scipy: gaussian_kde(values)(np.linspace(
values.min(), values.max(), num=100)), here also with Silverman's rule, with the factor 0.3 and over `values[values > mean]`.
The positions are the float64 np.linspace of the (exact) float32 minimum and maximum, which is what the device computes; the
notebook's own call, given float32 scalars, returns these positions rounded to float32.

Writes tests/golden/intensity_stats.npz.  Data only.
"""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intensity_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VOLUMES = {"a": (61, (5, 7, 9), 1.0, 0.0), "b": (62, (7, 11, 37), 20.0, 17.3), "c": (63, (10, 10, 10), 1.0, 1.0e4)}   # seed, shape, scale, shift
BANDWIDTHS = {"scott": None, "silverman": "silverman", "f03": 0.3}
POSITIONS = 100


def reference_average_mapping(ref_root):
    nb = json.load(open(os.path.join(ref_root, "classification", "train_ENC_CLF.ipynb")))
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and "def _get_average_mapping" in src:
            break
    else:
        raise RuntimeError("no cell defines _get_average_mapping")
    src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith(("%", "!")))
    keep = []
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == "_get_average_mapping":
            keep.append(node)
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "STANDARD_RANGE" for t in node.targets):
            keep.append(node)
    assert len(keep) == 2, [type(k).__name__ for k in keep]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "train_ENC_CLF_cell", "exec"), ns)
    return ns["_get_average_mapping"]


def main(ref_root):
    from scipy.stats import gaussian_kde
    rec = {}
    fn = reference_average_mapping(ref_root)
    rng = np.random.default_rng(20261020)
    db = np.sort(rng.uniform(0.0, 900.0, size=(5, 13)), axis=1)
    db[1] *= 20.0                      # another scanner's range
    db[2, :3] = 0.0                    # background up to the 10th percentile
    rec["database"], rec["mapping"] = db, fn(db.copy())
    assert np.array_equal(rec["mapping"], intensity_ref.average_mapping_ref(db)), "restatement differs from the reference"
    flat = np.vstack([db, np.full((1, 13), 7.0)])          # an image without range: the nan_to_num branch
    with np.errstate(all="ignore"):
        rec["database_flat"], rec["mapping_flat"] = flat, fn(flat.copy())
    for name, (seed, shape, scale, shift) in VOLUMES.items():
        vol = (intensity_ref.t1_like(seed, shape) * np.float32(scale) + np.float32(shift)).astype(np.float32)
        rec["vol_" + name] = vol
        values = vol.ravel()
        for tag, sel in (("all", values), ("mask", values[values > values.mean()])):
            rec["pos_%s_%s" % (name, tag)] = positions = np.linspace(np.float64(sel.min()), np.float64(sel.max()), num=POSITIONS)
            for bw, method in BANDWIDTHS.items():
                rec["kde_%s_%s_%s" % (name, tag, bw)] = gaussian_kde(sel, bw_method=method)(positions)
    path = os.path.join(GOLDEN, "intensity_stats.npz")
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(rec)))


if __name__ == "__main__":
    main(sys.argv[1])
