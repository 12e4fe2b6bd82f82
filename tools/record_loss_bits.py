"""Record the bits of the loss family into tests/golden/loss_family_bits.json (on a machine with the GPU, from the repository
root, after building the library):

    python tools/record_loss_bits.py [--out FILE]

For every case of tests/loss_cases.py: bit_cases() (the float-target Dice, the class-map Dice, CE / focal alone and fused with that Dice, and the
boundary loss; both storage types, inputs from the seeded CPU generators of the test suites) the file holds the loss as its int32 bit pattern and the sha256 of the gradient's bytes
in NDHWC order.  tests/test_dice_gpu.py recomputes every case and asserts equality, which is how a change of csrc/loss_index.h, loss.hip,
ce_loss.hip or the boundary part of distance.hip that means to keep the arithmetic is held to it.

The file is valid for one toolchain: both sources are compiled with the default contraction mode, so another compiler may fuse other
multiply-adds and legitimately give other bits.  Re-recording is legitimate only then (or after a deliberate change of the
arithmetic), and only after the float64 parity cases of tests/test_dice_gpu.py and tests/test_labels_gpu.py pass with the new build;
never to make a refactor's changed bits pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import loss_cases
    from mri_epilepsy_diagnosis_amd import ops
    out = os.path.join(ROOT, "tests", "golden", "loss_family_bits.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    assert torch.cuda.is_available(), "recording needs the device"
    cases = {name: loss_cases.device_bits(ops, form, z, t, **kw) for name, form, z, t, kw in loss_cases.bit_cases()}
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), out))


if __name__ == "__main__":
    main()
