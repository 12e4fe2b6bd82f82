"""Record the bits of the tissue family into tests/golden/tissue_family_bits.json (on a machine with the GPU, from the repository
root, after building the library):

    python tools/record_tissue_bits.py [--out FILE]

For every entry of tests/tissue_bits.py: device_bits() (`em_pass`, `mrf_pass` and `apply` on the parity cases of tests/tissue_cases.py
and tests/tissue_mrf_cases.py, and a sweep over all 12 (classes, order) instances of the row kernels) the file holds the sha256 of the
output's bytes.  tests/test_tissue_mrf_gpu.py recomputes every entry and asserts equality, which is how a change of csrc/tissue.hip
that means to keep the arithmetic is held to it.

The file is valid for one toolchain, which it names: tissue.hip is compiled without contraction, but its digests depend on the device
`log` and `exp` as that compiler and its device library build them.  Re-recording is legitimate only with another toolchain (or after a
deliberate change of the arithmetic), and only after the float64 parity cases of tests/test_tissue_gpu.py and
tests/test_tissue_mrf_gpu.py pass with the new build; never to make a refactor's changed bits pass."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import tissue_bits
    from mri_epilepsy_diagnosis_amd import build, ops
    out = os.path.join(ROOT, "tests", "golden", "tissue_family_bits.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    assert torch.cuda.is_available(), "recording needs the device"
    version = subprocess.run([build.HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()
    toolchain = {"hipcc": [line for line in version if "version" in line], "flags": build.FLAGS + build.EXTRA_FLAGS["tissue.hip"],
                 "device": torch.cuda.get_device_name(0)}
    entries = tissue_bits.device_bits(ops)
    with open(out, "w") as f:
        json.dump({"toolchain": toolchain, "entries": entries}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d entries to %s" % (len(entries), out))


if __name__ == "__main__":
    main()
