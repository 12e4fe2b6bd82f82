"""Code-generation guard of the class-map loss kernels (CPU container: hipcc cross-compiles gfx950 without a GPU).

csrc/loss_index.h gives the class-map Dice, the cross-entropy / focal loss and the boundary loss one voxel walk, one row store and
one set of finalize helpers, as forced-inline templates around each kernel's per-voxel body.  That is only as good as the code the
compiler makes of it: the 32-class forwards sit at the edge of the register file.  This test compiles csrc/loss.hip, ce_loss.hip and
distance.hip device-only with the product's flags and holds every instantiation of the class-map kernels and their finalize kernels
to 0 bytes of scratch and to no fewer waves per SIMD than tests/golden/loss_family_resources.json records: the figures of the same
instantiations before the walk was shared, taken once from a cross-compile of that commit."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "tests", "golden", "loss_family_resources.json")
KERNELS = re.compile(r"dice_index_|ce_index_|boundary_|dice_finalize")


@pytest.mark.parametrize("src", ["loss.hip", "ce_loss.hip", "distance.hip"])
def test_class_map_kernels_keep_occupancy_and_spill_nothing(src, tmp_path):
    from mri_epilepsy_diagnosis_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc in this environment")
    with open(FIGURES) as f:
        want = json.load(f)["kernels"][src]
    cmd = [build.HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only",
                                                                         os.path.join(build.CSRC, src), "-o", str(tmp_path / "out.s")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                        r.stderr, flags=re.S)
    got = {name: (int(vg), int(ag), int(scratch), int(occ)) for name, vg, ag, scratch, occ in blocks if KERNELS.search(name)}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))      # every instantiation, and no other
    bad = []
    for name, (vg, ag, scratch, occ) in sorted(got.items()):
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d waves/SIMD (recorded: %d VGPRs, %d AGPRs, %d waves/SIMD)"
              % (name, vg, ag, scratch, occ, want[name]["vgprs"], want[name]["agprs"], want[name]["occupancy"]))
        if scratch != 0 or occ < want[name]["occupancy"]:
            bad.append((name, vg, ag, scratch, occ, want[name]))
    assert not bad, bad
