"""Static checks (no GPU needed: hipcc cross-compiles) on the mask kernels (masks.hip): the product library carries them for
gfx950, none uses scratch or a private segment, and the occupancy DESIGN.md states for the labelling and closing kernels is the
compiler's figure."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_scene_bounds", "k_morph", "k_unpack", "k_label_tiles", "k_label_seams", "k_label_flatten", "k_comp_stats", "k_select_init",
           "k_select", "k_prune_write", "k_mask_lut")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("masks") / "masks.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "masks.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S):
        found[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), occupancy=int(m.group(4)))
    return open(out).read(), found


def _named(found, kernel):
    hits = {n: u for n, u in found.items() if re.search(r"\d" + kernel + r"(?:I|E)", n)}
    assert hits, kernel
    return hits


def test_library_holds_the_mask_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


def test_no_scratch_no_private_segment(usage):
    isa, found = usage
    for k in KERNELS:
        for name, u in _named(found, k).items():
            print(k, u)
            assert u["scratch"] == 0, (name, u)
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", isa):
        assert int(m.group(1)) == 0


def test_labelling_and_closing_run_at_the_occupancy_design_md_states(usage):
    _, found = usage
    doc = open(os.path.join(REPO, "DESIGN.md")).read()
    for k in ("k_morph", "k_label_tiles", "k_label_seams", "k_label_flatten"):
        m = re.search(r"`" + k + r"`[^\n]*?(\d+) waves per SIMD", doc)
        assert m, "DESIGN.md does not state the occupancy of " + k
        for name, u in _named(found, k).items():
            assert int(m.group(1)) == u["occupancy"], (name, u)
