"""Static checks (no GPU needed: hipcc cross-compiles) on the thumbnail kernels of masks.hip: the product library carries them for
gfx950, none uses scratch, and the occupancy DESIGN.md section 2g states is the compiler's figure.  Resource usage only."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_thumb_init", "k_thumb_obj_stats", "k_thumb_complement", "k_thumb_comp_stats", "k_thumb_container", "k_thumb_pack",
           "k_thumb_blur_rows", "k_thumb_blur_cols", "k_thumb_compose")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("thumbs") / "masks.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "masks.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                         r".*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S):
        found[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), occupancy=int(m.group(4)), lds=int(m.group(5)))
    return found


def _one(found, kernel):
    hits = [u for n, u in found.items() if re.search(r"\d" + kernel + r"E", n)]
    assert len(hits) == 1, kernel
    return hits[0]


def test_library_holds_the_thumbnail_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    for k in KERNELS:
        assert k.encode() in blob, k


def test_no_scratch(usage):
    for k in KERNELS:
        assert _one(usage, k)["scratch"] == 0, k


def test_resources_are_the_ones_design_md_states(usage):
    doc = open(os.path.join(REPO, "DESIGN.md")).read()
    section = doc[doc.index("### 2g."):]
    for k in KERNELS:
        m = re.search(r"`" + k + r"`: (\d+) VGPRs, (\d+) B of LDS, (\d+) waves per SIMD", section)
        assert m, "DESIGN.md section 2g does not state the resources of " + k
        u = _one(usage, k)
        print(k, u)
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (u["vgprs"], u["lds"], u["occupancy"]), (k, u)
