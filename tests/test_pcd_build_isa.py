"""Static checks (no GPU needed: hipcc cross-compiles) on the cloud-building kernels (pcdbuild.hip): the product library carries
them for gfx950, they use no scratch and no private segment, and in the kernels that hold the rule's fp64 arithmetic every
v_fma_f64 belongs to a correctly rounded divide: none to the products and sums whose order DESIGN.md 2b fixes."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_pb_erode_rows", "k_pb_erode_cols", "k_pb_points", "k_pb_scan_chunks", "k_pb_scan_tops", "k_pb_scan_add", "k_pb_gather",
           "k_pb_write_raw", "k_pb_seg_bounds", "k_pb_keys", "k_pb_hist", "k_pb_scatter", "k_pb_heads", "k_pb_runs", "k_pb_obj_runs",
           "k_pb_voxels")
FMA_PER_DIVIDE = 5       # v_div_scale x 2, v_rcp, five v_fma_f64, v_div_fmas, v_div_fixup


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("pcdbuild") / "pcdbuild.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "pcdbuild.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = int(m.group(2))
    return open(out).read(), usage


def _bodies(isa, kernel):
    """Every instantiation of the kernel: (symbol, body)."""
    found = re.findall(r"^(_Z\w*" + kernel + r"\w*):[^\n]*\n(.*?)s_endpgm", isa, re.S | re.M)
    assert found, kernel
    return found


def test_library_holds_the_build_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


def test_no_scratch_no_private_segment(product):
    isa, usage = product
    assert len(_bodies(isa, "k_pb_points")) == 2                 # the counting and the writing instantiation
    for k in KERNELS:
        for name, _ in _bodies(isa, k):
            assert usage[name] == 0, (k, usage[name])
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", isa):
        assert int(m.group(1)) == 0
    assert "scratch_" not in isa and "buffer_store_dword off" not in isa


def test_fp64_products_and_sums_are_not_contracted(product):
    """Back-projection: two fp64 divides (x, y) and the fp32 divide of the depth.  Voxel origin: one divide; keys: three; the
    voxel kernel: three means and three colours.  Each fp64 divide brings exactly five v_fma_f64 and nothing else does."""
    isa, _ = product
    for k, divides in (("k_pb_points", 2), ("k_pb_seg_bounds", 1), ("k_pb_keys", 3), ("k_pb_voxels", 6)):
        for name, body in _bodies(isa, k):
            fixups = body.count("v_div_fixup_f64")
            fmas = len(re.findall(r"\bv_fmac?_f64", body))
            assert fixups == divides and fmas == FMA_PER_DIVIDE * fixups, (name, fixups, fmas)
            assert "v_rcp_f64" in body and len(re.findall(r"\bv_mul_f64", body)) > 0
    for name, body in _bodies(isa, "k_pb_points"):
        assert body.count("v_div_fixup_f32") == 1                # (float)d16 / 1000.0f, correctly rounded
