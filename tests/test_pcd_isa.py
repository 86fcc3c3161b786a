"""Static checks (no GPU needed: hipcc cross-compiles) on the point-cloud renderer's kernels (pcd.hip): the product
library carries them for gfx950, they use no scratch and no private segment, the splats are the 64-bit atomic minima
the render rule is built on (global for the background, LDS for the candidates), and nothing contracts the fp32
projection into FMAs beyond the correctly rounded divides."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_pcd_splat_bg", "k_pcd_resolve_bg", "k_pcd_candidates")


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("pcd") / "pcd.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "pcd.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = int(m.group(2))
    return open(out).read(), usage


def _body(isa, kernel):
    m = re.search(r"^(_Z\w*" + kernel + r"\w*):[^\n]*\n(.*?)s_endpgm", isa, re.S | re.M)
    assert m, kernel
    return m.group(1), m.group(2)


def test_library_holds_the_pcd_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


def test_no_scratch_no_private_segment(product):
    isa, usage = product
    for k in KERNELS:
        name, _ = _body(isa, k)
        assert usage[name] == 0, (k, usage[name])
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", isa):
        assert int(m.group(1)) == 0
    assert "scratch_" not in isa and "buffer_store_dword off" not in isa


def test_splats_are_64_bit_atomic_minima(product):
    isa, _ = product
    assert "global_atomic_umin_x2" in _body(isa, "k_pcd_splat_bg")[1]
    assert "ds_min_u64" in _body(isa, "k_pcd_candidates")[1]


def test_projection_is_not_contracted(product):
    """Every v_fma in the kernels belongs to a correctly rounded fp32 divide (v_div_scale / v_div_fmas / v_div_fixup, five
    per v_div_fixup_f32) or to an integer division's reciprocal estimate (the tile's row index): none to the projection."""
    isa, _ = product
    for k in ("k_pcd_splat_bg", "k_pcd_candidates"):
        body = _body(isa, k)[1]
        fixups = body.count("v_div_fixup_f32")
        fmas = len(re.findall(r"\bv_fmac?_f32", body))
        assert fixups >= 2 and fmas <= 5 * fixups + 2, (k, fixups, fmas)
