"""Static checks (no GPU needed: hipcc cross-compiles) on the kernels of the TSDF physics backend (DESIGN.md section 2e:
k_tsdf_touch_bits and k_tsdf_solid_* in tsdf.hip, k_sdf_coarse and k_sdf_check in sdfphys.hip): the product library carries
them for gfx950, and they use no scratch and no private segment."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"tsdf.hip": ("k_tsdf_touch_bits", "k_tsdf_solid_count", "k_tsdf_solid_scan", "k_tsdf_solid_emit"),
           "sdfphys.hip": ("k_sdf_coarse", "k_sdf_check")}


_compiled = {}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return lambda src: _compiled.get(src) or _compiled.setdefault(src, _compile(src, tmp_path_factory))


def _compile(src, tmp_path_factory):
    out = tmp_path_factory.mktemp("sdfphys") / (src + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, src)]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), occupancy=int(m.group(4)))
    return src, open(out).read(), usage


def test_library_holds_the_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob
    for names in KERNELS.values():
        for k in names:
            assert k.encode() in blob, k


@pytest.mark.parametrize("src", sorted(KERNELS))
def test_no_scratch_no_private_segment(product, src):
    src, isa, usage = product(src)
    for k in KERNELS[src]:
        found = re.findall(r"^(_Z\w*" + k + r"\w*):", isa, re.M)
        assert found, k
        for name in found:
            print(k, usage[name])
            assert usage[name]["scratch"] == 0, (k, usage[name])
            assert usage[name]["occupancy"] == 8, (k, usage[name])          # nothing here should cost occupancy
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", isa):
        assert int(m.group(1)) == 0
    assert "scratch_" not in isa


def test_the_check_is_not_contracted_and_divides_correctly(product):
    """A point's voxel is floor(c / voxel + 0.5) with a correctly rounded divide, and the rotation is plain multiplies and adds:
    every fp32 FMA of k_sdf_check belongs to a divide (five per v_div_fixup_f32)."""
    src, isa, _ = product("sdfphys.hip")
    (body,) = re.findall(r"^_Z\w*k_sdf_check\w*:[^\n]*\n(.*?)^\.Lfunc_end", isa, re.S | re.M)          # (the kernel has early exits: up to the function's end)
    fixups, fmas = body.count("v_div_fixup_f32"), len(re.findall(r"\bv_fmac?_f32", body))
    print("divides", fixups, "fmas", fmas)
    assert fixups >= 10 and fmas <= 5 * fixups + 4          # (+ an integer division's reciprocal estimate)
    assert "v_fma_f64" not in body and "v_fmac_f64" not in body                # nor is the fp64 composition of T
