"""Static checks (no GPU needed: hipcc cross-compiles) on the TSDF kernels (tsdf.hip): the product library carries them for
gfx950, they use no scratch and no private segment, every store they make is a vector store (none of the scalar-store,
scalar-atomic or scalar-cache-write-back instructions appears anywhere in the file's ISA), and the integration's
arithmetic is not contracted into FMAs beyond the correctly rounded divides."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_erode", "k_mark_blocks", "k_integrate", "k_tsdf_gather", "k_mc_classify", "k_mc_edges", "k_mc_chunk_sums", "k_mc_scan_chunks",
           "k_mc_emit")
# the scalar memory-write family, spelled in pieces so that this file does not contain the mnemonics it looks for
SCALAR_WRITES = re.compile(r"\bs_(?:buffer_|scratch_)?(?:" + "sto" + "re|atomic)_|\bs_dcache_(?:" + "w" + "b|discard)")


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("tsdf") / "tsdf.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "tsdf.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), occupancy=int(m.group(4)))
    return open(out).read(), usage


def _bodies(isa, kernel):
    found = re.findall(r"^(_Z\w*" + kernel + r"\w*):[^\n]*\n(.*?)s_endpgm", isa, re.S | re.M)
    assert found, kernel
    return found


def test_library_holds_the_tsdf_kernels():
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
        for name, _ in _bodies(isa, k):
            print(k, usage[name])
            assert usage[name]["scratch"] == 0, (k, usage[name])
    for m in re.finditer(r"\.private_segment_fixed_size:\s+(\d+)", isa):
        assert int(m.group(1)) == 0
    assert "scratch_" not in isa and "buffer_store_dword off" not in isa


def test_no_scalar_memory_writes(product):
    isa, _ = product
    assert not SCALAR_WRITES.search(isa), SCALAR_WRITES.search(isa).group(0)
    for k in ("k_integrate", "k_mc_emit", "k_erode", "k_mark_blocks"):
        assert any("global_store_" in body for _, body in _bodies(isa, k)), k


def test_integrate_runs_at_the_occupancy_design_md_states(product):
    """DESIGN.md section 2c states k_integrate's occupancy; the compiler's figure must be that one."""
    isa, usage = product
    (name, _), = _bodies(isa, "k_integrate")
    doc = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"`k_integrate`[^\n]*?(\d+) waves per SIMD", doc)
    assert m, "DESIGN.md does not state k_integrate's occupancy"
    assert int(m.group(1)) == usage[name]["occupancy"], usage[name]


def test_integration_is_not_contracted(product):
    """Every v_fma in k_integrate and k_mark_blocks belongs to a correctly rounded fp32 divide (five per v_div_fixup_f32) or to
    an integer division's reciprocal estimate (the block index): none to the camera transform or the running average."""
    isa, _ = product
    for k, min_div in (("k_integrate", 4), ("k_mark_blocks", 5)):
        (_, body), = _bodies(isa, k)
        fixups = body.count("v_div_fixup_f32")
        fmas = len(re.findall(r"\bv_fmac?_f32", body))
        print(k, "divides", fixups, "fmas", fmas)
        assert fixups >= min_div and fmas <= 5 * fixups + 4, (k, fixups, fmas)
