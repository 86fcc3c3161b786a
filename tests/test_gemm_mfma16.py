"""Static checks (no GPU needed: hipcc cross-compiles) on the MFMA shape of the bf16 GEMMs.

Every bf16 Linear kernel, k_gemm8 and every k_gemm instantiation, issues v_mfma_f32_16x16x32_bf16 and no
v_mfma_f32_32x32x16_bf16: rows of one product go through different kernels (the layer-0 background rows and the
touched rows, a chunk's remainder), and bit-identical logits need one MFMA shape and one K order in all of them.
The shape change must not cost registers: no scratch, and the occupancy each kernel had on the 32x32x16 shape
(the round-6 K loops, in the history: docs/history/r27.md)."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _compile(tmp_path_factory, *defines):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("mfma16") / "clip.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           *defines, "-I" + os.path.join(CSRC, "..", "..", "include"), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(out), os.path.join(CSRC, "clip.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                         r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = dict(vgprs=int(m.group(2)), scratch=int(m.group(3)), occupancy=int(m.group(4)))
    return open(out).read(), usage


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    return _compile(tmp_path_factory)


def bf16_gemms(isa):
    """(mangled name, template arguments, body) of every k_gemm8 (not the fp8 k_gemm8f) and k_gemm instantiation."""
    for m in re.finditer(r"^(_Z\d+(k_gemm8?)I(\w*?)EEv\w*):[^\n]*\n(.*?)s_endpgm", isa, re.S | re.M):
        args = tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(3) + "E"))
        yield m.group(1), m.group(2), args, m.group(4)


def test_every_bf16_gemm_issues_the_16x16x32_mfma_only(product):
    isa, _ = product
    seen = {"k_gemm8": 0, "k_gemm": 0}
    for name, kernel, _, body in bf16_gemms(isa):
        seen[kernel] += 1
        assert "v_mfma_f32_16x16x32_bf16" in body, name
        assert "v_mfma_f32_32x32x16_bf16" not in body, name
    assert seen["k_gemm8"] >= 6 and seen["k_gemm"] >= 10, seen


def test_no_scratch_and_round6_occupancy(product):
    isa, usage = product
    n = 0
    for name, kernel, args, _ in bf16_gemms(isa):
        u = usage[name]
        assert u["scratch"] == 0, (name, u)
        if kernel == "k_gemm8":
            want = 2                                           # 512 threads, 2 waves per SIMD: <= 256 VGPRs
        elif args[1:] == (4, 2, 2, 3):
            want = 2 if args[0] == 8 else 3                    # 256x128: <= 168 VGPRs (EPI_RESID_STATS_SPLIT: 188 on 32x32x16)
        else:
            want = 2
        assert u["occupancy"] >= want and u["vgprs"] <= 512 // want, (name, u)
        n += 1
    assert n >= 16, n
