"""Static checks (no GPU needed: hipcc cross-compiles) on the half-arithmetic instantiations of the marcher and the field hook
(nerf.hip, option "render_arith" 1 / 2): they exist for gfx950 — brick-free, fp16 operands, composite and parity mode, with and
without cone stepping — run their MLPs on v_mfma_f32_32x32x16_f16, round through fp32 -> fp16 converts (never a half-precision
or mixed-precision fma, which rounds once where the definition rounds twice), use no scratch, keep fp16 subnormals and hold no scalar memory
write; include/d2r.h documents the key."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# scalar stores / scalar atomics / scalar data-cache write-back and discard, spelled in pieces
FORBIDDEN = [re.compile(p) for p in (r"\bs_" + r"store_", r"\bs_buffer_" + r"store_", r"\bs_scratch_" + r"store_", r"\bs_" + r"atomic_",
                                     r"\bs_buffer_" + r"atomic_", r"\bs_dcache_" + r"wb", r"\bs_dcache_" + r"discard")]


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("nerf") / "nerf.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DD2R_MARCH_THREADS=768",
           "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", str(out), os.path.join(CSRC, "nerf.hip")]
    r = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=1800)
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S):
        usage[m.group(1)] = int(m.group(2))
    isa = open(out).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)s_endpgm", isa, re.S | re.M)}
    return isa, bodies, usage


def _half_kernels(bodies, arith):
    """k_march<COMPOSITE, 0, 0, -1, CONE, true, arith> and k_eval_points<-1, true, arith>"""
    march = [n for n in bodies if re.match(rf"_Z7k_marchILb[01]ELi0ELi0ELin1ELb[01]ELb1ELi{arith}EE", n)]
    points = [n for n in bodies if re.match(rf"_Z13k_eval_pointsILin1ELb1ELi{arith}EE", n)]
    return march, points


@pytest.mark.parametrize("arith", [1, 2])
def test_half_arithmetic_kernels_exist_and_are_few(product, arith):
    _, bodies, _ = product
    march, points = _half_kernels(bodies, arith)
    assert len(march) == 4 and len(points) == 1, (march, points)          # composite x cone; no brick or bf16 variants
    others = [n for n in bodies if re.search(rf"ELi{arith}EEv", n) and ("k_march" in n or "k_eval_points" in n) and n not in march + points]
    assert others == [], others


@pytest.mark.parametrize("arith", [1, 2])
def test_half_arithmetic_kernels_use_the_f16_mfma_and_no_scratch(product, arith):
    _, bodies, usage = product
    march, points = _half_kernels(bodies, arith)
    assert len(march) == 4 and len(points) == 1, (march, points)
    for n in march + points:
        body = bodies[n]
        assert usage[n] == 0, (n, usage[n])
        assert "scratch_" not in body
        assert "v_mfma_f32_32x32x16_f16" in body and "v_mfma_f32_32x32x16_bf16" not in body, n
        # one tile: 2+2 + 4 + 2+2 + 4+4 + 4 = 24 k-steps, every one its own MFMA followed by converts
        assert body.count("v_mfma_f32_32x32x16_f16") >= 24, n
        assert re.search(r"v_cvt_(pk_)?f16_f32", body), n
        # every rounding is an fp32 operation followed by a convert of its own: no half-precision fma, and no fma with a half RESULT
        # (v_fma_mixlo_f16 / _mixhi_ round the exact fma once, to half — not the definition's two roundings; measured on the GPU).
        # v_fma_mix_f32, half operands and an fp32 result, is the fp32 fma itself.
        assert not re.search(r"\bv_(pk_)?fma(c|ak|mk)?_f16\b", body) and not re.search(r"v_fma_mix(lo|hi)", body), n
        for p in FORBIDDEN:
            assert not p.search(body), (n, p.pattern)


def test_kernels_keep_fp16_subnormals(product):
    isa, bodies, _ = product
    names = sum((sum(_half_kernels(bodies, a), []) for a in (1, 2)), [])
    assert len(names) == 10
    for n in names:
        m = re.search(r"\.amdhsa_kernel " + re.escape(n) + r"\n(.*?)\.end_amdhsa_kernel", isa, re.S)
        assert m, n
        d = re.search(r"\.amdhsa_float_denorm_mode_16_64 (\d+)", m.group(1))
        assert d is None or int(d.group(1)) == 3, (n, d and d.group(1))       # 3 (the default when the directive is absent): keep input and output denormals


def test_library_holds_the_half_arithmetic_kernels():
    lib = os.path.join(REPO, "dream2real_amd", "libd2r.so")
    if not os.path.exists(lib):
        pytest.skip("libd2r.so not built")
    blob = open(lib, "rb").read()
    for arith in (1, 2):
        assert f"k_eval_pointsILin1ELb1ELi{arith}EE".encode() in blob
        assert f"ELi0ELi0ELin1ELb0ELb1ELi{arith}EE".encode() in blob


def test_header_documents_the_key():
    h = open(os.path.join(REPO, "include", "d2r.h")).read()
    doc = h[h.index("/* Tunables;"):h.index("D2R_API int d2r_ctx_set_option")]
    assert '"render_arith" (0 default, 1, 2)' in doc
    para = doc[doc.index('"render_arith"'):]
    for word in ("half", "k-step", "fp16", "mlp_f16", "d2r_nerf_eval_points"):
        assert word in para[:2500], word
    assert re.search(r"#define D2R_ABI_VERSION 10\b", h)
