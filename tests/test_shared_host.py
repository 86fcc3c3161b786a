"""The pure host parts of csrc/d2r_shared.h (staging layout, fp64 4x4 product and rigid inverse, colour packer), checked by a
stand-alone program: tests/shared_host_main.cpp includes the header alone, is built with hipcc and the library's floating-point
flags, and needs no device to run.  It prints one line per failure."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dream2real_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_layout_product_inverse_and_packer(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "shared_host")
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
           os.path.join(REPO, "tests", "shared_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
