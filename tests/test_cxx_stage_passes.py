"""The host arithmetic of scaled frames inside look-ahead passes (docs/source_stage.md "Passes") from a stand-alone program,
tests/cxx/stage_passes.cpp, under the address and undefined-behaviour sanitizers on the host side: buildScaleAxis and
scaleSpan (the host half of csrc/source_kernels.hip) at the passes' sizes and the ratio limits, the slots' bytes and the
rows a host caller's orientation binds (csrc/frame_geometry.h).  No GPU: the program makes no device call."""

import os
import subprocess

from helpers import ROOT


def test_stage_passes_host_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "stage_passes")
    csrc = os.path.join(ROOT, "joshupscale_amd", "csrc")
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + sanitize +
                          [os.path.join(csrc, "source_kernels.hip"), "-x", "hip", os.path.join(ROOT, "tests", "cxx", "stage_passes.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "stage_passes ok", out.stdout + out.stderr
