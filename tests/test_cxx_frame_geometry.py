"""joshupscale_amd/csrc/frame_geometry.h (rows at a signed stride, byte ranges and their overlap, plane shapes, the staged
layout of a host frame) from a stand-alone host program, tests/cxx/frame_geometry.cpp, under the address and
undefined-behaviour sanitizers.  No GPU, no HIP header: the header is plain C++."""

import os
import subprocess

from helpers import ROOT


def test_frame_geometry_host_program(tmp_path):
    exe = str(tmp_path / "frame_geometry")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "frame_geometry.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "frame_geometry ok", out.stdout + out.stderr
