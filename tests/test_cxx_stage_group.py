"""The host arithmetic of scaled members inside group passes (docs/source_stage.md "Group passes") from a stand-alone
program, tests/cxx/stage_group.cpp, under the address and undefined-behaviour sanitizers on the host side: the members
table of launchScaleBgrxMembers (the host half of csrc/source_kernels.hip) -- each member's pitch, the launch's LDS size,
the refusals -- and the slots a member needs with their bytes (csrc/frame_geometry.h).  No GPU: the program makes no
device call."""

import os
import subprocess

from helpers import ROOT


def test_stage_group_host_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "stage_group")
    csrc = os.path.join(ROOT, "joshupscale_amd", "csrc")
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + sanitize +
                          [os.path.join(csrc, "source_kernels.hip"), "-x", "hip", os.path.join(ROOT, "tests", "cxx", "stage_group.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "stage_group ok", out.stdout + out.stderr
