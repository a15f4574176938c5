"""The alpha routing rule (docs/alpha.md "Passes") from a stand-alone program, tests/cxx/alpha_route.cpp, under the address
and undefined-behaviour sanitizers on the host side: csrc/alpha_route.h, which the single-frame route, the passes and the
tiled runtime share -- for every format on either side and every location the kind of slot and the rows a frame binds as
alpha source and as alpha sink.  No GPU: the program makes no device call."""

import os
import subprocess

from helpers import ROOT


def test_alpha_route_host_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "alpha_route")
    csrc = os.path.join(ROOT, "joshupscale_amd", "csrc")
    sanitize = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + sanitize +
                          ["-x", "hip", os.path.join(ROOT, "tests", "cxx", "alpha_route.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "alpha_route ok", out.stdout + out.stderr
