"""Alpha in passes and on tiled objects, the parts that need no GPU (docs/alpha.md "Passes" and "Tiled"): the tiled Python
twin of alphaProblem held to the no-device hook, message for message; the new calls in the header, in the libraries and
in PRODUCT_SYMBOLS."""

import os
import re

import alpha_reference as A
import scale_filter_reference as F
from helpers import ROOT
from joshupscale_amd import runtime as R


def c_problem(lib, mode, filt, src, out):
    rc = lib.ju_debug_tiled_alpha_problem(mode, filt, src[0], src[1], out[0], out[1])
    return rc, (lib.ju_last_error().decode() if rc else "")


def test_the_tiled_limits_and_their_message_match_between_c_and_python(hip_library):
    lib = hip_library
    # (mode, filter, tiled source (w, h), output size (w, h) -- (0, 0): none, the output frame is four times the source)
    cases = [(A.ZERO, 0, (96, 60), (0, 0)), (A.OPAQUE, 3, (96, 60), (0, 0)), (A.SOURCE, 0, (96, 60), (0, 0)),
             (A.SOURCE, 2, (1280, 720), (1920, 1080)), (A.SOURCE, 0, (4096, 2304), (16384, 9216)),
             (A.SOURCE, 0, (4097, 2304), (0, 0)),                 # four times the source is beyond 16384
             (A.SOURCE, 0, (96, 60), (6, 4)), (A.SOURCE, 0, (96, 60), (5, 4)),  # 16 : 1 and just beyond
             (A.SOURCE, 2, (96, 60), (12, 8)), (A.SOURCE, 3, (96, 60), (11, 8)),  # a cubic filter: 8 : 1
             (A.SOURCE, 0, (96, 60), (1536, 960)), (A.SOURCE, 0, (96, 60), (1537, 960)),  # 1 : 16
             (A.SOURCE, 0, (96, 60), (96, 1)), (3, 0, (96, 60), (0, 0)), (-1, 0, (96, 60), (0, 0)), (A.SOURCE, 1, (96, 60), (0, 0)),
             (A.OPAQUE, 4, (96, 60), (384, 240)), (A.OPAQUE, 0, (96, 60), (5, 4))]
    refused = 0
    for mode, filt, src, out in cases:
        text = R.tiled_alpha_problem(mode, filt, src[0], src[1], out[0], out[1])
        frame = out if out != (0, 0) else (4 * src[0], 4 * src[1])
        assert text == R.alpha_problem(mode, filt, src[0], src[1], frame[0], frame[1])
        assert bool(text) == A.problem(mode, filt, src[0], src[1], frame[0], frame[1]), (mode, filt, src, out)
        want = (1, "std::invalid_argument: ju_tiled_set_alpha: " + text) if text else (0, "")
        assert c_problem(lib, mode, filt, src, out) == want, (mode, filt, src, out)
        if text and mode == A.SOURCE and filt in F.FILTERS:       # the message names alpha and both sizes
            assert "alpha" in text and f"{src[0]}x{src[1]}" in text and f"{frame[0]}x{frame[1]}" in text
        refused += bool(text)
    assert 0 < refused < len(cases)


def test_the_declared_surface(hip_library, product_library):
    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    for name in ("ju_set_alpha_lookahead", "ju_set_alpha_group", "ju_tiled_set_alpha", "ju_tiled_get_alpha"):
        assert name in declared("joshupscale_amd.h") and name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
        assert hasattr(product_library, name) and hasattr(hip_library, name)
    name = "ju_debug_tiled_alpha_problem"
    assert name in declared("joshupscale_amd_test.h") and name not in declared("joshupscale_amd.h")
    assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, name) and not hasattr(product_library, name)
    for cls, names in ((R.Runtime, ("set_alpha_lookahead", "set_alpha_group")), (R.TiledRuntime, ("set_alpha", "get_alpha"))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    for key in ("alpha_lookahead", "alpha_group", "lookahead_alpha_frames", "group_alpha_frames"):
        assert f'"{key}"' in header
    assert "Not covered: alpha inside passes" not in header
