"""Group passes on frames of any format and with the scene detector (ju_process_group_frames, ju_set_scene_group): what can
be held without a GPU -- the declared and bound symbols, and the table of cuts of the rotated clips the GPU tests
(tests/test_gpu_scene_group.py, tests/test_gpu_group_frames.py) rest on."""

import scene_reference as S
from helpers import M
from joshupscale_amd import runtime as R
from test_c_abi import declared_functions

THR = S.KNOWN_THRESHOLD
MEMBERS, TICKS = 8, 13
# the cut steps of member k, whose frame t is clip[(t + k) % 13]: S.run(rotated, THR) on the CPU
ROTATED_CUTS = {0: [4, 7, 10, 12], 1: [3, 6, 9, 11, 12], 2: [2, 5, 8, 10, 11], 3: [4, 7, 9, 10], 4: [3, 6, 8, 9],
                5: [2, 5, 7, 8, 12], 6: [4, 6, 7, 11], 7: [3, 5, 6, 10]}


def rotated(clip, k):
    """Member k's clip: the known clip rotated by k."""
    return [clip[(t + k) % len(clip)] for t in range(len(clip))]


def test_the_headers_declare_and_the_module_binds_the_new_symbols():
    product, hooks = declared_functions(), declared_functions("joshupscale_amd_test.h")
    for name in ("ju_process_group_frames", "ju_set_scene_group"):
        assert name in product and name in R.PRODUCT_SYMBOLS, name
    for name in ("ju_debug_scene_group", "ju_debug_scene_clear_items"):
        assert name in hooks and name in R.HOOK_SYMBOLS and name not in product, name
    assert tuple(product) == R.PRODUCT_SYMBOLS and tuple(hooks) == R.HOOK_SYMBOLS
    assert callable(R.process_group_frames) and callable(R.Runtime.set_scene_group)
    lib = R.load_library(True)
    for name in ("ju_process_group_frames", "ju_set_scene_group", "ju_debug_scene_group", "ju_debug_scene_clear_items"):
        assert hasattr(lib, name), name
    plain = R.load_library(False)
    assert hasattr(plain, "ju_process_group_frames") and not hasattr(plain, "ju_debug_scene_group")


def test_the_rotated_clips_cut_where_the_gpu_tests_expect():
    clip = S.known_clip(M.synthetic_frames, 30, 48)
    assert len(clip) == TICKS
    cuts = {k: S.cuts(S.run(rotated(clip, k), THR)) for k in range(MEMBERS)}
    assert cuts == ROTATED_CUTS
    by_tick = {t: [k for k in range(MEMBERS) if t in cuts[k]] for t in range(TICKS)}
    assert by_tick[0] == [] and by_tick[1] == []
    assert by_tick[2] == [2, 5] and by_tick[6] == [1, 4, 6, 7] and by_tick[10] == [0, 2, 3, 7]
    for t in range(2, TICKS):
        assert len(by_tick[t]) >= 2 and MEMBERS - len(by_tick[t]) >= 4, (t, by_tick[t])
