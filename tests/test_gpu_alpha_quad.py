"""The alpha kernels (csrc/alpha_kernels.hip) through ju_debug_alpha_scale and ju_debug_alpha_fill at narrow destinations
-- widths 2, 3, 5, 6, 7, 33 and 66, where a group of four columns meets the row end -- for every source and sink kind, at
odd byte offsets, with padded and bottom-up rows, against tests/alpha_reference.py code for code with every other bit of
the destination and the guard bytes held.  A destination whose address and stride are multiples of the pixel size and one
where they are not must hold the same bytes for the same data.  (The sweep was written for the four-pixels-per-lane form
of docs/alpha.md, "Measured and not kept"; it pins the kernels that stayed at the same widths.)"""

import numpy as np
import pytest

import alpha_reference as A
import scale_filter_reference as F
from test_gpu_alpha import SINK_LAYOUTS, SRC_LAYOUTS, alpha_fill, alpha_scale, last_error, pixels, scaled_plane, source_codes
from test_gpu_yuv import DevPlane

pytestmark = pytest.mark.gpu

WIDTHS = (2, 3, 5, 6, 7, 33, 66)
SRC_HW = (10, 13)                        # 13 -> 2 is within a cubic filter's 8 : 1, 13 -> 66 within 1 : 16
PIXEL_BYTES = {"byte": 4, "word": 8, "bits": 4}


def dst_height(w):
    return 11 if w % 2 else 5            # more than one tile row (8) and less than one


def pixel_aligned(plane, kind):
    """Whether the destination's address and stride are multiples of the pixel size."""
    return plane.ptr % PIXEL_BYTES[kind] == 0 and plane.stride % PIXEL_BYTES[kind] == 0


@pytest.mark.parametrize("sink_kind", ["byte", "word", "bits"])
def test_scale_at_narrow_widths_equals_the_definition_at_every_alignment(sink_kind):
    case = 0
    alignments = set()
    for w in WIDTHS:
        dst_hw = (dst_height(w), w)
        for src_kind in A.KINDS:
            filt = F.FILTERS[case % 3]
            content = "random" if src_kind != "none" else "top"
            want_codes = A.code(sink_kind, scaled_plane(src_kind, content, SRC_HW, dst_hw, filt))
            got = []
            for k, sink_lay in enumerate(SINK_LAYOUTS[sink_kind]):
                case += 1
                src_rows = d_src = None
                if src_kind != "none":
                    src_lays = SRC_LAYOUTS[src_kind]
                    src_rows = pixels(src_kind, SRC_HW, source_codes(src_kind, content, SRC_HW), 40 + w)
                    d_src = DevPlane(src_rows, **src_lays[k % len(src_lays)])
                before = pixels(sink_kind, dst_hw, np.random.default_rng(w).integers(0, A.TOP[sink_kind] + 1, dst_hw), 41 + w)
                d_dst = DevPlane(before, **sink_lay)
                alignments.add(pixel_aligned(d_dst, sink_kind))
                rc = alpha_scale(src_kind, sink_kind, filt, d_dst, dst_hw, d_src, SRC_HW)
                assert rc == 0, (last_error(), w, src_kind, filt, sink_lay)
                d_dst.check(pixels(sink_kind, dst_hw, want_codes, 41 + w))    # (the colour bits and the guards survive)
                if d_src is not None:
                    d_src.check(src_rows)
                got.append(np.array(d_dst._rows(d_dst.buf.cpu().numpy())))
            assert all(np.array_equal(got[0], g) for g in got[1:]), (w, src_kind)   # the same bytes at every alignment
    assert alignments == ({True} if sink_kind == "bits" else {True, False})   # (two-bit words are always 4-byte aligned)


@pytest.mark.parametrize("sink_kind", ["byte", "word", "bits"])
def test_fill_at_narrow_widths_writes_the_top_code_and_nothing_else(sink_kind):
    alignments = set()
    for w in WIDTHS + (257, 260):                                 # (past 256 columns, at both phases of four)
        dst_hw = (dst_height(w), w)
        got = []
        for sink_lay in SINK_LAYOUTS[sink_kind]:
            d_dst = DevPlane(pixels(sink_kind, dst_hw, np.zeros(dst_hw, np.int64), 50 + w), **sink_lay)
            alignments.add(pixel_aligned(d_dst, sink_kind))
            assert alpha_fill(sink_kind, d_dst, dst_hw) == 0, (last_error(), w, sink_lay)
            d_dst.check(pixels(sink_kind, dst_hw, np.full(dst_hw, A.TOP[sink_kind]), 50 + w))
            got.append(np.array(d_dst._rows(d_dst.buf.cpu().numpy())))
        assert all(np.array_equal(got[0], g) for g in got[1:]), w
    assert alignments == ({True} if sink_kind == "bits" else {True, False})
