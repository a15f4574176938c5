// The box of a tiled object's source mask (docs/tiled.md "A mask"; tests/tiled_mask_reference.py box): the rectangle of
// BLENDED coordinates outside which every pixel's mask texel is white, so that the stitch kernels read no mask and no source
// there and do exactly what the unmasked kernels do.  Computed once, when the mask is set, on the host.  Plain C++: no HIP.
//
// Pixel X of a B-wide frame reads texel floor((2 X + 1) MW / (2 B)) of an MW-wide mask -- monotone in X, so a mask column
// is sampled by one run of pixels or, where MW > B, by none.  Only SAMPLED texels count: the box is the bounding rectangle
// of the pixels whose texel is not white, and empty (all four 0) exactly when there is no such pixel.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ju {

constexpr std::size_t kMaskAxisMax = 16384;

struct MaskBox {
	int x0 = 0, y0 = 0, x1 = 0, y1 = 0;  // [x0, x1) x [y0, y1); empty: all 0
	bool empty() const { return x0 >= x1 || y0 >= y1; }
};

// the texel of an n-wide texture under the centre of pixel i of an `out`-wide frame
inline std::uint64_t maskTexel(std::uint64_t i, std::uint64_t n, std::uint64_t out) { return (2 * i + 1) * n / (2 * out); }

// What a mask of maskW x maskH over a blended frame of outW x outH cannot be, or "": the size limits of ju_set_source_mask,
// and the condition under which the kernels keep mask_blend_kernel's 32-bit texel arithmetic.
inline std::string maskSizeProblem(std::size_t maskW, std::size_t maskH, std::size_t outW, std::size_t outH) {
	if (maskW < 1 || maskH < 1 || maskW > kMaskAxisMax || maskH > kMaskAxisMax) return "the mask must be 1 .. 16384 pixels on each axis";
	const auto below32 = [](std::size_t out, std::size_t tex) {
		return out < (std::size_t{1} << 31) && 2ull * out * tex < (1ull << 32);
	};
	if (!below32(outW, maskW) || !below32(outH, maskH)) {
		return "a " + std::to_string(maskW) + "x" + std::to_string(maskH) + " mask over the blended frame " + std::to_string(outW) + "x" +
		       std::to_string(outH) + ": 2 x blended extent x mask extent must stay below 2^32";
	}
	return "";
}

// mask: the BGRX texel (0, 0) of maskW x maskH texels in HOST memory, rows `stride` bytes apart (either sign); X is ignored.
// outW x outH: the blended frame.  Sizes as maskSizeProblem allows.
inline MaskBox maskBox(const std::uint8_t *mask, std::ptrdiff_t stride, int maskW, int maskH, int outW, int outH) {
	// per axis the sampled texels in ascending order, with the first and the last pixel that reads each
	struct Run {
		int texel, first, last;
	};
	const auto runs = [](int n, int out) {
		std::vector<Run> r;
		for (int i = 0; i < out; ++i) {
			const int t = static_cast<int>(maskTexel(static_cast<std::uint64_t>(i), static_cast<std::uint64_t>(n), static_cast<std::uint64_t>(out)));
			if (r.empty() || r.back().texel != t) r.push_back(Run{t, i, i});
			r.back().last = i;
		}
		return r;
	};
	const std::vector<Run> cols = runs(maskW, outW), rows = runs(maskH, outH);
	const auto white = [](const std::uint8_t *p) { return static_cast<int>(p[0]) + p[1] + p[2] == 765; };
	int lo = -1, hi = -1, top = -1, bottom = -1;  // indices into cols / rows
	for (int j = 0; j < static_cast<int>(rows.size()); ++j) {
		const std::uint8_t *row = mask + static_cast<std::ptrdiff_t>(rows[static_cast<std::size_t>(j)].texel) * stride;
		for (int i = 0; i < static_cast<int>(cols.size()); ++i) {
			if (white(row + 4 * static_cast<std::ptrdiff_t>(cols[static_cast<std::size_t>(i)].texel))) continue;
			if (lo < 0 || i < lo) lo = i;
			if (i > hi) hi = i;
			if (top < 0) top = j;
			bottom = j;
		}
	}
	MaskBox box;
	if (top < 0) return box;
	box.x0 = cols[static_cast<std::size_t>(lo)].first;
	box.x1 = cols[static_cast<std::size_t>(hi)].last + 1;
	box.y0 = rows[static_cast<std::size_t>(top)].first;
	box.y1 = rows[static_cast<std::size_t>(bottom)].last + 1;
	return box;
}

}  // namespace ju
