// The host arithmetic of scaled frames inside look-ahead passes, stand-alone and under the address and undefined-behaviour
// sanitizers (tests/test_cxx_stage_passes.py): buildScaleAxis and scaleSpan (source_kernels.hip, its host side) at the sizes
// the passes use and at the ratio limits -- every row's taps sum to 4096 and stay inside the source, and the column span
// the launch sizes its LDS tile with covers every tile of the kernel -- and the slots of a staged pass (frame_geometry.h):
// their bytes and the rows a host caller's orientation binds.  No device call is made.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "frame_geometry.h"
#include "kernels.h"

namespace {

int g_Failed = 0;
#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
			++g_Failed;                                                     \
		}                                                                   \
	} while (0)

void axis(int n, int m, int filter) {
	const ju::ScaleAxisHost a = ju::buildScaleAxis(n, m, filter);
	CHECK(a.n == n && a.m == m && static_cast<int>(a.start.size()) == m);
	CHECK(a.taps.size() == static_cast<std::size_t>(m) * ju::kScaleTapPitch);
	for (int d = 0; d < m; ++d) {
		const std::uint16_t *row = a.taps.data() + static_cast<std::size_t>(d) * ju::kScaleTapPitch;
		const int count = row[ju::kScaleMaxTaps];
		CHECK(count >= 1 && count <= ju::kScaleMaxTaps);
		CHECK(a.start[d] >= 0 && a.start[d] + count <= n);
		long sum = 0, absSum = 0;
		for (int t = 0; t < count; ++t) {
			const long q = filter == ju::kScaleTriangle ? static_cast<long>(row[t]) : static_cast<long>(static_cast<std::int16_t>(row[t]));
			sum += q;
			absSum += q < 0 ? -q : q;
		}
		CHECK(sum == 4096);
		CHECK(absSum <= ju::kScaleAbsSumMax);
	}
	// the span: a multiple of 4 that holds every tile's columns from its first (rounded down to 4) to its last, with the
	// one column of slack on either side the signed form of the kernels reads
	const int span = ju::scaleSpan(a);
	CHECK(span >= 4 && span % 4 == 0);
	const int slack = filter == ju::kScaleTriangle ? 0 : 1;
	for (int d0 = 0; d0 < m; d0 += ju::kScaleTileW) {
		const int d1 = std::min(d0 + ju::kScaleTileW, m) - 1;
		int first = n, end = 0;
		for (int d = d0; d <= d1; ++d) {
			const int count = a.taps[static_cast<std::size_t>(d) * ju::kScaleTapPitch + ju::kScaleMaxTaps];
			first = std::min(first, a.start[d]);
			end = std::max(end, a.start[d] + count);
		}
		const int tileFirst = std::max(a.start[d0] - slack, 0) & ~3;
		const int tileEnd = std::min(a.start[d1] + a.taps[static_cast<std::size_t>(d1) * ju::kScaleTapPitch + ju::kScaleMaxTaps] + slack, n);
		CHECK(first >= tileFirst && end <= tileEnd);  // (every row of the tile inside what the tile loads)
		CHECK(tileEnd - tileFirst <= span);
	}
	// the LDS tile of the launch: 3 channels x kScaleTileH rows x the padded pitch, within 64 KB
	const std::size_t pitch = static_cast<std::size_t>(span + span / 32 + 1);
	CHECK(3 * ju::kScaleTileH * pitch * sizeof(unsigned) <= 64 * 1024);
}

void axes() {
	const int filters[] = {ju::kScaleTriangle, ju::kScaleCatmullRom, ju::kScaleMitchell};
	for (int filter : filters) {
		// the passes' sizes: 720p / 480p / 1080p sources for 480x270, the model's 1920x1080 to 720p and 2160p; the tests' sizes
		const int pairs[][2] = {{1280, 480}, {720, 270}, {720, 480}, {480, 270}, {1920, 480}, {1080, 270}, {1920, 1280}, {1080, 720},
		    {1920, 3840}, {1080, 2160}, {72, 48}, {48, 30}, {50, 48}, {34, 30}, {192, 128}, {120, 80}, {192, 288}, {120, 180}, {192, 130},
		    {120, 90}, {46, 24}, {23, 24}, {12, 24}, {24, 24}, {6, 96}, {4, 64}, {2, 32}, {8192, 1024}, {3, 2}};
		for (const auto &p : pairs) axis(p[0], p[1], filter);
		const int down = ju::scaleDownMax(filter);
		axis(64 * down, 64, filter);  // the ratio limits
		axis(1024, 1024 / down, filter);
		bool refused = false;
		try {
			ju::buildScaleAxis(64 * down + 1, 64, filter);
		} catch (const std::invalid_argument &) {
			refused = true;
		}
		CHECK(refused);
	}
	bool refused = false;
	try {
		ju::buildScaleAxis(48, 30, 1);  // (the reserved filter value)
	} catch (const std::invalid_argument &) {
		refused = true;
	}
	CHECK(refused);
}

void slots() {
	// 1280x720 in, 480x270 -> 1920x1080 model, 3840x2160 out: what the documents quote
	const ju::StageSlotBytes b = ju::stageSlotBytes(1280, 720, 480, 270, 1920, 1080, 3840, 2160);
	CHECK(b.source == 3686400 && b.input == 518400 && b.modelOutput == 8294400);
	CHECK(b.out8 == 33177600 && b.out16 == 66355200);
	const ju::StageSlotBytes big = ju::stageSlotBytes(8192, 8192, 8192, 8192, 16384, 16384, 16384, 16384);
	CHECK(big.out16 == 2147483648ull);  // (beyond 32 bits: size_t arithmetic throughout)
	// the rows a host caller's orientation binds, walked as a kernel does: every byte inside the slot, each row once
	for (bool topDown : {true, false}) {
		const std::size_t w = 50, h = 34;
		std::vector<std::uint8_t> slot(w * h * 4, 0);
		const ju::SlotRows r = ju::slotRows(w, h, topDown);
		CHECK(r.stride == (topDown ? 200 : -200));
		std::uint8_t *row = slot.data() + r.first;
		for (std::size_t y = 0; y < h; ++y, row += (y < h ? r.stride : 0)) {
			for (std::size_t x = 0; x < w * 4; ++x) row[x] += 1;
		}
		CHECK(std::all_of(slot.begin(), slot.end(), [](std::uint8_t v) { return v == 1; }));
		CHECK(r.first == (topDown ? 0u : (h - 1) * w * 4));
	}
}

}  // namespace

int main() {
	axes();
	slots();
	if (g_Failed) return 1;
	std::printf("stage_passes ok\n");
	return 0;
}
