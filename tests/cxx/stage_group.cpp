// The host arithmetic of scaled members inside group passes, stand-alone and under the address and undefined-behaviour
// sanitizers (tests/test_cxx_stage_group.py): the members table of launchScaleBgrxMembers (source_kernels.hip, its host
// side) -- each member's own pitch from its own axis, the launch's LDS the largest member's tile, the refusals -- and the
// slots one member of a staged group pass needs and what they cost (frame_geometry.h).  No device call is made: the
// table's pointers are host addresses that nothing dereferences.
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

template <typename Fn>
bool refused(Fn fn) {
	try {
		fn();
	} catch (const std::invalid_argument &) {
		return true;
	}
	return false;
}

// a member as a runtime's Scaler makes it: the axes of srcW x srcH -> dstW x dstH through `filter`
struct Axes {
	ju::ScaleAxisHost x, y;
	ju::ScaleAxisDev xd, yd;
	int span;
	Axes(int srcW, int srcH, int dstW, int dstH, int filter)
	    : x(ju::buildScaleAxis(srcW, dstW, filter)), y(ju::buildScaleAxis(srcH, dstH, filter)) {
		xd = ju::ScaleAxisDev{x.start.data(), x.taps.data(), filter};
		yd = ju::ScaleAxisDev{y.start.data(), y.taps.data(), filter};
		span = ju::scaleSpan(x);
	}
};

void members() {
	std::vector<std::uint8_t> image(64);
	std::uint8_t *p = image.data();
	// the group test's members into 24 x 16, the widest tile beside the narrowest into 480 x 16, and 720p sources for 480 x 270
	struct Case {
		int srcW, srcH, dstW, dstH, filter;
	};
	const Case cases[] = {{46, 30, 24, 16, ju::kScaleTriangle}, {23, 17, 24, 16, ju::kScaleCatmullRom}, {12, 8, 24, 16, ju::kScaleMitchell},
	    {24, 16, 24, 16, ju::kScaleTriangle}, {6, 4, 24, 16, ju::kScaleCatmullRom}, {1920, 64, 480, 16, ju::kScaleTriangle},
	    {480, 16, 480, 16, ju::kScaleMitchell}, {1280, 720, 480, 270, ju::kScaleTriangle}, {3840, 2160, 480, 270, ju::kScaleCatmullRom},
	    {7680, 270, 480, 270, ju::kScaleTriangle}};
	ju::ScaleMembers table{};
	std::size_t most = 0;
	int n = 0;
	for (const Case &c : cases) {
		const Axes a(c.srcW, c.srcH, c.dstW, c.dstH, c.filter);
		const ju::ScaleMember m = ju::scaleMember(p, -static_cast<std::ptrdiff_t>(c.srcW) * 4, c.srcW, p, 4 * c.dstW + 3, a.xd, a.yd, a.span);
		CHECK(m.pitch == a.span + a.span / 32 + 1 && m.srcW == c.srcW);
		CHECK(m.cubic == (c.filter != ju::kScaleTriangle ? 1 : 0));
		CHECK(m.xStart == a.x.start.data() && m.yTaps == a.y.taps.data() && m.srcStride == -static_cast<std::ptrdiff_t>(c.srcW) * 4);
		const std::size_t lds = static_cast<std::size_t>(3) * ju::kScaleTileH * static_cast<std::size_t>(m.pitch) * sizeof(unsigned);
		CHECK(lds <= 64 * 1024);
		ju::ScaleMembers one{};
		one.member[0] = m;
		CHECK(ju::scaleMembersLds(one, 1) == lds);
		if (n < ju::kFlowBatchMax) {
			table.member[n++] = m;
			most = lds > most ? lds : most;
			CHECK(ju::scaleMembersLds(table, n) == most);  // the launch's LDS: the largest member's tile, whatever the order
		}
		// the ends of the tile, as the kernel computes them from the member's own tables, stay inside the member's pitch
		for (int d0 = 0; d0 < c.dstW; d0 += ju::kScaleTileW) {
			const int d1 = (d0 + ju::kScaleTileW < c.dstW ? d0 + ju::kScaleTileW : c.dstW) - 1;
			const int slack = m.cubic ? 1 : 0;
			const int first = (a.x.start[d0] - slack > 0 ? a.x.start[d0] - slack : 0) & ~3;
			int end = a.x.start[d1] + a.x.taps[static_cast<std::size_t>(d1) * ju::kScaleTapPitch + ju::kScaleMaxTaps] + slack;
			end = end < c.srcW ? end : c.srcW;
			const int quads = (end - first + 3) >> 2;
			const int lastColumn = 4 * quads - 1;
			CHECK(lastColumn + (lastColumn >> 5) < m.pitch);
		}
	}
	CHECK(sizeof(ju::ScaleMembers) <= 640 && sizeof(ju::ScaleMember) * ju::kFlowBatchMax == sizeof(ju::ScaleMembers));
	// the refusals
	const Axes a(46, 30, 24, 16, ju::kScaleTriangle), cubic(46, 30, 24, 16, ju::kScaleMitchell);
	CHECK(refused([&] { ju::scaleMember(nullptr, 4, 46, p, 4, a.xd, a.yd, a.span); }));
	CHECK(refused([&] { ju::scaleMember(p, 4, 46, nullptr, 4, a.xd, a.yd, a.span); }));
	CHECK(refused([&] { ju::scaleMember(p, 4, 0, p, 4, a.xd, a.yd, a.span); }));
	CHECK(refused([&] { ju::scaleMember(p, 4, 46, p, 4, a.xd, a.yd, a.span + 2); }));
	CHECK(refused([&] { ju::scaleMember(p, 4, 46, p, 4, a.xd, cubic.yd, a.span); }));   // axes of two filters
	CHECK(refused([&] { ju::scaleMember(p, 4, 46, p, 4, ju::ScaleAxisDev{}, a.yd, a.span); }));
	CHECK(refused([&] { ju::scaleMember(p, 4, 8192, p, 4, a.xd, a.yd, 8192); }));       // a tile beyond 64 KB
	CHECK(refused([&] { ju::scaleMembersLds(table, 0); }));
	CHECK(refused([&] { ju::scaleMembersLds(table, ju::kFlowBatchMax + 1); }));
	ju::ScaleMembers empty{};
	CHECK(refused([&] { ju::scaleMembersLds(empty, 1); }));
}

void slots() {
	// 1280x720 in, 480x270 -> 1920x1080 model, 3840x2160 out: what the documents quote, per member
	const ju::StageSlotBytes b = ju::stageSlotBytes(1280, 720, 480, 270, 1920, 1080, 3840, 2160);
	using N = ju::StageSlotNeeds;
	auto same = [](const N &x, const N &y) {
		return x.source == y.source && x.input == y.input && x.modelOutput == y.modelOutput && x.out8 == y.out8 && x.out16 == y.out16;
	};
	// a mask alone: no slot; a plain member: none
	CHECK(same(ju::stageSlotNeeds(0, true, true, true), N{false, false, false, false, false}));
	CHECK(same(ju::stageSlotNeeds(2, true, true, false), N{false, false, false, false, false}));
	// a source size: the model-size input always, the source-size frame for a host or non-BGRX source only
	CHECK(same(ju::stageSlotNeeds(1, false, true, true), N{false, true, false, false, false}));
	CHECK(same(ju::stageSlotNeeds(3, true, false, false), N{true, true, false, false, false}));
	// an output size: the model-size output always, the 8-bit frame for a host or non-BGRX output, the 16-bit frame for a deep one
	CHECK(same(ju::stageSlotNeeds(4, true, false, false), N{false, false, true, false, false}));
	CHECK(same(ju::stageSlotNeeds(6, false, true, false), N{false, false, true, true, false}));
	CHECK(same(ju::stageSlotNeeds(7, true, true, true), N{true, true, true, true, true}));
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(0, true, true, true)) == 0);
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(1, false, false, false)) == 518400);                 // device BGRX 720p in
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(1, true, false, false)) == 518400 + 3686400);        // NV12 720p in
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(4, false, false, false)) == 8294400);                // device BGRX 2160p out
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(5, true, true, false)) == 518400 + 3686400 + 8294400 + 33177600);
	CHECK(ju::stageSlotTotal(b, ju::stageSlotNeeds(7, true, true, true)) == 518400 + 3686400 + 8294400 + 33177600 + 66355200);
	const ju::StageSlotBytes big = ju::stageSlotBytes(8192, 8192, 8192, 8192, 16384, 16384, 16384, 16384);
	CHECK(ju::stageSlotTotal(big, ju::stageSlotNeeds(7, true, true, true)) == 268435456ull * 2 + 1073741824ull * 2 + 2147483648ull);
}

}  // namespace

int main() {
	members();
	slots();
	if (g_Failed) return 1;
	std::printf("stage_group ok\n");
	return 0;
}
