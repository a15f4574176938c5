// The alpha routing rule, stand-alone and under the address and undefined-behaviour sanitizers
// (tests/test_cxx_alpha_route.py): csrc/alpha_route.h -- for every format on either side of a frame and every location,
// which kind of slot and which rows the frame binds as the alpha source and as the alpha sink.  The rows are host
// addresses that nothing dereferences; no device call is made.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "alpha_route.h"
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

using ju::PixelFormat;

// every format of the table (kernels.h) with the slot docs/alpha.md gives it
struct Slot {
	PixelFormat format;
	int kind;
};
const Slot kSlots[] = {{PixelFormat::Bgrx, ju::kAlphaByte}, {PixelFormat::I420, ju::kAlphaNone}, {PixelFormat::Nv12, ju::kAlphaNone},
    {PixelFormat::P010, ju::kAlphaNone}, {PixelFormat::I010, ju::kAlphaNone}, {PixelFormat::Yuy2, ju::kAlphaNone},
    {PixelFormat::Uyvy, ju::kAlphaNone}, {PixelFormat::I422, ju::kAlphaNone}, {PixelFormat::P210, ju::kAlphaNone},
    {PixelFormat::I210, ju::kAlphaNone}, {PixelFormat::I444, ju::kAlphaNone}, {PixelFormat::I410, ju::kAlphaNone},
    {PixelFormat::Bgr24, ju::kAlphaNone}, {PixelFormat::Rgb24, ju::kAlphaNone}, {PixelFormat::Rgbx, ju::kAlphaByte},
    {PixelFormat::Bgrx64, ju::kAlphaWord}, {PixelFormat::Rgbp8, ju::kAlphaNone}, {PixelFormat::Rgbp10, ju::kAlphaNone},
    {PixelFormat::Rgbp16, ju::kAlphaNone}, {PixelFormat::Rgbph, ju::kAlphaNone}, {PixelFormat::Rgbps, ju::kAlphaNone},
    {PixelFormat::Bgr96f, ju::kAlphaNone}, {PixelFormat::X2bgr10, ju::kAlphaBits}, {PixelFormat::X2rgb10, ju::kAlphaBits},
    {PixelFormat::V210, ju::kAlphaNone}, {PixelFormat::Y210, ju::kAlphaNone}, {PixelFormat::Y410, ju::kAlphaNone}};

// one side as a route binds it: the caller's memory and the route's staging, each with BGRX rows and a plane 0
struct Memory {
	std::vector<std::uint8_t> callerBgrx, callerPlane, stagedBgrx, stagedPlane;
	Memory() : callerBgrx(64), callerPlane(64), stagedBgrx(64), stagedPlane(64) {}
};

// what a route hands the rule for a side of `format` at `device`, top-down or bottom-up: a BGRX side has only BGRX rows --
// the caller's or the staged copy; any other side has the network's BGRX rows (always the route's own) and plane 0
ju::AlphaSide sideOf(const Memory &m, PixelFormat format, bool device, std::ptrdiff_t stride) {
	ju::AlphaSide s;
	s.planar = format != PixelFormat::Bgrx;
	s.format = format;
	const ju::AlphaSideRows callerBgrx{m.callerBgrx.data(), stride}, stagedBgrx{m.stagedBgrx.data(), stride};
	const ju::AlphaSideRows callerPlane{m.callerPlane.data(), stride}, stagedPlane{m.stagedPlane.data(), stride};
	s.bgrx = s.planar ? stagedBgrx : ju::alphaLocated(device, callerBgrx, stagedBgrx);
	if (s.planar) s.plane0 = ju::alphaLocated(device, callerPlane, stagedPlane);
	return s;
}

void kinds() {
	for (const Slot &slot : kSlots) CHECK(ju::alphaKind(slot.format) == slot.kind);
	// no format outside the table has a slot
	for (int f = -2; f < 64; ++f) {
		bool known = false;
		for (const Slot &slot : kSlots) known = known || ju::fmt(slot.format) == f;
		if (!known) CHECK(ju::alphaKind(static_cast<PixelFormat>(f)) == ju::kAlphaNone);
	}
}

void sides() {
	Memory in, out;
	int launched = 0, pairs = 0;
	for (const Slot &a : kSlots) {
		for (const Slot &b : kSlots) {
			for (int where = 0; where < 4; ++where) {  // (input device?, output device?)
				for (std::ptrdiff_t stride : {std::ptrdiff_t(16), std::ptrdiff_t(-16)}) {
					const bool inDevice = (where & 1) != 0, outDevice = (where & 2) != 0;
					const ju::AlphaRows src = ju::alphaRowsOf(sideOf(in, a.format, inDevice, stride));
					const ju::AlphaRows sink = ju::alphaRowsOf(sideOf(out, b.format, outDevice, stride));
					++pairs;
					// the source: the slot's kind, in the caller's memory for a device frame, else in the staged copy -- and of a
					// non-BGRX format never the decoded BGRX rows, whose X is 0
					CHECK(src.kind == a.kind);
					if (a.kind == ju::kAlphaNone) {
						CHECK(src.ptr == nullptr && src.stride == 0);  // (the opaque constant: nothing is read)
					} else if (a.format == PixelFormat::Bgrx) {
						CHECK(src.ptr == (inDevice ? in.callerBgrx.data() : in.stagedBgrx.data()) && src.stride == stride);
					} else {
						CHECK(src.ptr == (inDevice ? in.callerPlane.data() : in.stagedPlane.data()) && src.stride == stride);
						CHECK(src.ptr != in.stagedBgrx.data() && src.ptr != in.callerBgrx.data());
					}
					// the sink: likewise; a format without a slot gets no launch in any mode
					CHECK(sink.kind == b.kind);
					if (b.kind == ju::kAlphaNone) {
						CHECK(sink.ptr == nullptr);
					} else if (b.format == PixelFormat::Bgrx) {
						CHECK(sink.ptr == (outDevice ? out.callerBgrx.data() : out.stagedBgrx.data()) && sink.stride == stride);
					} else {
						CHECK(sink.ptr == (outDevice ? out.callerPlane.data() : out.stagedPlane.data()) && sink.stride == stride);
					}
					for (int mode : {ju::kAlphaZero, ju::kAlphaOpaque, ju::kAlphaSource}) {
						const bool launches = ju::alphaLaunches(mode, sink.kind);
						CHECK(launches == (mode != ju::kAlphaZero && b.kind != ju::kAlphaNone));
						launched += launches ? 1 : 0;
					}
				}
			}
		}
	}
	const int n = static_cast<int>(sizeof(kSlots) / sizeof(kSlots[0]));
	CHECK(pairs == n * n * 8);
	CHECK(launched == n * 5 * 8 * 2);  // (five formats with a slot, two modes that launch)
}

}  // namespace

int main() {
	kinds();
	sides();
	if (g_Failed) {
		std::printf("alpha_route: %d checks failed\n", g_Failed);
		return 1;
	}
	std::printf("alpha_route ok\n");
	return 0;
}
