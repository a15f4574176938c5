// The arithmetic of frames in memory, free of HIP and of the engine: rows at a signed stride, the bytes a frame covers,
// the shape of a format's planes and the layout of a host frame's planes in a device staging buffer.  Header-only.
//
// A format is passed in as its row of the table in kernels.h (YuvFormatInfo; `Info` below is any type with its fields
// `sampling`, `planes`, `sampleBytes`, `pixelBytes`), so that this header needs no HIP header and a host program can
// test it alone (tests/cxx/frame_geometry.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace ju {

// `rows` rows at a signed stride, `ptr` addressing the first LOGICAL row: the row lowest in memory, the distance between
// rows there, and whether memory order is logical order (a bottom-up frame: its lowest row is the last logical one)
struct RowSpan {
	std::uint8_t *lowest;
	std::size_t pitch;
	bool topDown;
};
inline RowSpan rowSpan(const void *ptr, std::ptrdiff_t stride, std::size_t rows) {
	auto *first = const_cast<std::uint8_t *>(static_cast<const std::uint8_t *>(ptr));
	const bool up = stride >= 0;
	return {up ? first : first + static_cast<std::ptrdiff_t>(rows - 1) * stride, static_cast<std::size_t>(up ? stride : -stride), up};
}

// The bytes those rows cover, [begin, end): from the lowest row's first byte to the highest row's last
struct ByteRange {
	const std::uint8_t *begin = nullptr, *end = nullptr;
};
inline ByteRange rowsRange(const void *ptr, std::ptrdiff_t stride, std::size_t rows, std::size_t rowBytes) {
	const RowSpan s = rowSpan(ptr, stride, rows);
	return {s.lowest, s.lowest + (rows - 1) * s.pitch + rowBytes};
}
inline bool overlap(const ByteRange &a, const ByteRange &b) { return a.begin < b.end && b.begin < a.end; }

// The bytes of every plane of a frame (BGRX: its one image) and their address space (host and device addresses are
// different spaces: equal addresses there are different bytes).  No planes: a frame that covers no bytes of any space.
struct FrameExtent {
	ByteRange plane[3];
	int planes = 0;
	int space = 0;
};
inline bool overlap(const FrameExtent &a, const FrameExtent &b) {
	if (a.space != b.space) return false;
	for (int i = 0; i < a.planes; ++i) {
		for (int j = 0; j < b.planes; ++j) {
			if (overlap(a.plane[i], b.plane[j])) return true;
		}
	}
	return false;
}

// Plane k of a frame of the given size: rows, bytes per row (planar: Y, U, V or R, G, B; semi-planar: Y, UV; packed: one
// plane of pixelBytes per pixel -- YUY2 / UYVY 2, BGR24 3, RGBX 4, BGRX64 8, BGR96F 12; samples of 1, 2 or 4 bytes; a
// negative pixelBytes: V210's rows of 16 bytes per six pixels, the last group whole)
struct PlaneShape {
	std::size_t rows, rowBytes;
};
// A format = sampling (420 / 422 / 444; 0: RGB, every plane full size) x storage (planar / semi-planar Y, UV / packed: one
// plane) x sample size: all of it from the one table (kernels.h)
template <typename Info>
PlaneShape planeShape(const Info &info, std::size_t w, std::size_t h, int k) {
	const auto b = static_cast<std::size_t>(info.sampleBytes);
	if (info.planes == 1 && info.pixelBytes < 0) return {h, 16 * ((w + 5) / 6)};  // V210: whole groups of six pixels
	if (info.planes == 1) return {h, static_cast<std::size_t>(info.pixelBytes) * w};
	if (k == 0 || info.sampling == 0) return {h, w * b};
	const std::size_t cw = info.sampling == 444 ? w : w / 2;  // chroma samples per row (a semi-planar row holds both planes')
	return {info.sampling != 420 ? h : h / 2, (info.planes == 2 ? 2 * cw : cw) * b};
}

template <typename Info>
FrameExtent frameExtent(const Info &info, std::size_t w, std::size_t h, void *const planes[3], const std::ptrdiff_t strides[3],
    int space) {
	FrameExtent e;
	e.planes = info.planes;
	e.space = space;
	for (int k = 0; k < e.planes; ++k) {
		const PlaneShape p = planeShape(info, w, h, k);
		e.plane[k] = rowsRange(planes[k], strides[k], p.rows, p.rowBytes);
	}
	return e;
}
// (a BGRX image: one plane of 4 bytes per pixel)
inline FrameExtent imageExtent(const void *ptr, std::ptrdiff_t stride, std::size_t w, std::size_t h, int space) {
	FrameExtent e;
	e.planes = 1;
	e.space = space;
	e.plane[0] = rowsRange(ptr, stride, h, w * 4);
	return e;
}

// A host frame's planes in a device staging buffer: plane after plane, rows padded to stagePitch, in the caller's MEMORY
// order -- a bottom-up plane stays bottom-up there and the kernel addresses it from its last row with a negative pitch.
// Per plane: where its rows begin (what a copy of the plane's rows in memory order addresses), its first LOGICAL row and
// the signed pitch a kernel walks from there.
inline std::size_t stagePitch(std::size_t rowBytes) { return (rowBytes + 63) / 64 * 64; }
struct StagedLayout {
	struct Plane {
		std::size_t begin, first;
		std::ptrdiff_t pitch;
	};
	Plane plane[3] = {};
	std::size_t bytes = 0;
};
template <typename Info>
StagedLayout stagedLayout(const Info &info, std::size_t w, std::size_t h, const std::ptrdiff_t strides[3]) {
	StagedLayout l;
	for (int k = 0; k < info.planes; ++k) {
		const PlaneShape p = planeShape(info, w, h, k);
		const std::size_t pitch = stagePitch(p.rowBytes);
		const bool up = strides[k] >= 0;
		l.plane[k] = {l.bytes, up ? l.bytes : l.bytes + (p.rows - 1) * pitch,
		    up ? static_cast<std::ptrdiff_t>(pitch) : -static_cast<std::ptrdiff_t>(pitch)};
		l.bytes += pitch * p.rows;
	}
	return l;
}

// bytes of a staging buffer that holds a frame of the size in any format of `table` (BGR96F and the three f32 planes of
// RGBPS take the most: 12 bytes per pixel and the row padding)
template <typename Table>
std::size_t yuvStageBytes(const Table &table, std::size_t w, std::size_t h) {
	const std::ptrdiff_t up[3] = {1, 1, 1};
	std::size_t most = 0;
	for (const auto &info : table) {
		const std::size_t n = stagedLayout(info, w, h, up).bytes;
		most = n > most ? n : most;
	}
	return most;
}

// A look-ahead pass's own dense BGRX image of width x height bound to a host caller's row order (Engine::bindSide): the
// image is copied in MEMORY order, so a bottom-up caller's first logical row is the image's last and the kernels walk it
// with a negative stride.  `first`: the byte offset of the first logical row.
struct SlotRows {
	std::size_t first;
	std::ptrdiff_t stride;
};
inline SlotRows slotRows(std::size_t width, std::size_t height, bool topDown) {
	const std::size_t row = width * 4;
	return topDown ? SlotRows{0, static_cast<std::ptrdiff_t>(row)} : SlotRows{(height - 1) * row, -static_cast<std::ptrdiff_t>(row)};
}

// Bytes of the slots of one frame of a staged pass (Engine::bindFrame; docs/output_stage.md "Passes"): the BGRX frame at
// source size, the model-size input and output, the 8-bit and the 16-bit frame at output size.
struct StageSlotBytes {
	std::size_t source, input, modelOutput, out8, out16;
};
inline StageSlotBytes stageSlotBytes(std::size_t srcW, std::size_t srcH, std::size_t inW, std::size_t inH, std::size_t modelW,
    std::size_t modelH, std::size_t outW, std::size_t outH) {
	return {srcW * srcH * 4, inW * inH * 4, modelW * modelH * 4, outW * outH * 4, outW * outH * 8};
}

// Which of those slots one frame of a staged look-ahead pass, or one member of a staged group pass, needs
// (Engine::bindFrame; docs/source_stage.md "Group passes"): stage = bit 0 a source size, bit 1 a mask, bit 2 an output
// size; stagedIn / stagedOut: the side is a host image or not BGRX (a device BGRX image is read / written where it is);
// deepOut: a deep format encoded from the f16 state.  A mask alone needs none: the blend is in place over the frame the
// plain pass binds.
struct StageSlotNeeds {
	bool source, input, modelOutput, out8, out16;
};
inline StageSlotNeeds stageSlotNeeds(int stage, bool stagedIn, bool stagedOut, bool deepOut) {
	const bool scaledIn = (stage & 1) != 0, scaledOut = (stage & 4) != 0;
	return {scaledIn && stagedIn, scaledIn, scaledOut, scaledOut && stagedOut, scaledOut && deepOut};
}
inline std::size_t stageSlotTotal(const StageSlotBytes &b, const StageSlotNeeds &n) {
	return (n.source ? b.source : 0) + (n.input ? b.input : 0) + (n.modelOutput ? b.modelOutput : 0) + (n.out8 ? b.out8 : 0) +
	       (n.out16 ? b.out16 : 0);
}

}  // namespace ju
