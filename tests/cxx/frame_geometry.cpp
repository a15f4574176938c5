// joshupscale_amd/csrc/frame_geometry.h alone, on the host (tests/test_cxx_frame_geometry.py builds this with
// -fsanitize=address,undefined): the cases no other test reaches in isolation.  Formats are rows of the table in
// kernels.h, restated here by their four geometry fields -- the header takes any type that has them.
#include <cstdio>
#include <initializer_list>

#include "frame_geometry.h"

namespace {

struct Format {
	const char *name;
	int sampling, planes, sampleBytes, pixelBytes;
};
// one format of each sampling and storage kind (kernels.h, kFormatTable)
constexpr Format kI420{"I420", 420, 3, 1, 0}, kNv12{"NV12", 420, 2, 1, 0}, kP010{"P010", 420, 2, 2, 0}, kYuy2{"YUY2", 422, 1, 1, 2},
    kI422{"I422", 422, 3, 1, 0}, kP210{"P210", 422, 2, 2, 0}, kI444{"I444", 444, 3, 1, 0}, kI410{"I410", 444, 3, 2, 0},
    kBgr24{"BGR24", 0, 1, 1, 3}, kRgbps{"RGBPS", 0, 3, 4, 0}, kBgr96f{"BGR96F", 0, 1, 4, 12};

int g_Failed = 0;
#define CHECK(cond)                                                            \
	do {                                                                       \
		if (!(cond)) {                                                         \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
			++g_Failed;                                                        \
		}                                                                      \
	} while (0)

bool shapeIs(const Format &f, std::size_t w, std::size_t h, int k, std::size_t rows, std::size_t rowBytes) {
	const ju::PlaneShape p = ju::planeShape(f, w, h, k);
	if (p.rows == rows && p.rowBytes == rowBytes) return true;
	std::printf("%s %zux%zu plane %d: %zu rows of %zu bytes, expected %zu of %zu\n", f.name, w, h, k, p.rows, p.rowBytes, rows,
	    rowBytes);
	return false;
}

void rows() {
	std::uint8_t mem[64] = {};
	// one row: the stride does not matter, whatever its sign
	for (std::ptrdiff_t stride : {16, -16, 40, -40}) {
		const ju::RowSpan s = ju::rowSpan(mem + 8, stride, 1);
		CHECK(s.lowest == mem + 8 && s.topDown == (stride > 0));
		const ju::ByteRange r = ju::rowsRange(mem + 8, stride, 1, 12);
		CHECK(r.begin == mem + 8 && r.end == mem + 20);
	}
	// bottom-up: the first logical row is the highest in memory, the lowest row is the last logical one
	const ju::RowSpan up = ju::rowSpan(mem + 48, -16, 4);
	CHECK(up.lowest == mem && up.pitch == 16 && !up.topDown);
	const ju::ByteRange r = ju::rowsRange(mem + 48, -16, 4, 10);
	CHECK(r.begin == mem && r.end == mem + 58);
	const ju::RowSpan down = ju::rowSpan(mem, 16, 4);
	CHECK(down.lowest == mem && down.pitch == 16 && down.topDown);
}

void overlaps() {
	std::uint8_t mem[256] = {};
	constexpr int kHost = 0, kDevice = 1;
	// two images that touch: a.end == b.begin
	const ju::FrameExtent a = ju::imageExtent(mem, 16, 4, 4, kHost), b = ju::imageExtent(mem + 64, 16, 4, 4, kHost);
	CHECK(a.plane[0].end == b.plane[0].begin);
	CHECK(!ju::overlap(a, b) && !ju::overlap(b, a));
	const ju::FrameExtent c = ju::imageExtent(mem + 63, 16, 4, 4, kHost);
	CHECK(ju::overlap(a, c) && ju::overlap(c, a) && ju::overlap(b, c));
	// the same with the second image bottom-up (its ptr addresses its highest row)
	const ju::FrameExtent bUp = ju::imageExtent(mem + 64 + 48, -16, 4, 4, kHost);
	CHECK(bUp.plane[0].begin == mem + 64 && !ju::overlap(a, bUp) && ju::overlap(b, bUp));
	// equal addresses in different address spaces are different bytes
	const ju::FrameExtent aDev = ju::imageExtent(mem, 16, 4, 4, kDevice);
	CHECK(!ju::overlap(a, aDev) && ju::overlap(aDev, aDev));
	// three planes of which the third alone lies over the image: every plane counts
	void *planes[3] = {mem + 128, mem + 160, mem + 60};
	const std::ptrdiff_t strides[3] = {4, 2, 2};
	const ju::FrameExtent yuv = ju::frameExtent(kI420, 4, 4, planes, strides, kHost);
	CHECK(yuv.planes == 3 && yuv.plane[2].begin == mem + 60 && yuv.plane[2].end == mem + 64);
	CHECK(ju::overlap(yuv, a) && ju::overlap(a, yuv) && !ju::overlap(yuv, b));
	planes[2] = mem + 64;
	CHECK(!ju::overlap(ju::frameExtent(kI420, 4, 4, planes, strides, kHost), a));
	// a frame without planes (a graphics resource) covers nothing
	CHECK(!ju::overlap(ju::FrameExtent{}, a) && !ju::overlap(a, ju::FrameExtent{}));
}

void shapes() {
	// 2x2: the smallest frame every format takes
	CHECK(shapeIs(kI420, 2, 2, 0, 2, 2) && shapeIs(kI420, 2, 2, 1, 1, 1) && shapeIs(kI420, 2, 2, 2, 1, 1));
	CHECK(shapeIs(kNv12, 2, 2, 0, 2, 2) && shapeIs(kNv12, 2, 2, 1, 1, 2));
	CHECK(shapeIs(kP010, 2, 2, 0, 2, 4) && shapeIs(kP010, 2, 2, 1, 1, 4));
	CHECK(shapeIs(kYuy2, 2, 2, 0, 2, 4));
	CHECK(shapeIs(kI422, 2, 2, 0, 2, 2) && shapeIs(kI422, 2, 2, 1, 2, 1) && shapeIs(kI422, 2, 2, 2, 2, 1));
	CHECK(shapeIs(kP210, 2, 2, 0, 2, 4) && shapeIs(kP210, 2, 2, 1, 2, 4));
	CHECK(shapeIs(kI444, 2, 2, 0, 2, 2) && shapeIs(kI444, 2, 2, 2, 2, 2));
	CHECK(shapeIs(kI410, 2, 2, 0, 2, 4) && shapeIs(kI410, 2, 2, 1, 2, 4));
	CHECK(shapeIs(kBgr24, 2, 2, 0, 2, 6) && shapeIs(kBgr96f, 2, 2, 0, 2, 24));
	CHECK(shapeIs(kRgbps, 2, 2, 0, 2, 8) && shapeIs(kRgbps, 2, 2, 2, 2, 8));
	// 4:4:4 and RGB take odd sizes: no plane loses a column or a row
	CHECK(shapeIs(kI444, 7, 3, 0, 3, 7) && shapeIs(kI444, 7, 3, 1, 3, 7) && shapeIs(kI444, 7, 3, 2, 3, 7));
	CHECK(shapeIs(kI410, 7, 3, 2, 3, 14) && shapeIs(kBgr24, 7, 3, 0, 3, 21) && shapeIs(kRgbps, 7, 3, 1, 3, 28));
}

void staging() {
	CHECK(ju::stagePitch(1) == 64 && ju::stagePitch(64) == 64 && ju::stagePitch(65) == 128);
	// NV12 70x6, both planes bottom-up: Y 6 rows of 70 bytes (pitch 128), UV 3 rows of 70 bytes
	const std::ptrdiff_t upsideDown[3] = {-100, -80, 0};
	const ju::StagedLayout nv12 = ju::stagedLayout(kNv12, 70, 6, upsideDown);
	CHECK(nv12.plane[0].begin == 0 && nv12.plane[0].first == 5 * 128 && nv12.plane[0].pitch == -128);
	CHECK(nv12.plane[1].begin == 6 * 128 && nv12.plane[1].first == 6 * 128 + 2 * 128 && nv12.plane[1].pitch == -128);
	CHECK(nv12.bytes == 9 * 128);
	// ... and with a top-down chroma plane under a bottom-up luma plane
	const std::ptrdiff_t mixed[3] = {-100, 80, 0};
	const ju::StagedLayout nv12Mixed = ju::stagedLayout(kNv12, 70, 6, mixed);
	CHECK(nv12Mixed.plane[0].first == 5 * 128 && nv12Mixed.plane[1].first == 6 * 128 && nv12Mixed.plane[1].pitch == 128);
	CHECK(nv12Mixed.bytes == nv12.bytes);
	// packed YUY2 70x6, top-down: one plane of 140-byte rows (pitch 192)
	const std::ptrdiff_t down[3] = {200, 0, 0};
	const ju::StagedLayout yuy2 = ju::stagedLayout(kYuy2, 70, 6, down);
	CHECK(yuy2.plane[0].begin == 0 && yuy2.plane[0].first == 0 && yuy2.plane[0].pitch == 192 && yuy2.bytes == 6 * 192);
	// the buffer for any format of a table holds each of them: here RGBPS's three planes of 280-byte rows (pitch 320) are
	// the most, ahead of BGR96F's rows of 840 bytes (pitch 896)
	const Format table[] = {kI420, kNv12, kP010, kYuy2, kI422, kP210, kI444, kI410, kBgr24, kRgbps, kBgr96f};
	const std::size_t most = ju::yuvStageBytes(table, 70, 6);
	CHECK(most == 18 * 320 && ju::stagedLayout(kBgr96f, 70, 6, down).bytes == 6 * 896);
	for (const Format &f : table) CHECK(ju::stagedLayout(f, 70, 6, down).bytes <= most);
	CHECK(nv12.bytes <= most && yuy2.bytes <= most);
	// a 1-row, 1-plane frame
	const ju::StagedLayout one = ju::stagedLayout(kBgr24, 5, 1, upsideDown);
	CHECK(one.plane[0].first == 0 && one.plane[0].pitch == -64 && one.bytes == 64);
}

}  // namespace

int main() {
	rows();
	overlaps();
	shapes();
	staging();
	if (g_Failed) return 1;
	std::printf("frame_geometry ok\n");
	return 0;
}
