// The tile of the scale kernels (source_kernels.hip, the head of that file) with the SOURCE of its vertical pass as a
// template parameter: the one body of scale_bgrx_kernel, its items and members forms and scale_state_kernel, whose sources
// are rows in memory, and of the tiled object's fused kernels (tile_kernels.hip), whose source is the blend of the tiles'
// outputs or states formed in registers.  One workgroup of 256 threads per tile of kScaleTileW x kScaleTileH destination
// pixels; vertical pass: sum qy * sample into LDS as [3][kScaleTileH][pitch], column c at c + c / 32; horizontal pass: a
// thread per destination pixel.  Everything but the vertical pass's loads is common, so the scaled bytes of every kernel
// built on a tile are those of scale_bgrx_kernel / scale_state_kernel by construction.
//
// A source of the 8-bit tile provides
//     Column column(int x, int row) const    what a lane keeps for source columns x .. x + 3 (x = 0 mod 4), at `row`
//     uint4 load(Column c, int x) const      the four BGRX pixels of the column's current row
//     Column next(Column c) const            the column one row further down
// and a source of the 16-bit tile the same for columns x, x + 1 (x even): load returns the two pixels as (B | G << 16, R,
// B | G << 16, R) in 16-bit words of the source's own kind, and its static sample(word) makes the 16-bit sample P of
// one.  A column past the source's width is never a tap: any value will do.  A source is made inside the tile from its
// Args (what the kernel was launched with), behind the tile's extent.
//
// Included by device code only; everything lives in the including file's unnamed namespace.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "kernel_common.h"
#include "kernels.h"

namespace ju {

namespace {
// The source columns of a tile of destination columns d0 .. d1: from the first tap of d0 to the last tap of d1 for the
// triangle, whose rows start and end in ascending order.  A cubic row loses a tap whose weight is exactly 0 at either
// end (Catmull-Rom at distance 1, Mitchell at 8/7), at most one per end, so a row inside the tile can reach one column
// further than the tile's outer rows (buildCubicAxis checks that it is never more): one column of slack on either side.
template <bool kSigned>
__host__ __device__ inline int tileFirst(int first) {
	return kSigned ? (first > 0 ? first - 1 : 0) : first;
}
template <bool kSigned>
__host__ __device__ inline int tileEnd(int end, int n) {
	return kSigned ? (end < n ? end + 1 : n) : end;
}

__device__ inline unsigned loadPixel(const std::uint8_t *p) {
	if ((reinterpret_cast<std::uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const unsigned *>(p);
	return static_cast<unsigned>(p[0]) | (static_cast<unsigned>(p[1]) << 8) | (static_cast<unsigned>(p[2]) << 16) |
	       (static_cast<unsigned>(p[3]) << 24);
}

__device__ inline void storePixel(std::uint8_t *p, unsigned v) {
	if ((reinterpret_cast<std::uintptr_t>(p) & 3) == 0) {
		*reinterpret_cast<unsigned *>(p) = v;
		return;
	}
	p[0] = static_cast<std::uint8_t>(v);
	p[1] = static_cast<std::uint8_t>(v >> 8);
	p[2] = static_cast<std::uint8_t>(v >> 16);
	p[3] = static_cast<std::uint8_t>(v >> 24);
}

// LDS column of tile column c: one word of padding per 32 columns (see the head of source_kernels.hip)
__device__ inline int ldsColumn(int c) { return c + (c >> 5); }

// the tables of one axis as the kernels take them (ScaleAxisDev without the host's choice of form)
struct ScaleTaps {
	const int *start;
	const std::uint16_t *taps;
};

// The two forms of a scale kernel.  Unsigned, the triangle: u16 taps, unsigned sums, no clamp (rows of non-negative taps
// summing to 4096 cannot leave the range).  Signed, the cubic filters: the same words read as i16, signed 32-bit
// vertical sums in LDS (|sum| <= top * 6144: < 2^21 for 8-bit samples, < 2^29 for 16-bit ones), a signed 64-bit horizontal
// sum (|sum| < 2^34 / 2^42), and the shifted result -- narrow again: below 2^18 in size -- clamped to 0 .. top.
template <bool kSigned>
struct ScaleForm {
	using Tap = std::conditional_t<kSigned, std::int16_t, std::uint16_t>;
	using Sum = std::conditional_t<kSigned, int, unsigned>;                    // a tap in a register; a vertical sum
	using Sum8 = std::conditional_t<kSigned, long long, unsigned>;             // the horizontal sum of 8-bit samples
	using Sum16 = std::conditional_t<kSigned, long long, unsigned long long>;  // ... of 16-bit samples
};

// (sum + 2^23) >> 24 of a horizontal sum that already holds the 2^23: floor; the signed form clamps to 0 .. kTop
template <bool kSigned, int kTop, typename T>
__device__ inline unsigned scaleResult(T sum) {
	if constexpr (kSigned) {
		return static_cast<unsigned>(min(max(static_cast<int>(sum >> 24), 0), kTop));
	} else {
		return static_cast<unsigned>(sum >> 24);
	}
}

// P of one f16 of the state, as StateSource::sample (colour_kernels.hip) forms it: exact in f32
__device__ inline unsigned stateSample(unsigned bits) {
	const float s = static_cast<float>(__builtin_bit_cast(f16, static_cast<unsigned short>(bits)));
	return static_cast<unsigned>(fminf(fmaxf(floorf((s + 0.5f) * 65536.0f), 0.0f), 65535.0f));
}

// BGRX rows in memory, any byte alignment and signed stride: 16 bytes per load where the rows are 16-byte aligned, so a
// wave reads contiguous row segments; else pixel by pixel, the column clamped to the row
struct ScaleRows8 {
	const std::uint8_t *src;
	std::ptrdiff_t stride;
	int width;
	std::uintptr_t low;  // the low bits of address and stride: 0 where every row is 16-byte aligned
	using Column = const std::uint8_t *;  // the current row
	struct Args {
		const std::uint8_t *src;
		std::ptrdiff_t stride;
		int width;
	};
	__device__ __forceinline__ explicit ScaleRows8(const Args &a)
	    : src(a.src), stride(a.stride), width(a.width),
	      low((reinterpret_cast<std::uintptr_t>(a.src) | static_cast<std::uintptr_t>(a.stride)) & 15) {}
	__device__ __forceinline__ Column column(int, int row) const { return src + static_cast<std::ptrdiff_t>(row) * stride; }
	__device__ __forceinline__ uint4 load(Column row, int x) const {
		unsigned px[4];
		const bool aligned = low == 0;
		if (aligned && x + 4 <= width) {
			const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * x);
			px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) px[k] = loadPixel(row + 4 * min(x + k, width - 1));  // (past the row: never a tap)
		}
		return make_uint4(px[0], px[1], px[2], px[3]);
	}
	__device__ __forceinline__ Column next(Column row) const { return row + stride; }
};

// The dense f16 state [srcH][width][4] (B, G, R, unused): 16 bytes per tap where the pair of columns is 16-byte aligned
// (every pair of an even width, every other row of an odd one), else two 8-byte loads, the column clamped to the row
struct ScaleState16 {
	const f16 *src;
	int width;
	std::size_t rowWords;  // f16 per state row
	using Column = const f16 *;  // the current row
	struct Args {
		const f16 *src;
		int width;
	};
	__device__ __forceinline__ explicit ScaleState16(const Args &a) : src(a.src), width(a.width), rowWords(static_cast<std::size_t>(a.width) * 4) {}
	__device__ __forceinline__ Column column(int, int row) const { return src + static_cast<std::size_t>(row) * rowWords; }
	__device__ __forceinline__ uint4 load(Column row, int x) const {
		const f16 *at = row + 4 * static_cast<std::size_t>(x);
		if (x + 2 <= width && (reinterpret_cast<std::uintptr_t>(at) & 15) == 0) return *reinterpret_cast<const uint4 *>(at);
		uint2 px[2];
#pragma unroll
		for (int k = 0; k < 2; ++k) {  // (past the row: never a tap)
			px[k] = *reinterpret_cast<const uint2 *>(row + 4 * static_cast<std::size_t>(min(x + k, width - 1)));
		}
		return make_uint4(px[0].x, px[0].y, px[1].x, px[1].y);
	}
	__device__ static __forceinline__ unsigned sample(unsigned bits) { return stateSample(bits); }  // (an f16 of the state)
	__device__ __forceinline__ Column next(Column row) const { return row + rowWords; }
};

// One tile of 8-bit samples: the workgroup's tile is blockIdx.x, blockIdx.y.  THE body of every launch form -- the single
// frame, the items of a look-ahead pass, the members of a group pass, the tiled object's fused blend -- so their bytes are
// equal by construction.  Sums: qy * sample <= 255 * 4096 < 2^20 (the signed form: below 2^21 in size), exact in an LDS
// word; the horizontal sum qx * LDS + 2^23 below 2^32 (signed: 64 bits).  dst: BGRX rows at any byte alignment, X = 0.
template <bool kSigned, typename Source>
__device__ __forceinline__ void scaleTile8(const typename Source::Args &args, int srcW, std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride,
    int dstW, int dstH, ScaleTaps ax, ScaleTaps ay, int pitch) {
	using Tap = typename ScaleForm<kSigned>::Tap;
	using Sum = typename ScaleForm<kSigned>::Sum;
	using Wide = typename ScaleForm<kSigned>::Sum8;
	extern __shared__ unsigned tileWords[];  // [3][kScaleTileH][pitch]: sum qy * src per channel
	Sum *tile = reinterpret_cast<Sum *>(tileWords);
	const int tid = threadIdx.x;
	const int dx0 = blockIdx.x * kScaleTileW, dy0 = blockIdx.y * kScaleTileH;
	const int dxLast = min(dx0 + kScaleTileW, dstW) - 1;
	const int xs0 = tileFirst<kSigned>(ax.start[dx0]) & ~3;
	const int xs1 = tileEnd<kSigned>(ax.start[dxLast] + ax.taps[dxLast * kScaleTapPitch + kScaleMaxTaps], srcW);
	const int quads = (xs1 - xs0 + 3) >> 2;
	const Source source(args);

	// vertical pass: item = (tile row, four source columns)
	for (int item = tid; item < kScaleTileH * quads; item += 256) {
		const int r = item / quads, q = item - r * quads;
		const int dy = dy0 + r;
		if (dy >= dstH) continue;
		const int x = xs0 + 4 * q;
		const Tap *qy = reinterpret_cast<const Tap *>(ay.taps) + dy * kScaleTapPitch;
		const int count = qy[kScaleMaxTaps];
		typename Source::Column column = source.column(x, ay.start[dy]);
		Sum acc[12];
#pragma unroll
		for (int i = 0; i < 12; ++i) acc[i] = 0;
		for (int t = 0; t < count; ++t, column = source.next(column)) {
			const Sum w = qy[t];
			const uint4 v = source.load(column, x);
			const unsigned px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				acc[3 * k] += w * static_cast<Sum>(px[k] & 255);
				acc[3 * k + 1] += w * static_cast<Sum>((px[k] >> 8) & 255);
				acc[3 * k + 2] += w * static_cast<Sum>((px[k] >> 16) & 255);
			}
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int col = ldsColumn(4 * q + k);
#pragma unroll
			for (int c = 0; c < 3; ++c) tile[(c * kScaleTileH + r) * pitch + col] = acc[3 * k + c];
		}
	}
	__syncthreads();

	// horizontal pass: a thread per destination pixel
	const int tx = tid & (kScaleTileW - 1), ty = tid / kScaleTileW;
	const int dx = dx0 + tx, dy = dy0 + ty;
	if (dx >= dstW || dy >= dstH) return;
	const Tap *qx = reinterpret_cast<const Tap *>(ax.taps) + dx * kScaleTapPitch;
	const int count = qx[kScaleMaxTaps];
	const int first = ax.start[dx] - xs0;
	Wide b = 1u << 23, g = 1u << 23, r = 1u << 23;
	const Sum *tb = tile + ty * pitch, *tg = tile + (kScaleTileH + ty) * pitch, *tr = tile + (2 * kScaleTileH + ty) * pitch;
	for (int t = 0; t < count; ++t) {
		const Wide w = qx[t];
		const int col = ldsColumn(first + t);
		b += w * tb[col];  // (the signed form: i32 x i32 + i64, one v_mad_i64_i32)
		g += w * tg[col];
		r += w * tr[col];
	}
	storePixel(dst + static_cast<std::ptrdiff_t>(dy) * dstStride + 4 * dx, scaleResult<kSigned, 255>(b) |
	    (scaleResult<kSigned, 255>(g) << 8) | (scaleResult<kSigned, 255>(r) << 16));
}

// One tile of 16-bit samples P -> the dense u16 frame [dstH][dstW][4] (B, G, R, 0): out = (sum qy qx P + 2^23) >> 24.  The
// tile, the tables and the LDS layout of scaleTile8; an item of the vertical pass is (tile row, two source columns).
// Vertical sums reach 65535 * 4096 < 2^28 (signed: 2^29 in size; 32 bits in LDS), the horizontal sum 2^40 (2^42): a 64-bit
// accumulator.  One 8-byte store per pixel.
template <bool kSigned, typename Source>
__device__ __forceinline__ void scaleTile16(const typename Source::Args &args, int srcW, std::uint16_t *dst, int dstW, int dstH,
    ScaleTaps ax, ScaleTaps ay, int pitch) {
	using Tap = typename ScaleForm<kSigned>::Tap;
	using Sum = typename ScaleForm<kSigned>::Sum;
	using Wide = typename ScaleForm<kSigned>::Sum16;
	extern __shared__ unsigned tileWords[];  // [3][kScaleTileH][pitch]: sum qy * P per channel, below 2^28 (signed: 2^29 in size)
	Sum *tile = reinterpret_cast<Sum *>(tileWords);
	const int tid = threadIdx.x;
	const int dx0 = blockIdx.x * kScaleTileW, dy0 = blockIdx.y * kScaleTileH;
	const int dxLast = min(dx0 + kScaleTileW, dstW) - 1;
	const int xs0 = tileFirst<kSigned>(ax.start[dx0]) & ~3;
	const int xs1 = tileEnd<kSigned>(ax.start[dxLast] + ax.taps[dxLast * kScaleTapPitch + kScaleMaxTaps], srcW);
	const int pairs = (xs1 - xs0 + 1) >> 1;
	const Source source(args);

	for (int item = tid; item < kScaleTileH * pairs; item += 256) {
		const int r = item / pairs, q = item - r * pairs;
		const int dy = dy0 + r;
		if (dy >= dstH) continue;
		const int x = xs0 + 2 * q;
		const Tap *qy = reinterpret_cast<const Tap *>(ay.taps) + dy * kScaleTapPitch;
		const int count = qy[kScaleMaxTaps];
		typename Source::Column column = source.column(x, ay.start[dy]);
		Sum acc[6];
#pragma unroll
		for (int i = 0; i < 6; ++i) acc[i] = 0;
		for (int t = 0; t < count; ++t, column = source.next(column)) {
			const Sum w = qy[t];
			const uint4 v = source.load(column, x);
			const uint2 px[2] = {make_uint2(v.x, v.y), make_uint2(v.z, v.w)};
#pragma unroll
			for (int k = 0; k < 2; ++k) {
				acc[3 * k] += w * static_cast<Sum>(Source::sample(px[k].x & 0xffff));
				acc[3 * k + 1] += w * static_cast<Sum>(Source::sample(px[k].x >> 16));
				acc[3 * k + 2] += w * static_cast<Sum>(Source::sample(px[k].y & 0xffff));
			}
		}
#pragma unroll
		for (int k = 0; k < 2; ++k) {
			const int col = ldsColumn(2 * q + k);
#pragma unroll
			for (int c = 0; c < 3; ++c) tile[(c * kScaleTileH + r) * pitch + col] = acc[3 * k + c];
		}
	}
	__syncthreads();

	const int tx = tid & (kScaleTileW - 1), ty = tid / kScaleTileW;
	const int dx = dx0 + tx, dy = dy0 + ty;
	if (dx >= dstW || dy >= dstH) return;
	const Tap *qx = reinterpret_cast<const Tap *>(ax.taps) + dx * kScaleTapPitch;
	const int count = qx[kScaleMaxTaps];
	const int first = ax.start[dx] - xs0;
	Wide b = 1u << 23, g = 1u << 23, r = 1u << 23;  // (each sum stays below 2^40; the signed form: 2^42 in size)
	const Sum *tb = tile + ty * pitch, *tg = tile + (kScaleTileH + ty) * pitch, *tr = tile + (2 * kScaleTileH + ty) * pitch;
	for (int t = 0; t < count; ++t) {
		const Wide w = qx[t];
		const int col = ldsColumn(first + t);
		b += w * tb[col];
		g += w * tg[col];
		r += w * tr[col];
	}
	const unsigned lo = scaleResult<kSigned, 65535>(b) | (scaleResult<kSigned, 65535>(g) << 16);
	*reinterpret_cast<uint2 *>(dst + (static_cast<std::size_t>(dy) * dstW + dx) * 4) = make_uint2(lo, scaleResult<kSigned, 65535>(r));
}

}  // namespace

}  // namespace ju
