// The alpha channel on gfx950 (docs/alpha.md): the alpha slot of a four-sample frame -- byte 3 of BGRX / RGBX, word 3 of
// BGRX64, the two top bits of X2RGB10 / X2BGR10 -- scaled from the input frame's size straight to the output frame's size
// by the project's integer scaler, or filled with the format's top code.
//
// The kernels compute exactly the numpy definition of tests/alpha_reference.py: the 16-bit plane A of the input (257 a
// of a byte, the word itself, 21845 a of a two-bit code, 65535 where the format has no slot), A' = (sum qy qx A + 2^23)
// >> 24 with buildScaleAxis's tables (clamped to 0 .. 65535 by the cubic filters' form), and the slot's code of A'
// ((A' + 128) / 257, A', (A' + 10922) / 21845).
//
//   alpha_scale_kernel<kSigned, Src, Sink>  scale_tile.h's tile for ONE channel of 16-bit samples: a workgroup of 256
//                       threads per kScaleTileW x kScaleTileH destination pixels.  Vertical pass: item = (tile row, four
//                       source columns), sum qy * A (<= 65535 * 4096 < 2^28; the signed form 65535 * 6144 < 2^29 in size:
//                       one 32-bit word) into LDS as [kScaleTileH][pitch], column c at c + c / 32 -- a third of
//                       scale_state_kernel's LDS at the same ratio.  Horizontal pass: a thread per destination pixel, a
//                       64-bit sum (< 2^40; signed 2^42 in size), scaleResult<kSigned, 65535>, one store through the sink.
//   alpha_fill_kernel<Sink>  a thread per destination pixel stores the top code through the sink; no tables, no LDS.
//
// Src: what a lane reads for four columns of the current row -- AlphaBytes (byte 3 of four-byte pixels, any byte
// alignment and signed stride: one 16-byte load where every row is 16-byte aligned, as ScaleRows8, else a byte per pixel
// with the column clamped to the row), AlphaWords (word 3 of eight-byte pixels, 2-byte aligned: two 16-byte loads where
// the rows are 16-byte aligned, else a word per pixel), AlphaBits (the top two bits of 32-bit words, 4-byte aligned) and
// AlphaOpaque (65535: an input without a slot; nothing is read).
//
// Sink: where a lane's one result goes -- AlphaByteSink, AlphaWordSink, AlphaBitsSink.  No other bit of the destination
// changes.  The byte sink is a BYTE STORE, not a read-modify-write of the aligned word: a pixel at an odd byte address
// shares its aligned words with its neighbours, whose lanes would rewrite each other's colour bytes; the byte store is
// right at every alignment and reads nothing (what it costs: docs/alpha.md "Measurements").  The word sink is one 16-bit
// store.  The two-bit sink must keep the 30 colour bits of a word
// only its own lane touches (the words are 4-byte aligned), so it is a read-modify-write of that word.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): docs/alpha.md holds the table; no
// instantiation uses scratch.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"
#include "kernels.h"
#include "scale_tile.h"

namespace ju {

std::string alphaProblem(int mode, int filter, std::size_t inW, std::size_t inH, std::size_t outW, std::size_t outH) {
	if (mode != kAlphaZero && mode != kAlphaOpaque && mode != kAlphaSource) {
		return "unknown alpha mode " + std::to_string(mode) +
		       " (the modes are JU_ALPHA_ZERO = 0, JU_ALPHA_OPAQUE = 1 and JU_ALPHA_SOURCE = 2)";
	}
	const std::string unknown = scaleFilterProblem(filter);
	if (!unknown.empty()) return unknown;
	if (mode != kAlphaSource) return "";  // (the sizes count where alpha is scaled)
	const std::size_t down = static_cast<std::size_t>(scaleDownMax(filter));
	auto axisOk = [down](std::size_t n, std::size_t m) {
		const auto lo = static_cast<std::size_t>(kOutputAxisMin), hi = static_cast<std::size_t>(kOutputAxisMax);
		return n >= lo && n <= hi && m >= lo && m <= hi && n <= down * m && m <= kSourceRatioMax * n;
	};
	if (axisOk(inW, outW) && axisOk(inH, outH)) return "";
	return "alpha from the source: the input frame " + std::to_string(inW) + "x" + std::to_string(inH) + " and the output frame " +
	       std::to_string(outW) + "x" + std::to_string(outH) + " must be " + std::to_string(kOutputAxisMin) + " .. " +
	       std::to_string(kOutputAxisMax) + " on each axis, the input at most " + std::to_string(down) +
	       " times the output and the output at most " + std::to_string(kSourceRatioMax) +
	       " times the input (the alpha scaler goes from one straight to the other)";
}

namespace {

// ---- sources: four 16-bit samples A of columns x .. x + 3 (x = 0 mod 4) of the current row ----------------------------
struct AlphaQuad {
	unsigned a[4];
};

struct AlphaBytes {
	const std::uint8_t *src;
	std::ptrdiff_t stride;
	int width;
	std::uintptr_t low;  // the low bits of address and stride: 0 where every row is 16-byte aligned
	using Column = const std::uint8_t *;  // the current row
	__device__ __forceinline__ AlphaBytes(const std::uint8_t *p, std::ptrdiff_t s, int w)
	    : src(p), stride(s), width(w), low((reinterpret_cast<std::uintptr_t>(p) | static_cast<std::uintptr_t>(s)) & 15) {}
	__device__ __forceinline__ Column column(int row) const { return src + static_cast<std::ptrdiff_t>(row) * stride; }
	__device__ __forceinline__ Column next(Column row) const { return row + stride; }
	__device__ __forceinline__ AlphaQuad load(Column row, int x) const {
		AlphaQuad q;
		if (low == 0 && x + 4 <= width) {
			const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * x);
			q.a[0] = v.x >> 24, q.a[1] = v.y >> 24, q.a[2] = v.z >> 24, q.a[3] = v.w >> 24;
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) q.a[k] = row[4 * min(x + k, width - 1) + 3];  // (past the row: never a tap)
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) q.a[k] *= 257u;
		return q;
	}
};

struct AlphaWords {
	const std::uint8_t *src;
	std::ptrdiff_t stride;
	int width;
	std::uintptr_t low;
	using Column = const std::uint8_t *;
	__device__ __forceinline__ AlphaWords(const std::uint8_t *p, std::ptrdiff_t s, int w)
	    : src(p), stride(s), width(w), low((reinterpret_cast<std::uintptr_t>(p) | static_cast<std::uintptr_t>(s)) & 15) {}
	__device__ __forceinline__ Column column(int row) const { return src + static_cast<std::ptrdiff_t>(row) * stride; }
	__device__ __forceinline__ Column next(Column row) const { return row + stride; }
	__device__ __forceinline__ AlphaQuad load(Column row, int x) const {
		AlphaQuad q;
		if (low == 0 && x + 4 <= width) {
			const uint4 *at = reinterpret_cast<const uint4 *>(row + 8 * x);
			const uint4 v0 = at[0], v1 = at[1];
			q.a[0] = v0.y >> 16, q.a[1] = v0.w >> 16, q.a[2] = v1.y >> 16, q.a[3] = v1.w >> 16;
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) q.a[k] = *reinterpret_cast<const std::uint16_t *>(row + 8 * min(x + k, width - 1) + 6);
		}
		return q;
	}
};

struct AlphaBits {
	const std::uint8_t *src;
	std::ptrdiff_t stride;
	int width;
	std::uintptr_t low;
	using Column = const std::uint8_t *;
	__device__ __forceinline__ AlphaBits(const std::uint8_t *p, std::ptrdiff_t s, int w)
	    : src(p), stride(s), width(w), low((reinterpret_cast<std::uintptr_t>(p) | static_cast<std::uintptr_t>(s)) & 15) {}
	__device__ __forceinline__ Column column(int row) const { return src + static_cast<std::ptrdiff_t>(row) * stride; }
	__device__ __forceinline__ Column next(Column row) const { return row + stride; }
	__device__ __forceinline__ AlphaQuad load(Column row, int x) const {
		AlphaQuad q;
		if (low == 0 && x + 4 <= width) {
			const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * x);
			q.a[0] = v.x >> 30, q.a[1] = v.y >> 30, q.a[2] = v.z >> 30, q.a[3] = v.w >> 30;
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) q.a[k] = *reinterpret_cast<const unsigned *>(row + 4 * min(x + k, width - 1)) >> 30;
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) q.a[k] *= 21845u;
		return q;
	}
};

struct AlphaOpaque {  // an input without a slot: 65535 everywhere, nothing read
	using Column = int;
	__device__ __forceinline__ AlphaOpaque(const std::uint8_t *, std::ptrdiff_t, int) {}
	__device__ __forceinline__ Column column(int) const { return 0; }
	__device__ __forceinline__ Column next(Column) const { return 0; }
	__device__ __forceinline__ AlphaQuad load(Column, int) const { return AlphaQuad{{65535u, 65535u, 65535u, 65535u}}; }
};

// ---- sinks: the slot of pixel (x, y) takes the code of the 16-bit sample a ---------------------------------------------
struct AlphaByteSink {
	__device__ static __forceinline__ void store(std::uint8_t *dst, std::ptrdiff_t stride, int x, int y, unsigned a) {
		dst[static_cast<std::ptrdiff_t>(y) * stride + 4 * x + 3] = static_cast<std::uint8_t>((a + 128u) / 257u);
	}
};
struct AlphaWordSink {
	__device__ static __forceinline__ void store(std::uint8_t *dst, std::ptrdiff_t stride, int x, int y, unsigned a) {
		*reinterpret_cast<std::uint16_t *>(dst + static_cast<std::ptrdiff_t>(y) * stride + 8 * x + 6) = static_cast<std::uint16_t>(a);
	}
};
struct AlphaBitsSink {
	__device__ static __forceinline__ void store(std::uint8_t *dst, std::ptrdiff_t stride, int x, int y, unsigned a) {
		unsigned *p = reinterpret_cast<unsigned *>(dst + static_cast<std::ptrdiff_t>(y) * stride + 4 * x);
		*p = (*p & 0x3fffffffu) | (((a + 10922u) / 21845u) << 30);
	}
};

template <bool kSigned, typename Src, typename Sink>
__global__ __launch_bounds__(256) void alpha_scale_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride, int srcW,
    std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW, int dstH, ScaleTaps ax, ScaleTaps ay, int pitch) {
	using Tap = typename ScaleForm<kSigned>::Tap;
	using Sum = typename ScaleForm<kSigned>::Sum;
	using Wide = typename ScaleForm<kSigned>::Sum16;
	extern __shared__ unsigned tileWords[];  // [kScaleTileH][pitch]: sum qy * A, below 2^28 (signed: 2^29 in size)
	Sum *tile = reinterpret_cast<Sum *>(tileWords);
	const int tid = threadIdx.x;
	const int dx0 = blockIdx.x * kScaleTileW, dy0 = blockIdx.y * kScaleTileH;
	const int dxLast = min(dx0 + kScaleTileW, dstW) - 1;
	const int xs0 = tileFirst<kSigned>(ax.start[dx0]) & ~3;
	const int xs1 = tileEnd<kSigned>(ax.start[dxLast] + ax.taps[dxLast * kScaleTapPitch + kScaleMaxTaps], srcW);
	const int quads = (xs1 - xs0 + 3) >> 2;
	const Src source(src, srcStride, srcW);

	// vertical pass: item = (tile row, four source columns)
	for (int item = tid; item < kScaleTileH * quads; item += 256) {
		const int r = item / quads, q = item - r * quads;
		const int dy = dy0 + r;
		if (dy >= dstH) continue;
		const int x = xs0 + 4 * q;
		const Tap *qy = reinterpret_cast<const Tap *>(ay.taps) + dy * kScaleTapPitch;
		const int count = qy[kScaleMaxTaps];
		typename Src::Column column = source.column(ay.start[dy]);
		Sum acc[4] = {0, 0, 0, 0};
		for (int t = 0; t < count; ++t, column = source.next(column)) {
			const Sum w = qy[t];
			const AlphaQuad v = source.load(column, x);
#pragma unroll
			for (int k = 0; k < 4; ++k) acc[k] += w * static_cast<Sum>(v.a[k]);
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) tile[r * pitch + ldsColumn(4 * q + k)] = acc[k];
	}
	__syncthreads();

	// horizontal pass: a thread per destination pixel
	const int tx = tid & (kScaleTileW - 1), ty = tid / kScaleTileW;
	const int dx = dx0 + tx, dy = dy0 + ty;
	if (dx >= dstW || dy >= dstH) return;
	const Tap *qx = reinterpret_cast<const Tap *>(ax.taps) + dx * kScaleTapPitch;
	const int count = qx[kScaleMaxTaps];
	const int first = ax.start[dx] - xs0;
	Wide sum = 1u << 23;
	const Sum *row = tile + ty * pitch;
	for (int t = 0; t < count; ++t) {
		const Wide w = qx[t];
		sum += w * row[ldsColumn(first + t)];
	}
	Sink::store(dst, dstStride, dx, dy, scaleResult<kSigned, 65535>(sum));
}

template <typename Sink>
__global__ __launch_bounds__(256) void alpha_fill_kernel(std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW, int dstH) {
	const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= dstW || y >= dstH) return;
	Sink::store(dst, dstStride, x, y, 65535u);
}

// the rows a side covers: pixel bytes and the alignment its address and stride must have
struct AlphaLayout {
	int pixelBytes, align;
};
AlphaLayout sinkLayout(int kind) {
	switch (kind) {
	case kAlphaByte: return {4, 1};
	case kAlphaWord: return {8, 2};
	case kAlphaBits: return {4, 4};
	default: throw std::invalid_argument("alpha: unknown sink kind " + std::to_string(kind) + " (0 byte 3, 1 word 3, 2 bits 30-31)");
	}
}

void checkRows(const char *who, const char *side, const void *ptr, std::ptrdiff_t stride, int width, AlphaLayout l) {
	const auto row = static_cast<std::ptrdiff_t>(width) * l.pixelBytes;
	if (ptr == nullptr) throw std::invalid_argument(std::string(who) + ": NULL " + side);
	if (stride > -row && stride < row) throw std::invalid_argument(std::string(who) + ": " + side + ": |stride| smaller than a row");
	if (reinterpret_cast<std::uintptr_t>(ptr) % static_cast<unsigned>(l.align) != 0 || stride % l.align != 0) {
		throw std::invalid_argument(std::string(who) + ": " + side + ": the address and the stride must be multiples of " +
		                            std::to_string(l.align));
	}
}

template <bool kSigned, typename Src>
auto scaleKernelOf(int sinkKind) {
	switch (sinkKind) {
	case kAlphaByte: return alpha_scale_kernel<kSigned, Src, AlphaByteSink>;
	case kAlphaWord: return alpha_scale_kernel<kSigned, Src, AlphaWordSink>;
	default: return alpha_scale_kernel<kSigned, Src, AlphaBitsSink>;
	}
}

template <bool kSigned>
auto scaleKernelOf(int srcKind, int sinkKind) {
	switch (srcKind) {
	case kAlphaByte: return scaleKernelOf<kSigned, AlphaBytes>(sinkKind);
	case kAlphaWord: return scaleKernelOf<kSigned, AlphaWords>(sinkKind);
	case kAlphaBits: return scaleKernelOf<kSigned, AlphaBits>(sinkKind);
	default: return scaleKernelOf<kSigned, AlphaOpaque>(sinkKind);
	}
}

}  // namespace

void launchAlphaScale(const AlphaRows &src, int srcW, int srcH, const AlphaRows &dst, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream) {
	const char *who = "launchAlphaScale";
	if (srcW < 1 || srcH < 1 || dstW < 1 || dstH < 1 || spanX < 4 || spanX % 4 || x.start == nullptr || x.taps == nullptr ||
	    y.start == nullptr || y.taps == nullptr) {
		throw std::invalid_argument("launchAlphaScale: bad arguments");
	}
	if (src.kind != kAlphaNone) {
		if (src.kind != kAlphaByte && src.kind != kAlphaWord && src.kind != kAlphaBits) {
			throw std::invalid_argument("alpha: unknown source kind " + std::to_string(src.kind) +
			                            " (0 byte 3, 1 word 3, 2 bits 30-31, 3 none: opaque)");
		}
		checkRows(who, "source", src.ptr, src.stride, srcW, sinkLayout(src.kind));
	}
	checkRows(who, "destination", dst.ptr, dst.stride, dstW, sinkLayout(dst.kind));
	const int pitch = spanX + spanX / 32 + 1;
	const std::size_t lds = static_cast<std::size_t>(kScaleTileH) * static_cast<std::size_t>(pitch) * sizeof(unsigned);
	if (lds > 64 * 1024) throw std::invalid_argument("launchAlphaScale: the tile does not fit the LDS");
	if (x.filter != y.filter) throw std::invalid_argument("launchAlphaScale: the two axes' tables must be of one filter");
	const dim3 grid(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW),
	    static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH));
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	const auto kernel = x.filter != kScaleTriangle ? scaleKernelOf<true>(src.kind, dst.kind) : scaleKernelOf<false>(src.kind, dst.kind);
	hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, static_cast<const std::uint8_t *>(src.ptr), src.stride, srcW,
	    static_cast<std::uint8_t *>(dst.ptr), dst.stride, dstW, dstH, tx, ty, pitch);
	hipCheckLaunch("alpha_scale");
}

void launchAlphaFill(const AlphaRows &dst, int dstW, int dstH, hipStream_t stream) {
	if (dstW < 1 || dstH < 1) throw std::invalid_argument("launchAlphaFill: bad arguments");
	checkRows("launchAlphaFill", "destination", dst.ptr, dst.stride, dstW, sinkLayout(dst.kind));
	const dim3 grid(static_cast<unsigned>((dstW + 63) / 64), static_cast<unsigned>((dstH + 3) / 4));
	auto *p = static_cast<std::uint8_t *>(dst.ptr);
	switch (dst.kind) {
	case kAlphaByte: hipLaunchKernelGGL(alpha_fill_kernel<AlphaByteSink>, grid, dim3(64, 4), 0, stream, p, dst.stride, dstW, dstH); break;
	case kAlphaWord: hipLaunchKernelGGL(alpha_fill_kernel<AlphaWordSink>, grid, dim3(64, 4), 0, stream, p, dst.stride, dstW, dstH); break;
	default: hipLaunchKernelGGL(alpha_fill_kernel<AlphaBitsSink>, grid, dim3(64, 4), 0, stream, p, dst.stride, dstW, dstH); break;
	}
	hipCheckLaunch("alpha_fill");
}

}  // namespace ju
