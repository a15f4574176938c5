// The source stage on gfx950 (docs/source_stage.md): a BGRX source of any size scaled to the model's input by an
// integer filter -- the triangle, or one of two cubic filters (Catmull-Rom, Mitchell-Netravali) -- and the source drawn
// back over the upscaled frame through a mask.
//
// The kernels compute exactly the numpy definitions of tests/source_reference.py and tests/scale_filter_reference.py.
// The host builds the per-axis tables (buildScaleAxis: start index, tap count and 16-bit taps summing to 4096 per
// destination index); the device only multiplies and adds integers.  The triangle's form (<false>), unsigned:
//
//   scale_bgrx_kernel   one workgroup per tile of kScaleTileW x kScaleTileH destination pixels.  Vertical pass: every
//                       source column the tile needs, for each of the tile's rows, sum qy * src (<= 255 * 4096 < 2^20,
//                       exact) into LDS -- a thread takes four source columns, 16 bytes per load where the source rows
//                       are 16-byte aligned, so a wave reads contiguous row segments.  Horizontal pass: a thread per
//                       destination pixel, sum qx * LDS + 2^23 >> 24 (< 2^32).  Lanes of a half-wave read LDS columns
//                       N / M apart (ds_read_b32: banks (a / 4) % 32 per 32-lane half), which is a 4-way conflict at
//                       1920 -> 480; the tile stores column c at c + c / 32, which puts the 32 lanes of every power-
//                       of-two ratio up to 16 on 32 different banks (and the vertical pass's four-column writes too).
//   scale_bgrx_items_kernel  the same tile (scaleBgrxTile, the one body of both) over the sources of a look-ahead pass:
//                       grid.z = item, each with its own pointers and strides from a by-value table.
//   scale_bgrx_members_kernel  the same tile over the sources of a group pass: grid.z = member, each with its own source
//                       size, tables, LDS pitch and form from a by-value table; one destination size for all.
//   mask_blend_kernel   a thread per output pixel; mask and source are point sampled.
//   scale_state_kernel  the output stage's 16-bit path (docs/output_stage.md): scale_bgrx_kernel's tile over the dense f16
//                       state, each sample first P = floor((s + 0.5) * 65536) saturated (StateSource::sample of
//                       colour_kernels.hip).  Vertical sums reach 65535 * 4096 < 2^28 (32 bits in LDS), the horizontal
//                       sum 2^40: a 64-bit accumulator.  Two source pixels per 16-byte load, one 8-byte store per pixel.
//
// The cubic filters' form (<true>) of both scale kernels is the same code on signed types (ScaleForm): taps read as i16,
// rows of sum |q| <= 6144, so a vertical sum is below 2^21 (2^29 for the state) in size and still one signed LDS word
// under the same tile, padding and loads; the horizontal sum is 64 bits signed (2^34 / 2^42 in size), shifted with its
// sign and clamped to 0 .. 255 / 65535.  The triangle's instantiations are, instruction for instruction, the kernels
// from before the template (docs/source_stage.md "Filters").
//
// The tile itself -- both passes, the two forms, the LDS layout -- is scale_tile.h, with the source of the vertical pass
// as a template parameter: the kernels here read rows in memory (ScaleRows8, ScaleState16); the tiled object's fused
// kernels (tile_kernels.hip) run the same tile over the blend of its tiles.
//
// Resources (tools/kernel_resources.py): scale_bgrx_kernel and scale_bgrx_items_kernel hold 52 VGPRs in either form and no
// scratch; scale_bgrx_members_kernel, which carries both forms behind a uniform branch, 52 VGPRs and no scratch too.
//
// Rows are addressed with their signed stride; pixels off 4-byte alignment move byte by byte.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernel_common.h"
#include "kernels.h"
#include "scale_tile.h"

namespace ju {

std::string scaleFilterProblem(int filter) {
	if (scaleFilterKnown(filter)) return "";
	return "unknown filter " + std::to_string(filter) +
	       " (the filters are JU_SCALE_TRIANGLE = 0, JU_SCALE_CATMULL_ROM = 2 and JU_SCALE_MITCHELL = 3)";
}

namespace {

// The raw weight of a cubic filter at distance u / D, u >= 0: the kernel times 2 D^3 (Catmull-Rom, a = -0.5) or 18 D^3
// (Mitchell-Netravali, B = C = 1/3), 0 from 2 D on.  D <= 32768: every term stays below 2^53.
long long cubicWeight(int filter, long long u, long long D) {
	if (u >= 2 * D) return 0;
	if (filter == kScaleCatmullRom) {
		return u < D ? 3 * u * u * u - 5 * u * u * D + 2 * D * D * D : -u * u * u + 5 * u * u * D - 8 * u * D * D + 4 * D * D * D;
	}
	return u < D ? 21 * u * u * u - 36 * u * u * D + 16 * D * D * D
	             : -7 * u * u * u + 36 * u * u * D - 60 * u * D * D + 32 * D * D * D;
}

// One axis of a cubic filter (tests/scale_filter_reference.py axis_table): the run of source indices with u < 2 D, zero
// weights trimmed at both ends; q = floor(4096 w / S) toward minus infinity; the remainder to the first largest w.
ScaleAxisHost buildCubicAxis(int n, int m, int filter) {
	ScaleAxisHost a;
	a.n = n;
	a.m = m;
	a.filter = filter;
	a.start.assign(static_cast<std::size_t>(m), 0);
	a.taps.assign(static_cast<std::size_t>(m) * kScaleTapPitch, 0);
	const long long N = n, M = m, D = 2 * std::max(N, M);
	if (D > 32768) throw std::logic_error("buildScaleAxis: an axis beyond 16384 samples");
	long long firstMost = 0, endMost = 0;
	for (long long d = 0; d < M; ++d) {
		const long long c = (2 * d + 1) * N;
		const auto weight = [&](long long s) {
			const long long t = (2 * s + 1) * M - c;
			return cubicWeight(filter, t < 0 ? -t : t, D);
		};
		// from a little before the support to a little behind it, then trimmed to the first and the last weight that is not 0
		long long s0 = std::max((c - 2 * D) / (2 * M) - 1, 0LL), s1 = std::min((c + 2 * D) / (2 * M) + 2, N);
		while (s0 < s1 && weight(s0) == 0) ++s0;
		while (s1 > s0 && weight(s1 - 1) == 0) --s1;
		if (s1 == s0) throw std::logic_error("buildScaleAxis: a destination index without taps");
		if (s1 - s0 > kScaleMaxTaps) throw std::logic_error("buildScaleAxis: more than 33 taps");
		const int count = static_cast<int>(s1 - s0);
		long long w[kScaleMaxTaps];
		long long sum = 0;
		int best = 0;
		for (int i = 0; i < count; ++i) {
			w[i] = weight(s0 + i);
			sum += w[i];
			if (w[i] > w[best]) best = i;  // (the first of the largest)
		}
		if (sum <= 0) throw std::logic_error("buildScaleAxis: a row whose weights do not sum above 0");
		long long q[kScaleMaxTaps];
		long long total = 0, absSum = 0;
		for (int i = 0; i < count; ++i) {
			const long long num = w[i] * 4096;  // (|w| <= 32 D^3 <= 2^50)
			q[i] = num / sum - (num % sum < 0 ? 1 : 0);
			total += q[i];
		}
		q[best] += 4096 - total;
		for (int i = 0; i < count; ++i) absSum += q[i] < 0 ? -q[i] : q[i];
		if (absSum > kScaleAbsSumMax) throw std::logic_error("buildScaleAxis: a row with sum |q| above 6144");
		std::uint16_t *out = a.taps.data() + static_cast<std::size_t>(d) * kScaleTapPitch;
		for (int i = 0; i < count; ++i) out[i] = static_cast<std::uint16_t>(static_cast<std::int16_t>(q[i]));
		out[kScaleMaxTaps] = static_cast<std::uint16_t>(count);
		a.start[static_cast<std::size_t>(d)] = static_cast<int>(s0);
		// what the kernels' tile span rests on (tileFirst / tileEnd): no earlier row starts or ends more than one index later
		firstMost = std::max(firstMost, s0);
		endMost = std::max(endMost, s1);
		if (s0 < firstMost - 1 || s1 < endMost - 1) throw std::logic_error("buildScaleAxis: rows more than one index out of order");
	}
	return a;
}

}  // namespace

ScaleAxisHost buildScaleAxis(int n, int m, int filter) {
	const std::string unknown = scaleFilterProblem(filter);
	if (!unknown.empty()) throw std::invalid_argument("buildScaleAxis: " + unknown);
	if (n < 1 || m < 1 || n > scaleDownMax(filter) * static_cast<long long>(m) || m > kSourceRatioMax * static_cast<long long>(n)) {
		throw std::invalid_argument("buildScaleAxis: " + std::to_string(n) + " -> " + std::to_string(m) +
		                            " is beyond a factor of " + std::to_string(n > m ? scaleDownMax(filter) : kSourceRatioMax));
	}
	if (filter != kScaleTriangle) return buildCubicAxis(n, m, filter);
	ScaleAxisHost a;
	a.n = n;
	a.m = m;
	a.start.assign(static_cast<std::size_t>(m), 0);
	a.taps.assign(static_cast<std::size_t>(m) * kScaleTapPitch, 0);
	const long long N = n, M = m, D = 2 * std::max(N, M);
	for (long long d = 0; d < M; ++d) {
		const long long c = (2 * d + 1) * N;
		// the first source index with a positive weight: (2 s + 1) M > c - D
		long long s0 = (c - D) / (2 * M) - 1;
		s0 = std::max(s0, 0LL);
		while (s0 < N && (2 * s0 + 1) * M - c <= -D) ++s0;
		long long w[kScaleMaxTaps];
		int count = 0;
		long long sum = 0;
		for (long long s = s0; s < N; ++s) {
			const long long t = (2 * s + 1) * M - c;
			const long long v = D - (t < 0 ? -t : t);
			if (v <= 0) break;
			if (count == kScaleMaxTaps) throw std::logic_error("buildScaleAxis: more than 33 taps");
			w[count++] = v;
			sum += v;
		}
		if (count == 0) throw std::logic_error("buildScaleAxis: a destination index without taps");
		std::uint16_t *q = a.taps.data() + static_cast<std::size_t>(d) * kScaleTapPitch;
		long long total = 0;
		int best = 0;
		for (int i = 0; i < count; ++i) {
			q[i] = static_cast<std::uint16_t>(w[i] * 4096 / sum);
			total += q[i];
			if (w[i] > w[best]) best = i;  // (the first of the largest)
		}
		q[best] = static_cast<std::uint16_t>(q[best] + (4096 - total));
		q[kScaleMaxTaps] = static_cast<std::uint16_t>(count);
		a.start[static_cast<std::size_t>(d)] = static_cast<int>(s0);
	}
	return a;
}

namespace {
// "within a factor of 16 of" for the triangle; a cubic filter reduces by 8 at the most: "at most 8 times" the model's
// input for a source, "at least an 8th of" the model's output for an output size
std::string ratioWords(int filter, bool sourceSide) {
	if (filter == kScaleTriangle) return " and within a factor of " + std::to_string(kSourceRatioMax) + " of";
	const std::string up = std::to_string(kSourceRatioMax), down = std::to_string(kCubicDownMax);
	return sourceSide ? ", at most " + down + " times and at least a " + up + "th of"
	                  : ", at most " + up + " times and at least an " + down + "th of";
}
}  // namespace

std::string sourceSizeProblem(std::size_t srcW, std::size_t srcH, std::size_t inW, std::size_t inH, int filter) {
	const std::string unknown = scaleFilterProblem(filter);
	if (!unknown.empty()) return unknown;
	const std::size_t down = static_cast<std::size_t>(scaleDownMax(filter));
	auto axisOk = [down](std::size_t n, std::size_t m) {
		return n >= static_cast<std::size_t>(kSourceAxisMin) && n <= static_cast<std::size_t>(kSourceAxisMax) &&
		       n <= down * m && m <= kSourceRatioMax * n;
	};
	if (axisOk(srcW, inW) && axisOk(srcH, inH)) return "";
	return "source size " + std::to_string(srcW) + "x" + std::to_string(srcH) + ": each axis must be " +
	       std::to_string(kSourceAxisMin) + " .. " + std::to_string(kSourceAxisMax) + ratioWords(filter, true) +
	       " the model's input " + std::to_string(inW) + "x" + std::to_string(inH);
}

std::string outputSizeProblem(std::size_t outW, std::size_t outH, std::size_t modelW, std::size_t modelH, int filter) {
	const std::string unknown = scaleFilterProblem(filter);
	if (!unknown.empty()) return unknown;
	const std::size_t down = static_cast<std::size_t>(scaleDownMax(filter));
	auto axisOk = [down](std::size_t m, std::size_t n) {
		return m >= static_cast<std::size_t>(kOutputAxisMin) && m <= static_cast<std::size_t>(kOutputAxisMax) &&
		       n <= down * m && m <= kSourceRatioMax * n;
	};
	if (axisOk(outW, modelW) && axisOk(outH, modelH)) return "";
	return "output size " + std::to_string(outW) + "x" + std::to_string(outH) + ": each axis must be " +
	       std::to_string(kOutputAxisMin) + " .. " + std::to_string(kOutputAxisMax) + ratioWords(filter, false) +
	       " the model's output " + std::to_string(modelW) + "x" + std::to_string(modelH);
}

int scaleSpan(const ScaleAxisHost &x) {
	int span = 4;
	for (int d0 = 0; d0 < x.m; d0 += kScaleTileW) {
		const int d1 = std::min(d0 + kScaleTileW, x.m) - 1;
		int first = x.start[static_cast<std::size_t>(d0)];
		int end = x.start[static_cast<std::size_t>(d1)] + x.taps[static_cast<std::size_t>(d1) * kScaleTapPitch + kScaleMaxTaps];
		if (x.filter != kScaleTriangle) first = tileFirst<true>(first), end = tileEnd<true>(end, x.n);  // (as the signed kernels)
		first &= ~3;
		span = std::max(span, (end - first + 3) / 4 * 4);
	}
	return span;
}

namespace {

// One tile of scale_bgrx_kernel (the head of the file; scale_tile.h holds the body) over BGRX rows in memory.  THE body of
// all three launch forms -- the single frame, the items of a look-ahead pass, the members of a group pass -- so their
// bytes are equal by construction.
template <bool kSigned>
__device__ __forceinline__ void scaleBgrxTile(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride, int srcW,
    std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW, int dstH, ScaleTaps ax, ScaleTaps ay, int pitch) {
	scaleTile8<kSigned, ScaleRows8>({src, srcStride, srcW}, srcW, dst, dstStride, dstW, dstH, ax, ay, pitch);
}

template <bool kSigned>
__global__ __launch_bounds__(256) void scale_bgrx_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    int srcW, std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW, int dstH, ScaleTaps ax,
    ScaleTaps ay, int pitch) {
	scaleBgrxTile<kSigned>(src, srcStride, srcW, dst, dstStride, dstW, dstH, ax, ay, pitch);
}

// The sources of a look-ahead pass in one launch (Engine::runBatch; docs/source_stage.md "Passes"): grid (tiles x, tiles
// y, item), item blockIdx.z of the by-value table with its own pointers and strides -- a workgroup reads its item's four
// words from the kernel arguments with scalar loads, uniform over the workgroup.  Sizes, taps and pitch are the launch's;
// the 16-byte path is decided per item inside the tile, from the item's own address and stride.
template <bool kSigned>
__global__ __launch_bounds__(256) void scale_bgrx_items_kernel(ScaleItems items, int srcW, int dstW, int dstH, ScaleTaps ax,
    ScaleTaps ay, int pitch) {
	const ScaleItem &it = items.item[blockIdx.z];
	scaleBgrxTile<kSigned>(it.src, it.srcStride, srcW, it.dst, it.dstStride, dstW, dstH, ax, ay, pitch);
}

// The sources of a group pass in one launch (Engine::runGroupPass; docs/source_stage.md "Group passes"): grid (tiles x,
// tiles y, member).  The destination is the model's input for every member, so the tile grid is common; everything else
// is the member's own, read from the by-value table through blockIdx.z with scalar loads.  The form is a branch on the
// member's flag, uniform over the workgroup; either side is scaleBgrxTile, so the bytes are those of scale_bgrx_kernel.
// The launch's dynamic LDS is the largest member's tile; a member addresses its own rows by its own pitch.
__global__ __launch_bounds__(256) void scale_bgrx_members_kernel(ScaleMembers members, int dstW, int dstH) {
	const ScaleMember &m = members.member[blockIdx.z];
	const ScaleTaps ax{m.xStart, m.xTaps}, ay{m.yStart, m.yTaps};
	if (m.cubic) {
		scaleBgrxTile<true>(m.src, m.srcStride, m.srcW, m.dst, m.dstStride, dstW, dstH, ax, ay, m.pitch);
	} else {
		scaleBgrxTile<false>(m.src, m.srcStride, m.srcW, m.dst, m.dstStride, dstW, dstH, ax, ay, m.pitch);
	}
}

// The dense f16 state [srcH][srcW][4] (B, G, R, unused) -> the dense u16 frame [dstH][dstW][4] (B, G, R, 0):
// out = (sum qy qx P + 2^23) >> 24.  The tile, the tables and the LDS layout of scale_bgrx_kernel (scaleTile16 of
// scale_tile.h); an item of the vertical pass is (tile row, two source columns): 16 bytes per tap where that pair is
// 16-byte aligned (every pair of an even width, every other row of an odd one), else two 8-byte loads, the column clamped
// to the row.
template <bool kSigned>
__global__ __launch_bounds__(256) void scale_state_kernel(const f16 *__restrict__ src, int srcW,
    std::uint16_t *__restrict__ dst, int dstW, int dstH, ScaleTaps ax, ScaleTaps ay, int pitch) {
	scaleTile16<kSigned, ScaleState16>({src, srcW}, srcW, dst, dstW, dstH, ax, ay, pitch);
}

__global__ __launch_bounds__(256) void mask_blend_kernel(std::uint8_t *__restrict__ gen, std::ptrdiff_t genStride,
    unsigned outW, unsigned outH, const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride, unsigned srcW,
    unsigned srcH, const std::uint8_t *__restrict__ mask, std::ptrdiff_t maskStride, unsigned maskW, unsigned maskH) {
	const unsigned x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
	if (x >= outW || y >= outH) return;
	// texel of a W-wide texture under the centre of pixel x: floor((2 x + 1) W / (2 outW)), below 2^32 (launchMaskBlend)
	const unsigned mx = (2 * x + 1) * maskW / (2 * outW), my = (2 * y + 1) * maskH / (2 * outH);
	const unsigned m = loadPixel(mask + static_cast<std::ptrdiff_t>(my) * maskStride + 4 * mx);
	const unsigned a = 765 - ((m & 255) + ((m >> 8) & 255) + ((m >> 16) & 255));
	if (a == 0) return;
	const unsigned sx = (2 * x + 1) * srcW / (2 * outW), sy = (2 * y + 1) * srcH / (2 * outH);
	const unsigned s = loadPixel(src + static_cast<std::ptrdiff_t>(sy) * srcStride + 4 * sx);
	std::uint8_t *p = gen + static_cast<std::ptrdiff_t>(y) * genStride + 4 * x;
	const unsigned g = loadPixel(p);
	unsigned out = 0;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const unsigned sc = (s >> (8 * c)) & 255, gc = (g >> (8 * c)) & 255;
		out |= ((sc * a + gc * (765 - a) + 382) / 765) << (8 * c);
	}
	storePixel(p, out);
}

}  // namespace

void launchScaleBgrx(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, int srcH, std::uint8_t *dst,
    std::ptrdiff_t dstStride, int dstW, int dstH, const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX,
    hipStream_t stream) {
	if (src == nullptr || dst == nullptr || srcW < 1 || srcH < 1 || dstW < 1 || dstH < 1 || spanX < 4 || spanX % 4) {
		throw std::invalid_argument("launchScaleBgrx: bad arguments");
	}
	const int pitch = spanX + spanX / 32 + 1;
	const std::size_t lds = static_cast<std::size_t>(3) * kScaleTileH * static_cast<std::size_t>(pitch) * sizeof(unsigned);
	if (lds > 64 * 1024) throw std::invalid_argument("launchScaleBgrx: the tile does not fit the LDS");
	const dim3 grid(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW),
	    static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH));
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	if (x.filter != y.filter) throw std::invalid_argument("launchScaleBgrx: the two axes' tables must be of one filter");
	const auto kernel = x.filter != kScaleTriangle ? scale_bgrx_kernel<true> : scale_bgrx_kernel<false>;  // (spanX is of that form too)
	hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, src, srcStride, srcW, dst, dstStride, dstW, dstH, tx, ty, pitch);
	hipCheckLaunch("scale_bgrx");
}

void launchScaleBgrxItems(const ScaleItems &items, int count, int srcW, int srcH, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream) {
	if (count < 1 || count > kFlowBatchMax) throw std::invalid_argument("launchScaleBgrxItems: 1 .. 8 items");
	if (srcW < 1 || srcH < 1 || dstW < 1 || dstH < 1 || spanX < 4 || spanX % 4) {
		throw std::invalid_argument("launchScaleBgrxItems: bad arguments");
	}
	for (int i = 0; i < count; ++i) {
		if (items.item[i].src == nullptr || items.item[i].dst == nullptr) throw std::invalid_argument("launchScaleBgrxItems: bad arguments");
	}
	const int pitch = spanX + spanX / 32 + 1;
	const std::size_t lds = static_cast<std::size_t>(3) * kScaleTileH * static_cast<std::size_t>(pitch) * sizeof(unsigned);
	if (lds > 64 * 1024) throw std::invalid_argument("launchScaleBgrxItems: the tile does not fit the LDS");
	const dim3 grid(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW),
	    static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH), static_cast<unsigned>(count));
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	if (x.filter != y.filter) throw std::invalid_argument("launchScaleBgrxItems: the two axes' tables must be of one filter");
	const auto kernel = x.filter != kScaleTriangle ? scale_bgrx_items_kernel<true> : scale_bgrx_items_kernel<false>;
	hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, items, srcW, dstW, dstH, tx, ty, pitch);
	hipCheckLaunch("scale_bgrx_items");
}

ScaleMember scaleMember(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, std::uint8_t *dst, std::ptrdiff_t dstStride,
    const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX) {
	if (src == nullptr || dst == nullptr || srcW < 1 || spanX < 4 || spanX % 4 || x.start == nullptr || x.taps == nullptr ||
	    y.start == nullptr || y.taps == nullptr) {
		throw std::invalid_argument("scaleMember: bad arguments");
	}
	if (x.filter != y.filter) throw std::invalid_argument("scaleMember: the two axes' tables must be of one filter");
	ScaleMember m;
	m.src = src;
	m.srcStride = srcStride;
	m.dst = dst;
	m.dstStride = dstStride;
	m.xStart = x.start;
	m.xTaps = x.taps;
	m.yStart = y.start;
	m.yTaps = y.taps;
	m.srcW = srcW;
	m.pitch = spanX + spanX / 32 + 1;
	m.cubic = x.filter != kScaleTriangle ? 1 : 0;
	ScaleMembers one{};
	one.member[0] = m;
	if (scaleMembersLds(one, 1) > 64 * 1024) throw std::invalid_argument("scaleMember: the tile does not fit the LDS");
	return m;
}

std::size_t scaleMembersLds(const ScaleMembers &members, int count) {
	if (count < 1 || count > kFlowBatchMax) throw std::invalid_argument("launchScaleBgrxMembers: 1 .. 8 members");
	std::size_t most = 0;
	for (int i = 0; i < count; ++i) {
		if (members.member[i].pitch < 1) throw std::invalid_argument("launchScaleBgrxMembers: bad arguments");
		most = std::max(most, static_cast<std::size_t>(3) * kScaleTileH * static_cast<std::size_t>(members.member[i].pitch) * sizeof(unsigned));
	}
	return most;
}

void launchScaleBgrxMembers(const ScaleMembers &members, int count, int dstW, int dstH, hipStream_t stream) {
	const std::size_t lds = scaleMembersLds(members, count);  // (the largest member's tile; refuses a count outside 1 .. 8)
	if (dstW < 1 || dstH < 1) throw std::invalid_argument("launchScaleBgrxMembers: bad arguments");
	for (int i = 0; i < count; ++i) {
		const ScaleMember &m = members.member[i];
		if (m.src == nullptr || m.dst == nullptr || m.srcW < 1 || m.xStart == nullptr || m.xTaps == nullptr || m.yStart == nullptr ||
		    m.yTaps == nullptr) {
			throw std::invalid_argument("launchScaleBgrxMembers: bad arguments");
		}
	}
	if (lds > 64 * 1024) throw std::invalid_argument("launchScaleBgrxMembers: the tile does not fit the LDS");
	const dim3 grid(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW),
	    static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH), static_cast<unsigned>(count));
	hipLaunchKernelGGL(scale_bgrx_members_kernel, grid, dim3(256), lds, stream, members, dstW, dstH);
	hipCheckLaunch("scale_bgrx_members");
}

void launchScaleState(const void *state, int srcW, int srcH, std::uint16_t *dst, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream) {
	if (state == nullptr || dst == nullptr || srcW < 1 || srcH < 1 || dstW < 1 || dstH < 1 || spanX < 4 || spanX % 4 ||
	    (reinterpret_cast<std::uintptr_t>(state) & 15) != 0 || (reinterpret_cast<std::uintptr_t>(dst) & 7) != 0) {
		throw std::invalid_argument("launchScaleState: bad arguments");
	}
	const int pitch = spanX + spanX / 32 + 1;
	const std::size_t lds = static_cast<std::size_t>(3) * kScaleTileH * static_cast<std::size_t>(pitch) * sizeof(unsigned);
	if (lds > 64 * 1024) throw std::invalid_argument("launchScaleState: the tile does not fit the LDS");
	const dim3 grid(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW),
	    static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH));
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	if (x.filter != y.filter) throw std::invalid_argument("launchScaleState: the two axes' tables must be of one filter");
	const auto kernel = x.filter != kScaleTriangle ? scale_state_kernel<true> : scale_state_kernel<false>;  // (spanX is of that form too)
	hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, static_cast<const f16 *>(state), srcW, dst, dstW, dstH, tx, ty, pitch);
	hipCheckLaunch("scale_state");
}

void launchMaskBlend(std::uint8_t *gen, std::ptrdiff_t genStride, int outW, int outH, const std::uint8_t *src,
    std::ptrdiff_t srcStride, int srcW, int srcH, const std::uint8_t *mask, std::ptrdiff_t maskStride, int maskW,
    int maskH, hipStream_t stream) {
	if (gen == nullptr || src == nullptr || mask == nullptr || outW < 1 || outH < 1 || srcW < 1 || srcH < 1 || maskW < 1 ||
	    maskH < 1) {
		throw std::invalid_argument("launchMaskBlend: bad arguments");
	}
	const auto below32 = [](int out, int tex) { return 2ull * static_cast<unsigned>(out) * static_cast<unsigned>(tex) < (1ull << 32); };
	if (!below32(outW, srcW) || !below32(outW, maskW) || !below32(outH, srcH) || !below32(outH, maskH)) {
		throw std::invalid_argument("launchMaskBlend: 2 x output extent x texture extent must stay below 2^32");
	}
	const dim3 grid(static_cast<unsigned>((outW + 63) / 64), static_cast<unsigned>((outH + 3) / 4));
	hipLaunchKernelGGL(mask_blend_kernel, grid, dim3(64, 4), 0, stream, gen, genStride, static_cast<unsigned>(outW),
	    static_cast<unsigned>(outH), src, srcStride, static_cast<unsigned>(srcW), static_cast<unsigned>(srcH), mask,
	    maskStride, static_cast<unsigned>(maskW), static_cast<unsigned>(maskH));
	hipCheckLaunch("mask_blend");
}

}  // namespace ju
