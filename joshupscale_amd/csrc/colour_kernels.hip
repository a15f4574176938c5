// 8-bit 4:2:0 YUV (I420 / YV12 / NV12) <-> BGRX conversion on gfx950: the colour staging of ju_process_frame.
//
// Both kernels are integer arithmetic and compute exactly the numpy definition of tests/yuv_reference.py (formulas:
// INTEGRATION.md, "YUV frames").  They are HBM-bound: one thread covers a strip of 16 pixels x 2 luma rows (one row of
// chroma cells), lanes run along the strip's row and wrap to the next row pair, so a wave reads and writes contiguous
// bytes; where a row is 16-byte aligned (every staging buffer, every plane a decoder allocates) its bytes move as
// 16-byte loads / stores, elsewhere (odd offsets, odd strides, the last strip of a row) byte by byte.  Rows are
// addressed with their signed stride: bottom-up planes need no flip pass.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernel_common.h"
#include "kernels.h"

namespace ju {
// Encode coefficients (kernel arguments).  8-bit: x 65536, rounded half away from zero (tests/yuv_reference.py).  10-bit
// (tests/yuv10_reference.py): x 2^32 / 65535, applied to a 16-bit sample P per channel (each below 2^26; products summed in
// 64 bits).  oy = luma offset (16 / 64 limited, 0 full range).
struct YuvEncode {
	int yr, yg, yb, ur, ug, ub, vr, vg, vb, oy;
};
struct YuvEncode10 {
	int yr, yg, yb, ur, ug, ub, vr, vg, vb, oy;
};
namespace {

constexpr int kStrip = 16;  // luma pixels per thread and row

// four dwords moved as ONE 16-byte access (a struct of four members is split into member accesses, which the compiler
// then merges with an equal dword path and loses the width)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ inline bool alignedTo(const void *p, unsigned a) {
	return (reinterpret_cast<std::uintptr_t>(p) & (a - 1)) == 0;
}

__device__ inline int byteOf(const unsigned *w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255; }

__device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// `N` (8 or 16) bytes of one row from byte `col` on, as words; `fast`: in range and aligned (else byte by byte, the
// column index clamped to `last`)
template <int N>
__device__ inline void loadBytes(const std::uint8_t *row, int col, int last, bool fast, unsigned (&w)[N / 4]) {
	if (fast && alignedTo(row + col, N)) {
		if constexpr (N == 16) {
			const uint4 v = *reinterpret_cast<const uint4 *>(row + col);
			w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
		} else {
			const uint2 v = *reinterpret_cast<const uint2 *>(row + col);
			w[0] = v.x, w[1] = v.y;
		}
		return;
	}
	if (fast && alignedTo(row + col, 4)) {
#pragma unroll
		for (int q = 0; q < N / 4; ++q) w[q] = reinterpret_cast<const unsigned *>(row + col)[q];
		return;
	}
#pragma unroll
	for (int q = 0; q < N / 4; ++q) {
		unsigned x = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) x |= static_cast<unsigned>(row[min(col + 4 * q + b, last)]) << (8 * b);
		w[q] = x;
	}
}

// `N` bytes (8 or 16) of one row from byte `col` on; `fast`: all in range (else only the first `n`)
template <int N>
__device__ inline void storeBytes(std::uint8_t *row, int col, int n, bool fast, const unsigned (&w)[N / 4]) {
	if (fast && alignedTo(row + col, N)) {
		if constexpr (N == 16) {
			*reinterpret_cast<uint4 *>(row + col) = make_uint4(w[0], w[1], w[2], w[3]);
		} else {
			*reinterpret_cast<uint2 *>(row + col) = make_uint2(w[0], w[1]);
		}
		return;
	}
	if (fast && alignedTo(row + col, 4)) {
#pragma unroll
		for (int q = 0; q < N / 4; ++q) reinterpret_cast<unsigned *>(row + col)[q] = w[q];
		return;
	}
#pragma unroll
	for (int k = 0; k < N; ++k) {
		if (fast || k < n) row[col + k] = static_cast<std::uint8_t>(byteOf(w, k));
	}
}

// The chroma upsampling of a 4:2:0 decode under siting S (kChroma*; tests/chroma_siting_reference.py), in integers at a
// scale of 2^kLog2.  Per axis, co-sited: position 2i takes 2 c[i], 2i + 1 takes c[i] + c[i + 1]; centred: 3 c[i] + c[i - 1]
// and 3 c[i] + c[i + 1].  Left = co-sited x centred (the scale of 8 every kernel here had), centre = centred x centred (16),
// top-left = co-sited x co-sited (4); the luma term and the rounding shift follow the scale, which leaves the bytes those
// of the definition's one scale: (2 a + 2^19) >> 20 = (a + 2^18) >> 19.
template <int S>
struct Upsample420 {
	static constexpr int kLog2 = S == kChromaCenter ? 4 : (S == kChromaTopLeft ? 2 : 3);
	static constexpr int kN = S == kChromaCenter ? 10 : 9;     // samples of a chroma row: [0 .. 8] = columns c0 .. c0 + 8, [9] = c0 - 1
	static constexpr int kRow0 = S == kChromaTopLeft ? 1 : 0;  // of the rows [0 .. 2] = j - 1, j, j + 1: the first one read
	// luma row 2j + r from chroma rows j - 1, j, j + 1
	__device__ static int vertical(int above, int at, int below, int r) {
		if constexpr (S == kChromaTopLeft) return r == 0 ? 2 * at : at + below;
		else return 3 * at + (r == 0 ? above : below);
	}
	// luma column x0 + p from the row's samples
	template <int N>
	__device__ static int horizontal(const int (&v)[N], int p) {
		const int i = p >> 1;
		if constexpr (S == kChromaCenter) return 3 * v[i] + ((p & 1) ? v[i + 1] : v[i == 0 ? 9 : i - 1]);
		else return (p & 1) ? v[i] + v[i + 1] : 2 * v[i];
	}
};

// Y, U, V (I420) or Y, UV (NV12) -> BGRX.  Thread = chroma row j (luma rows 2j, 2j + 1) x luma columns x0 .. x0 + 15;
// it reads chroma rows j - 1 .. j + 1 at columns x0 / 2 .. x0 / 2 + 8 (clamped to the plane).  The strip of thread `idx`:
// the body of both decode kernels below, so that a frame decoded inside a look-ahead pass has the single frame's bytes.
template <bool NV12, int S>
__device__ inline void yuv420ToBgrxStrip(const YuvPlanes &src, const YuvDecode &k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H, int idx) {
	using Up = Upsample420<S>;
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * (H / 2)) return;
	const int j = idx / strips;
	const int x0 = (idx - j * strips) * kStrip;
	const int CW = W / 2, CH = H / 2;
	const int c0 = x0 / 2;
	const bool full = x0 + kStrip <= W;

	// chroma rows j - 1, j, j + 1 (clamped; top-left: j and j + 1 only), 9 samples each: columns c0 .. c0 + 8 (clamped);
	// centre: a tenth, [9] = column c0 - 1 (clamped), the last cell of the neighbouring strip
	int cu[3][Up::kN], cv[3][Up::kN];
	if constexpr (Up::kRow0 > 0) {  // (row j - 1 is not read and not used)
#pragma unroll
		for (int i = 0; i < Up::kN; ++i) cu[0][i] = cv[0][i] = 0;
	}
#pragma unroll
	for (int r = Up::kRow0; r < 3; ++r) {
		const int jr = min(max(j - 1 + r, 0), CH - 1);
		const int last = min(c0 + 8, CW - 1);
		if constexpr (NV12) {
			const std::uint8_t *row = src.u + static_cast<std::ptrdiff_t>(jr) * src.uStride;
			if (!full) {  // (the last strip of a row: U and V clamped to the last cell each)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const int c = min(c0 + i, CW - 1);
					cu[r][i] = row[2 * c];
					cv[r][i] = row[2 * c + 1];
				}
			} else {
				unsigned w[4];
				loadBytes<16>(row, 2 * c0, 2 * CW - 1, true, w);
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					cu[r][i] = byteOf(w, 2 * i);
					cv[r][i] = byteOf(w, 2 * i + 1);
				}
			}
			cu[r][8] = row[2 * last];
			cv[r][8] = row[2 * last + 1];
			if constexpr (Up::kN > 9) {
				const int before = max(c0 - 1, 0);
				cu[r][9] = row[2 * before];
				cv[r][9] = row[2 * before + 1];
			}
		} else {
			const std::uint8_t *rowU = src.u + static_cast<std::ptrdiff_t>(jr) * src.uStride;
			const std::uint8_t *rowV = src.v + static_cast<std::ptrdiff_t>(jr) * src.vStride;
			unsigned wu[2], wv[2];
			loadBytes<8>(rowU, c0, CW - 1, full, wu);
			loadBytes<8>(rowV, c0, CW - 1, full, wv);
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				cu[r][i] = byteOf(wu, i);
				cv[r][i] = byteOf(wv, i);
			}
			cu[r][8] = rowU[last];
			cv[r][8] = rowV[last];
			if constexpr (Up::kN > 9) {
				const int before = max(c0 - 1, 0);
				cu[r][9] = rowU[before];
				cv[r][9] = rowV[before];
			}
		}
	}

#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const int y = 2 * j + r;
		unsigned yw[4];
		loadBytes<16>(src.y + static_cast<std::ptrdiff_t>(y) * src.yStride, x0, W - 1, full, yw);
		int vu[Up::kN], vv[Up::kN];
#pragma unroll
		for (int i = 0; i < Up::kN; ++i) {
			vu[i] = Up::vertical(cu[0][i], cu[1][i], cu[2][i], r);
			vv[i] = Up::vertical(cv[0][i], cv[1][i], cv[2][i], r);
		}
		unsigned px[16];
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			const int du = Up::horizontal(vu, p) - (128 << Up::kLog2);
			const int dv = Up::horizontal(vv, p) - (128 << Up::kLog2);
			const int yd = k.ky * ((1 << Up::kLog2) * (byteOf(yw, p) - k.oy));
			const int R = clamp255((yd + k.krv * dv + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			const int G = clamp255((yd - k.kgu * du - k.kgv * dv + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			const int B = clamp255((yd + k.kbu * du + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			px[p] = static_cast<unsigned>(B) | (static_cast<unsigned>(G) << 8) | (static_cast<unsigned>(R) << 16);
		}
		std::uint8_t *row = dst + static_cast<std::ptrdiff_t>(y) * dstStride;
		const int n = min(kStrip, W - x0);
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const unsigned w[4] = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
			storeBytes<16>(row, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, w);
		}
	}
}

template <bool NV12, int S>
__global__ __launch_bounds__(256) void yuv420_to_bgrx_kernel(YuvPlanes src, YuvDecode k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H) {
	yuv420ToBgrxStrip<NV12, S>(src, k, dst, dstStride, W, H, blockIdx.x * 256 + threadIdx.x);
}

// The chroma sum of an encode under siting S, 4:2:0 (`Rows`: both axes) or 4:2:2 (the horizontal axis only).  Per axis,
// co-sited: [1, 2, 1] on 2i - 1 (clamped to 0), 2i, 2i + 1, weight 4; centred: [1, 1] on 2i, 2i + 1, weight 2.  The rounding
// shift of every encode is the coefficients' 16 or 32 bits + kLog2.
template <int S, bool Rows>
struct ChromaSum {
	static constexpr bool kCoH = S != kChromaCenter, kCoV = Rows && S == kChromaTopLeft;
	static constexpr int kLog2 = (kCoH ? 2 : 1) + (Rows ? (kCoV ? 2 : 1) : 0);  // 4:2:0: 3 (left), 2 (centre), 4 (top-left)
	static constexpr int kRow0 = kCoV ? -1 : 0;                                 // the luma rows summed: 2j + kRow0 .. 2j + 1
	__device__ static constexpr int rowWeight(int r) { return (kCoV && r == 0) ? 2 : 1; }
	// columns 2i - 1, 2i, 2i + 1
	__device__ static int across(int a, int b, int c) {
		if constexpr (kCoH) return a + 2 * b + c;
		else return b + c;
	}
	// (the same of get(q), get(q + 1), get(q + 2), each formed where it is summed)
	template <typename Get>
	__device__ static int acrossOf(Get get, int q) {
		if constexpr (kCoH) return get(q) + 2 * get(q + 1) + get(q + 2);
		else return get(q + 1) + get(q + 2);
	}
};

// BGRX -> Y, U, V (I420) or Y, UV (NV12).  Thread = luma rows 2j, 2j + 1 x columns x0 .. x0 + 15 (+ column x0 - 1,
// clamped to 0, for the chroma filter) -> 2 x 16 luma bytes and chroma cells x0 / 2 .. x0 / 2 + 7 of row j.
// (top-left: a third row, 2j - 1 clamped to 0 -- the row above's second -- enters the chroma sums only, accumulated row by row)
template <bool NV12, int S>
__global__ __launch_bounds__(256) void bgrx_to_yuv420_kernel(const std::uint8_t *__restrict__ src,
    std::ptrdiff_t srcStride, YuvEncode k, YuvPlanes dst, int W, int H) {
	using Sum = ChromaSum<S, true>;
	const int strips = (W + kStrip - 1) / kStrip;
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= strips * (H / 2)) return;
	const int j = idx / strips;
	const int x0 = (idx - j * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);  // luma columns of this strip (even)

	// per chroma cell: the sums of R, G, B of weight 2^Sum::kLog2 (left: [1, 2, 1] x [1, 1], 8 x C)
	int sr[8], sg[8], sb[8];
#pragma unroll
	for (int i = 0; i < 8; ++i) sr[i] = sg[i] = sb[i] = 0;
#pragma unroll
	for (int r = Sum::kRow0; r < 2; ++r) {
		const int y = r < 0 ? max(2 * j - 1, 0) : 2 * j + r;
		const std::uint8_t *row = src + static_cast<std::ptrdiff_t>(y) * srcStride;
		unsigned px[17];  // px[0] = column x0 - 1 (clamped), px[1 + p] = column x0 + p
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			unsigned w[4];
			// (byte path: whole pixels, the column clamped to W - 1)
			if (full) {
				loadBytes<16>(row, 4 * (x0 + 4 * q), 4 * W - 1, true, w);
			} else {
#pragma unroll
				for (int b = 0; b < 4; ++b) {
					const std::uint8_t *p = row + 4 * min(x0 + 4 * q + b, W - 1);
					w[b] = p[0] | (p[1] << 8) | (p[2] << 16);
				}
			}
#pragma unroll
			for (int b = 0; b < 4; ++b) px[1 + 4 * q + b] = w[b];
		}
		if constexpr (Sum::kCoH) {
			const std::uint8_t *p = row + 4 * max(x0 - 1, 0);
			px[0] = p[0] | (p[1] << 8) | (p[2] << 16);
		} else {
			px[0] = 0;  // (not summed)
		}
		if (r >= 0) {
			unsigned yw[4] = {0, 0, 0, 0};
#pragma unroll
			for (int p = 0; p < 16; ++p) {
				const int B = px[1 + p] & 255, G = (px[1 + p] >> 8) & 255, R = (px[1 + p] >> 16) & 255;
				const int Y = clamp255(k.oy + ((k.yr * R + k.yg * G + k.yb * B + (1 << 15)) >> 16));
				yw[p >> 2] |= static_cast<unsigned>(Y) << (8 * (p & 3));
			}
			storeBytes<16>(dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride, x0, n, full, yw);
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			// columns 2i - 1, 2i, 2i + 1 of the strip = px[2i], px[2i + 1], px[2i + 2]
			const unsigned a = px[2 * i], b = px[2 * i + 1], c = px[2 * i + 2];
			sb[i] += Sum::rowWeight(r) * Sum::across(a & 255, b & 255, c & 255);
			sg[i] += Sum::rowWeight(r) * Sum::across((a >> 8) & 255, (b >> 8) & 255, (c >> 8) & 255);
			sr[i] += Sum::rowWeight(r) * Sum::across((a >> 16) & 255, (b >> 16) & 255, (c >> 16) & 255);
		}
	}
	unsigned uw[2] = {0, 0}, vw[2] = {0, 0};
#pragma unroll
	for (int i = 0; i < 8; ++i) {
		const int U = clamp255(128 + ((k.ur * sr[i] + k.ug * sg[i] + k.ub * sb[i] + (1 << (15 + Sum::kLog2))) >> (16 + Sum::kLog2)));
		const int V = clamp255(128 + ((k.vr * sr[i] + k.vg * sg[i] + k.vb * sb[i] + (1 << (15 + Sum::kLog2))) >> (16 + Sum::kLog2)));
		uw[i >> 2] |= static_cast<unsigned>(U) << (8 * (i & 3));
		vw[i >> 2] |= static_cast<unsigned>(V) << (8 * (i & 3));
	}
	const int c0 = x0 / 2;
	if constexpr (NV12) {
		unsigned w[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) {  // U0 V0 U1 V1 from cells 2q, 2q + 1
			const unsigned u = (uw[q >> 1] >> (16 * (q & 1))) & 0xffff, v = (vw[q >> 1] >> (16 * (q & 1))) & 0xffff;
			w[q] = (u & 255) | ((v & 255) << 8) | ((u >> 8) << 16) | ((v >> 8) << 24);
		}
		storeBytes<16>(dst.u + static_cast<std::ptrdiff_t>(j) * dst.uStride, 2 * c0, n, full, w);
	} else {
		storeBytes<8>(dst.u + static_cast<std::ptrdiff_t>(j) * dst.uStride, c0, n / 2, full, uw);
		storeBytes<8>(dst.v + static_cast<std::ptrdiff_t>(j) * dst.vStride, c0, n / 2, full, vw);
	}
}

// ---- 10-bit 4:2:0: P010 (Y, interleaved UV; the value in the upper 10 bits of each word) / I010 (Y, U, V; the value
// in the low 10 bits) ------------------------------------------------------------------------------------------------
__device__ inline int sampleOf(const unsigned *w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xffff; }

__device__ inline int clamp1023(int v) { return v < 0 ? 0 : (v > 1023 ? 1023 : v); }

__device__ inline unsigned wordAt(const std::uint8_t *row, int sample) {
	return *reinterpret_cast<const std::uint16_t *>(row + 2 * static_cast<std::ptrdiff_t>(sample));
}

// `N` (8 or 16) 16-bit samples of one row from sample `col` on, two per word; `fast`: in range (16-byte loads where
// the address is 16-byte aligned, dwords at 4), else sample by sample, the index clamped to `last`
template <int N>
__device__ inline void loadSamples(const std::uint8_t *row, int col, int last, bool fast, unsigned (&w)[N / 2]) {
	const std::uint8_t *p = row + 2 * static_cast<std::ptrdiff_t>(col);
	if (fast && alignedTo(p, 16)) {
#pragma unroll
		for (int q = 0; q < N / 8; ++q) {
			const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
			w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
		}
		return;
	}
	if (fast && alignedTo(p, 4)) {
#pragma unroll
		for (int q = 0; q < N / 2; ++q) w[q] = reinterpret_cast<const unsigned *>(p)[q];
		return;
	}
#pragma unroll
	for (int q = 0; q < N / 2; ++q) {
		w[q] = wordAt(row, min(col + 2 * q, last)) | (wordAt(row, min(col + 2 * q + 1, last)) << 16);
	}
}

// `N` (8 or 16) 16-bit samples of one row from sample `col` on; `fast`: all in range (else only the first `n`)
template <int N>
__device__ inline void storeSamples(std::uint8_t *row, int col, int n, bool fast, const unsigned (&w)[N / 2]) {
	std::uint8_t *p = row + 2 * static_cast<std::ptrdiff_t>(col);
	if (fast && alignedTo(p, 16)) {
#pragma unroll
		for (int q = 0; q < N / 8; ++q) {
			reinterpret_cast<uint4 *>(p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
		}
		return;
	}
	if (fast && alignedTo(p, 4)) {
#pragma unroll
		for (int q = 0; q < N / 2; ++q) reinterpret_cast<unsigned *>(p)[q] = w[q];
		return;
	}
#pragma unroll
	for (int k = 0; k < N; ++k) {
		if (fast || k < n) reinterpret_cast<std::uint16_t *>(p)[k] = static_cast<std::uint16_t>(sampleOf(w, k));
	}
}

// P010 / I010 -> BGRX (u8): the strip of yuv420ToBgrxStrip with 16-bit samples -- 32 B of Y per row, 16 (+2) B of each
// chroma plane row or 32 (+4) B of UV, from three chroma rows.  `k`: the coefficients for 10-bit words.
template <bool P010, int S>
__device__ inline void yuv420p10ToBgrxStrip(const YuvPlanes &src, const YuvDecode &k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H, int idx) {
	using Up = Upsample420<S>;
	constexpr int kShift = P010 ? 6 : 0;  // (word >> 6, or word & 0x3ff)
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * (H / 2)) return;
	const int j = idx / strips;
	const int x0 = (idx - j * strips) * kStrip;
	const int CW = W / 2, CH = H / 2;
	const int c0 = x0 / 2;
	const bool full = x0 + kStrip <= W;

	int cu[3][Up::kN], cv[3][Up::kN];
	if constexpr (Up::kRow0 > 0) {  // (row j - 1 is not read and not used)
#pragma unroll
		for (int i = 0; i < Up::kN; ++i) cu[0][i] = cv[0][i] = 0;
	}
#pragma unroll
	for (int r = Up::kRow0; r < 3; ++r) {
		const int jr = min(max(j - 1 + r, 0), CH - 1);
		const int last = min(c0 + 8, CW - 1);
		if constexpr (P010) {
			const std::uint8_t *row = src.u + static_cast<std::ptrdiff_t>(jr) * src.uStride;
			if (!full) {  // (the last strip of a row: U and V clamped to the last cell each)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const int c = min(c0 + i, CW - 1);
					cu[r][i] = wordAt(row, 2 * c) >> kShift;
					cv[r][i] = wordAt(row, 2 * c + 1) >> kShift;
				}
			} else {
				unsigned w[8];
				loadSamples<16>(row, 2 * c0, 2 * CW - 1, true, w);
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					cu[r][i] = sampleOf(w, 2 * i) >> kShift;
					cv[r][i] = sampleOf(w, 2 * i + 1) >> kShift;
				}
			}
			cu[r][8] = wordAt(row, 2 * last) >> kShift;
			cv[r][8] = wordAt(row, 2 * last + 1) >> kShift;
			if constexpr (Up::kN > 9) {
				const int before = max(c0 - 1, 0);
				cu[r][9] = wordAt(row, 2 * before) >> kShift;
				cv[r][9] = wordAt(row, 2 * before + 1) >> kShift;
			}
		} else {
			const std::uint8_t *rowU = src.u + static_cast<std::ptrdiff_t>(jr) * src.uStride;
			const std::uint8_t *rowV = src.v + static_cast<std::ptrdiff_t>(jr) * src.vStride;
			unsigned wu[4], wv[4];
			loadSamples<8>(rowU, c0, CW - 1, full, wu);
			loadSamples<8>(rowV, c0, CW - 1, full, wv);
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				cu[r][i] = sampleOf(wu, i) & 0x3ff;
				cv[r][i] = sampleOf(wv, i) & 0x3ff;
			}
			cu[r][8] = wordAt(rowU, last) & 0x3ff;
			cv[r][8] = wordAt(rowV, last) & 0x3ff;
			if constexpr (Up::kN > 9) {
				const int before = max(c0 - 1, 0);
				cu[r][9] = wordAt(rowU, before) & 0x3ff;
				cv[r][9] = wordAt(rowV, before) & 0x3ff;
			}
		}
	}

#pragma unroll
	for (int r = 0; r < 2; ++r) {
		const int y = 2 * j + r;
		unsigned yw[8];
		loadSamples<16>(src.y + static_cast<std::ptrdiff_t>(y) * src.yStride, x0, W - 1, full, yw);
		int vu[Up::kN], vv[Up::kN];
#pragma unroll
		for (int i = 0; i < Up::kN; ++i) {
			vu[i] = Up::vertical(cu[0][i], cu[1][i], cu[2][i], r);
			vv[i] = Up::vertical(cv[0][i], cv[1][i], cv[2][i], r);
		}
		unsigned px[16];
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			const int du = Up::horizontal(vu, p) - (512 << Up::kLog2);
			const int dv = Up::horizontal(vv, p) - (512 << Up::kLog2);
			const int Y = P010 ? sampleOf(yw, p) >> kShift : sampleOf(yw, p) & 0x3ff;
			const int yd = k.ky * ((1 << Up::kLog2) * (Y - k.oy));
			const int R = clamp255((yd + k.krv * dv + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			const int G = clamp255((yd - k.kgu * du - k.kgv * dv + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			const int B = clamp255((yd + k.kbu * du + (1 << (15 + Up::kLog2))) >> (16 + Up::kLog2));
			px[p] = static_cast<unsigned>(B) | (static_cast<unsigned>(G) << 8) | (static_cast<unsigned>(R) << 16);
		}
		std::uint8_t *row = dst + static_cast<std::ptrdiff_t>(y) * dstStride;
		const int n = min(kStrip, W - x0);
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const unsigned w[4] = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
			storeBytes<16>(row, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, w);
		}
	}
}

template <bool P010, int S>
__global__ __launch_bounds__(256) void yuv420p10_to_bgrx_kernel(YuvPlanes src, YuvDecode k,
    std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int W, int H) {
	yuv420p10ToBgrxStrip<P010, S>(src, k, dst, dstStride, W, H, blockIdx.x * 256 + threadIdx.x);
}

// the sample kinds of the RGB formats ("RGB formats" below)
enum RgbKind : int { kU8, kW16, kW10, kHalf, kUnit, kF255 };

// The 16-bit samples P (0 .. 65535) of 17 pixels of one row -- column x0 - 1 (clamped to 0) and columns x0 .. x0 + 15
// (clamped to W - 1) -- as the two sources of the 10-bit encode form them; kept packed (registers), read through b / g / r.
// From the engine's f16 state [H][W][4] (B, G, R, 0; dense, 16-byte aligned): floor((s + 0.5) * 65536), saturated.  In
// f32 that is exact: every f16 of magnitude up to 0.5 is a multiple of 2^-24, and s + 0.5 then has 24 significant bits.
struct StateSource {
	using Pixel = uint2;  // x = P_B | P_G << 16, y = P_R
	const f16 *state;
	static constexpr int kScale = 1;
	__device__ static unsigned sample(unsigned bits) {
		const float s = static_cast<float>(__builtin_bit_cast(f16, static_cast<unsigned short>(bits)));
		return static_cast<unsigned>(fminf(fmaxf(floorf((s + 0.5f) * 65536.0f), 0.0f), 65535.0f));
	}
	__device__ static Pixel unpack(unsigned lo, unsigned hi) {
		return make_uint2(sample(lo & 0xffff) | (sample(lo >> 16) << 16), sample(hi & 0xffff));
	}
	__device__ static int b(Pixel p) { return static_cast<int>(p.x & 0xffff); }
	__device__ static int g(Pixel p) { return static_cast<int>(p.x >> 16); }
	__device__ static int r(Pixel p) { return static_cast<int>(p.y); }
	__device__ void load(int y, int x0, int W, bool full, Pixel (&px)[17]) const {
		const f16 *row = state + static_cast<std::size_t>(y) * W * 4;
		{
			const uint2 v = *reinterpret_cast<const uint2 *>(row + 4 * max(x0 - 1, 0));
			px[0] = unpack(v.x, v.y);
		}
		if (full && alignedTo(row, 16)) {  // (a row of an odd width starts at 8 bytes: pixel by pixel below)
#pragma unroll
			for (int q = 0; q < 8; ++q) {
				const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * (x0 + 2 * q));
				px[1 + 2 * q] = unpack(v.x, v.y);
				px[2 + 2 * q] = unpack(v.z, v.w);
			}
		} else {
#pragma unroll
			for (int p = 0; p < 16; ++p) {
				const uint2 v = *reinterpret_cast<const uint2 *>(row + 4 * min(x0 + p, W - 1));
				px[1 + p] = unpack(v.x, v.y);
			}
		}
	}
	// An RGB encode ("RGB formats" below) reads the strip's 16 pixels as they lie in memory (no neighbour column: nothing
	// is filtered) and forms one channel's sample of kind K (RgbKind): t = s + 0.5, exact in f32; W16 is `sample`, W10 its
	// upper 10 bits, the float kinds clamp(t, 0, 1), that as f16 rounded to nearest even, or x 255.
	using Raw = uint2;  // the pixel's four f16: x = B | G << 16, y = R | unused << 16
	__device__ static unsigned rawB(Raw p) { return p.x & 0xffff; }
	__device__ static unsigned rawG(Raw p) { return p.x >> 16; }
	__device__ static unsigned rawR(Raw p) { return p.y & 0xffff; }
	template <int K>
	__device__ static unsigned deep(unsigned bits) {
		if constexpr (K == kW16) return sample(bits);
		else if constexpr (K == kW10) return sample(bits) >> 6;
		else {
			const float t = static_cast<float>(__builtin_bit_cast(f16, static_cast<unsigned short>(bits))) + 0.5f;
			const float u = fminf(fmaxf(t, 0.0f), 1.0f);
			if constexpr (K == kUnit) return __builtin_bit_cast(unsigned, u);
			else if constexpr (K == kHalf) return __builtin_bit_cast(unsigned short, static_cast<f16>(u));
			else return __builtin_bit_cast(unsigned, u * 255.0f);
		}
	}
	__device__ void loadRaw(int y, int x0, int W, bool full, Raw (&px)[16]) const {
		const f16 *row = state + static_cast<std::size_t>(y) * W * 4;
		if (full && alignedTo(row, 16)) {  // (a row of an odd width starts at 8 bytes: pixel by pixel below)
#pragma unroll
			for (int q = 0; q < 8; ++q) {
				const u32x4 v = *reinterpret_cast<const u32x4 *>(row + 4 * (x0 + 2 * q));
				px[2 * q] = make_uint2(v.x, v.y);
				px[2 * q + 1] = make_uint2(v.z, v.w);
			}
		} else {
#pragma unroll
			for (int p = 0; p < 16; ++p) px[p] = *reinterpret_cast<const uint2 *>(row + 4 * min(x0 + p, W - 1));
		}
	}
};

// From a u8 BGRX frame (any alignment, signed stride): P = 257 u8 -- the bytes stay bytes, see kScale.
struct Bgrx8Source {
	using Pixel = unsigned;  // B | G << 8 | R << 16, as in the frame
	const std::uint8_t *src;
	std::ptrdiff_t stride;
	static constexpr int kScale = 257;  // (applied to the weighted sums: 257 sum(c u8) = sum(c P), in integers)
	__device__ static int b(Pixel p) { return static_cast<int>(p & 255); }
	__device__ static int g(Pixel p) { return static_cast<int>((p >> 8) & 255); }
	__device__ static int r(Pixel p) { return static_cast<int>((p >> 16) & 255); }
	__device__ void load(int y, int x0, int W, bool full, Pixel (&px)[17]) const {
		const std::uint8_t *row = src + static_cast<std::ptrdiff_t>(y) * stride;
		{
			const std::uint8_t *p = row + 4 * max(x0 - 1, 0);
			px[0] = p[0] | (p[1] << 8) | (p[2] << 16);
		}
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			unsigned w[4];
			if (full) {
				loadBytes<16>(row, 4 * (x0 + 4 * q), 4 * W - 1, true, w);
			} else {
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const std::uint8_t *p = row + 4 * min(x0 + 4 * q + i, W - 1);
					w[i] = p[0] | (p[1] << 8) | (p[2] << 16);
				}
			}
#pragma unroll
			for (int i = 0; i < 4; ++i) px[1 + 4 * q + i] = w[i];
		}
	}
	// For an RGB encode: P = 257 u8; the float kinds f32(u8) / 255 (one correctly rounded division), that as f16, or f32(u8).
	using Raw = unsigned;  // B | G << 8 | R << 16, as in the frame
	__device__ static unsigned rawB(Raw p) { return p & 255; }
	__device__ static unsigned rawG(Raw p) { return (p >> 8) & 255; }
	__device__ static unsigned rawR(Raw p) { return (p >> 16) & 255; }
	template <int K>
	__device__ static unsigned deep(unsigned u) {
		if constexpr (K == kW16) return 257 * u;
		else if constexpr (K == kW10) return (257 * u) >> 6;
		else if constexpr (K == kUnit) return __builtin_bit_cast(unsigned, static_cast<float>(u) / 255.0f);
		else if constexpr (K == kHalf) {
			return __builtin_bit_cast(unsigned short, static_cast<f16>(static_cast<float>(u) / 255.0f));
		} else if constexpr (K == kF255) return __builtin_bit_cast(unsigned, static_cast<float>(u));
		else return u;
	}
	__device__ void loadRaw(int y, int x0, int W, bool full, Raw (&px)[16]) const {
		const std::uint8_t *row = src + static_cast<std::ptrdiff_t>(y) * stride;
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			unsigned w[4];
			if (full) {
				loadBytes<16>(row, 4 * (x0 + 4 * q), 4 * W - 1, true, w);
			} else {
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const std::uint8_t *p = row + 4 * min(x0 + 4 * q + i, W - 1);
					w[i] = p[0] | (p[1] << 8) | (p[2] << 16);
				}
			}
#pragma unroll
			for (int i = 0; i < 4; ++i) px[4 * q + i] = w[i];
		}
	}
};

// From a dense u16 BGRX frame [H][W][4] (B, G, R, unused; 8-byte aligned: the output stage's scaled 16-bit frame,
// docs/output_stage.md): the sample is P itself.  Rows of an odd width start at 8 bytes, as the state's.
struct Bgrx16Source {
	using Pixel = uint2;  // x = P_B | P_G << 16, y = P_R | unused << 16
	const std::uint16_t *frame;
	static constexpr int kScale = 1;
	__device__ static int b(Pixel p) { return static_cast<int>(p.x & 0xffff); }
	__device__ static int g(Pixel p) { return static_cast<int>(p.x >> 16); }
	__device__ static int r(Pixel p) { return static_cast<int>(p.y & 0xffff); }
	__device__ void load(int y, int x0, int W, bool full, Pixel (&px)[17]) const {
		const std::uint16_t *row = frame + static_cast<std::size_t>(y) * W * 4;
		px[0] = *reinterpret_cast<const uint2 *>(row + 4 * max(x0 - 1, 0));
		Raw raw[16];
		loadRaw(y, x0, W, full, raw);
#pragma unroll
		for (int p = 0; p < 16; ++p) px[1 + p] = raw[p];
	}
	// For an RGB encode: W16 = P, W10 = P >> 6; the float kinds f32(P) / 65535 (one correctly rounded division), that as
	// f16 rounded to nearest even, or f32(P) / 257.
	using Raw = uint2;
	__device__ static unsigned rawB(Raw p) { return p.x & 0xffff; }
	__device__ static unsigned rawG(Raw p) { return p.x >> 16; }
	__device__ static unsigned rawR(Raw p) { return p.y & 0xffff; }
	template <int K>
	__device__ static unsigned deep(unsigned p) {
		if constexpr (K == kW16) return p;
		else if constexpr (K == kW10) return p >> 6;
		else if constexpr (K == kUnit) return __builtin_bit_cast(unsigned, static_cast<float>(p) / 65535.0f);
		else if constexpr (K == kHalf) {
			return __builtin_bit_cast(unsigned short, static_cast<f16>(static_cast<float>(p) / 65535.0f));
		} else return __builtin_bit_cast(unsigned, static_cast<float>(p) / 257.0f);
	}
	__device__ void loadRaw(int y, int x0, int W, bool full, Raw (&px)[16]) const {
		const std::uint16_t *row = frame + static_cast<std::size_t>(y) * W * 4;
		if (full && alignedTo(row, 16)) {
#pragma unroll
			for (int q = 0; q < 8; ++q) {
				const u32x4 v = *reinterpret_cast<const u32x4 *>(row + 4 * (x0 + 2 * q));
				px[2 * q] = make_uint2(v.x, v.y);
				px[2 * q + 1] = make_uint2(v.z, v.w);
			}
		} else {
#pragma unroll
			for (int p = 0; p < 16; ++p) px[p] = *reinterpret_cast<const uint2 *>(row + 4 * min(x0 + p, W - 1));
		}
	}
};

// P -> Y, U, V (I010) or Y, UV (P010): the strip body of both 10-bit encodes.  Thread = luma rows 2j, 2j + 1 x columns
// x0 .. x0 + 15 -> 2 x 32 B of Y and 16 B of U and of V (32 B of UV).  64-bit accumulators: the products reach 2^45.
template <bool P010, int S, typename Source>
__device__ inline void toYuv420p10Strip(const Source &source, const YuvEncode10 &k, const YuvPlanes &dst, int W, int H,
    int idx) {
	using Sum = ChromaSum<S, true>;
	constexpr int kShift = P010 ? 6 : 0;
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * (H / 2)) return;
	const int j = idx / strips;
	const int x0 = (idx - j * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);  // luma columns of this strip (even)

	int sr[8], sg[8], sb[8];  // per chroma cell: the sums of the source's samples, of weight 2^Sum::kLog2 (left: [1, 2, 1] x [1, 1])
#pragma unroll
	for (int i = 0; i < 8; ++i) sr[i] = sg[i] = sb[i] = 0;
#pragma unroll
	for (int r = Sum::kRow0; r < 2; ++r) {  // (top-left: row 2j - 1, clamped to 0, enters the chroma sums only)
		const int y = r < 0 ? max(2 * j - 1, 0) : 2 * j + r;
		typename Source::Pixel px[17];  // [0] = column x0 - 1 (clamped), [1 + p] = column x0 + p
		source.load(y, x0, W, full, px);
		if (r >= 0) {
			unsigned yw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
			for (int p = 0; p < 16; ++p) {
				const long long acc = (static_cast<long long>(k.yr) * Source::r(px[1 + p]) +
				                       static_cast<long long>(k.yg) * Source::g(px[1 + p]) +
				                       static_cast<long long>(k.yb) * Source::b(px[1 + p])) * Source::kScale + (1ll << 31);
				const int Y = clamp1023(k.oy + static_cast<int>(acc >> 32));
				yw[p >> 1] |= static_cast<unsigned>(Y << kShift) << (16 * (p & 1));
			}
			storeSamples<16>(dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride, x0, n, full, yw);
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			// columns 2i - 1, 2i, 2i + 1 of the strip = px[2i], px[2i + 1], px[2i + 2]
			sb[i] += Sum::rowWeight(r) * Sum::across(Source::b(px[2 * i]), Source::b(px[2 * i + 1]), Source::b(px[2 * i + 2]));
			sg[i] += Sum::rowWeight(r) * Sum::across(Source::g(px[2 * i]), Source::g(px[2 * i + 1]), Source::g(px[2 * i + 2]));
			sr[i] += Sum::rowWeight(r) * Sum::across(Source::r(px[2 * i]), Source::r(px[2 * i + 1]), Source::r(px[2 * i + 2]));
		}
	}
	unsigned uw[4] = {0, 0, 0, 0}, vw[4] = {0, 0, 0, 0};
#pragma unroll
	for (int i = 0; i < 8; ++i) {
		const long long au = (static_cast<long long>(k.ur) * sr[i] + static_cast<long long>(k.ug) * sg[i] +
		                      static_cast<long long>(k.ub) * sb[i]) * Source::kScale + (1ll << (31 + Sum::kLog2));
		const long long av = (static_cast<long long>(k.vr) * sr[i] + static_cast<long long>(k.vg) * sg[i] +
		                      static_cast<long long>(k.vb) * sb[i]) * Source::kScale + (1ll << (31 + Sum::kLog2));
		const int U = clamp1023(512 + static_cast<int>(au >> (32 + Sum::kLog2)));
		const int V = clamp1023(512 + static_cast<int>(av >> (32 + Sum::kLog2)));
		uw[i >> 1] |= static_cast<unsigned>(U << kShift) << (16 * (i & 1));
		vw[i >> 1] |= static_cast<unsigned>(V << kShift) << (16 * (i & 1));
	}
	const int c0 = x0 / 2;
	if constexpr (P010) {
		unsigned w[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {  // U_i V_i
			w[i] = ((uw[i >> 1] >> (16 * (i & 1))) & 0xffff) | (((vw[i >> 1] >> (16 * (i & 1))) & 0xffff) << 16);
		}
		storeSamples<16>(dst.u + static_cast<std::ptrdiff_t>(j) * dst.uStride, 2 * c0, n, full, w);
	} else {
		storeSamples<8>(dst.u + static_cast<std::ptrdiff_t>(j) * dst.uStride, c0, n / 2, full, uw);
		storeSamples<8>(dst.v + static_cast<std::ptrdiff_t>(j) * dst.vStride, c0, n / 2, full, vw);
	}
}

template <bool P010, int S>
__global__ __launch_bounds__(256) void state_to_yuv420p10_kernel(const f16 *__restrict__ state, YuvEncode10 k,
    YuvPlanes dst, int W, int H) {
	toYuv420p10Strip<P010, S>(StateSource{state}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <bool P010, int S>
__global__ __launch_bounds__(256) void frame16_to_yuv420p10_kernel(const std::uint16_t *__restrict__ frame, YuvEncode10 k,
    YuvPlanes dst, int W, int H) {
	toYuv420p10Strip<P010, S>(Bgrx16Source{frame}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

// (214 VGPRs: the scheduler hoists the byte extractions of a row over its 64-bit sums; held to 128 registers with
// amdgpu_waves_per_eu the kernel spills 352 B per lane, so it is left alone -- at 1920x1080 the grid is 254 workgroups on
// 256 CUs, one wave per SIMD, and the occupancy limit is never reached)
template <bool P010, int S>
__global__ __launch_bounds__(256) void bgrx_to_yuv420p10_kernel(const std::uint8_t *__restrict__ src,
    std::ptrdiff_t srcStride, YuvEncode10 k, YuvPlanes dst, int W, int H) {
	toYuv420p10Strip<P010, S>(Bgrx8Source{src, srcStride}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

// ---- 4:2:2 and 4:4:4, 8- and 10-bit (tests/yuv_sampled_reference.py; docs/yuv_io.md, "4:2:2 and 4:4:4") ----------------
// Nothing couples rows here, so a thread's strip is 16 luma pixels of ONE row: thread idx = row idx / strips, columns
// x0 .. x0 + 15.  Chroma is co-sited with the even luma columns (4:2:2) or with every pixel (4:4:4); the luma formulas,
// the coefficients and the sample P are those of the 4:2:0 kernels above.  F is the frame's PixelFormat value.
template <int F>
struct SampledTraits {
	static constexpr bool kPacked = F == kYuy2 || F == kUyvy;
	static constexpr bool kDeep = F == kP210 || F == kI210 || F == kI410 || F == kY210 || F == kY410;
	static constexpr bool kFull = F == kI444 || F == kI410 || F == kY410;  // (4:4:4: a chroma sample per pixel)
	static constexpr bool kSemi = F == kP210;
	static constexpr int kShift = (F == kP210 || F == kY210) ? 6 : 0;  // (word >> 6, or word & 0x3ff)
	static constexpr int kYByte = F == kYuy2 ? 0 : 1;        // packed: the byte of Y0 in a pair's four (U: 1 - kYByte)
	static constexpr int kMid = kDeep ? 512 : 128;
};

// (runs of samples: "RGB formats" below; Y410's dwords move as such a run)
template <int B, int N, int G>
__device__ inline void loadRun(const std::uint8_t *row, int first, int lastGroup, bool fast, unsigned (&w)[N * B / 4]);
template <int B, int N>
__device__ inline void storeRun(std::uint8_t *row, int first, int n, bool fast, const unsigned (&w)[N * B / 4]);

// The strip's 16 luma samples and its chroma samples as integers: 4:4:4 cu / cv[0 .. 15]; 4:2:2 cu / cv[0 .. 7] = cells
// x0 / 2 .. x0 / 2 + 7 and [8] = the next cell, for the odd column of the last pixel.  Every index is clamped to its row.
template <int F>
__device__ inline void loadSampledStrip(const YuvPlanes &src, int y, int x0, int W, bool full, int (&ys)[16],
    int (&cu)[17], int (&cv)[17]) {
	using T = SampledTraits<F>;
	const int CW = T::kFull ? W : W / 2;
	const int c0 = T::kFull ? x0 : x0 / 2;
	const std::uint8_t *rowY = src.y + static_cast<std::ptrdiff_t>(y) * src.yStride;
	if constexpr (F == kY210) {  // 16-bit words Y0 U Y1 V per pixel pair, two words a dword
		if (full) {
			unsigned w[16];
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				unsigned h[8];
				loadSamples<16>(rowY, 2 * x0 + 16 * q, 2 * W - 1, true, h);
#pragma unroll
				for (int i = 0; i < 8; ++i) w[8 * q + i] = h[i];
			}
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				ys[2 * i] = (w[2 * i] & 0xffff) >> T::kShift;
				cu[i] = w[2 * i] >> (16 + T::kShift);
				ys[2 * i + 1] = (w[2 * i + 1] & 0xffff) >> T::kShift;
				cv[i] = w[2 * i + 1] >> (16 + T::kShift);
			}
		} else {
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				const int c = min(c0 + i, CW - 1);
				ys[2 * i] = wordAt(rowY, 4 * c) >> T::kShift;
				cu[i] = wordAt(rowY, 4 * c + 1) >> T::kShift;
				ys[2 * i + 1] = wordAt(rowY, 4 * c + 2) >> T::kShift;
				cv[i] = wordAt(rowY, 4 * c + 3) >> T::kShift;
			}
		}
		const int last = min(c0 + 8, CW - 1);
		cu[8] = wordAt(rowY, 4 * last + 1) >> T::kShift;
		cv[8] = wordAt(rowY, 4 * last + 3) >> T::kShift;
		return;
	}
	if constexpr (F == kY410) {  // one dword per pixel: U, Y, V from bit 0 on, bits 30-31 ignored
		unsigned w[16];
		loadRun<4, 16, 1>(rowY, x0, W - 1, full, w);
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			cu[p] = w[p] & 0x3ff;
			ys[p] = (w[p] >> 10) & 0x3ff;
			cv[p] = (w[p] >> 20) & 0x3ff;
		}
		return;
	}
	if constexpr (T::kPacked) {
		constexpr int yb = T::kYByte, cb = 1 - T::kYByte;
		if (full) {
			unsigned w[8];
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				unsigned h[4];
				loadBytes<16>(rowY, 2 * x0 + 16 * q, 2 * W - 1, true, h);
#pragma unroll
				for (int i = 0; i < 4; ++i) w[4 * q + i] = h[i];
			}
#pragma unroll
			for (int i = 0; i < 8; ++i) {  // one word per pixel pair
				ys[2 * i] = (w[i] >> (8 * yb)) & 255;
				ys[2 * i + 1] = (w[i] >> (8 * yb + 16)) & 255;
				cu[i] = (w[i] >> (8 * cb)) & 255;
				cv[i] = (w[i] >> (8 * cb + 16)) & 255;
			}
		} else {
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				const std::uint8_t *p = rowY + 4 * min(c0 + i, CW - 1);
				ys[2 * i] = p[yb];
				ys[2 * i + 1] = p[yb + 2];
				cu[i] = p[cb];
				cv[i] = p[cb + 2];
			}
		}
		const std::uint8_t *p = rowY + 4 * min(c0 + 8, CW - 1);
		cu[8] = p[cb];
		cv[8] = p[cb + 2];
		return;
	}
	if constexpr (T::kDeep) {
		unsigned yw[8];
		loadSamples<16>(rowY, x0, W - 1, full, yw);
#pragma unroll
		for (int p = 0; p < 16; ++p) ys[p] = T::kShift ? sampleOf(yw, p) >> T::kShift : sampleOf(yw, p) & 0x3ff;
	} else {
		unsigned yw[4];
		loadBytes<16>(rowY, x0, W - 1, full, yw);
#pragma unroll
		for (int p = 0; p < 16; ++p) ys[p] = byteOf(yw, p);
	}
	const std::uint8_t *rowU = src.u + static_cast<std::ptrdiff_t>(y) * src.uStride;
	if constexpr (T::kSemi) {  // P210: U_i V_i words
		if (full) {
			unsigned w[8];
			loadSamples<16>(rowU, 2 * c0, 2 * CW - 1, true, w);
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				cu[i] = sampleOf(w, 2 * i) >> T::kShift;
				cv[i] = sampleOf(w, 2 * i + 1) >> T::kShift;
			}
		} else {
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				const int c = min(c0 + i, CW - 1);
				cu[i] = wordAt(rowU, 2 * c) >> T::kShift;
				cv[i] = wordAt(rowU, 2 * c + 1) >> T::kShift;
			}
		}
		const int last = min(c0 + 8, CW - 1);
		cu[8] = wordAt(rowU, 2 * last) >> T::kShift;
		cv[8] = wordAt(rowU, 2 * last + 1) >> T::kShift;
		return;
	} else {
		const std::uint8_t *rowV = src.v + static_cast<std::ptrdiff_t>(y) * src.vStride;
		constexpr int N = T::kFull ? 16 : 8;
		if constexpr (T::kDeep) {
			unsigned wu[N / 2], wv[N / 2];
			loadSamples<N>(rowU, c0, CW - 1, full, wu);
			loadSamples<N>(rowV, c0, CW - 1, full, wv);
#pragma unroll
			for (int i = 0; i < N; ++i) {
				cu[i] = sampleOf(wu, i) & 0x3ff;
				cv[i] = sampleOf(wv, i) & 0x3ff;
			}
			if constexpr (!T::kFull) {
				const int last = min(c0 + 8, CW - 1);
				cu[8] = wordAt(rowU, last) & 0x3ff;
				cv[8] = wordAt(rowV, last) & 0x3ff;
			}
		} else {
			unsigned wu[N / 4], wv[N / 4];
			loadBytes<N>(rowU, c0, CW - 1, full, wu);
			loadBytes<N>(rowV, c0, CW - 1, full, wv);
#pragma unroll
			for (int i = 0; i < N; ++i) {
				cu[i] = byteOf(wu, i);
				cv[i] = byteOf(wv, i);
			}
			if constexpr (!T::kFull) {
				const int last = min(c0 + 8, CW - 1);
				cu[8] = rowU[last];
				cv[8] = rowV[last];
			}
		}
	}
}

// 4:2:2 chroma at luma column x0 + p from the strip's cells c[0 ..] and the cell before them: left, at a scale of 8, c[i] at
// even columns and the mean of two at odd ones; centre, at a scale of 4, 3 c[i] + c[i - 1] and 3 c[i] + c[i + 1]
template <int S, int N>
__device__ inline int chromaAt422(const int (&c)[N], int before, int p) {
	const int i = p >> 1;
	if constexpr (S == kChromaCenter) return 3 * c[i] + ((p & 1) ? c[i + 1] : (i == 0 ? before : c[i - 1]));
	else return (p & 1) ? 4 * (c[i] + c[i + 1]) : 8 * c[i];
}

// chroma cell `c` (in range) of row y of a 4:2:2 format: what the centre siting reads of the strip to the left
template <int F>
__device__ inline void loadChromaCell(const YuvPlanes &src, int y, int c, int *u, int *v) {
	using T = SampledTraits<F>;
	static_assert(!T::kFull, "4:2:2 only");
	const std::uint8_t *rowY = src.y + static_cast<std::ptrdiff_t>(y) * src.yStride;
	if constexpr (F == kY210) {
		*u = wordAt(rowY, 4 * c + 1) >> T::kShift;
		*v = wordAt(rowY, 4 * c + 3) >> T::kShift;
	} else if constexpr (T::kPacked) {
		*u = rowY[4 * c + 1 - T::kYByte];
		*v = rowY[4 * c + 3 - T::kYByte];
	} else if constexpr (T::kSemi) {
		const std::uint8_t *rowU = src.u + static_cast<std::ptrdiff_t>(y) * src.uStride;
		*u = wordAt(rowU, 2 * c) >> T::kShift;
		*v = wordAt(rowU, 2 * c + 1) >> T::kShift;
	} else {
		const std::uint8_t *rowU = src.u + static_cast<std::ptrdiff_t>(y) * src.uStride;
		const std::uint8_t *rowV = src.v + static_cast<std::ptrdiff_t>(y) * src.vStride;
		if constexpr (T::kDeep) {
			*u = wordAt(rowU, c) & 0x3ff;
			*v = wordAt(rowV, c) & 0x3ff;
		} else {
			*u = rowU[c];
			*v = rowV[c];
		}
	}
}

// planes -> BGRX: the strip of thread `idx`; the body of the single-frame kernel and of the items kernel's branch.
// `k`: decodeCoefficients for the format (8-bit samples or 10-bit words).  S: kChromaLeft, or (4:2:2) kChromaCenter -- then
// the chroma at the pixel is 3 c[i] + c[i -+ 1], at a scale of 4, and cell x0 / 2 - 1 (clamped to 0) is read too.
template <int F, int S>
__device__ inline void yuvSampledToBgrxStrip(const YuvPlanes &src, const YuvDecode &k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H, int idx) {
	using T = SampledTraits<F>;
	static_assert(S == kChromaLeft || (S == kChromaCenter && !T::kFull), "4:2:2: left or centre; 4:4:4 has no siting");
	constexpr int kLog2 = S == kChromaCenter ? 2 : 3;  // log2 of the scale of the chroma at the pixel
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	int ys[16], cu[17], cv[17];
	loadSampledStrip<F>(src, y, x0, W, full, ys, cu, cv);
	int beforeU = 0, beforeV = 0;
	if constexpr (S == kChromaCenter) loadChromaCell<F>(src, y, max(x0 / 2 - 1, 0), &beforeU, &beforeV);
	unsigned px[16];
#pragma unroll
	for (int p = 0; p < 16; ++p) {
		int du, dv;  // 2^kLog2 x chroma at the pixel, less 2^kLog2 x the mid value
		if constexpr (T::kFull) {
			du = 8 * cu[p];
			dv = 8 * cv[p];
		} else {
			du = chromaAt422<S>(cu, beforeU, p);
			dv = chromaAt422<S>(cv, beforeV, p);
		}
		du -= T::kMid << kLog2;
		dv -= T::kMid << kLog2;
		const int yd = k.ky * ((1 << kLog2) * (ys[p] - k.oy));
		const int R = clamp255((yd + k.krv * dv + (1 << (15 + kLog2))) >> (16 + kLog2));
		const int G = clamp255((yd - k.kgu * du - k.kgv * dv + (1 << (15 + kLog2))) >> (16 + kLog2));
		const int B = clamp255((yd + k.kbu * du + (1 << (15 + kLog2))) >> (16 + kLog2));
		px[p] = static_cast<unsigned>(B) | (static_cast<unsigned>(G) << 8) | (static_cast<unsigned>(R) << 16);
	}
	std::uint8_t *row = dst + static_cast<std::ptrdiff_t>(y) * dstStride;
	const int n = min(kStrip, W - x0);
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const unsigned w[4] = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
		storeBytes<16>(row, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, w);
	}
}

template <int F, int S>
__global__ __launch_bounds__(256) void yuv_sampled_to_bgrx_kernel(YuvPlanes src, YuvDecode k,
    std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int W, int H) {
	yuvSampledToBgrxStrip<F, S>(src, k, dst, dstStride, W, H, blockIdx.x * 256 + threadIdx.x);
}

// The strip's samples (8-bit: bytes, 10-bit: values 0 .. 1023) into the planes of format F: `n` luma columns of row y
// from x0 (all 16 where `full`), `cu` / `cv` per chroma cell (4:2:2: 8) or per pixel (4:4:4: 16).
template <int F>
__device__ inline void storeSampledStrip(const YuvPlanes &dst, int y, int x0, int n, bool full, const int (&ys)[16],
    const int (&cu)[16], const int (&cv)[16]) {
	using T = SampledTraits<F>;
	const int c0 = T::kFull ? x0 : x0 / 2;
	const int cn = T::kFull ? n : n / 2;
	std::uint8_t *rowY = dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride;
	if constexpr (F == kY210) {  // (the low 6 bits of every word: 0)
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			unsigned w[8];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const int c = 4 * q + i;
				w[2 * i] = static_cast<unsigned>(ys[2 * c] << T::kShift) | (static_cast<unsigned>(cu[c] << T::kShift) << 16);
				w[2 * i + 1] = static_cast<unsigned>(ys[2 * c + 1] << T::kShift) | (static_cast<unsigned>(cv[c] << T::kShift) << 16);
			}
			storeSamples<16>(rowY, 2 * x0 + 16 * q, 2 * n - 16 * q, full, w);
		}
		return;
	}
	if constexpr (F == kY410) {  // (bits 30-31: 0)
		unsigned w[16];
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			w[p] = static_cast<unsigned>(cu[p]) | (static_cast<unsigned>(ys[p]) << 10) | (static_cast<unsigned>(cv[p]) << 20);
		}
		storeRun<4, 16>(rowY, x0, n, full, w);
		return;
	}
	if constexpr (T::kPacked) {
		constexpr int yb = T::kYByte, cb = 1 - T::kYByte;
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			unsigned w[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const int c = 4 * q + i;
				w[i] = (static_cast<unsigned>(ys[2 * c]) << (8 * yb)) | (static_cast<unsigned>(ys[2 * c + 1]) << (8 * yb + 16)) |
				       (static_cast<unsigned>(cu[c]) << (8 * cb)) | (static_cast<unsigned>(cv[c]) << (8 * cb + 16));
			}
			storeBytes<16>(rowY, 2 * x0 + 16 * q, 2 * n - 16 * q, full, w);
		}
		return;
	}
	constexpr int N = T::kFull ? 16 : 8;
	if constexpr (T::kDeep) {
		unsigned yw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
		for (int p = 0; p < 16; ++p) yw[p >> 1] |= static_cast<unsigned>(ys[p] << T::kShift) << (16 * (p & 1));
		storeSamples<16>(rowY, x0, n, full, yw);
		std::uint8_t *rowU = dst.u + static_cast<std::ptrdiff_t>(y) * dst.uStride;
		if constexpr (T::kSemi) {
			unsigned w[8];
#pragma unroll
			for (int i = 0; i < 8; ++i) {  // U_i V_i
				w[i] = static_cast<unsigned>(cu[i] << T::kShift) | (static_cast<unsigned>(cv[i] << T::kShift) << 16);
			}
			storeSamples<16>(rowU, 2 * c0, 2 * cn, full, w);
		} else {
			unsigned uw[N / 2], vw[N / 2];
#pragma unroll
			for (int i = 0; i < N / 2; ++i) {
				uw[i] = static_cast<unsigned>(cu[2 * i]) | (static_cast<unsigned>(cu[2 * i + 1]) << 16);
				vw[i] = static_cast<unsigned>(cv[2 * i]) | (static_cast<unsigned>(cv[2 * i + 1]) << 16);
			}
			storeSamples<N>(rowU, c0, cn, full, uw);
			storeSamples<N>(dst.v + static_cast<std::ptrdiff_t>(y) * dst.vStride, c0, cn, full, vw);
		}
	} else {
		unsigned yw[4] = {0, 0, 0, 0}, uw[N / 4], vw[N / 4];
#pragma unroll
		for (int p = 0; p < 16; ++p) yw[p >> 2] |= static_cast<unsigned>(ys[p]) << (8 * (p & 3));
#pragma unroll
		for (int i = 0; i < N / 4; ++i) {
			uw[i] = static_cast<unsigned>(cu[4 * i]) | (static_cast<unsigned>(cu[4 * i + 1]) << 8) |
			        (static_cast<unsigned>(cu[4 * i + 2]) << 16) | (static_cast<unsigned>(cu[4 * i + 3]) << 24);
			vw[i] = static_cast<unsigned>(cv[4 * i]) | (static_cast<unsigned>(cv[4 * i + 1]) << 8) |
			        (static_cast<unsigned>(cv[4 * i + 2]) << 16) | (static_cast<unsigned>(cv[4 * i + 3]) << 24);
		}
		storeBytes<16>(rowY, x0, n, full, yw);
		storeBytes<N>(dst.u + static_cast<std::ptrdiff_t>(y) * dst.uStride, c0, cn, full, uw);
		storeBytes<N>(dst.v + static_cast<std::ptrdiff_t>(y) * dst.vStride, c0, cn, full, vw);
	}
}

// BGRX u8 -> the 8-bit formats (YUY2, UYVY, I422, I444).  4:2:2: the [1, 2, 1] sum of a row (4 x the mean), 4:4:4: the
// pixel itself; the rounding constant and the shift follow the sum's weight.
template <int F, int S>
__global__ __launch_bounds__(256) void bgrx_to_yuv_sampled_kernel(const std::uint8_t *__restrict__ src,
    std::ptrdiff_t srcStride, YuvEncode k, YuvPlanes dst, int W, int H) {
	using T = SampledTraits<F>;
	using Sum = ChromaSum<S, false>;
	static_assert(S == kChromaLeft || (S == kChromaCenter && !T::kFull), "4:2:2: left or centre; 4:4:4 has no siting");
	const int strips = (W + kStrip - 1) / kStrip;
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);
	unsigned px[17];  // [0] = column x0 - 1 (clamped), [1 + p] = column x0 + p
	Bgrx8Source{src, srcStride}.load(y, x0, W, full, px);
	int ys[16], cu[16], cv[16];
#pragma unroll
	for (int p = 0; p < 16; ++p) {
		const int B = px[1 + p] & 255, G = (px[1 + p] >> 8) & 255, R = (px[1 + p] >> 16) & 255;
		ys[p] = clamp255(k.oy + ((k.yr * R + k.yg * G + k.yb * B + (1 << 15)) >> 16));
	}
	constexpr int kW = T::kFull ? 0 : Sum::kLog2;  // log2 of the chroma sum's weight
#pragma unroll
	for (int i = 0; i < (T::kFull ? 16 : 8); ++i) {
		int sr, sg, sb;
		if constexpr (T::kFull) {
			sb = px[1 + i] & 255, sg = (px[1 + i] >> 8) & 255, sr = (px[1 + i] >> 16) & 255;
		} else {  // columns 2i - 1, 2i, 2i + 1 of the strip = px[2i], px[2i + 1], px[2i + 2]
			const unsigned a = px[2 * i], b = px[2 * i + 1], c = px[2 * i + 2];
			sb = Sum::across(a & 255, b & 255, c & 255);
			sg = Sum::across((a >> 8) & 255, (b >> 8) & 255, (c >> 8) & 255);
			sr = Sum::across((a >> 16) & 255, (b >> 16) & 255, (c >> 16) & 255);
		}
		cu[i] = clamp255(128 + ((k.ur * sr + k.ug * sg + k.ub * sb + (1 << (15 + kW))) >> (16 + kW)));
		cv[i] = clamp255(128 + ((k.vr * sr + k.vg * sg + k.vb * sb + (1 << (15 + kW))) >> (16 + kW)));
	}
	storeSampledStrip<F>(dst, y, x0, n, full, ys, cu, cv);
}

// P -> the 10-bit formats (P210, I210, I410): the strip body of both sources, as toYuv420p10Strip is for 4:2:0.
template <int F, int S, typename Source>
__device__ inline void toYuvSampled10Strip(const Source &source, const YuvEncode10 &k, const YuvPlanes &dst, int W, int H,
    int idx) {
	using T = SampledTraits<F>;
	using Sum = ChromaSum<S, false>;
	static_assert(S == kChromaLeft || (S == kChromaCenter && !T::kFull), "4:2:2: left or centre; 4:4:4 has no siting");
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);
	typename Source::Pixel px[17];  // [0] = column x0 - 1 (clamped), [1 + p] = column x0 + p
	source.load(y, x0, W, full, px);
	int ys[16], cu[16], cv[16];
#pragma unroll
	for (int p = 0; p < 16; ++p) {
		const long long acc = (static_cast<long long>(k.yr) * Source::r(px[1 + p]) +
		                       static_cast<long long>(k.yg) * Source::g(px[1 + p]) +
		                       static_cast<long long>(k.yb) * Source::b(px[1 + p])) * Source::kScale + (1ll << 31);
		ys[p] = clamp1023(k.oy + static_cast<int>(acc >> 32));
	}
	constexpr int kW = T::kFull ? 0 : Sum::kLog2;  // log2 of the chroma sum's weight
#pragma unroll
	for (int i = 0; i < (T::kFull ? 16 : 8); ++i) {
		int sr, sg, sb;
		if constexpr (T::kFull) {
			sb = Source::b(px[1 + i]), sg = Source::g(px[1 + i]), sr = Source::r(px[1 + i]);
		} else {
			sb = Sum::across(Source::b(px[2 * i]), Source::b(px[2 * i + 1]), Source::b(px[2 * i + 2]));
			sg = Sum::across(Source::g(px[2 * i]), Source::g(px[2 * i + 1]), Source::g(px[2 * i + 2]));
			sr = Sum::across(Source::r(px[2 * i]), Source::r(px[2 * i + 1]), Source::r(px[2 * i + 2]));
		}
		const long long au = (static_cast<long long>(k.ur) * sr + static_cast<long long>(k.ug) * sg +
		                      static_cast<long long>(k.ub) * sb) * Source::kScale + (1ll << (31 + kW));
		const long long av = (static_cast<long long>(k.vr) * sr + static_cast<long long>(k.vg) * sg +
		                      static_cast<long long>(k.vb) * sb) * Source::kScale + (1ll << (31 + kW));
		cu[i] = clamp1023(512 + static_cast<int>(au >> (32 + kW)));
		cv[i] = clamp1023(512 + static_cast<int>(av >> (32 + kW)));
	}
	storeSampledStrip<F>(dst, y, x0, n, full, ys, cu, cv);
}

template <int F, int S>
__global__ __launch_bounds__(256) void state_to_yuv_sampled10_kernel(const f16 *__restrict__ state, YuvEncode10 k,
    YuvPlanes dst, int W, int H) {
	toYuvSampled10Strip<F, S>(StateSource{state}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int F, int S>
__global__ __launch_bounds__(256) void frame16_to_yuv_sampled10_kernel(const std::uint16_t *__restrict__ frame,
    YuvEncode10 k, YuvPlanes dst, int W, int H) {
	toYuvSampled10Strip<F, S>(Bgrx16Source{frame}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int F, int S>
__global__ __launch_bounds__(256) void bgrx_to_yuv_sampled10_kernel(const std::uint8_t *__restrict__ src,
    std::ptrdiff_t srcStride, YuvEncode10 k, YuvPlanes dst, int W, int H) {
	toYuvSampled10Strip<F, S>(Bgrx8Source{src, srcStride}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

// ---- RGB formats: 24-bit, RGBX, planar 8 / 10 / 16 bit, f16, f32 (tests/rgb_reference.py; docs/yuv_io.md, "RGB formats") ----
// The network's BGRX frame in another layout and, for the deep formats, another sample kind; no colour space.  The
// thread shape of the 4:2:2 / 4:4:4 section: 16 pixels of ONE row per thread.  A strip is a run of samples in each plane
// it touches (planar: 16 in each of R, G, B; packed: 48 or 64 in the one plane) that moves as 16-byte accesses where the
// run starts 16-byte aligned, as dwords at 4, else sample by sample -- tested per run, since dense rows of 3-byte pixels
// start at every alignment.  F is the frame's PixelFormat value.

template <int B>
__device__ inline void putSample(unsigned *w, int k, unsigned v) {  // (into words that start as 0)
	if constexpr (B == 4) w[k] = v;
	else if constexpr (B == 2) w[k >> 1] |= v << (16 * (k & 1));
	else w[k >> 2] |= v << (8 * (k & 3));
}

template <int B>
__device__ inline unsigned loadSample(const std::uint8_t *p) {
	if constexpr (B == 4) return *reinterpret_cast<const unsigned *>(p);
	else if constexpr (B == 2) return *reinterpret_cast<const std::uint16_t *>(p);
	else return *p;
}

// `N` samples of `B` bytes of one row from sample `first` on, little-endian in words.  `fast`: all in range -- 16-byte
// loads where the run starts 16-byte aligned, dwords at 4, else sample by sample from the one address; not `fast`: sample
// by sample in groups of `G` (a packed pixel; `first` a multiple of G), the group's index clamped to `lastGroup`
template <int B, int N, int G>
__device__ inline void loadRun(const std::uint8_t *row, int first, int lastGroup, bool fast, unsigned (&w)[N * B / 4]) {
	constexpr int kWords = N * B / 4;
	static_assert(kWords % 4 == 0 && N % G == 0, "a run is whole 16-byte groups and whole pixels");
	const std::uint8_t *p = row + static_cast<std::ptrdiff_t>(first) * B;
	if (fast && alignedTo(p, 16)) {
#pragma unroll
		for (int q = 0; q < kWords / 4; ++q) {
			const u32x4 v = reinterpret_cast<const u32x4 *>(p)[q];
			w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
		}
		return;
	}
	if (fast && alignedTo(p, 4)) {
#pragma unroll
		for (int q = 0; q < kWords; ++q) w[q] = reinterpret_cast<const unsigned *>(p)[q];
		return;
	}
#pragma unroll
	for (int q = 0; q < kWords; ++q) w[q] = 0;
	if (fast) {
#pragma unroll
		for (int k = 0; k < N; ++k) putSample<B>(w, k, loadSample<B>(p + k * B));
		return;
	}
#pragma unroll
	for (int g = 0; g < N / G; ++g) {
		const std::uint8_t *pg = row + static_cast<std::ptrdiff_t>(min(first / G + g, lastGroup)) * (G * B);
#pragma unroll
		for (int i = 0; i < G; ++i) putSample<B>(w, g * G + i, loadSample<B>(pg + i * B));
	}
}

template <int B>
__device__ inline unsigned sampleAt(const unsigned *w, int k) {
	if constexpr (B == 4) return w[k];
	else if constexpr (B == 2) return static_cast<unsigned>(sampleOf(w, k));
	else return static_cast<unsigned>(byteOf(w, k));
}

// `N` samples of `B` bytes of one row from sample `first` on; `fast`: all in range (else only the first `n`)
template <int B, int N>
__device__ inline void storeRun(std::uint8_t *row, int first, int n, bool fast, const unsigned (&w)[N * B / 4]) {
	constexpr int kWords = N * B / 4;
	std::uint8_t *p = row + static_cast<std::ptrdiff_t>(first) * B;
	if (fast && alignedTo(p, 16)) {
#pragma unroll
		for (int q = 0; q < kWords / 4; ++q) {
			const u32x4 v = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
			reinterpret_cast<u32x4 *>(p)[q] = v;
		}
		return;
	}
	if (fast && alignedTo(p, 4)) {
#pragma unroll
		for (int q = 0; q < kWords; ++q) reinterpret_cast<unsigned *>(p)[q] = w[q];
		return;
	}
#pragma unroll
	for (int k = 0; k < N; ++k) {
		if (fast || k < n) {
			if constexpr (B == 4) reinterpret_cast<unsigned *>(p)[k] = w[k];
			else if constexpr (B == 2) reinterpret_cast<std::uint16_t *>(p)[k] = static_cast<std::uint16_t>(sampleOf(w, k));
			else p[k] = static_cast<std::uint8_t>(byteOf(w, k));
		}
	}
}

template <int F>
struct RgbTraits {
	static constexpr bool kPlanar = F >= kRgbp8 && F <= kRgbps;  // planes R, G, B; else ONE plane of kPixel samples a pixel
	static constexpr int kPixel = kPlanar ? 1 : ((F == kRgbx || F == kBgrx64) ? 4 : 3);
	static constexpr int kB = (F == kRgb24 || F == kRgbx) ? 2 : 0, kG = 1, kR = 2 - kB;  // a packed pixel's samples
	// X2RGB10 / X2BGR10: ONE dword per pixel holding the three 10-bit samples from bits kBShift, 10 and 20 - kBShift on
	static constexpr bool kWord10 = F == kX2rgb10 || F == kX2bgr10;
	static constexpr int kBShift = F == kX2rgb10 ? 0 : 20;
	static constexpr int kKind = (F == kBgrx64 || F == kRgbp16) ? kW16
	    : (F == kRgbp10 || kWord10) ? kW10 : F == kRgbph ? kHalf : F == kRgbps ? kUnit : F == kBgr96f ? kF255 : kU8;
	static constexpr int kBytes = kKind == kU8 ? 1 : ((kKind == kUnit || kKind == kF255) ? 4 : 2);
};

// floor(clamp(v, 0, top) scale + 0.5) with the product rounded to f32 BEFORE the sum (no fused multiply-add: the
// definition is a multiply followed by an add); NaN -> 0, +-inf clamp
__device__ inline unsigned roundedU8(float v, float top, float scale) {
#pragma clang fp contract(off)
	v = v >= 0.0f ? v : 0.0f;  // (false for NaN)
	v = v > top ? top : v;
	const float scaled = v * scale;
	return static_cast<unsigned>(floorf(scaled + 0.5f));
}

// one sample of kind K (its bits) -> the u8 the network consumes
template <int K>
__device__ inline unsigned u8OfSample(unsigned s) {
	if constexpr (K == kW16) return (s + 128) / 257;
	else if constexpr (K == kW10) {
		const unsigned p = s & 0x3ff;
		return (((p << 6) | (p >> 4)) + 128) / 257;
	} else if constexpr (K == kHalf) {
		return roundedU8(static_cast<float>(__builtin_bit_cast(f16, static_cast<unsigned short>(s))), 1.0f, 255.0f);
	} else if constexpr (K == kUnit) return roundedU8(__builtin_bit_cast(float, s), 1.0f, 255.0f);
	else if constexpr (K == kF255) return roundedU8(__builtin_bit_cast(float, s), 255.0f, 1.0f);
	else return s;
}

// planes -> BGRX: the strip of thread `idx`; the body of the single-frame kernel and of the items kernel's branch
template <int F>
__device__ __forceinline__ void rgbToBgrxStrip(const YuvPlanes &src, std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride,
    int W, int H, int idx) {
	using T = RgbTraits<F>;
	constexpr int B = T::kBytes, K = T::kKind;
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);
	std::uint8_t *out = dst + static_cast<std::ptrdiff_t>(y) * dstStride;
	if constexpr (T::kWord10) {
		unsigned w[16];
		loadRun<4, 16, 1>(src.y + static_cast<std::ptrdiff_t>(y) * src.yStride, x0, W - 1, full, w);
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			unsigned px[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) {  // (u8OfSample reads the low 10 bits: bits 30-31 are ignored)
				const unsigned v = w[4 * q + i];
				px[i] = u8OfSample<K>(v >> T::kBShift) | (u8OfSample<K>(v >> 10) << 8) | (u8OfSample<K>(v >> (20 - T::kBShift)) << 16);
			}
			storeBytes<16>(out, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, px);
		}
	} else if constexpr (T::kPlanar) {
		unsigned wr[4 * B], wg[4 * B], wb[4 * B];
		loadRun<B, 16, 1>(src.y + static_cast<std::ptrdiff_t>(y) * src.yStride, x0, W - 1, full, wr);
		loadRun<B, 16, 1>(src.u + static_cast<std::ptrdiff_t>(y) * src.uStride, x0, W - 1, full, wg);
		loadRun<B, 16, 1>(src.v + static_cast<std::ptrdiff_t>(y) * src.vStride, x0, W - 1, full, wb);
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			unsigned px[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const int p = 4 * q + i;
				px[i] = u8OfSample<K>(sampleAt<B>(wb, p)) | (u8OfSample<K>(sampleAt<B>(wg, p)) << 8) |
				        (u8OfSample<K>(sampleAt<B>(wr, p)) << 16);
			}
			storeBytes<16>(out, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, px);
		}
	} else {
		// in runs of C pixels, the fewest whose bytes are whole 16-byte groups (BGR24 / RGB24: all 16, 48 B; else 4); four
		// pixels are 16 bytes of BGRX, stored as they are formed
		constexpr int P = T::kPixel, C = (4 * P * B) % 16 == 0 ? 4 : 16;
		const std::uint8_t *row = src.y + static_cast<std::ptrdiff_t>(y) * src.yStride;
#pragma unroll
		for (int c = 0; c < 16 / C; ++c) {
			unsigned w[C * P * B / 4];
			loadRun<B, C * P, P>(row, (x0 + c * C) * P, W - 1, full, w);
#pragma unroll
			for (int q = 0; q < C / 4; ++q) {
				unsigned px[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int p = 4 * q + i;
					px[i] = u8OfSample<K>(sampleAt<B>(w, p * P + T::kB)) | (u8OfSample<K>(sampleAt<B>(w, p * P + T::kG)) << 8) |
					        (u8OfSample<K>(sampleAt<B>(w, p * P + T::kR)) << 16);
				}
				const int x = c * C + 4 * q;  // (first pixel of the four, within the strip)
				storeBytes<16>(out, 4 * (x0 + x), 4 * (n - x), full, px);
			}
		}
	}
}

template <int F>
__global__ __launch_bounds__(256) void rgb_to_bgrx_kernel(YuvPlanes src, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H) {
	rgbToBgrxStrip<F>(src, dst, dstStride, W, H, blockIdx.x * 256 + threadIdx.x);
}

// source -> the planes of format F: the strip body of both encodes.  The X samples of RGBX / BGRX64 are written 0.
template <int F, typename Source>
__device__ inline void toRgbStrip(const Source &source, const YuvPlanes &dst, int W, int H, int idx) {
	using T = RgbTraits<F>;
	constexpr int B = T::kBytes, K = T::kKind;
	const int strips = (W + kStrip - 1) / kStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kStrip;
	const bool full = x0 + kStrip <= W;
	const int n = min(kStrip, W - x0);
	typename Source::Raw px[16];
	source.loadRaw(y, x0, W, full, px);
	if constexpr (T::kWord10) {  // (bits 30-31: 0)
		unsigned w[16];
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			w[p] = (Source::template deep<K>(Source::rawB(px[p])) << T::kBShift) | (Source::template deep<K>(Source::rawG(px[p])) << 10) |
			       (Source::template deep<K>(Source::rawR(px[p])) << (20 - T::kBShift));
		}
		storeRun<4, 16>(dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride, x0, n, full, w);
	} else if constexpr (T::kPlanar) {
		unsigned wr[4 * B], wg[4 * B], wb[4 * B];
#pragma unroll
		for (int q = 0; q < 4 * B; ++q) wr[q] = wg[q] = wb[q] = 0;
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			putSample<B>(wr, p, Source::template deep<K>(Source::rawR(px[p])));
			putSample<B>(wg, p, Source::template deep<K>(Source::rawG(px[p])));
			putSample<B>(wb, p, Source::template deep<K>(Source::rawB(px[p])));
		}
		storeRun<B, 16>(dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride, x0, n, full, wr);
		storeRun<B, 16>(dst.u + static_cast<std::ptrdiff_t>(y) * dst.uStride, x0, n, full, wg);
		storeRun<B, 16>(dst.v + static_cast<std::ptrdiff_t>(y) * dst.vStride, x0, n, full, wb);
	} else {
		constexpr int P = T::kPixel;
		unsigned w[4 * P * B];
#pragma unroll
		for (int q = 0; q < 4 * P * B; ++q) w[q] = 0;
#pragma unroll
		for (int p = 0; p < 16; ++p) {
			putSample<B>(w, p * P + T::kB, Source::template deep<K>(Source::rawB(px[p])));
			putSample<B>(w, p * P + T::kG, Source::template deep<K>(Source::rawG(px[p])));
			putSample<B>(w, p * P + T::kR, Source::template deep<K>(Source::rawR(px[p])));
		}
		storeRun<B, 16 * P>(dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride, x0 * P, n * P, full, w);
	}
}

template <int F>
__global__ __launch_bounds__(256) void bgrx_to_rgb_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    YuvPlanes dst, int W, int H) {
	toRgbStrip<F>(Bgrx8Source{src, srcStride}, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int F>
__global__ __launch_bounds__(256) void state_to_rgb_kernel(const f16 *__restrict__ state, YuvPlanes dst, int W, int H) {
	toRgbStrip<F>(StateSource{state}, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int F>
__global__ __launch_bounds__(256) void frame16_to_rgb_kernel(const std::uint16_t *__restrict__ frame, YuvPlanes dst, int W,
    int H) {
	toRgbStrip<F>(Bgrx16Source{frame}, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

// ---- V210: 10-bit 4:2:2, six pixels in four dwords (tests/packed10_reference.py; docs/yuv_io.md, "Packed 10-bit") -------
// A group of six pixels is 16 bytes: w0 = Cb0 Y0 Cr0, w1 = Y1 Cb1 Y2, w2 = Cr1 Y3 Cb2, w3 = Y4 Cr2 Y5, three 10-bit samples a
// dword from bit 0 on, bits 30-31 unused.  A thread owns TWO whole groups of one row (12 pixels), so that no group is
// shared between threads; a row is whole groups (its last one padded with unused sample slots: ignored in, 0 out), and
// the plane is only 4-byte aligned, so a group moves as one 16-byte access where it lies so and as four dwords elsewhere.
// The samples, the arithmetic and the sample P are P210's (the 4:2:2 section above).
constexpr int kGroupStrip = 12;  // luma pixels per thread and row

__device__ inline void loadGroup(const std::uint8_t *p, unsigned *w) {
	if (alignedTo(p, 16)) {
		const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
		w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
	} else {
#pragma unroll
		for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const unsigned *>(p)[q];
	}
}

__device__ inline void storeGroup(std::uint8_t *p, const unsigned *w) {
	if (alignedTo(p, 16)) {
		const u32x4 v = {w[0], w[1], w[2], w[3]};
		*reinterpret_cast<u32x4 *>(p) = v;
	} else {
#pragma unroll
		for (int q = 0; q < 4; ++q) reinterpret_cast<unsigned *>(p)[q] = w[q];
	}
}

// the plane -> BGRX: the strip of thread `idx`; the body of the single-frame kernel and of the items kernel's branch.
// Chroma cell c0 + 6, the right-hand neighbour of the strip's last odd column, is the first of the NEXT thread's groups;
// cells beyond W / 2 - 1 -- that one in a row's last strip, and the unused slots of a partial group -- take the last cell's.
template <int S>
__device__ inline void v210ToBgrxStrip(const YuvPlanes &src, const YuvDecode &k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H, int idx) {
	static_assert(S == kChromaLeft || S == kChromaCenter, "4:2:2: left or centre");
	constexpr int kLog2 = S == kChromaCenter ? 2 : 3;  // log2 of the scale of the chroma at the pixel
	const int strips = (W + kGroupStrip - 1) / kGroupStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kGroupStrip;
	const int groups = (W + 5) / 6, g0 = x0 / 6, CW = W / 2, c0 = x0 / 2;
	const bool full = x0 + kGroupStrip <= W;
	const std::uint8_t *row = src.y + static_cast<std::ptrdiff_t>(y) * src.yStride;
	unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	loadGroup(row + 16 * g0, w);
	if (g0 + 1 < groups) loadGroup(row + 16 * (g0 + 1), w + 4);
	int ys[12], cu[7], cv[7];
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		const unsigned *q = w + 4 * g;
		cu[3 * g] = q[0] & 0x3ff, ys[6 * g] = (q[0] >> 10) & 0x3ff, cv[3 * g] = (q[0] >> 20) & 0x3ff;
		ys[6 * g + 1] = q[1] & 0x3ff, cu[3 * g + 1] = (q[1] >> 10) & 0x3ff, ys[6 * g + 2] = (q[1] >> 20) & 0x3ff;
		cv[3 * g + 1] = q[2] & 0x3ff, ys[6 * g + 3] = (q[2] >> 10) & 0x3ff, cu[3 * g + 2] = (q[2] >> 20) & 0x3ff;
		ys[6 * g + 4] = q[3] & 0x3ff, cv[3 * g + 2] = (q[3] >> 10) & 0x3ff, ys[6 * g + 5] = (q[3] >> 20) & 0x3ff;
	}
	int beforeU = cu[0], beforeV = cv[0];  // (centre: cell c0 - 1, the last of the group to the left; clamped to cell 0)
	if constexpr (S == kChromaCenter) {
		if (g0 > 0) {
			const uint2 prev = make_uint2(*reinterpret_cast<const unsigned *>(row + 16 * g0 - 8),
			    *reinterpret_cast<const unsigned *>(row + 16 * g0 - 4));
			beforeU = (prev.x >> 20) & 0x3ff, beforeV = (prev.y >> 10) & 0x3ff;
		}
	}
	cu[6] = cv[6] = 0;
	if (g0 + 2 < groups) {  // (a group that exists begins with a cell that exists)
		const unsigned next = *reinterpret_cast<const unsigned *>(row + 16 * (g0 + 2));
		cu[6] = next & 0x3ff, cv[6] = (next >> 20) & 0x3ff;
	}
#pragma unroll
	for (int i = 1; i < 7; ++i) {
		if (c0 + i >= CW) cu[i] = cu[i - 1], cv[i] = cv[i - 1];
	}
	unsigned px[kGroupStrip];
#pragma unroll
	for (int p = 0; p < kGroupStrip; ++p) {
		// 2^kLog2 x chroma at the pixel, less 2^kLog2 x the mid value
		const int du = chromaAt422<S>(cu, beforeU, p) - (512 << kLog2);
		const int dv = chromaAt422<S>(cv, beforeV, p) - (512 << kLog2);
		const int yd = k.ky * ((1 << kLog2) * (ys[p] - k.oy));
		const int R = clamp255((yd + k.krv * dv + (1 << (15 + kLog2))) >> (16 + kLog2));
		const int G = clamp255((yd - k.kgu * du - k.kgv * dv + (1 << (15 + kLog2))) >> (16 + kLog2));
		const int B = clamp255((yd + k.kbu * du + (1 << (15 + kLog2))) >> (16 + kLog2));
		px[p] = static_cast<unsigned>(B) | (static_cast<unsigned>(G) << 8) | (static_cast<unsigned>(R) << 16);
	}
	std::uint8_t *out = dst + static_cast<std::ptrdiff_t>(y) * dstStride;
	const int n = min(kGroupStrip, W - x0);
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		const unsigned v[4] = {px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]};
		storeBytes<16>(out, 4 * (x0 + 4 * q), 4 * (n - 4 * q), full, v);
	}
}

template <int S>
__global__ __launch_bounds__(256) void v210_to_bgrx_kernel(YuvPlanes src, YuvDecode k, std::uint8_t *__restrict__ dst,
    std::ptrdiff_t dstStride, int W, int H) {
	v210ToBgrxStrip<S>(src, k, dst, dstStride, W, H, blockIdx.x * 256 + threadIdx.x);
}

// P -> the plane: the strip body of the three encodes.  The source's load covers columns x0 - 1 (clamped to 0: the
// left-hand neighbour of the [1, 2, 1] sum) and x0 .. x0 + 15 (clamped to W - 1), of which the strip uses the first 12; its
// wide path needs all 16 in range.  Sample slots beyond W are written 0, and a group is written whole.
template <int S, typename Source>
__device__ inline void toV210Strip(const Source &source, const YuvEncode10 &k, const YuvPlanes &dst, int W, int H, int idx) {
	using Sum = ChromaSum<S, false>;
	static_assert(S == kChromaLeft || S == kChromaCenter, "4:2:2: left or centre");
	const int strips = (W + kGroupStrip - 1) / kGroupStrip;
	if (idx >= strips * H) return;
	const int y = idx / strips;
	const int x0 = (idx - y * strips) * kGroupStrip;
	const int groups = (W + 5) / 6, g0 = x0 / 6, CW = W / 2, c0 = x0 / 2;
	typename Source::Pixel px[17];  // [0] = column x0 - 1 (clamped), [1 + p] = column x0 + p
	source.load(y, x0, W, x0 + kStrip <= W, px);
	unsigned ys[12], cu[6], cv[6];
#pragma unroll
	for (int p = 0; p < 12; ++p) {
		const long long acc = (static_cast<long long>(k.yr) * Source::r(px[1 + p]) +
		                       static_cast<long long>(k.yg) * Source::g(px[1 + p]) +
		                       static_cast<long long>(k.yb) * Source::b(px[1 + p])) * Source::kScale + (1ll << 31);
		ys[p] = x0 + p < W ? static_cast<unsigned>(clamp1023(k.oy + static_cast<int>(acc >> 32))) : 0u;
	}
#pragma unroll
	for (int i = 0; i < 6; ++i) {
		const int sb = Sum::acrossOf([&](int q) { return Source::b(px[q]); }, 2 * i);
		const int sg = Sum::acrossOf([&](int q) { return Source::g(px[q]); }, 2 * i);
		const int sr = Sum::acrossOf([&](int q) { return Source::r(px[q]); }, 2 * i);
		const long long au = (static_cast<long long>(k.ur) * sr + static_cast<long long>(k.ug) * sg +
		                      static_cast<long long>(k.ub) * sb) * Source::kScale + (1ll << (31 + Sum::kLog2));
		const long long av = (static_cast<long long>(k.vr) * sr + static_cast<long long>(k.vg) * sg +
		                      static_cast<long long>(k.vb) * sb) * Source::kScale + (1ll << (31 + Sum::kLog2));
		cu[i] = c0 + i < CW ? static_cast<unsigned>(clamp1023(512 + static_cast<int>(au >> (32 + Sum::kLog2)))) : 0u;
		cv[i] = c0 + i < CW ? static_cast<unsigned>(clamp1023(512 + static_cast<int>(av >> (32 + Sum::kLog2)))) : 0u;
	}
	std::uint8_t *row = dst.y + static_cast<std::ptrdiff_t>(y) * dst.yStride;
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		if (g0 + g >= groups) break;
		const unsigned w[4] = {cu[3 * g] | (ys[6 * g] << 10) | (cv[3 * g] << 20),
		    ys[6 * g + 1] | (cu[3 * g + 1] << 10) | (ys[6 * g + 2] << 20),
		    cv[3 * g + 1] | (ys[6 * g + 3] << 10) | (cu[3 * g + 2] << 20),
		    ys[6 * g + 4] | (cv[3 * g + 2] << 10) | (ys[6 * g + 5] << 20)};
		storeGroup(row + 16 * (g0 + g), w);
	}
}

template <int S>
__global__ __launch_bounds__(256) void bgrx_to_v210_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    YuvEncode10 k, YuvPlanes dst, int W, int H) {
	toV210Strip<S>(Bgrx8Source{src, srcStride}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int S>
__global__ __launch_bounds__(256) void state_to_v210_kernel(const f16 *__restrict__ state, YuvEncode10 k, YuvPlanes dst, int W,
    int H) {
	toV210Strip<S>(StateSource{state}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

template <int S>
__global__ __launch_bounds__(256) void frame16_to_v210_kernel(const std::uint16_t *__restrict__ frame, YuvEncode10 k,
    YuvPlanes dst, int W, int H) {
	toV210Strip<S>(Bgrx16Source{frame}, k, dst, W, H, blockIdx.x * 256 + threadIdx.x);
}

// The formats each kernel family instantiates, ONE list per family: the launchers below and the items kernel reach a
// format's kernel or strip body through forFormat alone.  4:2:0: <NV12> / <P010> = the list's second format; the encodes of
// the other two families pick the 8-bit or the deep kernel from the format's traits.
template <int... Fs>
struct Formats {};
using Yuv420 = Formats<kI420, kNv12>;
using Yuv420p10 = Formats<kI010, kP010>;
using Sampled = Formats<kYuy2, kUyvy, kI422, kP210, kI210, kI444, kI410, kY210, kY410>;
using Grouped = Formats<kV210>;
using Rgb = Formats<kBgr24, kRgb24, kRgbx, kBgrx64, kRgbp8, kRgbp10, kRgbp16, kRgbph, kRgbps, kBgr96f, kX2rgb10, kX2bgr10>;
// (the sitings a family's bodies are instantiated for, dispatched the same way on the frame's effectiveSiting)
using Sitings420 = Formats<kChromaLeft, kChromaCenter, kChromaTopLeft>;
using Sitings422 = Formats<kChromaLeft, kChromaCenter>;
// fn(std::integral_constant<int, F>, args...) for the F of the list that equals `format`; false: the list has no such format
template <int... Fs, typename Fn, typename... A>
__host__ __device__ inline bool forFormat(Formats<Fs...>, int format, Fn &&fn, const A &...args) {
	return ((format == Fs && (fn(std::integral_constant<int, Fs>{}, args...), true)) || ...);
}
// fn(std::integral_constant<int, S>) for the siting S of a format of the Sampled list: 4:4:4 has the one body
template <int F, typename Fn>
inline void forSampledSiting(int siting, Fn &&fn) {
	if constexpr (SampledTraits<F>::kFull) fn(std::integral_constant<int, kChromaLeft>{});
	else (void)forFormat(Sitings422{}, siting, fn);
}

// The inputs of a look-ahead pass in ONE launch: grid (blocks of one frame, items), blockIdx.y selects the item -- its
// format, planes, coefficients and destination, from the kernel arguments -- and the format is a branch every lane of the
// workgroup takes alike, and so is the item's siting, one level below.  At 480x270 one frame is 16 workgroups on 256 CUs: eight launches of that size would be eight
// launch latencies for one round of work (the shape addFlowAutoencoder's batched launches fixed for the flow net).
// (a 4:2:2 / 4:4:4 or RGB item has a strip per row: the grid then covers strips x H threads and a 4:2:0 item's upper half
// of them returns at once; an RGB item's coefficients are not read)
__device__ __forceinline__ void decodeItemStrip(const YuvDecodeItem &it, int W, int H, int idx) {
	// (captureless lambdas over the kernel's own COPY of the item: 96 bytes of scalar registers.  Through a reference into the
	// by-value argument the two levels of dispatch made the compiler keep all eight items in scratch)
	using Item = const YuvDecodeItem &;
	(void)(forFormat(Yuv420{}, it.format, [](auto f, Item it, int W, int H, int idx) {
		       (void)forFormat(Sitings420{}, it.siting, [](auto s, auto f, Item it, int W, int H, int idx) {
			       yuv420ToBgrxStrip<f() == kNv12, s()>(it.src, it.k, it.dst, it.dstStride, W, H, idx);
		       }, f, it, W, H, idx);
	       }, it, W, H, idx) ||
	       forFormat(Yuv420p10{}, it.format, [](auto f, Item it, int W, int H, int idx) {
		       (void)forFormat(Sitings420{}, it.siting, [](auto s, auto f, Item it, int W, int H, int idx) {
			       yuv420p10ToBgrxStrip<f() == kP010, s()>(it.src, it.k, it.dst, it.dstStride, W, H, idx);
		       }, f, it, W, H, idx);
	       }, it, W, H, idx) ||
	       forFormat(Sampled{}, it.format, [](auto f, Item it, int W, int H, int idx) {
		       if constexpr (SampledTraits<f()>::kFull) {
			       yuvSampledToBgrxStrip<f(), kChromaLeft>(it.src, it.k, it.dst, it.dstStride, W, H, idx);
		       } else {
			       (void)forFormat(Sitings422{}, it.siting, [](auto s, auto f, Item it, int W, int H, int idx) {
				       yuvSampledToBgrxStrip<f(), s()>(it.src, it.k, it.dst, it.dstStride, W, H, idx);
			       }, f, it, W, H, idx);
		       }
	       }, it, W, H, idx) ||
	       forFormat(Grouped{}, it.format, [](auto, Item it, int W, int H, int idx) {
		       (void)forFormat(Sitings422{}, it.siting, [](auto s, Item it, int W, int H, int idx) {
			       v210ToBgrxStrip<s()>(it.src, it.k, it.dst, it.dstStride, W, H, idx);
		       }, it, W, H, idx);
	       }, it, W, H, idx) ||
	       forFormat(Rgb{}, it.format, [](auto f, Item it, int W, int H, int idx) {
		       rgbToBgrxStrip<f()>(it.src, it.dst, it.dstStride, W, H, idx);
	       }, it, W, H, idx));
}

__global__ __launch_bounds__(256) void yuv420_to_bgrx_items_kernel(YuvDecodeItems items, int W, int H) {
	const YuvDecodeItem it = items.item[blockIdx.y];
	decodeItemStrip(it, W, H, blockIdx.x * 256 + threadIdx.x);
}

// The sized form (launchYuvToBgrxItemsSized: the members of a group pass): item blockIdx.y at its OWN width and height, read
// with the item from the kernel arguments.  The grid covers the largest item's strips; every strip body returns beyond its
// own frame's count, as the upper half of a 4:2:0 item's grid does above.  The strip bodies are the ones above.
__global__ __launch_bounds__(256) void yuv_to_bgrx_items_sized_kernel(YuvDecodeSizedItems items) {
	const YuvDecodeItem it = items.item[blockIdx.y];
	decodeItemStrip(it, items.width[blockIdx.y], items.height[blockIdx.y], blockIdx.x * 256 + threadIdx.x);
}

int roundHalfAway(double x) { return static_cast<int>(std::copysign(std::floor(std::fabs(x) * 65536.0 + 0.5), x)); }

// K_r, K_b and the range of a frame's `colorspace` (its matrix: BT.601, BT.709, BT.2020 non-constant luminance)
void colourSpace(int colorspace, double *kr, double *kb, bool *limited) {
	const int matrix = splitColourSpace(colorspace).matrix;
	*kr = matrix < 2 ? 0.299 : (matrix < 4 ? 0.2126 : 0.2627);
	*kb = matrix < 2 ? 0.114 : (matrix < 4 ? 0.0722 : 0.0593);
	*limited = matrix % 2 == 0;
}

// the siting of a frame's `colorspace` that the format's kernels distinguish
int sitingOf(const YuvFormatInfo &info, int colorspace) {
	return info.rgb() ? kChromaLeft : effectiveSiting(info, splitColourSpace(colorspace).siting);
}

// x 65536 for 8-bit samples, or for 10-bit words -> u8 (oy 64 | 0); an RGB format has none and its colour space is not read
YuvDecode decodeCoefficients(const YuvFormatInfo &info, int colorspace) {
	if (info.rgb()) return YuvDecode{};
	double kr, kb;
	bool limited;
	colourSpace(colorspace, &kr, &kb, &limited);
	const double kg = 1.0 - kr - kb;
	const bool words = info.words10();
	const double s = words ? (limited ? 255.0 / 896.0 : 255.0 / 1023.0) : (limited ? 255.0 / 224.0 : 1.0);
	YuvDecode k;
	k.ky = roundHalfAway(words ? (limited ? 255.0 / 876.0 : 255.0 / 1023.0) : (limited ? 255.0 / 219.0 : 1.0));
	k.krv = roundHalfAway(2 * (1 - kr) * s);
	k.kbu = roundHalfAway(2 * (1 - kb) * s);
	k.kgu = roundHalfAway(2 * kb * (1 - kb) / kg * s);
	k.kgv = roundHalfAway(2 * kr * (1 - kr) / kg * s);
	k.oy = limited ? (words ? 64 : 16) : 0;
	return k;
}

YuvEncode encodeCoefficients(int colorspace) {
	double kr, kb;
	bool limited;
	colourSpace(colorspace, &kr, &kb, &limited);
	const double kg = 1.0 - kr - kb;
	const double sy = limited ? 219.0 / 255.0 : 1.0, sc = limited ? 224.0 / 255.0 : 1.0;
	const double du = sc / (2 * (1 - kb)), dv = sc / (2 * (1 - kr));
	YuvEncode k;
	k.yr = roundHalfAway(sy * kr);
	k.yg = roundHalfAway(sy * kg);
	k.yb = roundHalfAway(sy * kb);
	k.ur = roundHalfAway(-kr * du);
	k.ug = roundHalfAway(-kg * du);
	k.ub = roundHalfAway((1 - kb) * du);
	k.vr = roundHalfAway((1 - kr) * dv);
	k.vg = roundHalfAway(-kg * dv);
	k.vb = roundHalfAway(-kb * dv);
	k.oy = limited ? 16 : 0;
	return k;
}

YuvEncode10 encodeCoefficients10(int colorspace) {
	double kr, kb;
	bool limited;
	colourSpace(colorspace, &kr, &kb, &limited);
	const double kg = 1.0 - kr - kb;
	const double sy = limited ? 876.0 : 1023.0, sc = limited ? 896.0 : 1023.0;
	const double du = sc / (2 * (1 - kb)), dv = sc / (2 * (1 - kr));
	// x 2^32 / 65535 (the 16-bit sample's full scale), rounded half away from zero: each below 2^26
	auto c = [](double x) {
		return static_cast<int>(std::copysign(std::floor(std::fabs(x / 65535.0 * 4294967296.0) + 0.5), x));
	};
	YuvEncode10 k;
	k.yr = c(sy * kr);
	k.yg = c(sy * kg);
	k.yb = c(sy * kb);
	k.ur = c(-kr * du);
	k.ug = c(-kg * du);
	k.ub = c((1 - kb) * du);
	k.vr = c((1 - kr) * dv);
	k.vg = c(-kg * dv);
	k.vb = c(-kb * dv);
	k.oy = limited ? 64 : 0;
	return k;
}

// threads of a frame in a format: one per strip -- 16 pixels (V210: 12, two groups) of a row or, for 4:2:0, of a row pair
std::size_t stripThreads(const YuvFormatInfo &info, int width, int height) {
	const int strip = info.pixelBytes == kGroupedRow ? kGroupStrip : kStrip;
	return static_cast<std::size_t>((width + strip - 1) / strip) * (info.perRow() ? height : height / 2);
}

// One strip kernel over a frame: a thread per strip; every kernel's arguments end in the frame's width and height
struct StripLaunch {
	const YuvFormatInfo &info;
	int width, height;
	hipStream_t stream;
	template <typename... P, typename... A>
	void operator()(const char *name, void (*kernel)(P...), const A &...args) const {
		const dim3 grid(blocksFor(stripThreads(info, width, height)));
		hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, args..., width, height);
		hipCheckLaunch(name);
	}
};

[[noreturn]] void noKernel(const char *what, int format) {
	throw std::invalid_argument(std::string(what) + ": format " + std::to_string(format) + " has no such kernel");
}

}  // namespace

void launchDecodeFrame(int format, int colorspace, const YuvPlanes &src, std::uint8_t *dst, std::ptrdiff_t dstStride,
    int width, int height, hipStream_t stream) {
	const StripLaunch run{formatInfo(format), width, height, stream};
	const YuvDecode k = decodeCoefficients(run.info, colorspace);
	const int siting = sitingOf(run.info, colorspace);
	if (!(forFormat(Yuv420{}, format, [&](auto f) {
		      forFormat(Sitings420{}, siting,
		          [&](auto s) { run("yuv420_to_bgrx", yuv420_to_bgrx_kernel<f() == kNv12, s()>, src, k, dst, dstStride); });
	      }) || forFormat(Yuv420p10{}, format, [&](auto f) {
		      forFormat(Sitings420{}, siting,
		          [&](auto s) { run("yuv420p10_to_bgrx", yuv420p10_to_bgrx_kernel<f() == kP010, s()>, src, k, dst, dstStride); });
	      }) || forFormat(Sampled{}, format, [&](auto f) {
		      forSampledSiting<f()>(siting,
		          [&](auto s) { run("yuv_sampled_to_bgrx", yuv_sampled_to_bgrx_kernel<f(), s()>, src, k, dst, dstStride); });
	      }) || forFormat(Grouped{}, format, [&](auto) {
		      forFormat(Sitings422{}, siting, [&](auto s) { run("v210_to_bgrx", v210_to_bgrx_kernel<s()>, src, k, dst, dstStride); });
	      }) || forFormat(Rgb{}, format, [&](auto f) { run("rgb_to_bgrx", rgb_to_bgrx_kernel<f()>, src, dst, dstStride); }))) {
		noKernel("decode", format);
	}
}

YuvDecodeItem yuvDecodeItem(int format, int colorspace, const YuvPlanes &src, std::uint8_t *dst, std::ptrdiff_t dstStride) {
	YuvDecodeItem it;
	it.src = src;
	it.k = decodeCoefficients(formatInfo(format), colorspace);
	it.dst = dst;
	it.dstStride = dstStride;
	it.format = format;
	it.siting = sitingOf(formatInfo(format), colorspace);
	return it;
}

void launchYuv420ToBgrxItems(const YuvDecodeItems &items, int count, int width, int height, hipStream_t stream) {
	if (count < 1 || count > kFlowBatchMax) throw std::invalid_argument("yuv420_to_bgrx_items: 1 .. 8 items");
	std::size_t threads = 0;  // (the most any item needs; an item's strip body returns beyond its own count)
	for (int i = 0; i < count; ++i) threads = std::max(threads, stripThreads(formatInfo(items.item[i].format), width, height));
	hipLaunchKernelGGL(yuv420_to_bgrx_items_kernel, dim3(blocksFor(threads), count), dim3(256), 0, stream, items, width,
	    height);
	hipCheckLaunch("yuv420_to_bgrx_items");
}

void launchYuvToBgrxItemsSized(const YuvDecodeSizedItems &items, int count, hipStream_t stream) {
	if (count < 1 || count > kFlowBatchMax) throw std::invalid_argument("yuv_to_bgrx_items_sized: 1 .. 8 items");
	std::size_t threads = 0;  // (the most any item needs at its own size)
	for (int i = 0; i < count; ++i) {
		if (items.width[i] < 1 || items.height[i] < 1) throw std::invalid_argument("yuv_to_bgrx_items_sized: a size below 1");
		threads = std::max(threads, stripThreads(formatInfo(items.item[i].format), items.width[i], items.height[i]));
	}
	hipLaunchKernelGGL(yuv_to_bgrx_items_sized_kernel, dim3(blocksFor(threads), count), dim3(256), 0, stream, items);
	hipCheckLaunch("yuv_to_bgrx_items_sized");
}

void launchEncodeFrame(int format, int colorspace, const std::uint8_t *src, std::ptrdiff_t srcStride, const YuvPlanes &dst,
    int width, int height, hipStream_t stream) {
	const StripLaunch run{formatInfo(format), width, height, stream};
	const int siting = sitingOf(run.info, colorspace);
	const bool done = forFormat(Yuv420{}, format, [&](auto f) {
		forFormat(Sitings420{}, siting, [&](auto s) {
			run("bgrx_to_yuv420", bgrx_to_yuv420_kernel<f() == kNv12, s()>, src, srcStride, encodeCoefficients(colorspace), dst);
		});
	}) || forFormat(Yuv420p10{}, format, [&](auto f) {
		forFormat(Sitings420{}, siting, [&](auto s) {
			run("bgrx_to_yuv420p10", bgrx_to_yuv420p10_kernel<f() == kP010, s()>, src, srcStride, encodeCoefficients10(colorspace), dst);
		});
	}) || forFormat(Sampled{}, format, [&](auto f) {
		forSampledSiting<f()>(siting, [&](auto s) {
			if constexpr (SampledTraits<f()>::kDeep) {
				run("bgrx_to_yuv_sampled10", bgrx_to_yuv_sampled10_kernel<f(), s()>, src, srcStride, encodeCoefficients10(colorspace), dst);
			} else {
				run("bgrx_to_yuv_sampled", bgrx_to_yuv_sampled_kernel<f(), s()>, src, srcStride, encodeCoefficients(colorspace), dst);
			}
		});
	}) || forFormat(Grouped{}, format, [&](auto) {
		forFormat(Sitings422{}, siting,
		    [&](auto s) { run("bgrx_to_v210", bgrx_to_v210_kernel<s()>, src, srcStride, encodeCoefficients10(colorspace), dst); });
	}) || forFormat(Rgb{}, format, [&](auto f) { run("bgrx_to_rgb", bgrx_to_rgb_kernel<f()>, src, srcStride, dst); });
	if (!done) noKernel("encode", format);
}

void launchEncodeState(int format, int colorspace, const void *state, const YuvPlanes &dst, int width, int height,
    hipStream_t stream) {
	const StripLaunch run{formatInfo(format), width, height, stream};
	const f16 *st = static_cast<const f16 *>(state);
	const int siting = sitingOf(run.info, colorspace);
	const bool done = forFormat(Yuv420p10{}, format, [&](auto f) {
		forFormat(Sitings420{}, siting, [&](auto s) {
			run("state_to_yuv420p10", state_to_yuv420p10_kernel<f() == kP010, s()>, st, encodeCoefficients10(colorspace), dst);
		});
	}) || forFormat(Sampled{}, format, [&](auto f) {
		if constexpr (SampledTraits<f()>::kDeep) {
			forSampledSiting<f()>(siting, [&](auto s) {
				run("state_to_yuv_sampled10", state_to_yuv_sampled10_kernel<f(), s()>, st, encodeCoefficients10(colorspace), dst);
			});
		} else {
			noKernel("encode from the state", format);
		}
	}) || forFormat(Grouped{}, format, [&](auto) {
		forFormat(Sitings422{}, siting,
		    [&](auto s) { run("state_to_v210", state_to_v210_kernel<s()>, st, encodeCoefficients10(colorspace), dst); });
	}) || forFormat(Rgb{}, format, [&](auto f) {
		if constexpr (RgbTraits<f()>::kKind != kU8) run("state_to_rgb", state_to_rgb_kernel<f()>, st, dst);
		else noKernel("encode from the state", format);
	});
	if (!done) noKernel("encode from the state", format);
}

void launchEncodeFrame16(int format, int colorspace, const std::uint16_t *frame, const YuvPlanes &dst, int width, int height,
    hipStream_t stream) {
	const StripLaunch run{formatInfo(format), width, height, stream};
	const int siting = sitingOf(run.info, colorspace);
	const bool done = forFormat(Yuv420p10{}, format, [&](auto f) {
		forFormat(Sitings420{}, siting, [&](auto s) {
			run("frame16_to_yuv420p10", frame16_to_yuv420p10_kernel<f() == kP010, s()>, frame, encodeCoefficients10(colorspace), dst);
		});
	}) || forFormat(Sampled{}, format, [&](auto f) {
		if constexpr (SampledTraits<f()>::kDeep) {
			forSampledSiting<f()>(siting, [&](auto s) {
				run("frame16_to_yuv_sampled10", frame16_to_yuv_sampled10_kernel<f(), s()>, frame, encodeCoefficients10(colorspace), dst);
			});
		} else {
			noKernel("encode from a 16-bit frame", format);
		}
	}) || forFormat(Grouped{}, format, [&](auto) {
		forFormat(Sitings422{}, siting,
		    [&](auto s) { run("frame16_to_v210", frame16_to_v210_kernel<s()>, frame, encodeCoefficients10(colorspace), dst); });
	}) || forFormat(Rgb{}, format, [&](auto f) {
		if constexpr (RgbTraits<f()>::kKind != kU8) run("frame16_to_rgb", frame16_to_rgb_kernel<f()>, frame, dst);
		else noKernel("encode from a 16-bit frame", format);
	});
	if (!done) noKernel("encode from a 16-bit frame", format);
}

}  // namespace ju
