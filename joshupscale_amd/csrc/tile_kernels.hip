// Tiled upscaling on gfx950 (docs/tiled.md): a BGRX source larger than the model cut into the model-size inputs of its
// tiles, and the tiles' upscaled outputs blended into one frame.  Both kernels compute exactly the numpy definitions of
// tests/tiled_reference.py; the host builds the layout (tile_geometry.h) and the device only copies, multiplies and adds
// integers.
//
//   tile_split_kernel   grid.z = tile; a lane takes four pixels of one tile row: 16 bytes per load where the source
//                       address is 16-byte aligned (a tile origin that is a multiple of four pixels in an aligned
//                       source), four 4-byte loads otherwise -- a wave reads one contiguous row segment either way --
//                       and one 16-byte store into the dense tile (X = 0).
//   tile_stitch_kernel  a lane takes four output pixels of one row, the groups laid so that every whole group begins
//                       on a 16-byte boundary of the DESTINATION row (a row that starts off 16 bytes has a short head
//                       group, written pixel by pixel, as is the tail).  Per pixel the two axis tables name the first
//                       tile and the weight of the next one; a group that lies under ONE tile -- all of a frame but
//                       its seams -- is one 16-byte load and one 16-byte store, a pixel on a seam reads two or four
//                       tiles: out = (sum wy wx v + 32768) >> 16 per byte, at most 65536 * 255 < 2^32.
//
// Both are bound by memory: the split moves 2 x 4 Ws Hs bytes and a little more (the overlaps are read and written
// twice), the stitch 2 x 64 Ws Hs.  Tile pointers and origins travel by value in the kernel arguments (TileSet).
// Rows are addressed with their signed stride; every address and stride is a multiple of 4 (the launchers refuse others).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"
#include "kernels.h"

namespace ju {

namespace {

constexpr unsigned kOpaqueMask = 0x00ffffffu;  // B, G, R kept, X = 0

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<std::uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(256) void tile_split_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    const TileSet tiles, int tileW, int tileH) {
	const int k = blockIdx.z;
	const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
	const int r = blockIdx.y * 4 + threadIdx.y;
	if (x0 >= tileW || r >= tileH) return;
	const std::uint8_t *s = src + static_cast<std::ptrdiff_t>(tiles.y[k] + r) * srcStride +
	                        static_cast<std::ptrdiff_t>(tiles.x[k] + x0) * 4;
	std::uint8_t *d = tiles.ptr[k] + (static_cast<std::size_t>(r) * tileW + x0) * 4;
	if (x0 + 4 <= tileW) {
		uint4 v;
		if (aligned16(s)) {
			v = *reinterpret_cast<const uint4 *>(s);
		} else {
			const unsigned *w = reinterpret_cast<const unsigned *>(s);
			v = make_uint4(w[0], w[1], w[2], w[3]);
		}
		v.x &= kOpaqueMask;
		v.y &= kOpaqueMask;
		v.z &= kOpaqueMask;
		v.w &= kOpaqueMask;
		if (aligned16(d)) {
			*reinterpret_cast<uint4 *>(d) = v;
		} else {
			unsigned *w = reinterpret_cast<unsigned *>(d);
			w[0] = v.x;
			w[1] = v.y;
			w[2] = v.z;
			w[3] = v.w;
		}
		return;
	}
	for (int i = 0; x0 + i < tileW; ++i) {  // the last group of a width that is no multiple of four
		reinterpret_cast<unsigned *>(d)[i] = reinterpret_cast<const unsigned *>(s)[i] & kOpaqueMask;
	}
}

// pixel (X, Y) of the frame as tile k holds it
__device__ __forceinline__ const std::uint8_t *tileAt(const TileSet &tiles, int k, int X, int Y, int tileOutW) {
	return tiles.ptr[k] + (static_cast<std::size_t>(Y - kTileScale * tiles.y[k]) * tileOutW + (X - kTileScale * tiles.x[k])) * 4;
}

// one output pixel from the up to four tiles its two table entries name
__device__ __forceinline__ unsigned stitchPixel(const TileSet &tiles, int nx, unsigned ex, unsigned ey, int X, int Y,
    int tileOutW) {
	const int tx = ex & 0xffffu, ty = ey & 0xffffu;
	const unsigned qx = ex >> 16, qy = ey >> 16;
	const unsigned wx[2] = {256u - qx, qx}, wy[2] = {256u - qy, qy};
	unsigned b = 32768u, g = 32768u, c = 32768u;
#pragma unroll
	for (int j = 0; j < 2; ++j) {
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			const unsigned w = wy[j] * wx[i];
			if (w == 0) continue;  // (a tile without weight is not read: it may not cover the pixel, or not exist)
			const unsigned v = *reinterpret_cast<const unsigned *>(tileAt(tiles, (ty + j) * nx + tx + i, X, Y, tileOutW));
			b += w * (v & 255u);
			g += w * ((v >> 8) & 255u);
			c += w * ((v >> 16) & 255u);
		}
	}
	return (b >> 16) | ((g >> 16) << 8) | ((c >> 16) << 16);
}

__global__ __launch_bounds__(256) void tile_stitch_kernel(std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int outW,
    int outH, const TileSet tiles, int nx, int tileOutW, const unsigned *__restrict__ xTable,
    const unsigned *__restrict__ yTable) {
	const int group = blockIdx.x * 64 + threadIdx.x;
	for (int Y = blockIdx.y * 4 + threadIdx.y; Y < outH; Y += gridDim.y * 4) {
		std::uint8_t *row = dst + static_cast<std::ptrdiff_t>(Y) * dstStride;
		// pixels in front of the row's first 16-byte boundary: group 0; whole groups from there on
		const int head = static_cast<int>(((16u - (reinterpret_cast<std::uintptr_t>(row) & 15u)) & 15u) >> 2);
		const int X0 = group == 0 ? 0 : head + 4 * (group - 1);
		const int X1 = group == 0 ? min(head, outW) : min(X0 + 4, outW);
		if (X0 >= X1) continue;
		const unsigned ey = yTable[Y];
		if (X1 - X0 == 4) {
			const unsigned e0 = xTable[X0], e1 = xTable[X0 + 1], e2 = xTable[X0 + 2], e3 = xTable[X0 + 3];
			uint4 v;
			const std::uint8_t *one = tileAt(tiles, (ey & 0xffffu) * nx + (e0 & 0xffffu), X0, Y, tileOutW);
			// (equal entries without weight: the four pixels lie under one tile, next to each other)
			if ((ey >> 16) == 0 && (e0 >> 16) == 0 && e0 == e1 && e0 == e2 && e0 == e3 && aligned16(one)) {
				v = *reinterpret_cast<const uint4 *>(one);
				v.x &= kOpaqueMask;
				v.y &= kOpaqueMask;
				v.z &= kOpaqueMask;
				v.w &= kOpaqueMask;
			} else {
				v.x = stitchPixel(tiles, nx, e0, ey, X0, Y, tileOutW);
				v.y = stitchPixel(tiles, nx, e1, ey, X0 + 1, Y, tileOutW);
				v.z = stitchPixel(tiles, nx, e2, ey, X0 + 2, Y, tileOutW);
				v.w = stitchPixel(tiles, nx, e3, ey, X0 + 3, Y, tileOutW);
			}
			std::uint8_t *d = row + static_cast<std::ptrdiff_t>(X0) * 4;
			if (aligned16(d)) {
				*reinterpret_cast<uint4 *>(d) = v;
			} else {  // (a frame narrower than its head: four pixels, but not on a boundary)
				unsigned *w = reinterpret_cast<unsigned *>(d);
				w[0] = v.x;
				w[1] = v.y;
				w[2] = v.z;
				w[3] = v.w;
			}
			continue;
		}
		for (int X = X0; X < X1; ++X) {
			reinterpret_cast<unsigned *>(row)[X] = stitchPixel(tiles, nx, xTable[X], ey, X, Y, tileOutW);
		}
	}
}

void checkTileSet(const char *who, const TileSet &tiles, int count, unsigned align) {
	if (count < 1 || count > kTileMax) throw std::invalid_argument(std::string(who) + ": 1 .. 64 tiles");
	for (int k = 0; k < count; ++k) {
		if (tiles.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(tiles.ptr[k]) % align) {
			throw std::invalid_argument(std::string(who) + ": tile " + std::to_string(k) + " is NULL or not " + std::to_string(align) +
			                            "-byte aligned");
		}
	}
}

void checkRows(const char *who, const void *ptr, std::ptrdiff_t stride) {
	if (ptr == nullptr || reinterpret_cast<std::uintptr_t>(ptr) % 4 || stride % 4) {
		throw std::invalid_argument(std::string(who) + ": the frame's address and stride must be multiples of 4");
	}
}

}  // namespace

void launchTileSplit(const std::uint8_t *src, std::ptrdiff_t srcStride, const TileSet &tiles, int count, int tileW, int tileH,
    hipStream_t stream) {
	checkTileSet("tile_split", tiles, count, 16);
	checkRows("tile_split", src, srcStride);
	if (tileW < 1 || tileH < 1) throw std::invalid_argument("tile_split: empty tiles");
	const dim3 grid((static_cast<unsigned>(tileW) + 255) / 256, (static_cast<unsigned>(tileH) + 3) / 4, static_cast<unsigned>(count));
	hipLaunchKernelGGL(tile_split_kernel, grid, dim3(64, 4), 0, stream, src, srcStride, tiles, tileW, tileH);
	hipCheckLaunch("tile_split");
}

void launchTileStitch(std::uint8_t *dst, std::ptrdiff_t dstStride, int outW, int outH, const TileSet &tiles, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, hipStream_t stream) {
	if (nx < 1 || ny < 1) throw std::invalid_argument("tile_stitch: 1 .. 64 tiles");
	checkTileSet("tile_stitch", tiles, nx * ny, 16);
	checkRows("tile_stitch", dst, dstStride);
	if (outW < 1 || outH < 1 || tileOutW < 1 || xTable == nullptr || yTable == nullptr) {
		throw std::invalid_argument("tile_stitch: empty frame or NULL table");
	}
	// a head group and the whole groups behind it: at most outW / 4 + 2 per row
	const unsigned groups = static_cast<unsigned>(outW) / 4 + 2;
	const unsigned rows = (static_cast<unsigned>(outH) + 3) / 4;
	const dim3 grid((groups + 63) / 64, rows < 65535u ? rows : 65535u);
	hipLaunchKernelGGL(tile_stitch_kernel, grid, dim3(64, 4), 0, stream, dst, dstStride, outW, outH, tiles, nx, tileOutW, xTable,
	    yTable);
	hipCheckLaunch("tile_stitch");
}

}  // namespace ju
