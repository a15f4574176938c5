// Tiled upscaling on gfx950 (docs/tiled.md): a BGRX source larger than the model cut into the model-size inputs of its
// tiles, and the tiles' upscaled outputs blended into one frame.  Both kernels compute exactly the numpy definitions of
// tests/tiled_reference.py; the host builds the layout (tile_geometry.h) and the device only copies, multiplies and adds
// integers.
//
//   tile_split_kernel   grid.z = tile; a lane takes four pixels of one tile row: ONE 16-byte load at the source's 4-byte-
//                       aligned address (gfx950 takes it at any such address; a wave reads one contiguous row segment)
//                       and ONE 16-byte store into the dense tile (X = 0); pixel by pixel only for a row's last group
//                       and for the rows of a tile width that is no multiple of four.
//   tile_split_frames_kernel  the split of the K frames of a look-ahead pass in ONE launch (docs/tiled.md "Look-ahead
//                       passes"): grid.z = frame * tiles + tile, each frame its own source, stride and alignment.
//   tile_split_scene_kernel  the split with the tiled stream's scene detector in the same pass (docs/tiled.md "Scene
//                       cuts"): the same grid and tile bytes, and per OWNED source pixel the kept frame read, summed
//                       against and rewritten -- 2 x 4 Ws Hs bytes on top of the split's.
//   tile_stitch_kernel  a lane takes four output pixels of one row, the groups laid so that every whole group begins
//                       on a 16-byte boundary of the DESTINATION row (a row that starts off 16 bytes has a short head
//                       group, written pixel by pixel, as is the tail).  Per pixel the two axis tables name the first
//                       tile and the weight of the next one; a group that lies under ONE tile -- all of a frame but
//                       its seams -- is one 16-byte load and one 16-byte store, a pixel on a seam reads two or four
//                       tiles: out = (sum wy wx v + 32768) >> 16 per byte, at most 65536 * 255 < 2^32.
//   tile_stitch_state_kernel  the same blend over the tiles' f16 STATES, per 16-bit sample P of a state, into a dense
//                       u16 frame that launchEncodeFrame16 encodes (deep outputs; tests/tiled_deep_reference.py): no
//                       head or tail groups, a capped grid that strides over the rows, 2 x 8 x 4 Ws x 4 Hs bytes.
//   tile_stitch_scale_kernel, tile_stitch_scale_state_kernel  the two blends FUSED into the output scaler (docs/tiled.md
//                       "An output size"; tests/tiled_output_reference.py): the scale kernels' tile (scale_tile.h) whose
//                       vertical pass forms each blended sample in registers, so the frame of 4 Ws x 4 Hs is never stored.
//   tile_stitch_mask_kernel, tile_stitch_mask_scale_kernel  the 8-bit stitch and its fused form under a SOURCE MASK
//                       (docs/tiled.md "A mask"; tests/tiled_mask_reference.py): inside the mask's box (mask_box.h) the
//                       blended pixel is mixed with the source pixel through its mask texel while it is in registers --
//                       mask_blend_kernel's integers; outside the box the unmasked kernels' path, no mask or source read.
//
// Split and stitch are bound by memory: the split moves 2 x 4 Ws Hs bytes and a little more (the overlaps are read and
// written twice), the stitch 2 x 64 Ws Hs.  Tile pointers and origins travel by value in the kernel arguments (TileSet); the
// state stitch and the fused kernels copy them into LDS once per workgroup.
// Rows are addressed with their signed stride; every address and stride is a multiple of 4 (the launchers refuse others).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"
#include "kernels.h"
#include "scale_tile.h"
#include "scene_decision.h"

namespace ju {

namespace {

constexpr unsigned kOpaqueMask = 0x00ffffffu;  // B, G, R kept, X = 0

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<std::uintptr_t>(p) & 15u) == 0; }

// what one lane of the split does: four pixels of row r of one tile, from x0 on (tile_split_kernel, tile_split_frames_kernel)
// -- into tile k's image, `at` bytes behind tiles.ptr[k] (a look-ahead pass's slot of the frame; 0: the tile itself)
__device__ __forceinline__ void splitLane(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride, const TileSet &tiles, int k,
    std::size_t at, int x0, int r, int tileW) {
	const std::uint8_t *s = src + static_cast<std::ptrdiff_t>(tiles.y[k] + r) * srcStride +
	                        static_cast<std::ptrdiff_t>(tiles.x[k] + x0) * 4;
	std::uint8_t *d = tiles.ptr[k] + at + (static_cast<std::size_t>(r) * tileW + x0) * 4;
	// A whole group into a 16-byte-aligned place -- every group of a tile whose width is a multiple of four: the tiles and a
	// pass's slots are 16-byte aligned (checkTileSet, launchTileSplitFrames) -- is ONE 16-byte store.  The source is read
	// as one 16-byte load whatever its address: gfx950 takes a dwordx4 load at a 4-byte-aligned address, so a frame's
	// alignment costs no other instruction, only the memory system's handling of the split access.
	if (x0 + 4 <= tileW && aligned16(d)) {
		const unsigned *w = reinterpret_cast<const unsigned *>(s);
		uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
		v.x &= kOpaqueMask;
		v.y &= kOpaqueMask;
		v.z &= kOpaqueMask;
		v.w &= kOpaqueMask;
		*reinterpret_cast<uint4 *>(__builtin_assume_aligned(d, 16)) = v;
		return;
	}
	// pixel by pixel: the last group of a width that is no multiple of four, and every group of such a tile's rows that
	// do not start on a 16-byte boundary
	for (int i = 0; i < 4 && x0 + i < tileW; ++i) {
		reinterpret_cast<unsigned *>(d)[i] = reinterpret_cast<const unsigned *>(s)[i] & kOpaqueMask;
	}
}

__global__ __launch_bounds__(256) void tile_split_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    const TileSet tiles, int tileW, int tileH) {
	const int k = blockIdx.z;
	const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
	const int r = blockIdx.y * 4 + threadIdx.y;
	if (x0 >= tileW || r >= tileH) return;
	splitLane(src, srcStride, tiles, k, 0, x0, r, tileW);
}

// ---- the split of a look-ahead pass (docs/tiled.md "Look-ahead passes") -------------------------------------------------
// tile_split_frames_kernel: tile_split_kernel over the K frames of a pass in ONE launch, grid.z = f * count + k (at most
// 8 x 64 slices).  Frame f's source and signed stride are frames.src[f] / frames.stride[f]; tile k's input of frame f lies at
// tiles.ptr[k] + f * slot.  f and k come from blockIdx alone, so what a workgroup reads of the two by-value arguments is
// uniform: scalar loads from the kernel-argument segment, no per-lane table and no scratch.  Nothing in the launch depends
// on a frame's alignment: each lane loads from its own frame's address, as in tile_split_kernel, so the frames of one pass
// may differ in alignment, stride, sign and padding.
__global__ __launch_bounds__(256) void tile_split_frames_kernel(const TileFrames frames, const TileSet tiles, std::size_t slot,
    int count, int tileW, int tileH) {
	const int f = blockIdx.z / static_cast<unsigned>(count);
	const int k = blockIdx.z - f * count;
	const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
	const int r = blockIdx.y * 4 + threadIdx.y;
	if (x0 >= tileW || r >= tileH) return;
	splitLane(frames.src[f], static_cast<std::ptrdiff_t>(frames.stride[f]), tiles, k, static_cast<std::size_t>(f) * slot, x0, r, tileW);
}

// ---- the split with the tiled stream's scene detector (docs/tiled.md "Scene cuts") --------------------------------------
// tile_split_scene_kernel: tile_split_kernel's grid and tile bytes, and in the same pass over the source scene_sad_kernel's
// sum against the kept SOURCE-size frame.  Tiles overlap, so a source pixel is COUNTED by one tile only, its owner: tile k
// owns [x[k], own.x1[k]) x [y[k], own.y1[k]) -- on a row a prefix of the tile's pixels, so a lane's group of four owns its
// first m pixels, 0 <= m <= 4 (a group may straddle the edge, or be a row's tail).  For an owned pixel the lane loads the
// kept pixel, adds |d| of B, G and R (v_sad_u8 on the three low bytes, 32-bit partials) and writes the masked pixel over
// it: no other lane of the grid touches that kept pixel.  Then scene_sad_kernel's reduction: wave sum, workgroup sum, one
// 64-bit atomic add per workgroup at agent scope, release, ticket; the workgroup that draws the last of sc.groups tickets
// takes the decision (sceneDecide).  No lane returns early -- a workgroup whose lanes own nothing, or lie outside the tile,
// still draws its ticket -- and no workgroup waits for another.
struct TileSceneArgs {
	std::uint32_t *prev;
	SceneState *st;
	SceneRecord *ring;
	unsigned long long step;
	long long pixels;
	int srcW, slot, hasPrev, resetMode;
	unsigned thresholdMilli, groups;
};

__global__ __launch_bounds__(256) void tile_split_scene_kernel(const std::uint8_t *__restrict__ src, std::ptrdiff_t srcStride,
    const TileSet tiles, const TileOwn own, int tileW, int tileH, const TileSceneArgs sc) {
	__shared__ unsigned waveSums[4];
	const int k = blockIdx.z;
	const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
	const int r = blockIdx.y * 4 + threadIdx.y;
	unsigned partial = 0;
	if (x0 < tileW && r < tileH) {
		const int sx = tiles.x[k] + x0, sy = tiles.y[k] + r;
		const std::uint8_t *s = src + static_cast<std::ptrdiff_t>(sy) * srcStride + static_cast<std::ptrdiff_t>(sx) * 4;
		std::uint8_t *d = tiles.ptr[k] + (static_cast<std::size_t>(r) * tileW + x0) * 4;
		std::uint32_t *kept = sc.prev + static_cast<std::size_t>(sy) * static_cast<std::size_t>(sc.srcW) + sx;
		const int n = min(4, tileW - x0);
		const int m = sy < own.y1[k] ? max(0, min(n, own.x1[k] - sx)) : 0;
		if (n == 4) {
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
			if (m == 4 && aligned16(kept)) {
				const uint4 o = *reinterpret_cast<const uint4 *>(kept);
				*reinterpret_cast<uint4 *>(kept) = v;
				partial = __builtin_amdgcn_sad_u8(v.x, o.x & kOpaqueMask, partial);
				partial = __builtin_amdgcn_sad_u8(v.y, o.y & kOpaqueMask, partial);
				partial = __builtin_amdgcn_sad_u8(v.z, o.z & kOpaqueMask, partial);
				partial = __builtin_amdgcn_sad_u8(v.w, o.w & kOpaqueMask, partial);
			} else {
				const unsigned px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					if (i < m) {
						partial = __builtin_amdgcn_sad_u8(px[i], kept[i] & kOpaqueMask, partial);
						kept[i] = px[i];
					}
				}
			}
		} else {
			for (int i = 0; i < n; ++i) {  // the last group of a width that is no multiple of four
				const unsigned p = reinterpret_cast<const unsigned *>(s)[i] & kOpaqueMask;
				reinterpret_cast<unsigned *>(d)[i] = p;
				if (i < m) {
					partial = __builtin_amdgcn_sad_u8(p, kept[i] & kOpaqueMask, partial);
					kept[i] = p;
				}
			}
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) partial += __shfl_down(partial, off, 64);
	if (threadIdx.x == 0) waveSums[threadIdx.y] = partial;  // (a wave is one row of the 64 x 4 workgroup)
	__syncthreads();
	if (threadIdx.x != 0 || threadIdx.y != 0) return;
	const unsigned long long groupSum = static_cast<unsigned long long>(waveSums[0]) + waveSums[1] + waveSums[2] + waveSums[3];
	__hip_atomic_fetch_add(&sc.st->acc, groupSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	// publish the add before the ticket (fence, then its wait, then the ticket: in that order)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const unsigned ticket = __hip_atomic_fetch_add(&sc.st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (ticket != sc.groups - 1) return;
	// ---- the last workgroup of the launch: the decision (scene_decision.h) ----
	sceneDecide(sc.st, sc.ring, sc.slot, sc.step, sc.hasPrev, sc.thresholdMilli, sc.resetMode, sc.pixels);
}

// pixel (X, Y) of the frame as tile k holds it (Tiles: the launch's TileSet, or the workgroup's TileView of it in LDS)
template <typename Tiles>
__device__ __forceinline__ const std::uint8_t *tileAt(const Tiles &tiles, int k, int X, int Y, int tileOutW) {
	return tiles.ptr[k] + (static_cast<std::size_t>(Y - kTileScale * tiles.y[k]) * tileOutW + (X - kTileScale * tiles.x[k])) * 4;
}

// one output pixel from the up to four tiles its two table entries name
template <typename Tiles>
__device__ __forceinline__ unsigned stitchPixel(const Tiles &tiles, int nx, unsigned ex, unsigned ey, int X, int Y,
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

// ---- the source mask (docs/tiled.md "A mask"; tests/tiled_mask_reference.py) ---------------------------------------------
// mask_blend_kernel's arithmetic (source_kernels.hip) on a blended pixel g in registers: m the mask texel, s the source
// pixel; a = 765 - (Bm + Gm + Rm), out = (s a + g (765 - a) + 382) / 765 per byte of B, G, R, X = 0; a == 0: g as it is.
__device__ __forceinline__ unsigned maskPixel(unsigned g, unsigned s, unsigned m) {
	const unsigned a = 765u - ((m & 255u) + ((m >> 8) & 255u) + ((m >> 16) & 255u));
	if (a == 0) return g;
	unsigned out = 0;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const unsigned sc = (s >> (8 * c)) & 255u, gc = (g >> (8 * c)) & 255u;
		out |= ((sc * a + gc * (765u - a) + 382u) / 765u) << (8 * c);
	}
	return out;
}

constexpr unsigned kWhiteTexel = 0x00ffffffu;  // a == 0: what a pixel outside the box takes for its mask texel

// The mask texels and the source pixels of up to four blended pixels X .. X + 3 of row Y, those inside [X, xEnd) and inside
// the box; the others white.  The addresses depend on coordinates only, so the loads are issued in front of the tile loads
// of the same pixels.  The source texel of (X, Y) is (X >> 2, Y >> 2): the blended frame is exactly four times the source.
struct MaskTaps {
	unsigned m[4], s[4];
};
__device__ __forceinline__ MaskTaps maskTaps(const TileMask &mk, int X, int xEnd, int Y, unsigned outW, unsigned outH) {
	const unsigned my = (2u * static_cast<unsigned>(Y) + 1u) * static_cast<unsigned>(mk.maskH) / (2u * outH);
	const std::uint8_t *mrow = mk.mask + static_cast<std::ptrdiff_t>(my) * mk.maskStride;
	const std::uint8_t *srow = mk.src + static_cast<std::ptrdiff_t>(Y >> 2) * mk.srcStride;
	MaskTaps t;
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int x = X + i;
		const bool in = x < xEnd && x >= mk.x0 && x < mk.x1;
		const unsigned mx = (2u * static_cast<unsigned>(x) + 1u) * static_cast<unsigned>(mk.maskW) / (2u * outW);
		t.m[i] = in ? *reinterpret_cast<const unsigned *>(mrow + 4 * static_cast<std::size_t>(mx)) : kWhiteTexel;
		t.s[i] = in ? *reinterpret_cast<const unsigned *>(srow + 4 * static_cast<std::size_t>(x >> 2)) : 0u;
	}
	return t;
}

// tile_stitch_kernel with the mask: the same grid, groups, head and tail rules and stores.  A group wholly outside the box
// takes tile_stitch_kernel's path as it stands; a group that touches the box forms its pixels the same way and then blends
// those inside the box with the source through their mask texels.
__global__ __launch_bounds__(256) void tile_stitch_mask_kernel(std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int outW,
    int outH, const TileSet tiles, int nx, int tileOutW, const unsigned *__restrict__ xTable,
    const unsigned *__restrict__ yTable, const TileMask mk) {
	const int group = blockIdx.x * 64 + threadIdx.x;
	for (int Y = blockIdx.y * 4 + threadIdx.y; Y < outH; Y += gridDim.y * 4) {
		std::uint8_t *row = dst + static_cast<std::ptrdiff_t>(Y) * dstStride;
		const int head = static_cast<int>(((16u - (reinterpret_cast<std::uintptr_t>(row) & 15u)) & 15u) >> 2);
		const int X0 = group == 0 ? 0 : head + 4 * (group - 1);
		const int X1 = group == 0 ? min(head, outW) : min(X0 + 4, outW);
		if (X0 >= X1) continue;
		const bool boxed = Y >= mk.y0 && Y < mk.y1 && X0 < mk.x1 && X1 > mk.x0;
		MaskTaps t;
		if (boxed) t = maskTaps(mk, X0, X1, Y, static_cast<unsigned>(outW), static_cast<unsigned>(outH));
		const unsigned ey = yTable[Y];
		if (X1 - X0 == 4) {
			const unsigned e0 = xTable[X0], e1 = xTable[X0 + 1], e2 = xTable[X0 + 2], e3 = xTable[X0 + 3];
			uint4 v;
			const std::uint8_t *one = tileAt(tiles, (ey & 0xffffu) * nx + (e0 & 0xffffu), X0, Y, tileOutW);
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
			if (boxed) {
				v.x = maskPixel(v.x, t.s[0], t.m[0]);
				v.y = maskPixel(v.y, t.s[1], t.m[1]);
				v.z = maskPixel(v.z, t.s[2], t.m[2]);
				v.w = maskPixel(v.w, t.s[3], t.m[3]);
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
#pragma unroll
		for (int i = 0; i < 3; ++i) {  // a head or a tail: one to three pixels
			const int X = X0 + i;
			if (X >= X1) break;
			unsigned p = stitchPixel(tiles, nx, xTable[X], ey, X, Y, tileOutW);
			if (boxed) p = maskPixel(p, t.s[i], t.m[i]);
			reinterpret_cast<unsigned *>(row)[X] = p;
		}
	}
}

// ---- the blend of the tiles' f16 states (docs/tiled.md "Deep outputs"; tests/tiled_deep_reference.py stitch16) ----------
// P of one f16 of a state, as StateSource::sample (colour_kernels.hip) forms it: exact in f32
__device__ __forceinline__ unsigned stateP(unsigned bits) {
	const float s = static_cast<float>(__builtin_bit_cast(f16, static_cast<unsigned short>(bits)));
	return static_cast<unsigned>(fminf(fmaxf(floorf((s + 0.5f) * 65536.0f), 0.0f), 65535.0f));
}

// two pixels of a state (eight f16: B, G, R, unused twice) as two pixels of the 16-bit frame (P_B | P_G << 16, P_R, twice)
__device__ __forceinline__ uint4 statePair(uint4 v) {
	return make_uint4(stateP(v.x & 0xffffu) | (stateP(v.x >> 16) << 16), stateP(v.y & 0xffffu),
	    stateP(v.z & 0xffffu) | (stateP(v.z >> 16) << 16), stateP(v.w & 0xffffu));
}

// the tiles as a workgroup holds them in LDS (below)
struct TileView {
	const std::uint8_t *const *ptr;
	const int *x, *y;
};

// one pixel of the 16-bit frame from the up to four states its two table entries name (8-byte loads)
__device__ __forceinline__ uint2 stitchStatePixel(const TileView &tiles, int nx, unsigned ex, unsigned ey, int X, int Y,
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
			const int k = (ty + j) * nx + tx + i;
			const uint2 v = *reinterpret_cast<const uint2 *>(
			    tiles.ptr[k] + (static_cast<std::size_t>(Y - kTileScale * tiles.y[k]) * tileOutW + (X - kTileScale * tiles.x[k])) * 8);
			b += w * stateP(v.x & 0xffffu);
			g += w * stateP(v.x >> 16);
			c += w * stateP(v.y & 0xffffu);
		}
	}
	return make_uint2((b >> 16) | (g & 0xffff0000u), c >> 16);
}

// A lane takes four pixels of a row from X0 = 0 (mod 4) -- 32 bytes of the destination, and 32-byte aligned in it and in
// every state that covers them (outW, tileOutW and every tile origin are multiples of four pixels): no head, no tail.  The
// grid is capped and strides over the rows, so the lane's four column entries are fetched ONCE, in front of the loop, and
// the next row's entry while this row's pixels are on their way: only the states' pointers and the pixels themselves are
// behind a dependent load.  Four pixels under one tile: two 16-byte loads, twelve samples, two 16-byte stores.
// The tiles' pointers and origins go from the kernel arguments into LDS once per workgroup: a lane's lookup by its own
// index is then an LDS read, not a load from the argument segment in every row.
__global__ __launch_bounds__(256) void tile_stitch_state_kernel(std::uint16_t *__restrict__ dst, int outW, int outH,
    const TileSet set, int nx, int count, int tileOutW, const unsigned *__restrict__ xTable,
    const unsigned *__restrict__ yTable) {
	__shared__ const std::uint8_t *sPtr[kTileMax];
	__shared__ int sX[kTileMax], sY[kTileMax];
	const int lane = threadIdx.y * 64 + threadIdx.x;
	if (lane < count) {
		sPtr[lane] = set.ptr[lane];
		sX[lane] = set.x[lane];
		sY[lane] = set.y[lane];
	}
	__syncthreads();
	const TileView tiles{sPtr, sX, sY};
	const int X0 = (blockIdx.x * 64 + threadIdx.x) * 4;
	int Y = blockIdx.y * 4 + threadIdx.y;
	if (X0 >= outW || Y >= outH) return;
	const int step = gridDim.y * 4;
	unsigned ey = yTable[Y];
	const uint4 ex = *reinterpret_cast<const uint4 *>(xTable + X0);
	// (equal entries without weight: the four columns lie under one tile column, whose origin every tile row shares)
	const bool oneColumn = (ex.x >> 16) == 0 && ex.x == ex.y && ex.x == ex.z && ex.x == ex.w;
	const int tx = ex.x & 0xffffu;
	const int xIn = X0 - kTileScale * tiles.x[tx];
	for (;;) {
		const int next = Y + step;
		const unsigned eyNext = next < outH ? yTable[next] : 0u;
		uint4 lo, hi;
		if (oneColumn && (ey >> 16) == 0) {
			const int k = (ey & 0xffffu) * nx + tx;
			const uint4 *s = reinterpret_cast<const uint4 *>(
			    tiles.ptr[k] + (static_cast<std::size_t>(Y - kTileScale * tiles.y[k]) * tileOutW + xIn) * 8);
			const uint4 a = s[0], b = s[1];
			lo = statePair(a);
			hi = statePair(b);
		} else {
			const uint2 p0 = stitchStatePixel(tiles, nx, ex.x, ey, X0, Y, tileOutW);
			const uint2 p1 = stitchStatePixel(tiles, nx, ex.y, ey, X0 + 1, Y, tileOutW);
			const uint2 p2 = stitchStatePixel(tiles, nx, ex.z, ey, X0 + 2, Y, tileOutW);
			const uint2 p3 = stitchStatePixel(tiles, nx, ex.w, ey, X0 + 3, Y, tileOutW);
			lo = make_uint4(p0.x, p0.y, p1.x, p1.y);
			hi = make_uint4(p2.x, p2.y, p3.x, p3.y);
		}
		uint4 *d = reinterpret_cast<uint4 *>(dst + (static_cast<std::size_t>(Y) * outW + X0) * 4);
		d[0] = lo;
		d[1] = hi;
		if (next >= outH) break;
		Y = next;
		ey = eyNext;
	}
}

// ---- blend and scale in one launch (docs/tiled.md "An output size"; tests/tiled_output_reference.py) --------------------
// The scale kernels' tile (scale_tile.h: scaleTile8 / scaleTile16, the body of scale_bgrx_kernel / scale_state_kernel) with
// a source that FORMS each sample of the blended frame in registers from the tiles' outputs (states): the blended frame of
// 4 Ws x 4 Hs is never stored.  Only the vertical pass's loads differ from the scaler's, so the scaled bytes are its by
// construction, and the blended samples are tile_stitch_kernel's (tile_stitch_state_kernel's): stitchPixel /
// stitchStatePixel, rounded to bytes (16-bit words) BEFORE the scaler multiplies them.
// A lane's column is four (two) blended columns from X = 0 mod 4 (mod 2): the frame's width is a multiple of four, so the
// group never crosses its end, and its column entries are fetched ONCE, in front of the tap loop; per tap the entry of
// the blended row.  Equal column entries without weight under a row entry without weight -- all of a frame but its seams
// -- are ONE 16-byte load from that tile, 16-byte aligned (tiles are dense and aligned, origins and X multiples of four
// pixels); else per pixel the two or four tiles that have weight.

// the tiles and the two blend tables as a fused kernel's source takes them
struct StitchArgs {
	TileView tiles;
	int nx, tileOutW;
	const unsigned *xTable, *yTable;
};

struct StitchColumn {
	unsigned ex[4];  // the columns' entries (the 16-bit source: two)
	int Y;           // the current blended row
	int tx, xIn;     // the first entry's tile column, and X inside it
	bool oneColumn;  // equal entries without weight: the group lies under one tile column
};

// the blended 8-bit frame: tile_stitch_kernel's pixels
struct StitchSource8 {
	using Args = StitchArgs;
	using Column = StitchColumn;
	StitchArgs a;
	__device__ __forceinline__ explicit StitchSource8(const Args &args) : a(args) {}
	__device__ __forceinline__ Column column(int x, int row) const {
		const uint4 e = *reinterpret_cast<const uint4 *>(a.xTable + x);
		Column c;
		c.ex[0] = e.x, c.ex[1] = e.y, c.ex[2] = e.z, c.ex[3] = e.w;
		c.Y = row;
		c.tx = e.x & 0xffffu;
		c.xIn = x - kTileScale * a.tiles.x[c.tx];
		c.oneColumn = (e.x >> 16) == 0 && e.x == e.y && e.x == e.z && e.x == e.w;
		return c;
	}
	__device__ __forceinline__ uint4 load(const Column &c, int x) const {
		const unsigned ey = a.yTable[c.Y];
		if (c.oneColumn && (ey >> 16) == 0) {
			const int k = (ey & 0xffffu) * a.nx + c.tx;
			return *reinterpret_cast<const uint4 *>(
			    a.tiles.ptr[k] + (static_cast<std::size_t>(c.Y - kTileScale * a.tiles.y[k]) * a.tileOutW + c.xIn) * 4);
		}
		return make_uint4(stitchPixel(a.tiles, a.nx, c.ex[0], ey, x, c.Y, a.tileOutW), stitchPixel(a.tiles, a.nx, c.ex[1], ey, x + 1, c.Y, a.tileOutW),
		    stitchPixel(a.tiles, a.nx, c.ex[2], ey, x + 2, c.Y, a.tileOutW), stitchPixel(a.tiles, a.nx, c.ex[3], ey, x + 3, c.Y, a.tileOutW));
	}
	__device__ __forceinline__ Column next(Column c) const {
		++c.Y;
		return c;
	}
};

// the blended 16-bit frame: tile_stitch_state_kernel's words, (P_B | P_G << 16, P_R) per pixel as statePair packs them
struct StitchSource16 {
	using Args = StitchArgs;
	using Column = StitchColumn;
	StitchArgs a;
	__device__ __forceinline__ explicit StitchSource16(const Args &args) : a(args) {}
	__device__ __forceinline__ Column column(int x, int row) const {
		const uint2 e = *reinterpret_cast<const uint2 *>(a.xTable + x);
		Column c;
		c.ex[0] = e.x, c.ex[1] = e.y, c.ex[2] = 0, c.ex[3] = 0;
		c.Y = row;
		c.tx = e.x & 0xffffu;
		c.xIn = x - kTileScale * a.tiles.x[c.tx];
		c.oneColumn = (e.x >> 16) == 0 && e.x == e.y;
		return c;
	}
	__device__ __forceinline__ uint4 load(const Column &c, int x) const {
		const unsigned ey = a.yTable[c.Y];
		if (c.oneColumn && (ey >> 16) == 0) {
			const int k = (ey & 0xffffu) * a.nx + c.tx;
			return statePair(*reinterpret_cast<const uint4 *>(
			    a.tiles.ptr[k] + (static_cast<std::size_t>(c.Y - kTileScale * a.tiles.y[k]) * a.tileOutW + c.xIn) * 8));
		}
		const uint2 p0 = stitchStatePixel(a.tiles, a.nx, c.ex[0], ey, x, c.Y, a.tileOutW);
		const uint2 p1 = stitchStatePixel(a.tiles, a.nx, c.ex[1], ey, x + 1, c.Y, a.tileOutW);
		return make_uint4(p0.x, p0.y, p1.x, p1.y);
	}
	__device__ static __forceinline__ unsigned sample(unsigned p) { return p; }  // (already a 16-bit sample)
	__device__ __forceinline__ Column next(Column c) const {
		++c.Y;
		return c;
	}
};

// The tiles' pointers and origins from the kernel arguments into LDS, once per workgroup (1 KB in front of the scaler's
// tile), as tile_stitch_state_kernel does: a lane's lookup by its own index is then an LDS read.  All 256 lanes reach the
// barrier.
__device__ __forceinline__ TileView tilesToLds(const TileSet &set, int count) {
	__shared__ const std::uint8_t *sPtr[kTileMax];
	__shared__ int sX[kTileMax], sY[kTileMax];
	const int lane = threadIdx.x;
	if (lane < count) {
		sPtr[lane] = set.ptr[lane];
		sX[lane] = set.x[lane];
		sY[lane] = set.y[lane];
	}
	__syncthreads();
	return {sPtr, sX, sY};
}

// outW: the blended frame's width (4 Ws); dst: BGRX rows of dstW x dstH at any byte alignment, signed stride
template <bool kSigned>
__global__ __launch_bounds__(256) void tile_stitch_scale_kernel(std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW,
    int dstH, int outW, const TileSet set, int nx, int count, int tileOutW, const unsigned *__restrict__ xTable,
    const unsigned *__restrict__ yTable, ScaleTaps ax, ScaleTaps ay, int pitch) {
	const TileView tiles = tilesToLds(set, count);
	scaleTile8<kSigned, StitchSource8>({tiles, nx, tileOutW, xTable, yTable}, outW, dst, dstStride, dstW, dstH, ax, ay, pitch);
}

// dst: the dense u16 frame [dstH][dstW][4], 8-byte aligned, X = 0
template <bool kSigned>
__global__ __launch_bounds__(256) void tile_stitch_scale_state_kernel(std::uint16_t *__restrict__ dst, int dstW, int dstH, int outW,
    const TileSet set, int nx, int count, int tileOutW, const unsigned *__restrict__ xTable, const unsigned *__restrict__ yTable,
    ScaleTaps ax, ScaleTaps ay, int pitch) {
	const TileView tiles = tilesToLds(set, count);
	scaleTile16<kSigned, StitchSource16>({tiles, nx, tileOutW, xTable, yTable}, outW, dst, dstW, dstH, ax, ay, pitch);
}

// The masked blended 8-bit frame (docs/tiled.md "A mask"): StitchSource8's pixels, and for a quad that touches the box the
// mask blend of its four pixels -- at the blended size, on the rounded bytes, BEFORE the scaler multiplies them.  A quad
// starts at x = 0 (mod 4): ONE source texel, (x >> 2, Y >> 2), and four mask texels -- loaded BEHIND the tile loads here:
// in front of them they stay live across stitchPixel's loads and cost the whole kernel a wave per SIMD (docs/tiled.md).
struct StitchMaskArgs {
	StitchArgs stitch;
	TileMask mask;
	unsigned outW, outH;  // the blended frame
};

// what a lane keeps for its quad beside StitchColumn: whether the quad's columns touch the box, and if so the byte offsets
// of its four mask texels in a mask row -- the divisions are done ONCE, in front of the tap loop (a column outside the box
// keeps the offset of its neighbour inside: never read)
struct StitchMaskColumn {
	StitchColumn c;
	unsigned mx[4];
	bool boxed;
};

struct StitchMaskSource8 {
	using Args = StitchMaskArgs;
	using Column = StitchMaskColumn;
	StitchSource8 base;
	TileMask mk;
	unsigned outW, outH;
	__device__ __forceinline__ explicit StitchMaskSource8(const Args &args) : base(args.stitch), mk(args.mask), outW(args.outW), outH(args.outH) {}
	__device__ __forceinline__ Column column(int x, int row) const {
		Column m;
		m.c = base.column(x, row);
		m.boxed = x < mk.x1 && x + 4 > mk.x0;
#pragma unroll
		for (int i = 0; i < 4; ++i) m.mx[i] = 0;
		if (m.boxed) {
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const unsigned X = static_cast<unsigned>(min(max(x + i, mk.x0), mk.x1 - 1));
				m.mx[i] = (2u * X + 1u) * static_cast<unsigned>(mk.maskW) / (2u * outW) * 4u;
			}
		}
		return m;
	}
	__device__ __forceinline__ uint4 load(const Column &m, int x) const {
		const int Y = m.c.Y;
		if (!m.boxed || Y < mk.y0 || Y >= mk.y1) return base.load(m.c, x);
		const uint4 v = base.load(m.c, x);
		const unsigned my = (2u * static_cast<unsigned>(Y) + 1u) * static_cast<unsigned>(mk.maskH) / (2u * outH);
		const std::uint8_t *mrow = mk.mask + static_cast<std::ptrdiff_t>(my) * mk.maskStride;
		const unsigned s = *reinterpret_cast<const unsigned *>(mk.src + static_cast<std::ptrdiff_t>(Y >> 2) * mk.srcStride + x);  // (texel x >> 2 at 4 bytes: x itself)
		unsigned t[4];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const bool in = x + i >= mk.x0 && x + i < mk.x1;
			t[i] = in ? *reinterpret_cast<const unsigned *>(mrow + m.mx[i]) : kWhiteTexel;
		}
		return make_uint4(maskPixel(v.x & kOpaqueMask, s, t[0]), maskPixel(v.y & kOpaqueMask, s, t[1]),
		    maskPixel(v.z & kOpaqueMask, s, t[2]), maskPixel(v.w & kOpaqueMask, s, t[3]));
	}
	__device__ __forceinline__ Column next(Column m) const {
		m.c = base.next(m.c);
		return m;
	}
};

// tile_stitch_scale_kernel over the masked frame
template <bool kSigned>
__global__ __launch_bounds__(256) void tile_stitch_mask_scale_kernel(std::uint8_t *__restrict__ dst, std::ptrdiff_t dstStride, int dstW,
    int dstH, int outW, int outH, const TileSet set, int nx, int count, int tileOutW, const unsigned *__restrict__ xTable,
    const unsigned *__restrict__ yTable, ScaleTaps ax, ScaleTaps ay, int pitch, const TileMask mk) {
	const TileView tiles = tilesToLds(set, count);
	scaleTile8<kSigned, StitchMaskSource8>({{tiles, nx, tileOutW, xTable, yTable}, mk, static_cast<unsigned>(outW), static_cast<unsigned>(outH)},
	    outW, dst, dstStride, dstW, dstH, ax, ay, pitch);
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

void launchTileSplitFrames(const TileFrames &frames, int frameCount, const TileSet &tiles, std::size_t slotBytes, int count, int tileW,
    int tileH, hipStream_t stream) {
	if (frameCount < 1 || frameCount > kFlowBatchMax) throw std::invalid_argument("tile_split_frames: 1 .. 8 frames");
	checkTileSet("tile_split_frames", tiles, count, 16);
	for (int f = 0; f < frameCount; ++f) {
		try {
			checkRows("tile_split_frames", frames.src[f], static_cast<std::ptrdiff_t>(frames.stride[f]));
		} catch (const std::invalid_argument &e) {
			throw std::invalid_argument(std::string(e.what()) + " (frame " + std::to_string(f) + ")");
		}
	}
	if (tileW < 1 || tileH < 1) throw std::invalid_argument("tile_split_frames: empty tiles");
	// (every frame's slot of a tile as aligned as the tile: the 16-byte stores)
	if (frameCount > 1 && (slotBytes % 16 || slotBytes < static_cast<std::size_t>(tileW) * static_cast<std::size_t>(tileH) * 4)) {
		throw std::invalid_argument("tile_split_frames: the slot stride must be a multiple of 16 and hold a tile");
	}
	const dim3 grid((static_cast<unsigned>(tileW) + 255) / 256, (static_cast<unsigned>(tileH) + 3) / 4,
	    static_cast<unsigned>(count) * static_cast<unsigned>(frameCount));
	hipLaunchKernelGGL(tile_split_frames_kernel, grid, dim3(64, 4), 0, stream, frames, tiles, slotBytes, count, tileW, tileH);
	hipCheckLaunch("tile_split_frames");
}

void launchTileSplitScene(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, int srcH, const TileSet &tiles,
    const TileOwn &own, int count, int tileW, int tileH, const SceneSadLaunch &q, hipStream_t stream) {
	checkTileSet("tile_split_scene", tiles, count, 16);
	checkRows("tile_split_scene", src, srcStride);
	if (tileW < 1 || tileH < 1) throw std::invalid_argument("tile_split_scene: empty tiles");
	if (srcW < tileW || srcH < tileH || srcW > kTileRatioMax * tileW || srcH > kTileRatioMax * tileH) {
		throw std::invalid_argument("tile_split_scene: a source size outside the tile's .. " + std::to_string(kTileRatioMax) + " times the tile's");
	}
	if (q.prev == nullptr || q.state == nullptr || q.ring == nullptr) throw std::invalid_argument("tile_split_scene: null detector buffer");
	if (reinterpret_cast<std::uintptr_t>(q.prev) % 4 || reinterpret_cast<std::uintptr_t>(q.state) % 8) {
		throw std::invalid_argument("tile_split_scene: the kept frame must be 4-byte, the detector's state 8-byte aligned");
	}
	if (q.slot < 0 || q.slot >= kSceneRing) throw std::invalid_argument("tile_split_scene: ring slot outside 0 .. 63");
	// the kept frame is written at source coordinates: every tile and its ownership rectangle inside the source
	for (int k = 0; k < count; ++k) {
		if (tiles.x[k] < 0 || tiles.y[k] < 0 || tiles.x[k] + tileW > srcW || tiles.y[k] + tileH > srcH || own.x1[k] < tiles.x[k] ||
		    own.y1[k] < tiles.y[k] || own.x1[k] > tiles.x[k] + tileW || own.y1[k] > tiles.y[k] + tileH) {
			throw std::invalid_argument("tile_split_scene: tile " + std::to_string(k) + " or what it owns lies outside the source");
		}
	}
	// the split's grid; the ticket count the kernel compares with is this grid's workgroup count
	const dim3 grid((static_cast<unsigned>(tileW) + 255) / 256, (static_cast<unsigned>(tileH) + 3) / 4, static_cast<unsigned>(count));
	TileSceneArgs sc{};
	sc.prev = q.prev;
	sc.st = q.state;
	sc.ring = q.ring;
	sc.step = static_cast<unsigned long long>(q.step);
	sc.pixels = static_cast<long long>(srcW) * srcH;
	sc.srcW = srcW;
	sc.slot = q.slot;
	sc.hasPrev = q.hasPrev;
	sc.resetMode = q.resetMode ? 1 : 0;
	sc.thresholdMilli = q.thresholdMilli;
	sc.groups = grid.x * grid.y * grid.z;
	hipLaunchKernelGGL(tile_split_scene_kernel, grid, dim3(64, 4), 0, stream, src, srcStride, tiles, own, tileW, tileH, sc);
	hipCheckLaunch("tile_split_scene");
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

void launchTileStitchState(std::uint16_t *dst16, int outW, int outH, const TileSet &states, int nx, int ny, int tileOutW,
    const unsigned *xTable, const unsigned *yTable, hipStream_t stream) {
	if (nx < 1 || ny < 1) throw std::invalid_argument("tile_stitch_state: 1 .. 64 tiles");
	checkTileSet("tile_stitch_state", states, nx * ny, 16);
	if (dst16 == nullptr || reinterpret_cast<std::uintptr_t>(dst16) % 16) {
		throw std::invalid_argument("tile_stitch_state: the 16-bit frame is NULL or not 16-byte aligned");
	}
	if (outW < 4 || outW % 4 || outH < 1 || tileOutW < 4 || tileOutW % 4) {
		throw std::invalid_argument("tile_stitch_state: widths must be multiples of four pixels");
	}
	if (xTable == nullptr || yTable == nullptr || reinterpret_cast<std::uintptr_t>(xTable) % 16) {
		throw std::invalid_argument("tile_stitch_state: NULL table, or an x table that is not 16-byte aligned");
	}
	// memory-bound: about 2048 workgroups at the most, which stride over the rows
	const unsigned gx = (static_cast<unsigned>(outW) / 4 + 63) / 64;
	const unsigned rows = (static_cast<unsigned>(outH) + 3) / 4;
	const unsigned cap = gx < 2048u ? 2048u / gx : 1u;
	const dim3 grid(gx, rows < cap ? rows : cap);
	hipLaunchKernelGGL(tile_stitch_state_kernel, grid, dim3(64, 4), 0, stream, dst16, outW, outH, states, nx, nx * ny, tileOutW,
	    xTable, yTable);
	hipCheckLaunch("tile_stitch_state");
}

namespace {
// what both fused launches check, and the scaler's tile in LDS behind the 1 KB of tile pointers and origins
struct StitchScaleLaunch {
	dim3 grid;
	std::size_t lds;
	int pitch;
};
StitchScaleLaunch stitchScaleLaunch(const std::string &who, const void *dst, int dstW, int dstH, int outW, int outH, const TileSet &tiles,
    int nx, int ny, int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y,
    int spanX) {
	if (nx < 1 || ny < 1) throw std::invalid_argument(who + ": 1 .. 64 tiles");
	checkTileSet(who.c_str(), tiles, nx * ny, 16);
	if (dst == nullptr || dstW < 1 || dstH < 1) throw std::invalid_argument(who + ": NULL or empty destination");
	if (outW < 4 || outW % 4 || outH < 1 || tileOutW < 4 || tileOutW % 4) {
		throw std::invalid_argument(who + ": widths must be multiples of four pixels");
	}
	if (xTable == nullptr || yTable == nullptr || reinterpret_cast<std::uintptr_t>(xTable) % 16) {
		throw std::invalid_argument(who + ": NULL table, or an x table that is not 16-byte aligned");
	}
	if (x.start == nullptr || x.taps == nullptr || y.start == nullptr || y.taps == nullptr || spanX < 4 || spanX % 4) {
		throw std::invalid_argument(who + ": bad scaler tables");
	}
	if (x.filter != y.filter) throw std::invalid_argument(who + ": the two axes' tables must be of one filter");
	StitchScaleLaunch l;
	l.pitch = spanX + spanX / 32 + 1;
	l.lds = static_cast<std::size_t>(3) * kScaleTileH * static_cast<std::size_t>(l.pitch) * sizeof(unsigned);
	constexpr std::size_t kTilesLds = kTileMax * (sizeof(void *) + 2 * sizeof(int));
	if (l.lds + kTilesLds > 64 * 1024) throw std::invalid_argument(who + ": the tile does not fit the LDS");
	l.grid = dim3(static_cast<unsigned>((dstW + kScaleTileW - 1) / kScaleTileW), static_cast<unsigned>((dstH + kScaleTileH - 1) / kScaleTileH));
	return l;
}
}  // namespace

void launchTileStitchScale(std::uint8_t *dst, std::ptrdiff_t dstStride, int dstW, int dstH, int outW, int outH, const TileSet &tiles,
    int nx, int ny, int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y,
    int spanX, hipStream_t stream) {
	const StitchScaleLaunch l = stitchScaleLaunch("tile_stitch_scale", dst, dstW, dstH, outW, outH, tiles, nx, ny, tileOutW, xTable, yTable,
	    x, y, spanX);
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	const auto kernel = x.filter != kScaleTriangle ? tile_stitch_scale_kernel<true> : tile_stitch_scale_kernel<false>;
	hipLaunchKernelGGL(kernel, l.grid, dim3(256), l.lds, stream, dst, dstStride, dstW, dstH, outW, tiles, nx, nx * ny, tileOutW, xTable,
	    yTable, tx, ty, l.pitch);
	hipCheckLaunch("tile_stitch_scale");
}

void launchTileStitchScaleState(std::uint16_t *dst16, int dstW, int dstH, int outW, int outH, const TileSet &states, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX,
    hipStream_t stream) {
	const StitchScaleLaunch l = stitchScaleLaunch("tile_stitch_scale_state", dst16, dstW, dstH, outW, outH, states, nx, ny, tileOutW,
	    xTable, yTable, x, y, spanX);
	if (reinterpret_cast<std::uintptr_t>(dst16) % 8) throw std::invalid_argument("tile_stitch_scale_state: the 16-bit frame is not 8-byte aligned");
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	const auto kernel = x.filter != kScaleTriangle ? tile_stitch_scale_state_kernel<true> : tile_stitch_scale_state_kernel<false>;
	hipLaunchKernelGGL(kernel, l.grid, dim3(256), l.lds, stream, dst16, dstW, dstH, outW, states, nx, nx * ny, tileOutW, xTable, yTable,
	    tx, ty, l.pitch);
	hipCheckLaunch("tile_stitch_scale_state");
}

namespace {
// what both masked launches check: the rows, the 32-bit texel arithmetic, and the box inside the blended frame -- whose
// pixels' source texels (X >> 2, Y >> 2) then lie inside the source of outW / 4 x outH / 4
void checkTileMask(const std::string &who, const TileMask &m, int outW, int outH) {
	if (outW < 4 || outW % 4 || outH < 4 || outH % 4) throw std::invalid_argument(who + ": the blended frame must be four times a source");
	checkRows(who.c_str(), m.src, m.srcStride);
	checkRows(who.c_str(), m.mask, m.maskStride);
	if (m.maskW < 1 || m.maskH < 1) throw std::invalid_argument(who + ": empty mask");
	const auto below32 = [](int out, int tex) { return 2ull * static_cast<unsigned>(out) * static_cast<unsigned>(tex) < (1ull << 32); };
	if (!below32(outW, m.maskW) || !below32(outH, m.maskH)) {
		throw std::invalid_argument(who + ": 2 x blended extent x mask extent must stay below 2^32");
	}
	if (m.x0 < 0 || m.y0 < 0 || m.x0 > m.x1 || m.y0 > m.y1 || m.x1 > outW || m.y1 > outH) {
		throw std::invalid_argument(who + ": the mask's box lies outside the blended frame");
	}
}
}  // namespace

void launchTileStitchMask(std::uint8_t *dst, std::ptrdiff_t dstStride, int outW, int outH, const TileSet &tiles, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, const TileMask &mask, hipStream_t stream) {
	if (nx < 1 || ny < 1) throw std::invalid_argument("tile_stitch_mask: 1 .. 64 tiles");
	checkTileSet("tile_stitch_mask", tiles, nx * ny, 16);
	checkRows("tile_stitch_mask", dst, dstStride);
	if (outW < 1 || outH < 1 || tileOutW < 1 || xTable == nullptr || yTable == nullptr) {
		throw std::invalid_argument("tile_stitch_mask: empty frame or NULL table");
	}
	checkTileMask("tile_stitch_mask", mask, outW, outH);
	// (tile_stitch_kernel's grid)
	const unsigned groups = static_cast<unsigned>(outW) / 4 + 2;
	const unsigned rows = (static_cast<unsigned>(outH) + 3) / 4;
	const dim3 grid((groups + 63) / 64, rows < 65535u ? rows : 65535u);
	hipLaunchKernelGGL(tile_stitch_mask_kernel, grid, dim3(64, 4), 0, stream, dst, dstStride, outW, outH, tiles, nx, tileOutW, xTable,
	    yTable, mask);
	hipCheckLaunch("tile_stitch_mask");
}

void launchTileStitchMaskScale(std::uint8_t *dst, std::ptrdiff_t dstStride, int dstW, int dstH, int outW, int outH, const TileSet &tiles,
    int nx, int ny, int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y,
    int spanX, const TileMask &mask, hipStream_t stream) {
	// (the 1 KB of tile pointers and origins in LDS is counted with the scaler's tile: stitchScaleLaunch)
	const StitchScaleLaunch l = stitchScaleLaunch("tile_stitch_mask_scale", dst, dstW, dstH, outW, outH, tiles, nx, ny, tileOutW, xTable,
	    yTable, x, y, spanX);
	checkTileMask("tile_stitch_mask_scale", mask, outW, outH);
	const ScaleTaps tx{x.start, x.taps}, ty{y.start, y.taps};
	const auto kernel = x.filter != kScaleTriangle ? tile_stitch_mask_scale_kernel<true> : tile_stitch_mask_scale_kernel<false>;
	hipLaunchKernelGGL(kernel, l.grid, dim3(256), l.lds, stream, dst, dstStride, dstW, dstH, outW, outH, tiles, nx, nx * ny, tileOutW,
	    xTable, yTable, tx, ty, l.pitch, mask);
	hipCheckLaunch("tile_stitch_mask_scale");
}

}  // namespace ju
