// The layout of tiled upscaling (docs/tiled.md; tests/tiled_reference.py is the definition), free of HIP and of the
// engine: where the tiles of one axis begin, and per output coordinate which tile covers it and how much of the next
// one is blended in.  Header-only; a host program tests it alone (tests/cxx/tile_geometry.cpp).
//
// Per axis: S the source length, t the tile (model) length, ov the overlap in source pixels; the scale is 4.
//   tiles    n = 1 if S == t, else ceil((S - ov) / (t - ov))
//   origins  x_i = floor(i (S - t) / (n - 1)); neighbours overlap by L_i = x_i + t - x_{i+1} >= ov
//   seam i   a ramp of R = 4 ov output pixels from r0_i = 4 x_{i+1} + floor((4 L_i - R) / 2): tile i alone in front of it,
//            tile i + 1 alone behind it, inside it at d = X - r0_i the weight q = ((2 d + 1) 256 + R) / (2 R) for tile
//            i + 1 and 256 - q for tile i.  ov = 0: a hard cut at r0_i.
// The bound ov <= t / 4 keeps consecutive ramps apart: no output coordinate needs three tiles of an axis.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ju {

constexpr int kTileScale = 4;
constexpr int kTileMax = 64;       // tiles of one frame
constexpr int kTileRatioMax = 8;   // source length / tile length, per axis

// One output coordinate: the first tile that covers it, and the weight 0 .. 256 of the tile behind that one (0: the first
// tile alone -- the tile behind it need not exist).  The device reads the table as 32-bit words: tile | weight << 16.
struct TileAxisEntry {
	std::uint16_t tile, weight;
};
static_assert(sizeof(TileAxisEntry) == 4, "the kernels read the table as 32-bit words");

struct TileAxis {
	std::vector<int> origin;           // [tiles], source pixels
	std::vector<TileAxisEntry> table;  // [4 S]
	int tiles() const { return static_cast<int>(origin.size()); }
};

// (the caller has checked the limits: tileLayoutProblem)
inline std::vector<int> tileOrigins(long S, long t, long ov) {
	if (S == t) return {0};
	const long n = (S - ov + (t - ov) - 1) / (t - ov);
	std::vector<int> x(static_cast<std::size_t>(n));
	for (long i = 0; i < n; ++i) x[static_cast<std::size_t>(i)] = static_cast<int>(i * (S - t) / (n - 1));
	return x;
}

// Ownership (docs/tiled.md "Scene cuts"): what counts every source coordinate of an axis exactly once although tiles
// overlap -- and three of them may cover one coordinate (t = 48, ov = 7, S = 90: origins 0, 21, 42).  Tile i owns
// [x_i, x_{i+1}), the last tile up to S; the interval lies inside the tile because neighbours overlap (L_i >= 0).
// Returns the intervals' ends, one per tile.
inline std::vector<int> tileOwnedEnds(const std::vector<int> &origin, long S) {
	std::vector<int> end(origin.size());
	for (std::size_t i = 0; i < origin.size(); ++i) end[i] = i + 1 < origin.size() ? origin[i + 1] : static_cast<int>(S);
	return end;
}

inline TileAxis tileAxis(long S, long t, long ov) {
	TileAxis a;
	a.origin = tileOrigins(S, t, ov);
	const int n = a.tiles();
	a.table.assign(static_cast<std::size_t>(kTileScale * S), TileAxisEntry{0, 0});
	const long R = kTileScale * ov;
	long begin = 0;  // the first coordinate tile i has alone
	for (int i = 0; i + 1 < n; ++i) {
		const long L = a.origin[i] + t - a.origin[i + 1];
		const long r0 = kTileScale * static_cast<long>(a.origin[i + 1]) + (kTileScale * L - R) / 2;
		for (long X = begin; X < r0; ++X) a.table[static_cast<std::size_t>(X)] = {static_cast<std::uint16_t>(i), 0};
		for (long d = 0; d < R; ++d) {
			const long q = ((2 * d + 1) * 256 + R) / (2 * R);
			a.table[static_cast<std::size_t>(r0 + d)] = {static_cast<std::uint16_t>(i), static_cast<std::uint16_t>(q)};
		}
		begin = r0 + R;
	}
	for (long X = begin; X < kTileScale * S; ++X) a.table[static_cast<std::size_t>(X)] = {static_cast<std::uint16_t>(n - 1), 0};
	return a;
}

// "" when a source of srcW x srcH may be tiled by a model of w x h at overlap ov, else what is wrong
inline std::string tileLayoutProblem(std::size_t srcW, std::size_t srcH, std::size_t w, std::size_t h, long ov) {
	const long most = static_cast<long>((w < h ? w : h) / 4);
	if (w == 0 || h == 0) return "the model has no frame size";
	if (ov < 0 || ov > most) return "overlap " + std::to_string(ov) + " outside 0 .. " + std::to_string(most);
	if (srcW < w || srcH < h || srcW > kTileRatioMax * w || srcH > kTileRatioMax * h) {
		return "source size " + std::to_string(srcW) + "x" + std::to_string(srcH) + " outside " + std::to_string(w) + "x" +
		       std::to_string(h) + " .. " + std::to_string(kTileRatioMax * w) + "x" + std::to_string(kTileRatioMax * h);
	}
	const std::size_t nx = tileOrigins(static_cast<long>(srcW), static_cast<long>(w), ov).size();
	const std::size_t ny = tileOrigins(static_cast<long>(srcH), static_cast<long>(h), ov).size();
	if (nx * ny > static_cast<std::size_t>(kTileMax)) {
		return std::to_string(nx) + "x" + std::to_string(ny) + " tiles are more than " + std::to_string(kTileMax);
	}
	return "";
}

// A call of more than `cap` tiles runs as several group passes: the fewest passes that hold them, filled evenly, so that
// no pass is left with a single tile (which would run outside the passes).  Pass p holds tiles begin(p) .. begin(p) + count(p) - 1.
struct TilePasses {
	int passes, base, larger;  // `larger` passes of base + 1 tiles, then passes of base
	int begin(int p) const { return p * base + (p < larger ? p : larger); }
	int count(int p) const { return base + (p < larger ? 1 : 0); }
};
inline TilePasses tilePasses(int tiles, int cap) {
	const int passes = (tiles + cap - 1) / cap;
	return {passes, tiles / passes, tiles % passes};
}

}  // namespace ju
