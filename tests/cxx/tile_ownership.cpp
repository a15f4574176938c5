// ju::tileOwnedEnds (joshupscale_amd/csrc/tile_geometry.h) alone, on the host (tests/test_tiled_scene_cpu.py builds this with
// -fsanitize=address,undefined and compares what it prints with tests/tiled_scene_reference.py).
// Arguments: tile lengths t.  Per t, for every overlap ov <= t / 4 and every source length t <= S <= 8 t, the ownership
// intervals [x_i, end_i) are checked here to partition [0, S) and to lie inside their tiles (exit status 1 otherwise), and
// one line "t ov sum tiles" is printed: sum = the sum over S and i of (end_i + 1) (i + 1) (S + 7), tiles = the sum of the
// tile counts -- what the Python restatement must reproduce.  Then, per t, the intervals of S = 2 t - 6 at ov = 7 t / 48
// written out ("example t ov S x:end ...").
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tile_geometry.h"

int main(int argc, char **argv) {
	if (argc < 2) {
		std::printf("usage: tile_ownership t...\n");
		return 2;
	}
	for (int a = 1; a < argc; ++a) {
		const long t = std::atol(argv[a]);
		if (t < 4 || t > 8192) return 2;
		for (long ov = 0; ov <= t / 4; ++ov) {
			unsigned long long sum = 0, tiles = 0;
			for (long S = t; S <= ju::kTileRatioMax * t; ++S) {
				const std::vector<int> x = ju::tileOrigins(S, t, ov);
				const std::vector<int> end = ju::tileOwnedEnds(x, S);
				if (end.size() != x.size() || x.empty() || x[0] != 0 || end.back() != S) return 1;
				for (std::size_t i = 0; i < x.size(); ++i) {
					if (end[i] < x[i] || end[i] > x[i] + t) return 1;                 // inside its tile
					if (i + 1 < x.size() && end[i] != x[i + 1]) return 1;               // the next interval begins where this one ends
					sum += static_cast<unsigned long long>(end[i] + 1) * (i + 1) * static_cast<unsigned long long>(S + 7);
				}
				tiles += x.size();
			}
			std::printf("%ld %ld %llu %llu\n", t, ov, sum, tiles);
		}
		const long ov = t * 7 / 48, S = 2 * t - 6;
		const std::vector<int> x = ju::tileOrigins(S, t, ov);
		const std::vector<int> end = ju::tileOwnedEnds(x, S);
		std::printf("example %ld %ld %ld", t, ov, S);
		for (std::size_t i = 0; i < x.size(); ++i) std::printf(" %d:%d", x[i], end[i]);
		std::printf("\n");
	}
	return 0;
}
