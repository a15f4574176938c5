// joshupscale_amd/csrc/tile_geometry.h alone, on the host (tests/test_tiled_cpu.py builds this with
// -fsanitize=address,undefined and compares what it prints with tests/tiled_reference.py, entry for entry).
// Arguments: groups of five integers "srcW srcH tileW tileH overlap".  Per group: the layout's verdict, and for an
// admitted layout both axes' origins and tables and the split of its tiles into group passes of at most 8.
#include <cstdio>
#include <cstdlib>

#include "tile_geometry.h"

namespace {

void printAxis(const char *name, const ju::TileAxis &a) {
	std::printf("%s origins", name);
	for (int x : a.origin) std::printf(" %d", x);
	std::printf("\n%s table", name);
	for (const ju::TileAxisEntry &e : a.table) std::printf(" %u:%u", static_cast<unsigned>(e.tile), static_cast<unsigned>(e.weight));
	std::printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
	if (argc < 6 || (argc - 1) % 5 != 0) {
		std::printf("usage: tile_geometry (srcW srcH tileW tileH overlap)...\n");
		return 2;
	}
	for (int i = 1; i + 4 < argc; i += 5) {
		const long sw = std::atol(argv[i]), sh = std::atol(argv[i + 1]), w = std::atol(argv[i + 2]), h = std::atol(argv[i + 3]);
		const long ov = std::atol(argv[i + 4]);
		std::printf("case %ld %ld %ld %ld %ld\n", sw, sh, w, h, ov);
		const std::string problem = ju::tileLayoutProblem(static_cast<std::size_t>(sw), static_cast<std::size_t>(sh),
		    static_cast<std::size_t>(w), static_cast<std::size_t>(h), ov);
		if (!problem.empty()) {
			std::printf("refused %s\n", problem.c_str());
			continue;
		}
		const ju::TileAxis x = ju::tileAxis(sw, w, ov), y = ju::tileAxis(sh, h, ov);
		printAxis("x", x);
		printAxis("y", y);
		const ju::TilePasses p = ju::tilePasses(x.tiles() * y.tiles(), 8);
		std::printf("passes");
		for (int k = 0; k < p.passes; ++k) std::printf(" %d+%d", p.begin(k), p.count(k));
		std::printf("\n");
	}
	return 0;
}
