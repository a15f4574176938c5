// ju::tilePassPlan and ju::clampTilePassCap (joshupscale_amd/csrc/tile_pass_plan.h) alone, on the host
// (tests/test_tiled_pass_cpu.py builds this with -fsanitize=address,undefined and compares what it prints with
// tests/tiled_pass_reference.py plan).  Argument: a file of cases, each two 32-bit integers -- count, cap -- followed by
// count x count bytes, the clash matrix row-major (byte [i][j] != 0 for i < j: frames i and j cannot share a pass), in an
// allocation of exactly that size (so a read outside the matrix is the sanitizer's).  Per case one line: the frames at
// which passes start ("-" for none).  Then "clamp F: C" for a few caps.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tile_pass_plan.h"

int main(int argc, char **argv) {
	if (argc != 2) {
		std::printf("usage: tile_pass_plan cases.bin\n");
		return 2;
	}
	std::FILE *f = std::fopen(argv[1], "rb");
	if (f == nullptr) return 2;
	std::int32_t head[2];
	while (std::fread(head, sizeof(head), 1, f) == 1) {
		const int count = head[0], cap = head[1];
		if (count < 0 || count > 4096) return 2;
		const std::size_t n = static_cast<std::size_t>(count);
		std::vector<std::uint8_t> clash(n * n);
		if (!clash.empty() && std::fread(clash.data(), 1, clash.size(), f) != clash.size()) return 2;
		const std::vector<int> starts = ju::tilePassPlan(count, cap, [&](int i, int j) {
			if (i < 0 || i >= j || j >= count) std::abort();  // only earlier frames of the call are asked about
			return clash.at(static_cast<std::size_t>(i) * n + static_cast<std::size_t>(j)) != 0;
		});
		if (starts.empty()) std::printf("-");
		for (std::size_t k = 0; k < starts.size(); ++k) std::printf(k ? " %d" : "%d", starts[k]);
		std::printf("\n");
	}
	std::fclose(f);
	for (int frames : {-3, 0, 1, 2, 8, 9, 1 << 30}) std::printf("clamp %d: %d\n", frames, ju::clampTilePassCap(frames));
	return 0;
}
