// ju::maskBox and ju::maskSizeProblem (joshupscale_amd/csrc/mask_box.h) alone, on the host (tests/test_tiled_mask_cpu.py
// builds this with -fsanitize=address,undefined and compares what it prints with tests/tiled_mask_reference.py box).
// Argument: a file of cases, each five 32-bit integers -- MW, MH, stride in bytes (negative: bottom-up), B, Bh -- followed
// by |stride| x MH bytes, the mask's rows in MEMORY order, in an allocation of exactly that size (so a read outside the
// rows is the sanitizer's).  Per case one line "x0 y0 x1 y1".  Then "problem MW MH B Bh: <text>" for a few sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mask_box.h"

int main(int argc, char **argv) {
	if (argc != 2) {
		std::printf("usage: mask_box cases.bin\n");
		return 2;
	}
	std::FILE *f = std::fopen(argv[1], "rb");
	if (f == nullptr) return 2;
	std::int32_t head[5];
	while (std::fread(head, sizeof(head), 1, f) == 1) {
		const int maskW = head[0], maskH = head[1], stride = head[2], outW = head[3], outH = head[4];
		const std::size_t pitch = static_cast<std::size_t>(std::abs(stride));
		if (maskW < 1 || maskH < 1 || pitch < static_cast<std::size_t>(maskW) * 4 || outW < 1 || outH < 1) return 2;
		if (!ju::maskSizeProblem(static_cast<std::size_t>(maskW), static_cast<std::size_t>(maskH), static_cast<std::size_t>(outW),
		        static_cast<std::size_t>(outH)).empty()) return 2;
		std::vector<std::uint8_t> rows(pitch * static_cast<std::size_t>(maskH));
		if (std::fread(rows.data(), 1, rows.size(), f) != rows.size()) return 2;
		const std::uint8_t *first = stride >= 0 ? rows.data() : rows.data() + pitch * static_cast<std::size_t>(maskH - 1);
		const ju::MaskBox b = ju::maskBox(first, stride, maskW, maskH, outW, outH);
		if (b.empty() != (b.x0 == 0 && b.y0 == 0 && b.x1 == 0 && b.y1 == 0)) return 1;  // empty is all 0, and nothing else is
		std::printf("%d %d %d %d\n", b.x0, b.y0, b.x1, b.y1);
	}
	std::fclose(f);
	const std::size_t sizes[][4] = {{1, 1, 4, 4}, {16384, 16384, 1536, 960}, {0, 5, 400, 280}, {7, 16385, 400, 280},
	    {16384, 5, 131072, 280}, {16384, 5, 131071, 280}, {7, 16384, 400, 131072}, {7, 5, 4294967296ull, 280}};
	for (const auto &s : sizes) {
		std::printf("problem %zu %zu %zu %zu: %s\n", s[0], s[1], s[2], s[3], ju::maskSizeProblem(s[0], s[1], s[2], s[3]).c_str());
	}
	return 0;
}
