// ju::SceneClock (joshupscale_amd/csrc/scene_clock.h) alone, on the host (tests/test_cxx_scene_clock.py builds this with
// -fsanitize=address,undefined and compares what it prints with its own arithmetic and tests/scene_reference.py Detector).
// Standard input: a script of operations, one per token group --
//   s        one detector step:   prints "step <record step> <ring slot> <has-predecessor bits> <memory>", then advance()
//   a <n>    a pass of n steps:   prints "pass <n> <first record step> <ring slot> <bits> <memory>", then advance(n)
//   r        restart()
//   n        start()
//   q <c>    a query for c records: prints "window <c>:" and the steps it returns, oldest first
// Every slot is also used as an index into an array of exactly kSceneRing elements, so one outside it is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scene_clock.h"

int main() {
	ju::SceneClock clock;
	std::vector<std::uint64_t> ring(static_cast<std::size_t>(ju::SceneClock::kSceneRing), 0);
	char op;
	while (std::scanf(" %c", &op) == 1) {
		if (op == 's') {
			std::printf("step %llu %d %d %u\n", static_cast<unsigned long long>(clock.steps), clock.slot(), clock.hasPrev(), clock.memory());
			ring[static_cast<std::size_t>(clock.slot())] = clock.steps;
			clock.advance();
		} else if (op == 'a') {
			int n = 0;
			if (std::scanf("%d", &n) != 1 || n < 1) return 2;
			std::printf("pass %d %llu %d %d %u\n", n, static_cast<unsigned long long>(clock.steps), clock.slot(), clock.hasPrev(), clock.memory());
			for (int i = 0; i < n; ++i) {
				const std::uint64_t step = clock.steps + static_cast<std::uint64_t>(i);
				ring[static_cast<std::size_t>(ju::SceneClock::slotOf(step))] = step;
			}
			clock.advance(static_cast<std::uint64_t>(n));
		} else if (op == 'r') {
			clock.restart();
		} else if (op == 'n') {
			clock.start();
		} else if (op == 'q') {
			int count = 0;
			if (std::scanf("%d", &count) != 1) return 2;
			const ju::SceneClock::Window w = clock.window(count);
			std::printf("window %d:", count);
			for (int k = 0; k < w.count; ++k) {
				// (read back through the ring, as SceneDetector::records does: the slot still holds that step)
				const std::uint64_t step = w.first + static_cast<std::uint64_t>(k);
				if (ring[static_cast<std::size_t>(ju::SceneClock::slotOf(step))] != step) return 1;
				std::printf(" %llu", static_cast<unsigned long long>(step));
			}
			std::printf("\n");
		} else {
			return 2;
		}
	}
	std::printf("scene_clock ok\n");
	return 0;
}
