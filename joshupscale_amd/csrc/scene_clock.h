// The scene detector's clock (docs/scene_detect.md "The clock"; tests/scene_reference.py Detector): how many steps the
// detector has taken, and everything derived from those two counts -- the record's step, its ring slot, the "has
// predecessor" bits of the decision and the steps a query for the last records returns.  One definition for every owner
// of a detector (scene_detector.h).  Plain C++: no HIP (tests/cxx/scene_clock.cpp).
#pragma once

#include <cstdint>

namespace ju {

struct SceneClock {
	// the records kept: kernels.h's ring of that name (scene_detector.h asserts the two are one number)
	static constexpr int kSceneRing = 64;

	std::uint64_t seen = 0;   // steps since the last start or restart: the frames in the detector's memory
	std::uint64_t steps = 0;  // steps since the last start: the next record's `step`

	void start() { seen = steps = 0; }  // a mode change: no predecessor, step 0
	void restart() { seen = 0; }        // a reset of the owner: no predecessor; the step count goes on
	void advance(std::uint64_t n = 1) {
		seen += n;
		steps += n;
	}
	// of the next step -- bit 0: frame t-1 is in the detector's memory, bit 1: frame t-2 is
	int hasPrev() const { return (seen >= 1 ? 1 : 0) | (seen >= 2 ? 2 : 0); }
	// the same as a count: 0, 1, or 2 for two and more (ScenePassDyn::seen)
	unsigned memory() const { return static_cast<unsigned>(seen < 2 ? seen : 2); }
	static int slotOf(std::uint64_t step) { return static_cast<int>(step % kSceneRing); }
	int slot() const { return slotOf(steps); }  // of the next step
	// the last min(count, kSceneRing, steps) steps, oldest first: [first, first + count)
	struct Window {
		std::uint64_t first;
		int count;
	};
	Window window(int count) const {
		std::uint64_t n = steps < static_cast<std::uint64_t>(kSceneRing) ? steps : static_cast<std::uint64_t>(kSceneRing);
		if (count < 0) count = 0;
		if (static_cast<std::uint64_t>(count) < n) n = static_cast<std::uint64_t>(count);
		return Window{steps - n, static_cast<int>(n)};
	}
};

}  // namespace ju
