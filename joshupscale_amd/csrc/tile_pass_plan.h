// Where the look-ahead passes of a tiled call start (docs/tiled.md "Look-ahead passes"; tests/tiled_pass_reference.py plan).
// A call of `count` consecutive frames runs as consecutive passes of at most `cap` frames.  A pass reads every source of
// its frames up front and writes its outputs frame by frame behind that, so frame j may not share a pass with an EARLIER
// frame i of it that it clashes with -- an input plane of one over an output plane of the other, in one address space.
// The plan is greedy: frame j starts a new pass when the running pass is full or holds a frame that clashes with j.  A
// function of count, the cap and the clash relation alone.  Plain C++: no HIP.
#pragma once

#include <vector>

namespace ju {

constexpr int kTilePassMax = 8;  // frames of one pass at most (the flow net's look-ahead cap, kFlowBatchMax)

inline int clampTilePassCap(int frames) { return frames < 1 ? 1 : (frames > kTilePassMax ? kTilePassMax : frames); }

// The indices at which passes start, ascending, the first 0; empty for count <= 0.  clash(i, j), asked for i < j only:
// whether frames i and j cannot share a pass.  A cap below 1 counts as 1.
template <typename Clash>
std::vector<int> tilePassPlan(int count, int cap, Clash &&clash) {
	std::vector<int> starts;
	if (count <= 0) return starts;
	if (cap < 1) cap = 1;
	int start = 0;
	starts.push_back(0);
	for (int j = 1; j < count; ++j) {
		bool fresh = j - start >= cap;
		for (int i = start; i < j && !fresh; ++i) fresh = clash(i, j);
		if (fresh) {
			start = j;
			starts.push_back(j);
		}
	}
	return starts;
}

}  // namespace ju
