// The scene detector's memory and clock (docs/scene_detect.md), once, for every owner of a detector: an Engine on its
// model-size input, a TiledRuntime on its source-size frame.  The owner validates the setting under its own name, waits
// for its own stream, launches the kernels and keeps whatever hangs on the buffers below (the graphs of passes that carry
// the detector; the tiled clear's table); the detector keeps the buffers, the counts and the arithmetic between them.
#pragma once

#include <cstddef>
#include <cstdint>

#include "hip_util.h"
#include "kernels.h"
#include "scene_clock.h"

namespace ju {

static_assert(SceneClock::kSceneRing == kSceneRing, "the clock's ring is the kernels' ring");

class SceneDetector {
public:
	int mode() const { return m_Mode; }
	std::uint32_t threshold() const { return m_Threshold; }
	const SceneClock &clock() const { return m_Clock; }
	// The setting, already validated (sceneDetectProblem) and behind the owner's wait for its stream.  The same mode: the
	// threshold alone, the memory stays, false.  Another mode is a start, true: the totals of the period that ends are kept,
	// the memory is replaced by fresh (zeroed) memory for a kept frame of `keptBytes` -- none while the mode is off -- and
	// the clock starts over.  Whatever is bound to the old buffers must have been dropped by the owner before.
	bool configure(int mode, std::uint32_t thresholdMilli, std::size_t keptBytes) {
		if (mode == m_Mode) {
			if (mode != 0) m_Threshold = thresholdMilli;
			return false;
		}
		DeviceBuffer prev, state;
		PinnedWords ring;
		if (mode != 0) {  // (made first: a failure leaves the detector as it was)
			prev = DeviceBuffer(keptBytes);
			state = DeviceBuffer(sizeof(SceneState));
			ring = PinnedWords(sizeof(SceneRecord) * (kSceneRing + 1));
		}
		m_FramesBase = total(false);
		m_CutsBase = total(true);
		m_Prev = std::move(prev);
		m_State = std::move(state);
		m_Ring = std::move(ring);
		m_Mode = mode;
		m_Threshold = mode != 0 ? thresholdMilli : 0;
		m_Clock.start();
		return true;
	}
	void restart() { m_Clock.restart(); }  // the owner's reset(): no predecessor; setting and step count stay
	void advance(std::uint64_t n = 1) { m_Clock.advance(n); }  // n steps have been enqueued
	// the last min(count, kSceneRing, steps seen) decisions, oldest first; returns how many.  The owner has waited for its stream.
	int records(SceneRecord *out, int count) const {
		if (m_Mode == 0 || m_Ring.host() == nullptr) return 0;
		const SceneClock::Window w = m_Clock.window(count);
		for (int k = 0; k < w.count; ++k) {
			const volatile SceneRecord &r = record(w.first + static_cast<std::uint64_t>(k));
			out[k].step = r.step;
			out[k].sad = r.sad;
			out[k].score = r.score;
			out[k].cut = r.cut;
			out[k].reserved = 0;
		}
		return w.count;
	}
	// "scene_frames" / "scene_cuts": cumulative over the on-periods, as of the decisions that have completed (the totals
	// record behind the ring, which the decision writes to host-mapped memory: no synchronisation)
	std::uint64_t total(bool cuts) const {
		if (m_Ring.host() == nullptr) return cuts ? m_CutsBase : m_FramesBase;
		const volatile SceneRecord *totals = reinterpret_cast<const volatile SceneRecord *>(m_Ring.host()) + kSceneRing;
		return cuts ? m_CutsBase + totals->sad : m_FramesBase + totals->step;
	}
	// whether the completed step `step`, one of the last kSceneRing, was a cut
	bool cutAt(std::uint64_t step) const { return record(step).cut != 0; }
	// the device addresses a launch takes
	std::uint32_t *prev() const { return m_Prev.as<std::uint32_t>(); }
	SceneState *state() const { return m_State.as<SceneState>(); }
	SceneRecord *ring() const { return reinterpret_cast<SceneRecord *>(m_Ring.device()); }
	// the next step's launch: memory, slot, step, predecessor bits and threshold (src, size and resetMode: the owner's)
	void fill(SceneSadLaunch &q) const {
		q.prev = prev();
		q.state = state();
		q.ring = ring();
		q.slot = m_Clock.slot();
		q.step = m_Clock.steps;
		q.hasPrev = m_Clock.hasPrev();
		q.thresholdMilli = m_Threshold;
	}

private:
	const volatile SceneRecord &record(std::uint64_t step) const {
		return reinterpret_cast<const volatile SceneRecord *>(m_Ring.host())[SceneClock::slotOf(step)];
	}
	int m_Mode = 0;
	std::uint32_t m_Threshold = 0;
	// the kept frame; the SceneState; kSceneRing records and the totals record behind them, host-mapped
	DeviceBuffer m_Prev, m_State;
	PinnedWords m_Ring;
	SceneClock m_Clock;
	std::uint64_t m_FramesBase = 0, m_CutsBase = 0;  // the totals of earlier on-periods
};

}  // namespace ju
