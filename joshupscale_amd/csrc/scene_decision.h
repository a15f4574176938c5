// The scene detector's decision (docs/scene_detect.md; tests/scene_reference.py `decide`), once, for the kernels that sum
// one frame against one kept frame: scene_sad_kernel (scene_kernels.hip) and tile_split_scene_kernel (tile_kernels.hip).
// Device code only; both include it behind kernels.h.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace ju {

// What the thread that drew the launch's LAST ticket does (every workgroup has added its sum to st->acc and released it
// before its ticket; the caller has drawn the ticket): acquire, read S and re-arm the accumulator and the ticket,
// D_t = min(S_t, |S_t - S_{t-1}|), cut_t = 1000 D_t >= threshold_milli N with N = 3 pixels, the record into ring[slot],
// the cumulative counters behind the ring, SceneState::resetNow = cut && resetMode.
__device__ __forceinline__ void sceneDecide(SceneState *st, SceneRecord *ring, int slot, unsigned long long step, int hasPrev,
    unsigned thresholdMilli, int resetMode, long long pixels) {
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	// read the sum and re-arm the accumulator in one atomic; then the ticket
	unsigned long long S = __hip_atomic_exchange(&st->acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (!(hasPrev & 1)) S = 0;  // no predecessor: what the kept frame held is not a frame of this stream
	unsigned long long D = 0;
	if ((hasPrev & 3) == 3) {
		const unsigned long long before = st->prevSad;
		const unsigned long long delta = S > before ? S - before : before - S;
		D = S < delta ? S : delta;
	}
	const unsigned long long N = 3ull * static_cast<unsigned long long>(pixels);
	const unsigned cut = 1000ull * D >= static_cast<unsigned long long>(thresholdMilli) * N ? 1u : 0u;
	st->prevSad = S;
	st->frames += 1;
	st->cuts += cut;
	st->resetNow = (cut && resetMode) ? 1u : 0u;
	SceneRecord *r = ring + slot;
	__hip_atomic_store(&r->step, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->sad, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->score, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->cut, cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	// the cumulative counters, behind the ring's 64 records (ju_get_stat reads them without a synchronisation)
	SceneRecord *totals = ring + kSceneRing;
	__hip_atomic_store(&totals->step, st->frames, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&totals->sad, st->cuts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace ju
