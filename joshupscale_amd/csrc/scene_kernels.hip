// Scene-cut detection on the GPU (docs/scene_detect.md; tests/scene_reference.py is the definition).
//
// scene_sad_kernel: S_t = sum |c_t - c_{t-1}| over the B, G and R bytes of the model-size BGRX frame the step consumes,
// against the kept previous frame, which it overwrites with c_t in the same pass.  Per-thread u32 partials -> wave sum ->
// workgroup sum -> ONE 64-bit integer atomic add per workgroup at agent scope: integer sums do not depend on the order
// of arrival, so S_t is bit-reproducible.  The workgroup that draws the last ticket takes the decision (release in
// every workgroup before its ticket, acquire in the last one behind it; no workgroup ever waits for another):
// D_t = min(S_t, |S_t - S_{t-1}|), cut_t = 1000 D_t >= threshold_milli N, the record into the host-mapped ring, the
// device flag reset_now, and the accumulator and the ticket back to zero for the next launch.
//
// scene_clear_kernel: launched behind it over the recurrent inputs of the step (the half of the state and of the frame
// history its program reads).  Every workgroup loads reset_now once and returns if it is 0; otherwise zeros, written as
// 16-byte vector stores with byte stores for an unaligned head and tail.  The decision never visits the host.
//
// scene_pass_kernel: the detector over the frames of a look-ahead pass in one launch (docs/scene_detect.md "Passes") -- the
// same sums, item against item, and all the decisions in order in the last workgroup.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"
#include "kernels.h"
#include "scene_decision.h"

namespace ju {

namespace {

constexpr int kSadThreads = 256;
// pixels per thread: 4 x 765 per thread and 1024 x 765 per workgroup stay far inside 32 bits
constexpr int kSadPerThread = 4;
constexpr int kSadPerGroup = kSadThreads * kSadPerThread;

__global__ __launch_bounds__(kSadThreads) void scene_sad_kernel(const std::uint8_t *__restrict__ src, long long srcStride,
    int W, long long pixels, std::uint32_t *__restrict__ prev, SceneState *st, SceneRecord *ring, int slot,
    unsigned long long step, int hasPrev, unsigned thresholdMilli, int resetMode) {
	__shared__ unsigned waveSums[kSadThreads / 64];
	// (pixel indices in 32 bits: the launcher admits at most 2^15 x 2^15 = 2^30 pixels, so one 32-bit division per pixel)
	const unsigned base = blockIdx.x * static_cast<unsigned>(kSadPerGroup) + threadIdx.x;
	const unsigned width = static_cast<unsigned>(W), count = static_cast<unsigned>(pixels);
	unsigned partial = 0;
#pragma unroll
	for (int k = 0; k < kSadPerThread; ++k) {
		const unsigned i = base + static_cast<unsigned>(k * kSadThreads);
		if (i < count) {
			const unsigned row = i / width, x = i - row * width;
			const unsigned cur = *reinterpret_cast<const std::uint32_t *>(src + static_cast<long long>(row) * srcStride + x * 4u);
			const unsigned old = prev[i];
			prev[i] = cur;
			// (B, G, R are the three low bytes of the little-endian word; X is not compared)
			partial = __builtin_amdgcn_sad_u8(cur & 0x00ffffffu, old & 0x00ffffffu, partial);
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) partial += __shfl_down(partial, off, 64);
	if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = partial;
	__syncthreads();
	if (threadIdx.x != 0) return;
	unsigned long long groupSum = 0;
#pragma unroll
	for (int w = 0; w < kSadThreads / 64; ++w) groupSum += waveSums[w];
	__hip_atomic_fetch_add(&st->acc, groupSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	// publish the add before the ticket (fence, then its wait, then the ticket: in that order)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const unsigned ticket = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (ticket != gridDim.x - 1) return;
	// ---- the last workgroup of the launch: the decision (scene_decision.h) ----
	sceneDecide(st, ring, slot, step, hasPrev, thresholdMilli, resetMode, pixels);
}

// scene_pass_kernel: scene_sad_kernel over the N frames of a look-ahead pass.  A thread owns its four pixels across ALL
// items -- it reads the kept frame once, walks the items in order (item j against item j - 1) and writes the last item
// over the kept frame -- so no workgroup reads a kept pixel another one writes.  The arithmetic per item is
// scene_sad_kernel's: v_sad_u8 on the three low bytes, u32 partials -> wave sum -> workgroup sum -> one 64-bit integer
// atomic add per item at agent scope; release, ticket, acquire in the last workgroup, which then takes the N decisions
// in order.  What differs between two replays of a captured pass (first step, ring slot, predecessors, threshold) is
// read from the host-mapped ScenePassDyn, by that one thread.
struct ScenePassParams {
	const std::uint8_t *frames[kFlowBatchMax];
	long long strides[kFlowBatchMax];
	int W, resetMode;
	long long pixels;
	std::uint32_t *prev;
	SceneState *st;
	ScenePassState *ps;
	const ScenePassDyn *dyn;
	SceneRecord *ring;
};

template <int N>
__global__ __launch_bounds__(kSadThreads) void scene_pass_kernel(ScenePassParams p) {
	__shared__ unsigned waveSums[N][kSadThreads / 64];
	const unsigned base = blockIdx.x * static_cast<unsigned>(kSadPerGroup) + threadIdx.x;
	const unsigned width = static_cast<unsigned>(p.W), count = static_cast<unsigned>(p.pixels);
	unsigned partial[N];
#pragma unroll
	for (int j = 0; j < N; ++j) partial[j] = 0;
#pragma unroll
	for (int k = 0; k < kSadPerThread; ++k) {
		const unsigned i = base + static_cast<unsigned>(k * kSadThreads);
		if (i < count) {
			const unsigned row = i / width, x = i - row * width;
			unsigned before = p.prev[i];
#pragma unroll
			for (int j = 0; j < N; ++j) {
				const unsigned cur = *reinterpret_cast<const std::uint32_t *>(p.frames[j] + static_cast<long long>(row) * p.strides[j] + x * 4u);
				partial[j] = __builtin_amdgcn_sad_u8(cur & 0x00ffffffu, before & 0x00ffffffu, partial[j]);
				before = cur;
			}
			p.prev[i] = before;
		}
	}
#pragma unroll
	for (int j = 0; j < N; ++j) {
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) partial[j] += __shfl_down(partial[j], off, 64);
		if ((threadIdx.x & 63) == 0) waveSums[j][threadIdx.x >> 6] = partial[j];
	}
	__syncthreads();
	if (threadIdx.x != 0) return;
#pragma unroll
	for (int j = 0; j < N; ++j) {
		unsigned long long groupSum = 0;
#pragma unroll
		for (int w = 0; w < kSadThreads / 64; ++w) groupSum += waveSums[j][w];
		__hip_atomic_fetch_add(&p.ps->acc[j], groupSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	// publish the adds before the ticket (fence, then its wait, then the ticket: in that order)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const unsigned ticket = __hip_atomic_fetch_add(&p.ps->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (ticket != gridDim.x - 1) return;
	// ---- the last workgroup of the launch: the N decisions, in order ----
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const unsigned long long stepBase = __hip_atomic_load(&p.dyn->stepBase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned seen = __hip_atomic_load(&p.dyn->seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned thresholdMilli = __hip_atomic_load(&p.dyn->thresholdMilli, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned slot = __hip_atomic_load(&p.dyn->slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned long long pixelBytes = 3ull * static_cast<unsigned long long>(p.pixels);
	unsigned long long before = p.st->prevSad, frames = p.st->frames, cuts = p.st->cuts;
	int latest = -1;
	unsigned reset = 0;
	for (int j = 0; j < N; ++j) {
		// read the sum and re-arm the accumulator in one atomic
		unsigned long long S = __hip_atomic_exchange(&p.ps->acc[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const unsigned inMemory = seen + static_cast<unsigned>(j);  // frames in the detector's memory in front of item j
		if (inMemory < 1) S = 0;  // no predecessor: what the kept frame held is not a frame of this stream
		unsigned long long D = 0;
		if (inMemory >= 2) {
			const unsigned long long delta = S > before ? S - before : before - S;
			D = S < delta ? S : delta;
		}
		const unsigned cut = 1000ull * D >= static_cast<unsigned long long>(thresholdMilli) * pixelBytes ? 1u : 0u;
		before = S;
		frames += 1;
		cuts += cut;
		reset = (cut && p.resetMode) ? 1u : 0u;
		if (reset) latest = j;
		p.ps->resetAt[j] = reset;
		p.ps->cutAt[j] = latest;
		SceneRecord *r = p.ring + (slot + static_cast<unsigned>(j)) % static_cast<unsigned>(kSceneRing);
		__hip_atomic_store(&r->step, stepBase + static_cast<unsigned long long>(j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&r->sad, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&r->score, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&r->cut, cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	__hip_atomic_store(&p.ps->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	p.st->prevSad = before;
	p.st->frames = frames;
	p.st->cuts = cuts;
	p.st->resetNow = reset;  // (the last item's; the per-frame detector sets it anew in front of every clear that reads it)
	SceneRecord *totals = p.ring + kSceneRing;
	__hip_atomic_store(&totals->step, frames, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&totals->sad, cuts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int N>
void launchScenePassN(const ScenePassParams &p, unsigned groups, hipStream_t stream) {
	hipLaunchKernelGGL(scene_pass_kernel<N>, dim3(groups), dim3(kSadThreads), 0, stream, p);
}

// scene_group_kernel: scene_sad_kernel over the n INDEPENDENT items of a group pass (Engine::processGroup) in one launch.
// blockIdx.y is the item: member y's frame against member y's own kept frame, which the same thread rewrites; the sums
// are scene_sad_kernel's (v_sad_u8 on the three low bytes, u32 partials -> wave sum -> workgroup sum -> one 64-bit
// integer atomic add per item and workgroup at agent scope, into that member's SceneState::acc).  One ticket for the
// whole grid (release in every workgroup before it, acquire in the last one behind it; nobody waits): the workgroup that
// draws the last one takes the n decisions, lane j item j's -- from member j's own SceneState, written back to it, the
// record into member j's own ring.  What varies between ticks (step, ring slot, predecessor bits, threshold, mode) is
// read from member j's host-mapped SceneGroupDyn, three 64-bit loads per item, side by side across the lanes.
struct SceneGroupParams {
	const std::uint8_t *frames[kFlowBatchMax];
	long long strides[kFlowBatchMax];
	std::uint32_t *prev[kFlowBatchMax];
	SceneState *st[kFlowBatchMax];
	SceneRecord *ring[kFlowBatchMax];
	const SceneGroupDyn *dyn[kFlowBatchMax];
	unsigned *ticket;
	int W, items;
	long long pixels;
};

__global__ __launch_bounds__(kSadThreads) void scene_group_kernel(SceneGroupParams p) {
	__shared__ unsigned waveSums[kSadThreads / 64];
	__shared__ unsigned lastGroup;
	const unsigned item = blockIdx.y;
	const std::uint8_t *__restrict__ src = p.frames[item];
	const long long srcStride = p.strides[item];
	std::uint32_t *__restrict__ prev = p.prev[item];
	const unsigned base = blockIdx.x * static_cast<unsigned>(kSadPerGroup) + threadIdx.x;
	const unsigned width = static_cast<unsigned>(p.W), count = static_cast<unsigned>(p.pixels);
	unsigned partial = 0;
#pragma unroll
	for (int k = 0; k < kSadPerThread; ++k) {
		const unsigned i = base + static_cast<unsigned>(k * kSadThreads);
		if (i < count) {
			const unsigned row = i / width, x = i - row * width;
			const unsigned cur = *reinterpret_cast<const std::uint32_t *>(src + static_cast<long long>(row) * srcStride + x * 4u);
			const unsigned old = prev[i];
			prev[i] = cur;
			partial = __builtin_amdgcn_sad_u8(cur & 0x00ffffffu, old & 0x00ffffffu, partial);
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) partial += __shfl_down(partial, off, 64);
	if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = partial;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long groupSum = 0;
#pragma unroll
		for (int w = 0; w < kSadThreads / 64; ++w) groupSum += waveSums[w];
		__hip_atomic_fetch_add(&p.st[item]->acc, groupSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		// publish the add before the ticket (fence, then its wait, then the ticket: in that order)
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		const unsigned ticket = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		lastGroup = ticket == gridDim.x * gridDim.y - 1 ? 1u : 0u;
	}
	__syncthreads();
	if (lastGroup == 0 || threadIdx.x >= static_cast<unsigned>(p.items)) return;
	// ---- the last workgroup of the launch: lane j takes item j's decision ----
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const unsigned j = threadIdx.x;
	// (the grid's one ticket: every workgroup has drawn, so nothing adds to it any more)
	if (j == 0) __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	const SceneGroupDyn *dyn = p.dyn[j];
	const unsigned long long step = __hip_atomic_load(&dyn->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned long long slotPrev = __hip_atomic_load(&dyn->slotHasPrev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned long long thrMode = __hip_atomic_load(&dyn->thresholdMode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	const unsigned slot = static_cast<unsigned>(slotPrev) % static_cast<unsigned>(kSceneRing);
	const unsigned hasPrev = static_cast<unsigned>(slotPrev >> 32);
	const unsigned thresholdMilli = static_cast<unsigned>(thrMode);
	const unsigned resetMode = static_cast<unsigned>(thrMode >> 32) == 2u ? 1u : 0u;
	SceneState *st = p.st[j];
	// read the sum and re-arm the accumulator in one atomic
	unsigned long long S = __hip_atomic_exchange(&st->acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (!(hasPrev & 1)) S = 0;  // no predecessor: what the kept frame held is not a frame of this stream
	unsigned long long D = 0;
	if ((hasPrev & 3) == 3) {
		const unsigned long long before = st->prevSad;
		const unsigned long long delta = S > before ? S - before : before - S;
		D = S < delta ? S : delta;
	}
	const unsigned long long N = 3ull * static_cast<unsigned long long>(p.pixels);
	const unsigned cut = 1000ull * D >= static_cast<unsigned long long>(thresholdMilli) * N ? 1u : 0u;
	const unsigned long long frames = st->frames + 1, cuts = st->cuts + cut;
	st->prevSad = S;
	st->frames = frames;
	st->cuts = cuts;
	st->resetNow = (cut && resetMode) ? 1u : 0u;
	SceneRecord *r = p.ring[j] + slot;
	__hip_atomic_store(&r->step, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->sad, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->score, D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&r->cut, cut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	SceneRecord *totals = p.ring[j] + kSceneRing;
	__hip_atomic_store(&totals->step, frames, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&totals->sad, cuts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int kClearThreads = 256;
constexpr int kClearVecsPerThread = 4;
constexpr long long kClearPerGroup = static_cast<long long>(kClearThreads) * kClearVecsPerThread * 16;

// bytes [0, n) of `p` -> 0 for the part of it this workgroup owns: chunk `chunk` of kClearPerGroup bytes, counted
// from the first 16-byte boundary at or behind p; chunk 0 also takes the bytes in front of that boundary
__device__ __forceinline__ void clearChunk(std::uint8_t *p, long long n, long long chunk) {
	long long head = static_cast<long long>((16 - (reinterpret_cast<std::uintptr_t>(p) & 15)) & 15);
	if (head > n) head = n;
	if (chunk == 0 && static_cast<long long>(threadIdx.x) < head) p[threadIdx.x] = 0;
	const long long vecs = (n - head) / 16;
	uint4 *v = reinterpret_cast<uint4 *>(p + head);
	const long long first = chunk * (kClearPerGroup / 16);
#pragma unroll
	for (int k = 0; k < kClearVecsPerThread; ++k) {
		const long long i = first + static_cast<long long>(k) * kClearThreads + threadIdx.x;
		if (i < vecs) v[i] = make_uint4(0u, 0u, 0u, 0u);
	}
	// the tail behind the last whole vector, by the workgroup that owns the end of the buffer
	const long long tailAt = head + vecs * 16, tail = n - tailAt;
	const long long lastChunk = vecs == 0 ? 0 : (vecs - 1) / (kClearPerGroup / 16);
	if (chunk == lastChunk && static_cast<long long>(threadIdx.x) < tail) p[tailAt + threadIdx.x] = 0;
}

__global__ __launch_bounds__(kClearThreads) void scene_clear_kernel(const unsigned *__restrict__ flag, std::uint8_t *a,
    long long aBytes, int aChunks, std::uint8_t *b, long long bBytes) {
	if (*flag == 0) return;
	const int g = static_cast<int>(blockIdx.x);
	if (g < aChunks) {
		clearChunk(a, aBytes, g);
	} else {
		clearChunk(b, bBytes, g - aChunks);
	}
}

// scene_clear_items_kernel: scene_clear_kernel for all members of a group pass in one launch.  blockIdx.y is the item,
// blockIdx.x the chunk of its two buffers; every workgroup loads its item's flag once and returns if it is 0 (so do the
// workgroups past the item's last chunk: the grid is as wide as the largest item).
struct SceneClearItemsParams {
	const unsigned *flag[kFlowBatchMax];
	std::uint8_t *a[kFlowBatchMax], *b[kFlowBatchMax];
	long long aBytes[kFlowBatchMax], bBytes[kFlowBatchMax];
	int aChunks[kFlowBatchMax], bChunks[kFlowBatchMax];
};

__global__ __launch_bounds__(kClearThreads) void scene_clear_items_kernel(SceneClearItemsParams p) {
	const unsigned item = blockIdx.y;
	if (*p.flag[item] == 0) return;
	const int g = static_cast<int>(blockIdx.x), aChunks = p.aChunks[item];
	if (g < aChunks) {
		clearChunk(p.a[item], p.aBytes[item], g);
	} else if (g - aChunks < p.bChunks[item]) {
		clearChunk(p.b[item], p.bBytes[item], g - aChunks);
	}
}

// scene_clear_tiles_kernel: the conditional clear of ALL tiles of a tiled frame (docs/tiled.md "Scene cuts") under ONE
// flag -- the tiled stream's SceneState::resetNow.  blockIdx.y is the tile, blockIdx.x the chunk of its two buffers; every
// workgroup loads the flag once and returns if it is 0 -- in front of any read of the table, which holds up to kTileMax
// entries (too many for kernel arguments) and which the host rewrites in front of every launch.  The arithmetic is
// scene_clear_items_kernel's.
__global__ __launch_bounds__(kClearThreads) void scene_clear_tiles_kernel(const unsigned *__restrict__ flag,
    const SceneClearTile *__restrict__ table) {
	if (*flag == 0) return;
	const SceneClearTile &t = table[blockIdx.y];
	const int g = static_cast<int>(blockIdx.x), aChunks = t.aChunks;
	if (g < aChunks) {
		clearChunk(t.a, t.aBytes, g);
	} else if (g - aChunks < t.bChunks) {
		clearChunk(t.b, t.bBytes, g - aChunks);
	}
}

int clearChunks(std::size_t bytes) {
	// (15 bytes of head at most; one chunk more than the vectors need never hurts: its stores are bounds-checked)
	return bytes == 0 ? 0 : static_cast<int>((bytes + static_cast<std::size_t>(kClearPerGroup) - 1) / static_cast<std::size_t>(kClearPerGroup));
}

}  // namespace

std::string sceneDetectProblem(int mode, std::uint32_t thresholdMilli) {
	if (mode < 0 || mode > 2) {
		return "mode must be JU_SCENE_OFF (0), JU_SCENE_REPORT (1) or JU_SCENE_RESET (2), got " + std::to_string(mode);
	}
	if (mode != 0 && (thresholdMilli < 1 || thresholdMilli > 255000)) {
		return "threshold_milli must be 1 .. 255000, got " + std::to_string(thresholdMilli);
	}
	return "";
}

void launchSceneSad(const SceneSadLaunch &q, hipStream_t stream) {
	if (q.src == nullptr || q.prev == nullptr || q.state == nullptr || q.ring == nullptr || q.width < 1 || q.height < 1 ||
	    q.width > kSceneAxisMax || q.height > kSceneAxisMax) {
		throw std::invalid_argument("scene_sad: null buffer or a size outside 1 .. " + std::to_string(kSceneAxisMax));
	}
	if (reinterpret_cast<std::uintptr_t>(q.src) % 4 != 0 || q.srcStride % 4 != 0) {
		throw std::invalid_argument("scene_sad: the frame and its stride must be 4-byte aligned");
	}
	const auto row = static_cast<std::ptrdiff_t>(q.width) * 4;
	if (q.srcStride > -row && q.srcStride < row) throw std::invalid_argument("scene_sad: |stride| smaller than a row");
	if (q.slot < 0 || q.slot >= kSceneRing) throw std::invalid_argument("scene_sad: ring slot outside 0 .. 63");
	const long long pixels = static_cast<long long>(q.width) * q.height;
	const unsigned groups = static_cast<unsigned>((pixels + kSadPerGroup - 1) / kSadPerGroup);
	hipLaunchKernelGGL(scene_sad_kernel, dim3(groups), dim3(kSadThreads), 0, stream, q.src, static_cast<long long>(q.srcStride),
	    q.width, pixels, q.prev, q.state, q.ring, q.slot, static_cast<unsigned long long>(q.step), q.hasPrev, q.thresholdMilli,
	    q.resetMode ? 1 : 0);
	hipCheckLaunch("scene_sad");
}

void launchScenePass(const ScenePassLaunch &q, hipStream_t stream) {
	if (q.items < 1 || q.items > kFlowBatchMax) throw std::invalid_argument("scene_pass: 1 .. " + std::to_string(kFlowBatchMax) + " frames");
	if (q.prev == nullptr || q.state == nullptr || q.pass == nullptr || q.dyn == nullptr || q.ring == nullptr || q.width < 1 ||
	    q.height < 1 || q.width > kSceneAxisMax || q.height > kSceneAxisMax) {
		throw std::invalid_argument("scene_pass: null buffer or a size outside 1 .. " + std::to_string(kSceneAxisMax));
	}
	const auto row = static_cast<std::ptrdiff_t>(q.width) * 4;
	ScenePassParams p{};
	for (int i = 0; i < q.items; ++i) {
		if (q.frames[i] == nullptr) throw std::invalid_argument("scene_pass: frame " + std::to_string(i) + " is null");
		if (reinterpret_cast<std::uintptr_t>(q.frames[i]) % 4 != 0 || q.strides[i] % 4 != 0) {
			throw std::invalid_argument("scene_pass: every frame and its stride must be 4-byte aligned");
		}
		if (q.strides[i] > -row && q.strides[i] < row) throw std::invalid_argument("scene_pass: |stride| smaller than a row");
		p.frames[i] = q.frames[i];
		p.strides[i] = static_cast<long long>(q.strides[i]);
	}
	p.W = q.width;
	p.resetMode = q.resetMode ? 1 : 0;
	p.pixels = static_cast<long long>(q.width) * q.height;
	p.prev = q.prev;
	p.st = q.state;
	p.ps = q.pass;
	p.dyn = q.dyn;
	p.ring = q.ring;
	const unsigned groups = static_cast<unsigned>((p.pixels + kSadPerGroup - 1) / kSadPerGroup);
	static_assert(kFlowBatchMax == 8, "one instantiation per pass length");
	switch (q.items) {
	case 1: launchScenePassN<1>(p, groups, stream); break;
	case 2: launchScenePassN<2>(p, groups, stream); break;
	case 3: launchScenePassN<3>(p, groups, stream); break;
	case 4: launchScenePassN<4>(p, groups, stream); break;
	case 5: launchScenePassN<5>(p, groups, stream); break;
	case 6: launchScenePassN<6>(p, groups, stream); break;
	case 7: launchScenePassN<7>(p, groups, stream); break;
	default: launchScenePassN<8>(p, groups, stream); break;
	}
	hipCheckLaunch("scene_pass");
}

void launchSceneGroup(const SceneGroupLaunch &q, hipStream_t stream) {
	if (q.items < 1 || q.items > kFlowBatchMax) throw std::invalid_argument("scene_group: 1 .. " + std::to_string(kFlowBatchMax) + " items");
	if (q.width < 1 || q.height < 1 || q.width > kSceneAxisMax || q.height > kSceneAxisMax) {
		throw std::invalid_argument("scene_group: a size outside 1 .. " + std::to_string(kSceneAxisMax));
	}
	const auto row = static_cast<std::ptrdiff_t>(q.width) * 4;
	SceneGroupParams p{};
	int present = 0;
	for (int i = 0; i < q.items; ++i) {
		const SceneGroupItem &it = q.item[i];
		if (it.frame == nullptr) continue;  // (a member without a detector)
		const std::string who = "scene_group: item " + std::to_string(i);
		if (it.prev == nullptr || it.state == nullptr || it.ring == nullptr || it.dyn == nullptr) throw std::invalid_argument(who + ": null buffer");
		if (reinterpret_cast<std::uintptr_t>(it.frame) % 4 != 0 || it.stride % 4 != 0) {
			throw std::invalid_argument(who + ": the frame and its stride must be 4-byte aligned");
		}
		if (it.stride > -row && it.stride < row) throw std::invalid_argument(who + ": |stride| smaller than a row");
		for (int k = 0; k < present; ++k) {
			if (p.prev[k] == it.prev || p.st[k] == it.state) throw std::invalid_argument(who + ": shares its detector memory with another item");
		}
		p.frames[present] = it.frame;
		p.strides[present] = static_cast<long long>(it.stride);
		p.prev[present] = it.prev;
		p.st[present] = it.state;
		p.ring[present] = it.ring;
		p.dyn[present] = it.dyn;
		++present;
	}
	if (present == 0) return;  // (no member detects: no launch)
	p.ticket = &p.st[0]->ticket;  // (the grid's one ticket: the first item's)
	p.W = q.width;
	p.items = present;
	p.pixels = static_cast<long long>(q.width) * q.height;
	const unsigned groups = static_cast<unsigned>((p.pixels + kSadPerGroup - 1) / kSadPerGroup);
	hipLaunchKernelGGL(scene_group_kernel, dim3(groups, static_cast<unsigned>(present)), dim3(kSadThreads), 0, stream, p);
	hipCheckLaunch("scene_group");
}

void launchSceneClearItems(const SceneClearItem *items, int n, hipStream_t stream) {
	if (n < 0 || n > kFlowBatchMax || (n > 0 && items == nullptr)) {
		throw std::invalid_argument("scene_clear_items: 0 .. " + std::to_string(kFlowBatchMax) + " items");
	}
	SceneClearItemsParams p{};
	int present = 0, widest = 0;
	for (int i = 0; i < n; ++i) {
		const SceneClearItem &it = items[i];
		if (it.flag == nullptr) continue;  // (a member that does not restart: absent)
		if ((it.a == nullptr && it.aBytes != 0) || (it.b == nullptr && it.bBytes != 0)) {
			throw std::invalid_argument("scene_clear_items: item " + std::to_string(i) + ": null buffer");
		}
		const int aChunks = clearChunks(it.aBytes), bChunks = clearChunks(it.bBytes);
		if (aChunks + bChunks == 0) continue;
		p.flag[present] = it.flag;
		p.a[present] = static_cast<std::uint8_t *>(it.a);
		p.b[present] = static_cast<std::uint8_t *>(it.b);
		p.aBytes[present] = static_cast<long long>(it.aBytes);
		p.bBytes[present] = static_cast<long long>(it.bBytes);
		p.aChunks[present] = aChunks;
		p.bChunks[present] = bChunks;
		widest = std::max(widest, aChunks + bChunks);
		++present;
	}
	if (present == 0) return;
	hipLaunchKernelGGL(scene_clear_items_kernel, dim3(static_cast<unsigned>(widest), static_cast<unsigned>(present)), dim3(kClearThreads), 0,
	    stream, p);
	hipCheckLaunch("scene_clear_items");
}

void launchSceneClearTiles(const unsigned *flag, const SceneClearItem *items, int n, volatile SceneClearTile *tableHost,
    const SceneClearTile *tableDev, hipStream_t stream) {
	if (n < 1 || n > kTileMax || items == nullptr) throw std::invalid_argument("scene_clear_tiles: 1 .. " + std::to_string(kTileMax) + " tiles");
	if (flag == nullptr || tableHost == nullptr || tableDev == nullptr) throw std::invalid_argument("scene_clear_tiles: null flag or table");
	int widest = 0;
	for (int i = 0; i < n; ++i) {
		const SceneClearItem &it = items[i];
		if ((it.a == nullptr && it.aBytes != 0) || (it.b == nullptr && it.bBytes != 0)) {
			throw std::invalid_argument("scene_clear_tiles: tile " + std::to_string(i) + ": null buffer");
		}
		const int aChunks = clearChunks(it.aBytes), bChunks = clearChunks(it.bBytes);
		volatile SceneClearTile &t = tableHost[i];
		t.a = static_cast<std::uint8_t *>(it.a);
		t.b = static_cast<std::uint8_t *>(it.b);
		t.aBytes = static_cast<long long>(it.aBytes);
		t.bBytes = static_cast<long long>(it.bBytes);
		t.aChunks = aChunks;
		t.bChunks = bChunks;
		widest = std::max(widest, aChunks + bChunks);
	}
	if (widest == 0) return;
	std::atomic_thread_fence(std::memory_order_seq_cst);  // (the table is in place before the launch is enqueued)
	hipLaunchKernelGGL(scene_clear_tiles_kernel, dim3(static_cast<unsigned>(widest), static_cast<unsigned>(n)), dim3(kClearThreads), 0,
	    stream, flag, tableDev);
	hipCheckLaunch("scene_clear_tiles");
}

void launchSceneClear(const unsigned *flag, void *a,std::size_t aBytes, void *b, std::size_t bBytes, hipStream_t stream) {
	if (flag == nullptr || (a == nullptr && aBytes != 0) || (b == nullptr && bBytes != 0)) {
		throw std::invalid_argument("scene_clear: null buffer");
	}
	const int aChunks = clearChunks(aBytes), bChunks = clearChunks(bBytes);
	if (aChunks + bChunks == 0) return;
	hipLaunchKernelGGL(scene_clear_kernel, dim3(static_cast<unsigned>(aChunks + bChunks)), dim3(kClearThreads), 0, stream, flag,
	    static_cast<std::uint8_t *>(a), static_cast<long long>(aBytes), aChunks, static_cast<std::uint8_t *>(b),
	    static_cast<long long>(bBytes));
	hipCheckLaunch("scene_clear");
}

}  // namespace ju
