// Look-ahead passes (processBatch, processFrames) and group passes (processGroup): several frames under the flow net's
// launches of one.  engine.cpp holds the per-frame program they reuse, engine_frames.cpp the staged path of the frames
// that run one by one.
#include <algorithm>
#include <atomic>
#include <set>
#include <stdexcept>
#include <string>

#include "alpha_route.h"
#include "engine.h"
#include "log.h"

namespace ju {

// ---------------------------------------------------------------------------------------------------------------
// Frame look-ahead.  The flow net reads LR frames only -- never the HR state (models.py:790, 823: its input is the
// packed history of the last num_flow_inputs frames) -- so the flow fields of n consecutive frames can be computed
// before the first of them is upscaled: ONE pass of the flow net's eight launches over n frames instead of n passes.
// At 480x270 each of those launches is ONE round of 136-240 workgroups on 256 CUs -- a 7-24 us latency chain (weights,
// staging, conv A, conv B, stores) with most SIMDs idle most of the time (0.3-0.6 waves per SIMD,
// profiles/r05_pmc_stall_flow.txt): over 8 frames the same launches take 62 instead of 105 us per frame
// (profiles/r05_flow_layers_pass.txt; priced beforehand by tools/probes/flow_batch_estimate.py), and a pass pays one
// synchronisation instead of eight: 2163 -> 2461 frames/s (profiles/r05_lookahead_bench_box_a.txt).  The recurrent part -- warp, tower,
// tail -- stays strictly frame by frame, and every frame's bytes are those of process(): the same kernels add the
// same terms in the same order whatever the launch's size.
//
// State.  Frame i of a pass reads the state frame i - 1 wrote; the pass owns the n - 1 buffers in between, reads
// m_State[set] and leaves the last frame's state in m_State[set ^ 1] and the last history in m_Packed[set ^ 1], as
// ONE process() call would: the pass flips the binding set once, and -- since nothing it wrote is read before the
// pass -- a pass that failed (resident tower: bounded wait expired) can be run again frame by frame.
//
// The scene detector inside a pass (setSceneLookahead; docs/scene_detect.md "Passes").  The detector reads the LR frames
// only, and all of them are there before the pass's first launch: scene_pass_kernel takes the n decisions in ONE launch in
// front of the flow net's and leaves resetAt[] / cutAt[] on the device.  In reset mode on a recurrent model the pass then
// restarts the recurrence itself: the first flow block takes its history by cutAt[] (the flow programs at kCutSet + set),
// and a scene_clear_kernel in front of frame i's steps zeroes its input state while resetAt[i] is set.  One exception
// to "writes nothing it reads": that clear may zero m_State[set] for frame 0 -- what a re-run of the frames, whose
// decisions stand, wants to find there too.
// ---------------------------------------------------------------------------------------------------------------
bool Engine::batchPlanned(int items, bool group) {
	if (!m_Config.recurrent()) {
		// a flow-free model: a pass is its frames' generator programs under one synchronisation -- no flow launches,
		// no pass tensors, and every frame's tail writes the one scratch state
		if (m_BatchUnsupported || m_Calibrate) return false;
		for (int set = 0; set < 2; ++set) m_BatchFlow[{items, set}];
		m_BatchFlow[{items, kGroupSet}];
		m_BatchCap = std::max({m_BatchCap, items, m_BatchMax});
		return true;
	}
	if (m_BatchUnsupported || m_Calibrate || m_Config.flowArch != 0 || !flowPacksInBlock() || m_Config.normalizeBrightness) {
		return false;
	}
	// (a pass that restarts the recurrence at scene cuts has flow launches of its own: the first block's cut-aware history)
	const bool cut = !group && scenePass() == 2;
	if (items <= m_BatchCap && m_BatchFlow.count({items, group ? kGroupSet : 0}) && (!cut || m_BatchFlow.count({items, kCutSet}))) {
		return true;
	}
	try {
		if (items > m_BatchCap) {
			// (the tensors of every pass so far are too small: start over)
			m_Stream.synchronize();
			m_BatchGraphs.clear();
			m_BatchFlow.clear();
			m_BatchTensors.clear();
			// (the whole cap at once: growing later reallocates the tensors every captured pass is bound to -- also the
			// registered ones -- and round 6's bench lost a registered short pass that way.  ~210 MB at 480x270 for 8 frames.)
			const int cap = std::max(items, m_BatchMax);
			for (const auto &kv : m_Tensors) {
				const bool flowTensor = kv.first == "flow" || kv.first.rfind("flow/", 0) == 0;
				if (!flowTensor) continue;
				Tensor t;
				t.count = kv.second.count * cap;
				t.isF32 = kv.second.isF32;
				t.isState = kv.second.isState;
				t.buf = DeviceBuffer(t.count * (t.isF32 ? 4 : 2));
				m_BatchTensors.emplace(kv.first, std::move(t));
			}
			m_BatchCap = cap;
		}
		if (group) {  // (a group pass chains no states: each member reads and writes its own)
			std::vector<Step> prog;
			addFlowAutoencoder(&prog, 0, items, true);
			m_BatchFlow[{items, kGroupSet}] = std::move(prog);
			return true;
		}
		for (int i = 0; i + 1 < m_BatchCap; ++i) {
			if (!m_BatchState[i].get()) m_BatchState[i] = DeviceBuffer(m_State[0].bytes());
		}
		for (int set = 0; set < 2; ++set) {
			if (!m_BatchFlow.count({items, set})) {
				std::vector<Step> prog;
				addFlowAutoencoder(&prog, set, items);
				m_BatchFlow[{items, set}] = std::move(prog);
			}
			if (cut && !m_BatchFlow.count({items, kCutSet + set})) {
				std::vector<Step> prog;
				addFlowAutoencoder(&prog, set, items, false, true);
				m_BatchFlow[{items, kCutSet + set}] = std::move(prog);
			}
		}
		return true;
	} catch (const std::exception &e) {
		// (std::logic_error: a launch of this model's flow plan has no item dimension; anything else -- the pass's
		// tensors did not fit the device -- equally means "frame by frame from now on", not a failed call)
		logMessage(dynamic_cast<const std::logic_error *>(&e) ? LogLevel::Info : LogLevel::Warning, "Engine",
		    std::string("frame look-ahead is off for this runtime: ") + e.what());
		m_BatchUnsupported = true;
		m_BatchFlow.clear();
		m_BatchTensors.clear();
		m_BatchCap = 0;
		return false;
	}
}

void Engine::setLookahead(int frames) {
	DeviceGuard g(m_Device);
	const int cap = std::min(std::max(frames, 1), kFlowBatchMax);
	if (cap < m_BatchMax) {
		// graphs of longer passes can no longer be asked for: drop them (their launches may still be in flight)
		m_Stream.synchronize();
		m_BatchGraphs.eraseIf([cap](const std::vector<PassKey> &key) { return static_cast<int>(key.size()) > cap; });
	}
	m_BatchMax = cap;
}

// The launches of one look-ahead pass over the n frames of m_Pass, in stream order (recorded when m_Stream is
// capturing): the flow net over all frames, then frame by frame the rest of binding set `set`'s per-frame program,
// bound to the frame's buffers, its flow field and its link of the state chain.
void Engine::runBatch(int set, int n, const std::function<void(const Step &, bool)> *around) {
	auto run = [&](const Step &st) {
		if (around) (*around)(st, false);
		st.run(m_Stream);
		if (around) (*around)(st, true);
	};
	const int scene = scenePass();
	const std::vector<Step> &flow = m_BatchFlow.at({n, scene == 2 ? kCutSet + set : set});
	const bool recurrent = m_Config.recurrent();  // (flow-free: no flow fields, no state chain)
	const long flowItem = recurrent ? static_cast<long>(m_Tensors.at("flow").count) * 2 : 0;
	const unsigned char *flowBase = recurrent ? m_BatchTensors.at("flow").buf.as<unsigned char>() : nullptr;
	const StateBind keepBind = m_StateBind[set];
	AtExit restore{[this, set, keepBind, keepIO = m_IO, keepFlow = m_FlowCur] {
		m_IO = keepIO;
		m_StateBind[set] = keepBind;
		m_FlowCur = keepFlow;
	}};
	// the pass's YUV inputs into their frames' BGRX buffers, all in one launch (a flow-free pass has no launch before it):
	// at the frames' own size -- the model's input, or under a source size the source-size slots (PassFrame::ends)
	const int stage = m_PassStage;
	std::size_t inW, inH, outW, outH;
	passSizes(stage, &inW, &inH, &outW, &outH);
	YuvDecodeItems items{};
	int decodes = 0;
	for (int i = 0; i < n; ++i) {
		const PassFrame &f = m_Pass[i];
		if (!f.in.yuv) continue;
		items.item[decodes++] = yuvDecodeItem(fmt(f.in.format), f.in.colorspace, f.in.planes, const_cast<std::uint8_t *>(f.ends.in),
		    f.ends.inStride);
	}
	if (decodes) launchYuv420ToBgrxItems(items, decodes, static_cast<int>(inW), static_cast<int>(inH), m_Stream);
	// a source size: ONE launch scales all n sources -- the caller's device images where they are, the upload slots, the
	// slots the decode launch above fills -- into the pass's model-size inputs, in front of the detector and the flow net,
	// which therefore read exactly what submitFrame gives them
	if (stage & 1) {
		ScaleItems scale{};
		for (int i = 0; i < n; ++i) {
			const PassFrame &f = m_Pass[i];
			scale.item[i] = ScaleItem{f.ends.in, f.ends.inStride, const_cast<std::uint8_t *>(f.io.in), f.io.inStride};
		}
		m_SrcScale.scaleBgrxItems(scale, n, m_Stream);
	}
	// The scene detector inside a pass: every frame of the pass is in place here (the caller's device frames, the upload
	// slots, the BGRX buffers the decode launch above fills), so ONE launch takes all n decisions in front of the flow
	// net's -- the records, and on the device resetAt[] for the clear in front of each frame and cutAt[] for the first
	// flow block's history.  The frames are read where they are, each with its own address and stride.
	ScenePassState *passState = scene ? m_ScenePassDev.as<ScenePassState>() : nullptr;
	if (scene) {
		const FrameSize fs = frameSize();
		ScenePassLaunch q;
		q.items = n;
		for (int i = 0; i < n; ++i) {
			q.frames[i] = m_Pass[i].io.in;
			q.strides[i] = m_Pass[i].io.inStride;
		}
		q.width = static_cast<int>(fs.inputWidth);
		q.height = static_cast<int>(fs.inputHeight);
		q.prev = m_Scene.prev();
		q.state = m_Scene.state();
		q.pass = passState;
		q.dyn = reinterpret_cast<const ScenePassDyn *>(m_ScenePassDyn.device());
		q.ring = m_Scene.ring();
		q.resetMode = scene == 2;
		launchScenePass(q, m_Stream);
	}
	for (const Step &st : flow) run(st);
	for (int i = 0; i < n; ++i) {
		m_IO = m_Pass[i].io;
		if (recurrent) {
			m_FlowCur = flowBase + i * flowItem;
			m_StateBind[set].in = i == 0 ? keepBind.in : m_BatchState[i - 1].get();
			m_StateBind[set].out = i + 1 == n ? keepBind.out : m_BatchState[i].get();
			// a cut at frame i: its input state is zero, as after reset() -- behind frame i - 1's tail and its encode (which
			// read that buffer: stream order), in front of frame i's warp; with the flag 0 every workgroup returns at once
			if (scene == 2) {
				launchSceneClear(&passState->resetAt[i], const_cast<void *>(m_StateBind[set].in), m_State[set].bytes(), nullptr, 0, m_Stream);
			}
		}
		for (const Step &st : m_Program[set]) {
			if (st.tag != "flow" && st.tag != "pack") run(st);
		}
		// (a 10-bit output from the state: THIS frame's link of the chain -- m_BatchState[i], the last frame's
		// m_State[set ^ 1]; a flow-free pass has one scratch state that the next frame's tail overwrites, so the encode
		// stays on this stream in front of the next frame's kernels)
		passTail(*this, m_Pass[i], stage, m_StateBind[set].out, m_StageSlots[i].out16);
	}
}

// Behind a frame's own steps, what submitFrame strings behind the program -- the single-frame launches with the owner's
// own mask and scaler, in stream order on this runtime's stream.
void Engine::passTail(Engine &owner, const PassFrame &f, int stage, void *stateOut, const DeviceBuffer &out16) {
	if (stage & 2) {
		// the mask, in place over the model-size frame the tail wrote (a slot the pass alone writes, or the caller's output),
		// through submitFrame's `source`: the frame's own source rows, or the model-size input when no source size is set
		owner.blendMask(f.io.out, f.io.outStride, f.ends.in, f.ends.inStride, f.size.inW, f.size.inH, m_Stream);
	}
	const std::uint16_t *frame16 = nullptr;
	if (stage & 4) {  // stageOutScaled's rules: the 8-bit frame, or for a deep format from the state the frame's steps wrote
		if (f.out.yuv && owner.deepFromState(f.out.format)) {
			auto *scaled16 = out16.as<std::uint16_t>();
			owner.m_OutScale.scaleState(stateOut, scaled16, m_Stream);
			frame16 = scaled16;
		} else {
			owner.m_OutScale.scaleBgrx(f.io.out, f.io.outStride, f.ends.out, f.ends.outStride, m_Stream);
		}
	}
	// a non-BGRX output: the frame's BGRX output at its own output size (a plain slot, or the owner's scaled slot) into the
	// caller's device planes / the staging slot.  A deep format is encoded from the f16 state THE OWNER's step just wrote
	// -- in a group pass never the lead's -- or from the blended or scaled 8-bit frame while the owner has a mask or
	// "hbd_from_state" 0 (deepFromState)
	if (f.out.yuv) {
		owner.encodeYuv(f.out.format, f.out.colorspace, f.out.planes, f.size.outW, f.size.outH, f.ends.out, f.ends.outStride, stateOut,
		    frame16, m_Stream);
	}
	// alpha (setAlphaLookahead, setAlphaGroup): the owner's one launch behind the frame's colour, the launch alphaInto makes
	// -- the owner's mode, filter and tables, in a group pass never the lead's -- over the rows bindFrame found; in front of
	// the signal, so a host frame is copied out with its alpha in place.  (A runtime whose mode is not 0 is in a pass only
	// under one of the two settings: passEligible.)
	owner.launchAlpha(f.alphaIn, f.alphaOut, m_Stream);
	// (a host frame: its bytes are complete in the slot `down` names -- tell the thread that copies them out)
	if (f.out.host) launchSignalHost(m_PassSignal.device(), m_Stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Alpha inside a pass (setAlphaLookahead, setAlphaGroup; docs/alpha.md "Passes").  Alpha lies outside the recurrence and
// touches no colour sample, so a pass takes it as it takes the mask blend and the encode: one launch behind the frame's
// colour, in stream order (passTail).  The input's alpha is read behind the output's colour -- from the caller's device
// rows, the upload slot or the staged planes, none of which the pass writes: the pass splitter keeps every output of a
// pass off every input of it, and checkAlphaOverlap refuses a device output over its own device input up front.  A
// captured pass bakes in the mode, the filter and the tables' addresses: PassKey::alpha keeps such a graph apart from the
// mode-0 graph over the same buffers, and every setter that changes one of the three drops these graphs (dropAlphaPasses).
// A pass that runs again goes frame by frame through submitFrame, which writes and counts alpha itself; the pass counts
// its frames only once it has completed.
// ---------------------------------------------------------------------------------------------------------------
void Engine::setAlphaLookahead(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_alpha_lookahead: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (m_AlphaLookahead != (on != 0)) dropAlphaPasses();
	m_AlphaLookahead = on != 0;
}

void Engine::setAlphaGroup(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_alpha_group: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();  // (group passes are eager: nothing is kept that the setting could make stale)
	m_AlphaGroup = on != 0;
}

void Engine::dropAlphaPasses() {
	m_BatchGraphs.eraseIf([](const std::vector<PassKey> &key) { return !key.empty() && key.front().alpha != 0; });
}

void Engine::blendMask(std::uint8_t *gen, std::ptrdiff_t genStride, const std::uint8_t *src, std::ptrdiff_t srcStride, std::size_t srcW,
    std::size_t srcH, hipStream_t stream) {
	const FrameSize fs = frameSize();
	launchMaskBlend(gen, genStride, static_cast<int>(fs.outputWidth), static_cast<int>(fs.outputHeight), src, srcStride,
	    static_cast<int>(srcW), static_cast<int>(srcH), m_Mask.first(), m_Mask.stride(), static_cast<int>(m_Mask.width()),
	    static_cast<int>(m_Mask.height()), stream);
}

// A frame may go into a pass when each of its two images is either a device-resident one the kernels can read / write in
// place (directEligible's conditions) or a host image of the right size (staged through the pass's own device buffers).
// A YUV side (checked by checkFrame before: processFrames) always can: the conversion kernels take any alignment.
bool Engine::passEligible(const AnyFrame &in, const AnyFrame &out, bool group) const {
	// (scaled / masked frames run one by one through submitFrame unless the passes carry the stages: setStageLookahead; a
	// group pass: setStageGroup)
	// (alpha: the staged single-frame route, whatever the stage and scene settings say -- unless the passes carry its
	// launch: setAlphaLookahead; a group pass: setAlphaGroup.  The stage and scene conditions then decide as in mode 0)
	if (m_AlphaMode != 0 && !(group ? m_AlphaGroup : m_AlphaLookahead)) return false;
	const int stage = stageBits(group);
	if (sourceStage() && !stage) return false;
	// (the scene detector: a pass computes the flow of all its frames from a history a cut inside it would invalidate --
	// unless the pass carries the detector and applies the cuts itself: setSceneLookahead; a group pass: setSceneGroup)
	if (m_Scene.mode() != 0 && !(group ? m_SceneGroup : m_SceneLookahead)) return false;
	std::size_t inW, inH, outW, outH;
	passSizes(stage, &inW, &inH, &outW, &outH);
	// scaled: the side's device image is read / written by a scale kernel, which takes any alignment and signed stride
	auto side = [&](const AnyFrame &a, std::size_t w, std::size_t h, unsigned align, bool scaled) {
		if (a.yuv) {
			const YuvFrame &y = a.planes;
			return (y.location == Location::Host || y.location == Location::Device) && y.width == w && y.height == h;
		}
		const Frame &f = a.bgrx;
		const auto row = static_cast<std::ptrdiff_t>(w * 4);
		if (f.ptr == nullptr || f.width != w || f.height != h || !(f.stride >= row || -f.stride >= row)) return false;
		if (f.location == Location::Host) return true;
		if (scaled) return f.location == Location::Device;
		return f.location == Location::Device && m_PreferDirect && reinterpret_cast<std::uintptr_t>(f.ptr) % align == 0 &&
		       f.stride % static_cast<std::ptrdiff_t>(align) == 0;
	};
	return side(in, inW, inH, 4, (stage & 1) != 0) && side(out, outW, outH, 8, (stage & 4) != 0);
}

void Engine::passSizes(int stage, std::size_t *inW, std::size_t *inH, std::size_t *outW, std::size_t *outH) const {
	const FrameSize fs = frameSize();
	*inW = (stage & 1) ? m_SrcScale.srcW() : fs.inputWidth;
	*inH = (stage & 1) ? m_SrcScale.srcH() : fs.inputHeight;
	*outW = (stage & 4) ? m_OutScale.dstW() : fs.outputWidth;
	*outH = (stage & 4) ? m_OutScale.dstH() : fs.outputHeight;
}

// ---------------------------------------------------------------------------------------------------------------
// Scaled and masked frames inside a pass (setStageLookahead; docs/source_stage.md and docs/output_stage.md, "Passes").
// The stages sit outside the recurrence -- the scaler in front of the model's input, blend and output scaler behind the
// frame the tail wrote -- so a pass takes them as it takes the colour conversions: the n sources are scaled by ONE launch
// (scale_bgrx_items_kernel) behind the one decode launch and in front of the detector and the flow net; blend, output
// scale and encode follow each frame's tail in stream order, reading that frame's link of the state chain.  What the
// network reads and writes in between are the pass's model-size slots (m_StageSlots[i].in / .modelOut); every launch is the
// one submitFrame makes, with the same arguments but the buffers, so the bytes are the frame-by-frame route's.
// ---------------------------------------------------------------------------------------------------------------
void Engine::setStageLookahead(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_stage_lookahead: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (m_StageLookahead != (on != 0)) dropStagePasses();
	m_StageLookahead = on != 0;
}

// The staged passes' graphs and the slots they are bound to: whenever a stage setter changes anything (the scalers'
// tables, the mask and the sizes are baked into those graphs).  The stream has drained: passes are synchronous.
void Engine::dropStagePasses() {
	m_Stream.synchronize();
	m_BatchGraphs.eraseIf([](const std::vector<PassKey> &key) { return !key.empty() && key.front().stage != 0; });
	for (StageSlots &slots : m_StageSlots) slots = StageSlots();
	// (this runtime's slots as a member of group passes: of the old sizes too.  A group pass is synchronous, so the lead's
	// stream, which ran the launches that used them, has drained, and no lead keeps a pointer to them: runGroupPass)
	m_GroupSlots = StageSlots();
}

void Engine::setStageGroup(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_stage_group: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (m_StageGroup != (on != 0)) m_GroupSlots = StageSlots();
	m_StageGroup = on != 0;
}

// Binds one frame of a pass: f->io = what the frame's kernels read and write -- the caller's device memory, or for a
// host image the pass's device buffer, addressed with the SIGN of the caller's stride (a bottom-up host frame is
// uploaded / downloaded in memory order and read / written bottom-up by the kernels: no flip pass).
//
// YUV frames (processFrames, processGroupFrames).  A YUV input is decoded into plain->in, a YUV output encoded from
// plain->out (top-down BGRX rows both), whatever the planes' location: f->in / f->out hold the planes those conversion
// launches read / write.  Device planes: the caller's, in place.  Host planes: plain->yuvIn / plain->yuvOut, plane
// after plane with rows padded to stagePitch and in the caller's MEMORY order, so a bottom-up plane is addressed from
// its last row with a negative pitch -- the layout of decodePlanes / stageOutYuv.
//
// A staged frame (stage != 0): a side under one of the owner's scalers is bound at the size set there, to the owner's
// slots (`staged`) in place of the plain ones, and lands in f->ends: the source-size rows the decode / upload fills and
// the scale launch reads, the output-size rows the output scaler writes.  f->io is then the model-size slot between that
// scaler and the network -- the input the scale launch fills, the frame the tail writes and the blend rewrites.  Without
// a scaler on a side the two are the same rows.
void Engine::bindFrame(PassFrame *f, const Engine &owner, int stage, const AnyFrame &in, const AnyFrame &out, StageSlots *staged,
    PassSlots *plain, PassKey *key) {
	const FrameSize fs = frameSize();
	PassExtent &sz = f->size;
	owner.passSizes(stage, &sz.inW, &sz.inH, &sz.outW, &sz.outH);
	const bool scaledIn = (stage & 1) != 0, scaledOut = (stage & 4) != 0;
	const StageSlotNeeds need = stageSlotNeeds(stage, in.yuv || locationOf(in) == Location::Host,
	    out.yuv || locationOf(out) == Location::Host, out.yuv && owner.deepFromState(out.planes.format));
	const StageSlotBytes bytes = stageSlotBytes(sz.inW, sz.inH, fs.inputWidth, fs.inputHeight, fs.outputWidth, fs.outputHeight, sz.outW,
	    sz.outH);
	auto slot = [](DeviceBuffer &b, std::size_t size) {
		if (!b.get()) b = DeviceBuffer(size);
	};
	if (need.input) slot(staged->in, bytes.input);
	if (need.modelOutput) slot(staged->modelOut, bytes.modelOutput);
	if (need.out16) slot(staged->out16, bytes.out16);
	// (src / out8 and the plane buffers: made by bindSide, which is handed the frame's sizes, when the side needs them)
	f->up = scaledIn ? PassCopy{&staged->src, &staged->srcYuv} : PassCopy{&plain->in, &plain->yuvIn};
	f->down = scaledOut ? PassCopy{&staged->out8, &staged->outYuv} : PassCopy{&plain->out, &plain->yuvOut};
	YuvKey unusedIn, unusedOut;
	const BoundRows r = bindSide(in, sz.inW, sz.inH, f->up.image, f->up.planes, &f->in, key ? &key->in : &unusedIn);
	const BoundRows w = bindSide(out, sz.outW, sz.outH, f->down.image, f->down.planes, &f->out, key ? &key->out : &unusedOut);
	f->io = f->ends = FrameIO{r.ptr, r.stride, w.ptr, w.stride};
	if (scaledIn) {
		f->io.in = staged->in.as<std::uint8_t>();
		f->io.inStride = static_cast<std::ptrdiff_t>(fs.inputWidth * 4);
	}
	if (scaledOut) {
		f->io.out = staged->modelOut.as<std::uint8_t>();
		f->io.outStride = static_cast<std::ptrdiff_t>(fs.outputWidth * 4);
	}
	// the alpha slots (alpha_route.h): a BGRX side's rows at the frame's own size -- the caller's device rows or the slot,
	// with the sign of a bottom-up host stride -- else plane 0 of the side's planes, the caller's or the staged ones
	auto alphaSide = [](const PassSide &s, const void *rows, std::ptrdiff_t stride) {
		AlphaSide a;
		a.planar = s.yuv;
		a.format = s.format;
		a.bgrx = AlphaSideRows{rows, stride};
		a.plane0 = AlphaSideRows{s.planes.y, s.planes.yStride};
		return alphaRowsOf(a);
	};
	f->alphaIn = alphaSide(f->in, f->ends.in, f->ends.inStride);
	f->alphaOut = alphaSide(f->out, f->ends.out, f->ends.outStride);
	if (f->out.host) {
		if (!m_PassSignal.host()) m_PassSignal = PinnedWords(64);
		if (!m_CopyStream) m_CopyStream = std::make_unique<Stream>();
	}
}

// The n frames of a look-ahead pass, each through this runtime's own slot i.  The key of the pass's graph is made of the
// bindings, so all-host passes of one length and orientation share one graph.  The staged slots of a kind are made for
// the whole cap when the first of them is needed, so no later pass moves what a captured one is bound to.
std::vector<Engine::PassKey> Engine::bindBatch(const AnyFrame *in, const AnyFrame *out, int n, int set, int stage) {
	m_PassStage = stage;
	const int cap = std::max(n, m_BatchMax);
	std::vector<PassKey> key(static_cast<std::size_t>(n));
	for (int i = 0; i < n; ++i) {
		PassFrame &f = m_Pass[i];
		PassKey &k = key[static_cast<std::size_t>(i)];
		bindFrame(&f, *this, stage, in[i], out[i], &m_StageSlots[i], &m_PassSlots[i], &k);
		for (auto kind : {&StageSlots::src, &StageSlots::srcYuv, &StageSlots::in, &StageSlots::modelOut, &StageSlots::out8,
		         &StageSlots::out16, &StageSlots::outYuv}) {
			const std::size_t size = (m_StageSlots[i].*kind).bytes();
			for (int j = 0; size != 0 && j < cap; ++j) {
				if (!(m_StageSlots[j].*kind).get()) m_StageSlots[j].*kind = DeviceBuffer(size);
			}
		}
		k.io = DirectKey{f.io.in, f.io.inStride, f.io.out, f.io.outStride, set};
		k.scene = scenePass();
		k.stage = stage;
		k.alpha = alphaPass(false);
		if (stage) k.ends = DirectKey{f.ends.in, f.ends.inStride, f.ends.out, f.ends.outStride, 0};
	}
	return key;
}

// The members of a group pass, bound on the lead (runGroupPass): member i's pair under member i's own stage bits and sizes
// in place of the lead's.  A side no scaler of member i touches is bound exactly as a plain group pass binds it -- the
// caller's device rows, or the lead's slot i (m_PassSlots, at the model's sizes).  A side under member i's source or output
// scaler goes through member i's OWN slots (m_GroupSlots), at member i's sizes.  No graph key: group passes are eager.
void Engine::bindGroup(Engine *const *m, const AnyFrame *in, const AnyFrame *out, int n, const int *stage) {
	m_PassStage = 0;
	for (int i = 0; i < n; ++i) bindFrame(&m_Pass[i], *m[i], stage[i], in[i], out[i], &m[i]->m_GroupSlots, &m_PassSlots[i], nullptr);
}

Engine::BoundRows Engine::bindSide(const AnyFrame &a, std::size_t width, std::size_t height, DeviceBuffer *image,
    DeviceBuffer *planes, PassSide *side, YuvKey *key) {
	*side = PassSide{};
	side->yuv = a.yuv;
	side->host = locationOf(a) == Location::Host;
	// (a device image: the caller's, in place)
	if (!a.yuv && !side->host) return {static_cast<std::uint8_t *>(a.bgrx.ptr), a.bgrx.stride};
	const auto row = static_cast<std::ptrdiff_t>(width * 4);
	if (!image->get()) *image = DeviceBuffer(height * static_cast<std::size_t>(row));
	auto *base = image->as<std::uint8_t>();
	if (!a.yuv) {  // a host image: the pass's buffer in the caller's memory order
		const SlotRows rows = slotRows(width, height, a.bgrx.stride >= 0);
		return {base + rows.first, rows.stride};
	}
	// a YUV side: the planes its conversion launch addresses, and what of them the graph bakes in
	const YuvFrame &y = a.planes;
	const YuvFormatInfo &info = formatInfo(y.format);
	side->format = y.format;
	side->colorspace = y.colorspace;
	key->format = static_cast<int>(y.format);
	// (ignored for RGB, and so is a siting the format's kernels do not distinguish: no second graph for another value)
	if (info.rgb()) {
		key->colorspace = 0;
	} else {
		const ColourSpace cs = splitColourSpace(y.colorspace);
		key->colorspace = cs.matrix | (effectiveSiting(info, cs.siting) << 8);
	}
	for (int k = 0; k < info.planes; ++k) {
		key->planes[k] = side->host ? nullptr : y.planes[k];
		key->strides[k] = side->host ? (y.strides[k] > 0 ? 1 : -1) : y.strides[k];
	}
	if (side->host) {
		if (!planes->get()) *planes = DeviceBuffer(yuvStageBytes(kFormatTable, y.width, y.height));
		side->planes = stagedPlanes(y, planes->as<std::uint8_t>());
	} else {
		side->planes = callerPlanes(y);
	}
	return {base, row};
}

// Every host input of the pass into its device buffer, rows in MEMORY order (the binding carries the orientation), on the
// engine's stream in front of the pass's launches.  Pageable memory: the runtime stages or page-locks per call, as in
// stageIn; 0.52 MB per BGRX frame, 0.19 MB per 4:2:0 frame -- plane by plane, as in decodePlanes.
void Engine::uploadPassInputs(const AnyFrame *in, int n) {
	for (int i = 0; i < n; ++i) {
		const PassFrame &f = m_Pass[i];
		if (!f.in.host) continue;
		// (a staged frame: at source size, into the source-size slot; a group pass: each member's own size)
		const std::size_t rowBytes = f.size.inW * 4, rows = f.size.inH;
		if (in[i].yuv) {
			copyPlanes(in[i].planes, f.up.planes->as<std::uint8_t>(), true, m_Stream);
			continue;
		}
		const RowSpan host = rowSpan(in[i].bgrx.ptr, in[i].bgrx.stride, rows);
		copyRows(f.up.image->get(), rowBytes, host.lowest, host.pitch, rowBytes, rows, hipMemcpyHostToDevice, m_Stream);
	}
}

// The thread blocked in processBatch: wait for frame i's completion count, copy frame i out on the copy stream while the
// GPU runs frame i + 1, in order.  The wait is bounded by the pass itself: once the engine's stream has drained, a count
// that has not arrived never will.  A YUV frame goes out plane by plane from its staging slot (3.1 MB at 1080p instead of
// BGRX's 8.3 MB), as in stageOutYuv.
void Engine::drainPassOutputs(const AnyFrame *out, int n) {
	volatile unsigned *word = m_PassSignal.host();
	unsigned due = 0;
	bool any = false;
	for (int i = 0; i < n; ++i) {
		const PassFrame &f = m_Pass[i];
		if (!f.out.host) continue;
		++due;
		auto arrived = [&] { return static_cast<int>(*word - m_PassSignalBase) >= static_cast<int>(due); };
		for (unsigned spins = 1; !arrived(); ++spins) {
			if ((spins & 255u) == 0) {
				const hipError_t st = hipStreamQuery(m_Stream);
				if (st == hipSuccess) {
					if (arrived()) break;
					throw std::runtime_error("look-ahead pass: the completion count of a host frame did not arrive");
				}
				if (st != hipErrorNotReady) JU_HIP(st);
			} else {
				__builtin_ia32_pause();
			}
		}
		any = true;
		// (a staged frame: rows and planes at the output size; a group pass: each member's own)
		const std::size_t rowBytes = f.size.outW * 4, rows = f.size.outH;
		if (out[i].yuv) {
			copyPlanes(out[i].planes, f.down.planes->as<std::uint8_t>(), false, *m_CopyStream);
			continue;
		}
		const RowSpan host = rowSpan(out[i].bgrx.ptr, out[i].bgrx.stride, rows);
		copyRows(host.lowest, host.pitch, f.down.image->get(), rowBytes, rowBytes, rows, hipMemcpyDeviceToHost, *m_CopyStream);
	}
	if (any) JU_HIP(hipStreamSynchronize(*m_CopyStream));
}

// ju_prepare_batch: the graphs of a tuple of frame buffers a caller is going to hand to processBatch, one per
// binding set, captured NOW (as prepareFrames does for one pair): nothing executes, no buffer is touched.  Returns
// the graphs captured; 0 for a tuple that will not go as one pass.
int Engine::prepareBatch(const Frame *in, const Frame *out, int n) {
	if (n < 0 || (n > 0 && (in == nullptr || out == nullptr))) throw std::invalid_argument("prepareBatch: bad arguments");
	DeviceGuard g(m_Device);
	if (n < 2 || n > m_BatchMax || !m_UseGraph || !m_DirectGraph) return 0;
	// (nothing is captured while a stage setting is on, whatever setStageLookahead says; alpha: passEligible, as in mode 0
	// under setAlphaLookahead)
	if (sourceStage()) return 0;
	const std::vector<AnyFrame> anyIn = anyOf(in, n), anyOut = anyOf(out, n);
	for (int i = 0; i < n; ++i) {
		if (!passEligible(anyIn[i], anyOut[i])) return 0;
	}
	if (!batchPlanned(n)) return 0;
	std::unique_lock<std::mutex> chain = chainBegin(m_Resident);  // (no capture while another engine's constructor drains the device)
	int captured = 0;
	for (int set = 0; set < 2; ++set) {
		// (a tuple handed over here keeps its graphs, as registered pairs do: the header promises that process calls on it
		// never capture; only a caller that keeps registering new tuples loses the registered one it used least recently)
		const std::vector<PassKey> key = bindBatch(anyIn.data(), anyOut.data(), n, set, 0);
		m_BatchGraphs.registerUnit(key);
		CachedGraph &e = m_BatchGraphs.use(key);
		if (e.graph.valid()) continue;
		{
			DryLaunchScope dry;  // the attributes of the tile heights this pass's launch sizes choose
			for (const Step &st : m_BatchFlow.at({n, scenePass() == 2 ? kCutSet + set : set})) st.run(m_Stream);
		}
		captured += prepareGraph(e, [&] { runBatch(set, n); });
		e.seen = 2;
	}
	return captured;
}

// One look-ahead pass over frames [0, n): enqueue only.  On return the binding set is flipped ONCE (see above).  The frames
// are counted by runPasses, once the pass has completed.
void Engine::submitBatch(const AnyFrame *in, const AnyFrame *out, int n) {
	const int set = m_Idx;
	const std::vector<PassKey> key = bindBatch(in, out, n, set, stageBits(false));
	uploadPassInputs(in, n);  // (outside the chain lock: a pageable upload blocks its caller)
	m_PassSignalBase = m_PassSignal.host() ? *m_PassSignal.host() : 0u;
	const int scene = scenePass();
	if (scene) {
		// what a captured pass cannot bake in: the detector's kernel reads it from host-mapped memory.  Passes are
		// synchronous, so no launch that reads the block is in flight while it is written.
		auto *dyn = reinterpret_cast<volatile ScenePassDyn *>(m_ScenePassDyn.host());
		const SceneClock &clock = m_Scene.clock();
		dyn->stepBase = clock.steps;
		dyn->seen = clock.memory();
		dyn->thresholdMilli = m_Scene.threshold();
		dyn->slot = static_cast<unsigned>(clock.slot());
		std::atomic_thread_fence(std::memory_order_seq_cst);
	}
	{
		std::unique_lock<std::mutex> chain = chainBegin(m_Resident);
		const auto launches = [&] { runBatch(set, n); };
		if (m_UseGraph && m_DirectGraph) {
			replayOrRun(m_BatchGraphs.use(key), m_BatchGraphs.registered(key), launches);
		} else {
			launches();
			++m_EagerRuns;
		}
		chainEnd(chain, m_Resident);
	}
	m_Idx = set ^ 1;
	if (scene) {  // n detector steps, taken by the pass's one launch
		m_Scene.advance(static_cast<std::uint64_t>(n));
		m_SceneRuns += static_cast<std::uint64_t>(n);
		m_ScenePassFrames += static_cast<std::uint64_t>(n);
	}
}

namespace {
std::atomic<int> g_PassRerun{0}, g_GroupRerun{0};
}  // namespace
void setPassRerun(int on) { g_PassRerun = on; }
void setGroupRerun(int on) { g_GroupRerun = on; }

void Engine::processBatch(const Frame *in, const Frame *out, int count) {
	if (count < 0 || (count > 0 && (in == nullptr || out == nullptr))) throw std::invalid_argument("processBatch: bad arguments");
	const std::vector<AnyFrame> anyIn = anyOf(in, count), anyOut = anyOf(out, count);
	if (sourceStage() || m_AlphaMode != 0) return processFrames(anyIn.data(), anyOut.data(), count);  // (every frame checked before the first runs)
	runPasses(anyIn.data(), anyOut.data(), count);
}

void Engine::processFrames(const AnyFrame *in, const AnyFrame *out, int count) {
	if (count < 0 || (count > 0 && (in == nullptr || out == nullptr))) {
		throw std::invalid_argument("ju_process_frames: NULL frames or a negative count");
	}
	for (int i = 0; i < count; ++i) {
		try {
			checkFrame(in[i], true);  // (every pair, also those that take submit())
			checkFrame(out[i], false);
			checkAlphaOverlap(in[i], out[i]);
		} catch (const std::invalid_argument &e) {
			throw std::invalid_argument("ju_process_frames: frame " + std::to_string(i) + ": " + e.what());
		}
	}
	runPasses(in, out, count);
}

void Engine::runPasses(const AnyFrame *in, const AnyFrame *out, int count) {
	DeviceGuard g(m_Device);
	int i = 0;
	while (i < count) {
		// the longest run of frames from i that can go as one pass: none of them READING what an earlier frame of the
		// pass writes (frame by frame such an input would be read after that write; the pass's flow sweep and its YUV
		// decode read every input first)
		// ... nor WRITING what an earlier frame of the pass reads: on the normal path that write comes after the read
		// (frame k's tail after frame j's, j < k), but a pass whose resident tower timed out is run again frame by frame
		// from its inputs, which must then still be what they were (advisor, round 5).  Every plane of a YUV frame counts.
		FrameExtent reads[kFlowBatchMax], writes[kFlowBatchMax];
		int n = 0;
		while (i + n < count && n < m_BatchMax && passEligible(in[i + n], out[i + n])) {
			reads[n] = extentOf(in[i + n]);
			writes[n] = extentOf(out[i + n]);
			bool clash = false;
			for (int k = 0; k < n && !clash; ++k) clash = overlap(reads[n], writes[k]) || overlap(writes[n], reads[k]);
			if (clash) break;
			++n;
		}
		if (n < 2 || !batchPlanned(n)) {
			runSynchronous(in[i], out[i]);
			++i;
			continue;
		}
		const int set = m_Idx;
		const int scene = scenePass();
		const std::uint64_t firstStep = m_Scene.clock().steps;
		submitBatch(in + i, out + i, n);
		drainPassOutputs(out + i, n);  // host frames: each copied out while the next one runs
		m_Stream.synchronizeSpin(m_SpinUs);
		const unsigned code = takeResidentError();
		if (code || g_PassRerun.load(std::memory_order_relaxed)) {
			// nothing the pass wrote was one of its inputs -- neither the state (see above) nor a frame buffer (the pass
			// splitter): the same frames again, one by one, on the per-block kernels
			// (the frames count as frames, not as a pass's: submitFrame adds a staged one to "source_stage_frames")
			m_Idx = set;
			if (code) fallbackToLayers(code);
			AtExit rerun{[this] { m_SceneRerun = false; }};  // (the pass's detector has run: its n decisions stand, no frame meets it again)
			for (int k = 0; k < n; ++k) {
				if (scene) {
					m_SceneRerun = true;
					// the restart at a cut, as the per-frame detector does it: what this frame is about to read as its
					// recurrent inputs is zero in front of exactly the frames whose record says so (the stream has drained)
					if (scene == 2 && m_Scene.cutAt(firstStep + static_cast<std::uint64_t>(k))) {
						m_State[m_Idx].zeroAsync(m_Stream);
						m_Packed[m_Idx].zeroAsync(m_Stream);
					}
				}
				if (code) {
					submitAny(in[i + k], out[i + k]);
					m_Stream.synchronize();
				} else {  // (the debug switch: the pass was sound, the resident tower still runs and may report)
					runSynchronous(in[i + k], out[i + k]);
				}
			}
		} else {
			// the pass has completed: its frames count as a pass's
			m_BatchFrames += static_cast<std::uint64_t>(n);
			if (m_PassStage) {  // (what the frames went through, whichever route they took: "source_stage_frames" counts them too)
				m_BatchStagedFrames += static_cast<std::uint64_t>(n);
				m_SourceFrames += static_cast<std::uint64_t>(n);
			}
			for (int k = 0; k < n; ++k) {
				m_BatchHostFrames += m_Pass[k].host() ? 1 : 0;
				m_BatchYuvFrames += m_Pass[k].yuv() ? 1 : 0;
				if (alphaLaunches(alphaPass(false), m_Pass[k].alphaOut.kind)) {  // (the launch passTail made for this frame)
					++m_BatchAlphaFrames;
					++m_AlphaFrames;
				}
				maybeRestoreResident();
			}
		}
		i += n;
	}
}

// ---------------------------------------------------------------------------------------------------------------
// Group passes (processGroup).  A server of N live streams has N frames at every tick, one per stream, and their flow
// nets are as independent as a look-ahead pass's: the flow net reads LR frames and each stream's own history only.  So
// the lead (members[0]) runs the flow net's launches ONCE over the n frames of a pass, on its batch tensors -- item i is
// member i's frame with member i's history (flow_block_kernel's independent-items form: PassFrame::groupPrev / groupOut) --
// and then, member by member on the lead's stream, each member's own non-flow steps, bound to its frame, flow item i
// and its state m_State[set_i] -> m_State[set_i ^ 1].  Per member that is the arithmetic of process(): the same kernels
// add the same terms in the same order whatever the launch's size.  Like a look-ahead pass, the pass writes nothing it
// reads (every member's state and history go to the other half of its ping-pong, the overlap test below keeps outputs
// off inputs), so a pass whose resident tower timed out runs again member by member.  The launches are eager: round 6
// measured eager launches per frame equal to graph replay.
//
// Frames of any format (processGroupFrames).  A member's pair is bound as a look-ahead pass binds a frame's (bindFrame on
// the lead: host planes into the lead's slots m_PassSlots, uploaded up front); ONE decode launch in front of
// the flow net covers every non-BGRX input of the pass (the items form of processFrames), and each member's encode sits
// behind that member's own steps on the lead's stream -- a deep format from THAT member's f16 state, the half its step
// just wrote.  Members under a source size, an output size or a mask stay on the staged single-frame route unless they
// asked to ride (setStageGroup, below).
//
// The scene detector inside a group pass (setSceneGroup; docs/scene_detect.md "Group passes").  The members are
// independent streams, so no cut-aware history is needed: scene_group_kernel takes the decision of every detecting
// member in ONE launch behind the decode launch -- item i against member i's own kept frame, from and into member i's
// own SceneState and ring -- and scene_clear_items_kernel zeroes, in ONE more launch, m_State[set_i] and m_Packed[set_i]
// of the members whose flag was raised: exactly what the per-frame scene_clear_kernel covers, in front of the flow net
// that reads m_Packed[set_i] as item i's groupPrev.  One exception to "writes nothing it reads", as in a look-ahead pass: those
// two buffers may be zeroed -- which is what the re-run of the members, whose decisions stand (m_SceneRerun), wants to
// find there too.
//
// Scaled and masked members inside a group pass (setStageGroup; docs/source_stage.md and docs/output_stage.md, "Group
// passes").  The stages sit outside the recurrence, so a pass takes them as a staged look-ahead pass does, per member
// instead of per frame: host planes upload and non-BGRX inputs decode at each member's OWN size (the decode launch's sized
// form), ONE launch (scale_bgrx_members_kernel: every member with its own source size, tables and filter form) scales the
// sources of all scaled members to the model's input in front of the group scene launch and the flow net, and behind each
// member's own steps follow that member's blend in place, its output scaler and its encode -- the single-frame launches
// with the member's own Scaler and mask.  What the network reads and writes in between are the member's own model-size
// slots (m_GroupSlots; bindGroup).
//
// A pass that runs again.  The blend rewrites the model-size frame in place, and the scale launch, the decode and the
// uploads fill slots -- but every one of those is either a slot the pass alone writes (the lead's, the member's own) or the
// caller's OUTPUT, never one of the call's inputs: the overlap test of processGroupFrames keeps every output plane, at its
// true size, off every input plane, and the states and histories go to the other halves.  The re-run of a member goes
// through its own process(), i.e. submitFrame, which stages again from the caller's source into the member's single-frame
// staging buffers and recomputes blend, scale and encode from there; it reads nothing the pass wrote.  So the bytes of a
// re-run are those of the member run alone, and "source_stage_frames" counts the frame once, by submitFrame.
// ---------------------------------------------------------------------------------------------------------------
bool Engine::sameModel(const Engine &o) const {
	return m_Device == o.m_Device && m_ModelDigest == o.m_ModelDigest && m_DtypeOverride == o.m_DtypeOverride;
}

void Engine::processGroup(Engine *const *members, const Frame *bgrxIn, const Frame *bgrxOut, int count,
    const std::function<void(bool)> &underPass, hipEvent_t after) {
	if (count < 0 || (count > 0 && (members == nullptr || bgrxIn == nullptr || bgrxOut == nullptr))) {
		throw std::invalid_argument("ju_process_group: NULL arguments or a negative count");
	}
	if (count == 0) return;
	const std::vector<AnyFrame> in = anyOf(bgrxIn, count), out = anyOf(bgrxOut, count);
	processGroupFrames(members, in.data(), out.data(), count, "ju_process_group", false, underPass, after);
}

// The caller's host work (underPass) exactly once per call: under the first group pass the call forms, else -- no pass, or
// an argument refused before one -- not at all (a refusal) or behind the members' frames, before the call returns.
void Engine::processGroupFrames(Engine *const *members, const AnyFrame *in, const AnyFrame *out, int count, const char *who,
    bool indexed, const std::function<void(bool)> &underPass, hipEvent_t after) {
	if (!underPass) return runGroups(members, in, out, count, who, indexed, underPass, after);
	bool ran = false;
	const std::function<void(bool)> once = [&](bool inPass) {
		if (ran) return;
		ran = true;
		underPass(inPass);
	};
	runGroups(members, in, out, count, who, indexed, once, after);
	if (count > 0) once(false);
}

void Engine::runGroups(Engine *const *members, const AnyFrame *in, const AnyFrame *out, int count, const char *who, bool indexed,
    const std::function<void(bool)> &underPass, hipEvent_t after) {
	const std::string name = who;
	if (count < 0 || (count > 0 && (members == nullptr || in == nullptr || out == nullptr))) {
		throw std::invalid_argument(name + ": NULL arguments or a negative count");
	}
	if (count == 0) return;
	std::set<const Engine *> seen;
	for (int i = 0; i < count; ++i) {
		if (members[i] == nullptr) throw std::invalid_argument(name + ": runtime " + std::to_string(i) + " is NULL");
		if (!seen.insert(members[i]).second) {
			throw std::invalid_argument(name + ": runtime " + std::to_string(i) + " appears twice");
		}
		if (!members[i]->sameModel(*members[0])) {
			throw std::invalid_argument(name + ": runtime " + std::to_string(i) +
			                            " does not match runtime 0 (device, model bytes or dtype)");
		}
		// what process() would refuse, up front: a group call launches nothing before every frame passed
		try {
			members[i]->checkFrame(in[i], true, who, true);
			members[i]->checkFrame(out[i], false, who, true);
			members[i]->checkAlphaOverlap(in[i], out[i]);
		} catch (const std::invalid_argument &e) {
			if (!indexed) throw;
			// ("<who>: <why>" -> "<who>: member i: <why>")
			const std::string what = e.what(), prefix = name + ": ";
			throw std::invalid_argument(prefix + "member " + std::to_string(i) + ": " +
			                            (what.compare(0, prefix.size(), prefix) == 0 ? what.substr(prefix.size()) : what));
		}
	}
	Engine &lead = *members[0];
	DeviceGuard g(lead.m_Device);
	auto alone = [&](int i) {
		// (a member on its own runs on its own stream: behind `after` there)
		if (after) JU_HIP(hipStreamWaitEvent(members[i]->m_Stream, after, 0));
		members[i]->process(in[i], out[i]);
	};
	if (count == 1) return alone(0);
	// An output over an input of the call (same address space; any two members, also one member's own pair; every plane
	// of a frame counts): member by member in list order, as ju_process_frame calls would run -- a pass reads every input
	// before any tail writes
	bool clash = false;
	for (int i = 0; i < count && !clash; ++i) {
		const FrameExtent w = extentOf(out[i]);
		for (int j = 0; j < count && !clash; ++j) clash = overlap(w, extentOf(in[j]));
	}
	std::vector<int> pass, rest;
	// (a detecting runtime stays member by member unless it asked to ride: setSceneGroup -- the pass then carries its detector)
	for (int i = 0; i < count; ++i) {
		// (a scaled or masked member stays on the staged single-frame route, whatever setStageLookahead says, unless it asked
		// to ride: setStageGroup -- passEligible then judges its pair as a staged look-ahead frame's, at its own sizes)
		(members[i]->passEligible(in[i], out[i], true) ? pass : rest).push_back(i);
	}
	const int cap = lead.m_BatchMax;
	if (clash || pass.size() < 2 || cap < 2) {
		for (int i = 0; i < count; ++i) alone(i);
		return;
	}
	// consecutive passes of at most the lead's look-ahead cap; a pass of one member is a plain process()
	for (std::size_t k = 0; k < pass.size(); k += static_cast<std::size_t>(cap)) {
		const int n = static_cast<int>(std::min(pass.size() - k, static_cast<std::size_t>(cap)));
		if (n < 2 || !lead.batchPlanned(n, true)) {
			for (int j = 0; j < n; ++j) alone(pass[k + j]);
			continue;
		}
		Engine *m[kFlowBatchMax];
		AnyFrame fi[kFlowBatchMax], fo[kFlowBatchMax];
		for (int j = 0; j < n; ++j) {
			m[j] = members[pass[k + j]];
			fi[j] = in[pass[k + j]];
			fo[j] = out[pass[k + j]];
		}
		runGroupPass(lead, m, fi, fo, n, underPass, after);
	}
	// frames a pass cannot take (graphics resources, device frames off the kernels' alignment): on their own.  No
	// buffer of the call overlaps another here, so the order changes no byte.
	for (int i : rest) alone(i);
}

void Engine::runGroupPass(Engine &L, Engine *const *m, const AnyFrame *in, const AnyFrame *out, int n,
    const std::function<void(bool)> &underPass, hipEvent_t after) {
	// everything of the pass runs on the lead's stream (the uploads too): ONE wait puts it behind `after`
	if (after) JU_HIP(hipStreamWaitEvent(L.m_Stream, after, 0));
	int sets[kFlowBatchMax];
	for (int i = 0; i < n; ++i) sets[i] = m[i]->m_Idx;
	// what each member brings along (setStageGroup): bit 0 its source scaler, bit 1 its mask, bit 2 its output scaler
	int stage[kFlowBatchMax];
	bool anyScaledIn = false;
	for (int i = 0; i < n; ++i) {
		stage[i] = m[i]->stageBits(true);
		anyScaledIn = anyScaledIn || (stage[i] & 1) != 0;
	}
	// L.m_Pass[i].io: what member i's network reads and writes (a host frame through L.m_PassSlots[i], a scaled side through
	// member i's own model-size slot); .ends: member i's rows at its own source / output size
	L.bindGroup(m, in, out, n, stage);
	AtExit unbind{[&L, n] {  // (the lead keeps no pointer to a member's slots beyond the pass)
		for (int i = 0; i < n; ++i) L.m_Pass[i].up = L.m_Pass[i].down = PassCopy{};
	}};
	L.uploadPassInputs(in, n);  // (each at its member's own size; outside the chain lock: a pageable upload blocks its caller)
	L.m_PassSignalBase = L.m_PassSignal.host() ? *L.m_PassSignal.host() : 0u;
	// The detecting members (they ride because they asked to: setSceneGroup).  What their decisions read that varies from
	// tick to tick goes into each member's own host-mapped words; the pass is synchronous, so nothing reads them now.
	bool detects[kFlowBatchMax] = {};
	bool anyDetects = false, anyRestarts = false;
	for (int i = 0; i < n; ++i) {
		Engine &e = *m[i];
		detects[i] = e.m_Scene.mode() != 0;
		if (!detects[i]) continue;
		anyDetects = true;
		// (a flow-free model has no recurrent input to clear: JU_SCENE_RESET reports)
		const bool restarts = e.m_Scene.mode() == 2 && e.m_Config.recurrent();
		anyRestarts = anyRestarts || restarts;
		auto *dyn = reinterpret_cast<volatile SceneGroupDyn *>(e.m_SceneGroupDyn.host());
		const SceneClock &clock = e.m_Scene.clock();
		dyn->step = clock.steps;
		dyn->slotHasPrev = static_cast<unsigned long long>(clock.slot()) | (static_cast<unsigned long long>(clock.hasPrev()) << 32);
		dyn->thresholdMode = static_cast<unsigned long long>(e.m_Scene.threshold()) | (static_cast<unsigned long long>(restarts ? 2 : 1) << 32);
	}
	if (anyDetects) std::atomic_thread_fence(std::memory_order_seq_cst);
	// 1. work a member has pending on its own stream (ju_enqueue) runs first
	for (int i = 0; i < n; ++i) {
		if (m[i] == &L) continue;
		const hipError_t st = hipStreamQuery(m[i]->m_Stream);
		if (st == hipSuccess) continue;  // (idle: everything it was given has completed)
		if (st != hipErrorNotReady) JU_HIP(st);
		m[i]->m_GroupEvent.record(m[i]->m_Stream);
		JU_HIP(hipStreamWaitEvent(L.m_Stream, m[i]->m_GroupEvent.get(), 0));
	}
	const bool recurrent = L.m_Config.recurrent();
	const long flowItem = recurrent ? static_cast<long>(L.m_Tensors.at("flow").count) * 2 : 0;
	const unsigned char *flowBase = recurrent ? L.m_BatchTensors.at("flow").buf.as<unsigned char>() : nullptr;
	{
		// 5. the device chain, once for the whole pass (chainBegin / chainEnd, for a pass that may hold several
		// members' resident towers): ordered after the frame submitted last by any other resident runtime, and any
		// member's next frame is ordered after the pass (lastOwner = the lead)
		bool resident = false;
		for (int i = 0; i < n; ++i) resident = resident || m[i]->m_Resident;
		std::unique_lock<std::mutex> chain = L.chainBegin(resident);
		// 2a. the pass's non-BGRX inputs into their members' BGRX slots, all in ONE launch (runBatch's): each at its own
		// size -- a scaled member's at its source size into its source-size slot, the others' at the model's into the lead's
		// slots.  While no member of the pass is scaled that is the launch of one size, unchanged.
		const FrameSize fs = L.frameSize();
		YuvDecodeSizedItems items{};
		int decodes = 0;
		for (int i = 0; i < n; ++i) {
			const PassFrame &f = L.m_Pass[i];
			if (!f.in.yuv) continue;
			items.width[decodes] = static_cast<int>(f.size.inW);
			items.height[decodes] = static_cast<int>(f.size.inH);
			items.item[decodes++] = yuvDecodeItem(fmt(f.in.format), f.in.colorspace, f.in.planes, const_cast<std::uint8_t *>(f.ends.in),
			    f.ends.inStride);
		}
		if (decodes && anyScaledIn) {
			launchYuvToBgrxItemsSized(items, decodes, L.m_Stream);
		} else if (decodes) {
			YuvDecodeItems same{};
			for (int k = 0; k < decodes; ++k) same.item[k] = items.item[k];
			launchYuv420ToBgrxItems(same, decodes, static_cast<int>(fs.inputWidth), static_cast<int>(fs.inputHeight), L.m_Stream);
		}
		// 2a'. ONE launch scales the sources of all scaled members -- the caller's device images where they are, the upload
		// slots, the slots the decode launch above fills -- each through its own member's tables into that member's model-size
		// input, in front of the detector and the flow net, which therefore read exactly what submitFrame gives them
		if (anyScaledIn) {
			ScaleMembers scale{};
			int scaled = 0;
			for (int i = 0; i < n; ++i) {
				if (!(stage[i] & 1)) continue;
				const PassFrame &f = L.m_Pass[i];
				scale.member[scaled++] = m[i]->m_SrcScale.member(f.ends.in, f.ends.inStride, const_cast<std::uint8_t *>(f.io.in), f.io.inStride);
			}
			launchScaleBgrxMembers(scale, scaled, static_cast<int>(fs.inputWidth), static_cast<int>(fs.inputHeight), L.m_Stream);
		}
		// 2b. the scene detector inside a group pass: every member's frame is in place (the caller's device frame, the lead's
		// upload slot, the slot the decode launch fills), so ONE launch takes the decision of every detecting member -- each
		// against its OWN kept frame, state and ring (the streams are independent: no cut-aware history) -- and ONE more
		// clears, for the members whose flag it raised, what their step is about to read as its recurrent inputs:
		// m_State[set_i] and m_Packed[set_i], the half the first flow block reads as its groupPrev.  After it a cut
		// member's whole history is zero, which is what reset() leaves.
		if (anyDetects) {
			SceneGroupLaunch q;
			q.items = n;
			q.width = static_cast<int>(fs.inputWidth);
			q.height = static_cast<int>(fs.inputHeight);
			SceneClearItem clears[kFlowBatchMax];
			for (int i = 0; i < n; ++i) {
				if (!detects[i]) continue;
				Engine &e = *m[i];
				SceneGroupItem &it = q.item[i];
				it.frame = L.m_Pass[i].io.in;
				it.stride = L.m_Pass[i].io.inStride;
				it.prev = e.m_Scene.prev();
				it.state = e.m_Scene.state();
				it.ring = e.m_Scene.ring();
				it.dyn = reinterpret_cast<const SceneGroupDyn *>(e.m_SceneGroupDyn.device());
				if (e.m_Scene.mode() == 2 && recurrent) {
					clears[i] = SceneClearItem{&it.state->resetNow, e.m_State[sets[i]].get(), e.m_State[sets[i]].bytes(),
					    e.m_Packed[sets[i]].get(), e.m_Packed[sets[i]].bytes()};
				}
			}
			launchSceneGroup(q, L.m_Stream);
			if (anyRestarts) launchSceneClearItems(clears, n, L.m_Stream);
			for (int i = 0; i < n; ++i) {  // one detector step per detecting member, taken by the pass's one launch
				if (!detects[i]) continue;
				m[i]->m_Scene.advance();
				++m[i]->m_SceneRuns;
				++m[i]->m_SceneGroupFrames;
			}
		}
		// 2. the flow net once over all items
		for (int i = 0; i < n; ++i) {
			L.m_Pass[i].groupPrev = m[i]->m_Packed[sets[i]].get();
			L.m_Pass[i].groupOut = m[i]->m_Packed[sets[i] ^ 1].get();
		}
		for (const Step &st : L.m_BatchFlow.at({n, kGroupSet})) st.run(L.m_Stream);
		// 3. member by member, its own steps on the lead's stream, bound to its frame and its flow item
		for (int i = 0; i < n; ++i) {
			Engine &e = *m[i];
			AtExit restore{[&e, keepIO = e.m_IO, keepFlow = e.m_FlowCur] {
				e.m_IO = keepIO;
				e.m_FlowCur = keepFlow;
			}};
			e.m_IO = L.m_Pass[i].io;
			if (recurrent) e.m_FlowCur = flowBase + i * flowItem;
			for (const Step &st : e.m_Program[sets[i]]) {
				if (st.tag != "flow" && st.tag != "pack") st.run(L.m_Stream);
			}
			// behind member i's own steps, on the lead's stream, with member i's own mask, scaler and 16-bit slot; the state
			// its step just wrote: its own m_State[set_i ^ 1] (a flow-free member: its one scratch state)
			L.passTail(e, L.m_Pass[i], stage[i], e.m_State[recurrent ? sets[i] ^ 1 : 0].get(), e.m_GroupSlots.out16);
		}
		L.chainEnd(chain, resident);
	}
	// 4. every member's stream after the pass
	L.m_GroupEvent.record(L.m_Stream);
	for (int i = 0; i < n; ++i) {
		if (m[i] != &L) JU_HIP(hipStreamWaitEvent(m[i]->m_Stream, L.m_GroupEvent.get(), 0));
	}
	L.drainPassOutputs(out, n);  // host frames: each copied out while the next member runs
	// the caller's host work under the pass: everything is enqueued and the chain lock is released, so it may block (a
	// pageable copy) while the GPU runs the pass.  Here and nowhere else: the re-run below does not repeat it.
	if (underPass) underPass(true);
	L.m_Stream.synchronizeSpin(L.m_SpinUs);
	// one synchronisation; then every member's resident-tower error word
	unsigned codes[kFlowBatchMax];
	bool failed = false;
	for (int i = 0; i < n; ++i) {
		codes[i] = m[i]->takeResidentError();
		failed = failed || codes[i] != 0;
	}
	if (failed || g_GroupRerun.load(std::memory_order_relaxed)) {
		// nothing the pass wrote is one of its inputs: the same frames again, member by member, each through its own
		// process() -- a member whose tower timed out on its per-block kernels from now on
		for (int i = 0; i < n; ++i) {
			if (codes[i]) m[i]->fallbackToLayers(codes[i]);
		}
		for (int i = 0; i < n; ++i) {
			// (the pass's detector has run: the member's decision stands, its kept frame is this frame already and, after a
			// cut, its cleared inputs are still in place -- the pass wrote the other halves only; no step meets it again)
			AtExit rerun{[e = m[i]] { e->m_SceneRerun = false; }};
			m[i]->m_SceneRerun = detects[i];
			m[i]->process(in[i], out[i]);
		}
		return;
	}
	for (int i = 0; i < n; ++i) {
		m[i]->m_Idx = sets[i] ^ 1;
		++m[i]->m_GroupFrames;
		m[i]->m_GroupYuvFrames += L.m_Pass[i].yuv() ? 1 : 0;
		if (stage[i]) {  // (what the frame went through, whichever route it took: "source_stage_frames" counts it too)
			++m[i]->m_GroupStagedFrames;
			++m[i]->m_SourceFrames;
		}
		if (alphaLaunches(m[i]->alphaPass(true), L.m_Pass[i].alphaOut.kind)) {  // (the launch passTail made for this member)
			++m[i]->m_GroupAlphaFrames;
			++m[i]->m_AlphaFrames;
		}
		m[i]->maybeRestoreResident();
	}
}

}  // namespace ju
