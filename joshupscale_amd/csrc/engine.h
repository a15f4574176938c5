// The per-frame recurrent super-resolution engine (MI355X / gfx950).
//
// Replaces the reference's TensorRTBackend (reference
// core/include/JoshUpscale/core/tensorrt_backend.h:20-53,
// core/src/tensorrt_backend.cc:117-288): same contract — construct from model
// bytes on the current device, `process(in, out)` = stage-in, one execution of
// the inference graph against binding set `idx`, stage-out, synchronise, flip
// `idx` — but the graph is this engine's own schedule of hand-written HIP
// kernels (*_kernels.hip) captured into two hipGraphs instead of a TensorRT
// execution context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "frame_io.h"
#include "graph_cache.h"
#include "hip_util.h"
#include "kernels.h"
#include "model.h"
#include "scene_detector.h"

namespace ju {

// runs f when the scope ends, also by an exception: what a call rebinds for its launches goes back to what it was
template <typename F>
struct AtExit {
	F f;
	~AtExit() { f(); }
};
template <typename F>
AtExit(F) -> AtExit<F>;

struct FrameSize {
	std::size_t inputWidth, inputHeight, outputWidth, outputHeight;
};

// Test flavour only (ju_debug_set "pass_rerun"): a look-ahead pass that completed normally is treated as one that must
// be run again -- binding set and counters restored, its frames one by one, without the fallback to the per-block kernels.
void setPassRerun(int on);
// Test flavour only (ju_debug_set "step_rerun"): process() treats every frame that completed normally as one whose
// resident tower reported -- binding set restored, the frame submitted again -- without the fallback to the per-block kernels.
void setStepRerun(int on);
// Test flavour only (ju_debug_set "group_rerun"): "pass_rerun" for group passes -- a group pass that completed normally
// is treated as one that must be run again: its members one by one through process(), without the detector.
void setGroupRerun(int on);

class Engine {
public:
	// dtypeOverride: -1 = the container's hint, else kF16 / kBF16.
	Engine(int device, const void *blob, std::size_t size, int dtypeOverride);
	~Engine();
	Engine(const Engine &) = delete;
	Engine &operator=(const Engine &) = delete;

	// One frame, synchronously, like Runtime::processImage (tensorrt_backend.cc:270-278): ju_process and ju_process_frame.
	// A BGRX pair while no source or output stage is set takes the caller's pointers or the staging copies (submit) and
	// is refused, if at all, where it is staged -- exactly as ju_process always behaved.  Every other pair -- a YUV side,
	// whose colour conversion takes the place of the staging copy on that side (colour_kernels.hip), or any pair while a
	// stage is set -- is checked before anything is launched and goes through the staging buffers (submitFrame).
	void process(const AnyFrame &in, const AnyFrame &out);
	// `count` consecutive frames of the stream, synchronously: the frames process(in[0], out[0]) ...
	// process(in[count - 1], out[count - 1]) would write, byte for byte -- but every input must hold its pixels when
	// the call is made (frame look-ahead): where the model and the frames allow (device-resident frames, the flow
	// auto-encoder's one-launch plan) the flow fields of up to kFlowBatchMax frames are computed in one pass of the
	// flow net's launches (engine_passes.cpp, "Frame look-ahead"); anything else runs frame by frame.
	void processBatch(const Frame *in, const Frame *out, int count);
	// Registers a tuple of device-resident frame buffers the caller is going to hand to processBatch as ONE pass
	// (2 .. JU_LOOKAHEAD frames): its graphs, one per binding set, are captured now -- what prepareFrames is to
	// process.  Nothing executes.  Returns the graphs captured (0: the tuple will not go as one pass).
	int prepareBatch(const Frame *in, const Frame *out, int count);
	// Frames per look-ahead pass, 1 (off) .. kFlowBatchMax, clamped.  Default: kFlowBatchMax, or JU_LOOKAHEAD at creation.
	void setLookahead(int frames);
	int lookahead() const { return m_BatchMax; }  // (also the most members one group pass holds)
	// One frame for each of `count` runtimes, synchronously: the bytes process(in[i], out[i]) for i = 0 .. count - 1 would
	// write, in every output and every member's state.  The members (distinct, one device, byte-identical model data,
	// one dtype override: std::invalid_argument otherwise, before anything is launched) share a pass where they can:
	// members[0] (the lead) runs the flow net ONCE over up to its look-ahead cap of frames, each the next frame of its
	// own stream, then every member's own recurrent steps, all on the lead's stream (engine_passes.cpp, "Group passes").
	// underPass (empty by default: exactly the launches of before): host work of the caller's to run ONCE per call while
	// the GPU runs the call's frames -- a group pass runs it between its last enqueue and its wait, behind chainEnd (it may
	// block: a pageable copy), with `true`; a call that forms no pass runs it exactly once all the same, before returning,
	// with `false` (nothing ran under it); a pass that has to be run again does not repeat it (the tiled runtime's deferred
	// copy-out: tiled.cpp).
	// after (null by default): everything the call launches runs behind that event -- a wait of the pass's lead's stream, or
	// of a member's own stream where the member runs on its own; no host wait (the tiled runtime orders a frame's group
	// passes behind the previous frame's stitch with it: tiled.cpp).
	static void processGroup(Engine *const *members, const Frame *in, const Frame *out, int count,
	    const std::function<void(bool)> &underPass = {}, hipEvent_t after = nullptr);
	// processGroup for frames of any format (ju_process_group_frames): formats, colour spaces, locations and strides are
	// independent per member and side.  EVERY pair is checked before anything is launched or uploaded (std::invalid_argument
	// names the member).  A pass decodes all its non-BGRX inputs in one launch in front of the flow net's and encodes each
	// member's output behind that member's own steps -- a deep format from THAT member's f16 state (engine_passes.cpp,
	// "Group passes").  who: the entry point in the messages; indexed: checkFrame's refusals name the member too.
	static void processGroupFrames(Engine *const *members, const AnyFrame *in, const AnyFrame *out, int count,
	    const char *who = "ju_process_group_frames", bool indexed = true, const std::function<void(bool)> &underPass = {},
	    hipEvent_t after = nullptr);
	// process() for device-resident frames without the wait (ju_enqueue, ju_enqueue_frame): enqueue only.
	void enqueue(const AnyFrame &in, const AnyFrame &out);
	void synchronize();
	// processBatch for frames of any format (ju_process_frames): the bytes and the state of process called frame by
	// frame in order.  EVERY pair is checked before anything is launched or uploaded (std::invalid_argument names
	// the frame; runtime and state as they were).  YUV sides ride in the passes: the pass's YUV inputs are decoded by one
	// launch in front of the flow net's, each YUV output is encoded behind its frame's tail (engine_passes.cpp, "YUV
	// frames in look-ahead passes").
	void processFrames(const AnyFrame *in, const AnyFrame *out, int count);
	// Registers a pair of device-resident frame buffers the caller is going to hand to
	// process() / enqueue(): the per-frame graphs of the pair (one per binding set) are
	// captured NOW, so that no later call pays a capture -- the reference captures its graphs
	// in the constructor too, never inside process (tensorrt_backend.cc:257-263).  Nothing
	// executes and the buffers are not touched.  Pairs that cannot take the direct path
	// (host frames, graphics resources, odd alignment) need nothing: their frames go through
	// the staging buffers, whose graphs the constructor captured.  Returns the number of
	// graphs captured by this call (0 when the pair was registered before).
	int prepareFrames(const Frame &in, const Frame &out);
	// Zero the recurrent state (what destroying and recreating the runtime does
	// in the reference: obs_plugin/src/filter.cc:146-151).
	void reset();

	// The source stage (docs/source_stage.md; engine_frames.cpp, "Source stage").  setSourceSize: input frames are
	// width x height from now on and are scaled to the model's input on the GPU ((0, 0): off; filter: a JU_SCALE_* value --
	// 0 triangle, 2 Catmull-Rom, 3 Mitchell).  setSourceMask: a BGRX image of any size, host or device, copied now (nullptr: no mask); the source is
	// drawn over every output frame through it.  While either is set every frame of every entry point runs one by one
	// through the staged path of submitFrame -- but for the look-ahead passes setStageLookahead allows and the group passes
	// setStageGroup allows.  reset() keeps both.
	void setSourceSize(std::size_t width, std::size_t height, int filter);
	void sourceSize(std::size_t *width, std::size_t *height) const;
	void setSourceMask(const Frame *mask);
	// The output stage (docs/output_stage.md; engine_frames.cpp, "Output stage").  setOutputSize: output frames are
	// width x height from now on -- the upscaled frame scaled on the GPU behind the graph and the mask blend ((0, 0): off;
	// filter: a JU_SCALE_* value, as for the source size).  State, frame history and flow inputs are the unscaled run's.  While it is set
	// every frame of every entry point runs one by one through submitFrame, as for a source size (setStageLookahead: the
	// look-ahead passes carry it; setStageGroup: the group passes).  reset() keeps it.
	void setOutputSize(std::size_t width, std::size_t height, int filter);
	void outputSize(std::size_t *width, std::size_t *height) const;
	// The alpha channel (docs/alpha.md; engine_frames.cpp, "Alpha").  setAlpha: mode JU_ALPHA_ZERO (the slot stays 0: no
	// launch, every route as without the setting), JU_ALPHA_OPAQUE (the format's top code) or JU_ALPHA_SOURCE (the input
	// frame's alpha scaled by `filter`, a JU_SCALE_* value, from the input frame's size straight to the output frame's
	// size); the filter is checked in every mode.  While the mode is not 0 every frame of every entry point runs one by
	// one through submitFrame, whatever setStageLookahead / setStageGroup say, and one launch follows the frame's colour --
	// unless setAlphaLookahead / setAlphaGroup let the passes carry that launch.  Waits for the stream; reset() keeps it.
	void setAlpha(int mode, int filter);
	void alpha(int *mode, int *filter) const;
	// Look-ahead passes while the alpha mode is not 0 (ju_set_alpha_lookahead; engine_passes.cpp, "Alpha inside a pass"):
	// 0 (default) = such a runtime's frames run one by one through submitFrame, 1 = the mode no longer keeps
	// processBatch / processFrames from forming passes (the stage and scene settings decide as in mode 0), and each
	// frame's one alpha launch follows its colour inside the pass.  Waits for the stream; reset() and setAlpha() keep it.
	void setAlphaLookahead(int on);
	// Group passes while the alpha mode is not 0 (ju_set_alpha_group): 0 (default) = processGroup / processGroupFrames run
	// this runtime on its own, 1 = it rides, and the pass makes its alpha launch with its own mode, filter and tables.
	// Independent of setAlphaLookahead.  Waits for the stream; reset() and setAlpha() keep it.
	void setAlphaGroup(int on);
	bool sourceStage() const { return m_SrcScale.set() || m_Mask.on() || m_OutScale.set(); }
	// The scene detector (docs/scene_detect.md; "Scene detector" below).  setSceneDetect: mode 0 off / 1 report / 2 reset
	// (JU_SCENE_*), thresholdMilli 1 .. 255000 while the mode is not off; waits for the stream; a call that changes the
	// mode starts the detector over (no predecessor, step 0).  reset() keeps the setting and forgets the predecessors.
	void setSceneDetect(int mode, std::uint32_t thresholdMilli);
	void sceneDetect(int *mode, std::uint32_t *thresholdMilli) const;
	// the most recent min(count, 64, steps seen) records, oldest first, after waiting for the stream; returns how many
	int sceneInfo(SceneRecord *out, int count);
	// Look-ahead passes while the detector is on (ju_set_scene_lookahead; engine_passes.cpp, "The scene detector inside
	// a pass"): 0 (default) = such a runtime's frames run one by one, 1 = passes are formed and carry the detector.
	// Waits for the stream; reset() and setSceneDetect() keep it.
	void setSceneLookahead(int on);
	// Group passes while the detector is on (ju_set_scene_group; engine_passes.cpp, "The scene detector inside a group
	// pass"): 0 (default) = processGroup runs this runtime on its own, 1 = it rides in the passes, which carry its
	// detector.  Waits for the stream; reset() and setSceneDetect() keep it.
	void setSceneGroup(int on);
	// Look-ahead passes while a source size, a mask or an output size is set (ju_set_stage_lookahead; engine_passes.cpp,
	// "Scaled and masked frames inside a pass"): 0 (default) = such a runtime's frames run one by one through submitFrame,
	// 1 = processBatch / processFrames form passes that carry the stages.  Waits for the stream; reset() keeps it.
	void setStageLookahead(int on);
	// Group passes while a source size, a mask or an output size is set (ju_set_stage_group; engine_passes.cpp, "Scaled and
	// masked members inside a group pass"): 0 (default) = processGroup / processGroupFrames run such a runtime on its own
	// through submitFrame, 1 = it rides in the passes, which carry its stages.  Independent of setStageLookahead.  Waits for
	// the stream; reset() keeps it.
	void setStageGroup(int on);

	FrameSize frameSize() const;
	int device() const { return m_Device; }
	DType dtype() const { return m_DType; }
	// JU_DTYPE_* as reported to the caller: 2 when the block convolutions run in e4m3
	int reportedDtype() const { return m_Fp8Tower ? 2 : static_cast<int>(m_DType); }
	const ModelConfig &config() const { return m_Config; }
	// The f16 state [4H][4W][4] (B, G, R, 0) the last frame left, on the device; valid after a synchronous call.  A frame
	// writes m_State[m_Idx ^ 1] and its call then flips m_Idx (what stageOutScaled and submitFrame read BEFORE the flip), so
	// behind the call it is m_State[m_Idx] -- readTensor's "state".  A flow-free model: its one scratch state.
	const void *lastState() const { return m_State[m_Config.recurrent() ? m_Idx : 0].get(); }
	// The two buffers the NEXT frame of a recurrent model reads as its recurrent inputs -- m_State[m_Idx] and m_Packed[m_Idx],
	// what sceneStep clears at a cut and reset() leaves zero -- as a conditional clear takes them (its flag left null).  The
	// tiled runtime's scene detector (tiled.cpp); valid between synchronous calls.
	SceneClearItem recurrentInputs() const {
		return SceneClearItem{nullptr, m_State[m_Idx].get(), m_State[m_Idx].bytes(), m_Packed[m_Idx].get(), m_Packed[m_Idx].bytes()};
	}
	void setUseGraph(bool on) { m_UseGraph = on; }

	// ---- introspection (tests, bench) ----
	// Copies a named internal tensor to host as f32; returns its element count
	// (call with dst == nullptr to query).  Names: see Engine::tensorNames().
	std::size_t readTensor(const std::string &name, float *dst, std::size_t capacity);
	std::vector<std::string> tensorNames() const;
	// Average device time (ms) of one launch of the steps carrying `tag`, measured
	// with HIP events on the engine's own stream over `iters` repetitions of that
	// group; *launches receives the number of kernel launches per repetition.  The timed
	// launches overwrite scratch tensors and possibly the recurrent state: the stream is
	// reset() afterwards (callers time AFTER their frames, as bench.py does).
	double timeSteps(const std::string &tag, int iters, int *launches);
	// FLOPs (2*MAC) of the steps carrying `tag` (one repetition).
	double flopsOf(const std::string &tag) const;
	// "graph_replays", "eager_runs", "direct_graphs", "resident_tower", "resident_flow",
	// "launches_per_frame"
	double stat(const std::string &key) const;
	// Test flavour only: what the launchers of the flow net's convolution kernels (and the residual-block launcher)
	// really launched for this runtime so far, one line per distinct launch (kernels.h PlanLog; the lines:
	// include/joshupscale_amd_test.h ju_plan_report).  Empty in the product library.
	std::string planReport() const { return m_PlanLog.text(); }

private:
	struct Tensor {
		DeviceBuffer buf;
		std::size_t count = 0;
		bool isF32 = false;
		bool isState = false;  // f16 regardless of the compute dtype
		int towerH = 0, towerW = 0, towerC = 0;  // != 0: zero-bordered tower layout
	};
	// A tensor as a conv operand: pointer to image pixel (0,0) + row pitch in pixels
	// (0 = dense).
	struct Operand {
		void *ptr = nullptr;
		int pitch = 0;
	};
	struct Step {
		std::string tag;
		double flops;
		std::function<void(hipStream_t)> run;
	};
	struct ConvWeights {
		DeviceBuffer w;
		DeviceBuffer wBlock;  // 64 -> 64 block convolutions: a second copy packed with nb = 1 for flow_block_kernel
		DeviceBuffer bias;
		int cinP = 0, cout = 0, taps = 9, cinReal = 0;
		int nb = 2, rw = 2;  // tile shape the weights were packed for
		bool splitK = false;  // a coarse flow layer that runs as conv_splitk_kernel (packed with nb = 1)
	};

	Tensor &addTensor(const std::string &name, std::size_t count, bool f32 = false,
	    bool state = false);
	// H x W: the resolution the layer runs at (decides its tile shape)
	ConvWeights &addConv(const std::string &name, const FoldedConv &f,
	    const std::vector<int> &cinMap, int H, int W);
	struct ItemStride {  // a look-ahead launch: the layer of `items` frames, their tensors `in` / `out` bytes apart
		int items;
		long in, out;
		ItemStride(int n = 1, long i = 0, long o = 0) : items(n), in(i), out(o) {}
	};
	// ---- the program builder (engine_program.cpp) ----
	// what a convolution's launch does besides the convolution; `tower`: conv_tower_kernel on tower-layout operands
	struct ConvOpt {
		bool relu = false, outHead = false, tower = false, pool = false, upsample = false;
		ItemStride item;
	};
	void addConvStep(std::vector<Step> *prog, const std::string &tag, const std::string &wname, Operand in, Operand res,
	    Operand out, int H, int W, const ConvOpt &opt);
	// group: the launches of a group pass (independent items: processGroup) -- `set` is then unused
	// cut: the first block takes its history by ScenePassState::cutAt (a pass that restarts the recurrence at scene cuts)
	void addFlowAutoencoder(std::vector<Step> *prog, int set, int items, bool group = false, bool cut = false);
	struct FlowBuild;
	void addFlowBlockStep(FlowBuild &f, const std::string &convA, const std::string &convB, const std::string &outName,
	    bool pool, bool outHead, int act2);
	void addPackingFlowBlockStep(FlowBuild &f, FlowBlockLaunch fb, double flops);
	void addDecoderUpsample(FlowBuild &f, int block);
	bool flowPacksInBlock() const;
	Operand operand(const std::string &name);
	Tensor &addTowerTensor(const std::string &name, int H, int W, int C);
	void buildWeights(const ModelFile &model);
	// Writes m_Program[set]: the stages below in this order, over one ProgramBuild.  Sets m_StateBind[set], m_FlowCur and
	// m_TrunkOut.
	void buildProgram(int set);
	struct ProgramBuild;
	void addInputSteps(ProgramBuild &b);     // lr_pack (flow-free), frame sums, pack
	void addFlowNetSteps(ProgramBuild &b);   // the auto-encoder, or a flow-resnet body and the head
	Operand addResidentFlowResnet(ProgramBuild &b);
	Operand addLayeredFlowResnet(ProgramBuild &b);
	void addWarpStep(ProgramBuild &b);
	void addGeneratorHeadSteps(ProgramBuild &b);  // calibration clear, generator/conv_1 where it is a launch
	void addTowerSteps(ProgramBuild &b);     // one of the four below
	void addResidentTower8Step(ProgramBuild &b);
	void addResidentTowerStep(ProgramBuild &b);
	void addLayeredTower8Steps(ProgramBuild &b);
	void addLayeredTowerSteps(ProgramBuild &b);
	void addTailSteps(ProgramBuild &b);      // nothing (in the tower), fused, or split
	void addTemporalStep(ProgramBuild &b);
	void addResBlockStep(std::vector<Step> *prog, const std::string &tag, const std::string &block, Operand in, Operand out,
	    int H, int W, int activation, float slope);
	void addCalibStep(std::vector<Step> *prog, int layer, const std::string &tensor);
	struct ResidentTower;
	ResidentTowerParams residentTowerParams(const ResidentTower &t, int H, int W, int nLayers, int activation, float slope);
	TailFusedLaunch fusedTail(Operand x, float slope, const unsigned *sums);
	void stageIn(const Frame &in);
	// the dense BGRX frame `src` of width x height -> the caller's image; raw: width x height x 4 bytes of scratch (the
	// flip of a bottom-up host image)
	void stageOut(const Frame &out, std::size_t width, std::size_t height, const std::uint8_t *src, std::uint8_t *raw);
	// YUV frames: decode into m_InStage / encode from m_OutStage; host planes go through m_YuvInStage / m_YuvOutStage.
	// A 10-bit output is encoded from the f16 state the step left (m_HbdFromState: the state IS the frame in float --
	// every model but normalize_brightness, whose state is output_raw - b, and output_flow, whose frame is pre_warp) or,
	// for those two, from the u8 frame like an 8-bit output.  Decided once, at creation; ju_get_stat "hbd_from_state".
	bool m_HbdFromState = true;
	// Source stage: the scaler from the size input frames must have (its source size; not set = the model's input) to
	// the model's input, its filter the one in effect ("source_filter"); the BGRX source frame at source size (host
	// uploads, decoded YUV) and the host planes of a YUV source; the mask's device copy (frame_io.h SourceMask).
	// m_SourceFrames: frames that went through the stage ("source_stage_frames").
	Scaler m_SrcScale;
	DeviceBuffer m_SrcStage, m_SrcYuvStage;
	SourceMask m_Mask;
	std::uint64_t m_SourceFrames = 0;
	// (width x height: the size of the frame encoded; of bgrx / state / frame16 the one the format's path reads)
	void encodeYuv(PixelFormat format, int colorspace, const YuvPlanes &planes, std::size_t width, std::size_t height,
	    const std::uint8_t *bgrx, std::ptrdiff_t bgrxStride, const void *state, const std::uint16_t *frame16 = nullptr,
	    hipStream_t stream = nullptr);  // (stream: nullptr = m_Stream; a group pass encodes on its lead's)
	// a deep format of a runtime whose state is the frame in float, without a mask: encoded from 16-bit samples
	bool deepFromState(PixelFormat format) const;
	// Output stage: the scaler from the model's output to the size output frames must have (its destination size; not
	// set = the model's output; "output_filter"), the scaled 8-bit and 16-bit frames, the planes of a host YUV output and
	// the flip scratch of a bottom-up host image
	Scaler m_OutScale;
	DeviceBuffer m_OutScaled8, m_OutScaled16, m_OutYuvStage, m_OutRawStage;
	void stageOutScaled(const AnyFrame &out);
	// Alpha: the mode and the filter set; the scaler from the input frame's size (the source size, else the model's
	// input) to the output frame's size (the output size, else the model's output) while the mode is JU_ALPHA_SOURCE,
	// rebuilt by setAlpha, setSourceSize and setOutputSize; where the frame in flight holds its alpha on the device
	// (submitFrame); frames whose slot the alpha kernels wrote ("alpha_frames").
	int m_AlphaMode = 0, m_AlphaFilter = 0;
	Scaler m_AlphaScale;
	AlphaRows m_AlphaSrc;
	std::uint64_t m_AlphaFrames = 0;
	// the alpha scaler the three setters would need for these frame sizes: an empty one unless `mode` is JU_ALPHA_SOURCE;
	// std::invalid_argument "<who>: <alphaProblem>" when the sizes are beyond it -- before the setter changes anything
	Scaler alphaScalerFor(const char *who, int mode, int filter, std::size_t inW, std::size_t inH, std::size_t outW, std::size_t outH) const;
	void frameSizes(std::size_t *inW, std::size_t *inH, std::size_t *outW, std::size_t *outH) const;
	// where the input frame's alpha lies once submitFrame has staged the frame; bgrx: the BGRX rows it staged
	AlphaRows alphaSource(const AnyFrame &in, const BgrxRows &bgrx);
	// the one alpha launch of a frame, behind its colour and in front of any copy to the host: nothing in mode 0 or for a
	// format without a slot
	void alphaInto(PixelFormat format, void *rows, std::ptrdiff_t stride);
	// THE alpha launch of both routes, with this runtime's mode, filter and tables at its frame sizes: the fill, or the
	// scale from `src`, into `sink` on `stream`.  False, and nothing launched, in mode 0 or for a sink without a slot
	// (alpha_route.h alphaLaunches).  Counts nothing: alphaInto counts its frame, a pass counts once it has completed.
	bool launchAlpha(const AlphaRows &src, const AlphaRows &sink, hipStream_t stream);
	// Alpha inside passes: the two settings; frames whose slot was written inside a look-ahead pass
	// ("lookahead_alpha_frames") and, as a member, inside a group pass ("group_alpha_frames") -- "alpha_frames" counts
	// them too.  alphaPass(group): the mode a pass formed now carries for this runtime, 0 when it carries none -- part of
	// the key of a look-ahead pass's graph, which bakes in the mode, the filter and the tables' addresses.
	bool m_AlphaLookahead = false, m_AlphaGroup = false;
	std::uint64_t m_BatchAlphaFrames = 0, m_GroupAlphaFrames = 0;
	int alphaPass(bool group) const { return (group ? m_AlphaGroup : m_AlphaLookahead) ? m_AlphaMode : 0; }
	// The graphs of the look-ahead passes that carry alpha: dropped whenever setAlpha, setAlphaLookahead or a size setter
	// changes what they baked in (the stream has drained: passes are synchronous)
	void dropAlphaPasses();
	// Scene detector: two eager launches on m_Stream in front of runProgram(), outside the chain lock and never captured
	// (sceneStep: submit and submitFrame, once m_IO.in holds the frame the program will read).  m_Scene: the setting, the
	// detector's memory on the model-size input and its clock (scene_detector.h).  m_SceneRerun: set around the re-run of a
	// frame (runSynchronous) -- THE one place that keeps a step from running the detector twice; m_SceneRuns counts the runs
	// ("scene_detector_runs").
	SceneDetector m_Scene;
	std::uint64_t m_SceneRuns = 0;
	bool m_SceneRerun = false;
	void sceneStep();
	// The detector inside look-ahead passes.  m_ScenePassDev: the ScenePassState (accumulators, ticket, resetAt[], cutAt[]),
	// allocated once and kept -- the cut-aware flow programs are bound to it; m_ScenePassDyn: the host-mapped ScenePassDyn
	// the host refreshes in front of every pass; m_ScenePassFrames: "scene_pass_frames".
	bool m_SceneLookahead = false;
	DeviceBuffer m_ScenePassDev;
	PinnedWords m_ScenePassDyn;
	std::uint64_t m_ScenePassFrames = 0;
	// what a pass formed now carries: 0 nothing, 1 the detector, 2 the detector and the restart at its cuts (reset mode
	// on a recurrent model: clear nodes and the cut-aware flow program) -- part of the key of a pass's graph
	int scenePass() const {
		if (!m_SceneLookahead || m_Scene.mode() == 0) return 0;
		return m_Scene.mode() == 2 && m_Config.recurrent() ? 2 : 1;
	}
	// binding set of the cut-aware flow launches in m_BatchFlow: {items, kCutSet + set}
	static constexpr int kCutSet = 4;
	// The detector inside group passes.  m_SceneGroup: the setting; m_SceneGroupDyn: this member's host-mapped SceneGroupDyn,
	// refreshed in front of every pass that carries it; m_SceneGroupFrames: "scene_group_frames".
	bool m_SceneGroup = false;
	PinnedWords m_SceneGroupDyn;
	std::uint64_t m_SceneGroupFrames = 0;
	void dropScenePassGraphs();  // the graphs of passes that carry the detector: bound to m_Scene's memory
	// Everything a frame call can refuse, before anything is launched; `who` names the entry point in the message.
	// declaredSize (ju_process_group): a NULL pointer is refused first and by name, and a graphics resource's DECLARED
	// size counts too -- otherwise the texture's own extent is checked when it is mapped, behind other members' launches.
	void checkFrame(const AnyFrame &f, bool input, const char *who = "processFrame", bool declaredSize = false) const;
	// THE pair decision (process, enqueue, the frames of runPasses): false = a BGRX pair while no source or output stage
	// is set -- submit(), unchecked; true = checkPair, then submitFrame()
	bool staged(const AnyFrame &in, const AnyFrame &out) const { return in.yuv || out.yuv || sourceStage() || m_AlphaMode != 0; }
	void checkPair(const AnyFrame &in, const AnyFrame &out) const;
	// JU_ALPHA_SOURCE: a device output over the device input is refused (checkPair, processFrames)
	void checkAlphaOverlap(const AnyFrame &in, const AnyFrame &out) const;
	// one frame's launches by that decision, enqueue only
	void submitAny(const AnyFrame &in, const AnyFrame &out);
	// (stage: where a host frame's planes are written before they are copied out)
	void stageOutYuv(const YuvFrame &out, const std::uint8_t *bgrx, const void *state, const std::uint16_t *frame16,
	    std::uint8_t *stage);
	void submitFrame(const AnyFrame &in, const AnyFrame &out);
	void bindStaging();
	// submitAny, wait, and on a resident-tower failure run the frame again on the per-layer path
	void runSynchronous(const AnyFrame &in, const AnyFrame &out);
	DeviceBuffer m_YuvInStage, m_YuvOutStage;
	void runProgram();
	void runSteps(int idx);  // binding set idx's launches against m_IO
	// Frame buffers the kernels read / write in THIS call.  Graph replay always uses
	// the internal staging buffers (static pointers); eager launches of device-resident
	// frames use the caller's buffers directly (no staging copies).
	struct FrameIO {
		const std::uint8_t *in = nullptr;
		std::ptrdiff_t inStride = 0;
		std::uint8_t *out = nullptr;
		std::ptrdiff_t outStride = 0;
	};
	FrameIO m_IO;
	// what the per-frame program of a binding set reads as the previous HR state / writes as the new one, and the
	// flow field its warp reads: read at launch (capture) time, like m_IO -- a look-ahead pass rebinds them per frame
	struct StateBind {
		const void *in = nullptr;
		void *out = nullptr;
	};
	StateBind m_StateBind[2];
	const void *m_FlowCur = nullptr;
	bool m_DirectIO = false;  // decided per call
	bool m_PreferDirect = true;  // JU_DIRECT=0: always stage (and replay the graph)
	void submit(const Frame &in, const Frame &out);

	int m_Device;
	ModelConfig m_Config;
	DType m_DType;
	Stream m_Stream;
	bool m_UseGraph = true;
	// process() polls the stream this long before it blocks (JU_SYNC_SPIN_US, 0 = block at once)
	unsigned m_SpinUs = 2000;
	int m_Idx = 0;
	std::string m_TrunkOut = "trunk_a";

	std::map<std::string, Tensor> m_Tensors;
	std::map<std::string, ConvWeights> m_Convs;
	// 8-bit tower (JU_DTYPE_FP8, fp8.h): e4m3 weights of the block convolutions, the two
	// e4m3 activation tensors (block input, first conv's output) and the per-tensor
	// exponents, index 2i = input of block i's conv_1, 2i+1 = input of its conv_2
	struct Fp8Conv {
		DeviceBuffer w, scaleA;
	};
	bool m_Fp8Tower = false;
	std::map<std::string, Fp8Conv> m_Fp8Convs;
	std::map<std::string, FoldedConv> m_Fp8Folded;  // (construction only)
	DeviceBuffer m_Fp8X, m_Fp8T;
	std::vector<int> m_Fp8Exp;
	// resident 8-bit tower (tower8_resident_kernel): every block's operands in one buffer each
	DeviceBuffer m_Fp8TowerW, m_Fp8TowerScaleA, m_Fp8TowerBias, m_Fp8TowerScaleB, m_Fp8TowerMul;
	DeviceBuffer m_TailW2, m_TailB2, m_TailW2Frag;
	DeviceBuffer m_Zeros;  // a zero page: the source of out-of-image pixels for LDS-DMA tile staging
	DeviceBuffer m_TemporalAcc;  // 32.32 fixed-point sum of |gen - pre_warp| (temporal filter)
	// flow auto-encoder: which blocks run as ONE launch (flow_block_kernel: both convs, the
	// pool, and the preceding bilinear x2).  Unit k < 2*nb = block k+1, the last = the head
	// pair flow/conv_1 + flow/conv_2.  JU_FLOW_CONV=generic: none.
	struct FlowUnit {
		bool fused = false;
		bool upsIn = false;  // its input is the half-resolution tensor (upsample folded into staging)
	};
	std::vector<FlowUnit> m_FlowUnits;
	bool m_FlowFused = true;
	// developer launch plan (kernels.h): the plan switches as read by the constructor, carried by every launch
	// descriptor of this runtime; all defaults, and no log, in the product library
	DevPlan m_Plan;
	PlanLog m_PlanLog;
	// residual blocks outside the resident tower (more regions than CUs, LeakyReLU models,
	// after a fallback): one launch per BLOCK (flow_block_kernel, intermediate tensor in LDS);
	// JU_TOWER=convs keeps one launch per convolution
	bool m_BlockFused = true;
	// JU_CALIBRATE=1 (tools/calibrate.py): per-convolution launches + max |output| of every
	// tower layer per frame into "tower_profile" (as float bit patterns)
	bool m_Calibrate = false;
	void planFlowUnits();
	bool flowConvIsFused(const std::string &name) const;
	bool m_FusedUpsample = true;  // flow decoder: bilinear x2 folded into the next conv's staging
	bool m_FusedPool = true;  // max-pool folded into the flow encoder's conv epilogues
	bool m_PackInBlock = true;  // the flow net's first block builds the packed input itself (JU_PACK=split: own launch)
	bool m_FusedTail = true;  // JU_TAIL=split: convT1 as a conv launch + the VALU tail kernel
	bool m_TailInTower = false;  // JU_TAIL=tower: the fused tail runs inside the resident tower launch
	DeviceBuffer m_InStage, m_OutStage, m_RawStage;
	// output_flow variant only: the u8 frame of the generator's writers, which nobody reads (buildProgram)
	DeviceBuffer m_DiscardFrame;
	DeviceBuffer m_State[2], m_Packed[2];
	// A resident tower (one launch for all convolutions of a 64-filter stack): the geometry of its regions, its layers'
	// weights in execution order -- collected on the host while the weights are built (addConv), uploaded by
	// setUpResidentTower -- the mailbox of its halo exchange and the publish counts per region.
	struct ResidentTower {
		int GX = 0, GY = 0, RH = 0;
		std::vector<std::uint16_t> hostW;
		std::vector<float> hostB;
		DeviceBuffer w, b, mail, flags;
	};
	// The constructor's phases, in its order (buildWeights and both buildProgram calls between them: engine.cpp).
	void readSwitches();
	bool setUpResidentTower(ResidentTower *t, bool wanted, int H, int W, int cus, bool leaky);
	void setUpResidentTowers();
	void allocateBuffers(const ModelFile &model);
	void packResidentTower8();
	void warmUpAndCapture();
	void captureFrameGraphs();  // both binding sets' programs against m_IO (nothing executes)
	void zeroResidentMailboxes();
	void dropGraphsAndRebuild();
	struct StepSpec;
	bool m_Resident = false;
	ResidentTower m_GenTower;  // the generator's: conv_1 and the residual blocks
	// flow-resnet (models.py:257-331) through the same resident kernel: conv_1 + its
	// residual blocks are a 64-filter tower too
	bool m_ResidentFlow = false;
	ResidentTower m_FlowTower;
	// The resident tower needs every workgroup co-resident.  When a bounded wait expires the
	// engine drops to the per-block kernels (fallbackToLayers) -- not for good: after
	// m_RetryAfter clean frames it tries the resident kernel again (the CUs may have been
	// taken only temporarily, e.g. by another process), backing off x4 after every failure.
	// JU_RESIDENT_RETRY=<frames> sets the first interval (default 512, 0 = never retry).
	bool m_ResidentCapable = false, m_ResidentFlowCapable = false;
	unsigned m_RetryBase = 512, m_RetryAfter = 0, m_CleanFrames = 0, m_Fallbacks = 0;
	void restoreResident();
	void maybeRestoreResident();
	// Two resident towers cannot share the GPU (each wants a workgroup on every CU and both
	// would wait for workgroups that cannot be scheduled).  Runtimes of one process on one
	// device therefore chain their frames through events when more than one of them uses the
	// resident kernel; a single runtime pays nothing.
	Event m_FrameDone;
	// (resident: whether the launches in between hold a resident tower -- m_Resident, or for a group pass, which the
	// lead chains once for all its members, any member's)
	std::unique_lock<std::mutex> chainBegin(bool resident);
	void chainEnd(std::unique_lock<std::mutex> &lock, bool resident);
	PinnedWords m_ResError;              // pinned, device-visible: word 0 = the tower's error report
	unsigned *m_ResErrorDev = nullptr;
	unsigned takeResidentError();        // 0 = none; clears it
	void fallbackToLayers(unsigned code);
	std::vector<Step> m_Program[2];
	GraphExec m_Graph[2];
	// Device-resident frames (JU_LOC_DEVICE, no staging): the kernels take the caller's
	// pointers, so a captured graph is valid for ONE (input, output, strides, binding set)
	// tuple.  Callers reuse a handful of frame buffers (OBS: one texture pair; bench.py:
	// 16 inputs, 1 output), so the graphs are cached by that tuple: prepareFrames() captures
	// a registered pair's two graphs at once (the reference captures in its constructor,
	// tensorrt_backend.cc:257-263); for an unregistered tuple the second call captures it and
	// every later one replays it.  Tuples seen once run eagerly, so a caller that hands over a
	// fresh pointer every frame never pays a capture.
	struct DirectKey {
		const void *in;
		std::ptrdiff_t inStride;
		void *out;
		std::ptrdiff_t outStride;
		int idx;
		bool operator<(const DirectKey &o) const {
			return std::tie(in, inStride, out, outStride, idx) <
			       std::tie(o.in, o.inStride, o.out, o.outStride, o.idx);
		}
	};
	// what prepareFrames registers: the pair, idx = 0 in the key -- one unit for the graphs of both binding sets
	struct PairOf {
		DirectKey operator()(DirectKey key) const {
			key.idx = 0;
			return key;
		}
	};
	// The two graph caches (graph_cache.h), over one use clock.  m_DirectGraphs: the per-frame graphs by DirectKey -- at
	// most 64 of pairs nobody registered (least recently used out) and 256 registered pairs, which stay registered when
	// the graphs are dropped (fallback to / return from the per-block path: captured again at their FIRST sighting).
	// m_BatchGraphs (the key: PassKey, below): the graphs of look-ahead passes -- 64 of tuples nobody registered, 256
	// handed to prepareBatch (a call registers one per binding set), whose registration goes with the graph.
	using CachedGraph = GraphEntry<GraphExec>;
	std::uint64_t m_DirectClock = 0;
	GraphCache<DirectKey, GraphExec, PairOf> m_DirectGraphs{m_DirectClock, 64, 256};
	bool directEligible(const Frame &in, const Frame &out) const;
	// THE submission of a cached graph's launches (runProgram's device frames, submitBatch): a graph that is there is
	// replayed; one that is not is captured at the tuple's second sighting -- a registered unit's at its first -- and
	// replayed; else the launches run eagerly.  Counts "graph_captures", "graph_replays" and "eager_runs".
	void replayOrRun(CachedGraph &e, bool registered, const std::function<void()> &launches);
	// prepareFrames / prepareBatch: the graph captured now unless it is there (nothing executes); returns the graphs
	// captured, counted as "prepared_captures"
	int prepareGraph(CachedGraph &e, const std::function<void()> &launches);
	void dropAllGraphs();  // of both caches: they replay the programs of the towers in use
	// frame look-ahead (processBatch; engine_passes.cpp): the flow net's tensors for m_BatchCap frames, the state buffers
	// between the frames of a pass, the flow launches per (frames, binding set) and the graphs per tuple of frame buffers;
	// the frames of the pass being recorded: m_Pass, below
	// The key of a pass's graph: per frame, everything a launch of the pass bakes in.  `io`: what the frame's kernels read
	// and write (bindFrame).  A YUV side adds its format and colour space and, for device planes, their pointers and
	// strides; for host planes (staged in the pass's own buffers) only the sign of each stride -- all-host passes of one
	// shape share one graph whatever the caller's addresses.  BGRX sides leave their YuvKey zero.
	struct YuvKey {
		int format = 0, colorspace = 0;
		const void *planes[3] = {};
		std::ptrdiff_t strides[3] = {};
		auto tie() const { return std::tie(format, colorspace, planes[0], planes[1], planes[2], strides[0], strides[1], strides[2]); }
	};
	struct PassKey {
		DirectKey io;
		YuvKey in, out;
		int scene = 0;  // scenePass() when the pass was bound: no graph serves another detector configuration
		// stageBits(false) when the pass was bound: a staged pass and a plain pass over the same buffers never share a graph.
		// `ends`: what a staged frame's scale, blend and encode launches read and write at the frame's own size -- the
		// caller's device image or the pass's slot (`io` is then the model-size pair in between)
		int stage = 0;
		DirectKey ends{};
		// alphaPass(false) when the pass was bound: a pass that carries the alpha launch and one over the same buffers in
		// mode 0 never share a graph; what else that launch bakes in (the filter, the tables) changes only through setters
		// that drop these graphs (dropAlphaPasses)
		int alpha = 0;
		bool operator<(const PassKey &o) const {
			if (alpha != o.alpha) return alpha < o.alpha;
			if (scene != o.scene) return scene < o.scene;
			if (stage != o.stage) return stage < o.stage;
			if (ends < o.ends) return true;
			if (o.ends < ends) return false;
			if (io < o.io) return true;
			if (o.io < io) return false;
			return std::make_tuple(in.tie(), out.tie()) < std::make_tuple(o.in.tie(), o.out.tie());
		}
	};
	std::map<std::string, Tensor> m_BatchTensors;
	DeviceBuffer m_BatchState[kFlowBatchMax - 1];
	int m_BatchCap = 0, m_BatchMax = kFlowBatchMax;
	bool m_BatchUnsupported = false;
	std::map<std::pair<int, int>, std::vector<Step>> m_BatchFlow;
	GraphCache<std::vector<PassKey>, GraphExec, UnitIsKey> m_BatchGraphs{m_DirectClock, 64, 256};
	// Host frames inside look-ahead passes (round 6; the AviSynth caller's frames, avisynth_plugin/src/main.cc:113-144, and
	// the only path the reference's own timer measures, scripts/inference/tensorrt/inference.py:245-251).  Frame by frame
	// the 8.3 MB of an output cross the PCIe link while the GPU idles -- the frame's rows all appear in its last
	// microseconds and the next frame needs this one's state.  Inside a pass that is no longer so: every input of the
	// pass is uploaded up front into the pass's own device buffers (m_PassSlots[i].in), frame i's kernels write
	// m_PassSlots[i].out, a one-thread kernel behind frame i's last launch counts it done in host-mapped memory (m_PassSignal), and the thread
	// blocked in processBatch copies frame i out on a second stream (SDMA, no CU) while frame i + 1 runs: only the last
	// frame's copy is exposed.  The copies go from / to the caller's pageable rows through the HIP runtime as in
	// stageIn / stageOut (cuda_convert.cc.cu:360-459); nothing of the caller's is page-locked (section 7 of DESIGN.md).
	// YUV sides: the frame's kernels read / write BGRX in those two slots whatever the side's location; `planes` are what
	// the side's conversion launch of the pass reads (in: decode) / writes (out: encode) -- the caller's device planes, or
	// for host planes m_PassSlots[i].yuvIn / .yuvOut (rows padded to stagePitch, in the caller's memory order).
	struct PassSide {
		bool host = false, yuv = false;
		PixelFormat format = PixelFormat::Bgrx;
		int colorspace = 0;
		YuvPlanes planes;
	};
	struct PassExtent {
		std::size_t inW = 0, inH = 0, outW = 0, outH = 0;
	};
	struct PassCopy {
		DeviceBuffer *image = nullptr, *planes = nullptr;
	};
	// Frame i (a group pass: member i) of the pass bound last, as bindFrame left it -- everything the pass's launches and
	// host copies know about it.  io: what the network reads and writes, addressed with the sign of a host caller's stride.
	// ends: the frame's rows at its own size (PassKey::ends) -- the same rows as io on a side without a scaler, else what
	// the scaler reads / writes there while io is the model-size staged slot in between.  size: the frame's size on either
	// side (passSizes under the owner's stage bits).  up / down: the device buffers the host copies of the frame go to /
	// come from.  groupPrev / groupOut: on the lead of a group pass, the history item i's first flow block reads / writes.
	// alphaIn / alphaOut: where the frame's alpha slots lie on the device, by alpha_route.h's rule over what was bound above
	// -- a BGRX side's `ends` rows, plane 0 of another format's planes; kAlphaNone for a format without a slot.
	// m_PassStage heads the array: the stage bits the look-ahead pass was bound with (a group pass: 0 -- each member
	// brings its own).  A fixed-address member: the step lambdas and the captured graphs hold pointers into it and read it
	// at launch time.
	struct PassFrame {
		PassSide in, out;
		FrameIO io, ends;
		PassExtent size;
		PassCopy up, down;
		AlphaRows alphaIn, alphaOut;
		const void *groupPrev = nullptr;
		void *groupOut = nullptr;
		bool host() const { return in.host || out.host; }
		bool yuv() const { return in.yuv || out.yuv; }
	};
	int m_PassStage = 0;
	PassFrame m_Pass[kFlowBatchMax];
	// binds one side of a pass's frame (bindFrame): fills `side` and the side's part of the graph key, returns what the
	// frame's kernels read / write there.  image / planes: the pass's own device buffers of that side and frame, made here
	// when first needed.
	struct BoundRows {
		std::uint8_t *ptr;
		std::ptrdiff_t stride;
	};
	BoundRows bindSide(const AnyFrame &a, std::size_t width, std::size_t height, DeviceBuffer *image, DeviceBuffer *planes,
	    PassSide *side, YuvKey *key);
	// the pass's own buffers of frame i at the model's sizes: the BGRX image and the host planes of either side
	struct PassSlots {
		DeviceBuffer in, out, yuvIn, yuvOut;
	};
	PassSlots m_PassSlots[kFlowBatchMax];
	// Scaled and masked frames inside passes (setStageLookahead, setStageGroup; engine_passes.cpp).  stageBits(group): what
	// a look-ahead pass formed now carries -- group: what this runtime brings into a group pass, the same bits under its
	// own setting -- 0 nothing, else bit 0 the source scaler, bit 1 the mask, bit 2 the output scaler.
	// StageSlots: the buffers of one frame under a scaler, each made when first needed at the sizes set -- src / srcYuv the
	// source-size BGRX frame and host planes, `in` the model-size input the one scale launch fills, modelOut the model-size
	// output the network writes under an output size, out8 / out16 / outYuv the 8-bit frame, the 16-bit frame and the host
	// planes at output size.  m_StageSlots: one per frame of the cap, for look-ahead passes.  m_GroupSlots: a member
	// contributes one frame per group pass, so it owns ONE, at THIS runtime's sizes.  All dropped by dropStagePasses, with
	// the staged passes' graphs, whenever one of this runtime's stage setters changes anything.  A member's slots live in
	// the member, not the lead: a setter or the destruction of one runtime touches no other runtime's memory, and the lead
	// keeps no pointer to them beyond the call (runGroupPass clears the records' up / down).
	// m_BatchStagedFrames: "lookahead_staged_frames"; m_GroupStagedFrames: "group_staged_frames".
	bool m_StageLookahead = false, m_StageGroup = false;
	int stageBits(bool group) const {
		if (!(group ? m_StageGroup : m_StageLookahead) || !sourceStage()) return 0;
		return (m_SrcScale.set() ? 1 : 0) | (m_Mask.on() ? 2 : 0) | (m_OutScale.set() ? 4 : 0);
	}
	struct StageSlots {
		DeviceBuffer src, srcYuv, in, modelOut, out8, out16, outYuv;
	};
	StageSlots m_StageSlots[kFlowBatchMax], m_GroupSlots;
	std::uint64_t m_BatchStagedFrames = 0, m_GroupStagedFrames = 0;
	void dropStagePasses();
	// Binds one frame of a pass, on the runtime whose stream runs it (the lead): fills `f` and, if asked, the sides' parts
	// of the frame's graph key.  owner: whose scalers, sizes and format rules apply -- this runtime for a look-ahead pass,
	// member i for a group pass; staged: the owner's slots for the sides under one of its scalers; plain: this runtime's
	// slots for the others.
	void bindFrame(PassFrame *f, const Engine &owner, int stage, const AnyFrame &in, const AnyFrame &out, StageSlots *staged,
	    PassSlots *plain, PassKey *key);
	// the members of a group pass, on the lead: member i's pair under member i's own stage bits, sizes and slots
	void bindGroup(Engine *const *m, const AnyFrame *in, const AnyFrame *out, int n, const int *stage);
	// What follows a frame's own steps in a pass, on this runtime's stream (the lead's): the owner's mask blend in place,
	// its output scaler, the encode, its alpha launch and the host signal.  stateOut: the state the frame's steps wrote; out16: the frame's
	// 16-bit slot at output size.
	void passTail(Engine &owner, const PassFrame &f, int stage, void *stateOut, const DeviceBuffer &out16);
	// this runtime's mask over the model-size frame `gen`, letting through the source rows `src` of srcW x srcH
	void blendMask(std::uint8_t *gen, std::ptrdiff_t genStride, const std::uint8_t *src, std::ptrdiff_t srcStride, std::size_t srcW,
	    std::size_t srcH, hipStream_t stream);
	// the size frames must have on a side of a pass bound with `stage`
	void passSizes(int stage, std::size_t *inW, std::size_t *inH, std::size_t *outW, std::size_t *outH) const;
	std::unique_ptr<Stream> m_CopyStream;
	PinnedWords m_PassSignal;
	unsigned m_PassSignalBase = 0;
	std::uint64_t m_BatchHostFrames = 0, m_BatchYuvFrames = 0;
	// group: as a member of a group pass -- under stageBits(true) and the detector's group setting
	bool passEligible(const AnyFrame &in, const AnyFrame &out, bool group = false) const;
	void uploadPassInputs(const AnyFrame *in, int n);
	void drainPassOutputs(const AnyFrame *out, int n);
	// the passes of processBatch / processFrames (whose staged pairs are checked: processFrames)
	void runPasses(const AnyFrame *in, const AnyFrame *out, int count);
	std::uint64_t m_BatchFrames = 0;
	// group: the flow launches of a group pass over `items` streams (processGroup), in m_BatchFlow at {items, kGroupSet}
	bool batchPlanned(int items, bool group = false);
	static constexpr int kGroupSet = 2;
	void submitBatch(const AnyFrame *in, const AnyFrame *out, int n);
	void runBatch(int set, int n, const std::function<void(const Step &, bool)> *around = nullptr);
	// the n frames of a look-ahead pass under stage = stageBits(false); returns the key of the pass's graph
	std::vector<PassKey> bindBatch(const AnyFrame *in, const AnyFrame *out, int n, int set, int stage);
	// Group passes (processGroup).  The model's identity: FNV-1a of the container bytes the engine was built from, and
	// the dtype it was asked for.  As a member: an event its stream records for the lead to wait on, and the frames it got
	// from passes ("group_frames").  (As the lead: the history each item's first flow block reads and writes is in m_Pass.)
	std::uint64_t m_ModelDigest = 0;
	int m_DtypeOverride = -1;
	Event m_GroupEvent;
	std::uint64_t m_GroupFrames = 0, m_GroupYuvFrames = 0;  // ("group_yuv_frames": those of them with a non-BGRX side)
	bool sameModel(const Engine &o) const;
	// one pass over members m[0 .. n) on `lead`'s stream and tensors (the lead need not be one of them)
	static void runGroupPass(Engine &lead, Engine *const *m, const AnyFrame *in, const AnyFrame *out, int n,
	    const std::function<void(bool)> &underPass, hipEvent_t after);
	static void runGroups(Engine *const *members, const AnyFrame *in, const AnyFrame *out, int count, const char *who, bool indexed,
	    const std::function<void(bool)> &underPass, hipEvent_t after);
	bool m_DirectGraph = true;  // JU_DIRECT_GRAPH=0: device frames always launch eagerly
	// Host frames (JU_LOC_CPU: the AviSynth caller, avisynth_plugin/src/main.cc:113-144) are copied from / to pageable
	// memory through the HIP runtime's own bounce buffers.  Page-locking recycled caller buffers (hipHostRegister at a
	// buffer's second sighting, JU_PIN_HOST=1) was built in round 5, measured at +2.3 % on that PCIe-bound path
	// (profiles/r05_host_path_ab.txt) and REMOVED: a registration on malloc'ed memory outlives its buffer in the HIP
	// runtime's view of those addresses -- later pageable copies from a recycled range were done as direct GPU reads of
	// an unmapped host page ("Memory access fault by GPU ... on address <host heap>", one run in two of the full GPU
	// suite; before that, hipErrorInvalidValue from torch's own hipMemcpy).  DESIGN.md section 7.
	// introspection ("graph_replays" / "eager_runs" / "graph_captures": captures of device-frame
	// graphs made inside process / enqueue, i.e. not by prepareFrames or the constructor)
	std::uint64_t m_GraphReplays = 0, m_EagerRuns = 0, m_InlineCaptures = 0, m_PreparedCaptures = 0;

public:
	std::uint64_t fallbacks() const { return m_Fallbacks; }
	// counters of how the per-frame program ran so far (tests, bench)
	std::uint64_t graphReplays() const { return m_GraphReplays; }
	std::uint64_t eagerRuns() const { return m_EagerRuns; }
};

}  // namespace ju
