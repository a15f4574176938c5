// Tiled upscaling (docs/tiled.md): a source larger than the model, cut into model-size tiles that overlap, each tile an
// independent recurrent stream of its own Engine, the tiles' outputs blended into one frame on the GPU.  No reference
// counterpart: the reference upscales exactly the model's size.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "mask_box.h"
#include "tile_geometry.h"
#include "tile_pass_plan.h"

namespace ju {

// The limits of ju_tiled_set_output_size as one message shared with its Python twin: outputSizeProblem's for the blended
// frame of 4 srcW x 4 srcH, which a limit's message then names as such; "" when width x height may be set.
std::string tiledOutputSizeProblem(std::size_t width, std::size_t height, std::size_t srcW, std::size_t srcH, int filter);

// The limits of ju_tiled_set_alpha as one message shared with its Python twin, and what ju_tiled_set_output_size asks
// before it changes the size: alphaProblem's with the tiled source size as the input frame and outW x outH -- (0, 0), no
// output size: the blended frame, four times the source -- as the output frame; "" when the setting may be made.
std::string tiledAlphaProblem(int mode, int filter, std::size_t srcW, std::size_t srcH, std::size_t outW, std::size_t outH);

class TiledRuntime {
public:
	// srcWidth x srcHeight: the size of every input frame; overlap: source pixels neighbouring tiles share at least.
	// std::invalid_argument for sizes or an overlap outside the limits (tileLayoutProblem), before any engine is built.
	TiledRuntime(int device, const void *blob, std::size_t size, int dtypeOverride, std::size_t srcWidth, std::size_t srcHeight,
	    int overlap);
	TiledRuntime(const TiledRuntime &) = delete;
	TiledRuntime &operator=(const TiledRuntime &) = delete;

	// One frame, synchronously: `in` of the source size, `out` of four times that (or the output size set), any format, host or device.  Both are
	// checked before anything is launched (std::invalid_argument "<who>: <why>"; every tile's state as it was).
	void process(const AnyFrame &in, const AnyFrame &out, const char *who);
	// `count` CONSECUTIVE frames of the tiled stream in one synchronous call (docs/tiled.md "Look-ahead passes"): in every
	// output plane, every tile's state and history, the detector's memory and records and every counter exactly what
	// process(in[i], out[i], ..) called in order would have left, under every setting -- but every input must hold its
	// pixels when the call is made.  Every pair is checked before anything is uploaded or launched (std::invalid_argument
	// "<who>: frame i: <why>"; the object as it was).  Runs as passes of at most lookahead() frames (tile_pass_plan.h): a
	// pass stages and splits all its sources up front, in ONE launch while the scene detector is off, then per frame the
	// group passes and the stitch, a host frame's copy-out deferred under the next frame's group passes.
	void processFrames(const AnyFrame *in, const AnyFrame *out, int count, const char *who);
	// Frames per look-ahead pass, 1 (every frame as process()) .. kTilePassMax, clamped.  Default: the members' look-ahead
	// (8, or JU_LOOKAHEAD at creation).  reset() keeps it.
	void setLookahead(int frames) { m_Lookahead = clampTilePassCap(frames); }
	int lookahead() const { return m_Lookahead; }
	// zeroes every tile's recurrent state (keeps setDeepFromState and setLookahead)
	void reset();
	// Deep outputs (docs/tiled.md "Deep outputs"): 1 = a deep format (P010, BGRX64, RGBPH, ...) is encoded from the blend of
	// the tiles' f16 states where the model's state is the frame in float ("hbd_from_state" 1; else the setting has no
	// effect); 0 (default) = from the blended 8-bit frame.  std::invalid_argument for another value.
	void setDeepFromState(int on);
	// The scene detector of the tiled stream (docs/tiled.md "Scene cuts"): ONE detector on the source-size frame, its
	// decision taken on the GPU inside the split's launch; mode 2 zeroes the recurrent inputs of ALL tiles at a cut, in one
	// launch in front of the group passes.  The member engines' own detectors stay off.  std::invalid_argument with
	// sceneDetectProblem's words; the same mode again changes only the threshold; a mode change is a detector start, and
	// turning the mode off frees the detector's memory.  reset() keeps mode and threshold and is a detector start.
	void setSceneDetect(int mode, std::uint32_t thresholdMilli);
	void sceneDetect(int *mode, std::uint32_t *thresholdMilli) const;
	// the last min(count, kSceneRing, steps seen) decisions, oldest first; returns how many
	int sceneInfo(SceneRecord *out, int count);
	// An output size (docs/tiled.md "An output size"): output frames are width x height from now on, the blended frame of
	// 4 srcWidth x 4 srcHeight scaled by `filter` (kScale*) INSIDE the blend's launch -- the blended frame is never stored.
	// (0, 0) turns it off.  The limits are outputSizeProblem's with the blended frame in the model output's place
	// (std::invalid_argument; the setting stays as it was).  Waits for the tiled stream, builds and uploads the two axes'
	// tables and drops the staging frames, whose sizes follow the output size.  reset() keeps it; tile states, frame
	// history, group passes and the scene detector do not know about it.
	void setOutputSize(std::size_t width, std::size_t height, int filter);
	void outputSize(std::size_t *width, std::size_t *height) const;  // (0, 0) while off
	// A source mask (docs/tiled.md "A mask"): from now on the source frame of each call is drawn back over the blended frame
	// through `mask` -- Engine::setSourceMask's definition at the blended size, applied to the blended sample in registers
	// inside the stitch's launch, in front of the output scaler.  A BGRX image of any size 1 .. 16384 per axis, host or
	// device, any stride of either sign, copied now; its box (mask_box.h) is computed now (a device mask is read back once
	// for it).  nullptr: no mask.  std::invalid_argument, the setting as it was: a graphics resource, a size out of range,
	// 2 x blended extent x mask extent not below 2^32.  reset(), setOutputSize and setSceneDetect keep it; tile inputs and
	// states, the group passes and the scene detector do not know about it; deep formats are encoded from the 8-bit frame
	// while it is set.
	void setSourceMask(const Frame *mask);
	// The alpha channel (docs/tiled.md "Alpha"; docs/alpha.md "Tiled"): Engine::setAlpha's modes, filter check and
	// definition with the tiled source size as the input frame and the output frame of this object -- four times the source,
	// or the output size set -- as the output frame.  The alpha plane is scaled straight from one to the other by ONE launch
	// per frame behind the stitch and the encode, in front of the copy out: never cut into tiles, never blended, never seen
	// by the tiles' engines, which stay in mode 0.  std::invalid_argument with alphaProblem's words for those two sizes, the
	// setting as it was; setOutputSize is refused likewise where it would leave JU_ALPHA_SOURCE outside the limits.  Waits
	// for the tiled stream; reset() keeps it.
	void setAlpha(int mode, int filter);
	void alpha(int *mode, int *filter) const;

	std::size_t srcWidth() const { return m_SrcW; }
	std::size_t srcHeight() const { return m_SrcH; }
	std::size_t tileWidth() const { return m_TileW; }
	std::size_t tileHeight() const { return m_TileH; }
	int tilesX() const { return m_X.tiles(); }
	int tilesY() const { return m_Y.tiles(); }
	int tiles() const { return tilesX() * tilesY(); }
	int overlap() const { return m_Overlap; }
	// the origin of tile `index` (row-major over the tile grid) in source pixels
	void tile(int index, std::size_t *x, std::size_t *y) const;
	// "tiles", "frames" (frames processed), "group_frames" (the members' frames that ran inside group passes, summed),
	// "deep_from_state" (the setting), "hbd_from_state" (the model's property, every tile's alike), "deep_state_frames"
	// (frames whose output was blended from the states), "lookahead" (the cap), "pass_calls" (passes run), "pass_frames"
	// (frames that ran inside a pass of two or more), "pass_split_launches" (multi-frame split launches),
	// "pass_overlapped_copies" (host outputs copied out under a later frame's group passes), "scene_mode", "scene_frames" / "scene_cuts" (the detector's
	// decisions and cuts, cumulative over its on-periods), "output_scaled" (1 while an output size is set), "output_filter"
	// (its kScale* value, 0 while off), "output_scaled_frames" (frames that took a fused blend-and-scale kernel),
	// "source_mask" (1 while a mask is set), "source_mask_frames" (frames processed while one was set), "mask_box_x0" /
	// "_y0" / "_x1" / "_y1" (the box in blended coordinates; all 0 while the mask is off or the box is empty), "alpha_mode" /
	// "alpha_filter" (the setting), "alpha_frames" (frames whose alpha slot the alpha launch wrote)
	double stat(const std::string &key) const;

private:
	void check(const AnyFrame &f, bool input, const char *who) const;
	// the source as 4-byte-aligned BGRX rows on the device (frame_io.h stageInBgrx): the caller's image where it is, or
	// `stage`; stage, yuv: where a source that is not read in place goes -- m_SrcStage / m_YuvIn, or a pass's slot of each,
	// made here when first needed
	BgrxRows stageIn(const AnyFrame &in, DeviceBuffer &stage, DeviceBuffer &yuv);
	// A host frame's copy-out, deferred (a pass): what stitchOut left in staging slot `slot` and where it goes
	struct HostCopy {
		bool pending = false, yuv = false;
		YuvFrame planes;                   // yuv: the caller's planes, and their staging layout at `stage`
		RowSpan rows{nullptr, 0, true};  // BGRX: the caller's rows in memory order, `height` of `rowBytes` from `stage`
		std::uint8_t *stage = nullptr;
		std::size_t rowBytes = 0, height = 0;
	};
	// part `part` of `parts` of a deferred copy, on `stream`: a BGRX frame's rows divided evenly, planes whole with part 0
	void copyOut(const HostCopy &c, int part, int parts, hipStream_t stream);
	void deferOrCopyPlanes(const YuvFrame &y, std::uint8_t *yuv, HostCopy *defer);
	// slot: which of the two staging frames per side (0 outside a pass); defer: null = a host frame is copied out on the
	// tiled stream behind its stitch (process()), else the copy is left to the caller in *defer
	// alphaSrc: where the frame's alpha lies on the device (alphaSource)
	void stitchOut(const AnyFrame &out, const BgrxRows &src, const AlphaRows &alphaSrc, int slot = 0, HostCopy *defer = nullptr);
	// a deep format while the setting is on and the tiles' states are their frames in float: the 16-bit path of stitchOut
	bool deepFromState(const AnyFrame &out) const;
	void stitchOutDeep(const YuvFrame &y, const AlphaRows &alphaSrc, int slot, HostCopy *defer);
	DeviceBuffer &lazy(DeviceBuffer &b, std::size_t bytes);
	void checkPair(const AnyFrame &in, const AnyFrame &out, const char *who) const;
	// every tile's engine by one frame, as group passes over the tile inputs `in`; under(p, passes, inPass): host work under
	// pass p (inPass false: no group pass was formed and the members have finished); after: the event the passes run behind
	void groupPasses(const TileSet &in, const std::function<void(int, int, bool)> &under, hipEvent_t after = nullptr);
	void runPass(const AnyFrame *in, const AnyFrame *out, int count);

	int m_Device;
	int m_Overlap;
	std::size_t m_SrcW, m_SrcH, m_TileW = 0, m_TileH = 0;
	TileAxis m_X, m_Y;
	std::vector<std::unique_ptr<Engine>> m_Engines;
	std::unique_ptr<Stream> m_Stream;
	// every tile's dense input / output, one after the other (m_In / m_Out name them for the kernels)
	DeviceBuffer m_TileIn, m_TileOut;
	std::size_t m_TileInBytes = 0, m_TileOutBytes = 0;
	TileSet m_In, m_Out;
	DeviceBuffer m_XTable, m_YTable;
	// frames that are not device BGRX: the BGRX source and result, and the planes of host frames of another format
	// (m_OutStage[1] / m_YuvOut[1]: the second staging slot of a look-ahead pass, made at the first pass that needs it)
	DeviceBuffer m_SrcStage, m_OutStage[2], m_YuvIn, m_YuvOut[2];
	// Look-ahead passes (processFrames), made at the first pass and sized by the cap: m_PassSrc / m_PassYuvIn the K source
	// slots (4 Ws Hs bytes each; a host frame's planes), m_PassIn K x T tile inputs -- frame f of tile k at m_PassSet.ptr[k]
	// + f * m_PassSlot -- m_CopyStream the stream of the deferred copies, m_Stitched[f & 1] the event behind frame f's last
	// output launch.
	int m_Lookahead = kTilePassMax;
	std::vector<DeviceBuffer> m_PassSrc, m_PassYuvIn;
	DeviceBuffer m_PassIn;
	TileSet m_PassSet;
	std::size_t m_PassSlot = 0;
	std::unique_ptr<Stream> m_CopyStream;
	std::unique_ptr<Event> m_Stitched[2];
	std::uint64_t m_PassCalls = 0, m_PassFrames = 0, m_PassSplitLaunches = 0, m_PassOverlappedCopies = 0;
	// deep outputs from the states: the setting, the model's property, the blended 16-bit frame (8 bytes per output pixel,
	// made at first use) and the frames that took the path
	bool m_DeepFromState = false, m_HbdFromState = false;
	DeviceBuffer m_Out16;
	std::uint64_t m_DeepStateFrames = 0;
	std::uint64_t m_Frames = 0;
	// the output size: the scaler's tables from the blended frame to it (set() while one is in effect) and the frames that
	// took a fused kernel.  m_OutStage, m_Out16 and m_YuvOut are then of the output size.
	Scaler m_OutScale;
	std::uint64_t m_OutputScaledFrames = 0;
	// the source mask's device copy (frame_io.h SourceMask), its box in blended coordinates and the frames processed while
	// one was set
	SourceMask m_Mask;
	MaskBox m_MaskBox;
	std::uint64_t m_MaskFrames = 0;
	// Alpha: the setting; the scaler from the source size to the output frame's size while the mode is JU_ALPHA_SOURCE,
	// rebuilt by setAlpha and setOutputSize; the frames whose slot was written.  alphaSource: alpha_route.h's rule on what
	// stageIn left on the device -- `src`, the BGRX rows it returned (the device frame in place or the staged copy, X as the
	// caller gave it), or plane 0 of an RGBX, BGRX64 or X2 input, the caller's or the copy staged in `yuvStage`; never the
	// decoded BGRX rows of such an input, whose X is 0.  alphaInto: the one launch of a frame, into the side of `format`
	// whose rows (a BGRX frame's, else plane 0 as the encode wrote it) are given; nothing in mode 0 or without a slot.
	int m_AlphaMode = 0, m_AlphaFilter = 0;
	Scaler m_AlphaScale;
	std::uint64_t m_AlphaFrames = 0;
	void outputFrameSize(std::size_t *width, std::size_t *height) const;  // the output size set, else four times the source
	AlphaRows alphaSource(const AnyFrame &in, const BgrxRows &src, const DeviceBuffer &yuvStage) const;
	void alphaInto(PixelFormat format, void *rows, std::ptrdiff_t stride, const AlphaRows &alphaSrc);
	// The scene detector: m_Scene the setting, the memory on the source-size frame (the kept frame: 4 Ws Hs bytes) and the
	// clock (scene_detector.h); m_SceneClear the clear's table of kTileMax SceneClearTile (host-mapped; RESET on a recurrent
	// model only), re-made with the detector's memory.  m_Own: what each tile counts (tileOwnedEnds).
	void splitIn(const BgrxRows &src, const TileSet &into);
	bool m_Recurrent = true;
	SceneDetector m_Scene;
	TileOwn m_Own;
	PinnedWords m_SceneClear;
};

}  // namespace ju
