// Tiled upscaling (docs/tiled.md): a source larger than the model, cut into model-size tiles that overlap, each tile an
// independent recurrent stream of its own Engine, the tiles' outputs blended into one frame on the GPU.  No reference
// counterpart: the reference upscales exactly the model's size.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "mask_box.h"
#include "tile_geometry.h"

namespace ju {

// The limits of ju_tiled_set_output_size as one message shared with its Python twin: outputSizeProblem's for the blended
// frame of 4 srcW x 4 srcH, which a limit's message then names as such; "" when width x height may be set.
std::string tiledOutputSizeProblem(std::size_t width, std::size_t height, std::size_t srcW, std::size_t srcH, int filter);

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
	// zeroes every tile's recurrent state (keeps setDeepFromState)
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
	// (frames whose output was blended from the states), "scene_mode", "scene_frames" / "scene_cuts" (the detector's
	// decisions and cuts, cumulative over its on-periods), "output_scaled" (1 while an output size is set), "output_filter"
	// (its kScale* value, 0 while off), "output_scaled_frames" (frames that took a fused blend-and-scale kernel),
	// "source_mask" (1 while a mask is set), "source_mask_frames" (frames processed while one was set), "mask_box_x0" /
	// "_y0" / "_x1" / "_y1" (the box in blended coordinates; all 0 while the mask is off or the box is empty)
	double stat(const std::string &key) const;

private:
	void check(const AnyFrame &f, bool input, const char *who) const;
	// the source as 4-byte-aligned BGRX rows on the device: the caller's image where it is, or m_SrcStage
	struct Rows {
		std::uint8_t *ptr;
		std::ptrdiff_t stride;
	};
	Rows stageIn(const AnyFrame &in);
	void stitchOut(const AnyFrame &out, const Rows &src);
	// a deep format while the setting is on and the tiles' states are their frames in float: the 16-bit path of stitchOut
	bool deepFromState(const AnyFrame &out) const;
	void stitchOutDeep(const YuvFrame &y);
	DeviceBuffer &lazy(DeviceBuffer &b, std::size_t bytes);

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
	DeviceBuffer m_SrcStage, m_OutStage, m_YuvIn, m_YuvOut;
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
	// the source mask in device memory, in the caller's row order (m_MaskStride < 0: bottom-up; m_MaskW == 0: none), its
	// box in blended coordinates and the frames processed while one was set
	DeviceBuffer m_Mask;
	std::size_t m_MaskW = 0, m_MaskH = 0;
	std::ptrdiff_t m_MaskStride = 0;
	MaskBox m_MaskBox;
	std::uint64_t m_MaskFrames = 0;
	// The scene detector, made when the mode is turned on: m_ScenePrev the kept source-size frame (4 Ws Hs bytes), m_SceneDev
	// the SceneState, m_SceneRing kSceneRing records + the totals (host-mapped), m_SceneClear the clear's table of kTileMax
	// SceneClearTile (host-mapped; RESET on a recurrent model only).  m_Own: what each tile counts (tileOwnedEnds).
	// m_SceneSeen: steps since the last start (the "has predecessor" bits); m_SceneSteps: steps since the mode was turned on
	// (the record's `step`, the ring slot).
	void splitIn(const Rows &src);
	bool m_Recurrent = true;
	int m_SceneMode = 0;
	std::uint32_t m_SceneThreshold = 0;
	TileOwn m_Own;
	DeviceBuffer m_ScenePrev, m_SceneDev;
	PinnedWords m_SceneRing, m_SceneClear;
	std::uint64_t m_SceneSeen = 0, m_SceneSteps = 0;
	std::uint64_t m_SceneFramesBase = 0, m_SceneCutsBase = 0;  // "scene_frames" / "scene_cuts" of earlier on-periods
};

}  // namespace ju
