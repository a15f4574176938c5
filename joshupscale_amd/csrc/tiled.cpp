// The tiled runtime (tiled.h; docs/tiled.md).  One frame: the source becomes BGRX rows on the device (the caller's image
// where it is, an upload, or the existing decode at source size), ONE launch cuts it into the tiles' inputs, the tiles'
// engines advance by one frame each as group passes (Engine::processGroup: the flow net of a pass's tiles in one pass of
// its launches), ONE launch blends the tiles' outputs into the frame -- straight into a device BGRX image, else into a
// staging frame that is copied out or encoded by the existing encode at output size.  With setDeepFromState a deep format
// is instead encoded from ONE launch's blend of the tiles' f16 states (stitchOutDeep).  Under a source mask (setSourceMask)
// the blend's launch also draws the source rows of step one back over the blended pixels, inside the mask's box.  The call
// is synchronous.  Several consecutive frames in one call (processFrames): the same steps as look-ahead passes -- all
// sources staged and cut up front, in ONE launch, a host frame copied out under the next frame's group passes (runPass).
#include "tiled.h"

#include "alpha_route.h"

#include <algorithm>
#include <stdexcept>

namespace ju {

namespace {
std::size_t roundUp(std::size_t n, std::size_t to) { return (n + to - 1) / to * to; }

ModelConfig configOf(const void *blob, std::size_t size) {
	const ModelFile model(blob, size);
	return model.config();
}
}  // namespace

TiledRuntime::TiledRuntime(int device, const void *blob, std::size_t size, int dtypeOverride, std::size_t srcWidth,
    std::size_t srcHeight, int overlap)
    : m_Device(device), m_Overlap(overlap), m_SrcW(srcWidth), m_SrcH(srcHeight) {
	const ModelConfig config = configOf(blob, size);  // (the loader's refusals first, then the layout's: no device yet)
	m_TileW = static_cast<std::size_t>(config.frameWidth);
	m_TileH = static_cast<std::size_t>(config.frameHeight);
	m_Recurrent = config.recurrent();
	const std::string problem = tileLayoutProblem(srcWidth, srcHeight, m_TileW, m_TileH, overlap);
	if (!problem.empty()) throw std::invalid_argument("ju_tiled_create: " + problem);
	m_X = tileAxis(static_cast<long>(srcWidth), static_cast<long>(m_TileW), overlap);
	m_Y = tileAxis(static_cast<long>(srcHeight), static_cast<long>(m_TileH), overlap);
	const int n = tiles();
	for (int k = 0; k < n; ++k) m_Engines.push_back(std::make_unique<Engine>(device, blob, size, dtypeOverride));
	m_HbdFromState = m_Engines[0]->stat("hbd_from_state") != 0;  // (the model's property: every tile's alike)
	m_Lookahead = clampTilePassCap(m_Engines[0]->lookahead());    // (8, or JU_LOOKAHEAD at creation)
	m_Stream = std::make_unique<Stream>();
	// (each tile's slot a multiple of 256 bytes: the kernels' 16-byte accesses, the group passes' 4- and 8-byte ones)
	m_TileInBytes = roundUp(m_TileW * m_TileH * 4, 256);
	m_TileOutBytes = roundUp(m_TileW * m_TileH * 64, 256);
	m_TileIn = DeviceBuffer(m_TileInBytes * static_cast<std::size_t>(n));
	m_TileOut = DeviceBuffer(m_TileOutBytes * static_cast<std::size_t>(n));
	for (int k = 0; k < n; ++k) {
		m_In.ptr[k] = m_TileIn.as<std::uint8_t>() + m_TileInBytes * static_cast<std::size_t>(k);
		m_Out.ptr[k] = m_TileOut.as<std::uint8_t>() + m_TileOutBytes * static_cast<std::size_t>(k);
		m_In.x[k] = m_Out.x[k] = m_X.origin[static_cast<std::size_t>(k % tilesX())];
		m_In.y[k] = m_Out.y[k] = m_Y.origin[static_cast<std::size_t>(k / tilesX())];
	}
	// what each tile counts for the scene detector: every source pixel has one owner
	const std::vector<int> endX = tileOwnedEnds(m_X.origin, static_cast<long>(srcWidth));
	const std::vector<int> endY = tileOwnedEnds(m_Y.origin, static_cast<long>(srcHeight));
	for (int k = 0; k < n; ++k) {
		m_Own.x1[k] = endX[static_cast<std::size_t>(k % tilesX())];
		m_Own.y1[k] = endY[static_cast<std::size_t>(k / tilesX())];
	}
	// both axes' tables, uploaded once
	m_XTable = DeviceBuffer(m_X.table.size() * sizeof(TileAxisEntry));
	m_YTable = DeviceBuffer(m_Y.table.size() * sizeof(TileAxisEntry));
	m_XTable.upload(m_X.table.data(), m_X.table.size() * sizeof(TileAxisEntry));
	m_YTable.upload(m_Y.table.data(), m_Y.table.size() * sizeof(TileAxisEntry));
}

void TiledRuntime::tile(int index, std::size_t *x, std::size_t *y) const {
	if (index < 0 || index >= tiles()) {
		throw std::invalid_argument("ju_tiled_get_tile: index " + std::to_string(index) + " outside 0 .. " + std::to_string(tiles() - 1));
	}
	if (x) *x = static_cast<std::size_t>(m_In.x[index]);
	if (y) *y = static_cast<std::size_t>(m_In.y[index]);
}

double TiledRuntime::stat(const std::string &key) const {
	if (key == "tiles") return tiles();
	if (key == "frames") return static_cast<double>(m_Frames);
	if (key == "deep_from_state") return m_DeepFromState ? 1.0 : 0.0;
	if (key == "hbd_from_state") return m_HbdFromState ? 1.0 : 0.0;
	if (key == "deep_state_frames") return static_cast<double>(m_DeepStateFrames);
	if (key == "lookahead") return m_Lookahead;
	if (key == "pass_calls") return static_cast<double>(m_PassCalls);
	if (key == "pass_frames") return static_cast<double>(m_PassFrames);
	if (key == "pass_split_launches") return static_cast<double>(m_PassSplitLaunches);
	if (key == "pass_overlapped_copies") return static_cast<double>(m_PassOverlappedCopies);
	if (key == "scene_mode") return m_Scene.mode();
	// (the totals behind the ring: the calls are synchronous, so the last decision is in them)
	if (key == "scene_frames" || key == "scene_cuts") return static_cast<double>(m_Scene.total(key == "scene_cuts"));
	if (key == "output_scaled") return m_OutScale.set() ? 1.0 : 0.0;
	if (key == "output_filter") return m_OutScale.filter();
	if (key == "output_scaled_frames") return static_cast<double>(m_OutputScaledFrames);
	if (key == "source_mask") return m_Mask.on() ? 1.0 : 0.0;
	if (key == "source_mask_frames") return static_cast<double>(m_MaskFrames);
	if (key == "mask_box_x0") return m_MaskBox.x0;
	if (key == "mask_box_y0") return m_MaskBox.y0;
	if (key == "mask_box_x1") return m_MaskBox.x1;
	if (key == "mask_box_y1") return m_MaskBox.y1;
	if (key == "alpha_mode") return m_AlphaMode;
	if (key == "alpha_filter") return m_AlphaFilter;
	if (key == "alpha_frames") return static_cast<double>(m_AlphaFrames);
	if (key == "group_frames") {
		double sum = 0;
		for (const auto &e : m_Engines) sum += e->stat("group_frames");
		return sum;
	}
	throw std::invalid_argument("ju_tiled_get_stat: unknown stat " + key);
}

void TiledRuntime::reset() {
	for (const auto &e : m_Engines) e->reset();
	m_Scene.restart();  // the scene detector has no predecessor after a reset; its setting and its step count stay
}

// ---------------------------------------------------------------------------------------------------------------
// Scene detector (docs/tiled.md "Scene cuts"): the engine's detector (scene_detector.h) on the source-size frame.
// ---------------------------------------------------------------------------------------------------------------
void TiledRuntime::setSceneDetect(int mode, std::uint32_t thresholdMilli) {
	const std::string problem = sceneDetectProblem(mode, thresholdMilli);
	if (!problem.empty()) throw std::invalid_argument("ju_tiled_set_scene_detect: " + problem);
	DeviceGuard g(m_Device);
	m_Stream->synchronize();
	// the clear's table goes and comes with the detector's memory, at a mode change
	// (a flow-free model has no recurrent input to clear: JU_SCENE_RESET reports)
	PinnedWords clear;
	if (mode != m_Scene.mode() && mode == 2 && m_Recurrent) clear = PinnedWords(sizeof(SceneClearTile) * kTileMax);
	if (m_Scene.configure(mode, thresholdMilli, m_SrcW * m_SrcH * 4)) m_SceneClear = std::move(clear);
}

void TiledRuntime::sceneDetect(int *mode, std::uint32_t *thresholdMilli) const {
	if (mode) *mode = m_Scene.mode();
	if (thresholdMilli) *thresholdMilli = m_Scene.threshold();
}

int TiledRuntime::sceneInfo(SceneRecord *out, int count) {
	if (count < 0 || (count > 0 && out == nullptr)) throw std::invalid_argument("ju_tiled_get_scene_info: NULL records or a negative count");
	DeviceGuard g(m_Device);
	m_Stream->synchronize();
	return m_Scene.records(out, count);
}

// The source into the tiles' inputs.  Detector off: the split alone, as ever.  On: ONE launch splits and takes the
// detector's step on the source frame (the split reads every source pixel anyway); in RESET mode on a recurrent model ONE
// more, behind it on the same stream, zeroes under the flag that step left what every tile's frame is about to read --
// m_State[m_Idx] and m_Packed[m_Idx] of each engine, the two buffers scene_clear_items_kernel covers for a group member.
// The host reads no decision.  A group pass that has to be run again (a resident-tower report) needs nothing new: the
// members have no detector of their own, and the pass wrote the OTHER halves only, so the cleared inputs are still in place.
// `into`: the tile inputs to fill -- m_In, or inside a look-ahead pass the frame's slot of m_PassIn.
void TiledRuntime::splitIn(const BgrxRows &src, const TileSet &into) {
	const int n = tiles();
	if (m_Scene.mode() == 0) {
		return launchTileSplit(src.ptr, src.stride, into, n, static_cast<int>(m_TileW), static_cast<int>(m_TileH), *m_Stream);
	}
	SceneSadLaunch q;
	m_Scene.fill(q);
	q.resetMode = m_Scene.mode() == 2 && m_Recurrent;
	launchTileSplitScene(src.ptr, src.stride, static_cast<int>(m_SrcW), static_cast<int>(m_SrcH), into, m_Own, n,
	    static_cast<int>(m_TileW), static_cast<int>(m_TileH), q, *m_Stream);
	if (q.resetMode) {
		// (rewritten every frame: the half a tile reads alternates.  The last frame's clear has completed: it ran in front of that frame's group passes, which are synchronous)
		SceneClearItem items[kTileMax];
		for (int k = 0; k < n; ++k) items[k] = m_Engines[static_cast<std::size_t>(k)]->recurrentInputs();
		launchSceneClearTiles(&q.state->resetNow, items, n, reinterpret_cast<volatile SceneClearTile *>(m_SceneClear.host()),
		    reinterpret_cast<const SceneClearTile *>(m_SceneClear.device()), *m_Stream);
	}
	m_Scene.advance();
}

// ---------------------------------------------------------------------------------------------------------------
// An output size (docs/tiled.md "An output size"): Engine::setOutputSize's rules with the blended frame in the place of the
// model's output.  The frame is scaled inside the blend's launch (stitchOut / stitchOutDeep), so all that is kept here is
// the scaler's two tables.
// ---------------------------------------------------------------------------------------------------------------
std::string tiledOutputSizeProblem(std::size_t width, std::size_t height, std::size_t srcW, std::size_t srcH, int filter) {
	const std::size_t bw = kTileScale * srcW, bh = kTileScale * srcH;
	const std::string problem = outputSizeProblem(width, height, bw, bh, filter);
	if (problem.empty() || !scaleFilterProblem(filter).empty()) return problem;
	return problem + " (of a tiled object: the blended frame " + std::to_string(bw) + "x" + std::to_string(bh) +
	       ", four times the tiled source size)";
}

void TiledRuntime::setOutputSize(std::size_t width, std::size_t height, int filter) {
	const bool off = width == 0 && height == 0;
	// (turning it off checks the filter all the same, as ju_set_output_size does)
	const std::string problem = tiledOutputSizeProblem(off ? kTileScale * m_SrcW : width, off ? kTileScale * m_SrcH : height, m_SrcW,
	    m_SrcH, filter);
	if (!problem.empty()) throw std::invalid_argument("ju_tiled_set_output_size: " + problem);
	// (alpha from the source goes straight from the source size to the new output frame: refused, both settings as they
	// were, where that leaves the alpha scaler's limits)
	const std::size_t aw = off ? kTileScale * m_SrcW : width, ah = off ? kTileScale * m_SrcH : height;
	const std::string alphaLimits = tiledAlphaProblem(m_AlphaMode, m_AlphaFilter, m_SrcW, m_SrcH, width, height);
	if (!alphaLimits.empty()) throw std::invalid_argument("ju_tiled_set_output_size: " + alphaLimits);
	DeviceGuard g(m_Device);
	Scaler scale, alphaScale;
	if (!off) scale.build(kTileScale * m_SrcW, kTileScale * m_SrcH, width, height, filter);
	if (m_AlphaMode == kAlphaSource) alphaScale.build(m_SrcW, m_SrcH, aw, ah, m_AlphaFilter);
	m_Stream->synchronize();  // (the call is synchronous, so nothing reads the old tables; kept for a stream shared later)
	m_OutScale = std::move(scale);
	m_AlphaScale = std::move(alphaScale);
	for (DeviceBuffer *b : {&m_OutStage[0], &m_OutStage[1], &m_Out16, &m_YuvOut[0], &m_YuvOut[1]}) *b = DeviceBuffer();  // (their sizes follow the output size)
}

void TiledRuntime::outputSize(std::size_t *width, std::size_t *height) const {
	if (width) *width = m_OutScale.dstW();
	if (height) *height = m_OutScale.dstH();
}

// ---------------------------------------------------------------------------------------------------------------
// A source mask (docs/tiled.md "A mask"): the engine's holder and copy (frame_io.h SourceMask), refused in this object's
// own order and words; the box is computed here, once.
// ---------------------------------------------------------------------------------------------------------------
void TiledRuntime::setSourceMask(const Frame *mask) {
	DeviceGuard g(m_Device);
	if (mask == nullptr) {
		m_Stream->synchronize();
		m_Mask = SourceMask();
		m_MaskBox = MaskBox();
		return;
	}
	if (mask->location != Location::Host && mask->location != Location::Device) {
		throw std::invalid_argument("ju_tiled_set_source_mask: the mask must be host or device memory");
	}
	const std::size_t bw = kTileScale * m_SrcW, bh = kTileScale * m_SrcH;  // the blended frame
	const std::string problem = maskSizeProblem(mask->width, mask->height, bw, bh);
	if (!problem.empty()) throw std::invalid_argument("ju_tiled_set_source_mask: " + problem);
	if (mask->ptr == nullptr) throw std::invalid_argument("ju_tiled_set_source_mask: NULL mask image");
	SourceMask copy = SourceMask::copyOf(*mask, "ju_tiled_set_source_mask");  // (copied once, now)
	const MaskBox box = copy.box(*mask, bw, bh);
	m_Stream->synchronize();
	m_Mask = std::move(copy);
	m_MaskBox = box;
}

// ---------------------------------------------------------------------------------------------------------------
// Alpha (docs/tiled.md "Alpha"): tests/alpha_reference.py from the tiled source size to the output frame's size.  The
// tiles' engines stay in mode 0 and the stitch kernels write X = 0 as ever; ONE launch of the engine's alpha kernels
// (launchAlphaFill / launchAlphaScale) rewrites the slot behind the frame's last colour launch, on the tiled stream.
// ---------------------------------------------------------------------------------------------------------------
std::string tiledAlphaProblem(int mode, int filter, std::size_t srcW, std::size_t srcH, std::size_t outW, std::size_t outH) {
	const bool off = outW == 0 && outH == 0;
	return alphaProblem(mode, filter, srcW, srcH, off ? kTileScale * srcW : outW, off ? kTileScale * srcH : outH);
}

void TiledRuntime::outputFrameSize(std::size_t *width, std::size_t *height) const {
	*width = m_OutScale.set() ? m_OutScale.dstW() : kTileScale * m_SrcW;
	*height = m_OutScale.set() ? m_OutScale.dstH() : kTileScale * m_SrcH;
}

void TiledRuntime::setAlpha(int mode, int filter) {
	std::size_t ow, oh;
	outputFrameSize(&ow, &oh);
	const std::string problem = tiledAlphaProblem(mode, filter, m_SrcW, m_SrcH, m_OutScale.dstW(), m_OutScale.dstH());
	if (!problem.empty()) throw std::invalid_argument("ju_tiled_set_alpha: " + problem);
	DeviceGuard g(m_Device);
	Scaler scale;
	if (mode == kAlphaSource) scale.build(m_SrcW, m_SrcH, ow, oh, filter);
	m_Stream->synchronize();
	m_AlphaScale = std::move(scale);
	m_AlphaMode = mode;
	m_AlphaFilter = filter;
}

void TiledRuntime::alpha(int *mode, int *filter) const {
	if (mode) *mode = m_AlphaMode;
	if (filter) *filter = m_AlphaFilter;
}

AlphaRows TiledRuntime::alphaSource(const AnyFrame &in, const BgrxRows &src, const DeviceBuffer &yuvStage) const {
	if (m_AlphaMode != kAlphaSource) return AlphaRows{};  // (nothing of the input is read)
	AlphaSide side;
	side.planar = in.yuv;
	side.bgrx = AlphaSideRows{src.ptr, src.stride};
	if (in.yuv) {
		side.format = in.planes.format;
		if (alphaKind(side.format) != kAlphaNone) {
			const YuvFrame &y = in.planes;
			const bool device = y.location == Location::Device;
			const YuvPlanes staged = device ? YuvPlanes{} : stagedPlanes(y, yuvStage.as<std::uint8_t>());
			side.plane0 = alphaLocated(device, AlphaSideRows{y.planes[0], y.strides[0]}, AlphaSideRows{staged.y, staged.yStride});
		}
	}
	return alphaRowsOf(side);
}

void TiledRuntime::alphaInto(PixelFormat format, void *rows, std::ptrdiff_t stride, const AlphaRows &alphaSrc) {
	AlphaSide side;
	side.planar = format != PixelFormat::Bgrx;
	side.format = format;
	side.bgrx = side.plane0 = AlphaSideRows{rows, stride};
	const AlphaRows sink = alphaRowsOf(side);
	if (!alphaLaunches(m_AlphaMode, sink.kind)) return;
	std::size_t ow, oh;
	outputFrameSize(&ow, &oh);
	if (m_AlphaMode == kAlphaOpaque) {
		launchAlphaFill(sink, static_cast<int>(ow), static_cast<int>(oh), *m_Stream);
	} else {
		launchAlphaScale(alphaSrc, static_cast<int>(m_SrcW), static_cast<int>(m_SrcH), sink, static_cast<int>(ow), static_cast<int>(oh),
		    m_AlphaScale.xAxis(), m_AlphaScale.yAxis(), m_AlphaScale.span(), *m_Stream);
	}
	++m_AlphaFrames;
}

void TiledRuntime::setDeepFromState(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_tiled_set_deep_from_state: " + std::to_string(on) + " is neither 0 nor 1");
	m_DeepFromState = on == 1;
}

// What ju_process_frame refuses for a frame of this size, and what a tiled frame cannot be: a graphics resource
void TiledRuntime::check(const AnyFrame &f, bool input, const char *who) const {
	const bool resized = !input && m_OutScale.set();  // (output frames are the output size while one is set)
	const std::size_t w = input ? m_SrcW : (resized ? m_OutScale.dstW() : kTileScale * m_SrcW);
	const std::size_t h = input ? m_SrcH : (resized ? m_OutScale.dstH() : kTileScale * m_SrcH);
	const std::string side = input ? "input" : "output";
	const std::string size = std::to_string(w) + "x" + std::to_string(h) +
	                         (input ? " (the tiled source size)" : (resized ? " (the output size set)" : " (four times the tiled source size)"));
	if (f.yuv) return checkPlanes(f.planes, side, w, h, size, who);
	auto refuse = [who](const std::string &why) { throw std::invalid_argument(std::string(who) + ": " + why); };
	const Frame &b = f.bgrx;
	if (b.location == Location::GraphicsResource) {
		refuse("graphics resources cannot be tiled " + side + "s (the tile kernels read and write host or device memory)");
	}
	if (b.ptr == nullptr) refuse("NULL " + side + " image");
	if (b.width != w || b.height != h) refuse(side + " image must be exactly " + size);
	const auto row = static_cast<std::ptrdiff_t>(w * 4);
	if (b.stride > -row && b.stride < row) refuse("|stride| smaller than a row");
}

DeviceBuffer &TiledRuntime::lazy(DeviceBuffer &b, std::size_t bytes) {
	if (b.bytes() < bytes) b = DeviceBuffer(bytes);
	return b;
}

// a device image on the split kernels' 4-byte alignment where it is; every other source through buffers sized here
BgrxRows TiledRuntime::stageIn(const AnyFrame &in, DeviceBuffer &srcStage, DeviceBuffer &yuvStage) {
	auto *stage = readsInPlace(in, true) ? nullptr : lazy(srcStage, m_SrcW * m_SrcH * 4).as<std::uint8_t>();
	const std::size_t planeBytes = hostPlaneBytes(in);
	auto *yuv = planeBytes ? lazy(yuvStage, planeBytes).as<std::uint8_t>() : nullptr;
	return stageInBgrx(in, m_SrcW, m_SrcH, stage, yuv, true, *m_Stream);
}

bool TiledRuntime::deepFromState(const AnyFrame &out) const {
	// (a mask: the masked frame exists in 8 bits only, as Engine::deepFromState has it)
	return out.yuv && m_DeepFromState && m_HbdFromState && !m_Mask.on() && formatInfo(out.planes.format).deep();
}

// The 16-bit path: ONE launch blends the states the tiles' last frames left -- the group passes are synchronous, so they
// are complete -- into the dense 16-bit frame, which the existing encode from such a frame turns into the caller's planes
// (a host frame's through their staging layout, as on the 8-bit route).
void TiledRuntime::stitchOutDeep(const YuvFrame &y, const AlphaRows &alphaSrc, int slot, HostCopy *defer) {
	const bool scaled = m_OutScale.set();
	const std::size_t bw = kTileScale * m_SrcW, bh = kTileScale * m_SrcH;  // the blended frame
	const std::size_t ow = scaled ? m_OutScale.dstW() : bw, oh = scaled ? m_OutScale.dstH() : bh;
	TileSet states = m_Out;  // (the origins; the pointers: each tile's state, whichever half its last frame wrote)
	for (int k = 0; k < tiles(); ++k) {
		states.ptr[k] = static_cast<std::uint8_t *>(const_cast<void *>(m_Engines[static_cast<std::size_t>(k)]->lastState()));
	}
	const bool host = y.location == Location::Host;
	std::uint8_t *yuv = host ? lazy(m_YuvOut[slot], stagedLayout(formatInfo(y.format), y.width, y.height, y.strides).bytes).as<std::uint8_t>() : nullptr;
	const YuvPlanes planes = host ? stagedPlanes(y, yuv) : callerPlanes(y);
	if (tiles() == 1 && !scaled) {
		// ONE tile: nothing to blend, and the frame is ju_process_frame's -- its encode from the state, which for the float
		// formats (RGBPH, RGBPS, BGR96F) is clamp(s + 0.5), not P / 65535 as from a 16-bit frame (docs/output_stage.md)
		launchEncodeState(fmt(y.format), y.colorspace, states.ptr[0], planes, static_cast<int>(ow), static_cast<int>(oh), *m_Stream);
	} else {
		auto *frame16 = lazy(m_Out16, ow * oh * 8).as<std::uint16_t>();
		if (scaled) {
			// ONE launch blends and scales (one tile too: ju_process_frame's bytes under ju_set_output_size, which also come
			// from a scaled 16-bit frame); nothing of the blended size is stored
			launchTileStitchScaleState(frame16, static_cast<int>(ow), static_cast<int>(oh), static_cast<int>(bw), static_cast<int>(bh), states,
			    tilesX(), tilesY(), static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(),
			    m_OutScale.xAxis(), m_OutScale.yAxis(), m_OutScale.span(), *m_Stream);
		} else {
			launchTileStitchState(frame16, static_cast<int>(ow), static_cast<int>(oh), states, tilesX(), tilesY(),
			    static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(), *m_Stream);
		}
		launchEncodeFrame16(fmt(y.format), y.colorspace, frame16, planes, static_cast<int>(ow), static_cast<int>(oh), *m_Stream);
	}
	alphaInto(y.format, planes.y, planes.yStride, alphaSrc);  // (plane 0 as the encode wrote it, in front of the copy out)
	if (host) deferOrCopyPlanes(y, yuv, defer);
	++m_DeepStateFrames;
}

void TiledRuntime::stitchOut(const AnyFrame &out, const BgrxRows &src, const AlphaRows &alphaSrc, int slot, HostCopy *defer) {
	// While an output size is set the frame is ow x oh of it and the blend's launch is the fused one, which forms the
	// blended frame in registers and writes the scaled one; everything behind the launch -- the staging frame, the copy
	// out, the encode -- is the same code at that size.  Off: exactly the launches of before.
	const bool scaled = m_OutScale.set();
	if (scaled) ++m_OutputScaledFrames;
	if (deepFromState(out)) return stitchOutDeep(out.planes, alphaSrc, slot, defer);
	const std::size_t bw = kTileScale * m_SrcW, bh = kTileScale * m_SrcH;  // the blended frame
	const std::size_t ow = scaled ? m_OutScale.dstW() : bw, oh = scaled ? m_OutScale.dstH() : bh, rowBytes = ow * 4;
	const auto plain = static_cast<std::ptrdiff_t>(rowBytes);
	// A mask whose box is not empty: the two masked launchers in the place of the two below, with the source rows stageIn
	// returned -- valid until the call returns.  No mask, or a white one: exactly the launches of before.
	const bool masked = m_Mask.on() && !m_MaskBox.empty();
	TileMask mk;
	if (masked) {
		mk.src = src.ptr;
		mk.srcStride = src.stride;
		mk.mask = m_Mask.first();
		mk.maskStride = m_Mask.stride();
		mk.maskW = static_cast<int>(m_Mask.width());
		mk.maskH = static_cast<int>(m_Mask.height());
		mk.x0 = m_MaskBox.x0, mk.y0 = m_MaskBox.y0, mk.x1 = m_MaskBox.x1, mk.y1 = m_MaskBox.y1;
	}
	auto stitch = [&](std::uint8_t *dst, std::ptrdiff_t stride) {
		if (masked && scaled) {
			return launchTileStitchMaskScale(dst, stride, static_cast<int>(ow), static_cast<int>(oh), static_cast<int>(bw), static_cast<int>(bh),
			    m_Out, tilesX(), tilesY(), static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(),
			    m_OutScale.xAxis(), m_OutScale.yAxis(), m_OutScale.span(), mk, *m_Stream);
		}
		if (masked) {
			return launchTileStitchMask(dst, stride, static_cast<int>(ow), static_cast<int>(oh), m_Out, tilesX(), tilesY(),
			    static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(), mk, *m_Stream);
		}
		if (scaled) {
			return launchTileStitchScale(dst, stride, static_cast<int>(ow), static_cast<int>(oh), static_cast<int>(bw), static_cast<int>(bh),
			    m_Out, tilesX(), tilesY(), static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(),
			    m_OutScale.xAxis(), m_OutScale.yAxis(), m_OutScale.span(), *m_Stream);
		}
		launchTileStitch(dst, stride, static_cast<int>(ow), static_cast<int>(oh), m_Out, tilesX(), tilesY(),
		    static_cast<int>(kTileScale * m_TileW), m_XTable.as<unsigned>(), m_YTable.as<unsigned>(), *m_Stream);
	};
	if (out.yuv) {  // the existing encode at output size, from the stitched 8-bit frame
		const YuvFrame &y = out.planes;
		auto *stage = lazy(m_OutStage[slot], rowBytes * oh).as<std::uint8_t>();
		stitch(stage, plain);
		const bool host = y.location == Location::Host;
		std::uint8_t *yuv = host ? lazy(m_YuvOut[slot], stagedLayout(formatInfo(y.format), y.width, y.height, y.strides).bytes).as<std::uint8_t>() : nullptr;
		const YuvPlanes planes = host ? stagedPlanes(y, yuv) : callerPlanes(y);
		launchEncodeFrame(fmt(y.format), y.colorspace, stage, plain, planes, static_cast<int>(ow), static_cast<int>(oh), *m_Stream);
		alphaInto(y.format, planes.y, planes.yStride, alphaSrc);  // (plane 0 as the encode wrote it, in front of the copy out)
		if (host) deferOrCopyPlanes(y, yuv, defer);
		return;
	}
	const Frame &b = out.bgrx;
	const bool device = b.location == Location::Device;
	if (device && reinterpret_cast<std::uintptr_t>(b.ptr) % 4 == 0 && b.stride % 4 == 0) {
		stitch(static_cast<std::uint8_t *>(b.ptr), b.stride);
		return alphaInto(PixelFormat::Bgrx, b.ptr, b.stride, alphaSrc);  // (the caller's aligned device rows)
	}
	// stitched in the caller's row order, copied out in memory order
	auto *stage = lazy(m_OutStage[slot], rowBytes * oh).as<std::uint8_t>();
	const RowSpan rows = rowSpan(b.ptr, b.stride, oh);
	std::uint8_t *first = rows.topDown ? stage : stage + static_cast<std::ptrdiff_t>(oh - 1) * plain;
	stitch(first, rows.topDown ? plain : -plain);
	alphaInto(PixelFormat::Bgrx, first, rows.topDown ? plain : -plain, alphaSrc);  // (the staging frame, in front of the copy out)
	if (defer != nullptr && !device) {  // a host frame of a pass: copied out by the caller, under the next frame's group passes
		defer->pending = true;
		defer->yuv = false;
		defer->rows = rows;
		defer->stage = stage;
		defer->rowBytes = rowBytes;
		defer->height = oh;
		return;
	}
	copyRows(rows.lowest, rows.pitch, stage, rowBytes, rowBytes, oh, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, *m_Stream);
}

// a host frame's planes out of their staging layout: now, on the tiled stream, or left to the pass (defer)
void TiledRuntime::deferOrCopyPlanes(const YuvFrame &y, std::uint8_t *yuv, HostCopy *defer) {
	if (defer == nullptr) return copyPlanes(y, yuv, false, *m_Stream);
	defer->pending = true;
	defer->yuv = true;
	defer->planes = y;
	defer->stage = yuv;
}

void TiledRuntime::copyOut(const HostCopy &c, int part, int parts, hipStream_t stream) {
	if (c.yuv) {  // (3.1 bytes per pixel or fewer against BGRX's 4, and plane by plane already: whole, with the first part)
		if (part == 0) copyPlanes(c.planes, c.stage, false, stream);
		return;
	}
	const std::size_t r0 = c.height * static_cast<std::size_t>(part) / static_cast<std::size_t>(parts);
	const std::size_t r1 = c.height * static_cast<std::size_t>(part + 1) / static_cast<std::size_t>(parts);
	if (r1 == r0) return;
	// (both sides in memory order: row r of the staging frame is row r of the caller's rows from their lowest)
	copyRows(c.rows.lowest + r0 * c.rows.pitch, c.rows.pitch, c.stage + r0 * c.rowBytes, c.rowBytes, c.rowBytes, r1 - r0,
	    hipMemcpyDeviceToHost, stream);
}

void TiledRuntime::checkPair(const AnyFrame &in, const AnyFrame &out, const char *who) const {
	check(in, true, who);
	check(out, false, who);
	if (ju::overlap(extentOf(out), extentOf(in))) {
		throw std::invalid_argument(std::string(who) + ": the output overlaps the input (the tiles read the source while the frame is written)");
	}
}

// Every tile's engine by one frame over the tile inputs `in`: a call of more tiles than one pass holds runs as the fewest
// passes, filled evenly (tilePasses) -- each call is synchronous.  under(p, passes), if any: the caller's host work under
// group pass p (Engine::processGroup runs it once: between the pass's last enqueue and its wait, or, where no pass was
// formed, behind the members' frames with inPass false).
void TiledRuntime::groupPasses(const TileSet &in, const std::function<void(int, int, bool)> &under, hipEvent_t after) {
	const int n = tiles();
	std::vector<Engine *> members(static_cast<std::size_t>(n));
	std::vector<Frame> tin(static_cast<std::size_t>(n)), tout(static_cast<std::size_t>(n));
	for (int k = 0; k < n; ++k) {
		members[k] = m_Engines[static_cast<std::size_t>(k)].get();
		tin[k] = Frame{in.ptr[k], Location::Device, static_cast<std::ptrdiff_t>(m_TileW * 4), m_TileW, m_TileH};
		tout[k] = Frame{m_Out.ptr[k], Location::Device, static_cast<std::ptrdiff_t>(m_TileW * 16), m_TileW * kTileScale, m_TileH * kTileScale};
	}
	const TilePasses passes = tilePasses(n, std::max(members[0]->lookahead(), 1));
	for (int p = 0; p < passes.passes; ++p) {
		const int at = passes.begin(p);
		if (under) {
			Engine::processGroup(members.data() + at, tin.data() + at, tout.data() + at, passes.count(p), [&](bool inPass) { under(p, passes.passes, inPass); },
			    after);
		} else {
			Engine::processGroup(members.data() + at, tin.data() + at, tout.data() + at, passes.count(p), {}, after);
		}
	}
}

void TiledRuntime::process(const AnyFrame &in, const AnyFrame &out, const char *who) {
	checkPair(in, out, who);
	DeviceGuard guard(m_Device);
	const BgrxRows src = stageIn(in, m_SrcStage, m_YuvIn);
	splitIn(src, m_In);
	// the group passes run on their lead's stream: the tiles' inputs (and at a scene cut their cleared recurrent inputs)
	// are complete before the first of them starts
	m_Stream->synchronize();
	groupPasses(m_In, {});
	stitchOut(out, src, alphaSource(in, src, m_YuvIn));
	m_Stream->synchronize();
	++m_Frames;
	if (m_Mask.on()) ++m_MaskFrames;
}

// ---------------------------------------------------------------------------------------------------------------
// Look-ahead passes (docs/tiled.md "Look-ahead passes").  The tiles' engines are driven exactly as process() drives them,
// frame by frame through the same group passes, so their states, histories and counters are process()'s; what a pass saves
// lies around them: K uploads and decodes issued up front, ONE split launch and ONE host wait for K frames, and a host
// frame's copy-out -- the largest single item of a 4K host frame -- under the next frame's group passes.
// ---------------------------------------------------------------------------------------------------------------
void TiledRuntime::processFrames(const AnyFrame *in, const AnyFrame *out, int count, const char *who) {
	const std::string name = who;
	if (count < 0 || (count > 0 && (in == nullptr || out == nullptr))) {
		throw std::invalid_argument(name + ": NULL frames or a negative count");
	}
	if (count == 0) return;
	// every pair, before anything is uploaded or launched ("<who>: <why>" -> "<who>: frame i: <why>")
	for (int i = 0; i < count; ++i) {
		try {
			checkPair(in[i], out[i], who);
		} catch (const std::invalid_argument &e) {
			const std::string what = e.what(), prefix = name + ": ";
			throw std::invalid_argument(prefix + "frame " + std::to_string(i) + ": " +
			                            (what.compare(0, prefix.size(), prefix) == 0 ? what.substr(prefix.size()) : what));
		}
	}
	if (count == 1 || m_Lookahead < 2) {
		for (int i = 0; i < count; ++i) process(in[i], out[i], who);
		return;
	}
	// A pass reads all its sources up front and writes its outputs frame by frame: an input plane over an output plane of
	// another frame of the call (one address space) keeps the two in different passes.  Outputs may repeat.
	std::vector<FrameExtent> ein(static_cast<std::size_t>(count)), eout(static_cast<std::size_t>(count));
	for (int i = 0; i < count; ++i) {
		ein[i] = extentOf(in[i]);
		eout[i] = extentOf(out[i]);
	}
	std::vector<int> starts = tilePassPlan(count, m_Lookahead, [&](int i, int j) {
		return ju::overlap(ein[j], eout[i]) || ju::overlap(eout[j], ein[i]);
	});
	starts.push_back(count);
	for (std::size_t p = 0; p + 1 < starts.size(); ++p) {
		const int at = starts[p], n = starts[p + 1] - at;
		if (n == 1) {
			process(in[at], out[at], who);
		} else {
			runPass(in + at, out + at, n);
		}
	}
}

void TiledRuntime::runPass(const AnyFrame *in, const AnyFrame *out, int count) {
	static_assert(kTilePassMax == kFlowBatchMax, "a pass's frames are the by-value argument of tile_split_frames_kernel");
	DeviceGuard guard(m_Device);
	const int n = tiles();
	// memory of the passes, made at the first one and sized by the cap: K source slots and K x T tile inputs
	const auto cap = static_cast<std::size_t>(std::max(m_Lookahead, count));
	if (m_PassSrc.size() < cap) {
		m_PassSrc.resize(cap);
		m_PassYuvIn.resize(cap);
	}
	m_PassSlot = m_TileInBytes * static_cast<std::size_t>(n);
	if (m_PassIn.bytes() < m_PassSlot * cap) {
		m_PassIn = DeviceBuffer(m_PassSlot * cap);
		for (int k = 0; k < n; ++k) {
			m_PassSet.ptr[k] = m_PassIn.as<std::uint8_t>() + m_TileInBytes * static_cast<std::size_t>(k);
			m_PassSet.x[k] = m_In.x[k];
			m_PassSet.y[k] = m_In.y[k];
		}
	}
	if (!m_CopyStream) {
		m_CopyStream = std::make_unique<Stream>();
		for (auto &e : m_Stitched) e = std::make_unique<Event>(hipEventDisableTiming);
	}
	// 1. the sources, all up front on the tiled stream: a device BGRX image on the kernels' alignment where it is, every
	// other one into its own slot.  (d) The slots, and the rule that inputs hold their pixels, keep the split's source rows
	// -- which a masked stitch reads again -- valid until stitch f.
	BgrxRows src[kTilePassMax];
	for (int f = 0; f < count; ++f) src[f] = stageIn(in[f], m_PassSrc[static_cast<std::size_t>(f)], m_PassYuvIn[static_cast<std::size_t>(f)]);
	auto slotOf = [&](int f) {
		TileSet t = m_PassSet;
		for (int k = 0; k < n; ++k) t.ptr[k] += m_PassSlot * static_cast<std::size_t>(f);
		return t;
	};
	// 2. the split: ONE launch for the whole pass while the detector is off (with it on: its decisions are sequential, so
	// the fused per-frame launch stays, in front of each frame's group passes -- step 3)
	const bool detects = m_Scene.mode() != 0;
	if (!detects) {
		TileFrames frames;
		for (int f = 0; f < count; ++f) {
			frames.src[f] = src[f].ptr;
			frames.stride[f] = static_cast<long long>(src[f].stride);
		}
		launchTileSplitFrames(frames, count, m_PassSet, m_PassSlot, n, static_cast<int>(m_TileW), static_cast<int>(m_TileH), *m_Stream);
		++m_PassSplitLaunches;
		// (b) the group passes run on their leads' streams: ONE host wait per pass puts every frame's tile inputs in front
		// of the first of them
		m_Stream->synchronize();
	}
	HostCopy copy[2];
	for (int f = 0; f < count; ++f) {
		const TileSet tin = slotOf(f);
		if (detects) {
			// 3. (b) with the detector on: the frame's split, decision and clear, and one host wait per frame as in process()
			splitIn(src[f], tin);
			m_Stream->synchronize();
		}
		// (a) frame f's group passes overwrite the tile outputs, and write the state halves, that stitch f - 1 reads: each
		// group pass's lead's stream -- a member's own on the member-by-member routes -- waits for the event behind
		// stitch f - 1 (Engine::processGroup's `after`); no host wait
		const hipEvent_t after = f > 0 ? m_Stitched[(f - 1) & 1]->get() : nullptr;
		// 5. the deferred copy: frame f - 1's host output goes out on the copy stream, behind the same event, while frame f's
		// group passes run -- a BGRX frame's rows divided among the passes, so that no pass is held up behind a whole frame
		const HostCopy &prev = copy[(f - 1) & 1];
		const bool overlapped = f > 0 && prev.pending;
		if (overlapped) {
			JU_HIP(hipStreamWaitEvent(*m_CopyStream, m_Stitched[(f - 1) & 1]->get(), 0));
			bool under = false;  // (whether any part ran while a group pass was in flight: the member-by-member routes do not overlap)
			groupPasses(tin, [&](int p, int passes, bool inPass) {
				under = under || inPass;
				copyOut(prev, p, passes, *m_CopyStream);
			}, after);
			// (c) staging slot (f - 1) & 1 is rewritten by stitch f + 1: copy f - 1 has completed here
			m_CopyStream->synchronize();
			copy[(f - 1) & 1].pending = false;
			if (under) ++m_PassOverlappedCopies;
		} else {
			groupPasses(tin, {}, after);
		}
		// 4. the blend, on the tiled stream; the group passes are synchronous, so the tiles' outputs and states are complete
		copy[f & 1] = HostCopy{};
		// (the alpha launch lies inside stitchOut, in front of the event that orders the deferred host copy)
		stitchOut(out[f], src[f], alphaSource(in[f], src[f], m_PassYuvIn[static_cast<std::size_t>(f)]), f & 1, &copy[f & 1]);
		m_Stitched[f & 1]->record(*m_Stream);
		++m_Frames;
		if (m_Mask.on()) ++m_MaskFrames;
	}
	// the last frame's copy runs behind the pass
	const HostCopy &last = copy[(count - 1) & 1];
	m_Stream->synchronize();
	if (last.pending) {
		copyOut(last, 0, 1, *m_CopyStream);
		m_CopyStream->synchronize();
	}
	++m_PassCalls;
	m_PassFrames += static_cast<std::uint64_t>(count);
}

}  // namespace ju
