// Frames in and out of the engine: the staging copies of BGRX images, the one frame check, YUV planes through the
// conversion kernels, the source stage (scale, mask) and the output stage, and submitFrame, the staged path that strings
// them around a frame's program.  engine.cpp holds the program and submit(), the direct path; engine_passes.cpp the
// look-ahead and group passes.
#include <stdexcept>
#include <string>

#include "alpha_route.h"
#include "engine.h"
#include "graphics.h"

namespace ju {

namespace {
// Scoped map of a graphics resource on the engine's stream (cuda.h:310-349 GraphicsResource):
// unmapped again when the copy has been enqueued, also when that throws.
struct MappedResource {
	GraphicsHandle *h;
	hipStream_t stream;
	GraphicsArray array;
	MappedResource(void *handle, hipStream_t s) : h(static_cast<GraphicsHandle *>(handle)), stream(s) {
		if (h == nullptr || h->backend == nullptr) throw std::invalid_argument("processImage: NULL graphics resource");
		array = h->backend->map(h->resource, stream);
	}
	~MappedResource() { h->backend->unmap(h->resource, stream); }
	MappedResource(const MappedResource &) = delete;
	MappedResource &operator=(const MappedResource &) = delete;
};
}  // namespace

void Engine::stageIn(const Frame &in) {
	const FrameSize fs = frameSize();
	checkFrame(anyOf(in), true, "processImage");  // (a pair that takes submit() is refused here, not up front)
	if (in.location == Location::GraphicsResource) {
		// map -> texture array -> staging buffer -> unmap (cuda_convert.h:57-77,
		// cuda_convert.cc.cu:380-397); the array's own extent is what counts
		MappedResource m(in.ptr, m_Stream);
		if (!m.array.fourBytes || m.array.width != fs.inputWidth || m.array.height != fs.inputHeight ||
		    in.width != fs.inputWidth || in.height != fs.inputHeight) {
			throw std::invalid_argument("processImage: input texture must be " + std::to_string(fs.inputWidth) + "x" +
			                            std::to_string(fs.inputHeight) + " with four 8-bit channels");
		}
		m.h->backend->copyFromArray(m_InStage.get(), fs.inputWidth * 4, m.array, fs.inputWidth * 4, fs.inputHeight,
		    m_Stream);
		return;
	}
	const std::size_t rowBytes = fs.inputWidth * 4;
	const std::size_t rows = fs.inputHeight;
	const auto plain = static_cast<std::ptrdiff_t>(rowBytes);
	auto *dst = m_InStage.as<std::uint8_t>();
	auto *src = static_cast<std::uint8_t *>(in.ptr);
	const RowSpan span = rowSpan(src, in.stride, rows);
	switch (in.location) {
	case Location::Host:
		if (span.topDown) {
			copyRows(dst, rowBytes, span.lowest, span.pitch, rowBytes, rows, hipMemcpyHostToDevice, m_Stream);
		} else {
			// bottom-up frame (AviSynth RGB32, avisynth_plugin/src/main.cc:125-142): upload
			// the rows in memory order, then flip on the device.
			auto *raw = m_RawStage.as<std::uint8_t>();
			copyRows(raw, rowBytes, span.lowest, span.pitch, rowBytes, rows, hipMemcpyHostToDevice, m_Stream);
			launchCopyRows(raw + (rows - 1) * rowBytes, -plain, dst, plain, rowBytes, rows, m_Stream);
		}
		break;
	case Location::Device:
		if (in.stride == plain) {
			copyRows(dst, rowBytes, src, rowBytes, rowBytes, rows, hipMemcpyDeviceToDevice, m_Stream);
		} else {
			launchCopyRows(src, in.stride, dst, plain, rowBytes, rows, m_Stream);
		}
		break;
	default:
		throw std::invalid_argument(
		    "processImage: GRAPHICS_RESOURCE images are not supported by this runtime");
	}
}

void Engine::stageOut(const Frame &out, std::size_t width, std::size_t height, const std::uint8_t *src, std::uint8_t *raw) {
	const FrameSize fs{0, 0, width, height};  // (the frame's own size: the model's output, or the output size set)
	checkFrame(anyOf(out), false, "processImage");  // (behind the step, for a pair that takes submit(): as ju_process always did)
	if (out.location == Location::GraphicsResource) {  // cuda_convert.cc.cu:419-436
		MappedResource m(out.ptr, m_Stream);
		if (!m.array.fourBytes || m.array.width != fs.outputWidth || m.array.height != fs.outputHeight ||
		    out.width != fs.outputWidth || out.height != fs.outputHeight) {
			throw std::invalid_argument("processImage: output texture must be " + std::to_string(fs.outputWidth) + "x" +
			                            std::to_string(fs.outputHeight) + " with four 8-bit channels");
		}
		m.h->backend->copyToArray(m.array, src, fs.outputWidth * 4, fs.outputWidth * 4, fs.outputHeight, m_Stream);
		return;
	}
	const std::size_t rowBytes = fs.outputWidth * 4;
	const std::size_t rows = fs.outputHeight;
	const auto plain = static_cast<std::ptrdiff_t>(rowBytes);
	auto *dst = static_cast<std::uint8_t *>(out.ptr);
	const RowSpan span = rowSpan(dst, out.stride, rows);
	switch (out.location) {
	case Location::Host:
		if (span.topDown) {
			copyRows(span.lowest, span.pitch, src, rowBytes, rowBytes, rows, hipMemcpyDeviceToHost, m_Stream);
		} else {  // (bottom-up: flip on the device, download the rows in memory order)
			launchCopyRows(src, plain, raw + (rows - 1) * rowBytes, -plain, rowBytes, rows, m_Stream);
			copyRows(span.lowest, span.pitch, raw, rowBytes, rowBytes, rows, hipMemcpyDeviceToHost, m_Stream);
		}
		break;
	case Location::Device:
		if (out.stride == plain) {
			copyRows(dst, rowBytes, src, rowBytes, rowBytes, rows, hipMemcpyDeviceToDevice, m_Stream);
		} else {
			launchCopyRows(src, plain, dst, out.stride, rowBytes, rows, m_Stream);
		}
		break;
	default:
		throw std::invalid_argument(
		    "processImage: GRAPHICS_RESOURCE images are not supported by this runtime");
	}
}

// Everything a frame call can refuse, checked before anything is launched (the BGRX side repeats what stageIn /
// stageOut would throw, so that a refused call has not run the step).
void Engine::checkFrame(const AnyFrame &f, bool input, const char *who, bool declaredSize) const {
	const FrameSize fs = frameSize();
	const bool scaled = input && m_SrcScale.set();  // (input frames are the source's size while one is set)
	const bool resized = !input && m_OutScale.set();  // (and output frames the output size)
	const std::size_t w = scaled ? m_SrcScale.srcW() : (resized ? m_OutScale.dstW() : (input ? fs.inputWidth : fs.outputWidth));
	const std::size_t h = scaled ? m_SrcScale.srcH() : (resized ? m_OutScale.dstH() : (input ? fs.inputHeight : fs.outputHeight));
	const std::string side = input ? "input" : "output";
	const std::string size = std::to_string(w) + "x" + std::to_string(h) +
	                         (scaled ? " (the source size set)" : (resized ? " (the output size set)" : ""));
	auto refuse = [who](const std::string &why) { throw std::invalid_argument(std::string(who) + ": " + why); };
	if (!f.yuv) {
		const Frame &b = f.bgrx;
		const bool resource = b.location == Location::GraphicsResource;
		if (resized && resource) {
			refuse("graphics resources cannot be outputs while an output size is set (the scaler writes host or device memory)");
		}
		if (scaled && resource) {
			refuse("graphics resources cannot be inputs while a source size is set (the scaler reads host or device memory)");
		}
		if (resource && !declaredSize) {
			if (b.ptr == nullptr) refuse("NULL graphics resource");
			return;  // (the texture's own extent is checked when it is mapped)
		}
		if (declaredSize && b.ptr == nullptr) refuse("NULL " + side + " image");
		if (b.ptr == nullptr || b.width != w || b.height != h) refuse(side + " image must be exactly " + size);
		const auto row = static_cast<std::ptrdiff_t>(w * 4);
		if (!resource && b.stride > -row && b.stride < row) refuse("|stride| smaller than a row");
		return;
	}
	checkPlanes(f.planes, side, w, h, size, who);
}

// The non-BGRX half of the one frame check, for a frame that must be w x h (`size`: how the messages call that size):
// shared with the tiled runtime (tiled.cpp), whose frames have its own sizes.
void checkPlanes(const YuvFrame &y, const std::string &side, std::size_t w, std::size_t h, const std::string &size, const char *who) {
	auto refuse = [who](const std::string &why) { throw std::invalid_argument(std::string(who) + ": " + why); };
	const YuvFormatInfo *known = yuvFormatInfo(fmt(y.format));
	if (known == nullptr) refuse("unknown " + side + " pixel format");
	const YuvFormatInfo &info = *known;
	const std::string name = info.name;
	// (an RGB frame has no colour space: the field is ignored)
	if (!info.rgb()) {  // (matrix | siting: kernels.h; a 4:4:4 format takes a valid siting and ignores it)
		const std::string fault = colourSpaceFault(y.colorspace, side + " ");
		if (!fault.empty()) refuse(fault);
	}
	if (y.location != Location::Host && y.location != Location::Device) {
		refuse(name + " " + side + " frames must be host or device memory (no graphics resources)");
	}
	if (info.sampling == 420 && (y.width % 2 || y.height % 2)) refuse(name + " needs an even width and height");
	if (info.sampling == 422 && y.width % 2) refuse(name + " (4:2:2) needs an even width");
	if (y.width != w || y.height != h) refuse(side + " frame must be exactly " + size);
	for (int k = 0; k < info.planes; ++k) {
		const std::string plane = side + " plane " + std::to_string(k);
		if (y.planes[k] == nullptr) refuse(plane + " is NULL");
		const auto sample = static_cast<std::size_t>(info.sampleBytes);
		if (sample > 1 && (reinterpret_cast<std::uintptr_t>(y.planes[k]) % sample != 0 ||
		                   y.strides[k] % static_cast<std::ptrdiff_t>(sample) != 0)) {
			refuse(plane + ": " + name + " samples are " + (sample == 2 ? "16-bit" : "32-bit") +
			       " words -- the plane's address and its stride must be multiples of " + std::to_string(sample));
		}
		const auto row = static_cast<std::ptrdiff_t>(planeShape(info, w, h, k).rowBytes);
		if (y.strides[k] > -row && y.strides[k] < row) refuse(plane + ": |stride| smaller than a row");
	}
}

void Engine::checkPair(const AnyFrame &in, const AnyFrame &out) const {
	if (!staged(in, out)) return;  // (a pair that takes submit() is refused where it is staged, as ju_process always did)
	checkFrame(in, true);
	checkFrame(out, false);
	checkAlphaOverlap(in, out);
}

// alpha from the source is read behind the frame's colour: an output over the input would have rewritten it
void Engine::checkAlphaOverlap(const AnyFrame &in, const AnyFrame &out) const {
	if (m_AlphaMode == kAlphaSource && locationOf(in) == Location::Device && locationOf(out) == Location::Device &&
	    overlap(extentOf(in), extentOf(out))) {
		throw std::invalid_argument("processFrame: under JU_ALPHA_SOURCE a device output must not overlap the device input (the "
		                            "input's alpha is read after the output's colour is written)");
	}
}

bool Engine::deepFromState(PixelFormat format) const {
	// (a mask: the blended frame exists in 8 bits only)
	return m_HbdFromState && !m_Mask.on() && formatInfo(format).deep();
}

// one encode launch on the engine's stream behind a frame's last kernel: the frame's BGRX rows -- or, for a 10-bit YUV or
// a deep RGB format of a runtime whose state is the frame in float (m_HbdFromState), the f16 state that frame left -- -> planes
void Engine::encodeYuv(PixelFormat format, int colorspace, const YuvPlanes &planes, std::size_t width, std::size_t height,
    const std::uint8_t *bgrx, std::ptrdiff_t bgrxStride, const void *state, const std::uint16_t *frame16, hipStream_t stream) {
	const int w = static_cast<int>(width), h = static_cast<int>(height);
	if (stream == nullptr) stream = m_Stream;
	if (!deepFromState(format)) {
		launchEncodeFrame(fmt(format), colorspace, bgrx, bgrxStride, planes, w, h, stream);
	} else if (frame16 != nullptr) {  // (the output stage: the state's samples, scaled)
		launchEncodeFrame16(fmt(format), colorspace, frame16, planes, w, h, stream);
	} else {
		launchEncodeState(fmt(format), colorspace, state, planes, w, h, stream);
	}
}

// the frame of out.width x out.height -- its dense BGRX rows, or for deepFromState formats the state or the 16-bit frame
void Engine::stageOutYuv(const YuvFrame &out, const std::uint8_t *bgrx, const void *state, const std::uint16_t *frame16,
    std::uint8_t *stage) {
	const bool host = out.location == Location::Host;
	// (a host frame: the kernel writes the staging buffer in the caller's row order, copied out below)
	const YuvPlanes pl = host ? stagedPlanes(out, stage) : callerPlanes(out);
	encodeYuv(out.format, out.colorspace, pl, out.width, out.height, bgrx, static_cast<std::ptrdiff_t>(out.width * 4), state,
	    frame16);
	alphaInto(out.format, pl.y, pl.yStride);
	if (host) copyPlanes(out, stage, false, m_Stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Source stage (docs/source_stage.md).  What the reference's OBS filter does around processImage in its graphics API
// (obs_plugin/src/filter.cc:351-379: any source drawn into the model's input texture; :393-402 with blend.effect: the
// point-sampled source drawn back over the output through mask.png), as two kernels around the staged graph of
// submitFrame: scale_bgrx_kernel fills m_InStage from the source frame, mask_blend_kernel rewrites m_OutStage.  Both
// settings are per runtime and opt-in; neither touches a captured graph, the state or the frame history.
// ---------------------------------------------------------------------------------------------------------------
void Engine::setSourceSize(std::size_t width, std::size_t height, int filter) {
	DeviceGuard g(m_Device);
	const std::string unknown = scaleFilterProblem(filter);
	if (!unknown.empty()) throw std::invalid_argument("ju_set_source_size: " + unknown);
	const FrameSize fs = frameSize();
	std::size_t inW, inH, outW, outH;
	frameSizes(&inW, &inH, &outW, &outH);
	if (width == 0 && height == 0) {
		Scaler alpha = alphaScalerFor("ju_set_source_size", m_AlphaMode, m_AlphaFilter, fs.inputWidth, fs.inputHeight, outW, outH);
		m_Stream.synchronize();  // (enqueued frames may still read the tables)
		if (m_SrcScale.set()) dropStagePasses();
		m_SrcScale.clear();
		dropAlphaPasses();
		m_AlphaScale = std::move(alpha);
		m_SrcStage = DeviceBuffer();
		m_SrcYuvStage = DeviceBuffer();
		return;
	}
	const std::string problem = sourceSizeProblem(width, height, fs.inputWidth, fs.inputHeight, filter);
	if (!problem.empty()) throw std::invalid_argument("ju_set_source_size: " + problem);
	Scaler alpha = alphaScalerFor("ju_set_source_size", m_AlphaMode, m_AlphaFilter, width, height, outW, outH);
	Scaler scale;
	scale.build(width, height, fs.inputWidth, fs.inputHeight, filter);
	DeviceBuffer stage(width * height * 4), yuvStage(yuvStageBytes(kFormatTable, width, height));
	m_Stream.synchronize();
	dropStagePasses();  // (the staged passes' graphs and slots are of the old size and tables)
	m_SrcScale = std::move(scale);
	dropAlphaPasses();
	m_AlphaScale = std::move(alpha);
	m_SrcStage = std::move(stage);
	m_SrcYuvStage = std::move(yuvStage);
}

void Engine::sourceSize(std::size_t *width, std::size_t *height) const {
	if (width) *width = m_SrcScale.srcW();
	if (height) *height = m_SrcScale.srcH();
}

void Engine::setSourceMask(const Frame *mask) {
	DeviceGuard g(m_Device);
	if (mask == nullptr) {
		m_Stream.synchronize();
		if (m_Mask.on()) dropStagePasses();
		m_Mask = SourceMask();
		return;
	}
	if (mask->location != Location::Host && mask->location != Location::Device) {
		throw std::invalid_argument("ju_set_source_mask: the mask must be host or device memory");
	}
	if (mask->ptr == nullptr || mask->width < 1 || mask->height < 1 || mask->width > kMaskAxisMax || mask->height > kMaskAxisMax) {
		throw std::invalid_argument("ju_set_source_mask: the mask must be 1 .. 16384 pixels on each axis");
	}
	SourceMask copy = SourceMask::copyOf(*mask, "ju_set_source_mask");  // (copied once, now)
	m_Stream.synchronize();
	dropStagePasses();  // (their blend launches hold the old mask's address)
	m_Mask = std::move(copy);
}

// ---------------------------------------------------------------------------------------------------------------
// Output stage (docs/output_stage.md).  What the reference's OBS caller gets from OBS's canvas scaling behind
// processImage: the upscaled frame at any size.  Behind the staged graph and the mask blend of submitFrame the frame is
// scaled by the source stage's scaler (the triangle or a cubic filter) with the output axes' tables: the 8-bit frame in m_OutStage by
// scale_bgrx_kernel, or -- for a deep format that is encoded from the state (deepFromState) -- the state's 16-bit samples
// by scale_state_kernel into m_OutScaled16, which launchEncodeFrame16 encodes.  Nothing of the step itself changes.
// ---------------------------------------------------------------------------------------------------------------
void Engine::setOutputSize(std::size_t width, std::size_t height, int filter) {
	DeviceGuard g(m_Device);
	const FrameSize fs = frameSize();
	const bool off = width == 0 && height == 0;
	const std::string problem = outputSizeProblem(off ? fs.outputWidth : width, off ? fs.outputHeight : height, fs.outputWidth,
	    fs.outputHeight, filter);
	if (!problem.empty()) throw std::invalid_argument("ju_set_output_size: " + problem);
	std::size_t inW, inH, outW, outH;
	frameSizes(&inW, &inH, &outW, &outH);
	Scaler alpha = alphaScalerFor("ju_set_output_size", m_AlphaMode, m_AlphaFilter, inW, inH, off ? fs.outputWidth : width,
	    off ? fs.outputHeight : height);
	if (off) {
		m_Stream.synchronize();  // (enqueued frames may still read the tables and write the buffers)
		if (m_OutScale.set()) dropStagePasses();
		m_OutScale.clear();
		dropAlphaPasses();
		m_AlphaScale = std::move(alpha);
		for (DeviceBuffer *b : {&m_OutScaled8, &m_OutScaled16, &m_OutYuvStage, &m_OutRawStage}) *b = DeviceBuffer();
		return;
	}
	Scaler scale;
	scale.build(fs.outputWidth, fs.outputHeight, width, height, filter);
	DeviceBuffer scaled8(width * height * 4), scaled16(width * height * 8), raw(width * height * 4);
	DeviceBuffer yuvStage(yuvStageBytes(kFormatTable, width, height));
	m_Stream.synchronize();
	dropStagePasses();
	m_OutScale = std::move(scale);
	dropAlphaPasses();
	m_AlphaScale = std::move(alpha);
	m_OutScaled8 = std::move(scaled8);
	m_OutScaled16 = std::move(scaled16);
	m_OutRawStage = std::move(raw);
	m_OutYuvStage = std::move(yuvStage);
}

void Engine::outputSize(std::size_t *width, std::size_t *height) const {
	if (width) *width = m_OutScale.dstW();
	if (height) *height = m_OutScale.dstH();
}

// The stage-out of a frame while an output size is set: scale, then copy or encode at output size.  A device BGRX image
// is written in place (the kernel takes any alignment and signed stride); a host image and YUV planes go through the
// scaled staging buffers.
void Engine::stageOutScaled(const AnyFrame &out) {
	const std::size_t ow = m_OutScale.dstW(), oh = m_OutScale.dstH();
	auto scale8 = [&](std::uint8_t *dst, std::ptrdiff_t stride) {
		m_OutScale.scaleBgrx(m_OutStage.as<std::uint8_t>(), static_cast<std::ptrdiff_t>(m_OutScale.srcW() * 4), dst, stride, m_Stream);
	};
	auto *scaled8 = m_OutScaled8.as<std::uint8_t>();
	const auto plain = static_cast<std::ptrdiff_t>(ow * 4);
	if (!out.yuv) {
		const Frame &b = out.bgrx;
		if (b.location == Location::Device) {
			scale8(static_cast<std::uint8_t *>(b.ptr), b.stride);
			return alphaInto(PixelFormat::Bgrx, b.ptr, b.stride);  // (the caller's rows, where the scaler wrote them)
		}
		scale8(scaled8, plain);
		alphaInto(PixelFormat::Bgrx, scaled8, plain);
		return stageOut(b, ow, oh, scaled8, m_OutRawStage.as<std::uint8_t>());
	}
	auto *yuvStage = m_OutYuvStage.as<std::uint8_t>();
	if (deepFromState(out.planes.format)) {
		auto *scaled16 = m_OutScaled16.as<std::uint16_t>();
		m_OutScale.scaleState(m_State[m_Config.recurrent() ? m_Idx ^ 1 : 0].get(), scaled16, m_Stream);
		return stageOutYuv(out.planes, nullptr, nullptr, scaled16, yuvStage);
	}
	scale8(scaled8, plain);
	stageOutYuv(out.planes, scaled8, nullptr, nullptr, yuvStage);
}

// Staged frames (a YUV side; any pair while a source or output stage is set): always through the staging buffers -- the conversion kernel takes the place of the
// staging copy on its side and the binding set's staged graph replays unchanged.  The conversions are eager launches
// on m_Stream OUTSIDE the per-device chain lock, like the staging copies of submit().
void Engine::submitFrame(const AnyFrame &in, const AnyFrame &out) {
	m_DirectIO = false;
	bindStaging();
	const FrameSize fs = frameSize();
	// what the mask lets through: the source frame at source size, or the model-size input frame
	BgrxRows source{m_InStage.as<std::uint8_t>(), static_cast<std::ptrdiff_t>(fs.inputWidth * 4)};
	if (m_SrcScale.set()) {
		// the frame at source size: a device image where it is (the scaler takes any alignment), else through m_SrcStage
		source = stageInBgrx(in, m_SrcScale.srcW(), m_SrcScale.srcH(), m_SrcStage.as<std::uint8_t>(), m_SrcYuvStage.as<std::uint8_t>(),
		    false, m_Stream);
		m_SrcScale.scaleBgrx(source.ptr, source.stride, m_InStage.as<std::uint8_t>(), static_cast<std::ptrdiff_t>(fs.inputWidth * 4),
		    m_Stream);
	} else if (in.yuv) {
		decodePlanes(in.planes, m_YuvInStage.as<std::uint8_t>(), m_InStage.as<std::uint8_t>(), m_Stream);
	} else {
		stageIn(in.bgrx);
	}
	if (m_AlphaMode == kAlphaSource) m_AlphaSrc = alphaSource(in, source);
	sceneStep();  // (the decoded, scaled frame: what the program reads)
	{
		std::unique_lock<std::mutex> chain = chainBegin(m_Resident);
		runProgram();
		chainEnd(chain, m_Resident);
	}
	if (m_Mask.on()) {
		// over the frame handed to the caller only: state and history are the unmasked run's
		blendMask(m_OutStage.as<std::uint8_t>(), static_cast<std::ptrdiff_t>(fs.outputWidth * 4), source.ptr, source.stride,
		    m_SrcScale.set() ? m_SrcScale.srcW() : fs.inputWidth, m_SrcScale.set() ? m_SrcScale.srcH() : fs.inputHeight, m_Stream);
	}
	if (sourceStage()) ++m_SourceFrames;
	// (behind the frame's program and before the flip: the state this frame wrote is the binding set's output)
	if (m_OutScale.set()) {
		stageOutScaled(out);
	} else if (out.yuv) {
		stageOutYuv(out.planes, m_OutStage.as<std::uint8_t>(), m_State[m_Config.recurrent() ? m_Idx ^ 1 : 0].get(), nullptr,
		    m_YuvOutStage.as<std::uint8_t>());
	} else {
		alphaInto(PixelFormat::Bgrx, m_OutStage.get(), static_cast<std::ptrdiff_t>(fs.outputWidth * 4));  // (the dense frame stageOut copies)
		stageOut(out.bgrx, fs.outputWidth, fs.outputHeight, m_OutStage.as<std::uint8_t>(), m_RawStage.as<std::uint8_t>());
	}
	m_Idx ^= 1;
}

// ---------------------------------------------------------------------------------------------------------------
// Alpha (docs/alpha.md).  The reference writes X = 0 on every route (cuda_convert.cc.cu:39-45) and so does every kernel
// here; under ju_set_alpha ONE more launch follows a frame's colour on the staged route and writes the alpha slot of the
// frame about to be handed out -- the top code (alpha_fill_kernel), or the input frame's alpha scaled from the input
// frame's size straight to the output frame's size, never through the model's (alpha_scale_kernel).  The decode, encode
// and scale kernels are untouched: the slot they left 0 is rewritten behind them, before any copy to the host.
// ---------------------------------------------------------------------------------------------------------------
void Engine::frameSizes(std::size_t *inW, std::size_t *inH, std::size_t *outW, std::size_t *outH) const {
	const FrameSize fs = frameSize();
	*inW = m_SrcScale.set() ? m_SrcScale.srcW() : fs.inputWidth;
	*inH = m_SrcScale.set() ? m_SrcScale.srcH() : fs.inputHeight;
	*outW = m_OutScale.set() ? m_OutScale.dstW() : fs.outputWidth;
	*outH = m_OutScale.set() ? m_OutScale.dstH() : fs.outputHeight;
}

Scaler Engine::alphaScalerFor(const char *who, int mode, int filter, std::size_t inW, std::size_t inH, std::size_t outW,
    std::size_t outH) const {
	const std::string problem = alphaProblem(mode, filter, inW, inH, outW, outH);
	if (!problem.empty()) throw std::invalid_argument(std::string(who) + ": " + problem);
	Scaler scale;
	if (mode == kAlphaSource) scale.build(inW, inH, outW, outH, filter);
	return scale;
}

void Engine::setAlpha(int mode, int filter) {
	DeviceGuard g(m_Device);
	std::size_t inW, inH, outW, outH;
	frameSizes(&inW, &inH, &outW, &outH);
	Scaler alpha = alphaScalerFor("ju_set_alpha", mode, filter, inW, inH, outW, outH);
	m_Stream.synchronize();  // (enqueued frames may still read the tables)
	dropAlphaPasses();
	m_AlphaScale = std::move(alpha);
	m_AlphaMode = mode;
	m_AlphaFilter = filter;
}

void Engine::alpha(int *mode, int *filter) const {
	if (mode) *mode = m_AlphaMode;
	if (filter) *filter = m_AlphaFilter;
}

// (alpha_route.h: format and location give the kind and the rows -- the rule the passes bind by as well)
AlphaRows Engine::alphaSource(const AnyFrame &in, const BgrxRows &bgrx) {
	AlphaSide side;
	side.planar = in.yuv;
	// the BGRX rows: a device frame in place; a host frame (or a graphics resource) where submitFrame staged it
	side.bgrx = in.yuv ? AlphaSideRows{bgrx.ptr, bgrx.stride}
	                   : alphaLocated(in.bgrx.location == Location::Device, AlphaSideRows{in.bgrx.ptr, in.bgrx.stride},
	                         AlphaSideRows{bgrx.ptr, bgrx.stride});
	if (in.yuv) {
		side.format = in.planes.format;
		if (alphaKind(side.format) != kAlphaNone) {
			// a host frame: the planes decodePlanes uploaded, still in their staging buffer
			const bool device = in.planes.location == Location::Device;
			const YuvPlanes pl = device ? YuvPlanes{} : stagedPlanes(in.planes, (m_SrcScale.set() ? m_SrcYuvStage : m_YuvInStage).as<std::uint8_t>());
			side.plane0 = alphaLocated(device, AlphaSideRows{in.planes.planes[0], in.planes.strides[0]}, AlphaSideRows{pl.y, pl.yStride});
		}
	}
	return alphaRowsOf(side);
}

bool Engine::launchAlpha(const AlphaRows &src, const AlphaRows &sink, hipStream_t stream) {
	if (!alphaLaunches(m_AlphaMode, sink.kind)) return false;
	std::size_t inW, inH, outW, outH;
	frameSizes(&inW, &inH, &outW, &outH);
	if (m_AlphaMode == kAlphaOpaque) {
		launchAlphaFill(sink, static_cast<int>(outW), static_cast<int>(outH), stream);
	} else {
		launchAlphaScale(src, static_cast<int>(inW), static_cast<int>(inH), sink, static_cast<int>(outW), static_cast<int>(outH),
		    m_AlphaScale.xAxis(), m_AlphaScale.yAxis(), m_AlphaScale.span(), stream);
	}
	return true;
}

void Engine::alphaInto(PixelFormat format, void *rows, std::ptrdiff_t stride) {
	AlphaSide side;
	side.planar = format != PixelFormat::Bgrx;
	side.format = format;
	side.bgrx = side.plane0 = AlphaSideRows{rows, stride};  // (the side's own rows: the dense BGRX frame, or plane 0 as the encode wrote it)
	if (launchAlpha(m_AlphaSrc, alphaRowsOf(side), m_Stream)) ++m_AlphaFrames;
}

// ---------------------------------------------------------------------------------------------------------------
// Scene detector (docs/scene_detect.md).  Two eager launches per step in front of the step's program: the sum of
// absolute differences against the kept frame with the decision in its last workgroup, and the conditional clear of
// what the program is about to read as its recurrent inputs -- m_State[m_Idx] and m_Packed[m_Idx], the half reset()
// would have left zero for this step.  The binding set is NOT reset: the two sets' programs differ in bindings only.
// The host learns of a cut only when it asks (sceneInfo); nothing in the frame path waits for the decision.
// ---------------------------------------------------------------------------------------------------------------
void Engine::setSceneDetect(int mode, std::uint32_t thresholdMilli) {
	const std::string problem = sceneDetectProblem(mode, thresholdMilli);
	if (!problem.empty()) throw std::invalid_argument("ju_set_scene_detect: " + problem);
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	// A mode change is a start: fresh memory for the model-size input, no predecessor, step 0.  The only captured graphs
	// bound to the old buffers are those of passes that carry the detector (PassKey::scene != 0): they go first.
	if (mode != m_Scene.mode()) dropScenePassGraphs();
	const FrameSize fs = frameSize();
	m_Scene.configure(mode, thresholdMilli, fs.inputWidth * fs.inputHeight * 4);
}

void Engine::dropScenePassGraphs() {
	m_BatchGraphs.eraseIf([](const std::vector<PassKey> &key) { return !key.empty() && key.front().scene != 0; });
}

void Engine::setSceneLookahead(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_scene_lookahead: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (on && !m_ScenePassDev.get()) {
		m_ScenePassDev = DeviceBuffer(sizeof(ScenePassState));  // (DeviceBuffer memory starts zeroed)
		m_ScenePassDyn = PinnedWords(sizeof(ScenePassDyn));
	}
	m_SceneLookahead = on != 0;
}

void Engine::setSceneGroup(int on) {
	if (on != 0 && on != 1) throw std::invalid_argument("ju_set_scene_group: on must be 0 or 1, got " + std::to_string(on));
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (on && !m_SceneGroupDyn.host()) m_SceneGroupDyn = PinnedWords(sizeof(SceneGroupDyn));
	m_SceneGroup = on != 0;
}

void Engine::sceneDetect(int *mode, std::uint32_t *thresholdMilli) const {
	if (mode) *mode = m_Scene.mode();
	if (thresholdMilli) *thresholdMilli = m_Scene.threshold();
}

int Engine::sceneInfo(SceneRecord *out, int count) {
	if (count < 0 || (count > 0 && out == nullptr)) throw std::invalid_argument("ju_get_scene_info: NULL records or a negative count");
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	return m_Scene.records(out, count);
}

// One detector step on the frame m_IO.in holds when the program runs.  Called by submit / submitFrame for every step
// exactly once: the re-run of a frame (runSynchronous) comes through here with m_SceneRerun set and launches nothing.
void Engine::sceneStep() {
	if (m_Scene.mode() == 0 || m_SceneRerun) return;
	const FrameSize fs = frameSize();
	SceneSadLaunch q;
	q.src = m_IO.in;
	q.srcStride = m_IO.inStride;
	q.width = static_cast<int>(fs.inputWidth);
	q.height = static_cast<int>(fs.inputHeight);
	m_Scene.fill(q);
	// (a flow-free model has no recurrent input to clear: JU_SCENE_RESET reports)
	q.resetMode = m_Scene.mode() == 2 && m_Config.recurrent();
	launchSceneSad(q, m_Stream);
	if (q.resetMode) {
		launchSceneClear(&q.state->resetNow, m_State[m_Idx].get(), m_State[m_Idx].bytes(), m_Packed[m_Idx].get(),
		    m_Packed[m_Idx].bytes(), m_Stream);
	}
	m_Scene.advance();
	++m_SceneRuns;
}

}  // namespace ju
