// Frames at the engine's boundary and the host-side pieces every way in and out shares: the frame descriptors, the one
// row copy, the planes of a YUV frame as the conversion kernels take them, the stage-in of a source frame as BGRX rows,
// the source mask's device copy, and the scaler of the source and output stages.  The arithmetic itself is
// frame_geometry.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "frame_geometry.h"
#include "hip_util.h"
#include "kernels.h"
#include "mask_box.h"

namespace ju {

// Frame descriptor of the boundary (reference core/public/JoshUpscale/core.h:30-38):
// 4 bytes per pixel B,G,R,X; `stride` in bytes, may be negative (bottom-up);
// `ptr` addresses the first logical row.
enum class Location : std::uint8_t { Host = 0, Device = 1, GraphicsResource = 2 };

struct Frame {
	void *ptr;
	Location location;
	std::ptrdiff_t stride;
	std::size_t width;
	std::size_t height;
};

// A frame of ju_process_frame that is not BGRX (include/joshupscale_amd.h, ju_frame): a format of the table in kernels.h
// (PixelFormat: planes, words and sample kinds are described there), its planes each addressing their first logical row,
// strides in bytes of any sign.  Host or device.  An RGB format has no colour space: `colorspace` is ignored.
struct YuvFrame {
	PixelFormat format;
	int colorspace;  // 0 BT.601 limited, 1 BT.601 full, 2 BT.709 limited, 3 BT.709 full
	Location location;
	std::size_t width;
	std::size_t height;
	void *planes[3];
	std::ptrdiff_t strides[3];
};

// One side of a frame call: a BGRX frame (exactly as ju_process takes it) or a YUV one.
struct AnyFrame {
	bool yuv = false;
	Frame bgrx{};
	YuvFrame planes{};
};

inline AnyFrame anyOf(const Frame &f) {
	AnyFrame a;
	a.bgrx = f;
	return a;
}
inline std::vector<AnyFrame> anyOf(const Frame *f, int n) {
	std::vector<AnyFrame> a(static_cast<std::size_t>(n > 0 ? n : 0));
	for (int i = 0; i < n; ++i) a[static_cast<std::size_t>(i)].bgrx = f[i];
	return a;
}
inline Location locationOf(const AnyFrame &f) { return f.yuv ? f.planes.location : f.bgrx.location; }

// The bytes a frame covers, every plane of it, in its address space.  A graphics resource covers none: its `ptr` is a
// handle, not an address.
inline FrameExtent extentOf(const AnyFrame &a) {
	if (a.yuv) {
		const YuvFrame &y = a.planes;
		return frameExtent(formatInfo(y.format), y.width, y.height, y.planes, y.strides, static_cast<int>(y.location));
	}
	if (a.bgrx.location == Location::GraphicsResource) return FrameExtent{};
	return imageExtent(a.bgrx.ptr, a.bgrx.stride, a.bgrx.width, a.bgrx.height, static_cast<int>(a.bgrx.location));
}

// Everything a frame call refuses about a frame that is not BGRX and must be w x h, before anything is launched
// (std::invalid_argument "<who>: <why>"; side: "input" / "output"; size: how the messages call w x h).  The non-BGRX half
// of Engine::checkFrame, which the tiled runtime shares at its own sizes (engine_frames.cpp).
void checkPlanes(const YuvFrame &y, const std::string &side, std::size_t w, std::size_t h, const std::string &size, const char *who);

// THE row copy: `rows` rows of `rowBytes` from `src` to `dst` (each the row lowest in memory and the pitch between rows:
// rowSpan), enqueued on `stream` -- one contiguous copy when both sides are dense, a 2-D copy otherwise.  Pageable host
// memory goes through the HIP runtime's own bounce buffers (engine.h, "Host frames").
void copyRows(void *dst, std::size_t dstPitch, const void *src, std::size_t srcPitch, std::size_t rowBytes, std::size_t rows,
    hipMemcpyKind kind, hipStream_t stream);

// The caller's device planes as a conversion kernel takes them
YuvPlanes callerPlanes(const YuvFrame &f);
// A host frame's planes in the device staging buffer `stage` (stagedLayout: plane after plane, rows padded, in the
// caller's memory order)
YuvPlanes stagedPlanes(const YuvFrame &f, std::uint8_t *stage);
// The pageable copies between a host frame's planes and that staging layout, plane by plane on `stream`
void copyPlanes(const YuvFrame &f, std::uint8_t *stage, bool toDevice, hipStream_t stream);

// A source frame as BGRX rows on the device: the first logical row and the signed stride, as the kernels read them.
struct BgrxRows {
	const std::uint8_t *ptr = nullptr;
	std::ptrdiff_t stride = 0;
};
// Whether stageInBgrx reads `in` where it is: a device BGRX image -- aligned: only on the kernels' 4-byte alignment.
bool readsInPlace(const AnyFrame &in, bool aligned);
// The bytes of the staging layout stageInBgrx needs for `in`: a host frame's planes; 0 for every other frame.
std::size_t hostPlaneBytes(const AnyFrame &in);
// One decode launch on `stream`: the planes of `in` (host planes through `planeStage` first) -> dense BGRX rows at `bgrx`.
void decodePlanes(const YuvFrame &in, std::uint8_t *planeStage, std::uint8_t *bgrx, hipStream_t stream);
// THE stage-in of a source frame: `in`, checked to be width x height, as BGRX rows on the device, enqueued on `stream`.
// A device image is read in place (readsInPlace); any other image is copied to `stage` in its memory order, so a
// bottom-up image stays bottom-up and is read through a negative stride; planes are decoded into `stage` (decodePlanes).
// stage: 4 width height bytes, unused for a frame read in place; planeStage: hostPlaneBytes(in).  Allocates nothing.
BgrxRows stageInBgrx(const AnyFrame &in, std::size_t width, std::size_t height, std::uint8_t *stage, std::uint8_t *planeStage,
    bool aligned, hipStream_t stream);

// The source mask of a runtime (docs/source_stage.md; docs/tiled.md "A mask"): a BGRX image in device memory, in the
// caller's row order -- a bottom-up mask stays bottom-up and is read through a negative stride.  Empty: no mask.
class SourceMask {
public:
	// The copy of `mask` -- host or device memory, its size and pointer already checked by the owner -- made on the null
	// stream and waited for, as a blocking copy is: behind what the caller's own default-stream work wrote.
	// std::invalid_argument "<who>: |stride| smaller than a row" before anything is allocated.  The owner waits for its own
	// stream before it moves the copy into place.
	static SourceMask copyOf(const Frame &mask, const char *who);
	bool on() const { return m_Width != 0; }
	std::size_t width() const { return m_Width; }
	std::size_t height() const { return m_Height; }
	std::ptrdiff_t stride() const { return m_Stride; }  // (negative: bottom-up)
	const std::uint8_t *first() const;                  // texel (0, 0)
	// maskBox of this copy of `from` over a blended frame of outW x outH, from host memory: the caller's own rows, or the
	// copy read back once (set time, not the frame path)
	MaskBox box(const Frame &from, std::size_t outW, std::size_t outH) const;

private:
	DeviceBuffer m_Rows;
	std::size_t m_Width = 0, m_Height = 0;
	std::ptrdiff_t m_Stride = 0;
};

// The scaler of the source and the output stage (source_kernels.hip; docs/source_stage.md, docs/output_stage.md): both
// axes' tables on the device -- one buffer per axis, the start indices, then the taps -- and what the launches need
// beside them.  srcW x srcH -> dstW x dstH through one JU_SCALE_* filter.
class Scaler {
public:
	// Allocates and uploads first and replaces the scaler's state last: a throw leaves it as it was.  (To replace a
	// scaler whose tables enqueued launches may still read, build a new one, synchronise, then move it in.)
	// std::invalid_argument: buildScaleAxis's, for an unknown filter or a ratio outside its bounds.
	void build(std::size_t srcW, std::size_t srcH, std::size_t dstW, std::size_t dstH, int filter);
	void clear() { *this = Scaler(); }
	bool set() const { return m_SrcW != 0; }
	std::size_t srcW() const { return m_SrcW; }
	std::size_t srcH() const { return m_SrcH; }
	std::size_t dstW() const { return m_DstW; }
	std::size_t dstH() const { return m_DstH; }
	int filter() const { return m_Filter; }  // (JU_SCALE_*; 0 while not set)
	// the two axes' device tables and the x axis' scaleSpan, for a launch that scales from another source than rows in
	// memory (the tiled object's fused kernels: launchTileStitchScale / launchTileStitchScaleState)
	const ScaleAxisDev &xAxis() const { return m_XDev; }
	const ScaleAxisDev &yAxis() const { return m_YDev; }
	int span() const { return m_Span; }
	// launchScaleBgrx / launchScaleState (kernels.h) with the scaler's sizes and tables
	void scaleBgrx(const std::uint8_t *src, std::ptrdiff_t srcStride, std::uint8_t *dst, std::ptrdiff_t dstStride,
	    hipStream_t stream) const;
	// launchScaleBgrxItems: `count` frames of the scaler's sizes in one launch
	void scaleBgrxItems(const ScaleItems &items, int count, hipStream_t stream) const;
	void scaleState(const void *state, std::uint16_t *dst, hipStream_t stream) const;
	// this scaler's row of a launchScaleBgrxMembers table: its own source width, tables, tile pitch and form
	ScaleMember member(const std::uint8_t *src, std::ptrdiff_t srcStride, std::uint8_t *dst, std::ptrdiff_t dstStride) const;

private:
	DeviceBuffer m_X, m_Y;
	ScaleAxisDev m_XDev, m_YDev;
	int m_Span = 0, m_Filter = 0;
	std::size_t m_SrcW = 0, m_SrcH = 0, m_DstW = 0, m_DstH = 0;
};

}  // namespace ju
