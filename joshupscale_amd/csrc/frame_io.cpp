#include "frame_io.h"

#include <cstring>
#include <stdexcept>

namespace ju {

void copyRows(void *dst, std::size_t dstPitch, const void *src, std::size_t srcPitch, std::size_t rowBytes, std::size_t rows,
    hipMemcpyKind kind, hipStream_t stream) {
	if (dstPitch == rowBytes && srcPitch == rowBytes) {
		JU_HIP(hipMemcpyAsync(dst, src, rowBytes * rows, kind, stream));
	} else {
		JU_HIP(hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, rowBytes, rows, kind, stream));
	}
}

YuvPlanes callerPlanes(const YuvFrame &f) {
	YuvPlanes pl;
	std::uint8_t **plane[3] = {&pl.y, &pl.u, &pl.v};
	std::ptrdiff_t *stride[3] = {&pl.yStride, &pl.uStride, &pl.vStride};
	for (int k = 0; k < formatInfo(f.format).planes; ++k) {
		*plane[k] = static_cast<std::uint8_t *>(f.planes[k]);
		*stride[k] = f.strides[k];
	}
	return pl;
}

YuvPlanes stagedPlanes(const YuvFrame &f, std::uint8_t *stage) {
	const YuvFormatInfo &info = formatInfo(f.format);
	const StagedLayout l = stagedLayout(info, f.width, f.height, f.strides);
	YuvPlanes pl;
	std::uint8_t **plane[3] = {&pl.y, &pl.u, &pl.v};
	std::ptrdiff_t *stride[3] = {&pl.yStride, &pl.uStride, &pl.vStride};
	for (int k = 0; k < info.planes; ++k) {
		*plane[k] = stage + l.plane[k].first;
		*stride[k] = l.plane[k].pitch;
	}
	return pl;
}

void copyPlanes(const YuvFrame &f, std::uint8_t *stage, bool toDevice, hipStream_t stream) {
	const YuvFormatInfo &info = formatInfo(f.format);
	const StagedLayout l = stagedLayout(info, f.width, f.height, f.strides);
	for (int k = 0; k < info.planes; ++k) {
		const PlaneShape p = planeShape(info, f.width, f.height, k);
		const RowSpan host = rowSpan(f.planes[k], f.strides[k], p.rows);
		std::uint8_t *staged = stage + l.plane[k].begin;
		const std::size_t pitch = stagePitch(p.rowBytes);
		if (toDevice) {
			copyRows(staged, pitch, host.lowest, host.pitch, p.rowBytes, p.rows, hipMemcpyHostToDevice, stream);
		} else {
			copyRows(host.lowest, host.pitch, staged, pitch, p.rowBytes, p.rows, hipMemcpyDeviceToHost, stream);
		}
	}
}

bool readsInPlace(const AnyFrame &in, bool aligned) {
	if (in.yuv || in.bgrx.location != Location::Device) return false;
	return !aligned || (reinterpret_cast<std::uintptr_t>(in.bgrx.ptr) % 4 == 0 && in.bgrx.stride % 4 == 0);
}

std::size_t hostPlaneBytes(const AnyFrame &in) {
	const YuvFrame &y = in.planes;
	if (!in.yuv || y.location == Location::Device) return 0;
	return stagedLayout(formatInfo(y.format), y.width, y.height, y.strides).bytes;
}

void decodePlanes(const YuvFrame &in, std::uint8_t *planeStage, std::uint8_t *bgrx, hipStream_t stream) {
	const bool host = in.location != Location::Device;
	if (host) copyPlanes(in, planeStage, true, stream);
	const YuvPlanes pl = host ? stagedPlanes(in, planeStage) : callerPlanes(in);
	launchDecodeFrame(fmt(in.format), in.colorspace, pl, bgrx, static_cast<std::ptrdiff_t>(in.width * 4), static_cast<int>(in.width),
	    static_cast<int>(in.height), stream);
}

BgrxRows stageInBgrx(const AnyFrame &in, std::size_t width, std::size_t height, std::uint8_t *stage, std::uint8_t *planeStage,
    bool aligned, hipStream_t stream) {
	const std::size_t rowBytes = width * 4;
	const auto plain = static_cast<std::ptrdiff_t>(rowBytes);
	if (in.yuv) {
		decodePlanes(in.planes, planeStage, stage, stream);
		return {stage, plain};
	}
	const Frame &b = in.bgrx;
	if (readsInPlace(in, aligned)) return {static_cast<const std::uint8_t *>(b.ptr), b.stride};
	const RowSpan rows = rowSpan(b.ptr, b.stride, height);
	copyRows(stage, rowBytes, rows.lowest, rows.pitch, rowBytes, height,
	    b.location == Location::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream);
	if (rows.topDown) return {stage, plain};
	return {stage + static_cast<std::ptrdiff_t>(height - 1) * plain, -plain};
}

SourceMask SourceMask::copyOf(const Frame &mask, const char *who) {
	const std::size_t rowBytes = mask.width * 4;
	const auto plain = static_cast<std::ptrdiff_t>(rowBytes);
	if (mask.stride > -plain && mask.stride < plain) throw std::invalid_argument(std::string(who) + ": |stride| smaller than a row");
	SourceMask m;
	m.m_Rows = DeviceBuffer(rowBytes * mask.height);
	const RowSpan rows = rowSpan(mask.ptr, mask.stride, mask.height);
	copyRows(m.m_Rows.get(), rowBytes, rows.lowest, rows.pitch, rowBytes, mask.height,
	    mask.location == Location::Host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, nullptr);
	JU_HIP(hipStreamSynchronize(nullptr));
	m.m_Width = mask.width;
	m.m_Height = mask.height;
	m.m_Stride = rows.topDown ? plain : -plain;
	return m;
}

const std::uint8_t *SourceMask::first() const {
	// (a bottom-up mask: its last row in memory, read with the negative stride)
	return m_Rows.as<std::uint8_t>() + (m_Stride < 0 ? static_cast<std::ptrdiff_t>(m_Height - 1) * -m_Stride : 0);
}

MaskBox SourceMask::box(const Frame &from, std::size_t outW, std::size_t outH) const {
	const int w = static_cast<int>(m_Width), h = static_cast<int>(m_Height), ow = static_cast<int>(outW), oh = static_cast<int>(outH);
	if (from.location == Location::Host) return maskBox(static_cast<const std::uint8_t *>(from.ptr), from.stride, w, h, ow, oh);
	std::vector<std::uint8_t> back(m_Rows.bytes());
	JU_HIP(hipMemcpy(back.data(), m_Rows.get(), back.size(), hipMemcpyDeviceToHost));
	return maskBox(back.data() + (first() - m_Rows.as<std::uint8_t>()), m_Stride, w, h, ow, oh);
}

namespace {
// one device buffer per axis of the scaler: the start indices, then the taps
DeviceBuffer uploadScaleAxis(const ScaleAxisHost &a) {
	const std::size_t startBytes = a.start.size() * sizeof(int), tapBytes = a.taps.size() * sizeof(std::uint16_t);
	std::vector<unsigned char> host(startBytes + tapBytes);
	std::memcpy(host.data(), a.start.data(), startBytes);
	std::memcpy(host.data() + startBytes, a.taps.data(), tapBytes);
	DeviceBuffer buf(host.size());
	buf.upload(host.data(), host.size());
	return buf;
}
ScaleAxisDev scaleAxisDev(const DeviceBuffer &buf, const ScaleAxisHost &a) {
	return {buf.as<int>(), reinterpret_cast<const std::uint16_t *>(buf.as<int>() + a.start.size()), a.filter};
}
}  // namespace

void Scaler::build(std::size_t srcW, std::size_t srcH, std::size_t dstW, std::size_t dstH, int filter) {
	const ScaleAxisHost x = buildScaleAxis(static_cast<int>(srcW), static_cast<int>(dstW), filter);
	const ScaleAxisHost y = buildScaleAxis(static_cast<int>(srcH), static_cast<int>(dstH), filter);
	DeviceBuffer bx = uploadScaleAxis(x), by = uploadScaleAxis(y);
	m_X = std::move(bx);
	m_Y = std::move(by);
	m_XDev = scaleAxisDev(m_X, x);
	m_YDev = scaleAxisDev(m_Y, y);
	m_Span = scaleSpan(x);
	m_Filter = filter;
	m_SrcW = srcW;
	m_SrcH = srcH;
	m_DstW = dstW;
	m_DstH = dstH;
}

void Scaler::scaleBgrx(const std::uint8_t *src, std::ptrdiff_t srcStride, std::uint8_t *dst, std::ptrdiff_t dstStride,
    hipStream_t stream) const {
	launchScaleBgrx(src, srcStride, static_cast<int>(m_SrcW), static_cast<int>(m_SrcH), dst, dstStride, static_cast<int>(m_DstW),
	    static_cast<int>(m_DstH), m_XDev, m_YDev, m_Span, stream);
}

void Scaler::scaleBgrxItems(const ScaleItems &items, int count, hipStream_t stream) const {
	launchScaleBgrxItems(items, count, static_cast<int>(m_SrcW), static_cast<int>(m_SrcH), static_cast<int>(m_DstW),
	    static_cast<int>(m_DstH), m_XDev, m_YDev, m_Span, stream);
}

ScaleMember Scaler::member(const std::uint8_t *src, std::ptrdiff_t srcStride, std::uint8_t *dst, std::ptrdiff_t dstStride) const {
	return scaleMember(src, srcStride, static_cast<int>(m_SrcW), dst, dstStride, m_XDev, m_YDev, m_Span);
}

void Scaler::scaleState(const void *state, std::uint16_t *dst, hipStream_t stream) const {
	launchScaleState(state, static_cast<int>(m_SrcW), static_cast<int>(m_SrcH), dst, static_cast<int>(m_DstW),
	    static_cast<int>(m_DstH), m_XDev, m_YDev, m_Span, stream);
}

}  // namespace ju
