#include "frame_io.h"

#include <cstring>

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
