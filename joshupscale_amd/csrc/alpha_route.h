// Where the alpha slot of a frame's side lies (docs/alpha.md, "Routing" and "Passes"): which formats have a slot and of
// what kind (alphaKind), which of a side's rows hold it (alphaRowsOf: a BGRX side's own rows, else plane 0 of the
// format's planes -- never the decoded BGRX copy), and whether a frame gets a launch (alphaLaunches).  Written once for
// the single-frame route (Engine::alphaSource, Engine::alphaInto), the passes (Engine::bindFrame) and the tiled runtime
// (tiled.cpp).  The location half of the rule is one line, alphaLocated: the routes that stage a frame themselves
// (alphaSource, the tiler) choose through it; bindFrame's sides are already bound by location (bindSide) when it asks.
// Host arithmetic only: nothing here touches the device, and the rows it returns are addresses nothing in this header
// dereferences (tests/cxx/alpha_route.cpp).
#pragma once

#include <cstddef>

#include "kernels.h"

namespace ju {

// the slot of a format: byte 3 of BGRX / RGBX, word 3 of BGRX64, bits 30-31 of the X2 words; kAlphaNone for one without
constexpr int alphaKind(PixelFormat f) {
	switch (f) {
	case PixelFormat::Bgrx:
	case PixelFormat::Rgbx: return kAlphaByte;
	case PixelFormat::Bgrx64: return kAlphaWord;
	case PixelFormat::X2rgb10:
	case PixelFormat::X2bgr10: return kAlphaBits;
	default: return kAlphaNone;
	}
}

// Rows of a side on the device: the first logical row and the signed stride.
struct AlphaSideRows {
	const void *ptr = nullptr;
	std::ptrdiff_t stride = 0;
};

// One side of a frame once it lies on the device.  A BGRX side (`planar` false) IS its BGRX rows: `bgrx`.  Any other
// format has the BGRX rows the network reads or writes (`bgrx`: decoded with X = 0, or not yet encoded -- never the slot)
// and the planes of its own format, of which plane 0 holds the slot if the format has one: `plane0`.
struct AlphaSide {
	bool planar = false;
	PixelFormat format = PixelFormat::Bgrx;
	AlphaSideRows bgrx, plane0;
};

// The kind and the rows of a side, as a source (kAlphaNone: the opaque constant, nothing is read) and as a sink (kAlphaNone:
// nothing is launched and nothing is counted).
inline AlphaRows alphaRowsOf(const AlphaSide &s) {
	if (!s.planar) return AlphaRows{kAlphaByte, const_cast<void *>(s.bgrx.ptr), s.bgrx.stride};
	const int kind = alphaKind(s.format);
	if (kind == kAlphaNone) return AlphaRows{};
	return AlphaRows{kind, const_cast<void *>(s.plane0.ptr), s.plane0.stride};
}

// Where a side lies on the device: a device frame in place (`caller`), anything else -- a host frame, a graphics resource
// -- where its route staged it (`staged`: an upload slot or a staging buffer, addressed with the sign of a bottom-up host
// stride).
inline AlphaSideRows alphaLocated(bool device, const AlphaSideRows &caller, const AlphaSideRows &staged) {
	return device ? caller : staged;
}

// Whether a frame with this sink gets an alpha launch under `mode`
constexpr bool alphaLaunches(int mode, int sinkKind) { return mode != kAlphaZero && sinkKind != kAlphaNone; }

}  // namespace ju
