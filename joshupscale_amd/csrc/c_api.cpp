// extern "C" entry points of libJoshUpscale.so (include/joshupscale_amd.h).
// Exceptions never cross this boundary: each call is wrapped, the message is
// kept per thread for ju_last_error().

#include "joshupscale_amd.h"
#ifdef JU_TEST_HOOKS  // libJoshUpscale_test.so only (Makefile): the product library exports none of the hooks
#include "joshupscale_amd_test.h"
#endif

#include <cstdio>
#include <cstring>
#include <fstream>
#include <ios>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.h"
#include "fp8.h"
#include "graphics.h"
#include "log.h"
#include "model.h"
#include "tiled.h"

struct ju_runtime {
	std::unique_ptr<ju::Engine> engine;
};

struct ju_tiled {
	std::unique_ptr<ju::TiledRuntime> tiled;
};

namespace {

thread_local std::string g_LastError;

int fail(int code, const std::string &msg) {
	g_LastError = msg;
	ju::logMessage(ju::LogLevel::Error, "Core", msg);
	return code;
}

template <typename F>
int guarded(F &&f) {
	try {
		f();
		return JU_OK;
	} catch (const ju::HipError &e) {
		return fail(JU_ERR_DEVICE, std::string("HipException: ") + e.what());
	} catch (const std::invalid_argument &e) {
		return fail(JU_ERR_INVALID_ARGUMENT, std::string("std::invalid_argument: ") + e.what());
	} catch (const std::ios_base::failure &e) {
		return fail(JU_ERR_IO, std::string("std::ios_base::failure: ") + e.what());
	} catch (const std::bad_alloc &e) {
		return fail(JU_ERR_INTERNAL, std::string("std::bad_alloc: ") + e.what());
	} catch (const std::runtime_error &e) {
		return fail(JU_ERR_INTERNAL, std::string("std::runtime_error: ") + e.what());
	} catch (const std::exception &e) {
		return fail(JU_ERR_INTERNAL, std::string("std::exception: ") + e.what());
	} catch (...) {
		return fail(JU_ERR_INTERNAL, "unknown exception");
	}
}

}  // namespace

// exception mapping for the other translation units of the C ABI (comm.cpp)
int juGuarded(void (*fn)(void *), void *ctx) {
	return guarded([&] { fn(ctx); });
}

namespace {

ju::Frame toFrame(const ju_image *img) {
	if (img == nullptr) throw std::invalid_argument("image is NULL");
	if (img->location > JU_LOC_GRAPHICS_RESOURCE) {
		throw std::invalid_argument("image has an unknown location");
	}
	return ju::Frame{img->ptr, static_cast<ju::Location>(img->location), img->stride, img->width,
	    img->height};
}

std::vector<ju::Frame> toFrames(const ju_image *images, int count) {
	std::vector<ju::Frame> frames(static_cast<std::size_t>(count));
	for (int i = 0; i < count; ++i) frames[static_cast<std::size_t>(i)] = toFrame(images + i);
	return frames;
}

// A ju_frame as the engine's AnyFrame; BGRX frames exactly as toFrame makes them of a ju_image
ju::AnyFrame toAnyFrame(const ju_frame *f) {
	if (f == nullptr) throw std::invalid_argument("frame is NULL");
	ju::AnyFrame a;
	if (f->format == JU_FMT_BGRX) {
		const ju_image img{f->planes[0], f->location, f->strides[0], f->width, f->height};
		a.bgrx = toFrame(&img);
		return a;
	}
	if (ju::yuvFormatInfo(f->format) == nullptr) throw std::invalid_argument("frame has an unknown format " + std::to_string(f->format));
	if (f->location > JU_LOC_GRAPHICS_RESOURCE) throw std::invalid_argument("frame has an unknown location");
	a.yuv = true;
	a.planes.format = static_cast<ju::PixelFormat>(f->format);
	a.planes.colorspace = f->colorspace;
	a.planes.location = static_cast<ju::Location>(f->location);
	a.planes.width = f->width;
	a.planes.height = f->height;
	for (int k = 0; k < 3; ++k) {
		a.planes.planes[k] = f->planes[k];
		a.planes.strides[k] = f->strides[k];
	}
	return a;
}

ju::Engine &engineOf(ju_runtime *rt) {
	if (rt == nullptr || !rt->engine) throw std::invalid_argument("runtime is NULL");
	return *rt->engine;
}

ju::TiledRuntime &tiledOf(ju_tiled *t) {
	if (t == nullptr || !t->tiled) throw std::invalid_argument("tiled runtime is NULL");
	return *t->tiled;
}

// whole-file read with failbit/badbit exceptions, as core/src/core.cc:156-167
std::vector<char> readModelFile(const char *path) {
	std::ifstream f(path, std::ifstream::in | std::ifstream::binary | std::ifstream::ate);
	if (!f) throw std::ios_base::failure(std::string("cannot open model file ") + path);
	f.exceptions(std::ifstream::badbit | std::ifstream::failbit);
	const auto size = static_cast<std::size_t>(f.tellg());
	std::vector<char> bytes(size);
	f.seekg(0);
	f.read(bytes.data(), static_cast<std::streamsize>(size));
	return bytes;
}

int createFromBytes(int device, const void *bytes, std::size_t size, int dtype, ju_runtime **out) {
	return guarded([&] {
		if (out == nullptr) throw std::invalid_argument("out_runtime is NULL");
		*out = nullptr;
		int count = 0;
		JU_HIP(hipGetDeviceCount(&count));
		if (device < 0 || device >= count) {
			throw std::invalid_argument("device " + std::to_string(device) + " does not exist (" +
			                            std::to_string(count) + " HIP devices visible)");
		}
		ju::DeviceGuard guard(device);  // like cuda::DeviceContext in core/src/core.cc:168
		auto rt = std::make_unique<ju_runtime>();
		rt->engine = std::make_unique<ju::Engine>(device, bytes, size, dtype);
		*out = rt.release();
	});
}

}  // namespace

extern "C" {

int ju_create(int device_id, const char *model_path, ju_runtime **out_runtime) {
	std::vector<char> bytes;
	int rc = guarded([&] {
		if (model_path == nullptr) throw std::invalid_argument("model_path is NULL");
		bytes = readModelFile(model_path);
	});
	if (rc != JU_OK) return rc;
	return createFromBytes(device_id, bytes.data(), bytes.size(), JU_DTYPE_DEFAULT, out_runtime);
}

int ju_create_from_memory(int device_id, const void *model_bytes, size_t model_size, int dtype,
    ju_runtime **out_runtime) {
	return createFromBytes(device_id, model_bytes, model_size, dtype, out_runtime);
}

int ju_validate_model(const void *model_bytes, size_t model_size) {
	return guarded([&] {
		const ju::ModelFile model(model_bytes, model_size);
		(void)ju::foldModel(model);
	});
}

void ju_destroy(ju_runtime *runtime) {
	delete runtime;
}

int ju_process(ju_runtime *runtime, const ju_image *input, const ju_image *output) {
	return guarded([&] { engineOf(runtime).process(ju::anyOf(toFrame(input)), ju::anyOf(toFrame(output))); });
}

int ju_process_batch(ju_runtime *runtime, const ju_image *inputs, const ju_image *outputs, int count) {
	return guarded([&] {
		if (count < 0 || (count > 0 && (inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_process_batch: NULL images or a negative count");
		}
		const std::vector<ju::Frame> in = toFrames(inputs, count), out = toFrames(outputs, count);
		engineOf(runtime).processBatch(in.data(), out.data(), count);
	});
}

int ju_process_group(ju_runtime *const *runtimes, const ju_image *inputs, const ju_image *outputs, int count) {
	return guarded([&] {
		if (count < 0 || (count > 0 && (runtimes == nullptr || inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_process_group: NULL arguments or a negative count");
		}
		std::vector<ju::Engine *> engines(static_cast<std::size_t>(count));
		std::vector<ju::Frame> in(static_cast<std::size_t>(count)), out(static_cast<std::size_t>(count));
		for (int i = 0; i < count; ++i) {
			engines[i] = &engineOf(runtimes[i]);
			in[i] = toFrame(inputs + i);
			out[i] = toFrame(outputs + i);
		}
		ju::Engine::processGroup(engines.data(), in.data(), out.data(), count);
	});
}

int ju_process_group_frames(ju_runtime *const *runtimes, const ju_frame *inputs, const ju_frame *outputs, int count) {
	return guarded([&] {
		if (count < 0 || (count > 0 && (runtimes == nullptr || inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_process_group_frames: NULL arguments or a negative count");
		}
		std::vector<ju::Engine *> engines(static_cast<std::size_t>(count));
		std::vector<ju::AnyFrame> in(static_cast<std::size_t>(count)), out(static_cast<std::size_t>(count));
		for (int i = 0; i < count; ++i) {
			try {
				engines[i] = &engineOf(runtimes[i]);
				in[i] = toAnyFrame(inputs + i);
				out[i] = toAnyFrame(outputs + i);
			} catch (const std::invalid_argument &err) {
				throw std::invalid_argument("ju_process_group_frames: member " + std::to_string(i) + ": " + err.what());
			}
		}
		ju::Engine::processGroupFrames(engines.data(), in.data(), out.data(), count);
	});
}

int ju_prepare_batch(ju_runtime *runtime, const ju_image *inputs, const ju_image *outputs, int count, int *captured) {
	if (captured) *captured = 0;
	return guarded([&] {
		if (count < 0 || (count > 0 && (inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_prepare_batch: NULL images or a negative count");
		}
		const std::vector<ju::Frame> in = toFrames(inputs, count), out = toFrames(outputs, count);
		const int n = engineOf(runtime).prepareBatch(in.data(), out.data(), count);
		if (captured) *captured = n;
	});
}

int ju_set_lookahead(ju_runtime *runtime, int frames) {
	return guarded([&] { engineOf(runtime).setLookahead(frames); });
}

int ju_enqueue(ju_runtime *runtime, const ju_image *input, const ju_image *output) {
	return guarded([&] {
		const ju::Frame in = toFrame(input), out = toFrame(output);
		if (in.location != ju::Location::Device || out.location != ju::Location::Device) {
			throw std::invalid_argument("ju_enqueue needs JU_LOC_DEVICE images");
		}
		engineOf(runtime).enqueue(ju::anyOf(in), ju::anyOf(out));
	});
}

int ju_process_frame(ju_runtime *runtime, const ju_frame *input, const ju_frame *output) {
	return guarded([&] {
		engineOf(runtime).process(toAnyFrame(input), toAnyFrame(output));
	});
}

int ju_process_frames(ju_runtime *runtime, const ju_frame *inputs, const ju_frame *outputs, int count) {
	return guarded([&] {
		if (count < 0 || (count > 0 && (inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_process_frames: NULL frames or a negative count");
		}
		if (count == 0) return;
		ju::Engine &e = engineOf(runtime);
		std::vector<ju::AnyFrame> in(static_cast<std::size_t>(count)), out(static_cast<std::size_t>(count));
		for (int i = 0; i < count; ++i) {
			try {
				in[i] = toAnyFrame(inputs + i);
				out[i] = toAnyFrame(outputs + i);
			} catch (const std::invalid_argument &err) {
				throw std::invalid_argument("ju_process_frames: frame " + std::to_string(i) + ": " + err.what());
			}
		}
		e.processFrames(in.data(), out.data(), count);
	});
}

int ju_enqueue_frame(ju_runtime *runtime, const ju_frame *input, const ju_frame *output) {
	return guarded([&] {
		ju::Engine &e = engineOf(runtime);
		const ju::AnyFrame in = toAnyFrame(input), out = toAnyFrame(output);
		if (ju::locationOf(in) != ju::Location::Device || ju::locationOf(out) != ju::Location::Device) {
			throw std::invalid_argument("ju_enqueue_frame needs device frames");
		}
		e.enqueue(in, out);
	});
}

int ju_prepare_frames(ju_runtime *runtime, const ju_image *input, const ju_image *output, int *captured) {
	if (captured) *captured = 0;
	return guarded([&] {
		const int n = engineOf(runtime).prepareFrames(toFrame(input), toFrame(output));
		if (captured) *captured = n;
	});
}

int ju_synchronize(ju_runtime *runtime) {
	return guarded([&] { engineOf(runtime).synchronize(); });
}

int ju_get_size(const ju_runtime *runtime, size_t *input_width, size_t *input_height,
    size_t *output_width, size_t *output_height) {
	return guarded([&] {
		const ju::FrameSize fs = engineOf(const_cast<ju_runtime *>(runtime)).frameSize();
		if (input_width) *input_width = fs.inputWidth;
		if (input_height) *input_height = fs.inputHeight;
		if (output_width) *output_width = fs.outputWidth;
		if (output_height) *output_height = fs.outputHeight;
	});
}

int ju_set_source_size(ju_runtime *runtime, size_t src_width, size_t src_height, int filter) {
	return guarded([&] { engineOf(runtime).setSourceSize(src_width, src_height, filter); });
}

int ju_get_source_size(const ju_runtime *runtime, size_t *src_width, size_t *src_height) {
	return guarded([&] { engineOf(const_cast<ju_runtime *>(runtime)).sourceSize(src_width, src_height); });
}

int ju_set_source_mask(ju_runtime *runtime, const ju_image *mask) {
	return guarded([&] {
		ju::Engine &e = engineOf(runtime);
		if (mask == nullptr) return e.setSourceMask(nullptr);
		const ju::Frame f = toFrame(mask);
		e.setSourceMask(&f);
	});
}

int ju_set_output_size(ju_runtime *runtime, size_t width, size_t height, int filter) {
	return guarded([&] { engineOf(runtime).setOutputSize(width, height, filter); });
}

int ju_get_output_size(const ju_runtime *runtime, size_t *width, size_t *height) {
	return guarded([&] { engineOf(const_cast<ju_runtime *>(runtime)).outputSize(width, height); });
}

int ju_set_alpha(ju_runtime *runtime, int mode, int filter) {
	return guarded([&] { engineOf(runtime).setAlpha(mode, filter); });
}

int ju_get_alpha(const ju_runtime *runtime, int *mode, int *filter) {
	return guarded([&] { engineOf(const_cast<ju_runtime *>(runtime)).alpha(mode, filter); });
}

int ju_set_alpha_lookahead(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setAlphaLookahead(on); });
}

int ju_set_alpha_group(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setAlphaGroup(on); });
}

int ju_set_scene_detect(ju_runtime *runtime, int mode, uint32_t threshold_milli) {
	return guarded([&] { engineOf(runtime).setSceneDetect(mode, threshold_milli); });
}

int ju_get_scene_detect(const ju_runtime *runtime, int *mode, uint32_t *threshold_milli) {
	return guarded([&] { engineOf(const_cast<ju_runtime *>(runtime)).sceneDetect(mode, threshold_milli); });
}

int ju_get_scene_info(ju_runtime *runtime, ju_scene_info *out, int count, int *written) {
	return guarded([&] {
		static_assert(sizeof(ju_scene_info) == sizeof(ju::SceneRecord), "ju_scene_info is the kernel's record");
		if (written) *written = 0;
		const int n = engineOf(runtime).sceneInfo(reinterpret_cast<ju::SceneRecord *>(out), count);
		if (written) *written = n;
	});
}

int ju_set_scene_lookahead(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setSceneLookahead(on); });
}

int ju_set_scene_group(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setSceneGroup(on); });
}

int ju_set_stage_lookahead(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setStageLookahead(on); });
}

int ju_set_stage_group(ju_runtime *runtime, int on) {
	return guarded([&] { engineOf(runtime).setStageGroup(on); });
}

int ju_reset(ju_runtime *runtime) {
	return guarded([&] { engineOf(runtime).reset(); });
}

// ---- tiled upscaling (tiled.h; docs/tiled.md) ----
int ju_tiled_create_from_memory(int device_id, const void *model_bytes, size_t model_size, int dtype, size_t src_width,
    size_t src_height, int overlap, ju_tiled **out_tiled) {
	return guarded([&] {
		if (out_tiled == nullptr) throw std::invalid_argument("ju_tiled_create: out_tiled is NULL");
		*out_tiled = nullptr;
		if (model_bytes == nullptr) throw std::invalid_argument("ju_tiled_create: model_bytes is NULL");
		int count = 0;
		JU_HIP(hipGetDeviceCount(&count));
		if (device_id < 0 || device_id >= count) {
			throw std::invalid_argument("device " + std::to_string(device_id) + " does not exist (" + std::to_string(count) +
			                            " HIP devices visible)");
		}
		ju::DeviceGuard guard(device_id);
		auto t = std::make_unique<ju_tiled>();
		t->tiled = std::make_unique<ju::TiledRuntime>(device_id, model_bytes, model_size, dtype, src_width, src_height, overlap);
		*out_tiled = t.release();
	});
}

int ju_tiled_create(int device_id, const char *model_path, size_t src_width, size_t src_height, int overlap, ju_tiled **out_tiled) {
	std::vector<char> bytes;
	const int rc = guarded([&] {
		if (out_tiled == nullptr) throw std::invalid_argument("ju_tiled_create: out_tiled is NULL");
		*out_tiled = nullptr;
		if (model_path == nullptr) throw std::invalid_argument("ju_tiled_create: model_path is NULL");
		bytes = readModelFile(model_path);
	});
	if (rc != JU_OK) return rc;
	return ju_tiled_create_from_memory(device_id, bytes.data(), bytes.size(), JU_DTYPE_DEFAULT, src_width, src_height, overlap,
	    out_tiled);
}

void ju_tiled_destroy(ju_tiled *tiled) {
	delete tiled;
}

int ju_tiled_reset(ju_tiled *tiled) {
	return guarded([&] { tiledOf(tiled).reset(); });
}

int ju_tiled_set_deep_from_state(ju_tiled *tiled, int on) {
	return guarded([&] { tiledOf(tiled).setDeepFromState(on); });
}

int ju_tiled_set_output_size(ju_tiled *tiled, size_t width, size_t height, int filter) {
	return guarded([&] { tiledOf(tiled).setOutputSize(width, height, filter); });
}

int ju_tiled_set_source_mask(ju_tiled *tiled, const ju_image *mask) {
	return guarded([&] {
		ju::TiledRuntime &t = tiledOf(tiled);
		if (mask == nullptr) return t.setSourceMask(nullptr);
		const ju::Frame f = toFrame(mask);
		t.setSourceMask(&f);
	});
}

int ju_tiled_get_output_size(const ju_tiled *tiled, size_t *width, size_t *height) {
	return guarded([&] { tiledOf(const_cast<ju_tiled *>(tiled)).outputSize(width, height); });
}

int ju_tiled_set_alpha(ju_tiled *tiled, int mode, int filter) {
	return guarded([&] { tiledOf(tiled).setAlpha(mode, filter); });
}

int ju_tiled_get_alpha(const ju_tiled *tiled, int *mode, int *filter) {
	return guarded([&] { tiledOf(const_cast<ju_tiled *>(tiled)).alpha(mode, filter); });
}

int ju_tiled_process(ju_tiled *tiled, const ju_image *input, const ju_image *output) {
	return guarded([&] {
		ju::TiledRuntime &t = tiledOf(tiled);
		if (input == nullptr || output == nullptr) throw std::invalid_argument("ju_tiled_process: image is NULL");
		t.process(ju::anyOf(toFrame(input)), ju::anyOf(toFrame(output)), "ju_tiled_process");
	});
}

int ju_tiled_process_frame(ju_tiled *tiled, const ju_frame *input, const ju_frame *output) {
	return guarded([&] {
		ju::TiledRuntime &t = tiledOf(tiled);
		if (input == nullptr || output == nullptr) throw std::invalid_argument("ju_tiled_process_frame: frame is NULL");
		t.process(toAnyFrame(input), toAnyFrame(output), "ju_tiled_process_frame");
	});
}

int ju_tiled_process_batch(ju_tiled *tiled, const ju_image *inputs, const ju_image *outputs, int count) {
	return guarded([&] {
		ju::TiledRuntime &t = tiledOf(tiled);
		if (count < 0 || (count > 0 && (inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_tiled_process_batch: NULL images or a negative count");
		}
		std::vector<ju::AnyFrame> in(static_cast<std::size_t>(count)), out(static_cast<std::size_t>(count));
		for (int i = 0; i < count; ++i) {
			try {
				in[i] = ju::anyOf(toFrame(inputs + i));
				out[i] = ju::anyOf(toFrame(outputs + i));
			} catch (const std::invalid_argument &err) {
				throw std::invalid_argument("ju_tiled_process_batch: frame " + std::to_string(i) + ": " + err.what());
			}
		}
		t.processFrames(in.data(), out.data(), count, "ju_tiled_process_batch");
	});
}

int ju_tiled_process_frames(ju_tiled *tiled, const ju_frame *inputs, const ju_frame *outputs, int count) {
	return guarded([&] {
		ju::TiledRuntime &t = tiledOf(tiled);
		if (count < 0 || (count > 0 && (inputs == nullptr || outputs == nullptr))) {
			throw std::invalid_argument("ju_tiled_process_frames: NULL frames or a negative count");
		}
		std::vector<ju::AnyFrame> in(static_cast<std::size_t>(count)), out(static_cast<std::size_t>(count));
		for (int i = 0; i < count; ++i) {
			try {
				in[i] = toAnyFrame(inputs + i);
				out[i] = toAnyFrame(outputs + i);
			} catch (const std::invalid_argument &err) {
				throw std::invalid_argument("ju_tiled_process_frames: frame " + std::to_string(i) + ": " + err.what());
			}
		}
		t.processFrames(in.data(), out.data(), count, "ju_tiled_process_frames");
	});
}

int ju_tiled_set_lookahead(ju_tiled *tiled, int frames) {
	return guarded([&] { tiledOf(tiled).setLookahead(frames); });
}

int ju_tiled_get_info(const ju_tiled *tiled, ju_tiled_info *info) {
	return guarded([&] {
		const ju::TiledRuntime &t = tiledOf(const_cast<ju_tiled *>(tiled));
		if (info == nullptr) throw std::invalid_argument("ju_tiled_get_info: info is NULL");
		*info = ju_tiled_info{t.srcWidth(), t.srcHeight(), 4 * t.srcWidth(), 4 * t.srcHeight(), t.tileWidth(), t.tileHeight(),
		    t.tilesX(), t.tilesY(), t.overlap()};
	});
}

int ju_tiled_get_tile(const ju_tiled *tiled, int index, size_t *x, size_t *y) {
	return guarded([&] { tiledOf(const_cast<ju_tiled *>(tiled)).tile(index, x, y); });
}

int ju_tiled_get_stat(const ju_tiled *tiled, const char *key, double *value) {
	return guarded([&] {
		if (key == nullptr || value == nullptr) throw std::invalid_argument("ju_tiled_get_stat: null argument");
		*value = tiledOf(const_cast<ju_tiled *>(tiled)).stat(key);
	});
}

int ju_tiled_set_scene_detect(ju_tiled *tiled, int mode, uint32_t threshold_milli) {
	return guarded([&] { tiledOf(tiled).setSceneDetect(mode, threshold_milli); });
}

int ju_tiled_get_scene_detect(const ju_tiled *tiled, int *mode, uint32_t *threshold_milli) {
	return guarded([&] { tiledOf(const_cast<ju_tiled *>(tiled)).sceneDetect(mode, threshold_milli); });
}

int ju_tiled_get_scene_info(ju_tiled *tiled, ju_scene_info *out, int count, int *written) {
	return guarded([&] {
		if (written) *written = 0;
		const int n = tiledOf(tiled).sceneInfo(reinterpret_cast<ju::SceneRecord *>(out), count);
		if (written) *written = n;
	});
}

#ifdef JU_TEST_HOOKS
namespace {
// what both tile hooks check before a launch: the layout's limits, the tile count, the frame's rows; then the TileSet
void debugTileSet(const char *who, size_t src_width, size_t src_height, size_t tile_width, size_t tile_height, int overlap,
    void *const *tiles, int count, const void *frame, ptrdiff_t stride, size_t row_pixels, ju::TileSet *out, int *nx, int *ny) {
	const std::string name = who;
	constexpr size_t kMost = 1u << 13;
	if (tile_width < 1 || tile_height < 1 || tile_width > kMost || tile_height > kMost) {
		throw std::invalid_argument(name + ": a tile size outside 1 .. 8192");
	}
	const std::string problem = ju::tileLayoutProblem(src_width, src_height, tile_width, tile_height, overlap);
	if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
	const ju::TileAxis x = ju::tileAxis(static_cast<long>(src_width), static_cast<long>(tile_width), overlap);
	const ju::TileAxis y = ju::tileAxis(static_cast<long>(src_height), static_cast<long>(tile_height), overlap);
	if (tiles == nullptr || frame == nullptr) throw std::invalid_argument(name + ": null buffer");
	if (count != x.tiles() * y.tiles()) {
		throw std::invalid_argument(name + ": the layout has " + std::to_string(x.tiles() * y.tiles()) + " tiles, not " + std::to_string(count));
	}
	const auto row = static_cast<ptrdiff_t>(4 * row_pixels);
	if (stride > -row && stride < row) throw std::invalid_argument(name + ": |stride| smaller than a row");
	for (int k = 0; k < count; ++k) {
		out->ptr[k] = static_cast<std::uint8_t *>(tiles[k]);
		out->x[k] = x.origin[static_cast<size_t>(k % x.tiles())];
		out->y[k] = y.origin[static_cast<size_t>(k / x.tiles())];
	}
	*nx = x.tiles();
	*ny = y.tiles();
}
}  // namespace

int ju_debug_tile_split(const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count) {
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		debugTileSet("ju_debug_tile_split", src_width, src_height, tile_width, tile_height, overlap, tiles, count, src, src_stride,
		    src_width, &set, &nx, &ny);
		ju::launchTileSplit(static_cast<const std::uint8_t *>(src), src_stride, set, count, static_cast<int>(tile_width),
		    static_cast<int>(tile_height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_split_frames(const void *const *srcs, const ptrdiff_t *src_strides, int frames, size_t src_width, size_t src_height,
    size_t tile_width, size_t tile_height, int overlap, void *const *tiles, size_t slot_bytes, int count) {
	return guarded([&] {
		const std::string name = "ju_debug_tile_split_frames";
		if (frames < 1 || frames > ju::kFlowBatchMax) throw std::invalid_argument(name + ": 1 .. 8 frames");
		if (srcs == nullptr || src_strides == nullptr) throw std::invalid_argument(name + ": null buffer");
		int nx = 0, ny = 0;
		ju::TileSet set;
		ju::TileFrames list;
		for (int f = 0; f < frames; ++f) {  // every frame's rows, as ju_debug_tile_split checks its one frame's
			try {
				debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, srcs[f], src_strides[f], src_width,
				    &set, &nx, &ny);
			} catch (const std::invalid_argument &err) {
				throw std::invalid_argument(std::string(err.what()) + " (frame " + std::to_string(f) + ")");
			}
			list.src[f] = static_cast<const std::uint8_t *>(srcs[f]);
			list.stride[f] = static_cast<long long>(src_strides[f]);
		}
		if (slot_bytes % 16 || slot_bytes < 4 * tile_width * tile_height) {
			throw std::invalid_argument(name + ": the slot stride must be a multiple of 16 and hold a tile");
		}
		ju::launchTileSplitFrames(list, frames, set, slot_bytes, count, static_cast<int>(tile_width), static_cast<int>(tile_height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_split_scene(const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count, void *prev, void *state, ju_scene_info *record,
    int has_prev, uint32_t threshold_milli, int reset_mode) {
	return guarded([&] {
		static_assert(sizeof(ju::SceneState) == 40, "the layout include/joshupscale_amd_test.h describes");
		const std::string name = "ju_debug_tile_split_scene";
		int nx = 0, ny = 0;
		ju::TileSet set;
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, src, src_stride, src_width,
		    &set, &nx, &ny);
		if (prev == nullptr || state == nullptr || record == nullptr) throw std::invalid_argument(name + ": null detector buffer");
		if (reinterpret_cast<std::uintptr_t>(src) % 4 || src_stride % 4) {
			throw std::invalid_argument(name + ": the frame's address and stride must be multiples of 4");
		}
		if (reinterpret_cast<std::uintptr_t>(prev) % 4 || reinterpret_cast<std::uintptr_t>(state) % 8) {
			throw std::invalid_argument(name + ": the kept frame must be 4-byte, the state 8-byte aligned");
		}
		if (has_prev != 0 && has_prev != 1 && has_prev != 3) throw std::invalid_argument(name + ": has_prev must be 0, 1 or 3");
		const std::string problem = ju::sceneDetectProblem(reset_mode ? 2 : 1, threshold_milli);
		if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
		for (int k = 0; k < count; ++k) {
			if (set.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(set.ptr[k]) % 16) {
				throw std::invalid_argument(name + ": tile " + std::to_string(k) + " is NULL or not 16-byte aligned");
			}
		}
		const std::vector<int> endX = ju::tileOwnedEnds(ju::tileOrigins(static_cast<long>(src_width), static_cast<long>(tile_width), overlap),
		    static_cast<long>(src_width));
		const std::vector<int> endY = ju::tileOwnedEnds(ju::tileOrigins(static_cast<long>(src_height), static_cast<long>(tile_height), overlap),
		    static_cast<long>(src_height));
		ju::TileOwn own;
		for (int k = 0; k < count; ++k) {
			own.x1[k] = endX[static_cast<size_t>(k % nx)];
			own.y1[k] = endY[static_cast<size_t>(k / nx)];
		}
		ju::PinnedWords ring(sizeof(ju::SceneRecord) * (ju::kSceneRing + 1));
		ju::SceneSadLaunch q;
		q.prev = static_cast<std::uint32_t *>(prev);
		q.state = static_cast<ju::SceneState *>(state);
		q.ring = reinterpret_cast<ju::SceneRecord *>(ring.device());
		q.hasPrev = has_prev;
		q.thresholdMilli = threshold_milli;
		q.resetMode = reset_mode != 0;
		ju::launchTileSplitScene(static_cast<const std::uint8_t *>(src), src_stride, static_cast<int>(src_width), static_cast<int>(src_height),
		    set, own, count, static_cast<int>(tile_width), static_cast<int>(tile_height), q, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		const auto *r = reinterpret_cast<const volatile ju::SceneRecord *>(ring.host());
		record->step = r->step;
		record->sad = r->sad;
		record->score = r->score;
		record->cut = r->cut;
		record->reserved = 0;
	});
}

int ju_debug_scene_clear_tiles(int count, const void *flag, void *const *a, const size_t *a_bytes, void *const *b,
    const size_t *b_bytes) {
	return guarded([&] {
		const std::string name = "ju_debug_scene_clear_tiles";
		if (count < 1 || count > ju::kTileMax) throw std::invalid_argument(name + ": count must be 1 .. 64");
		if (flag == nullptr || a == nullptr || a_bytes == nullptr || b == nullptr || b_bytes == nullptr) {
			throw std::invalid_argument(name + ": NULL flag or array");
		}
		if (reinterpret_cast<std::uintptr_t>(flag) % 4) throw std::invalid_argument(name + ": the flag word must be 4-byte aligned");
		ju::SceneClearItem items[ju::kTileMax];
		for (int i = 0; i < count; ++i) {
			if ((a[i] == nullptr && a_bytes[i] != 0) || (b[i] == nullptr && b_bytes[i] != 0)) {
				throw std::invalid_argument(name + ": tile " + std::to_string(i) + ": null buffer");
			}
			items[i] = ju::SceneClearItem{nullptr, a[i], a_bytes[i], b[i], b_bytes[i]};
		}
		ju::PinnedWords table(sizeof(ju::SceneClearTile) * ju::kTileMax);
		ju::launchSceneClearTiles(static_cast<const unsigned *>(flag), items, count, reinterpret_cast<volatile ju::SceneClearTile *>(table.host()),
		    reinterpret_cast<const ju::SceneClearTile *>(table.device()), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_stitch(void *dst, ptrdiff_t dst_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count) {
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		debugTileSet("ju_debug_tile_stitch", src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst, dst_stride,
		    4 * src_width, &set, &nx, &ny);
		const ju::TileAxis x = ju::tileAxis(static_cast<long>(src_width), static_cast<long>(tile_width), overlap);
		const ju::TileAxis y = ju::tileAxis(static_cast<long>(src_height), static_cast<long>(tile_height), overlap);
		ju::DeviceBuffer xTable(x.table.size() * sizeof(ju::TileAxisEntry)), yTable(y.table.size() * sizeof(ju::TileAxisEntry));
		xTable.upload(x.table.data(), x.table.size() * sizeof(ju::TileAxisEntry));
		yTable.upload(y.table.data(), y.table.size() * sizeof(ju::TileAxisEntry));
		ju::launchTileStitch(static_cast<std::uint8_t *>(dst), dst_stride, static_cast<int>(4 * src_width), static_cast<int>(4 * src_height),
		    set, nx, ny, static_cast<int>(4 * tile_width), xTable.as<unsigned>(), yTable.as<unsigned>(), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_stitch_state(void *dst16, size_t src_width, size_t src_height, size_t tile_width, size_t tile_height, int overlap,
    void *const *tiles, int count) {
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		const std::string name = "ju_debug_tile_stitch_state";
		// (the dense 16-bit frame: rows of 8 bytes per pixel)
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst16,
		    static_cast<ptrdiff_t>(32 * src_width), 4 * src_width, &set, &nx, &ny);
		// what the launcher would refuse, in front of the tables' device memory
		if (reinterpret_cast<std::uintptr_t>(dst16) % 16) throw std::invalid_argument(name + ": the 16-bit frame is not 16-byte aligned");
		for (int k = 0; k < count; ++k) {
			if (set.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(set.ptr[k]) % 16) {
				throw std::invalid_argument(name + ": tile " + std::to_string(k) + " is NULL or not 16-byte aligned");
			}
		}
		const ju::TileAxis x = ju::tileAxis(static_cast<long>(src_width), static_cast<long>(tile_width), overlap);
		const ju::TileAxis y = ju::tileAxis(static_cast<long>(src_height), static_cast<long>(tile_height), overlap);
		ju::DeviceBuffer xTable(x.table.size() * sizeof(ju::TileAxisEntry)), yTable(y.table.size() * sizeof(ju::TileAxisEntry));
		xTable.upload(x.table.data(), x.table.size() * sizeof(ju::TileAxisEntry));
		yTable.upload(y.table.data(), y.table.size() * sizeof(ju::TileAxisEntry));
		ju::launchTileStitchState(static_cast<std::uint16_t *>(dst16), static_cast<int>(4 * src_width), static_cast<int>(4 * src_height),
		    set, nx, ny, static_cast<int>(4 * tile_width), xTable.as<unsigned>(), yTable.as<unsigned>(), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}
namespace {
// What both fused hooks share behind debugTileSet: the output size's limits, the tiles' alignment, the blend's tables and
// the scaler's, all in front of the launch.
struct DebugStitchScale {
	ju::DeviceBuffer xTable, yTable;
	ju::Scaler scale;
};
void debugStitchScale(const std::string &name, size_t dst_width, size_t dst_height, int filter, size_t src_width, size_t src_height,
    size_t tile_width, size_t tile_height, int overlap, const ju::TileSet &set, int count, DebugStitchScale *out) {
	const std::string problem = ju::tiledOutputSizeProblem(dst_width, dst_height, src_width, src_height, filter);
	if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
	for (int k = 0; k < count; ++k) {
		if (set.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(set.ptr[k]) % 16) {
			throw std::invalid_argument(name + ": tile " + std::to_string(k) + " is NULL or not 16-byte aligned");
		}
	}
	const ju::TileAxis x = ju::tileAxis(static_cast<long>(src_width), static_cast<long>(tile_width), overlap);
	const ju::TileAxis y = ju::tileAxis(static_cast<long>(src_height), static_cast<long>(tile_height), overlap);
	out->xTable = ju::DeviceBuffer(x.table.size() * sizeof(ju::TileAxisEntry));
	out->yTable = ju::DeviceBuffer(y.table.size() * sizeof(ju::TileAxisEntry));
	out->xTable.upload(x.table.data(), x.table.size() * sizeof(ju::TileAxisEntry));
	out->yTable.upload(y.table.data(), y.table.size() * sizeof(ju::TileAxisEntry));
	out->scale.build(4 * src_width, 4 * src_height, dst_width, dst_height, filter);
}
}  // namespace

int ju_debug_tile_stitch_scale(void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, int filter, size_t src_width,
    size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count) {
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		const std::string name = "ju_debug_tile_stitch_scale";
		// (the layout's refusals, then |stride| against a row of the OUTPUT size)
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst, dst_stride, dst_width, &set,
		    &nx, &ny);
		DebugStitchScale d;
		debugStitchScale(name, dst_width, dst_height, filter, src_width, src_height, tile_width, tile_height, overlap, set, count, &d);
		ju::launchTileStitchScale(static_cast<std::uint8_t *>(dst), dst_stride, static_cast<int>(dst_width), static_cast<int>(dst_height),
		    static_cast<int>(4 * src_width), static_cast<int>(4 * src_height), set, nx, ny, static_cast<int>(4 * tile_width),
		    d.xTable.as<unsigned>(), d.yTable.as<unsigned>(), d.scale.xAxis(), d.scale.yAxis(), d.scale.span(), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_stitch_scale_state(void *dst16, size_t dst_width, size_t dst_height, int filter, size_t src_width, size_t src_height,
    size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count) {
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		const std::string name = "ju_debug_tile_stitch_scale_state";
		// (the dense 16-bit frame: rows of 8 bytes per pixel)
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst16,
		    static_cast<ptrdiff_t>(8 * dst_width), 2 * dst_width, &set, &nx, &ny);
		if (reinterpret_cast<std::uintptr_t>(dst16) % 8) throw std::invalid_argument(name + ": the 16-bit frame is not 8-byte aligned");
		DebugStitchScale d;
		debugStitchScale(name, dst_width, dst_height, filter, src_width, src_height, tile_width, tile_height, overlap, set, count, &d);
		ju::launchTileStitchScaleState(static_cast<std::uint16_t *>(dst16), static_cast<int>(dst_width), static_cast<int>(dst_height),
		    static_cast<int>(4 * src_width), static_cast<int>(4 * src_height), set, nx, ny, static_cast<int>(4 * tile_width),
		    d.xTable.as<unsigned>(), d.yTable.as<unsigned>(), d.scale.xAxis(), d.scale.yAxis(), d.scale.span(), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}
#endif  // JU_TEST_HOOKS

const char *ju_last_error(void) {
	return g_LastError.c_str();
}

void ju_set_log_callback(ju_log_callback callback, void *user) {
	ju::setLogCallback(callback, user);
}

int ju_get_gl_device_index(int *out_device) {
	if (out_device) *out_device = -1;
	return guarded([&] {
		if (out_device == nullptr) throw std::invalid_argument("out_device is NULL");
		*out_device = ju::graphicsBackend().deviceIndex();
	});
}

int ju_get_gl_image(uint32_t gl_texture, int type, ju_image *out_image) {
	if (out_image) *out_image = ju_image{};
	return guarded([&] {
		if (out_image == nullptr) throw std::invalid_argument("out_image is NULL");
		if (type != 0 && type != 1) throw std::invalid_argument("image type must be 0 (input) or 1 (output)");
		ju::GraphicsBackend &backend = ju::graphicsBackend();
		std::size_t w = 0, h = 0;
		void *res = backend.registerImage(gl_texture, type, &w, &h);
		out_image->ptr = new ju::GraphicsHandle{&backend, res};
		out_image->location = JU_LOC_GRAPHICS_RESOURCE;
		out_image->stride = 0;
		out_image->width = w;
		out_image->height = h;
	});
}

void ju_release_gl_image(ju_image *image) {
	if (image == nullptr || image->location != JU_LOC_GRAPHICS_RESOURCE || image->ptr == nullptr) return;
	auto *h = static_cast<ju::GraphicsHandle *>(image->ptr);
	try {
		h->backend->unregisterImage(h->resource);
	} catch (...) {
	}
	delete h;
	image->ptr = nullptr;
}

#ifdef JU_TEST_HOOKS
int ju_debug_fake_gl_texture(uint32_t gl_texture, void *device_ptr, size_t pitch, size_t width, size_t height,
    int bytes_per_pixel) {
	return guarded([&] {
		if (device_ptr == nullptr) {
			ju::fakeGraphicsReset();
			return;
		}
		ju::fakeGraphicsDefineTexture(gl_texture, device_ptr, pitch, width, height, bytes_per_pixel);
	});
}

void ju_debug_fake_gl_counters(int *registered, int *mapped, int *maps, int *unmaps) {
	ju::fakeGraphicsCounters(registered, mapped, maps, unmaps);
}
#endif  // JU_TEST_HOOKS

int ju_get_dtype(const ju_runtime *runtime) {
	if (runtime == nullptr || !runtime->engine) return -1;
	return runtime->engine->reportedDtype();
}

#ifdef JU_TEST_HOOKS
int ju_read_tensor(ju_runtime *runtime, const char *name, float *dst, size_t capacity,
    size_t *count) {
	return guarded([&] {
		if (name == nullptr) throw std::invalid_argument("name is NULL");
		const std::size_t n = engineOf(runtime).readTensor(name, dst, capacity);
		if (count) *count = n;
	});
}

int ju_plan_report(ju_runtime *runtime, char *dst, size_t capacity, size_t *length) {
	return guarded([&] {
		const std::string text = engineOf(runtime).planReport();
		if (length) *length = text.size();
		if (dst == nullptr) return;
		if (capacity < text.size() + 1) throw std::invalid_argument("ju_plan_report: buffer too small");
		std::memcpy(dst, text.c_str(), text.size() + 1);
	});
}

int ju_time_steps(ju_runtime *runtime, const char *tag, int iters, double *ms_per_launch,
    int *launches, double *flops) {
	return guarded([&] {
		const std::string t = tag ? tag : "";
		ju::Engine &e = engineOf(runtime);
		const double ms = e.timeSteps(t, iters, launches);
		if (ms_per_launch) *ms_per_launch = ms;
		if (flops) *flops = e.flopsOf(t);
	});
}
#endif  // JU_TEST_HOOKS

int ju_get_stat(const ju_runtime *runtime, const char *key, double *value) {
	return guarded([&] {
		if (key == nullptr || value == nullptr) throw std::invalid_argument("ju_get_stat: null argument");
#ifndef JU_TEST_HOOKS  // a counter of the test flavour (joshupscale_amd_test.h, "step_rerun")
		if (std::strcmp(key, "scene_detector_runs") == 0) throw std::invalid_argument("unknown stat scene_detector_runs");
#endif
		*value = engineOf(const_cast<ju_runtime *>(runtime)).stat(key);
	});
}

#ifdef JU_TEST_HOOKS
int ju_debug_set(const char *key, int value) {
	return guarded([&] {
		const std::string k = key ? key : "";
		if (k == "tower_variant") ju::setTowerVariant(value);
		else if (k == "resident_fault") ju::setResidentFault(value);
		else if (k == "tower_fast") ju::setResidentTowerFast(value);
		else if (k == "tower_unit_rows") ju::setResidentTowerUnitRows(value);
		else if (k == "res_block_plain") ju::setResBlockPlain(value);
		else if (k == "fp8_block_form") ju::setFp8BlockForm(value);
		else if (k == "pass_rerun") ju::setPassRerun(value);
		else if (k == "step_rerun") ju::setStepRerun(value);
		else if (k == "group_rerun") ju::setGroupRerun(value);
		else throw std::invalid_argument("unknown debug key " + k);
	});
}

namespace {
// What the single-kernel conversion hooks and ju_debug_yuv_items share.  A hook = its name, the formats of the table it
// admits (`family`: how its refusal of another calls them) and its ops: 0 decode planes -> BGRX `image`, 1 encode the BGRX
// `image` -> planes and, where ops >= 3, 2 encode the dense f16 tensor `image` -> planes, the deep formats only; where
// ops == 4, 3 encode the dense u16 frame `image` (launchEncodeFrame16) -> planes.
struct ConversionHook {
	const char *name, *family;
	bool (*admits)(const ju::YuvFormatInfo &);
	int ops;
	bool rowStrides;  // refuse strides smaller than a row
	[[noreturn]] void refuse(const std::string &why) const { throw std::invalid_argument(std::string(name) + ": " + why); }

	const ju::YuvFormatInfo &format(int value) const {
		const ju::YuvFormatInfo *info = ju::yuvFormatInfo(value);
		if (info == nullptr || !admits(*info)) refuse(std::string("not ") + family + " format");
		return *info;
	}
	// Everything a hook refuses about one frame before a launch, in the order size, null, alignment; then its planes
	ju::YuvPlanes planes(const ju::YuvFormatInfo &info, int op, size_t width, size_t height, const void *image,
	    ptrdiff_t image_stride, void *const *planes, const ptrdiff_t *strides) const {
		if (op == 2 && !info.deep()) refuse("op 2 takes the deep formats only (10-bit YUV; RGB of more than 8 bits)");
		if (width == 0 || height == 0 || width > (1u << 15) || height > (1u << 15) ||
		    (info.sampling == 420 && height % 2) || ((info.sampling == 420 || info.sampling == 422) && width % 2)) {
			refuse("sizes 1 .. 32768, an even width for 4:2:0 and 4:2:2, an even height for 4:2:0");
		}
		if (image == nullptr || planes == nullptr || strides == nullptr) refuse("null buffer");
		const auto row = static_cast<ptrdiff_t>(info.planes == 1 ? ju::planeShape(info, width, height, 0).rowBytes : info.sampleBytes * width);
		for (int k = 0; k < info.planes; ++k) {
			if (planes[k] == nullptr) refuse("null buffer");
			if (reinterpret_cast<std::uintptr_t>(planes[k]) % info.sampleBytes || strides[k] % info.sampleBytes) {
				refuse(info.sampleBytes == 2 ? "16-bit planes need even addresses and strides"
				                             : "32-bit planes need addresses and strides that are multiples of 4");
			}
			if (rowStrides && strides[k] > -row && strides[k] < row) refuse("|stride| smaller than a row");
		}
		const auto imageRow = static_cast<ptrdiff_t>(4 * width);
		if (rowStrides && op < 2 && image_stride > -imageRow && image_stride < imageRow) {
			refuse("|image_stride| smaller than a row");
		}
		if (op == 2 && reinterpret_cast<std::uintptr_t>(image) % 16) refuse("the f16 tensor must be 16-byte aligned");
		if (op == 3 && reinterpret_cast<std::uintptr_t>(image) % 8) refuse("the u16 frame must be 8-byte aligned");
		ju::YuvPlanes p;
		std::uint8_t **plane[3] = {&p.y, &p.u, &p.v};
		std::ptrdiff_t *stride[3] = {&p.yStride, &p.uStride, &p.vStride};
		for (int k = 0; k < info.planes; ++k) {
			*plane[k] = static_cast<std::uint8_t *>(planes[k]);
			*stride[k] = strides[k];
		}
		return p;
	}
	int run(int op, int format, int colorspace, size_t width, size_t height, void *image, ptrdiff_t image_stride,
	    void *const *planes, const ptrdiff_t *strides) const {
		return guarded([&] {
			if (op < 0 || op >= ops) refuse(ops == 2 ? "direction must be 0 or 1" : (ops == 3 ? "op must be 0, 1 or 2" : "op must be 0 .. 3"));
			const ju::YuvPlanes p = this->planes(this->format(format), op, width, height, image, image_stride, planes, strides);
			const int w = static_cast<int>(width), h = static_cast<int>(height);
			if (op == 0) {
				ju::launchDecodeFrame(format, colorspace, p, static_cast<std::uint8_t *>(image), image_stride, w, h, nullptr);
			} else if (op == 1) {
				ju::launchEncodeFrame(format, colorspace, static_cast<const std::uint8_t *>(image), image_stride, p, w, h, nullptr);
			} else if (op == 2) {
				ju::launchEncodeState(format, colorspace, image, p, w, h, nullptr);
			} else {
				ju::launchEncodeFrame16(format, colorspace, static_cast<const std::uint16_t *>(image), p, w, h, nullptr);
			}
			JU_HIP(hipStreamSynchronize(nullptr));
		});
	}
};
using Info = const ju::YuvFormatInfo &;
const ConversionHook kDebugYuv{"ju_debug_yuv", "a YUV", [](Info f) { return f.sampling == 420 && !f.deep(); }, 2, false};
const ConversionHook kDebugYuv10{"ju_debug_yuv10", "a 10-bit", [](Info f) { return f.sampling == 420 && f.deep(); }, 3, false};
// (the packed 10-bit formats -- one plane of 10-bit samples -- have a hook of their own; the two before it keep their families)
constexpr bool packed10(Info f) { return f.planes == 1 && f.bits == 10; }
const ConversionHook kDebugYuvSampled{"ju_debug_yuv_sampled", "a 4:2:2 / 4:4:4",
    [](Info f) { return (f.sampling == 422 || f.sampling == 444) && !packed10(f); }, 3, false};
const ConversionHook kDebugRgb{"ju_debug_rgb", "an RGB", [](Info f) { return f.rgb() && !packed10(f); }, 3, true};
const ConversionHook kDebugPacked10{"ju_debug_packed10", "a packed 10-bit", [](Info f) { return packed10(f); }, 4, true};
const ConversionHook kDebugYuvItems{"ju_debug_yuv_items", "a YUV", [](Info) { return true; }, 1, false};
}  // namespace

int ju_debug_yuv(int direction, int format, int colorspace, size_t width, size_t height, void *bgrx,
    ptrdiff_t bgrx_stride, void *const planes[3], const ptrdiff_t strides[3]) {
	return kDebugYuv.run(direction, format, colorspace, width, height, bgrx, bgrx_stride, planes, strides);
}

int ju_debug_yuv10(int op, int format, int colorspace, size_t width, size_t height, void *image, ptrdiff_t image_stride,
    void *const planes[3], const ptrdiff_t strides[3]) {
	return kDebugYuv10.run(op, format, colorspace, width, height, image, image_stride, planes, strides);
}

int ju_debug_yuv_sampled(int op, int format, int colorspace, size_t width, size_t height, void *image,
    ptrdiff_t image_stride, void *const planes[3], const ptrdiff_t strides[3]) {
	return kDebugYuvSampled.run(op, format, colorspace, width, height, image, image_stride, planes, strides);
}

int ju_debug_rgb(int op, int format, size_t width, size_t height, void *image, ptrdiff_t image_stride,
    void *const planes[3], const ptrdiff_t strides[3]) {
	return kDebugRgb.run(op, format, 0, width, height, image, image_stride, planes, strides);
}

int ju_debug_packed10(int op, int format, int colorspace, size_t width, size_t height, void *image, ptrdiff_t image_stride,
    void *const planes[3], const ptrdiff_t strides[3]) {
	return kDebugPacked10.run(op, format, colorspace, width, height, image, image_stride, planes, strides);
}

int ju_debug_yuv_items(int count, const int *formats, const int *colorspaces, size_t width, size_t height,
    void *const *bgrx, const ptrdiff_t *bgrx_strides, void *const *planes, const ptrdiff_t *strides) {
	return guarded([&] {
		const ConversionHook &hook = kDebugYuvItems;
		if (count < 1 || count > ju::kFlowBatchMax) hook.refuse("1 .. 8 items");
		if (!formats || !colorspaces || !bgrx || !bgrx_strides || !planes || !strides) hook.refuse("null argument");
		for (int i = 0; i < count; ++i) hook.format(formats[i]);  // (every format before any buffer)
		ju::YuvDecodeItems items{};
		for (int i = 0; i < count; ++i) {
			const ju::YuvPlanes p = hook.planes(hook.format(formats[i]), 0, width, height, bgrx[i], bgrx_strides[i],
			    planes + 3 * i, strides + 3 * i);
			items.item[i] = ju::yuvDecodeItem(formats[i], colorspaces[i], p, static_cast<std::uint8_t *>(bgrx[i]), bgrx_strides[i]);
		}
		ju::launchYuv420ToBgrxItems(items, count, static_cast<int>(width), static_cast<int>(height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_yuv_items_sized(int count, const int *formats, const int *colorspaces, const size_t *widths, const size_t *heights,
    void *const *bgrx, const ptrdiff_t *bgrx_strides, void *const *planes, const ptrdiff_t *strides) {
	return guarded([&] {
		const ConversionHook hook{"ju_debug_yuv_items_sized", "a YUV", [](Info) { return true; }, 1, false};
		if (count < 1 || count > ju::kFlowBatchMax) hook.refuse("1 .. 8 items");
		if (!formats || !colorspaces || !widths || !heights || !bgrx || !bgrx_strides || !planes || !strides) hook.refuse("null argument");
		for (int i = 0; i < count; ++i) hook.format(formats[i]);  // (every format before any buffer)
		ju::YuvDecodeSizedItems items{};
		for (int i = 0; i < count; ++i) {
			const ju::YuvPlanes p = hook.planes(hook.format(formats[i]), 0, widths[i], heights[i], bgrx[i], bgrx_strides[i],
			    planes + 3 * i, strides + 3 * i);
			items.item[i] = ju::yuvDecodeItem(formats[i], colorspaces[i], p, static_cast<std::uint8_t *>(bgrx[i]), bgrx_strides[i]);
			items.width[i] = static_cast<int>(widths[i]);
			items.height[i] = static_cast<int>(heights[i]);
		}
		ju::launchYuvToBgrxItemsSized(items, count, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_source(int op, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, const void *src,
    ptrdiff_t src_stride, size_t src_width, size_t src_height, const void *mask, ptrdiff_t mask_stride, size_t mask_width,
    size_t mask_height) {
	return guarded([&] {
		if (op == 2) {  // the limits of ju_set_source_size alone: no device
			const std::string problem = ju::sourceSizeProblem(src_width, src_height, dst_width, dst_height);
			if (!problem.empty()) throw std::invalid_argument("ju_set_source_size: " + problem);
			return;
		}
		if (op != 0 && op != 1) throw std::invalid_argument("ju_debug_source: op must be 0, 1 or 2");
		constexpr size_t kMost = 1u << 15;
		if (dst == nullptr || src == nullptr || dst_width < 1 || dst_height < 1 || src_width < 1 || src_height < 1 ||
		    dst_width > kMost || dst_height > kMost || src_width > kMost || src_height > kMost) {
			throw std::invalid_argument("ju_debug_source: null buffer or a size outside 1 .. 32768");
		}
		const int dw = static_cast<int>(dst_width), dh = static_cast<int>(dst_height);
		const int sw = static_cast<int>(src_width), sh = static_cast<int>(src_height);
		if (op == 0) {
			ju::Scaler scale;
			scale.build(src_width, src_height, dst_width, dst_height, ju::kScaleTriangle);
			scale.scaleBgrx(static_cast<const std::uint8_t *>(src), src_stride, static_cast<std::uint8_t *>(dst), dst_stride, nullptr);
			JU_HIP(hipStreamSynchronize(nullptr));
			return;
		}
		if (mask == nullptr || mask_width < 1 || mask_height < 1 || mask_width > kMost || mask_height > kMost) {
			throw std::invalid_argument("ju_debug_source: null mask or a mask size outside 1 .. 32768");
		}
		ju::launchMaskBlend(static_cast<std::uint8_t *>(dst), dst_stride, dw, dh, static_cast<const std::uint8_t *>(src),
		    src_stride, sw, sh, static_cast<const std::uint8_t *>(mask), mask_stride, static_cast<int>(mask_width),
		    static_cast<int>(mask_height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_output(int op, void *dst, size_t dst_width, size_t dst_height, const void *src, size_t src_width,
    size_t src_height, int format, int colorspace, void *const planes[3], const ptrdiff_t strides[3]) {
	return guarded([&] {
		if (op == 2) {  // the limits of ju_set_output_size alone: no device
			const std::string problem = ju::outputSizeProblem(dst_width, dst_height, src_width, src_height, format);
			if (!problem.empty()) throw std::invalid_argument("ju_set_output_size: " + problem);
			return;
		}
		if (op != 0 && op != 1) throw std::invalid_argument("ju_debug_output: op must be 0, 1 or 2");
		constexpr size_t kMost = 1u << 15;
		if (src == nullptr || dst_width < 1 || dst_height < 1 || dst_width > kMost || dst_height > kMost) {
			throw std::invalid_argument("ju_debug_output: null buffer or a size outside 1 .. 32768");
		}
		const int dw = static_cast<int>(dst_width), dh = static_cast<int>(dst_height);
		if (op == 0) {
			if (dst == nullptr || src_width < 1 || src_height < 1 || src_width > kMost || src_height > kMost) {
				throw std::invalid_argument("ju_debug_output: null buffer or a size outside 1 .. 32768");
			}
			ju::Scaler scale;
			scale.build(src_width, src_height, dst_width, dst_height, ju::kScaleTriangle);
			scale.scaleState(src, static_cast<std::uint16_t *>(dst), nullptr);
			JU_HIP(hipStreamSynchronize(nullptr));
			return;
		}
		const ju::YuvFormatInfo *info = ju::yuvFormatInfo(format);
		if (info == nullptr || !info->deep()) {
			throw std::invalid_argument("ju_debug_output: op 1 takes the deep formats only (10-bit YUV; RGB of more than 8 bits)");
		}
		if (reinterpret_cast<std::uintptr_t>(src) % 8) throw std::invalid_argument("ju_debug_output: the u16 frame must be 8-byte aligned");
		const ConversionHook hook{"ju_debug_output", "a deep", [](Info f) { return f.deep(); }, 2, false};
		// (op 1 of the hook's checks: sizes, parity, null planes, sample alignment)
		const ju::YuvPlanes p = hook.planes(*info, 1, dst_width, dst_height, src, static_cast<ptrdiff_t>(8 * dst_width), planes, strides);
		for (int k = 0; k < info->planes; ++k) {  // strides of at least the plane's own row: a chroma row may be half a luma row
			const auto row = static_cast<ptrdiff_t>(ju::planeShape(*info, dst_width, dst_height, k).rowBytes);
			if (strides[k] > -row && strides[k] < row) hook.refuse("|stride| smaller than a row");
		}
		ju::launchEncodeFrame16(format, colorspace, static_cast<const std::uint16_t *>(src), p, dw, dh, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_scale(int op, int filter, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, const void *src,
    ptrdiff_t src_stride, size_t src_width, size_t src_height, int *start, int *count, int16_t *taps) {
	return guarded([&] {
		if (op == 2 || op == 3) {  // the limits of ju_set_source_size / ju_set_output_size for a filter: no device
			const std::string problem = op == 2 ? ju::sourceSizeProblem(src_width, src_height, dst_width, dst_height, filter)
			                                    : ju::outputSizeProblem(dst_width, dst_height, src_width, src_height, filter);
			if (!problem.empty()) {
				throw std::invalid_argument(std::string(op == 2 ? "ju_set_source_size: " : "ju_set_output_size: ") + problem);
			}
			return;
		}
		if (op == 4) {  // one axis' table, src_width -> dst_width: no device
			constexpr size_t kMost = 1u << 15;
			if (start == nullptr || count == nullptr || taps == nullptr || src_width < 1 || dst_width < 1 || src_width > kMost ||
			    dst_width > kMost) {
				throw std::invalid_argument("ju_debug_scale: null array or an extent outside 1 .. 32768");
			}
			const ju::ScaleAxisHost a = ju::buildScaleAxis(static_cast<int>(src_width), static_cast<int>(dst_width), filter);
			for (size_t d = 0; d < dst_width; ++d) {
				const std::uint16_t *row = a.taps.data() + d * ju::kScaleTapPitch;
				start[d] = a.start[d];
				count[d] = row[ju::kScaleMaxTaps];
				for (int t = 0; t < ju::kScaleMaxTaps; ++t) taps[d * ju::kScaleMaxTaps + t] = static_cast<int16_t>(row[t]);
			}
			return;
		}
		if (op != 0 && op != 1) throw std::invalid_argument("ju_debug_scale: op must be 0 .. 4");
		constexpr size_t kMost = 1u << 15;
		if (dst == nullptr || src == nullptr || dst_width < 1 || dst_height < 1 || src_width < 1 || src_height < 1 ||
		    dst_width > kMost || dst_height > kMost || src_width > kMost || src_height > kMost) {
			throw std::invalid_argument("ju_debug_scale: null buffer or a size outside 1 .. 32768");
		}
		ju::Scaler scale;
		scale.build(src_width, src_height, dst_width, dst_height, filter);
		if (op == 0) {
			scale.scaleBgrx(static_cast<const std::uint8_t *>(src), src_stride, static_cast<std::uint8_t *>(dst), dst_stride, nullptr);
		} else {
			scale.scaleState(src, static_cast<std::uint16_t *>(dst), nullptr);
		}
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_alpha_scale(int source_kind, int sink_kind, int filter, void *dst, ptrdiff_t dst_stride, size_t dst_width,
    size_t dst_height, const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height) {
	return guarded([&] {
		constexpr size_t kMost = 1u << 15;
		if (dst_width < 1 || dst_height < 1 || src_width < 1 || src_height < 1 || dst_width > kMost || dst_height > kMost ||
		    src_width > kMost || src_height > kMost) {
			throw std::invalid_argument("ju_debug_alpha_scale: a size outside 1 .. 32768");
		}
		ju::Scaler scale;
		scale.build(src_width, src_height, dst_width, dst_height, filter);
		ju::launchAlphaScale(ju::AlphaRows{source_kind, const_cast<void *>(src), src_stride}, static_cast<int>(src_width),
		    static_cast<int>(src_height), ju::AlphaRows{sink_kind, dst, dst_stride}, static_cast<int>(dst_width),
		    static_cast<int>(dst_height), scale.xAxis(), scale.yAxis(), scale.span(), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_alpha_fill(int sink_kind, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height) {
	return guarded([&] {
		constexpr size_t kMost = 1u << 15;
		if (dst_width < 1 || dst_height < 1 || dst_width > kMost || dst_height > kMost) {
			throw std::invalid_argument("ju_debug_alpha_fill: a size outside 1 .. 32768");
		}
		ju::launchAlphaFill(ju::AlphaRows{sink_kind, dst, dst_stride}, static_cast<int>(dst_width), static_cast<int>(dst_height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tiled_alpha_problem(int mode, int filter, size_t src_width, size_t src_height, size_t out_width, size_t out_height) {
	return guarded([&] {
		const std::string problem = ju::tiledAlphaProblem(mode, filter, src_width, src_height, out_width, out_height);
		if (!problem.empty()) throw std::invalid_argument("ju_tiled_set_alpha: " + problem);
	});
}

int ju_debug_alpha_problem(int mode, int filter, size_t in_width, size_t in_height, size_t out_width, size_t out_height) {
	return guarded([&] {
		const std::string problem = ju::alphaProblem(mode, filter, in_width, in_height, out_width, out_height);
		if (!problem.empty()) throw std::invalid_argument("ju_set_alpha: " + problem);
	});
}

int ju_debug_scale_items(int count, int filter, void *const *dst, const ptrdiff_t *dst_strides, size_t dst_width,
    size_t dst_height, const void *const *src, const ptrdiff_t *src_strides, size_t src_width, size_t src_height) {
	return guarded([&] {
		if (count < 1 || count > ju::kFlowBatchMax) throw std::invalid_argument("ju_debug_scale_items: count must be 1 .. 8");
		if (dst == nullptr || dst_strides == nullptr || src == nullptr || src_strides == nullptr) {
			throw std::invalid_argument("ju_debug_scale_items: NULL array");
		}
		constexpr size_t kMost = 1u << 15;
		if (dst_width < 1 || dst_height < 1 || src_width < 1 || src_height < 1 || dst_width > kMost || dst_height > kMost ||
		    src_width > kMost || src_height > kMost) {
			throw std::invalid_argument("ju_debug_scale_items: a size outside 1 .. 32768");
		}
		ju::ScaleItems items{};
		for (int i = 0; i < count; ++i) {
			if (dst[i] == nullptr || src[i] == nullptr) throw std::invalid_argument("ju_debug_scale_items: NULL buffer");
			items.item[i] = ju::ScaleItem{static_cast<const std::uint8_t *>(src[i]), src_strides[i], static_cast<std::uint8_t *>(dst[i]),
			    dst_strides[i]};
		}
		ju::Scaler scale;
		scale.build(src_width, src_height, dst_width, dst_height, filter);
		scale.scaleBgrxItems(items, count, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_scale_members(int count, const int *filters, void *const *dst, const ptrdiff_t *dst_strides, size_t dst_width,
    size_t dst_height, const void *const *src, const ptrdiff_t *src_strides, const size_t *src_widths, const size_t *src_heights) {
	return guarded([&] {
		if (count < 1 || count > ju::kFlowBatchMax) throw std::invalid_argument("ju_debug_scale_members: count must be 1 .. 8");
		if (filters == nullptr || dst == nullptr || dst_strides == nullptr || src == nullptr || src_strides == nullptr ||
		    src_widths == nullptr || src_heights == nullptr) {
			throw std::invalid_argument("ju_debug_scale_members: NULL array");
		}
		constexpr size_t kMost = 1u << 15;
		if (dst_width < 1 || dst_height < 1 || dst_width > kMost || dst_height > kMost) {
			throw std::invalid_argument("ju_debug_scale_members: a size outside 1 .. 32768");
		}
		for (int i = 0; i < count; ++i) {
			if (src_widths[i] < 1 || src_heights[i] < 1 || src_widths[i] > kMost || src_heights[i] > kMost) {
				throw std::invalid_argument("ju_debug_scale_members: a size outside 1 .. 32768");
			}
			if (dst[i] == nullptr || src[i] == nullptr) throw std::invalid_argument("ju_debug_scale_members: NULL buffer");
		}
		for (int i = 0; i < count; ++i) {  // (every member's filter and ratios before any device call: buildScaleAxis refuses)
			ju::buildScaleAxis(static_cast<int>(src_widths[i]), static_cast<int>(dst_width), filters[i]);
			ju::buildScaleAxis(static_cast<int>(src_heights[i]), static_cast<int>(dst_height), filters[i]);
		}
		// each member its own scaler, as each runtime of a group pass has
		ju::Scaler scalers[ju::kFlowBatchMax];
		ju::ScaleMembers members{};
		for (int i = 0; i < count; ++i) {
			scalers[i].build(src_widths[i], src_heights[i], dst_width, dst_height, filters[i]);
			members.member[i] = scalers[i].member(static_cast<const std::uint8_t *>(src[i]), src_strides[i],
			    static_cast<std::uint8_t *>(dst[i]), dst_strides[i]);
		}
		ju::launchScaleBgrxMembers(members, count, static_cast<int>(dst_width), static_cast<int>(dst_height), nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_scene(int op, const void *frame, ptrdiff_t stride, size_t width, size_t height, void *prev, void *state,
    int has_prev, uint32_t threshold_milli, int reset_mode, ju_scene_info *record, void *clear_a, size_t a_bytes,
    void *clear_b, size_t b_bytes) {
	return guarded([&] {
		if (op == 2) {  // the refusals of ju_set_scene_detect alone: no device
			const std::string problem = ju::sceneDetectProblem(has_prev, threshold_milli);  // (has_prev: the mode)
			if (!problem.empty()) throw std::invalid_argument("ju_set_scene_detect: " + problem);
			return;
		}
		if (op == 1) {  // scene_clear_kernel alone; `state`: the device flag word
			ju::launchSceneClear(static_cast<const unsigned *>(state), clear_a, a_bytes, clear_b, b_bytes, nullptr);
			JU_HIP(hipStreamSynchronize(nullptr));
			return;
		}
		if (op != 0) throw std::invalid_argument("ju_debug_scene: op must be 0, 1 or 2");
		if (record == nullptr) throw std::invalid_argument("ju_debug_scene: record is NULL");
		ju::PinnedWords ring(sizeof(ju::SceneRecord) * (ju::kSceneRing + 1));
		ju::SceneSadLaunch q;
		q.src = static_cast<const std::uint8_t *>(frame);
		q.srcStride = stride;
		q.width = static_cast<int>(std::min<size_t>(width, 1u << 20));
		q.height = static_cast<int>(std::min<size_t>(height, 1u << 20));
		q.prev = static_cast<std::uint32_t *>(prev);
		q.state = static_cast<ju::SceneState *>(state);
		q.ring = reinterpret_cast<ju::SceneRecord *>(ring.device());
		q.hasPrev = has_prev;
		q.thresholdMilli = threshold_milli;
		q.resetMode = reset_mode != 0;
		ju::launchSceneSad(q, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		const auto *r = reinterpret_cast<const volatile ju::SceneRecord *>(ring.host());
		record->step = r->step;
		record->sad = r->sad;
		record->score = r->score;
		record->cut = r->cut;
		record->reserved = 0;
	});
}

int ju_debug_scene_pass(int count, const void *const *frames, const ptrdiff_t *strides, size_t width, size_t height, void *prev,
    void *state, void *pass_state, int has_prev, uint64_t first_step, uint32_t threshold_milli, int reset_mode,
    ju_scene_info *records, uint32_t *reset_at, int32_t *cut_at) {
	return guarded([&] {
		static_assert(sizeof(ju::ScenePassState) == 136, "the layout include/joshupscale_amd_test.h describes");
		if (count < 1 || count > ju::kFlowBatchMax) throw std::invalid_argument("ju_debug_scene_pass: count must be 1 .. 8");
		if (frames == nullptr || strides == nullptr || records == nullptr || reset_at == nullptr || cut_at == nullptr) {
			throw std::invalid_argument("ju_debug_scene_pass: NULL array");
		}
		if (has_prev != 0 && has_prev != 1 && has_prev != 3) throw std::invalid_argument("ju_debug_scene_pass: has_prev must be 0, 1 or 3");
		ju::PinnedWords ring(sizeof(ju::SceneRecord) * (ju::kSceneRing + 1));
		ju::PinnedWords dynWords(sizeof(ju::ScenePassDyn));
		auto *dyn = reinterpret_cast<volatile ju::ScenePassDyn *>(dynWords.host());
		dyn->stepBase = first_step;
		dyn->seen = has_prev == 3 ? 2u : static_cast<unsigned>(has_prev);
		dyn->thresholdMilli = threshold_milli;
		dyn->slot = static_cast<unsigned>(first_step % ju::kSceneRing);
		ju::ScenePassLaunch q;
		q.items = count;
		for (int i = 0; i < count; ++i) {
			q.frames[i] = static_cast<const std::uint8_t *>(frames[i]);
			q.strides[i] = strides[i];
		}
		q.width = static_cast<int>(std::min<size_t>(width, 1u << 20));
		q.height = static_cast<int>(std::min<size_t>(height, 1u << 20));
		q.prev = static_cast<std::uint32_t *>(prev);
		q.state = static_cast<ju::SceneState *>(state);
		q.pass = static_cast<ju::ScenePassState *>(pass_state);
		q.dyn = reinterpret_cast<const ju::ScenePassDyn *>(dynWords.device());
		q.ring = reinterpret_cast<ju::SceneRecord *>(ring.device());
		q.resetMode = reset_mode != 0;
		ju::launchScenePass(q, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		const auto *r = reinterpret_cast<const volatile ju::SceneRecord *>(ring.host());
		for (int i = 0; i < count; ++i) {
			const volatile ju::SceneRecord &rec = r[(first_step + static_cast<uint64_t>(i)) % ju::kSceneRing];
			records[i].step = rec.step;
			records[i].sad = rec.sad;
			records[i].score = rec.score;
			records[i].cut = rec.cut;
			records[i].reserved = 0;
		}
		ju::ScenePassState after;
		JU_HIP(hipMemcpy(&after, pass_state, sizeof(after), hipMemcpyDeviceToHost));
		for (int i = 0; i < count; ++i) {
			reset_at[i] = after.resetAt[i];
			cut_at[i] = after.cutAt[i];
		}
	});
}

int ju_debug_scene_group(int count, const void *const *frames, const ptrdiff_t *strides, size_t width, size_t height,
    void *const *prev, void *const *states, const int *has_prev, const uint64_t *first_steps, const uint32_t *threshold_milli,
    const int *modes, ju_scene_info *records, uint32_t *reset_flags) {
	return guarded([&] {
		static_assert(sizeof(ju::SceneState) == 40, "the layout include/joshupscale_amd_test.h describes");
		if (count < 1 || count > ju::kFlowBatchMax) throw std::invalid_argument("ju_debug_scene_group: count must be 1 .. 8");
		if (frames == nullptr || strides == nullptr || prev == nullptr || states == nullptr || has_prev == nullptr ||
		    first_steps == nullptr || threshold_milli == nullptr || modes == nullptr || records == nullptr || reset_flags == nullptr) {
			throw std::invalid_argument("ju_debug_scene_group: NULL array");
		}
		const std::size_t ringBytes = sizeof(ju::SceneRecord) * (ju::kSceneRing + 1);
		ju::PinnedWords rings(ringBytes * static_cast<std::size_t>(count));
		ju::PinnedWords dynWords(sizeof(ju::SceneGroupDyn) * static_cast<std::size_t>(count));
		auto *dyn = reinterpret_cast<volatile ju::SceneGroupDyn *>(dynWords.host());
		ju::SceneGroupLaunch q;
		q.items = count;
		q.width = static_cast<int>(std::min<size_t>(width, 1u << 20));
		q.height = static_cast<int>(std::min<size_t>(height, 1u << 20));
		for (int i = 0; i < count; ++i) {
			records[i] = ju_scene_info{};
			reset_flags[i] = 0;
			if (frames[i] == nullptr) continue;  // an absent item
			const std::string who = "ju_debug_scene_group: item " + std::to_string(i);
			if (has_prev[i] != 0 && has_prev[i] != 1 && has_prev[i] != 3) throw std::invalid_argument(who + ": has_prev must be 0, 1 or 3");
			if (modes[i] != 1 && modes[i] != 2) throw std::invalid_argument(who + ": mode must be JU_SCENE_REPORT (1) or JU_SCENE_RESET (2)");
			dyn[i].step = first_steps[i];
			dyn[i].slotHasPrev = (first_steps[i] % ju::kSceneRing) | (static_cast<unsigned long long>(has_prev[i]) << 32);
			dyn[i].thresholdMode = static_cast<unsigned long long>(threshold_milli[i]) | (static_cast<unsigned long long>(modes[i]) << 32);
			ju::SceneGroupItem &it = q.item[i];
			it.frame = static_cast<const std::uint8_t *>(frames[i]);
			it.stride = strides[i];
			it.prev = static_cast<std::uint32_t *>(prev[i]);
			it.state = static_cast<ju::SceneState *>(states[i]);
			it.ring = reinterpret_cast<ju::SceneRecord *>(reinterpret_cast<unsigned char *>(rings.device()) + ringBytes * static_cast<std::size_t>(i));
			it.dyn = reinterpret_cast<const ju::SceneGroupDyn *>(dynWords.device()) + i;
		}
		ju::launchSceneGroup(q, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		for (int i = 0; i < count; ++i) {
			if (frames[i] == nullptr) continue;
			const auto *ring = reinterpret_cast<const volatile ju::SceneRecord *>(
			    reinterpret_cast<const volatile unsigned char *>(rings.host()) + ringBytes * static_cast<std::size_t>(i));
			const volatile ju::SceneRecord &rec = ring[first_steps[i] % ju::kSceneRing];
			records[i].step = rec.step;
			records[i].sad = rec.sad;
			records[i].score = rec.score;
			records[i].cut = rec.cut;
			records[i].reserved = 0;
			ju::SceneState after;
			JU_HIP(hipMemcpy(&after, states[i], sizeof(after), hipMemcpyDeviceToHost));
			reset_flags[i] = after.resetNow;
		}
	});
}

int ju_debug_scene_clear_items(int count, const void *const *flags, void *const *a, const size_t *a_bytes, void *const *b,
    const size_t *b_bytes) {
	return guarded([&] {
		if (count < 1 || count > ju::kFlowBatchMax) throw std::invalid_argument("ju_debug_scene_clear_items: count must be 1 .. 8");
		if (flags == nullptr || a == nullptr || a_bytes == nullptr || b == nullptr || b_bytes == nullptr) {
			throw std::invalid_argument("ju_debug_scene_clear_items: NULL array");
		}
		ju::SceneClearItem items[ju::kFlowBatchMax];
		for (int i = 0; i < count; ++i) {
			items[i] = ju::SceneClearItem{static_cast<const unsigned *>(flags[i]), a[i], a_bytes[i], b[i], b_bytes[i]};
		}
		ju::launchSceneClearItems(items, count, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_temporal(void *state, const void *pre_warp, void *out, ptrdiff_t out_stride, const void *sums, size_t width,
    size_t height, float strength, float threshold, float gain, int window, unsigned flags, uint64_t *acc,
    size_t acc_capacity) {
	return guarded([&] {
		auto refuse = [](const std::string &why) { throw std::invalid_argument("ju_debug_temporal: " + why); };
		if (state == nullptr || pre_warp == nullptr || out == nullptr) refuse("null buffer");
		if (width < 1 || height < 1 || width > 8192 || height > 8192) refuse("a size outside 1 .. 8192");
		if (reinterpret_cast<std::uintptr_t>(state) % 8 || reinterpret_cast<std::uintptr_t>(pre_warp) % 8) {
			refuse("the f16 tensors must be 8-byte aligned");
		}
		if (reinterpret_cast<std::uintptr_t>(out) % 4 || out_stride % 4 || reinterpret_cast<std::uintptr_t>(sums) % 4) {
			refuse("32-bit planes need addresses and strides that are multiples of 4");
		}
		// the model loader's bounds and wording (model.cpp validateConfig)
		if (!(strength >= 0.0f && strength <= 1.0f) || !(threshold >= 0.0f && threshold <= 1.0f)) {
			refuse("temporal filter strength/threshold must be in [0, 1]");
		}
		if (window < 0 || window > 4096) refuse("temporal filter window must be in 0..4096");
		if (!(gain >= 0.0f && gain <= 1e6f)) refuse("temporal filter gain must be in [0, 1e6]");
		if (flags & ~7u) refuse("unknown temporal flag bits");
		const int H = static_cast<int>(height), W = static_cast<int>(width);
		const std::size_t words = ju::temporalAccWords(H, W, window);
		if ((acc == nullptr) != (acc_capacity == 0) || (acc != nullptr && acc_capacity < words)) {
			refuse("acc and acc_capacity go together, and the capacity is at least the window grid");
		}
		// the filter's own words start as ones (zero_words_kernel has to clear them), the words behind them as zeros
		const std::size_t total = std::max(words, acc_capacity);
		ju::DeviceBuffer scratch(8 * total);
		JU_HIP(hipMemset(scratch.get(), 0xff, 8 * words));
		JU_HIP(hipStreamSynchronize(nullptr));
		const ju::TemporalParams tp{strength, threshold, gain, window, (flags & 1u) ? 1 : 0, (flags & 2u) ? 1 : 0,
		    (flags & 4u) ? 1 : 0};
		ju::launchTemporalFilter(state, pre_warp, static_cast<std::uint8_t *>(out), out_stride, H, W,
		    static_cast<const unsigned *>(sums), scratch.as<unsigned long long>(), tp, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		if (acc != nullptr) JU_HIP(hipMemcpy(acc, scratch.get(), 8 * acc_capacity, hipMemcpyDeviceToHost));
	});
}

int ju_debug_e4m3(const float *values, unsigned char *codes, size_t count) {
	return guarded([&] {
		if (count && (!values || !codes)) throw std::invalid_argument("ju_debug_e4m3: null buffer");
		for (size_t i = 0; i < count; ++i) codes[i] = ju::e4m3FromFloat(values[i]);
	});
}

// ---- the network's compute kernels alone (docs/exact_tests.md) --------------------------------------------------------------
}  // extern "C"
namespace {

constexpr int kDebugAxisMax = 4096;

struct DebugRefuse {
	const char *hook;
	[[noreturn]] void operator()(const std::string &why) const { throw std::invalid_argument(std::string(hook) + ": " + why); }
};

bool misaligned(const void *p, std::uintptr_t a) { return reinterpret_cast<std::uintptr_t>(p) % a != 0; }

ju::DType debugDType(const DebugRefuse &refuse, int dtype) {
	if (dtype != JU_DTYPE_F16 && dtype != JU_DTYPE_BF16) refuse("dtype must be JU_DTYPE_F16 or JU_DTYPE_BF16");
	return dtype == JU_DTYPE_F16 ? ju::kF16 : ju::kBF16;
}

void debugActivation(const DebugRefuse &refuse, int act, float slope) {
	if (act < 0 || act > 2) refuse("an activation code outside 0 .. 2");
	// the model loader's bound (model.cpp): max(x, slope x) is LeakyReLU only for a slope in [0, 1]
	if (act == 2 && !(slope >= 0.0f && slope <= 1.0f)) refuse("a LeakyReLU slope outside [0, 1]");
}

ju::DevPlan debugPlan(const DebugRefuse &refuse, const ju_debug_plan &p, ju::PlanLog *log) {
	if (p.flow_tile < 0 || p.res_block < 0 || p.res_block > 2 || p.conv_stages < -1 || p.conv_stages > 2 || p.splitk_rows < 0 ||
	    p.splitk_blocks < 0 || p.splitk_blocks > 2 || p.conv_nb < 0 || p.conv_nb > 2 || p.conv_rw < 0 || p.conv_rw > 2) {
		refuse("a plan field out of range");
	}
	ju::DevPlan plan;
	plan.flowTile = p.flow_tile;
	plan.resBlock = p.res_block;
	plan.convStages = p.conv_stages;
	plan.splitkRows = p.splitk_rows;
	plan.splitkBlocks = p.splitk_blocks;
	plan.convNb = p.conv_nb;
	plan.convRw = p.conv_rw;
	plan.log = log;
	return plan;
}

void debugPlanText(const ju::PlanLog &log, char *dst, std::size_t capacity) {
	if (dst == nullptr || capacity == 0) return;
	const std::string text = log.text();
	const std::size_t n = std::min(text.size(), capacity - 1);
	std::memcpy(dst, text.data(), n);
	dst[n] = '\0';
}

// host f32 [taps][cinReal][cout] -> the kernel-ready weights on the device, through the product's packer
ju::DeviceBuffer debugPackWeights(const float *w, int taps, int cinReal, int cinPadded, int cout, int nb, ju::DType dt) {
	ju::FoldedConv conv;
	conv.taps = taps;
	conv.cin = cinReal;
	conv.cout = cout;
	conv.w.assign(w, w + static_cast<std::size_t>(taps) * cinReal * cout);
	std::vector<int> cinMap(static_cast<std::size_t>(cinPadded), -1);
	for (int c = 0; c < cinReal; ++c) cinMap[static_cast<std::size_t>(c)] = c;
	const std::vector<std::uint16_t> packed = ju::packConvWeights(conv, cinMap, nb, dt);
	ju::DeviceBuffer dev(packed.size() * 2);
	dev.upload(packed.data(), packed.size() * 2);
	return dev;
}

ju::DeviceBuffer debugUploadBias(const float *bias, int cout) {
	ju::DeviceBuffer dev(static_cast<std::size_t>(cout) * 4);
	dev.upload(bias, static_cast<std::size_t>(cout) * 4);
	return dev;
}

// pitch (pixels, 0 = dense) of a tensor `width` pixels wide; item stride of `rows` such rows of `channels` 16-bit values
void debugPitch(const DebugRefuse &refuse, int pitch, int width, const char *what) {
	if (pitch != 0 && (pitch < width || pitch > 2 * kDebugAxisMax)) refuse(std::string(what) + " pitch below the row (or beyond 8192)");
}
void debugItemStride(const DebugRefuse &refuse, int items, long long stride, int pitch, int width, int rows, int channels, const char *what) {
	if (items <= 1) return;
	const long long tensor = 2ll * (pitch ? pitch : width) * rows * channels;
	if (stride < tensor || stride % 16 != 0 || stride > (1ll << 32)) {
		refuse(std::string(what) + " item stride must be a multiple of 16, at least the tensor");
	}
}

}  // namespace
extern "C" {

int ju_debug_conv(const ju_debug_conv_args *a) {
	return guarded([&] {
		const DebugRefuse refuse{"ju_debug_conv"};
		if (a == nullptr) refuse("null arguments");
		const ju::DType dt = debugDType(refuse, a->dtype);
		if (a->kernel < 0 || a->kernel > 2) refuse("kernel must be 0 (conv), 1 (split-K) or 2 (tower)");
		if (a->in == nullptr || a->out == nullptr || a->weights == nullptr || a->bias == nullptr) refuse("null buffer");
		if ((a->plan_text == nullptr) != (a->plan_capacity == 0)) refuse("plan_text and plan_capacity go together");
		if (misaligned(a->in, 16) || misaligned(a->out, 16) || misaligned(a->res, 16)) refuse("tensors must be 16-byte aligned");
		if (a->H < 1 || a->W < 1 || a->H > kDebugAxisMax || a->W > kDebugAxisMax) refuse("a size outside 1 .. 4096");
		if (a->cin < 16 || a->cin > 1024 || a->cout < 32 || a->cout > 1024 || a->cin_real < 1 || a->cin_real > a->cin) {
			refuse("channels: cin 16 .. 1024, cin_real 1 .. cin, cout 32 .. 1024");
		}
		debugActivation(refuse, a->relu, a->slope);
		const int items = a->items;
		if (items < 1 || items > ju::kFlowBatchMax) refuse("items must be 1 .. 8");
		// launchConvT's own checks, in its words
		if (a->cin % 16 != 0 || a->cout % 32 != 0 || (a->nb != 1 && a->nb != 2) || (a->rw != 1 && a->rw != 2) ||
		    a->cout % (32 * a->nb) != 0) {
			refuse("conv: cin must be a multiple of 16, cout of 32*nb");
		}
		if (a->taps != 9 && a->taps != 1) refuse("conv: unsupported shape");
		if (a->taps == 1 && ju::convCK(a->cin) == 16) refuse("conv: unsupported shape");
		// (the tile form is launchConv's: the split-K kernel has its own and is held to convSplitKSupported below)
		if (a->pool && ((a->kernel != 1 && a->rw != 2) || a->H % 2 || a->W % 2 || a->res != nullptr || a->out_head)) {
			refuse("conv: fused max-pool needs rw = 2, even H and W, 16-bit output");
		}
		if (a->upsample && (a->taps != 9 || ju::convCK(a->cin) != 64 || a->nb != 1 || a->H % 2 || a->W % 2 || a->pool)) {
			refuse("conv: fused upsampling needs 3x3, cin % 64 == 0, nb = 1, even H and W");
		}
		if (items > 1 && a->res != nullptr) refuse("launchConv: a look-ahead launch (items > 1) takes no residual");
		const int inW = a->upsample ? a->W / 2 : a->W, inH = a->upsample ? a->H / 2 : a->H;
		const int outW = a->pool ? a->W / 2 : a->W, outH = a->pool ? a->H / 2 : a->H;
		debugPitch(refuse, a->in_pitch, inW, "input");
		debugPitch(refuse, a->out_pitch, outW, "output");
		debugPitch(refuse, a->res_pitch, a->W, "residual");
		debugItemStride(refuse, items, a->in_item_bytes, a->in_pitch, inW, inH, a->cin, "input");
		debugItemStride(refuse, items, a->out_item_bytes, a->out_pitch, outW, outH, a->cout, "output");

		ju::PlanLog log;
		const ju::DevPlan plan = debugPlan(refuse, a->plan, &log);
		ju::ConvParams p{};
		p.in = a->in;
		p.res = a->res;
		p.out = a->out;
		p.H = a->H;
		p.W = a->W;
		p.cin = a->cin;
		p.cout = a->cout;
		p.taps = a->taps;
		p.relu = a->relu;
		p.slope = a->slope;
		p.outHead = a->out_head ? 1 : 0;
		p.pool = a->pool ? 1 : 0;
		p.upsample = a->upsample ? 1 : 0;
		p.inPitch = a->in_pitch;
		p.outPitch = a->out_pitch;
		p.resPitch = a->res_pitch;
		p.nb = a->nb;
		p.rw = a->rw;
		p.items = items;
		p.inItemBytes = static_cast<long>(a->in_item_bytes);
		p.outItemBytes = static_cast<long>(a->out_item_bytes);
		p.plan = &plan;
		if (a->kernel == 1 && !ju::convSplitKSupported(p)) refuse("split-K conv: unsupported layer");
		if (a->kernel == 2) {
			const int pitch = ju::towerPitch(a->W);
			const bool fits = a->taps == 9 && a->cin == 64 && a->cout == 64 && !a->out_head && a->nb == 2 && a->in_pitch == pitch &&
			                  a->out_pitch == pitch && (a->res == nullptr || a->res_pitch == pitch);
			if (!fits || a->pool || a->upsample || items > 1) {
				refuse("the tower kernel needs 3x3 64 -> 64, nb = 2, one item, no pool or upsampling, and every pitch towerPitch(W)");
			}
		}

		const ju::DeviceBuffer wgt = debugPackWeights(a->weights, a->taps, a->cin_real, a->cin, a->cout, a->nb, dt);
		const ju::DeviceBuffer bias = debugUploadBias(a->bias, a->cout);
		p.wgt = wgt.get();
		p.bias = bias.as<float>();
		if (a->kernel == 0) {
			ju::launchConv(dt, p, nullptr);
		} else if (a->kernel == 1) {
			const ju::DeviceBuffer zeros(256);  // (DeviceBuffer memory starts zeroed)
			ju::launchConvSplitK(dt, p, zeros.get(), nullptr);
			JU_HIP(hipStreamSynchronize(nullptr));
		} else {
			ju::launchConvTower(dt, p, nullptr);
		}
		JU_HIP(hipStreamSynchronize(nullptr));
		debugPlanText(log, a->plan_text, a->plan_capacity);
	});
}

int ju_debug_flow_block(const ju_debug_flow_block_args *a) {
	return guarded([&] {
		const DebugRefuse refuse{"ju_debug_flow_block"};
		if (a == nullptr) refuse("null arguments");
		const ju::DType dt = debugDType(refuse, a->dtype);
		if (a->in == nullptr || a->out == nullptr || a->weights1 == nullptr || a->bias1 == nullptr || a->weights2 == nullptr ||
		    a->bias2 == nullptr) {
			refuse("null buffer");
		}
		if ((a->plan_text == nullptr) != (a->plan_capacity == 0)) refuse("plan_text and plan_capacity go together");
		if (misaligned(a->in, 16) || misaligned(a->out, 16)) refuse("tensors must be 16-byte aligned");
		if (a->H < 1 || a->W < 1 || a->H > kDebugAxisMax || a->W > kDebugAxisMax) refuse("a size outside 1 .. 4096");
		debugActivation(refuse, a->act1, a->slope);
		debugActivation(refuse, a->act2, a->slope);
		const int items = a->items;
		if (items < 1) refuse("items must be 1 .. 8");
		if (items > ju::kFlowBatchMax) refuse("flow block: more look-ahead frames than kFlowBatchMax");
		if (items > 1 && a->residual) refuse("flow block: the residual form has no look-ahead launch");
		if (a->upsample && (a->H % 2 || a->W % 2)) refuse("flow block: fused upsampling needs even H and W");
		if (a->pool && (a->H % 2 || a->W % 2)) refuse("flow block: fused max-pool needs even H and W");
		// the launcher's table (flow_kernels.hip JU_FB_CASE): cin, cmid, upsample, pool, 0 plain / 1 flow head / 2 residual
		static const int table[10][5] = {{16, 32, 0, 1, 0}, {32, 64, 0, 1, 0}, {64, 128, 0, 1, 0}, {256, 128, 1, 0, 0},
		    {256, 128, 0, 0, 0}, {128, 64, 1, 0, 0}, {128, 64, 0, 0, 0}, {64, 32, 1, 0, 1}, {64, 32, 0, 0, 1}, {64, 64, 0, 0, 2}};
		if (a->residual && a->out_head) refuse("flow block: unsupported shape");
		const int outk = a->residual ? 2 : (a->out_head ? 1 : 0);
		bool known = false;
		for (const auto &t : table) {
			known = known || (a->cin == t[0] && a->cmid == t[1] && (a->upsample != 0) == (t[2] != 0) && (a->pool != 0) == (t[3] != 0) &&
			                     outk == t[4]);
		}
		if (!known) refuse("flow block: unsupported shape");
		if (a->cin_real < 1 || a->cin_real > a->cin) refuse("cin_real must be 1 .. cin");
		const int inW = a->upsample ? a->W / 2 : a->W, inH = a->upsample ? a->H / 2 : a->H;
		const int outW = a->pool ? a->W / 2 : a->W, outH = a->pool ? a->H / 2 : a->H;
		debugPitch(refuse, a->in_pitch, inW, "input");
		debugPitch(refuse, a->out_pitch, outW, "output");
		debugItemStride(refuse, items, a->in_item_bytes, a->in_pitch, inW, inH, a->cin, "input");
		debugItemStride(refuse, items, a->out_item_bytes, a->out_pitch, outW, outH, a->cmid, "output");

		ju::PlanLog log;
		const ju::DevPlan plan = debugPlan(refuse, a->plan, &log);
		const ju::DeviceBuffer w1 = debugPackWeights(a->weights1, 9, a->cin_real, a->cin, a->cmid, 1, dt);
		const ju::DeviceBuffer w2 = debugPackWeights(a->weights2, 9, a->cmid, a->cmid, a->cmid, 1, dt);
		const ju::DeviceBuffer b1 = debugUploadBias(a->bias1, a->cmid);
		const ju::DeviceBuffer b2 = debugUploadBias(a->bias2, a->cmid);
		ju::FlowBlockLaunch q{};
		q.in = a->in;
		q.w1 = w1.get();
		q.b1 = b1.as<float>();
		q.w2 = w2.get();
		q.b2 = b2.as<float>();
		q.out = a->out;
		q.H = a->H;
		q.W = a->W;
		q.inPitch = a->in_pitch;
		q.outPitch = a->out_pitch;
		q.cin = a->cin;
		q.cmid = a->cmid;
		q.upsample = a->upsample != 0;
		q.pool = a->pool != 0;
		q.outHead = a->out_head != 0;
		q.residual = a->residual != 0;
		q.act1 = a->act1;
		q.act2 = a->act2;
		q.slope = a->slope;
		q.items = items;
		q.inItemBytes = static_cast<long>(a->in_item_bytes);
		q.outItemBytes = static_cast<long>(a->out_item_bytes);
		q.plan = &plan;
		ju::launchFlowBlock(dt, q, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
		debugPlanText(log, a->plan_text, a->plan_capacity);
	});
}

int ju_debug_resample(const ju_debug_resample_args *a) {
	return guarded([&] {
		const DebugRefuse refuse{"ju_debug_resample"};
		if (a == nullptr) refuse("null arguments");
		const ju::DType dt = debugDType(refuse, a->dtype);
		if (a->op != 0 && a->op != 1) refuse("op must be 0 (upsample) or 1 (max-pool)");
		if (a->in == nullptr || a->out == nullptr) refuse("null buffer");
		if (misaligned(a->in, 16) || misaligned(a->out, 16)) refuse("tensors must be 16-byte aligned");
		if (a->H < 1 || a->W < 1 || a->H > kDebugAxisMax || a->W > kDebugAxisMax) refuse("a size outside 1 .. 4096");
		if (a->C < 8 || a->C > 1024 || a->C % 8 != 0) refuse("C must be a multiple of 8, 8 .. 1024");
		if (a->items < 1 || a->items > ju::kFlowBatchMax) refuse("items must be 1 .. 8");
		if (a->op == 1 && (a->H % 2 || a->W % 2)) refuse("the max-pool needs even H and W");
		if (a->op == 1 && a->items != 1) refuse("the max-pool takes one item");
		if (a->op == 0) ju::launchUpsample2(dt, a->in, a->out, a->H, a->W, a->C, nullptr, a->items);
		else ju::launchMaxPool2(dt, a->in, a->out, a->H, a->W, a->C, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_warp(const ju_debug_warp_args *a) {
	return guarded([&] {
		const DebugRefuse refuse{"ju_debug_warp"};
		if (a == nullptr) refuse("null arguments");
		const ju::DType dt = debugDType(refuse, a->dtype);
		if (a->state == nullptr || a->flow == nullptr || a->frame == nullptr || a->out == nullptr) refuse("null buffer");
		if (a->H < 1 || a->W < 1 || a->H > kDebugAxisMax || a->W > kDebugAxisMax) refuse("a size outside 1 .. 4096");
		if (a->pad_top < 0 || a->pad_left < 0 || a->pad_top > kDebugAxisMax || a->pad_left > kDebugAxisMax ||
		    a->PW < a->W + a->pad_left || a->PW > 2 * kDebugAxisMax) {
			refuse("the flow field: pads 0 .. 4096 and PW at least W + pad_left");
		}
		if (a->out_pitch != 0 && (a->out_pitch < a->W || a->out_pitch > 2 * kDebugAxisMax)) refuse("output pitch below the row (or beyond 8192)");
		if (misaligned(a->state, 8) || misaligned(a->pre_warp_out, 8)) refuse("the f16 state tensors must be 8-byte aligned");
		if (misaligned(a->flow, 16) || misaligned(a->out, 16)) refuse("the flow field and the records must be 16-byte aligned");
		const auto rowOk = [](std::ptrdiff_t stride, std::ptrdiff_t row) { return stride % 4 == 0 && (stride >= row || -stride >= row); };
		if (misaligned(a->frame, 4) || !rowOk(a->frame_stride, 4 * static_cast<std::ptrdiff_t>(a->W))) {
			refuse("the LR frame must be 4-byte aligned with a stride that is a multiple of 4 and at least a row");
		}
		if (misaligned(a->sums, 4)) refuse("sums must be 4-byte aligned");
		if (a->out_u8 != nullptr) {
			// (the launcher's own refusal, in its words)
			if (misaligned(a->out_u8, 4) || a->out_stride % 4 != 0) refuse("warp_pack: the frame output must be 4-byte aligned");
			if (!rowOk(a->out_stride, 16 * static_cast<std::ptrdiff_t>(a->W))) refuse("the frame output's stride is below its row");
		}
		ju::launchWarpPack(dt, a->state, a->flow, static_cast<const std::uint8_t *>(a->frame), a->frame_stride, a->out, a->out_pitch,
		    a->H, a->W, a->PW, a->pad_top, a->pad_left, static_cast<const unsigned *>(a->sums), a->pre_warp_out,
		    static_cast<std::uint8_t *>(a->out_u8), a->out_stride, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

namespace {
// What both masked hooks check behind debugTileSet, before any device call: the source's and the mask's rows and the mask's
// size against the blended frame.  Then the box, by the product's function, from the mask read back to the host.
void debugTileMask(const std::string &name, size_t src_width, size_t src_height, const void *source, ptrdiff_t source_stride,
    const void *mask, ptrdiff_t mask_stride, size_t mask_width, size_t mask_height, ju::TileMask *out) {
	if (source == nullptr) throw std::invalid_argument(name + ": null source");
	const std::string problem = ju::maskSizeProblem(mask_width, mask_height, 4 * src_width, 4 * src_height);
	if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
	if (reinterpret_cast<std::uintptr_t>(source) % 4 || source_stride % 4 || reinterpret_cast<std::uintptr_t>(mask) % 4 || mask_stride % 4) {
		throw std::invalid_argument(name + ": the source's and the mask's address and stride must be multiples of 4");
	}
	const auto srcRow = static_cast<ptrdiff_t>(4 * src_width), maskRow = static_cast<ptrdiff_t>(4 * mask_width);
	if ((source_stride > -srcRow && source_stride < srcRow) || (mask_stride > -maskRow && mask_stride < maskRow)) {
		throw std::invalid_argument(name + ": |stride| of the source or the mask smaller than a row");
	}
	// the mask's rows in memory order, read back once; the box from them
	const ju::RowSpan rows = ju::rowSpan(const_cast<void *>(mask), mask_stride, mask_height);
	const size_t pitch = rows.pitch, bytes = pitch * (mask_height - 1) + static_cast<size_t>(maskRow);
	std::vector<std::uint8_t> back(bytes);
	JU_HIP(hipMemcpy(back.data(), rows.lowest, bytes, hipMemcpyDeviceToHost));
	const std::uint8_t *first = rows.topDown ? back.data() : back.data() + (mask_height - 1) * pitch;
	const ju::MaskBox box = ju::maskBox(first, mask_stride, static_cast<int>(mask_width), static_cast<int>(mask_height),
	    static_cast<int>(4 * src_width), static_cast<int>(4 * src_height));
	ju::TileMask &m = *out;
	m.src = static_cast<const std::uint8_t *>(source);
	m.srcStride = source_stride;
	m.mask = static_cast<const std::uint8_t *>(mask);
	m.maskStride = mask_stride;
	m.maskW = static_cast<int>(mask_width);
	m.maskH = static_cast<int>(mask_height);
	m.x0 = box.x0, m.y0 = box.y0, m.x1 = box.x1, m.y1 = box.y1;
}
}  // namespace

int ju_debug_tile_stitch_mask(void *dst, ptrdiff_t dst_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count, const void *source, ptrdiff_t source_stride, const void *mask,
    ptrdiff_t mask_stride, size_t mask_width, size_t mask_height) {
	if (mask == nullptr) {  // no mask: the unmasked launch, as the object routes it
		return ju_debug_tile_stitch(dst, dst_stride, src_width, src_height, tile_width, tile_height, overlap, tiles, count);
	}
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		const std::string name = "ju_debug_tile_stitch_mask";
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst, dst_stride, 4 * src_width, &set,
		    &nx, &ny);
		if (reinterpret_cast<std::uintptr_t>(dst) % 4 || dst_stride % 4) {
			throw std::invalid_argument(name + ": the frame's address and stride must be multiples of 4");
		}
		for (int k = 0; k < count; ++k) {
			if (set.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(set.ptr[k]) % 16) {
				throw std::invalid_argument(name + ": tile " + std::to_string(k) + " is NULL or not 16-byte aligned");
			}
		}
		ju::TileMask m;
		debugTileMask(name, src_width, src_height, source, source_stride, mask, mask_stride, mask_width, mask_height, &m);
		const ju::TileAxis x = ju::tileAxis(static_cast<long>(src_width), static_cast<long>(tile_width), overlap);
		const ju::TileAxis y = ju::tileAxis(static_cast<long>(src_height), static_cast<long>(tile_height), overlap);
		ju::DeviceBuffer xTable(x.table.size() * sizeof(ju::TileAxisEntry)), yTable(y.table.size() * sizeof(ju::TileAxisEntry));
		xTable.upload(x.table.data(), x.table.size() * sizeof(ju::TileAxisEntry));
		yTable.upload(y.table.data(), y.table.size() * sizeof(ju::TileAxisEntry));
		ju::launchTileStitchMask(static_cast<std::uint8_t *>(dst), dst_stride, static_cast<int>(4 * src_width), static_cast<int>(4 * src_height),
		    set, nx, ny, static_cast<int>(4 * tile_width), xTable.as<unsigned>(), yTable.as<unsigned>(), m, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_tile_stitch_mask_scale(void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, int filter, size_t src_width,
    size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count, const void *source,
    ptrdiff_t source_stride, const void *mask, ptrdiff_t mask_stride, size_t mask_width, size_t mask_height) {
	if (mask == nullptr) {  // no mask: the unmasked launch, as the object routes it
		return ju_debug_tile_stitch_scale(dst, dst_stride, dst_width, dst_height, filter, src_width, src_height, tile_width, tile_height,
		    overlap, tiles, count);
	}
	return guarded([&] {
		int nx = 0, ny = 0;
		ju::TileSet set;
		const std::string name = "ju_debug_tile_stitch_mask_scale";
		debugTileSet(name.c_str(), src_width, src_height, tile_width, tile_height, overlap, tiles, count, dst, dst_stride, dst_width, &set,
		    &nx, &ny);
		// (the size limits and the tiles' alignment first, then the mask's; the tables' device memory behind both)
		const std::string problem = ju::tiledOutputSizeProblem(dst_width, dst_height, src_width, src_height, filter);
		if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
		for (int k = 0; k < count; ++k) {
			if (set.ptr[k] == nullptr || reinterpret_cast<std::uintptr_t>(set.ptr[k]) % 16) {
				throw std::invalid_argument(name + ": tile " + std::to_string(k) + " is NULL or not 16-byte aligned");
			}
		}
		ju::TileMask m;
		debugTileMask(name, src_width, src_height, source, source_stride, mask, mask_stride, mask_width, mask_height, &m);
		DebugStitchScale d;
		debugStitchScale(name, dst_width, dst_height, filter, src_width, src_height, tile_width, tile_height, overlap, set, count, &d);
		ju::launchTileStitchMaskScale(static_cast<std::uint8_t *>(dst), dst_stride, static_cast<int>(dst_width), static_cast<int>(dst_height),
		    static_cast<int>(4 * src_width), static_cast<int>(4 * src_height), set, nx, ny, static_cast<int>(4 * tile_width),
		    d.xTable.as<unsigned>(), d.yTable.as<unsigned>(), d.scale.xAxis(), d.scale.yAxis(), d.scale.span(), m, nullptr);
		JU_HIP(hipStreamSynchronize(nullptr));
	});
}

int ju_debug_mask_box(const void *mask, ptrdiff_t mask_stride, size_t mask_width, size_t mask_height, size_t width, size_t height,
    int *box) {
	return guarded([&] {
		const std::string name = "ju_debug_mask_box";
		if (mask == nullptr || box == nullptr) throw std::invalid_argument(name + ": null argument");
		if (width < 1 || height < 1 || width > (1u << 20) || height > (1u << 20)) throw std::invalid_argument(name + ": a frame size outside 1 .. 2^20");
		const std::string problem = ju::maskSizeProblem(mask_width, mask_height, width, height);
		if (!problem.empty()) throw std::invalid_argument(name + ": " + problem);
		const auto row = static_cast<ptrdiff_t>(4 * mask_width);
		if (mask_stride > -row && mask_stride < row) throw std::invalid_argument(name + ": |stride| smaller than a row");
		const ju::MaskBox b = ju::maskBox(static_cast<const std::uint8_t *>(mask), mask_stride, static_cast<int>(mask_width),
		    static_cast<int>(mask_height), static_cast<int>(width), static_cast<int>(height));
		box[0] = b.x0, box[1] = b.y0, box[2] = b.x1, box[3] = b.y1;
	});
}

int ju_debug_tiled_pass_plan(int count, int cap, const unsigned char *clash, int *starts, int capacity, int *passes) {
	return guarded([&] {
		const std::string name = "ju_debug_tiled_pass_plan";
		if (passes == nullptr || (capacity > 0 && starts == nullptr) || capacity < 0) throw std::invalid_argument(name + ": null argument");
		if (count < 0 || count > 4096) throw std::invalid_argument(name + ": count outside 0 .. 4096");
		if (count > 0 && clash == nullptr) throw std::invalid_argument(name + ": null argument");
		const std::vector<int> plan = ju::tilePassPlan(count, cap, [&](int i, int j) {
			return clash[static_cast<std::size_t>(i) * static_cast<std::size_t>(count) + static_cast<std::size_t>(j)] != 0;
		});
		*passes = static_cast<int>(plan.size());
		for (int k = 0; k < capacity && k < *passes; ++k) starts[k] = plan[static_cast<std::size_t>(k)];
	});
}
#endif  // JU_TEST_HOOKS

const char *ju_version(void) {
	#ifdef JU_TEST_HOOKS
	return "joshupscale-amd 0.1 (gfx950, test hooks)";
#else
	return "joshupscale-amd 0.1 (gfx950)";
#endif
}

}  // extern "C"
