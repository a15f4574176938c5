/*
 * joshupscale_amd.h -- C ABI of the MI355X-native JoshUpscale runtime.
 *
 * This is the drop-in boundary for the reference's core/ runtime: plain C,
 * plain pointers and sizes, no C++ or torch types.  Each entry point states the
 * reference interface it replaces (paths relative to the reference repository).
 * The C++ surface the AviSynth/OBS plugins compile against
 * (include/JoshUpscale/core.h) is a thin shim over these functions; so are the
 * Python (ctypes) bindings in joshupscale_amd/runtime.py.
 *
 * Threading: a ju_runtime is not thread-safe (one internal HIP stream; the
 * reference declares MT_SERIALIZED, avisynth_plugin/src/main.cc:176-178).
 * Several runtimes, also on different devices, may coexist.  ju_last_error()
 * is thread-local.
 *
 * Every function returning int returns JU_OK (0) or a JU_ERR_* code; the
 * message is then available from ju_last_error() on the calling thread.
 */
#ifndef JOSHUPSCALE_AMD_H_
#define JOSHUPSCALE_AMD_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define JU_API __attribute__((visibility("default")))
#else
#define JU_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ju_runtime ju_runtime;

enum {
	JU_OK = 0,
	JU_ERR_INVALID_ARGUMENT = 1, /* std::invalid_argument in the reference */
	JU_ERR_IO = 2,               /* std::ios_base::failure (model file) */
	JU_ERR_DEVICE = 3,           /* HIP error (CudaException, core/include/JoshUpscale/core/cuda.h:24-32) */
	JU_ERR_UNSUPPORTED = 4,
	JU_ERR_INTERNAL = 5
};

/* DataLocation of core/public/JoshUpscale/core.h:30.  JU_LOC_DEVICE is the
 * reference's CUDA location reinterpreted as "HIP device pointer". */
enum { JU_LOC_CPU = 0, JU_LOC_DEVICE = 1, JU_LOC_GRAPHICS_RESOURCE = 2 };

/* Compute precision of MFMA operands / stored activations.  JU_DTYPE_FP8: the 64->64
 * residual-block convolutions of the generator run on OCP e4m3 operands (block-scaled
 * MFMA; the counterpart of the reference's TensorRT INT8 engines,
 * scripts/inference/tensorrt/quantize_int8.py:140-209), every other layer and the
 * residual stream stay fp16. */
enum { JU_DTYPE_DEFAULT = -1, JU_DTYPE_F16 = 0, JU_DTYPE_BF16 = 1, JU_DTYPE_FP8 = 2 };

/* LogLevel of core/public/JoshUpscale/core.h:21. */
enum { JU_LOG_INFO = 0, JU_LOG_WARNING = 1, JU_LOG_ERROR = 2 };

/* Mirrors struct Image (core/public/JoshUpscale/core.h:32-38) field for field:
 * 4 bytes per pixel, byte order B,G,R,X (X ignored on input, written 0 on
 * output); stride in bytes, may be negative (bottom-up frames, ptr = first
 * logical row); width/height in pixels. */
typedef struct ju_image {
	void *ptr;
	uint8_t location;
	ptrdiff_t stride;
	size_t width;
	size_t height;
} ju_image;

/* ---- 4:2:0 YUV frames, 8- and 10-bit (no reference counterpart: the reference takes BGRX Images only) ------------
 * Video decoders emit and encoders take NV12 / I420 (AviSynth: YV12 = I420 with the chroma planes swapped -- planes
 * are passed by pointer, so their order in memory does not matter).  ju_process_frame converts on the GPU, inside the
 * runtime's own staging: a YUV input is decoded into the BGRX frame the network consumes, the network's BGRX output is
 * encoded into the caller's planes.  Input and output formats are independent (all 25 pairs).  A YUV frame is one
 * step of the same recurrent stream: ju_process, ju_process_frame, ju_process_frames and ju_process_batch may be mixed
 * on one runtime.
 *
 * The conversion is integer arithmetic, defined exactly ("YUV frames").  ju_frame.colorspace is
 * JU_CS_* | JU_CHROMA_*, per frame and per side:
 *
 *   JU_CS_* (the low byte): BT.601, BT.709 or BT.2020 non-constant-luminance coefficients (K_r, K_b = 0.299, 0.114 /
 *   0.2126, 0.0722 / 0.2627, 0.0593), limited (16..235 / 16..240; 10-bit 64..940 / 64..960) or full range.
 *
 *   JU_CHROMA_* (bits 8-9): where chroma sample (i, j) sits among the luma samples at integer (x, y).
 *     JU_CHROMA_LEFT     (2i,       2j + 1/2)  MPEG-2 / H.264 / most HEVC; 0, so a plain JU_CS_* value means this
 *     JU_CHROMA_CENTER   (2i + 1/2, 2j + 1/2)  JPEG / MJPEG / MPEG-1 (ffmpeg yuvj420p / yuvj422p, with JU_CS_*_FULL)
 *     JU_CHROMA_TOPLEFT  (2i,       2j)        UHD HEVC, H.273 chroma_sample_loc_type 2
 *   Decoding interpolates bilinearly between the two nearest chroma samples of each axis -- a co-sited axis takes c[i] at
 *   2i and (c[i] + c[i+1]) / 2 at 2i + 1, a centred axis (3 c[i] + c[i-1]) / 4 and (3 c[i] + c[i+1]) / 4 -- and encoding
 *   filters R, G, B symmetrically about the chroma position: [1,2,1] on a co-sited axis, [1,1] on a centred one.  4:2:2
 *   has the horizontal axis only (TOPLEFT is LEFT there); a 4:4:4 format accepts a siting and ignores it.
 *
 * Refused with JU_ERR_INVALID_ARGUMENT before anything runs: a low byte above 5 ("unknown ... colour space N"), the siting
 * field 3 ("unknown ... chroma siting 3") and any bit above bit 9.  tests/chroma_siting_reference.py is the definition,
 * bit for bit.
 *
 * 10-bit 4:2:0 (what HEVC Main10 / AV1 decoders and encoders and high-bit-depth AviSynth+ scripts hold): samples are
 * 16-bit little-endian words.  JU_FMT_P010: planes as NV12, the 10-bit value in the UPPER bits (word = value << 6); on
 * input the low 6 bits are ignored, on output they are written 0.  JU_FMT_I010 (yuv420p10le): planes as I420, the value
 * in the LOW 10 bits; on input the upper 6 bits are ignored, on output they are 0.  Limited range is 64..940 / 64..960.
 * A 10-bit input is decoded to the same 8-bit BGRX frame the network consumes.  A 10-bit OUTPUT is encoded from the
 * runtime's f16 recurrent state -- the frame in float, before the truncation to 8 bits -- so it carries real 10-bit
 * precision; models whose state is not the frame (normalize_brightness, output_flow) encode it from the 8-bit frame
 * instead (257 x u8).  ju_get_stat "hbd_from_state" tells which (1 / 0); it is fixed at creation.
 *
 * 4:2:2 and 4:4:4 (what capture devices deliver -- YUY2 / UYVY -- and what keeps the colour detail of the 4x output).
 * Chroma is co-sited horizontally with the even luma columns, as above; every row has its own chroma row.  Decoding a
 * 4:2:2 frame takes the chroma sample at even columns and the mean of two at odd ones; encoding filters [1,2,1] along
 * the row.  4:4:4 resamples nothing.  Coefficients, ranges, the 10-bit words and the source of a 10-bit output are those
 * of the 4:2:0 formats of the same depth.
 *
 *   format        sampling  bits  planes and layout
 *   JU_FMT_YUY2   4:2:2     8     one plane, [H][2W] bytes: Y0 U Y1 V per pixel pair
 *   JU_FMT_UYVY   4:2:2     8     one plane, [H][2W] bytes: U Y0 V Y1
 *   JU_FMT_I422   4:2:2     8     Y [H][W], U and V [H][W/2] (AviSynth YV16: pass the pointers swapped)
 *   JU_FMT_P210   4:2:2     10    Y [H][W] words, UV [H][W] words (U first); value in the UPPER 10 bits, as P010
 *   JU_FMT_I210   4:2:2     10    Y [H][W], U and V [H][W/2] words; value in the LOW 10 bits, as I010
 *   JU_FMT_I444   4:4:4     8     Y, U, V [H][W] (YV24)
 *   JU_FMT_I410   4:4:4     10    Y, U, V [H][W] words; value in the low 10 bits (yuv444p10le)
 *
 * 4:2:2 needs an even width (any height), 4:4:4 neither; the 4:2:0 formats need both even.  With these coefficients a
 * JU_FMT_I410 frame carries an 8-bit frame without loss: decoding the encoding of 257 x u8 returns every colour.
 *
 * RGB in other layouts and depths (what OpenCV, ffmpeg rgb24 / bgr24 / gbrp* / gbrpf32le / bgra64le, VapourSynth RGBS /
 * RGBH and AviSynth+ RGBP* / RGB64 hold; BGR96F is the [1,H,W,3] float tensor of a model whose uint8 input and output were
 * turned into float).  `colorspace` is ignored, as for BGRX.  Planar planes are passed as planes[0..2] = R, G, B: a caller
 * whose memory order is G, B, R (ffmpeg gbrp*, AviSynth+) passes the pointers in that order, as for YV12 above.
 *
 *   format          layout
 *   JU_FMT_BGR24    one plane, [H][3W] bytes B,G,R
 *   JU_FMT_RGB24    one plane, [H][3W] bytes R,G,B
 *   JU_FMT_RGBX     one plane, [H][4W] bytes R,G,B,X (X ignored in, 0 out)
 *   JU_FMT_BGRX64   one plane, [H][4W] 16-bit LE words B,G,R,X (X ignored in, 0 out)
 *   JU_FMT_RGBP8    R, G, B [H][W] bytes
 *   JU_FMT_RGBP10   R, G, B [H][W] words, value in the LOW 10 bits (upper 6 ignored in, 0 out)
 *   JU_FMT_RGBP16   R, G, B [H][W] words
 *   JU_FMT_RGBPH    R, G, B [H][W] IEEE f16, nominal range 0..1
 *   JU_FMT_RGBPS    R, G, B [H][W] IEEE f32, nominal range 0..1
 *   JU_FMT_BGR96F   one plane, [H][3W] f32 B,G,R, nominal range 0..255
 *
 * Any width and height.  Every input is reduced to the 8-bit BGRX frame the network consumes: the 8-bit formats are a
 * permutation of bytes; a 16-bit word P gives (P + 128) / 257; a 10-bit value p is widened to P = (p << 6) | (p >> 4)
 * first; an f16 / f32 sample v gives floor(clamp(v, 0, 1) * 255 + 0.5) and a BGR96F sample floor(clamp(v, 0, 255) + 0.5)
 * (NaN gives 0, infinities clamp).  This ROUNDS where the reference's castKernel truncates; on integer-valued floats,
 * which is all the reference ever produces, the two agree.  8-bit outputs are a permutation of the BGRX output's bytes.
 * The deep outputs (BGRX64, RGBP10 / 16 / H / S, BGR96F) come from the same source as a 10-bit YUV output ("hbd_from_state"):
 * from the f16 state s, t = s + 0.5, the word is floor(65536 t) saturated (RGBP10: its upper 10 bits), RGBPS is clamp(t, 0,
 * 1), RGBPH that value rounded to f16, BGR96F clamp(t, 0, 1) * 255 -- the frame in float without the truncating cast;
 * from the 8-bit frame (normalize_brightness and output_flow models, or while a source mask is set) the word is 257 u8,
 * RGBPS u8 / 255, BGR96F u8.  tests/rgb_reference.py is the definition, bit for bit.
 *
 * Packed 10-bit (what capture cards, hardware decoders and 10-bit desktop surfaces really hold).  ONE plane of
 * little-endian words each; arithmetic, coefficients and the source of an output are those of the planar format of the
 * same sampling (P210, I410, RGBP10) -- only the words differ:
 *
 *   format          sampling  layout (samples are 10-bit fields, from bit 0 on)              row bytes
 *   JU_FMT_V210     4:2:2     six pixels in four 32-bit words of three samples (bits 0-9,     16 ceil(W / 6)
 *                             10-19, 20-29): Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
 *   JU_FMT_Y210     4:2:2     16-bit words Y0 U Y1 V per pixel pair, the value in the UPPER   4 W
 *                             10 bits, as P010 (ffmpeg y210le)
 *   JU_FMT_Y410     4:4:4     one 32-bit word per pixel: U, Y, V (ffmpeg xv30le)              4 W
 *   JU_FMT_X2RGB10  RGB       one 32-bit word per pixel: B, G, R (ffmpeg x2rgb10le)           4 W
 *   JU_FMT_X2BGR10  RGB       one 32-bit word per pixel: R, G, B (x2bgr10le, R10G10B10A2)     4 W
 *
 * Bits 30-31 of every 32-bit word, the low 6 bits of a Y210 word and the sample slots of V210's last group beyond the
 * width (W mod 6 = 2 or 4) are ignored on input and written 0 on output; all 16 bytes of a last partial V210 group are
 * written, and nothing beyond a row's bytes is read or written (the conventional V210 stride, 128 ceil(W / 48), is the
 * caller's to pass).  V210 and Y210 need an even width; Y410 and the two RGB formats take any size.  Plane addresses and
 * strides are multiples of 4 (Y210: of 2).  Like I410, a Y410 frame carries an 8-bit frame without loss.
 * tests/packed10_reference.py is the definition, bit for bit.
 *
 * Memory: each runtime holds two staging buffers for host planes that fit the largest format (JU_FMT_BGR96F / JU_FMT_RGBPS,
 * 12 bytes per pixel: 24.9 MB for a 1920x1080 output, 12.4 MB more than the YUV formats needed; 1.6 MB for a 480x270
 * input), and ju_process_frames allocates one such slot per frame of a pass on first use (twice the former size).  All
 * are sized once for the largest format: nothing is regrown behind a captured graph.
 *
 * Limits: 8- and 10-bit YUV (no 12- or 16-bit: P016 and friends need an encode to 16-bit codes that is not defined yet;
 * no NV16 / NV21 / NV24; the three chroma sitings above, none for the alpha plane; BT.2020 non-constant luminance only, no
 * PQ / HLG transfer function); RGB without 12-bit and without dithering; alpha (X, and the two top bits of an
 * x2rgb10 / x2bgr10 word) is ignored and written 0 unless ju_set_alpha, below, says otherwise; float inputs are quantised to 8 bits like every input,
 * they do not reach the network unquantised; no YUV or RGB graphics resources (GL textures stay BGRX); look-ahead passes
 * take these frames through ju_process_frames (ju_process_batch and ju_prepare_batch take ju_image, i.e. BGRX) and
 * group passes through ju_process_group_frames (ju_process_group takes ju_image); the C++ plugin surface
 * (JoshUpscale/core.h) is unchanged and takes BGRX only. */
enum { JU_FMT_BGRX = 0, JU_FMT_I420 = 1, JU_FMT_NV12 = 2, JU_FMT_P010 = 3, JU_FMT_I010 = 4 };
enum {
	JU_FMT_YUY2 = 16, JU_FMT_UYVY = 17, JU_FMT_I422 = 18, JU_FMT_P210 = 19, JU_FMT_I210 = 20,
	JU_FMT_I444 = 24, JU_FMT_I410 = 25
};
enum {
	JU_FMT_BGR24 = 32, JU_FMT_RGB24 = 33, JU_FMT_RGBX = 34, JU_FMT_BGRX64 = 35, JU_FMT_RGBP8 = 36, JU_FMT_RGBP10 = 37,
	JU_FMT_RGBP16 = 38, JU_FMT_RGBPH = 39, JU_FMT_RGBPS = 40, JU_FMT_BGR96F = 41
};
enum { JU_FMT_X2BGR10 = 44, JU_FMT_X2RGB10 = 45, JU_FMT_V210 = 48, JU_FMT_Y210 = 49, JU_FMT_Y410 = 50 }; /* packed 10-bit */
enum {
	JU_CS_BT601_LIMITED = 0, JU_CS_BT601_FULL = 1, JU_CS_BT709_LIMITED = 2, JU_CS_BT709_FULL = 3,
	JU_CS_BT2020_LIMITED = 4, JU_CS_BT2020_FULL = 5
};
enum { JU_CHROMA_LEFT = 0, JU_CHROMA_CENTER = 1 << 8, JU_CHROMA_TOPLEFT = 2 << 8 }; /* or-ed into ju_frame.colorspace */

typedef struct ju_frame {
	int format;            /* JU_FMT_* */
	int colorspace;        /* JU_CS_* | JU_CHROMA_*; ignored for JU_FMT_BGRX and the RGB formats (32..45) */
	uint8_t location;      /* JU_LOC_CPU or JU_LOC_DEVICE (BGRX: any location a ju_image takes) */
	size_t width, height;  /* in pixels (luma); even for the 4:2:0 formats, an even width for 4:2:2 */
	void *planes[3];       /* BGRX, YUY2, UYVY and the packed RGB formats: [0]; planar formats: Y, U, V or R, G, B; NV12 /
	                          P010 / P210: Y, interleaved UV (U first); planes beyond a format's count are not read */
	ptrdiff_t strides[3];  /* BYTES per row of each plane (first logical row at planes[k]), any sign,
	                          |stride| >= the plane's row bytes: Y = width, U / V = width / 2 (4:4:4: width), UV = width,
	                          YUY2 / UYVY = 2 width, BGRX = 4 width; the 10-bit formats: twice that; RGB: width x 3 (BGR24 /
	                          RGB24), 4 (RGBX), 8 (BGRX64), 12 (BGR96F), planar width x 1, 2 or 4; packed 10-bit: V210
	                          16 ceil(width / 6), Y210 / Y410 / X2RGB10 / X2BGR10 4 width.  Plane addresses and strides are
	                          multiples of 2 for 16-bit and f16 samples and of 4 for f32 samples and 32-bit words */
} ju_frame;

/* Replaces createRuntime(int deviceId, const std::filesystem::path &modelPath)
 * (core/public/JoshUpscale/core.h:91-92, core/src/core.cc:153-175, 197-199):
 * reads the whole model file, selects the device for the duration of the call,
 * builds the engine.  The file is this runtime's .jupw container
 * (joshupscale_amd/model_file.py), not a TensorRT engine. */
JU_API int ju_create(int device_id, const char *model_path, ju_runtime **out_runtime);

/* Same, from model bytes already in memory (what TensorRTBackend's constructor
 * takes: core/src/tensorrt_backend.cc:117).  dtype: JU_DTYPE_*.  Used by the
 * multi-GPU launcher after the RCCL weight broadcast. */
JU_API int ju_create_from_memory(int device_id, const void *model_bytes, size_t model_size,
    int dtype, ju_runtime **out_runtime);

/* Parses and checks a model container WITHOUT touching a device: header ranges,
 * tensor table bounds, presence and shape of every layer's variables, the channel
 * chain of the graph, BatchNorm folding.  The same code runs first inside
 * ju_create*; this entry point lets a caller (or a CI job on a box without a GPU)
 * reject a bad or hostile file early.  No reference counterpart: TensorRT's
 * deserializeCudaEngine is the validator there (core/src/tensorrt_backend.cc:145-148).
 * JU_OK, or JU_ERR_INVALID_ARGUMENT with the reason in ju_last_error(). */
JU_API int ju_validate_model(const void *model_bytes, size_t model_size);

/* Replaces Runtime::~Runtime via delete (core.h:65-66). NULL is a no-op. */
JU_API void ju_destroy(ju_runtime *runtime);

/* Replaces Runtime::processImage(const Image&, const Image&) (core.h:68-69,
 * core/src/core.cc:177-189, core/src/tensorrt_backend.cc:270-278): stage-in,
 * one recurrent step, stage-out, stream synchronise, state ping-pong.
 * Unlike the reference (assert only, core.cc:179-182) wrong sizes are an
 * error (JU_ERR_INVALID_ARGUMENT). */
JU_API int ju_process(ju_runtime *runtime, const ju_image *input, const ju_image *output);

/* Frame look-ahead (no reference counterpart; the reference's callers hand over one frame at a time,
 * avisynth_plugin/src/main.cc:113-144): `count` CONSECUTIVE frames of the stream in one synchronous call.
 * outputs[i] receives exactly the bytes ju_process(inputs[i], outputs[i]) called in order would have written,
 * and the recurrent state afterwards is the same -- but ALL inputs must hold their pixels when the call is made
 * (an input that overlaps the OUTPUT of an earlier frame of the call -- to be read after that write, frame by frame --
 * simply starts a new pass, and so does an output that overlaps an earlier frame's INPUT).
 * The flow net reads LR frames only, never the HR state, so the runtime computes the flow fields of up to 8 frames in
 * ONE pass of the flow net's launches, which fill the chip where one frame's do not (-40 % flow time per frame at
 * 480x270); warp, tower and tail stay strictly frame by frame.  JU_LOC_DEVICE frames are read and written in place;
 * host frames (JU_LOC_CPU) ride in the same passes -- every input uploaded up front, each output copied out while the
 * next frame's kernels run (pageable memory; nothing of the caller's is page-locked).  Frames a pass cannot take (GL
 * resources, a model without the one-launch flow plan) simply run as ju_process does.  For callers that can read
 * ahead: a file transcoder, an AviSynth filter fetching child frames n .. n+7.
 * ju_set_lookahead caps the frames per pass (1 = off); its default is 8, or JU_LOOKAHEAD=<1..8> at creation. */
JU_API int ju_process_batch(ju_runtime *runtime, const ju_image *inputs, const ju_image *outputs, int count);
/* Frames per look-ahead pass of ju_process_batch for THIS runtime, 1 (every frame as ju_process does) .. 8; values
 * outside are clamped.  Passes registered with ju_prepare_batch that are longer than the new cap are forgotten; RAISING
 * the cap after passes have run or been registered re-allocates the passes' tensors, and every pass graph is then
 * captured again at its next use (set the cap once, before ju_prepare_batch).  The
 * setter is what a host application uses; the JU_LOOKAHEAD environment variable only sets the default of runtimes
 * created afterwards (one process, several filters: each sets its own). */
JU_API int ju_set_lookahead(ju_runtime *runtime, int frames);
/* What ju_prepare_frames is to ju_process: registers a tuple of 2 .. cap (ju_set_lookahead) frame buffers -- device or host -- the
 * caller is going to hand to ju_process_batch as one pass; its hipGraphs (one per binding set) are captured now,
 * nothing executes.  Unregistered tuples are captured at their second use.  *captured (optional) = graphs captured
 * by this call; 0 for a tuple that will not run as one pass. */
JU_API int ju_prepare_batch(ju_runtime *runtime, const ju_image *inputs, const ju_image *outputs, int count, int *captured);

/* Several streams on one GPU (no reference counterpart): one frame for each of `count` runtimes, synchronously -- the
 * same bytes, in every output and in every runtime's recurrent state and frame history, as
 * ju_process(runtimes[i], &inputs[i], &outputs[i]) for i = 0 .. count-1.  For a server of live streams (several OBS
 * sources, one runtime per incoming video): it cannot read ahead in one stream, but it holds one frame of every stream at
 * each tick, and their flow nets are as independent as a look-ahead pass's.  So runtimes[0], the lead, runs the flow
 * net's launches ONCE over up to its ju_set_lookahead cap (default 8) of the frames, each with its own runtime's frame
 * history, and then every runtime's warp, tower and tail in turn -- all on the lead's stream, under one synchronisation.
 * Longer calls split into consecutive passes.
 * Members: distinct runtimes on one device, created from byte-identical model data with the same dtype (ju_get_dtype).
 * JU_ERR_INVALID_ARGUMENT, checked before anything is launched (a refused call changes no runtime's state): a NULL
 * pointer, count < 0, a runtime twice, runtimes that do not match, an image of the wrong size or |stride| or an
 * unknown location.  count == 0 does nothing; count == 1 is ju_process.
 * Member by member, as ju_process calls in list order (same bytes, no pass): models without the look-ahead's one-launch
 * flow plan (flow res-net, normalize_brightness) or a lead whose look-ahead is unavailable, and any call in which an
 * output overlaps an input of the call (host and device addresses apart).  Images a pass cannot take (GL resources,
 * JU_LOC_DEVICE images off 4-byte (input) / 8-byte (output) alignment) run on their own after the pass.  Host images
 * ride in the pass as in ju_process_batch.  Flow-free models: the pass is the members' generator programs.
 * Work a member has enqueued (ju_enqueue) runs before its frame; the runtimes may be driven by other calls between
 * group calls (ju_process, ju_process_batch, ju_reset), each by one thread at a time.  Memory: the lead holds the pass's
 * flow tensors -- those of ju_process_batch, about 210 MB at 480x270 for 8 frames, shared with its look-ahead
 * passes; the other members allocate nothing.  ju_get_stat "group_frames": frames a runtime got from group passes.
 * A member whose scene detector is on runs on its own unless it asked to ride (ju_set_scene_group); a member under a
 * source size, an output size or a mask runs on its own, on the staged single-frame route, unless it asked to ride
 * (ju_set_stage_group). */
JU_API int ju_process_group(ju_runtime *const *runtimes, const ju_image *inputs, const ju_image *outputs, int count);
/* ju_process_group on frames of any format: one frame for each of `count` runtimes, synchronously.  Every plane of every
 * output -- and nothing around it --, every member's recurrent state, frame history and f16 state are those of
 * ju_process_frame(runtimes[i], &inputs[i], &outputs[i]) for i = 0 .. count-1.  For the stream server whose decoders hand
 * over NV12 / P010 and whose capture cards hand over YUY2 / v210.  Formats, colour spaces, locations (host or device
 * planes) and strides of any sign are independent per member and per side, as in ju_process_frames; a call of BGRX frames
 * only behaves as ju_process_group with the same pointers.
 * Membership, passes and the member-by-member cases are ju_process_group's; a member's pair rides in a pass where a
 * look-ahead pass of ju_process_frames would take it, and otherwise runs on its own behind the pass.  An output plane over
 * any input plane of any member of the call (same address space) sends the whole call member by member in list order.
 * Inside a pass host planes are uploaded up front into the lead's slots, ONE launch in front of the flow net's decodes
 * every non-BGRX input of the pass, each member's output is encoded behind that member's own steps on the lead's stream
 * -- a deep format (P010, BGRX64, RGBPH, Y410, ...) of a runtime with "hbd_from_state" 1 from THAT member's f16 state --
 * and host outputs are copied out while the next member's kernels run.  Memory: the lead holds one staging slot per
 * member of a pass and side in use (as ju_process_frames does per frame).
 * JU_ERR_INVALID_ARGUMENT: whatever ju_process_frame refuses, for ANY member; a NULL array, count < 0, a runtime twice,
 * runtimes that do not match.  Every pair is checked before anything is launched or uploaded, the message names the
 * member's index, and no runtime's state, frame history, detector memory or stats change.  count == 0 does nothing;
 * count == 1 is ju_process_frame.
 * ju_get_stat "group_yuv_frames": frames of a runtime that went through a group pass with a non-BGRX side (also counted
 * by "group_frames").
 * Members under a source size, an output size or a mask stay on the staged single-frame route unless they asked to ride
 * (ju_set_stage_group, behind ju_set_stage_lookahead below): the pass then carries their stages.
 * Not provided: graph capture of group passes (they are eager launches); a ju_prepare_* counterpart; the C++ plugin
 * surface. */
JU_API int ju_process_group_frames(ju_runtime *const *runtimes, const ju_frame *inputs, const ju_frame *outputs, int count);

/* Asynchronous form for JU_LOC_DEVICE images: enqueues the same work on the
 * runtime's stream and returns; ju_synchronize() waits.  Frames are still
 * strictly ordered (the recurrence is carried by stream order). */
JU_API int ju_enqueue(ju_runtime *runtime, const ju_image *input, const ju_image *output);
JU_API int ju_synchronize(ju_runtime *runtime);

/* One step of the stream on frames of any format (ju_frame; synchronous, like ju_process).  A pair of BGRX frames
 * behaves exactly as ju_process with the same pointers, strides and locations (GL resources and the direct device path
 * included).  Where a side is YUV its conversion kernel replaces that side's staging copy; host planes are uploaded /
 * copied out plane by plane (4:2:0 moves 1.5 bytes per pixel over PCIe instead of BGRX's 4).
 * JU_ERR_INVALID_ARGUMENT, checked before anything is launched (a refused call leaves the runtime and its state as
 * they were): an odd width or height of a YUV frame, a size other than the runtime's, a NULL plane, an unknown format
 * or colour space, a YUV frame at JU_LOC_GRAPHICS_RESOURCE, a |stride| smaller than the plane's row. */
JU_API int ju_process_frame(ju_runtime *runtime, const ju_frame *input, const ju_frame *output);
/* Frame look-ahead on frames of any format: `count` CONSECUTIVE frames of the stream in one synchronous call.
 * outputs[i] receives exactly the bytes ju_process_frame(&inputs[i], &outputs[i]) called in order would have written --
 * every plane, and nothing around it -- and the recurrent state and frame history afterwards are the same; ALL inputs
 * must hold their pixels when the call is made.  For the transcoder that reads ahead AND holds NV12 / I420: inside a pass
 * a host 4:2:0 frame pair moves 3.3 MB over PCIe instead of BGRX's 8.8 MB, the outputs' planes copied out while the next
 * frame's kernels run.  Formats, colour spaces, locations and strides (any sign) are independent per frame and per side,
 * as in ju_process_frame; a call of BGRX frames only behaves as ju_process_batch.
 * Passes are those of ju_process_batch: at most ju_set_lookahead frames each, longer calls split into consecutive
 * passes; a frame a pass cannot take (a GL resource, a JU_LOC_DEVICE BGRX image off 4-byte (input) / 8-byte (output)
 * alignment, any frame of a model without the one-launch flow plan) runs on its own in stream order, as
 * ju_process_frame would run it, and the passes continue behind it.  A frame with an input plane over an output plane of
 * an earlier frame of the pass (same address space), or an output plane over an earlier input plane, starts a new pass.
 * The YUV inputs of a pass are decoded by ONE launch in front of the flow net's; every YUV output is encoded behind its
 * frame's tail.  Device planes are read and written in place; nothing of the caller's is page-locked.
 * JU_ERR_INVALID_ARGUMENT: a NULL array or count < 0; and whatever ju_process_frame refuses, for ANY frame of the call --
 * every pair is checked before anything is launched or uploaded, the message names the frame's index, and the runtime
 * and its state stay as they were.  count == 0 does nothing.
 * ju_get_stat "lookahead_yuv_frames": frames with a YUV side that went through passes (also counted by
 * "lookahead_frames" and, with a host side, "lookahead_host_frames").
 * Not provided: a ju_prepare_* counterpart (an unregistered tuple of device planes is captured at its second use, as in
 * ju_process_batch; all-host passes of one shape share one graph); the C++ plugin surface.  (Group passes take these
 * frames through ju_process_group_frames.) */
JU_API int ju_process_frames(ju_runtime *runtime, const ju_frame *inputs, const ju_frame *outputs, int count);
/* Asynchronous form (like ju_enqueue): JU_LOC_DEVICE frames only -- a host frame is JU_ERR_INVALID_ARGUMENT;
 * ju_synchronize waits. */
JU_API int ju_enqueue_frame(ju_runtime *runtime, const ju_frame *input, const ju_frame *output);

/* Registers a pair of JU_LOC_DEVICE frame buffers the caller is going to pass to ju_process /
 * ju_enqueue: the hipGraphs of the pair (one per binding set) are captured NOW, so that no
 * later call captures anything -- the reference captures its two graphs in the constructor
 * (core/src/tensorrt_backend.cc:257-263), never inside process (:270-278).  Nothing executes
 * and the buffers are not read or written.  Callers reuse a handful of buffers (OBS: one
 * texture pair, obs_plugin/src/filter.cc:242-279); a caller that does not register still gets
 * a graph from the second use of a pair on.  JU_LOC_CPU / graphics-resource images need
 * nothing (their frames go through the staging buffers whose graphs exist from ju_create on):
 * the call checks the sizes and returns.  *captured (may be NULL) receives the number of
 * graphs captured by this call: 2 for a new device pair, 0 otherwise.  Up to 256 pairs stay
 * registered; beyond that the pair used least recently is forgotten with its graphs. */
JU_API int ju_prepare_frames(ju_runtime *runtime, const ju_image *input, const ju_image *output, int *captured);

/* Replaces Runtime::getInputWidth/Height, getOutputWidth/Height (core.h:71-82). */
JU_API int ju_get_size(const ju_runtime *runtime, size_t *input_width, size_t *input_height,
    size_t *output_width, size_t *output_height);

/* Zeroes the recurrent state; equivalent to destroying and recreating the
 * runtime as the OBS filter does on a model switch (obs_plugin/src/filter.cc:146-151). */
JU_API int ju_reset(ju_runtime *runtime);

/* ---- sources of any size, masked pass-through (docs/source_stage.md) ------------------------------------------------
 * What the reference's only caller of its shipped models, the OBS filter, does around processImage in its graphics API:
 * it draws a source of any size into the model's input texture (obs_plugin/src/filter.cc:351-379) and draws the
 * point-sampled source back over the upscaled frame through a mask, so that HUD and text stay the crisp source
 * (filter.cc:215-217, 393-402, obs_plugin/data/effects/blend.effect, obs_plugin/data/mask.png).  Here both are kernels
 * inside the runtime, in integers, defined exactly (docs/source_stage.md; tests/source_reference.py).  Both settings are
 * opt-in and per runtime; with neither set every entry point behaves byte for byte as without them.  ju_reset keeps both.
 *
 * ju_set_source_size: input frames are src_width x src_height from now on -- on EVERY entry point, exactly that size
 * (YUV: even), anything else is JU_ERR_INVALID_ARGUMENT before anything is launched -- and are scaled to the model's
 * input on the GPU: out = (sum qy qx src + 2^23) >> 24 with 12-bit triangle-filter coefficients (Pillow's BILINEAR
 * before its quantisation), X = 0; a source of the model's size passes through byte for byte.  A YUV source is decoded
 * at source size by the conversion of ju_process_frame, unchanged, then scaled.  Host sources upload at source size.
 * (0, 0) turns it off.  filter: JU_SCALE_TRIANGLE (the above), JU_SCALE_CATMULL_ROM (the bicubic of Pillow's BICUBIC,
 * a = -0.5) or JU_SCALE_MITCHELL (Mitchell-Netravali, B = C = 1/3); the value 1 is reserved and refused, as is every other
 * value.  The cubic filters have negative coefficients, so their result is clamped: out = clamp((sum qy qx src + 2^23) >>
 * 24, 0, 255), nothing rounded or clipped between the axes (docs/source_stage.md "Filters";
 * tests/scale_filter_reference.py).  Catmull-Rom interpolates: a source of the model's size passes through byte for
 * byte, as with the triangle.  Mitchell does not: it filters (softens) such a source too.  Limits
 * (JU_ERR_INVALID_ARGUMENT): each source axis 2 .. 8192, at least a 16th of the model's input axis and at most 16 times
 * it -- 8 times with a cubic filter, whose support is twice as wide (at most 33 taps per axis).
 * ju_get_size keeps reporting the model's sizes; ju_get_source_size reports (0, 0) while off.
 *
 * ju_set_source_mask: a BGRX image of any size (1 .. 16384 per axis), JU_LOC_CPU or JU_LOC_DEVICE, copied to device
 * memory by the call; NULL removes it.  For output pixel (x, y) of the OW x OH frame the source texel is
 * (floor((2x+1) SW / (2 OW)), floor((2y+1) SH / (2 OH))) -- point sampled, the source being the (decoded) frame at source
 * size, or the model-size input frame while no source size is set -- the mask texel likewise with the mask's size,
 * a = 765 - (Rm + Gm + Bm), out = (src a + gen (765 - a) + 382) / 765 per channel, X = 0: a white mask shows the network's
 * frame, a black one the source.  The blend touches only the frame handed to the caller: recurrent state, frame history
 * and f16 state are those of the unmasked run.  While a mask is set a JU_FMT_P010 / JU_FMT_I010 output is encoded from
 * the blended 8-bit frame (257 x u8), whatever "hbd_from_state" says -- that stat keeps reporting the model's property.
 *
 * While either is set every frame of ju_process, ju_enqueue, ju_process_frame, ju_enqueue_frame, ju_process_frames,
 * ju_process_batch, ju_process_group and the C++ processImage runs on its own, in stream order, through the runtime's
 * staging buffers (scale, the staged graph, blend, stage-out): no direct device path, no look-ahead or group pass
 * ("lookahead_frames" / "group_frames" do not count them, "source_stage_frames" does), ju_prepare_frames /
 * ju_prepare_batch capture nothing.  JU_LOC_GRAPHICS_RESOURCE inputs are refused while a source size is set (outputs,
 * and inputs under a mask alone, are taken).  Turning both off restores the other paths.  ju_set_stage_lookahead
 * (below, behind ju_set_output_size) lifts this for the look-ahead passes of ju_process_batch and ju_process_frames,
 * ju_set_stage_group (behind it) for the group passes of ju_process_group and ju_process_group_frames.
 * Not provided: scaled or masked frames inside group passes of a runtime that has not asked to ride (the default:
 * ju_set_stage_group(rt, 1), below, provides them); Lanczos or any other filter whose weights
 * need a transcendental function (they would not be defined bit for bit: docs/source_stage.md); OBS's own
 * OBS_EFFECT_BILINEAR_LOWRES arithmetic (it is not in the reference tree).  The scaler on the output side is
 * ju_set_output_size, below. */
enum { JU_SCALE_TRIANGLE = 0, JU_SCALE_CATMULL_ROM = 2, JU_SCALE_MITCHELL = 3 }; /* (1: reserved, refused) */
JU_API int ju_set_source_size(ju_runtime *runtime, size_t src_width, size_t src_height, int filter);
JU_API int ju_get_source_size(const ju_runtime *runtime, size_t *src_width, size_t *src_height);
JU_API int ju_set_source_mask(ju_runtime *runtime, const ju_image *mask);

/* ---- an output size: the upscaled frame at any size (docs/output_stage.md) ----------------------------------------------
 * The models hand their frame back at exactly 4 x their input; the reference's OBS caller resizes it with OBS's canvas
 * scaling, behind processImage, on the GPU.  A transcoder, a stream server or an AviSynth script has no graphics API to
 * do that with, so the runtime scales the frame itself.  Opt-in and per runtime; with no output size set every entry
 * point behaves byte for byte as without it.  ju_reset keeps the setting.
 *
 * ju_set_output_size: output frames are width x height from now on -- on EVERY entry point, exactly that size (the YUV
 * parity rules apply to it), anything else is JU_ERR_INVALID_ARGUMENT before anything is launched.  The frame is scaled
 * behind the network and the mask blend by the source stage's filter with the output axes' tables:
 * out = (sum qy qx v + 2^23) >> 24, an output of the model's size passing through unchanged.
 *   8-bit formats, and every format while a mask is set or "hbd_from_state" is 0: v is the 8-bit BGRX frame (after the
 *   blend); deep formats are then encoded from the scaled 8-bit frame (257 x u8), as without an output size.
 *   Deep formats otherwise (JU_FMT_P010, I010, P210, I210, I410, BGRX64, RGBP10, RGBP16, RGBPH, RGBPS, BGR96F and the five
 *   packed 10-bit formats): v is the
 *   state's 16-bit sample P = floor((s + 0.5) * 65536), saturated; the scaled P is encoded -- 10-bit YUV as from the state,
 *   16-bit words P, 10-bit words P >> 6, unit floats f32(P) / 65535 (RGBPH: that as f16), BGR96F f32(P) / 257.
 * (0, 0) turns it off.  filter: JU_SCALE_TRIANGLE, JU_SCALE_CATMULL_ROM or JU_SCALE_MITCHELL, as for ju_set_source_size
 * (1 and every other value: refused); with a cubic filter out = clamp((sum qy qx v + 2^23) >> 24, 0, top), top = 255 for
 * the 8-bit frame and 65535 for P.  An output of the model's size passes through unchanged with the triangle and with
 * Catmull-Rom; Mitchell filters it.  Limits (JU_ERR_INVALID_ARGUMENT): each axis 2 .. 16384, at most 16 times the model's
 * output axis and at least a 16th of it -- an 8th with a cubic filter.  ju_get_size keeps reporting the model's sizes;
 * ju_get_output_size reports (0, 0) while off.  Recurrent state, frame history and flow inputs are the unscaled run's.
 *
 * While it is set frames are routed as for a source size: one by one through the staging buffers, no direct device path,
 * no look-ahead or group pass ("source_stage_frames" counts them), ju_prepare_* capture nothing.  A JU_LOC_DEVICE BGRX
 * output is written in place, any alignment and signed stride.  JU_LOC_GRAPHICS_RESOURCE outputs are refused.
 * ju_get_stat: "output_scaled" (1 / 0), "output_filter" (the JU_SCALE_* value in effect, 0 while off).
 * ju_set_stage_lookahead, below, lifts the "no look-ahead pass" for ju_process_batch and ju_process_frames, and
 * ju_set_stage_group the "no group pass" for ju_process_group and ju_process_group_frames. */
JU_API int ju_set_output_size(ju_runtime *runtime, size_t width, size_t height, int filter);
JU_API int ju_get_output_size(const ju_runtime *runtime, size_t *width, size_t *height);

/* ---- the alpha channel: opaque, or scaled from the source (docs/alpha.md) -----------------------------------------------
 * Every four-sample format has an alpha slot -- byte 3 of JU_FMT_BGRX and JU_FMT_RGBX, word 3 of JU_FMT_BGRX64, the two
 * top bits of JU_FMT_X2RGB10 and JU_FMT_X2BGR10 -- which the reference ignores on input and writes 0 on output.
 * ju_set_alpha says what output frames hold there.  Opt-in and per runtime; ju_reset keeps the setting.
 *   JU_ALPHA_ZERO (the default): 0 -- every route byte for byte, launch for launch and stat for stat as without the call.
 *   JU_ALPHA_OPAQUE: the format's top code, 255 / 65535 / 3, in every output frame that has a slot.
 *   JU_ALPHA_SOURCE: the input frame's alpha, scaled on the GPU by the project's exact integer scaler from the input
 *     frame's size (the source size if one is set, else the model's input) STRAIGHT to the output frame's size (the
 *     output size if one is set, else the model's output), never through the model's size.  The 16-bit plane A of the
 *     input: 257 a of a byte, a BGRX64 word itself, 21845 a of a two-bit code, 65535 for a format without a slot (every
 *     YUV format, BGR24 / RGB24, the planar RGB formats, BGR96F).  A' = (sum qy qx A + 2^23) >> 24 with the tables of
 *     `filter` (clamped to 0 .. 65535 with a cubic filter).  The slot: (A' + 128) / 257 of a byte, A' of a word,
 *     (A' + 10922) / 21845 of two bits.  Equal sizes under the triangle or Catmull-Rom give the input's alpha back code
 *     for code.  tests/alpha_reference.py is the definition, in integers.
 * filter: JU_SCALE_TRIANGLE, JU_SCALE_CATMULL_ROM or JU_SCALE_MITCHELL (anything else: refused); ignored, but still
 * checked, in the first two modes.  Alpha is independent of everything else: colour samples, state, frame history,
 * detector records and deep outputs are those of the same runtime in mode 0; the mask does not touch alpha.  An output
 * format without a slot gets nothing and nothing is launched for it.
 * Limits (JU_ERR_INVALID_ARGUMENT, the setting as it was): a mode or a filter out of range; under JU_ALPHA_SOURCE each
 * axis of both frame sizes 2 .. 16384, the input at most 16 times the output (8 with a cubic filter) and the output at
 * most 16 times the input.  A source size and an output size can together leave these limits (16:1 in, 1:16 out):
 * whichever of ju_set_alpha, ju_set_source_size and ju_set_output_size would do so is refused, the message names alpha
 * and both sizes, and all three settings stay as they were.  Under JU_ALPHA_SOURCE a JU_LOC_DEVICE output that overlaps
 * the JU_LOC_DEVICE input is refused before anything is launched (the alpha is read behind the frame's colour).
 * Routing: while the mode is not JU_ALPHA_ZERO frames of every entry point run one by one through the staging buffers, in
 * stream order, with one more launch behind the frame's colour and in front of any copy to the host; no direct device
 * path, no look-ahead or group pass whatever ju_set_stage_lookahead, ju_set_stage_group and the scene settings say (in a
 * group call such a runtime runs on its own behind the pass), ju_prepare_* capture nothing -- unless ju_set_alpha_lookahead
 * / ju_set_alpha_group, below, let the passes carry the launch.  JU_ALPHA_ZERO restores all of
 * them.  The setter waits for the stream.  ju_get_stat: "alpha_mode", "alpha_filter", "alpha_frames" (frames whose alpha
 * slot these launches wrote).  Not covered: premultiplied alpha, the direct device path of single frames, the C++ surface. */
enum { JU_ALPHA_ZERO = 0, JU_ALPHA_OPAQUE = 1, JU_ALPHA_SOURCE = 2 };
JU_API int ju_set_alpha(ju_runtime *runtime, int mode, int filter);
JU_API int ju_get_alpha(const ju_runtime *runtime, int *mode, int *filter);

/* ---- alpha inside look-ahead passes and group passes (docs/alpha.md: "Passes") ------------------------------------------
 * ju_set_alpha_lookahead(rt, 1): while the alpha mode is not JU_ALPHA_ZERO, ju_process_batch and ju_process_frames form
 * their look-ahead passes again, under all their usual rules -- the mode no longer decides; the stage and scene
 * conditions decide as for a runtime in mode 0, so a runtime under a source size, a mask or an output size still needs
 * ju_set_stage_lookahead, and a detecting one ju_set_scene_lookahead.  Inside a pass the frame's one alpha launch follows
 * its colour -- the tail, the mask blend, the output scaler and the encode -- in stream order, in front of the copy of a
 * host frame.  It is the launch of the single-frame route: same mode, filter and tables, same source and sink rows by
 * format and location (a JU_LOC_DEVICE frame where it is, a host frame in the pass's upload slot, plane 0 of an RGBX,
 * BGRX64 or X2 frame; a format without a slot reads as opaque on the input side and gets no launch on the output side).
 * Every output byte, the state and the frame history equal those of the same frames sent one by one.  The default is 0:
 * such frames run one by one, as described above, byte for byte and stat for stat.  A value other than 0 or 1 is
 * JU_ERR_INVALID_ARGUMENT ("ju_set_alpha_lookahead: on must be 0 or 1, got N") and leaves the setting as it was; the call
 * waits for the stream; ju_reset and ju_set_alpha keep the setting.
 * Graphs: a captured pass bakes in the mode, the filter and the tables; ju_set_alpha, this call and every size setter that
 * rebuilds the alpha scaler drop the graphs of the passes that carry alpha (captured again at the second sighting of their
 * buffers).  With the setting on ju_prepare_batch captures as in mode 0 (that is, while no stage setting is on);
 * ju_prepare_frames captures nothing, as before.  A pass that has to run again (the resident tower reported) runs its
 * frames one by one through the staged route, which writes their alpha.
 * Unchanged by the setting: ju_process, ju_enqueue, ju_process_frame, ju_enqueue_frame and the C++ processImage keep the
 * staged single-frame route; under JU_ALPHA_SOURCE a JU_LOC_DEVICE output over its own JU_LOC_DEVICE input stays refused.
 * ju_get_stat: "alpha_lookahead" (1 / 0) and "lookahead_alpha_frames", the frames whose slot was written inside a pass;
 * "alpha_frames" counts them too, each frame once. */
JU_API int ju_set_alpha_lookahead(ju_runtime *runtime, int on); /* default 0 */
/* ju_set_alpha_group(rt, 1): this runtime rides in the passes of ju_process_group and ju_process_group_frames while its
 * alpha mode is not JU_ALPHA_ZERO (under a stage setting it also needs ju_set_stage_group, with the detector on
 * ju_set_scene_group), and the pass makes its alpha launch behind its own steps, blend, scaler and encode, on the lead's
 * stream, with THIS member's mode, filter, tables and sizes -- never the lead's.  For every member the bytes, the state and
 * the history equal those of ju_process_frame on that member alone.  The default is 0: such a member runs on its own
 * behind the pass.  Per member; independent of ju_set_alpha_lookahead; a value other than 0 or 1 is
 * JU_ERR_INVALID_ARGUMENT ("ju_set_alpha_group: on must be 0 or 1, got N") and leaves the setting as it was; the call waits
 * for the stream; ju_reset and ju_set_alpha keep the setting.  ju_get_stat: "alpha_group" (1 / 0) and
 * "group_alpha_frames", this runtime's frames whose slot was written inside a group pass ("alpha_frames" counts them too). */
JU_API int ju_set_alpha_group(ju_runtime *runtime, int on); /* default 0 */

/* ---- scaled and masked frames inside look-ahead passes (docs/source_stage.md, docs/output_stage.md: "Passes") ----------
 * ju_set_stage_lookahead(rt, 1): while a source size, a mask or an output size is set, ju_process_batch and
 * ju_process_frames form their look-ahead passes again, under all their usual rules (the cap, the overlap splitter, host
 * and YUV frames, the scene detector with ju_set_scene_lookahead), and the passes carry the stages.  Every output byte,
 * the state and the frame history equal those of the same frames sent one by one.  The default is 0: such frames run one
 * by one, as described above, byte for byte and stat for stat.  A value other than 0 or 1 is JU_ERR_INVALID_ARGUMENT
 * ("ju_set_stage_lookahead: on must be 0 or 1, got N"); the call waits for the stream; ju_reset keeps the setting.
 *
 * Eligibility.  A frame of a pass must be the source size on its input side if one is set, else the model's input, and
 * the output size on its output side if one is set, else the model's output.  A JU_LOC_DEVICE BGRX image on a side that
 * a scaler touches is read / written where it is, at any alignment and any signed stride; on a side that no scaler
 * touches it keeps the conditions of the plain passes (input 4-byte, output 8-byte aligned address and stride; direct
 * device access not turned off), else the frame runs on its own.  Host and YUV sides are taken as in plain passes.
 * JU_LOC_GRAPHICS_RESOURCE frames are refused or run one by one, as without the setting.  The size and parity checks of
 * every frame of the call run before anything is launched.
 *
 * Inside a pass: host sources upload at source size and YUV sources are decoded at source size, all in one launch; ONE
 * launch then scales all the pass's sources to the model's input, in front of the scene detector and the flow net, which
 * read exactly the frame they read one by one.  Behind each frame's last kernel, in stream order: the mask blend in
 * place, then the output scaler and the encode by the rules of ju_set_output_size -- a deep format from that frame's own
 * f16 state, or from the blended / scaled 8-bit frame while a mask is set or "hbd_from_state" is 0.
 *
 * Unchanged by the setting: ju_process, ju_enqueue, ju_process_frame, ju_enqueue_frame, ju_process_group (whose passes
 * have a setting of their own, ju_set_stage_group) and the C++ processImage keep the staged single-frame route while a
 * stage is set; ju_prepare_batch / ju_prepare_frames capture
 * nothing while one is (a staged pass captures its graph at the second sighting of its buffers).
 *
 * Memory.  The pass keeps slots per frame of the look-ahead cap, made when first needed at the sizes set and dropped,
 * with the staged passes' graphs, whenever ju_set_source_size, ju_set_source_mask, ju_set_output_size or this call
 * changes anything: a model-size input and output (4 bytes per pixel each), a source-size BGRX frame for a host or YUV
 * source, and for a host or YUV output an 8-bit frame at output size (4 bytes per pixel; 33 MB at 3840x2160) plus, for a
 * deep format from the state, a 16-bit frame (8 bytes per pixel; 66 MB at 3840x2160) -- each times the cap (8).
 *
 * ju_get_stat: "stage_lookahead" (1 / 0) and "lookahead_staged_frames", the frames that went through a pass while a
 * stage setting was on; "lookahead_frames", "lookahead_host_frames" / "lookahead_yuv_frames" and "source_stage_frames"
 * count them too (the last says what a frame went through, not which route it took). */
JU_API int ju_set_stage_lookahead(ju_runtime *runtime, int on);

/* ---- scaled and masked members inside group passes (docs/source_stage.md, docs/output_stage.md: "Group passes") ---------
 * For the stream server whose incoming videos are not the model's size: eight 720p sources, each scaled to the model and
 * handed back at 1080p or 2160p, one frame of each at every tick.
 * ju_set_stage_group(rt, 1): this runtime rides in the passes of ju_process_group and ju_process_group_frames while it
 * has a source size, a mask or an output size set, and the pass carries its stages.  Its frame must then be the sizes
 * every entry point already demands of it: its own source size on the input side if one is set, its own output size on
 * the output side if one is set.  For every member, every plane of its output and nothing around it, its recurrent
 * state, frame history, f16 state, detector records and stats (but the counters below) equal those of
 * ju_process_frame(runtimes[i], &inputs[i], &outputs[i]) with the same settings.  The default is 0: such a member runs on
 * its own, as described above, byte for byte and stat for stat.  A value other than 0 or 1 is JU_ERR_INVALID_ARGUMENT
 * ("ju_set_stage_group: on must be 0 or 1, got N"); the call waits for the stream; ju_reset keeps the setting.  It is
 * independent of ju_set_stage_lookahead.
 *
 * The setting is per member and the members are independent: one call may mix plain members, staged members that ride,
 * staged members with the setting off (these run alone, as before) and detecting members (ju_set_scene_group); every
 * member may have its own source size, filter, mask and output size; the lead needs no stage.
 *
 * Eligibility of a riding member's pair is that of a staged look-ahead frame (ju_set_stage_lookahead, above): on a side
 * a scaler of that member touches a JU_LOC_DEVICE BGRX image is taken at any alignment and any signed stride, on a side
 * none touches it keeps the plain pass's alignment conditions, else the member runs on its own; host and YUV sides are
 * taken; JU_LOC_GRAPHICS_RESOURCE frames run alone or are refused, as without the setting.  The call-wide overlap test
 * covers every plane at its true size (source size on the input side, output size on the output side).  All size and
 * parity checks of every member run before anything is launched or uploaded; a refused call changes no runtime.
 *
 * Inside a pass: host planes upload at each member's own source size and ONE launch decodes every non-BGRX input at its
 * own size; ONE launch then scales the sources of all scaled members, each through its own tables and filter, to the
 * model's input, in front of the group scene launch and the flow net, which read exactly the model-size frame they read
 * member by member.  Behind each member's own steps, on the lead's stream: that member's mask blend in place (its source
 * sampled from its own source rows), its output scaler and its encode by the rules of ju_set_output_size -- a deep format
 * from that member's own f16 state, or from the blended / scaled 8-bit frame while it has a mask or "hbd_from_state" is
 * 0.  Host outputs are copied out at output size while the next member's kernels run.  The pass stays synchronous and
 * its launches eager.
 *
 * Memory.  A member contributes one frame per pass, so it owns ONE set of slots (not one per frame of a cap), made when
 * first needed at its own sizes and dropped whenever ju_set_source_size, ju_set_source_mask, ju_set_output_size or this
 * call changes anything for it: under a source size a model-size input (4 bytes per pixel; 0.5 MB at 480x270) and, for
 * a host or non-BGRX source, a source-size BGRX frame (3.7 MB at 1280x720) and its host planes; under an output size a
 * model-size output (8.3 MB at 1920x1080) and, for a host or non-BGRX output, an 8-bit frame at output size (33 MB at
 * 3840x2160) and its host planes plus, for a deep format from the state, a 16-bit frame (66 MB at 3840x2160).  A mask
 * alone needs none.  The slots live in the member: no setter and no ju_destroy touches another runtime's memory.
 *
 * ju_get_stat: "stage_group" (1 / 0) and "group_staged_frames", this runtime's frames that went through a group pass
 * while one of its stage settings was on; "group_frames", "group_yuv_frames" and "source_stage_frames" count them too.
 * Not provided: graph capture of group passes; a ju_prepare_* counterpart; GL resources under a stage; the C++ plugin
 * surface. */
JU_API int ju_set_stage_group(ju_runtime *runtime, int on); /* default 0 */

/* ---- scene cuts: detected on the GPU, the recurrence restarted at them (docs/scene_detect.md) -----------------------------
 * Every frame is built from the previous output warped by a flow field and from three frames of history; across a hard
 * cut all of that belongs to another scene.  ju_reset is the remedy, but the caller has to know where the cuts are and
 * the call waits.  The detector finds them on the GPU, in exact integers, and restarts the recurrence there without a
 * host round trip.  Opt-in and per runtime; with the mode off (the default) every entry point behaves byte for byte as
 * without it.  ju_reset keeps the setting.
 *
 * Definition (tests/scene_reference.py).  c_t: the model-size BGRX frame step t consumes -- behind decoding and the
 * source scaler -- of W x H pixels; the X byte is ignored; N = 3 W H.  S_t = sum |c_t - c_(t-1)| over the N colour bytes,
 * a 64-bit integer, 0 while frame t-1 is not in the detector's memory.  D_t = min(S_t, |S_t - S_(t-1)|) when frames t-1
 * and t-2 both are, else 0 (ffmpeg scdet's score as a raw sum: the first two frames after a start never cut).
 * cut_t = (1000 D_t >= threshold_milli N).  threshold_milli: thousandths of an 8-bit code value per byte, 1 .. 255000;
 * 10000 is scdet's default of 10.  The detector has no predecessor after ju_create, after ju_reset and after a
 * ju_set_scene_detect call that changes the mode; a detected cut does not clear the detector's own memory (the frame
 * after a flash is thereby told from a second cut).
 *
 * JU_SCENE_REPORT: cuts are recorded, no byte of any output or of the state changes.  JU_SCENE_RESET: at a cut the
 * step's recurrent inputs are zeroed on the GPU in front of the step -- the frame, the state and the history are those
 * of a ju_reset called before that frame.  A flow-free model ("recurrent" 0) takes JU_SCENE_RESET as JU_SCENE_REPORT.
 * ju_set_scene_detect waits for the stream; an unknown mode, or a threshold outside 1 .. 255000 while the mode is not
 * off, is JU_ERR_INVALID_ARGUMENT.  The same mode again changes the threshold only.
 * ju_get_scene_info waits for the stream (valid after ju_enqueue and multi-frame calls) and returns the most recent
 * min(count, 64, steps seen) records, oldest first; `step` counts detector steps from 0 at the call that turned the
 * detector on and continues across ju_reset.  A frame refused by its checks does not reach the detector.
 * ju_get_stat: "scene_mode", "scene_frames", "scene_cuts" (cumulative, as of the steps that have completed).
 *
 * While the mode is not off look-ahead and group passes are not formed (a pass computes the flow of all its frames
 * from a history a cut inside it would invalidate): ju_process_batch, ju_process_frames and ju_process_group run such
 * a runtime's frames one by one in stream order ("lookahead_frames" / "group_frames" do not count them), and
 * ju_prepare_batch captures nothing; ju_prepare_frames works as before and the direct device path and its graphs stay
 * in use.  Turning the mode off restores the passes; the two settings below let the passes carry the detector.
 *
 * ju_set_scene_lookahead(rt, 1) lifts that for look-ahead passes: ju_process_batch and ju_process_frames form their
 * passes under all their usual rules (the cap, the overlap splitter, eligibility, host and YUV frames) and
 * ju_prepare_batch captures, while the detector is on.  A pass then carries the detector itself: one launch in front of
 * the flow net's takes the decisions of all its frames on the GPU, and in JU_SCENE_RESET mode the pass applies each cut
 * without a host round trip -- the first flow block builds its history from the frames since the cut and zeros, and a
 * conditional clear in front of each frame zeroes its input state.  Every output byte, the state, the history and every
 * ju_scene_info record equal those of the same frames sent one by one through ju_process / ju_process_frame with the same
 * detector setting.  The default is 0 (the paragraph above); a value other than 0 or 1 is JU_ERR_INVALID_ARGUMENT; the
 * call waits for the stream; ju_reset and ju_set_scene_detect keep the setting.  ju_get_stat: "scene_lookahead" (1 / 0),
 * "scene_pass_frames" (frames whose detector step ran inside a pass; "lookahead_frames" counts them too).  Frames under
 * a source size, an output size or a mask stay one by one unless ju_set_stage_lookahead is set.  Group passes have a
 * setting of their own, whatever this one says:
 *
 * ju_set_scene_group(rt, 1) lets this runtime ride in the passes of ju_process_group and ju_process_group_frames while
 * its detector is on (JU_SCENE_REPORT or JU_SCENE_RESET).  The members of a pass are independent streams, so a pass
 * needs no cut-aware history: ONE launch behind the decode launch and in front of the flow net's takes the decision of
 * every detecting member -- each against its own kept frame, with its own mode and threshold, into its own records --
 * and in JU_SCENE_RESET mode ONE more zeroes the recurrent inputs (state and frame history) of the members that cut, on
 * the GPU.  For every member, every output byte, the state, the history and every ju_scene_info record equal those of the
 * same frames sent through ju_process / ju_process_frame with the same detector setting; step numbers continue from
 * wherever the member stands, and ju_get_scene_info, the cumulative counters and the predecessor bits advance per member
 * as one per-frame step does.  The setting is per member: members with the detector off, with it on and the setting on,
 * and with it on and the setting off (these run alone, as before) may be mixed in one call; the lead needs no detector.
 * The default is 0 (the paragraph above); a value other than 0 or 1 is JU_ERR_INVALID_ARGUMENT; the call waits for the
 * stream; ju_reset and ju_set_scene_detect keep the setting.  ju_get_stat: "scene_group" (1 / 0), "scene_group_frames"
 * (frames whose detector step ran inside a group pass; "group_frames" counts them too). */
enum { JU_SCENE_OFF = 0, JU_SCENE_REPORT = 1, JU_SCENE_RESET = 2 };
typedef struct ju_scene_info {
	uint64_t step, sad, score; /* the detector step, S_t, D_t */
	uint32_t cut, reserved;    /* cut_t (0 / 1) */
} ju_scene_info;
JU_API int ju_set_scene_detect(ju_runtime *runtime, int mode, uint32_t threshold_milli);
JU_API int ju_get_scene_detect(const ju_runtime *runtime, int *mode, uint32_t *threshold_milli);
JU_API int ju_get_scene_info(ju_runtime *runtime, ju_scene_info *out, int count, int *written);
JU_API int ju_set_scene_lookahead(ju_runtime *runtime, int on);
JU_API int ju_set_scene_group(ju_runtime *runtime, int on); /* default 0 */

/* ---- tiled upscaling: sources larger than the model (no reference counterpart: the reference upscales exactly the
 * model's size -- its AviSynth caller "must be in RGB32 format, 480x270") ------------------------------------------------
 * A ju_tiled upscales frames of src_width x src_height to four times that size with a model of W x H: the source is cut
 * into W x H tiles that overlap by at least `overlap` source pixels, every tile is an independent recurrent stream with a
 * runtime of its own, and the tiles' 4W x 4H outputs are blended into the frame across their seams -- cut and blend are
 * one GPU launch each, the tiles advance together as ju_process_group passes (the flow nets of up to 8 tiles in one
 * pass of their launches; more tiles split evenly into several passes).  docs/tiled.md holds the definition:
 *   per axis (S source length, t tile length, ov overlap): n = 1 tiles if S == t, else ceil((S - ov) / (t - ov)), at
 *   x_i = floor(i (S - t) / (n - 1)); between tiles i and i + 1 a linear ramp of 4 ov output pixels centred in their
 *   overlap, tile i alone in front of it and tile i + 1 alone behind it (ov = 0: a hard cut);
 *   out = (sum wy wx v + 32768) >> 16 per byte of B, G, R over the up to four tiles the two axes name, X = 0.
 * A pixel under one tile is that tile's byte; a source of exactly W x H is ONE tile, and its frames are ju_process's
 * byte for byte.  In general every frame equals, byte for byte, the blend of what ju_process gives n runtimes fed the
 * tiles (tests/tiled_reference.py).
 * Limits (JU_ERR_INVALID_ARGUMENT): 0 <= overlap <= min(W, H) / 4; W <= src_width <= 8 W and H <= src_height <= 8 H; at
 * most 64 tiles.  Memory: every tile holds a whole runtime (weights and activations, about what ju_create takes) plus
 * 68 W H bytes of tile frames; host frames and frames that are not BGRX add one staging frame per side. */
typedef struct ju_tiled ju_tiled;
typedef struct ju_tiled_info {
	size_t src_width, src_height, out_width, out_height, tile_width, tile_height;
	int tiles_x, tiles_y, overlap;
} ju_tiled_info;
/* The arguments of ju_create_from_memory (dtype: JU_DTYPE_*), then the source size and the overlap.  The model bytes are
 * checked first, then the limits above -- both before any runtime is created.  *out_tiled is NULL on failure. */
JU_API int ju_tiled_create_from_memory(int device_id, const void *model_bytes, size_t model_size, int dtype,
    size_t src_width, size_t src_height, int overlap, ju_tiled **out_tiled);
/* ju_tiled_create_from_memory on the bytes of a model file, with the container's dtype (JU_ERR_IO: the file). */
JU_API int ju_tiled_create(int device_id, const char *model_path, size_t src_width, size_t src_height, int overlap,
    ju_tiled **out_tiled);
JU_API void ju_tiled_destroy(ju_tiled *tiled); /* NULL: nothing */
/* Zeroes every tile's recurrent state: the next frame is the first of a fresh object. */
JU_API int ju_tiled_reset(ju_tiled *tiled);
/* One frame, synchronously: `input` a BGRX image of src_width x src_height, `output` one of four times that (or of the
 * output size set: ju_tiled_set_output_size below); each
 * JU_LOC_CPU or JU_LOC_DEVICE with a stride of any sign.  A JU_LOC_DEVICE image at a 4-byte-aligned address and stride
 * is read / written where it is; any other goes through a staging frame.
 * JU_ERR_INVALID_ARGUMENT, before anything is launched and with every tile's state unchanged: a NULL pointer, an image
 * that is not exactly that size, |stride| smaller than a row, an unknown location, a graphics resource, an output that
 * overlaps the input (same address space). */
JU_API int ju_tiled_process(ju_tiled *tiled, const ju_image *input, const ju_image *output);
/* ju_tiled_process on frames of any JU_FMT_* format, host or device: the input is decoded at source size by the
 * conversion ju_process_frame uses, the blended 8-bit frame is encoded at output size -- by default also a deep format
 * (P010, BGRX64, ...), which ju_process_frame would take from the f16 state (ju_tiled_set_deep_from_state below).  Refused
 * as above, and whatever ju_process_frame refuses for a frame of that size (an odd size for a subsampled format, an
 * unknown format or colour space, a NULL or misaligned plane, |stride| smaller than a row). */
JU_API int ju_tiled_process_frame(ju_tiled *tiled, const ju_frame *input, const ju_frame *output);
/* Look-ahead passes of a tiled stream (docs/tiled.md "Look-ahead passes"; no reference counterpart): ju_process_batch /
 * ju_process_frames restated for a tiled object.  `count` CONSECUTIVE frames of the tiled stream in one synchronous call:
 * every plane of outputs[i] holds exactly the bytes ju_tiled_process_frame(&inputs[i], &outputs[i]), called in order, would
 * have written, and nothing around those planes is written; every tile's recurrent state and frame history, the
 * detector's memory and records and every counter that frame-by-frame calls advance are the same afterwards -- under
 * ju_tiled_set_deep_from_state, an output size, a source mask and the scene detector in either mode alike.  All inputs
 * must hold their pixels when the call is made.  Formats, colour spaces, locations and strides of either sign are
 * independent per frame and per side; a call of BGRX frames behaves as ju_tiled_process_batch with the same pointers.
 * count == 0 does nothing, count == 1 is ju_tiled_process_frame, and calls longer than the cap split into consecutive
 * passes.  ju_tiled_set_lookahead caps the frames per pass (1 .. 8, clamped; 1 = every frame as ju_tiled_process_frame);
 * the default is the members' look-ahead: 8, or JU_LOOKAHEAD=<1..8> at creation.  ju_tiled_reset keeps the cap.
 * A pass of K frames uploads and decodes its sources up front, cuts all of them into the tiles' inputs in ONE launch
 * (per frame, fused with the detector, while ju_tiled_set_scene_detect is on), then runs per frame the tiles' group
 * passes and the blend; a JU_LOC_CPU output is copied out while the NEXT frame's group passes run.  A frame starts a new
 * pass if one of its input planes overlaps an output plane of an earlier frame of the pass (same address space) or one of
 * its output planes an earlier frame's input plane; outputs may repeat (the same buffer for frames i and i + 2 ends up
 * holding frame i + 2).  Device memory, made at the first pass and sized by the cap: K source slots of 4 src_width
 * src_height bytes, K x tiles tile inputs, and a second staging frame per side in use.
 * JU_ERR_INVALID_ARGUMENT: a NULL array, count < 0, and whatever ju_tiled_process_frame refuses for ANY frame of the call
 * -- every pair is checked before anything is uploaded or launched, the message names the frame ("frame i: ..."), and
 * the object, its tiles, the detector and the stats stay as they were.
 * ju_tiled_get_stat: "lookahead" (the cap), "pass_calls" (passes run), "pass_frames" (frames that ran inside a pass of
 * two or more frames), "pass_split_launches" (multi-frame split launches), "pass_overlapped_copies" (host outputs copied
 * out while a group pass of a later frame was in flight: not where the tiles run one by one, as in a one-tile object). */
JU_API int ju_tiled_process_batch(ju_tiled *tiled, const ju_image *inputs, const ju_image *outputs, int count);
JU_API int ju_tiled_process_frames(ju_tiled *tiled, const ju_frame *inputs, const ju_frame *outputs, int count);
JU_API int ju_tiled_set_lookahead(ju_tiled *tiled, int frames);
/* Deep outputs from the tiles' f16 states (no reference counterpart: the reference has no tiles and writes 8-bit frames).
 * on = 1: a deep output format (P010, I010, P210, I210, I410, V210, Y210, Y410, BGRX64, RGBP10, RGBP16, RGBPH, RGBPS,
 * BGR96F, X2RGB10, X2BGR10) is encoded from the blend of the tiles' states instead of the blended 8-bit frame: with P the
 * 16-bit sample floor((s + 0.5) 65536), saturated, of a tile's state, out16 = (sum wy wx P + 32768) >> 16 per channel over
 * the same weights, and the planes are what ju_process_frame's encode makes of such a 16-bit frame -- so the low bits are
 * the network's, as on every other route (docs/tiled.md "Deep outputs"; tests/tiled_deep_reference.py).  A source of
 * exactly W x H, ONE tile, is encoded straight from that tile's state: ju_process_frame's bytes.  It costs one more frame
 * of 8 bytes per output pixel in device memory, made at the first such frame of two tiles or more.  on = 0 (the default): every
 * format from the 8-bit frame, the bytes of earlier versions.  The setting has no effect on 8-bit formats, on the tiles'
 * states, or for a model whose state is not its frame in float (normalize_brightness, output = "pre_warp":
 * ju_tiled_get_stat "hbd_from_state" 0), whose deep frames stay the 8-bit route's.  ju_tiled_reset keeps it.  Another value
 * is JU_ERR_INVALID_ARGUMENT and leaves the setting as it was. */
JU_API int ju_tiled_set_deep_from_state(ju_tiled *tiled, int on);
/* An output size for tiled frames (docs/tiled.md "An output size"; no reference counterpart: the reference has no tiles and
 * hands out the model's size).  ju_tiled_set_output_size: output frames are width x height from now on, exactly that size
 * (the YUV parity rules apply to it; anything else is JU_ERR_INVALID_ARGUMENT naming "the output size set", before anything
 * is launched and with every tile's state unchanged).  The blended frame of B x Bh = 4 src_width x 4 src_height is scaled
 * by ju_set_output_size's scaler and filters INSIDE the blend's launch: the scaler's vertical pass reads the tiles' outputs
 * (states) and forms each blended sample in registers, so the B x Bh frame is never stored and no buffer of that size is
 * allocated.  By definition (tests/tiled_output_reference.py), with no tolerance:
 *   8-bit frame: the blend rounds to bytes first, (sum wy wx v + 32768) >> 16, and the scaler runs on those bytes,
 *   (sum qy qx v + 2^23) >> 24, clamped to 0 .. 255 with a cubic filter; BGRX is that frame (X = 0), every other format its
 *   encode -- a deep format on this route carries 257 x u8;
 *   16-bit frame, for a deep format while ju_tiled_set_deep_from_state is 1 and "hbd_from_state" is 1: the same two steps
 *   on the 16-bit samples P of the tiles' states, encoded as ju_set_output_size encodes a scaled 16-bit frame.
 * An output size of exactly B x Bh gives the unscaled frame with the triangle and with Catmull-Rom; Mitchell filters it.  A
 * source of exactly W x H, ONE tile, gives byte for byte the frames of ju_process_frame under ju_set_output_size with the
 * same arguments (the float formats included: both sides are f32(P) / 65535 of a 16-bit frame).
 * (0, 0) turns it off (the filter must still be a known one, as for ju_set_output_size).  Limits (JU_ERR_INVALID_ARGUMENT,
 * the message names B x Bh as four times the tiled source size; the setting stays as it was): each axis 2 .. 16384, at
 * most 16 times the blended axis and at least a 16th of it -- an 8th with a cubic filter; filter one of JU_SCALE_TRIANGLE,
 * JU_SCALE_CATMULL_ROM, JU_SCALE_MITCHELL (1 and every other value: refused).  The setter waits for the tiled stream and
 * drops the staging frames, whose sizes follow the output size; ju_tiled_reset keeps the setting.  A JU_LOC_DEVICE BGRX
 * output at a 4-byte-aligned address and stride is written in place, with a stride of either sign.  ju_tiled_get_info keeps
 * reporting out_width = 4 src_width, the blended size, as ju_get_size keeps reporting the model's; tile states, frame
 * history, group passes and the scene detector do not know about the setting.
 * ju_tiled_get_output_size: (0, 0) while off.
 * ju_tiled_get_stat: "output_scaled" (1 / 0), "output_filter" (the JU_SCALE_* value in effect, 0 while off),
 * "output_scaled_frames" (the frames that took a fused blend-and-scale kernel). */
JU_API int ju_tiled_set_output_size(ju_tiled *tiled, size_t width, size_t height, int filter);
JU_API int ju_tiled_get_output_size(const ju_tiled *tiled, size_t *width, size_t *height);
/* A source mask for tiled frames (docs/tiled.md "A mask"; no reference counterpart in the core; the OBS filter's
 * blend.effect: obs_plugin/src/filter.cc:215-217, 393-402, as ju_set_source_mask).  From now on the source frame of each
 * call is drawn back over the blended frame through `mask`, so HUD, subtitles and text stay the crisp source: a BGRX image
 * of any size, each axis 1 .. 16384, JU_LOC_CPU or JU_LOC_DEVICE, any stride of either sign; copied to device memory now.
 * NULL turns it off.  By definition (tests/tiled_mask_reference.py), in integers, with B x Bh = 4 src_width x 4 src_height
 * the blended frame and c the source frame of the call as the split reads it (a device BGRX image in place, a host image as
 * staged, any other format as decoded at source size):
 *   masked = ju_set_source_mask's blend of the blended 8-bit frame: a = 765 - (Bm + Gm + Rm) at the mask texel
 *   floor((2 X + 1) MW / (2 B)), likewise in y; out = (c a + blend (765 - a) + 382) / 765 per byte of B, G, R with c the
 *   source texel (X >> 2, Y >> 2); X = 0; a pixel with a == 0 is the blended pixel unchanged.  The blend rounds to bytes
 *   first, the mask works on those bytes, and under ju_tiled_set_output_size the scaler follows: mask at the blended size,
 *   then the scale, as a plain runtime does.  The blend is applied to the blended sample in registers inside the stitch's
 *   launch -- also the fused blend-and-scale launch, which never stores the blended frame.
 * Every other format is the 8-bit encode of that frame; while a mask is set a deep format is encoded from the 8-bit frame
 * (257 x u8), the rule of ju_process_frame under a mask: ju_tiled_set_deep_from_state is accepted and has no effect, and
 * "deep_state_frames" does not advance.  Tile inputs and states, frame history, group passes and the scene detector do not
 * know about the mask.  A source of exactly W x H, ONE tile, gives the frames of ju_process / ju_process_frame under
 * ju_set_source_mask with the same mask (and ju_set_output_size where one is set).
 * At set time the host computes the box, the rectangle of blended coordinates that holds every pixel whose mask texel is
 * not white (a device mask is read back once for it); outside it the kernels read no mask and no source and do what the
 * unmasked kernels do, and a mask without such a pixel costs nothing.
 * JU_ERR_INVALID_ARGUMENT, the setting as it was: a graphics resource, a NULL image, a size out of range, |stride| smaller
 * than a row, 2 B MW >= 2^32 or 2 Bh MH >= 2^32.  ju_tiled_reset, ju_tiled_set_output_size and ju_tiled_set_scene_detect
 * keep the mask.
 * ju_tiled_get_stat: "source_mask" (1 / 0), "source_mask_frames" (the frames processed while a mask was set),
 * "mask_box_x0", "mask_box_y0", "mask_box_x1", "mask_box_y1" (the box; all 0 while the mask is off or the box is empty). */
JU_API int ju_tiled_set_source_mask(ju_tiled *tiled, const ju_image *mask);
/* The alpha channel of tiled frames (docs/tiled.md "Alpha"; docs/alpha.md "Tiled").  ju_set_alpha's modes (JU_ALPHA_ZERO,
 * the default: every launch as without the call; JU_ALPHA_OPAQUE; JU_ALPHA_SOURCE), filter check and definition
 * (tests/alpha_reference.py, unchanged), with the tiled source size as the input frame and this object's output frame --
 * four times the source size, or the output size while ju_tiled_set_output_size is set -- as the output frame.  The alpha
 * plane is scaled straight from one to the other by ONE launch per frame on the tiled stream, behind the stitch (also the
 * masked, scaled and fused ones) and the encode, in front of the copy out (in a look-ahead pass: in front of what orders
 * the deferred host copy).  It is never cut into tiles, never blended and never seen by the tiles' engines, which stay in
 * mode 0: the colour bytes, the tiles' states, the detector, the mask's blend and the deep outputs are those of the same
 * object in mode 0.  It is read where the source already lies on the device -- a JU_LOC_DEVICE frame in place, the staged
 * copy of a host frame, plane 0 of an RGBX, BGRX64 or X2 input (never its decoded BGRX copy, whose X is 0); an input
 * without a slot is opaque; an output format without a slot gets no launch.  The existing refusal of an output that
 * overlaps the input covers the ordering.  A source of exactly W x H, ONE tile, gives the slots of ju_process_frame under
 * ju_set_alpha.
 * JU_ERR_INVALID_ARGUMENT, every setting as it was: a mode or filter out of range; under JU_ALPHA_SOURCE the limits of
 * ju_set_alpha between those two sizes -- whichever of ju_tiled_set_alpha and ju_tiled_set_output_size would leave them
 * is refused, and the message names alpha and both sizes.  The setter waits for the tiled stream; ju_tiled_reset keeps the
 * setting.  ju_tiled_get_stat: "alpha_mode", "alpha_filter", "alpha_frames" (frames whose slot the launch wrote). */
JU_API int ju_tiled_set_alpha(ju_tiled *tiled, int mode, int filter);
JU_API int ju_tiled_get_alpha(const ju_tiled *tiled, int *mode, int *filter);
JU_API int ju_tiled_get_info(const ju_tiled *tiled, ju_tiled_info *info);
/* The origin of tile `index` (0 .. tiles_x tiles_y - 1, row-major over the tile grid) in source pixels. */
JU_API int ju_tiled_get_tile(const ju_tiled *tiled, int index, size_t *x, size_t *y);
/* "tiles"; "frames": frames processed; "group_frames": the tiles' frames that ran inside group passes, summed over the
 * tiles (tiles x frames while every pass holds at least two tiles); "deep_from_state": the setting of
 * ju_tiled_set_deep_from_state; "hbd_from_state": 1 where the model's f16 state is its frame in float (ju_get_stat's key,
 * every tile's alike); "deep_state_frames": the frames whose output was blended from the tiles' states; "lookahead",
 * "pass_calls", "pass_frames", "pass_split_launches", "pass_overlapped_copies": ju_tiled_process_frames above;
 * "scene_mode", "scene_frames", "scene_cuts": the detector below, the two counters cumulative as ju_get_stat's;
 * "output_scaled", "output_filter", "output_scaled_frames": ju_tiled_set_output_size above; "source_mask",
 * "source_mask_frames", "mask_box_x0" .. "mask_box_y1": ju_tiled_set_source_mask above; "alpha_mode", "alpha_filter",
 * "alpha_frames": ju_tiled_set_alpha above.  An unknown key is
 * JU_ERR_INVALID_ARGUMENT. */
JU_API int ju_tiled_get_stat(const ju_tiled *tiled, const char *key, double *value);
/* The scene detector of a tiled stream (docs/tiled.md "Scene cuts"; no reference counterpart).  ju_set_scene_detect's
 * definition, modes, threshold, refusals and records, with ONE detector on the tiled object that looks at the SOURCE frame:
 * c_t is the src_width x src_height BGRX frame of call t as the split reads it (a device BGRX image in place, a host
 * image as staged, any other format as decoded at source size), N = 3 src_width src_height.  The sum is taken inside the
 * split's launch -- every source pixel counted by one tile, its owner -- and the decision never visits the host.  In
 * JU_SCENE_RESET mode a cut zeroes the recurrent inputs of ALL tiles in one launch in front of the group passes: from that
 * frame on every output byte (8-bit, and deep with ju_tiled_set_deep_from_state) equals that of an object with the
 * detector off on which ju_tiled_reset was called before exactly that frame.  JU_SCENE_REPORT changes no byte; a flow-free
 * model takes RESET as REPORT.  The tiles' own detectors stay off.  The same mode again changes only the threshold; a mode
 * change, ju_tiled_create* and ju_tiled_reset start the detector (no predecessor); `step` counts from the call that turned
 * it on and continues across ju_tiled_reset; turning the mode off frees its memory (4 src_width src_height bytes on the
 * device, 65 records and a table of 64 entries in host-mapped memory).  A refused frame does not reach the detector.
 * ju_tiled_get_scene_info: the last min(count, 64, steps seen) records, oldest first.  A source of exactly W x H gives the
 * frames and records of ju_process under ju_set_scene_detect with the same arguments. */
JU_API int ju_tiled_set_scene_detect(ju_tiled *tiled, int mode, uint32_t threshold_milli);
JU_API int ju_tiled_get_scene_detect(const ju_tiled *tiled, int *mode, uint32_t *threshold_milli);
JU_API int ju_tiled_get_scene_info(ju_tiled *tiled, ju_scene_info *out, int count, int *written);
/* Not provided for a tiled object: ju_set_source_size (the output size is ju_tiled_set_output_size, the mask
 * ju_tiled_set_source_mask, the scene detector ju_tiled_set_scene_detect, look-ahead passes ju_tiled_process_frames),
 * ju_prepare_* and ju_enqueue counterparts, graphics resources, graph capture, the C++ plugin surface. */

/* Replaces getExceptionString() (core.h:94): message of the last failed call on
 * this thread ("" if none). The pointer stays valid until the next failing
 * call on the same thread. */
JU_API const char *ju_last_error(void);

/* Replaces setLogSink(LogSink*) (core.h:23-28). callback NULL restores the
 * default sink (stderr, warnings and errors only unless JU_VERBOSE=1). */
typedef void (*ju_log_callback)(const char *tag, int level, const char *message, void *user);
JU_API void ju_set_log_callback(ju_log_callback callback, void *user);

/* Replaces getGLDeviceIndex() (core.h:60, core/src/core.cc:140-149): the HIP device that
 * drives the calling thread's current OpenGL context (hipGLGetDevices). */
JU_API int ju_get_gl_device_index(int *out_device);

/* Replaces getGLImage(image, type) (core.h:61-62, core.cc:92-138): registers an OpenGL
 * 2-D texture (RGBA8 / BGRX, the caller's GL context current) with the HIP runtime
 * (hipGraphicsGLRegisterImage; type 0 = input, read only; 1 = output, write discard) and
 * describes it as a JU_LOC_GRAPHICS_RESOURCE image whose width / height are the
 * texture's.  ju_process maps it, copies texture array <-> staging buffer and unmaps it
 * (core/include/JoshUpscale/core/cuda.h:310-349, core/src/cuda_convert.cc.cu:380-397,
 * 419-436).  Release with ju_release_gl_image (the reference's ~GLResourceImage). */
JU_API int ju_get_gl_image(uint32_t gl_texture, int type, ju_image *out_image);
JU_API void ju_release_gl_image(ju_image *image);

/* ---- multi-GPU start-up (BASELINE.json config 4; no reference counterpart: the reference
 * has no distributed code).  N GPUs = N independent streams, one process per GPU; the ONLY
 * collective is the broadcast of the model container from rank 0, so that one rank reads
 * the file.  RCCL (librccl, opened at first use) over xGMI.  The launcher carries the
 * JU_COMM_ID_BYTES id from the rank that called ju_comm_unique_id to the others
 * (bench.py: through torch.distributed's rendezvous). ---------------------------------- */
typedef struct ju_comm ju_comm;
#define JU_COMM_ID_BYTES 128
JU_API int ju_comm_unique_id(void *id_out /* JU_COMM_ID_BYTES */);
JU_API int ju_comm_create(const void *id, int rank, int world_size, int device_id, ju_comm **out_comm);
/* ncclBroadcast of `size` bytes (uint8) from `root`'s buffer into every rank's buffer. */
JU_API int ju_comm_broadcast(ju_comm *comm, void *bytes, size_t size, int root);
/* In-place maximum over ranks of one double (the bench's max-over-ranks elapsed time). */
JU_API int ju_comm_allreduce_max(ju_comm *comm, double *value);
/* ncclCommCount: the number of ranks this communicator really spans. */
JU_API int ju_comm_count(const ju_comm *comm, int *count);
JU_API void ju_comm_destroy(ju_comm *comm);

/* ---- introspection (no reference counterpart).  The test and measurement hooks (ju_debug_*,
 * ju_read_tensor, ju_time_steps) are NOT part of this library: they are declared in
 * joshupscale_amd_test.h and exported only by libJoshUpscale_test.so (built with -DJU_TEST_HOOKS);
 * the reference exports nothing but its JOSHUPSCALE_EXPORT symbols (core/CMakeLists.txt:29-36). -- */

/* Compute dtype actually in use (JU_DTYPE_F16 / JU_DTYPE_BF16 / JU_DTYPE_FP8). */
JU_API int ju_get_dtype(const ju_runtime *runtime);

/* How the runtime has been executing: "graph_replays" / "eager_runs" (per-frame programs
 * submitted as one hipGraph replay / as individual launches so far), "graph_captures"
 * (graphs captured INSIDE ju_process / ju_enqueue so far; captures by ju_prepare_frames:
 * "prepared_captures"), "registered_pairs", "direct_graphs"
 * (graphs cached for JU_LOC_DEVICE frame tuples), "resident_tower" / "resident_flow"
 * (1 when the one-launch tower kernel is in use), "launches_per_frame", "tower_variant",
 * "group_frames" (frames this runtime got from ju_process_group / ju_process_group_frames passes; of them
 * "group_yuv_frames" with a non-BGRX side),
 * "lookahead_frames" (frames that went through look-ahead passes; of them "lookahead_host_frames" with a host side,
 * "lookahead_yuv_frames" with a YUV side, 8- or 10-bit),
 * "source_scaled" / "source_mask" (1 while ju_set_source_size / ju_set_source_mask is in effect), "source_stage_frames"
 * (frames that went through the source stage or the output stage), "output_scaled" (1 while ju_set_output_size is in
 * effect), "source_filter" / "output_filter" (the JU_SCALE_* value ju_set_source_size / ju_set_output_size has in effect;
 * 0 while off), "alpha_mode" / "alpha_filter" (what ju_set_alpha set) and "alpha_frames" (frames whose alpha slot the
 * alpha launches wrote),
 * "hbd_from_state" (1: this runtime encodes JU_FMT_P010 / JU_FMT_I010 outputs from its f16 state; 0: from the 8-bit
 * frame -- normalize_brightness and output_flow models),
 * "recurrent" (1: the model has a flow net and a recurrent state; 0: a flow-free single-image model,
 * flow_arch "none" of the container -- every frame is upscaled on its own, ju_reset does nothing),
 * "output_select" (0: the frames are the generator's; 1: an output_flow model, header word 140 of the container --
 * every frame is pre_warp, the previous output warped by the flow field, while state and history advance exactly as
 * in the plain model.  The model file decides it.  There is no setter: every per-frame program and every captured
 * graph is built from the model at creation, and a switch would have to forget all of them). */
JU_API int ju_get_stat(const ju_runtime *runtime, const char *key, double *value);

/* Library version string, e.g. "joshupscale-amd 0.1 (gfx950)". */
JU_API const char *ju_version(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* JOSHUPSCALE_AMD_H_ */
