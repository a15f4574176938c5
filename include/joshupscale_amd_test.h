/* Test and measurement hooks of the MI355X engine.  NOT part of the product ABI: the shipped
 * libJoshUpscale.so exports none of these (tests/test_c_abi.py checks `nm -D`); they exist only in
 * libJoshUpscale_test.so, the same objects linked with c_api.cpp / graphics.cpp compiled under
 * -DJU_TEST_HOOKS (Makefile).  The reference hides everything that is not JOSHUPSCALE_EXPORT
 * (core/CMakeLists.txt:29-36): a plugin host must not be able to flip engine behaviour.
 * Users: tests/, bench.py (ju_time_steps for the roofline's in-frame kernel time), tools/. */
#ifndef JOSHUPSCALE_AMD_TEST_H_
#define JOSHUPSCALE_AMD_TEST_H_

#include "joshupscale_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test double for the graphics path (no GL context exists on a headless GPU box): texture
 * ids defined here resolve to pitched device buffers; device_ptr NULL removes the double
 * again.  Counters: resources registered / currently mapped / map and unmap calls. */
JU_API int ju_debug_fake_gl_texture(uint32_t gl_texture, void *device_ptr, size_t pitch, size_t width,
    size_t height, int bytes_per_pixel);
JU_API void ju_debug_fake_gl_counters(int *registered, int *mapped, int *maps, int *unmaps);

/* Copies a named internal tensor to host memory as float32.  *count receives the
 * element count; dst may be NULL to query it.  Names: "state" (last output_raw,
 * f16 [4H][4W][4]), "flow" (f16 [PH][PW][32], the flow head before depth-to-space), "flow_in", "gen_in", "trunk",
 * "tail_y", and the per-layer flow activations.  "flow" and the flow activations are the PER-FRAME tensors: a look-ahead pass
 * (ju_process_batch) computes its flow fields in tensors of its own and does not update them; "state", "flow_in" and "gen_in"
 * are what the last frame of a pass left, as after ju_process. */
JU_API int ju_read_tensor(ju_runtime *runtime, const char *name, float *dst, size_t capacity,
    size_t *count);

/* Average device time in milliseconds of ONE kernel launch among the per-frame
 * steps tagged `tag` ("tower" = the 3x3 64->64 convolutions of the generator's
 * residual blocks, "flow", "warp", "gen_head", "tail", "pack", "" = all),
 * measured with HIP events on the runtime's own stream over `iters`
 * repetitions.  *launches = kernel launches per repetition, *flops = their
 * algorithmic FLOPs (2*MAC) per repetition.  "tag#k": only the k-th launch of the tag.
 * "tag@frame" (also "tag#k@frame"): the tagged launches timed INSIDE whole frames -- every step
 * of the frame runs, HIP events bracket the tagged launches -- i.e. the kernel in the clock and
 * cache context of the real workload (what a kernel trace of the benchmark averages).  Timing
 * overwrites scratch tensors and the recurrent state: the state is reset (as by ju_reset)
 * before the call returns. */
JU_API int ju_time_steps(ju_runtime *runtime, const char *tag, int iters, double *ms_per_launch,
    int *launches, double *flops);

/* The launch plans this runtime's launchers of the flow net's convolution kernels (and of the residual blocks outside
 * the resident tower) have really used since it was created: text, one line per distinct launch in first-launch order,
 * '\n' after each, NUL-terminated.  *length receives the length without the NUL; dst may be NULL to query it.  A launcher
 * ignores a forced value (JU_FLOW_TILE, JU_SPLITK_PLAN, JU_CONV_TILE, JU_CONV_DBUF, JU_RES_BLOCK) the
 * shape does not have: what ran is what stands here.  Lines, every value a decimal number:
 *   flow_block cin= cmid= ups= pool= outk= pack= indep= H= W= items= rows= heights=<a,b,..>
 *       (outk 1 the f16 flow head, 2 the residual form; items: frames of the launch; rows: the tile height launched;
 *        heights: every height this block shape has, i.e. that fits LDS)
 *   conv_splitk cin= cout= pool= H= W= items= rows= blocks=      (blocks: cout blocks per workgroup)
 *   conv_mfma taps= ck= cin= cout= ups= pool= H= W= items= nb= rw= stages=
 *   res_block H= W=  /  res_block_pipe H= W= */
JU_API int ju_plan_report(ju_runtime *runtime, char *dst, size_t capacity, size_t *length);

/* Developer switches (timing ablations and fault injection; never needed by a
 * caller).  Keys: "tower_variant" (0 = product kernel, 4 = phase profile, 5 = per-layer
 * output maxima for quantisation calibration, 8 = the resident tower's plain schedule:
 * same bytes, tests compare it with the product's); "resident_fault" n
 * (launch the resident tower n workgroups short: tests the fallback); "pass_rerun" 1 (a look-ahead
 * pass that completed normally is run again frame by frame, as after a resident-tower report but without the
 * fallback: the re-run's bookkeeping; no kernel misbehaves -- a pass that carried the scene detector keeps its decisions,
 * and the frames run again without it); "step_rerun" 1 (the same for a single frame: ju_process
 * and the frame-by-frame steps of the multi-frame calls submit every frame a second time, as after a resident-tower
 * report but without the fallback; the scene detector must not run for the second submission: ju_get_stat
 * "scene_detector_runs" counts its runs); "group_rerun" 1 ("pass_rerun" for the passes of ju_process_group and
 * ju_process_group_frames: a group pass that completed normally is run again member by member; members whose detector
 * the pass carried keep its decisions and run again without it). */
JU_API int ju_debug_set(const char *key, int value);

/* The loader's e4m3 quantiser (round to nearest even, saturating at +-448), exposed so
 * that the CPU tests can pin it against the oracle's restatement.  No device needed. */
JU_API int ju_debug_e4m3(const float *values, unsigned char *codes, size_t count);

/* One of the two colour conversion kernels of ju_process_frame alone, on caller-supplied device buffers, on the
 * current device (synchronous).  direction 0: planes (format JU_FMT_I420 / JU_FMT_NV12) -> BGRX at `bgrx`;
 * 1: BGRX -> planes.  Any byte alignment, any signed strides (as in ju_frame). */
JU_API int ju_debug_yuv(int direction, int format, int colorspace, size_t width, size_t height, void *bgrx,
    ptrdiff_t bgrx_stride, void *const planes[3], const ptrdiff_t strides[3]);

/* The decode kernel of ju_process_frames' look-ahead passes alone (yuv420_to_bgrx_items_kernel: the YUV inputs of a
 * pass in one launch), on caller-supplied device buffers, synchronously: `count` (1 .. 8) items of one width x height,
 * item i = format formats[i] (JU_FMT_I420 / JU_FMT_NV12 / JU_FMT_P010 / JU_FMT_I010, mixed freely), colour space colorspaces[i], planes planes[3 i .. 3 i + 2] with
 * strides[3 i .. 3 i + 2] (the third unused for NV12) -> BGRX rows at bgrx[i], bgrx_strides[i] bytes apart.  Any byte
 * alignment, any signed strides (10-bit items: multiples of 2).  Per item the bytes of ju_debug_yuv direction 0 /
 * ju_debug_yuv10 op 0. */
JU_API int ju_debug_yuv_items(int count, const int *formats, const int *colorspaces, size_t width, size_t height,
    void *const *bgrx, const ptrdiff_t *bgrx_strides, void *const *planes, const ptrdiff_t *strides);

/* One of the three 10-bit conversion kernels alone (format JU_FMT_P010 / JU_FMT_I010), on caller-supplied device buffers,
 * on the current device (synchronous).  op 0: planes -> BGRX u8 rows at `image`, image_stride bytes apart; op 1: BGRX u8
 * rows at `image` -> planes (the encode of runtimes whose state is not the frame: P = 257 u8); op 2: the dense f16 tensor
 * [height][width][4] (B, G, R, unused) at `image`, 16-byte aligned, image_stride ignored -> planes (the encode from the
 * recurrent state: P = floor((s + 0.5) * 65536), saturated).  Plane addresses and strides: bytes, multiples of 2, any sign. */
JU_API int ju_debug_yuv10(int op, int format, int colorspace, size_t width, size_t height, void *image,
    ptrdiff_t image_stride, void *const planes[3], const ptrdiff_t strides[3]);

/* One of the 4:2:2 / 4:4:4 conversion kernels alone (format JU_FMT_YUY2 .. JU_FMT_I410), on caller-supplied device
 * buffers, on the current device (synchronous).  op 0: planes -> BGRX rows at `image`; op 1: BGRX u8 rows at `image` ->
 * planes (10-bit formats: P = 257 u8); op 2, 10-bit formats only: the dense f16 tensor [height][width][4] at `image`,
 * 16-byte aligned, image_stride ignored -> planes.  4:2:2 needs an even width; any height, and for 4:4:4 any width.
 * Planes beyond the format's count are not read.  ju_debug_yuv_items takes these formats as items too. */
JU_API int ju_debug_yuv_sampled(int op, int format, int colorspace, size_t width, size_t height, void *image,
    ptrdiff_t image_stride, void *const planes[3], const ptrdiff_t strides[3]);

/* One of the RGB conversion kernels alone (format JU_FMT_BGR24 .. JU_FMT_BGR96F; tests/rgb_reference.py), on
 * caller-supplied device buffers, on the current device (synchronous).  op 0: planes -> BGRX rows at `image`; op 1: BGRX
 * u8 rows at `image` -> planes (deep formats: from the 8-bit frame); op 2, deep formats only: the dense f16 tensor
 * [height][width][4] at `image`, 16-byte aligned, image_stride ignored -> planes.  Any width and height; plane addresses
 * and strides are multiples of the sample size.  ju_debug_yuv_items takes these formats as items too. */
JU_API int ju_debug_rgb(int op, int format, size_t width, size_t height, void *image, ptrdiff_t image_stride,
    void *const planes[3], const ptrdiff_t strides[3]);

/* One of the packed 10-bit conversion kernels alone (format JU_FMT_V210 / Y210 / Y410 / X2RGB10 / X2BGR10;
 * tests/packed10_reference.py), on caller-supplied device buffers, on the current device (synchronous).  Another format,
 * a NULL buffer, an odd V210 / Y210 width, a plane off its alignment (4 bytes; Y210: 2) or a stride below the row bytes
 * is JU_ERR_INVALID_ARGUMENT before any device call.  op 0: the plane -> BGRX rows at `image`; op 1: BGRX u8 rows at
 * `image` -> the plane (P = 257 u8); op 2: the dense f16 tensor [height][width][4] at `image`, 16-byte aligned,
 * image_stride ignored -> the plane; op 3: the dense u16 frame [height][width][4] (B, G, R, unused) at `image`, 8-byte
 * aligned, image_stride ignored -> the plane (the sample is P itself).  Only planes[0] / strides[0] are read; `colorspace`
 * is ignored for the two RGB formats.  ju_debug_yuv_items takes these formats as items too. */
JU_API int ju_debug_packed10(int op, int format, int colorspace, size_t width, size_t height, void *image,
    ptrdiff_t image_stride, void *const planes[3], const ptrdiff_t strides[3]);

/* The source stage's kernels alone (docs/source_stage.md), on caller-supplied device buffers of BGRX rows with any byte
 * alignment and any signed strides, on the current device (synchronous).  op 0: the scaler -- `src` (src_width x
 * src_height) -> `dst` (dst_width x dst_height), tables built as ju_set_source_size builds them; the mask arguments are
 * ignored.  op 1: the blend -- `dst` is the frame (the network's output, rewritten in place), `src` the source that shows
 * where the mask is dark, `mask` the mask, each of its own size.  op 2: no device and no buffers -- only the limits
 * ju_set_source_size applies to a source of src_width x src_height for a model input of dst_width x dst_height, with its
 * message (JU_ERR_INVALID_ARGUMENT) or JU_OK. */
JU_API int ju_debug_source(int op, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, const void *src,
    ptrdiff_t src_stride, size_t src_width, size_t src_height, const void *mask, ptrdiff_t mask_stride, size_t mask_width,
    size_t mask_height);

/* The output stage's pieces alone (docs/output_stage.md; tests/output_reference.py), on the current device (synchronous).
 * op 0: scale_state_kernel -- `src`, the dense f16 tensor [src_height][src_width][4] (16-byte aligned), -> `dst`, the dense
 * u16 frame [dst_height][dst_width][4] (8-byte aligned), tables built as ju_set_output_size builds them; format,
 * colorspace, planes and strides are ignored.  op 1: the encode of one deep format from the dense u16 frame `src` of
 * dst_width x dst_height into planes / strides (bytes, multiples of the sample size, any sign), as ju_debug_rgb takes
 * them; `dst` and the source size are ignored; a format that is not deep is JU_ERR_INVALID_ARGUMENT.  op 2: no device and
 * no buffers -- only the limits ju_set_output_size applies to an output size of dst_width x dst_height for a model output
 * of src_width x src_height and the filter passed in `format`, with its message (JU_ERR_INVALID_ARGUMENT) or JU_OK. */
JU_API int ju_debug_output(int op, void *dst, size_t dst_width, size_t dst_height, const void *src, size_t src_width,
    size_t src_height, int format, int colorspace, void *const planes[3], const ptrdiff_t strides[3]);

/* The scene detector's kernels alone (docs/scene_detect.md; tests/scene_reference.py), on the current device (synchronous).
 * op 0: scene_sad_kernel -- `frame`, device BGRX rows of width x height at any 4-byte-aligned address with any signed
 * stride of at least a row (bytes, a multiple of 4), against `prev`, the dense device BGRX frame kept so far, which is
 * rewritten with `frame`; `state`: 40 bytes of device memory, zero before the first call (the accumulator and the
 * ticket are zero again when the call returns, word 3 is the reset flag, bytes 16 .. 23 the S the next call compares
 * with); has_prev: bit 0 frame t-1 is in `prev`, bit 1 frame t-2 went before it; *record receives the decision (step 0).
 * op 1: scene_clear_kernel -- `state` is the device flag word; if it is not 0, clear_a[0 .. a_bytes) and
 * clear_b[0 .. b_bytes) become 0, any alignment; the other arguments are ignored.  op 2: no device and no buffers --
 * the refusals of ju_set_scene_detect for the mode passed in has_prev and threshold_milli, with their message
 * (JU_ERR_INVALID_ARGUMENT) or JU_OK. */
JU_API int ju_debug_scene(int op, const void *frame, ptrdiff_t stride, size_t width, size_t height, void *prev, void *state,
    int has_prev, uint32_t threshold_milli, int reset_mode, ju_scene_info *record, void *clear_a, size_t a_bytes,
    void *clear_b, size_t b_bytes);

/* scene_pass_kernel alone: the detector over the `count` (1 .. 8) frames of a look-ahead pass in one launch
 * (docs/scene_detect.md "Passes"), on the current device (synchronous).  frames[i] / strides[i]: device BGRX rows of
 * width x height, each at its own 4-byte-aligned address with its own signed stride of at least a row (a multiple of 4);
 * item i is compared with item i - 1, item 0 with `prev`, the dense kept frame, which is rewritten with the last item.
 * `state`: the 40 bytes of ju_debug_scene op 0 (bytes 16 .. 23: the S item 0 compares with, and afterwards the last
 * item's; frames and cuts behind it).  `pass_state`: 136 bytes of device memory, zero before the first call -- eight
 * 64-bit accumulators and the 32-bit ticket at byte 64 (all zero again when the call returns), then at byte 72
 * resetAt[8] (uint32) and at byte 104 cutAt[8] (int32).  has_prev: what is in the detector's memory in front of item 0,
 * as for op 0 of ju_debug_scene (0, 1 or 3).  records[i] receives item i's decision with step first_step + i;
 * reset_at[i] = cut_i && reset_mode; cut_at[i] = the latest item <= i with reset_at set, else -1. */
JU_API int ju_debug_scene_pass(int count, const void *const *frames, const ptrdiff_t *strides, size_t width, size_t height,
    void *prev, void *state, void *pass_state, int has_prev, uint64_t first_step, uint32_t threshold_milli, int reset_mode,
    ju_scene_info *records, uint32_t *reset_at, int32_t *cut_at);

/* scene_group_kernel alone: the detector over the `count` (1 .. 8) INDEPENDENT items of a group pass in one launch
 * (docs/scene_detect.md "Group passes"), on the current device (synchronous).  Item i: frames[i] / strides[i], device BGRX
 * rows of width x height at its own 4-byte-aligned address with its own signed stride of at least a row (a multiple of
 * 4), against prev[i], its own dense kept frame, which is rewritten with it; states[i]: its own 40 bytes of
 * ju_debug_scene op 0 (every accumulator and every ticket word are zero again when the call returns); has_prev[i] (0, 1
 * or 3), first_steps[i] (the record's step, and modulo 64 its ring slot), threshold_milli[i] and modes[i]
 * (JU_SCENE_REPORT or JU_SCENE_RESET) are what the kernel reads from the item's host-mapped words.  frames[i] == NULL:
 * an absent item -- none of its memory is touched, records[i] and reset_flags[i] are zero.  records[i] receives item i's
 * decision, reset_flags[i] = cut_i && modes[i] == JU_SCENE_RESET (the state's word 3). */
JU_API int ju_debug_scene_group(int count, const void *const *frames, const ptrdiff_t *strides, size_t width, size_t height,
    void *const *prev, void *const *states, const int *has_prev, const uint64_t *first_steps, const uint32_t *threshold_milli,
    const int *modes, ju_scene_info *records, uint32_t *reset_flags);

/* scene_clear_items_kernel alone: the conditional clear of `count` (1 .. 8) items in one launch.  flags[i]: the device
 * address of item i's 32-bit flag word (NULL: an absent item); if the word is not 0, a[i][0 .. a_bytes[i]) and
 * b[i][0 .. b_bytes[i]) become 0, any alignment and any sizes. */
JU_API int ju_debug_scene_clear_items(int count, const void *const *flags, void *const *a, const size_t *a_bytes,
    void *const *b, const size_t *b_bytes);

/* The scalers with a filter argument (docs/source_stage.md "Filters"; tests/scale_filter_reference.py); `filter` is a
 * JU_SCALE_* value.  op 0: the 8-bit scaler -- buffers, sizes and strides as ju_debug_source op 0.  op 1: the state
 * scaler -- `src` the dense f16 tensor, `dst` the dense u16 frame, as ju_debug_output op 0; the strides are ignored.
 * op 2 / op 3: no device and no buffers -- the limits ju_set_source_size (a source of src_width x src_height for a model
 * input of dst_width x dst_height) / ju_set_output_size (an output size of dst_width x dst_height for a model output of
 * src_width x src_height) apply for the filter, with their message (JU_ERR_INVALID_ARGUMENT) or JU_OK.  op 4: no device --
 * the table of one axis, src_width source samples -> dst_width destination samples, as the setters build it, copied into
 * host arrays: start[dst_width], count[dst_width] and taps[dst_width][33] (taps beyond a row's count are 0); the heights
 * and the buffers are ignored.  Ops 0 .. 3 ignore start, count and taps. */
JU_API int ju_debug_scale(int op, int filter, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height,
    const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height, int *start, int *count, int16_t *taps);

/* The alpha kernels alone (alpha_kernels.hip; docs/alpha.md; tests/alpha_reference.py): ONE synchronous launch each on
 * caller-supplied device buffers, on the current device.  A kind says where the slot lies in a side's rows: 0 byte 3 of
 * four-byte pixels (any byte alignment), 1 word 3 of eight-byte pixels (address and stride multiples of 2), 2 bits 30-31
 * of 32-bit words (multiples of 4); a source may also be 3, none: the plane is 65535 everywhere and `src` is not read.
 * Strides are bytes of any sign, sizes 1 .. 32768.  ju_debug_alpha_scale: the source's alpha of src_width x src_height
 * scaled by `filter` (a JU_SCALE_* value, held to its ratio limits) into the slots of dst_width x dst_height pixels; no
 * other bit of the destination changes.  ju_debug_alpha_fill: the top code into every slot.  JU_ERR_INVALID_ARGUMENT: an
 * unknown kind or filter, a NULL side, |stride| smaller than a row, a misaligned side, a size out of range.
 * ju_debug_alpha_problem: no device -- the limits of ju_set_alpha for a runtime whose input frames are in_width x
 * in_height and whose output frames are out_width x out_height, with its message (JU_ERR_INVALID_ARGUMENT) or JU_OK.
 * ju_debug_tiled_alpha_problem: no device -- the limits of ju_tiled_set_alpha for a tiled source of src_width x src_height
 * whose output size is out_width x out_height ((0, 0): none set, the output frame is four times the source), likewise. */
JU_API int ju_debug_alpha_scale(int source_kind, int sink_kind, int filter, void *dst, ptrdiff_t dst_stride, size_t dst_width,
    size_t dst_height, const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height);
JU_API int ju_debug_alpha_fill(int sink_kind, void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height);
JU_API int ju_debug_alpha_problem(int mode, int filter, size_t in_width, size_t in_height, size_t out_width, size_t out_height);
JU_API int ju_debug_tiled_alpha_problem(int mode, int filter, size_t src_width, size_t src_height, size_t out_width,
    size_t out_height);

/* The sources of a look-ahead pass scaled in one launch (scale_bgrx_items_kernel; docs/source_stage.md "Passes"): ONE
 * synchronous launch over `count` (1 .. 8) items on caller-supplied device buffers, on the current device.  Item i reads
 * BGRX rows of src_width x src_height at src[i] with the signed stride src_strides[i] and writes dst_width x dst_height
 * at dst[i] with dst_strides[i], any byte alignment each; sizes (1 .. 32768) and `filter` (a JU_SCALE_* value, held to
 * its ratio limits) are shared by all items.  Per item the bytes of ju_debug_scale op 0. */
JU_API int ju_debug_scale_items(int count, int filter, void *const *dst, const ptrdiff_t *dst_strides, size_t dst_width,
    size_t dst_height, const void *const *src, const ptrdiff_t *src_strides, size_t src_width, size_t src_height);

/* The sources of a group pass scaled in one launch (scale_bgrx_members_kernel; docs/source_stage.md "Group passes"): ONE
 * synchronous launch over `count` (1 .. 8) members on caller-supplied device buffers, on the current device.  Member i
 * reads BGRX rows of src_widths[i] x src_heights[i] at src[i] with the signed stride src_strides[i], through the filter
 * filters[i] (a JU_SCALE_* value, held to its ratio limits before any device call), and writes dst_width x dst_height --
 * the one destination size of the launch -- at dst[i] with dst_strides[i]; any byte alignment each, sizes 1 .. 32768.  Per
 * member the bytes of ju_debug_scale op 0. */
JU_API int ju_debug_scale_members(int count, const int *filters, void *const *dst, const ptrdiff_t *dst_strides,
    size_t dst_width, size_t dst_height, const void *const *src, const ptrdiff_t *src_strides, const size_t *src_widths,
    const size_t *src_heights);

/* The sized form of the passes' decode launch alone (yuv_to_bgrx_items_sized_kernel: the non-BGRX inputs of a group pass
 * whose members differ in size): ju_debug_yuv_items with a width and a height per item, widths[i] x heights[i] (the parity
 * rules of item i's format apply to them).  Per item the bytes of ju_debug_yuv_items at that size. */
JU_API int ju_debug_yuv_items_sized(int count, const int *formats, const int *colorspaces, const size_t *widths,
    const size_t *heights, void *const *bgrx, const ptrdiff_t *bgrx_strides, void *const *planes, const ptrdiff_t *strides);

/* The temporal output filter alone (launchTemporalFilter: zero_words_kernel, temporal_reduce_kernel, temporal_blend_kernel;
 * tests/temporal_reference.py), on caller-supplied device buffers, on the current device (synchronous).  `state`: the dense
 * f16 tensor [4 height][4 width][4] (8-byte aligned), rewritten in place; `pre_warp`: the same shape, read only; `out`: BGRX
 * rows of 4 width x 4 height at a 4-byte-aligned address with any signed stride that is a multiple of 4; `sums`: the six
 * words of launchFrameSums on the device (4-byte aligned), or NULL for a model without normalize_brightness; width and
 * height are the LR frame's, 1 .. 8192.  strength, threshold, gain and window are held to the model loader's bounds with
 * its wording; `flags` are the mode bits of the model file: 1 L2, 2 limit, 4 luma.  The hook allocates the accumulator
 * scratch itself -- the words the filter uses primed with ones, acc_capacity - temporalAccWords() further words with zeros --
 * and, where `acc` is not NULL, copies acc_capacity words (at least temporalAccWords(); the window grid in row-major
 * order, 32.32 fixed point) into that host array after the run.  A NULL buffer, a misaligned pointer or stride, a parameter
 * out of bounds, an unknown flag bit or a capacity that is too small is JU_ERR_INVALID_ARGUMENT before any device call. */
JU_API int ju_debug_temporal(void *state, const void *pre_warp, void *out, ptrdiff_t out_stride, const void *sums,
    size_t width, size_t height, float strength, float threshold, float gain, int window, unsigned flags,
    uint64_t *acc, size_t acc_capacity);

/* The two kernels of tiled upscaling alone (tile_split_kernel, tile_stitch_kernel; docs/tiled.md; the definitions:
 * tests/tiled_reference.py split / stitch), each ONE synchronous launch on caller-supplied device buffers, on the current
 * device, for a source of src_width x src_height tiled by tile_width x tile_height at `overlap` -- the layout ju_tiled
 * builds, held to its limits.  `tiles`: `count` dense images, 16-byte aligned, row-major over the tile grid; count must be
 * the layout's tile count.
 * ju_debug_tile_split reads BGRX rows of the source at `src` (address and signed stride multiples of 4) and writes every
 * tile's tile_width x tile_height input, X = 0.
 * ju_debug_tile_stitch reads every tile's 4 tile_width x 4 tile_height output and writes BGRX rows of 4 src_width x
 * 4 src_height at `dst` (address and signed stride multiples of 4; any 16-byte phase), X = 0, and nothing around them.
 * A NULL buffer, a misaligned pointer or stride, |stride| smaller than a row, sizes or an overlap outside the limits or
 * a wrong count is JU_ERR_INVALID_ARGUMENT before any device call. */
JU_API int ju_debug_tile_split(const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count);
JU_API int ju_debug_tile_stitch(void *dst, ptrdiff_t dst_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count);
/* The blend of the tiles' f16 states alone (tile_stitch_state_kernel; docs/tiled.md "Deep outputs"; the definition:
 * tests/tiled_deep_reference.py stitch16 over p_from_state), ONE synchronous launch on caller-supplied device buffers, on
 * the current device, for the same layout, held to the same limits.  `tiles`: `count` dense states [4 tile_height]
 * [4 tile_width][4] f16 (B, G, R and a fourth value that is ignored), 16-byte aligned, row-major over the tile grid.  It
 * writes the dense frame [4 src_height][4 src_width][4] of 16-bit words at `dst16` (16-byte aligned), X = 0, and nothing
 * behind it.  A NULL buffer, a misaligned pointer, sizes or an overlap outside the limits or a wrong count is
 * JU_ERR_INVALID_ARGUMENT before any device call. */
JU_API int ju_debug_tile_stitch_state(void *dst16, size_t src_width, size_t src_height, size_t tile_width, size_t tile_height,
    int overlap, void *const *tiles, int count);
/* The two fused kernels of a tiled object's output size alone (tile_stitch_scale_kernel, tile_stitch_scale_state_kernel;
 * docs/tiled.md "An output size"; the definitions: tests/tiled_output_reference.py frame8 / frame16), each ONE synchronous
 * launch on caller-supplied device buffers, on the current device, for the layout and the tiles of ju_debug_tile_stitch /
 * ju_debug_tile_stitch_state, held to the same limits, and an output of dst_width x dst_height through `filter`
 * (JU_SCALE_*), held to ju_tiled_set_output_size's limits with its message.
 * ju_debug_tile_stitch_scale writes BGRX rows at `dst` -- any byte alignment, signed stride -- X = 0, and nothing around them.
 * ju_debug_tile_stitch_scale_state writes the dense frame [dst_height][dst_width][4] of 16-bit words at `dst16` (8-byte
 * aligned), X = 0, and nothing behind it.  A NULL buffer, a misaligned tile or 16-bit frame, |stride| smaller than a row,
 * sizes, an overlap, an output size or a filter outside the limits or a wrong count is JU_ERR_INVALID_ARGUMENT before any
 * device call. */
JU_API int ju_debug_tile_stitch_scale(void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, int filter,
    size_t src_width, size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count);
JU_API int ju_debug_tile_stitch_scale_state(void *dst16, size_t dst_width, size_t dst_height, int filter, size_t src_width,
    size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count);
/* The two kernels of a tiled object's source mask alone (tile_stitch_mask_kernel, tile_stitch_mask_scale_kernel;
 * docs/tiled.md "A mask"; the definitions: tests/tiled_mask_reference.py masked / frame8), each ONE synchronous launch on
 * caller-supplied device buffers, on the current device: the arguments of ju_debug_tile_stitch / ju_debug_tile_stitch_scale,
 * held to the same limits, then `source`, the device BGRX rows of the src_width x src_height source, and `mask`, device
 * BGRX rows of mask_width x mask_height (1 .. 16384 each) -- addresses and signed strides multiples of 4.  The hooks compute
 * the box themselves, by the product's function, from the mask read back to the host.  A NULL `mask` is no mask: the
 * unmasked hook's launch.  Refused with JU_ERR_INVALID_ARGUMENT before any device call: what the unmasked hooks refuse, a
 * NULL source, a misaligned source, mask or (unscaled) destination, |stride| smaller than a row, a mask size out of range,
 * 2 x blended extent x mask extent not below 2^32.
 * ju_debug_mask_box touches no device: the box (x0, y0, x1, y1 into box[4]; all 0: empty) of a HOST mask over a blended
 * frame of width x height (csrc/mask_box.h; tests/tiled_mask_reference.py box). */
JU_API int ju_debug_tile_stitch_mask(void *dst, ptrdiff_t dst_stride, size_t src_width, size_t src_height, size_t tile_width,
    size_t tile_height, int overlap, void *const *tiles, int count, const void *source, ptrdiff_t source_stride, const void *mask,
    ptrdiff_t mask_stride, size_t mask_width, size_t mask_height);
JU_API int ju_debug_tile_stitch_mask_scale(void *dst, ptrdiff_t dst_stride, size_t dst_width, size_t dst_height, int filter,
    size_t src_width, size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count,
    const void *source, ptrdiff_t source_stride, const void *mask, ptrdiff_t mask_stride, size_t mask_width, size_t mask_height);
JU_API int ju_debug_mask_box(const void *mask, ptrdiff_t mask_stride, size_t mask_width, size_t mask_height, size_t width,
    size_t height, int *box);

/* The split of a look-ahead pass alone (tile_split_frames_kernel; docs/tiled.md "Look-ahead passes"; the definition:
 * tests/tiled_reference.py split, frame by frame): ONE synchronous launch over `frames` (1 .. 8) sources of src_width x
 * src_height -- srcs[f] / src_strides[f], each frame's own device BGRX rows, address and signed stride multiples of 4 --
 * into the layout of ju_debug_tile_split: tile k's input of frame f is written at tiles[k] + f * slot_bytes (a multiple of
 * 16 that holds a tile), X = 0, and nothing around it.  Refused with JU_ERR_INVALID_ARGUMENT before any device call: what
 * ju_debug_tile_split refuses, for any frame (the message names it), a frame count outside 1 .. 8, a NULL array, a slot
 * stride that is no multiple of 16 or smaller than a tile.
 * ju_debug_tiled_pass_plan touches no device: where the passes of a call of `count` (0 .. 4096) frames start under the cap
 * `cap` (csrc/tile_pass_plan.h; tests/tiled_pass_reference.py plan) -- clash[i * count + j] != 0 for i < j: frames i and j
 * cannot share a pass.  *passes: how many; starts[0 .. min(capacity, *passes)): their first frames. */
JU_API int ju_debug_tile_split_frames(const void *const *srcs, const ptrdiff_t *src_strides, int frames, size_t src_width,
    size_t src_height, size_t tile_width, size_t tile_height, int overlap, void *const *tiles, size_t slot_bytes, int count);
JU_API int ju_debug_tiled_pass_plan(int count, int cap, const unsigned char *clash, int *starts, int capacity, int *passes);

/* The two kernels of a tiled stream's scene detector alone (docs/tiled.md "Scene cuts"), each ONE synchronous launch on
 * caller-supplied device buffers, on the current device.
 * ju_debug_tile_split_scene: tile_split_scene_kernel -- the source, the layout and the tiles of ju_debug_tile_split (the
 * same tile bytes), and the detector's step on the source frame as op 0 of ju_debug_scene takes it: `prev`, the dense
 * device BGRX frame of src_width x src_height kept so far (4-byte aligned), is rewritten with the source, X = 0; `state`:
 * the 40 bytes of ju_debug_scene (8-byte aligned; zero before the first call; the accumulator and the ticket are zero
 * again when the call returns, word 3 is the reset flag, bytes 16 .. 23 the S the next call compares with, frames and cuts
 * behind it); has_prev 0, 1 or 3; threshold_milli 1 .. 255000; *record receives the decision (step 0) with
 * N = 3 src_width src_height.  Refused before any device call: what ju_debug_tile_split refuses, a NULL or misaligned
 * detector buffer, another has_prev, a threshold out of range.
 * ju_debug_scene_clear_tiles: scene_clear_tiles_kernel -- `flag`: the device address of ONE 32-bit flag word; if it is
 * not 0, a[i][0 .. a_bytes[i]) and b[i][0 .. b_bytes[i]) become 0 for every i < count (1 .. 64), any alignment and any
 * sizes; if it is 0 no byte changes. */
JU_API int ju_debug_tile_split_scene(const void *src, ptrdiff_t src_stride, size_t src_width, size_t src_height,
    size_t tile_width, size_t tile_height, int overlap, void *const *tiles, int count, void *prev, void *state,
    ju_scene_info *record, int has_prev, uint32_t threshold_milli, int reset_mode);
JU_API int ju_debug_scene_clear_tiles(int count, const void *flag, void *const *a, const size_t *a_bytes, void *const *b,
    const size_t *b_bytes);

/* ---- the network's compute kernels alone (docs/exact_tests.md; the definitions: tests/exact_reference.py) ----------------
 * Each hook is ONE synchronous launch of a product launcher on caller-supplied device buffers, on the current device, with
 * its arguments in a struct.  Whatever the launcher would throw on, a NULL or misaligned buffer (16 bytes for 16-bit
 * tensors), a size outside 1 .. 4096, a pitch below the row or an item stride below the tensor is
 * JU_ERR_INVALID_ARGUMENT with a message, before any device call.
 * Weights and bias are HOST f32 arrays in the folded order [taps][cin_real][cout] / [cout]; cin_real (1 .. cin) may be
 * below the padded channel count `cin` of the tensor.  The hook packs them with the product's packConvWeights (cinMap =
 * 0 .. cin_real - 1, then -1) for the kernel's nb and uploads them: the packer is part of what runs.
 * ju_debug_plan: the developer launch plan (the fields of DevPlan, csrc/kernels.h: JU_FLOW_TILE, JU_RES_BLOCK,
 * JU_CONV_DBUF, JU_SPLITK_PLAN, JU_CONV_TILE); conv_stages -1 and every other field 0 = the launcher's own choice.
 * plan_text / plan_capacity (NULL / 0: not wanted): receives the launch's lines of ju_plan_report, NUL-terminated,
 * cut at the capacity. */
typedef struct ju_debug_plan {
	int flow_tile, res_block, conv_stages, splitk_rows, splitk_blocks, conv_nb, conv_rw;
} ju_debug_plan;

/* kernel 0: launchConv (conv_mfma_kernel); 1: launchConvSplitK (conv_splitk_kernel; the hook supplies the zero page);
 * 2: launchConvTower (conv_tower_kernel) -- in / res / out are then the INTERIOR ORIGINS of tower-layout tensors
 * [8 ceil(H / 8) + 2][32 ceil(W / 32) + 2][64] whose border and surplus rows / columns are zero, every pitch is
 * 32 ceil(W / 32) + 2, and a shape launchConvTower would hand to launchConv is refused.  The other fields are
 * ConvParams' (csrc/kernels.h): pitches in pixels (0: dense), `upsample`: `in` is [H / 2][W / 2][cin] with in_pitch in its
 * pixels, `pool`: `out` is [H / 2][W / 2][cout] with out_pitch in its pixels, out_head: `out` is f16 whatever the dtype;
 * items 1 .. 8 with the byte strides between the items' tensors (multiples of 16, at least a tensor; items > 1 takes no
 * res and no tower).  dtype: JU_DTYPE_F16 / JU_DTYPE_BF16. */
typedef struct ju_debug_conv_args {
	int kernel, dtype;
	const void *in, *res;
	void *out;
	const float *weights, *bias;
	int H, W, cin, cin_real, cout, taps, relu;
	float slope;
	int out_head, pool, upsample, nb, rw;
	int in_pitch, out_pitch, res_pitch;
	int items;
	long long in_item_bytes, out_item_bytes;
	ju_debug_plan plan;
	char *plan_text;
	size_t plan_capacity;
} ju_debug_conv_args;
JU_API int ju_debug_conv(const ju_debug_conv_args *args);

/* launchFlowBlock (flow_block_kernel; residual: res_block_pipe_kernel, with plan.res_block 1 or a LeakyReLU res_block_kernel,
 * with plan.res_block 2 flow_block_kernel's residual form): conv A 3x3 cin -> cmid, act1, conv B 3x3 cmid -> cmid,
 * [+ in], act2, [2x2 max-pool].  weights1 [9][cin_real][cmid], weights2 [9][cmid][cmid].  The shapes are the launcher's
 * table (flow_kernels.hip JU_FB_CASE); the input-packing, independent-item and cut-aware forms of the first block are not
 * reachable from here.  A residual launch takes one item. */
typedef struct ju_debug_flow_block_args {
	int dtype;
	const void *in;
	void *out;
	const float *weights1, *bias1, *weights2, *bias2;
	int H, W, cin, cin_real, cmid;
	int upsample, pool, out_head, residual, act1, act2;
	float slope;
	int in_pitch, out_pitch;
	int items;
	long long in_item_bytes, out_item_bytes;
	ju_debug_plan plan;
	char *plan_text;
	size_t plan_capacity;
} ju_debug_flow_block_args;
JU_API int ju_debug_flow_block(const ju_debug_flow_block_args *args);

/* op 0: launchUpsample2 -- `items` dense tensors [H][W][C] one after the other -> [2 H][2 W][C] each; op 1: launchMaxPool2 --
 * [H][W][C] (H, W even) -> [H / 2][W / 2][C], items 1.  C a multiple of 8. */
typedef struct ju_debug_resample_args {
	int op, dtype;
	const void *in;
	void *out;
	int H, W, C, items;
} ju_debug_resample_args;
JU_API int ju_debug_resample(const ju_debug_resample_args *args);

/* launchWarpPack with every argument (csrc/kernels.h): state f16 [4 H][4 W][4] (8-byte aligned), flow f16 [..][PW][32]
 * read at (h + pad_top, w + pad_left), frame BGRX rows (4-byte aligned, signed stride a multiple of 4), out: the 64-slot
 * records at image pixel (0, 0), out_pitch in pixels (0: W); sums (may be NULL; passed through), pre_warp_out (may be
 * NULL) f16 [4 H][4 W][4], out_u8 (may be NULL) BGRX rows of 4 W x 4 H, 4-byte aligned, signed stride a multiple of 4. */
typedef struct ju_debug_warp_args {
	int dtype;
	const void *state, *flow, *frame;
	ptrdiff_t frame_stride;
	void *out;
	int out_pitch, H, W, PW, pad_top, pad_left;
	const void *sums;
	void *pre_warp_out, *out_u8;
	ptrdiff_t out_stride;
} ju_debug_warp_args;
JU_API int ju_debug_warp(const ju_debug_warp_args *args);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* JOSHUPSCALE_AMD_TEST_H_ */
