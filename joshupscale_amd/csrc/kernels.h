// Host-side launch interface of the gfx950 kernels ({conv,tower,frame}_kernels.hip).
//
// Every launcher enqueues on the given stream and returns immediately; none of
// them allocates, synchronises or touches the host heap, so the whole per-frame
// sequence can be captured into a hipGraph (engine.cpp), mirroring the
// reference's one captured graph per binding set
// (reference core/src/tensorrt_backend.cc:257-263).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "tile_geometry.h"

namespace ju {

enum DType : int { kF16 = 0, kBF16 = 1 };

inline std::size_t dtypeSize(DType) { return 2; }

// ---- developer launch plans (test flavour of the library only: dev_switch.h) ------------------
// The launchers of the flow net's convolution kernels choose a launch plan -- tile height, cout blocks per workgroup,
// staging depth -- from the tensor's size and the CU count; none of the choices changes a byte
// (tests/test_gpu_launch_plans.py holds every plan to the default's bytes).  A runtime of the test flavour reads the
// switches that force a plan ONCE, where it is constructed (Engine::Engine), into its DevPlan; the launch descriptors
// below carry a pointer to it, so that two runtimes of one process can differ and no launch looks at the environment.
// In the product library every descriptor's `plan` is null.
// PlanLog: what the launchers of ONE runtime really launched -- a forced value that does not fit the shape is ignored by
// its launcher, and a test reads from here that the plan it asked for ran.  One line per distinct launch, in first-launch
// order (ju_plan_report, include/joshupscale_amd_test.h, documents the lines).
class PlanLog {
public:
	void note(const std::string &line) {
		std::lock_guard<std::mutex> lock(m_Mutex);
		for (const std::string &l : m_Lines) {
			if (l == line) return;
		}
		m_Lines.push_back(line);
	}
	std::string text() const {
		std::lock_guard<std::mutex> lock(m_Mutex);
		std::string out;
		for (const std::string &l : m_Lines) out += l + "\n";
		return out;
	}

private:
	mutable std::mutex m_Mutex;
	std::vector<std::string> m_Lines;
};
struct DevPlan {
	int flowTile = 0;     // JU_FLOW_TILE=<rows>: flow_block_kernel's tile height where the shape has it (0: the cost rule)
	int resBlock = 0;     // JU_RES_BLOCK: 0 res_block_pipe_kernel, 1 "plain" res_block_kernel, 2 "tile" flow_block_kernel
	int convStages = -1;  // JU_CONV_DBUF=0|1|2: conv_mfma_kernel's staging depth on multi-chunk layers (-1: by launch size)
	int splitkRows = 0;   // JU_SPLITK_PLAN=<rows>[x<blocks>]: conv_splitk_kernel's tile height (even, 2 .. 34; 0: the rule) ...
	int splitkBlocks = 0; // ... and its cout blocks per workgroup (1 or 2; 2 only where the launcher's own rule may take it)
	int convNb = 0;       // JU_CONV_TILE=<nb>x<rw>: conv_mfma_kernel's tile form where convTiling is consulted (0: its choice)
	int convRw = 0;
	PlanLog *log = nullptr;
};

// ---- implicit-GEMM convolution on MFMA -----------------------------------
// in   : NHWC [H][W][cin]   16-bit, cin a multiple of 16
// wgt  : kernel-ready weights from packConvWeights() (model.cpp)
// bias : f32 [cout] (BN-folded bias or the layer's own bias)
// res  : optional NHWC [H][W][cout] 16-bit tensor added before the activation
// out  : NHWC [H][W][cout] in the compute type, or f16 (outHead: the flow head)
struct ConvParams {
	const void *in;
	const void *wgt;
	const float *bias;
	const void *res;
	void *out;
	int H, W;
	int cin, cout;
	int taps;    // 9 (3x3 "same") or 1 (1x1)
	int relu;    // activation: 0 none, 1 max(x, 0), 2 LeakyReLU (x < 0 ? slope * x : x)
	float slope; // negative slope for relu == 2
	int outHead; // store f16 whatever the compute type: the flow head (HR pixel offsets up to a few
	             // pixels: f16 resolves 2^-9 .. 2^-8 px there, bf16 would not)
	// 2x2 max-pool fused into the epilogue: out is [H/2][W/2][cout] (dense or pitched
	// in POOLED pixels).  Needs rw == 2, even H and W, no residual, 16-bit output.
	int pool;
	// TF1 bilinear x2 upsampling fused into the tile staging: `in` is the
	// half-resolution tensor [H/2][W/2][cin] (inPitch in its pixels), H and W are the
	// layer's (full) resolution.  Needs 3x3, cin a multiple of 64, nb == 1, even H, W.
	int upsample;
	// multi-chunk register-prefetch path (set by launchConv): 2 = two LDS stages, 1 = one
	int stages;
	// Row pitches in pixels (0 = dense, i.e. W).  The pointers address image
	// pixel (0,0); a tensor kept in the zero-bordered tower layout (below) is
	// passed as its interior origin plus its pitch.
	int inPitch, outPitch, resPitch;
	// Tile shape chosen per layer (convTiling): couts per workgroup = 32*nb (the
	// weights must be packed for the same nb), rows per wave rw (tile = 4*rw rows).
	int nb, rw;
	// Frame look-ahead (Engine::processBatch): the same layer of `items` consecutive frames in one launch, item i at
	// in + i * inItemBytes / out + i * outItemBytes.  0 or 1 = one frame.  Honoured by launchConv (grid.z; no residual
	// operand then) and launchConvSplitK; the flow block launcher has its own item fields (FlowBlockLaunch).
	int items;
	long inItemBytes, outItemBytes;
	// developer launch plan of the runtime (host side only; null: none -- always in the product library)
	const DevPlan *plan;
};

// Zero-bordered activation layout of the generator trunk ("tower layout"):
// [towerRows(H)][towerPitch(W)][C] with the image at row/column offset 1.  The
// one-pixel border and the rows/columns beyond the image are zero and are never
// written, so the persistent tower kernel stages tiles with no bounds checks and
// gets the convolution's zero padding for free.
inline int towerPitch(int W) { return (W + 31) / 32 * 32 + 2; }
inline int towerRows(int H) { return (H + 7) / 8 * 8 + 2; }
inline std::size_t towerPixels(int H, int W) {
	return static_cast<std::size_t>(towerRows(H)) * towerPitch(W);
}
inline std::size_t towerOrigin(int W) { return static_cast<std::size_t>(towerPitch(W)) + 1; }

// Channel chunk shared by the launcher and the packer.
inline int convCK(int cin) { return cin % 64 == 0 ? 64 : (cin % 32 == 0 ? 32 : 16); }

// Tile shape for an H x W layer: prefer the shape with the most operand reuse
// (nb = 2 cout blocks, rw = 2 rows per wave) but fall back to smaller tiles until
// the launch has enough workgroups to occupy the chip; the coarse levels of the
// flow auto-encoder (34x60 ... 68x120 pixels) otherwise run on 40-80 of 256 CUs.
// >= 2 workgroups per CU: the generic kernel stages synchronously, so a second
// resident workgroup is what overlaps loads with MFMAs.
constexpr long kConvTargetWgs = 512;
inline void convTiling(int H, int W, int cout, int *nb, int *rw) {
	const int tilesX = (W + 31) / 32;
	int bestNb = 1, bestRw = 1;
	long bestWgs = -1;
	const int nbs[2] = {2, 1};
	const int rws[2] = {2, 1};
	for (int a = 0; a < 2; ++a) {
		if (cout % (32 * nbs[a]) != 0) continue;
		for (int b = 0; b < 2; ++b) {
			const long wgs = (long)tilesX * ((H + 4 * rws[b] - 1) / (4 * rws[b])) * (cout / (32 * nbs[a]));
			// the largest tile is kept as soon as it fills the chip once (least weight
			// restaging); smaller tiles must reach two workgroups per CU to pay
			if (wgs >= ((a == 0 && b == 0) ? 256 : kConvTargetWgs)) {
				*nb = nbs[a];
				*rw = rws[b];
				return;
			}
			if (wgs > bestWgs) {
				bestWgs = wgs;
				bestNb = nbs[a];
				bestRw = rws[b];
			}
		}
	}
	*nb = bestNb;
	*rw = bestRw;
}

void launchConv(DType dt, const ConvParams &p, hipStream_t stream);

// ---- a flow auto-encoder block as one launch (flow_kernels.hip) ---------------------
// conv A 3x3 cin -> cmid, activation, conv B 3x3 cmid -> cmid, [activation], [2x2
// max-pool]; `upsample`: `in` is the half-resolution tensor [H/2][W/2][cin] and the TF1
// bilinear x2 is part of the tile staging.  Weights: packConvWeights with nb = 1.
// Attribute-only launches: while a DryLaunchScope lives on the calling thread, launchFlowBlock and launchConvSplitK
// do everything a launch does on the host (shape checks, tile choice, the dynamic-LDS attribute of an instantiation
// used for the first time) but enqueue nothing -- Engine::prepareBatch runs a look-ahead pass's flow launches this
// way before it CAPTURES them (hipFuncSetAttribute is not something to do inside a stream capture).
bool launchesAreDry();
struct DryLaunchScope {
	DryLaunchScope();
	~DryLaunchScope();
	DryLaunchScope(const DryLaunchScope &) = delete;
	DryLaunchScope &operator=(const DryLaunchScope &) = delete;
};

constexpr int kFlowBatchMax = 8;  // frames per look-ahead pass of the flow net (Engine::processBatch)
struct FlowBlockLaunch {
	const void *in;
	const void *w1;
	const float *b1;
	const void *w2;
	const float *b2;
	void *out;      // [H][W][cmid], pooled [H/2][W/2][cmid]; f16 when outHead
	int H, W;       // the block's resolution (after the upsampling)
	int inPitch, outPitch;  // row pitches in pixels of the tensors as stored (0 = dense)
	int cin, cmid;  // cin padded to 16
	bool upsample, pool, outHead;
	// res_block (models.py:193-254): out = act(conv B(act(conv A(x))) + x), cin == cmid;
	// in / out may be tower-layout tensors (interior origin + pitch)
	bool residual;
	int act1, act2;  // ConvParams::relu codes
	float slope;
	// The flow net's first block (cin 16, cmid 32, pool) can build its input itself -- the work
	// of launchPackFrames, one launch less: packOut != nullptr.  `in` is then unused; the block
	// reads the u8 frame and the previous packed tensor, and writes the new packed tensor
	// [H][W][16] (H, W = the padded size) as a side effect.
	const std::uint8_t *packFrame;
	std::ptrdiff_t packFrameStride;
	const void *packPrev;
	void *packOut;
	int frameH, frameW, padTop, padLeft, numInputs;
	const unsigned *sums;
	// Frame look-ahead: the block of `items` (<= kFlowBatchMax) consecutive frames in one launch (grid.z), item i at
	// in + i * inItemBytes / out + i * outItemBytes; 0 or 1 = one frame.  With input packing, item i's current frame
	// is packFrames[i] and its history slot k is packFrames[i - k] where the launch holds that frame, else what
	// packPrev holds for it; only the LAST item writes packOut (the history of the frame after the batch), and
	// `sums` must be null.  packFrame / packFrameStride are ignored when items > 1.
	int items;
	long inItemBytes, outItemBytes;
	const std::uint8_t *packFrames[kFlowBatchMax];
	std::ptrdiff_t packFrameStrides[kFlowBatchMax];
	// Independent items (Engine::processGroup): item i of `items` (>= 1) is the next frame of a stream of its own --
	// frame packFrames[i], history packPrevs[i], new history written to packOuts[i] by every item; per item the
	// arithmetic of a one-frame launch.  packPrev / packOut / packFrame are ignored, `sums` must be null.
	bool independentItems;
	const void *packPrevs[kFlowBatchMax];
	void *packOuts[kFlowBatchMax];
	// Cut-aware history (a look-ahead pass of a runtime whose scene detector restarts the recurrence: items > 1, not
	// independent): device array of `items` ints, read by the kernel -- ScenePassState::cutAt.  With c = cutAt[i] >= 0,
	// item i's history slot h is frame i - h while i - h >= c and exact +0 otherwise, and nothing is taken from
	// packPrev; with cutAt[i] < 0 the arithmetic above.  The last item's record, written to packOut, is that record.
	const int *cutAt;
	const DevPlan *plan;  // developer launch plan of the runtime (null: none -- always in the product library)
};
// H x W: the block's resolution (the 128-filter blocks run as one launch only where their 2-row tiles are ONE round of the
// chip: flow_kernels.hip); 0 = shape only
bool flowBlockSupported(int cin, int cmid, bool upsample, bool pool, bool outHead, int H = 0, int W = 0);
void launchFlowBlock(DType dt, const FlowBlockLaunch &q, hipStream_t stream);

// One 3x3 convolution of the flow net's coarse levels (cin 128 / 256, a few thousand pixels), the
// input channels split over the eight waves of a workgroup (splitk_kernels.hip, conv_splitk_kernel).
// Weights: packConvWeights with nb = 1.  `zeros`: >= 16 zero bytes of device memory.
bool convSplitKSupported(const ConvParams &p);
void launchConvSplitK(DType dt, const ConvParams &p, const void *zeros, hipStream_t stream);

// Persistent 3x3 64->64 kernel of the generator tower.  in/res/out must be
// tower-layout tensors addressed at their interior origin with
// pitch == towerPitch(W); other shapes fall back to launchConv.
void launchConvTower(DType dt, const ConvParams &p, hipStream_t stream);

// ---- 8-bit (e4m3) residual-block convolution (fp8_kernels.hip, scheme: fp8.h) ---
// All tensors are tower-layout ALLOCATION STARTS (row -1, column -1 of the image).
struct Fp8TowerParams {
	const void *in8;      // e4m3 input, 64 B per pixel
	const void *weights;  // packFp8TowerWeights().w on the device
	const int *scaleA;    // [64] E8M0 codes per output channel
	const float *bias;    // [64]
	void *stream;         // second conv of a block: the 16-bit residual stream, updated in place
	                      // (out = relu(conv + stream)); nullptr: first conv (out = relu(conv))
	void *out8;           // e4m3 copy of the output (the next convolution's input)
	int inExp;            // the input tensor holds e4m3(x * 2^inExp)
	int outExp;           // the output copy holds e4m3(y * 2^outExp)
	int H, W;
	int leaky;            // `activation: lrelu` models: LeakyReLU(slope) instead of ReLU
	float slope;
};
void launchConvTowerFp8(DType dt, const Fp8TowerParams &p, hipStream_t stream);
// One residual block of the 8-bit tower per launch (the intermediate e4m3 tensor stays in
// LDS): in8 -> conv A -> ReLU -> e4m3(2^midExp) -> conv B -> + stream -> ReLU -> stream
// (in place) and out8 = e4m3(stream * 2^outExp).  in8 / out8 must be different tensors.
struct Fp8BlockLaunch {
	const void *in8;
	void *out8;
	void *stream;
	const void *w1, *w2;      // packFp8TowerWeights().w of the two convolutions
	const int *scaleA1, *scaleA2;
	const float *b1, *b2;
	int inExp, midExp, outExp;
	int H, W;
	int leaky;            // `activation: lrelu` models
	float slope;
};
void launchResBlockFp8(DType dt, const Fp8BlockLaunch &q, hipStream_t stream);
// e4m3(max(x, 0) * 2^exponent) of a 16-bit tower tensor (allocation starts); leaky: the tensor
// is a LeakyReLU output, e4m3(clamp(x * 2^exponent, +-448))
void launchQuantizeTower(DType dt, const void *in, void *out8, int H, int W, int exponent, bool leaky,
    hipStream_t stream);

// ---- resident tower: every residual-block convolution in one launch --------
// in: first layer's input addressed at image pixel (0,0) with row pitch inPitch
// (0 = dense W); out: tower-layout tensor addressed at its interior origin.
// weights: nLayers consecutive 64->64 3x3 kernels in packConvWeights (nb = 2)
// order, bias nLayers x 64.  hasHead: layer 0 is a plain conv+ReLU (generator
// conv_1), residual blocks (conv, conv + skip) follow.
// mailbox (residentMailboxBytes) carries the halo exchange between neighbouring
// workgroups as self-validating 16-byte slots; counters (residentCounterBytes) holds
// each region's publish counts, from which the slot epochs follow -- both zeroed
// together, once, and again after a failed launch; *error is written (non-zero) if a
// bounded wait expires.  Needs GX*GY co-resident workgroups.
struct ResidentTowerParams {
	const void *in;
	int inPitch;
	int hasHead;
	void *out;
	const void *weights;
	const float *bias;
	void *mailbox;
	unsigned *counters;
	unsigned *error;
	void *debug;  // optional: GX*GY*4*8 u64 cycle sums (diagnostic variant 4 only)
	int H, W;
	int GX, GY, RH;
	int nLayers;
	// `activation: lrelu` models (models.py:24-27): LeakyReLU(slope) instead of ReLU after every
	// layer; the mailbox must then be residentMailboxBytes(GX, GY, true) (twice the slots: a
	// LeakyReLU output has no free sign bit for the slot epoch)
	int leaky;
	float slope;
	// Optional fused generator tail (tailW1 != nullptr): instead of writing the last
	// layer to `out`, every workgroup runs the tail (launchTailFused's arithmetic) on
	// its LDS-resident region and writes the HR state and the BGRX frame directly.
	const void *tailW1;       // convT1 as 1x1 conv 64->128, packConvWeights order with nb = 2
	const float *tailB1;      // [128]
	const void *tailW2;       // packTailWeights fragments
	const float *tailB2;      // [3]
	const std::uint8_t *frame;
	std::ptrdiff_t frameStride;
	void *state;              // f16 [4H][4W][4]
	std::uint8_t *outU8;
	std::ptrdiff_t outStride;
	const unsigned *sums;     // normalize_brightness channel sums or nullptr
};
bool residentTowerGeometry(int H, int W, int numCUs, int *GX, int *GY, int *RH);
std::size_t residentMailboxBytes(int GX, int GY, bool leaky = false);
// every region of the frame has the shape the fast schedule of the resident tower is built for
bool residentTowerFastGeometry(int H, int W, int GX, int GY, int RH);
void setResBlockPlain(int on);       // tests / JU_RES_BLOCK=plain: res_block_kernel instead of res_block_pipe_kernel
bool resBlockPlain();
void setResidentTowerFast(int on);  // tests / JU_TOWER_FAST=0: the general schedule everywhere
void setFp8BlockForm(int form);     // tests / JU_FP8_BLOCK: res_block_fp8_kernel as 0 = by geometry, 1 = solo, 2 = duo
bool residentTowerFast();
// rows of the fast schedule's work unit for this geometry: 4 (row quads: every region 32 x 16 or 32 x 14) or 2 (row
// pairs); ReLU towers only -- LeakyReLU towers always run pairs
int residentTowerUnitRows(int H, int W, int GX, int GY, int RH);
void setResidentTowerUnitRows(int rows);  // tests: 2 = row pairs everywhere, anything else the default
inline std::size_t residentCounterBytes(int GX, int GY) {
	return (static_cast<std::size_t>(GX) * GY * 2 * sizeof(unsigned) + 63) / 64 * 64;
}
void launchResidentTower(DType dt, const ResidentTowerParams &p, hipStream_t stream);

// Timing-only ablation switch of the tower kernel (0 = product kernel).
// the resident tower's K loops run v_mfma_f32_16x16x32 (weights packed by packTowerWeightsM16, model.cpp) or 32x32x16
bool residentTowerM16();
void setTowerVariant(int variant);
int towerVariant();
// Test hook: launch the resident tower `n` workgroups short, so that the bounded
// neighbour waits expire (exercises the engine's fallback to the per-layer path).
void setResidentFault(int n);
int residentFaultForTests();

// ---- resident 8-bit tower (tower8_kernels.hip): every residual block of the e4m3 tower in
// one launch; the 16-bit stream and the two e4m3 tiles stay in LDS.  in / out: 16-bit tower
// tensors (allocation starts): generator conv_1's output in, the last block's stream out.
// Per convolution i of the 2 B: weights (packFp8TowerWeights, 36864 B each), scaleA[i][64],
// bias[i][64], scaleB[i] (E8M0 code of its input tensor's scale), outMul[i] (2^e of the
// e4m3 tensor its output feeds); outMul[2 B] = the scale of the tower's input tensor.
struct ResidentTower8Params {
	const void *in;
	void *out;
	const void *weights;
	const int *scaleA;
	const float *bias;
	const int *scaleB;
	const float *outMul;
	void *mailbox;       // residentMailboxBytes8, zeroed with the counters
	unsigned *counters;  // residentCounterBytes
	unsigned *error;
	int H, W;
	int GX, GY, RH;
	int nLayers;
	int leaky;           // `activation: lrelu` models; the mailbox is then residentMailboxBytes8(GX, GY, true)
	float slope;
	void *debug;         // developer builds (-DJU_T8_PROF, tools/tower8_phases.py): [regions][4 waves][8] cycle sums; unused otherwise
};
std::size_t residentMailboxBytes8(int GX, int GY, bool leaky = false);
void launchResidentTower8(DType dt, const ResidentTower8Params &p, hipStream_t stream);

// ---- flow-net helpers -------------------------------------------------------
// cur frame (u8 BGRX, signed row stride) + previous packed history ->
// packed [PH][PW][16]: ch 0-2 current frame (x/255-0.5, zero in the pad border),
// ch 3-11 = previous ch 0-8, ch 12-15 zero.
void launchPackFrames(DType dt, const std::uint8_t *frame, std::ptrdiff_t frameStride,
    const void *prevPacked, void *curPacked, int H, int W, int PH, int PW, int padTop,
    int padLeft, int numInputs, const unsigned *sums, hipStream_t stream);

// normalize_brightness (reference models.py:772-779): exact integer sums of the B, G, R
// bytes of the frame -> three 64-bit sums as (low, high) word pairs sums[0..5]; the kernels taking
// `sums` derive the scalar brightness from them (brightnessOf; nullptr = feature off).
void launchFrameSums(const std::uint8_t *frame, std::ptrdiff_t frameStride, int H, int W,
    unsigned *sums, hipStream_t stream);

// [nPix][16] 16-bit -> channels 0..15 of [nPix][64] records (the rest is not written).
void launchExpandChannels(DType dt, const void *in16, void *out64, int nPix, hipStream_t stream);
void launchMaxPool2(DType dt, const void *in, void *out, int H, int W, int C,
    hipStream_t stream);  // in [H][W][C] -> out [H/2][W/2][C]

// TF1 asymmetric bilinear, in [H][W][C] -> out [2H][2W][C]; items > 1: the dense tensors of a look-ahead launch's
// frames, one after the other
void launchUpsample2(DType dt, const void *in, void *out, int H, int W, int C, hipStream_t stream, int items = 1);

// ---- warp + space-to-depth + concat ----------------------------------------
// state : previous HR output, f16 [4H][4W][4] (B,G,R,0)
// flow  : f16 [PH][PW][32], channel (i*4+j)*2 + {dy,dx} (depth-to-space is free)
// frame : current LR frame, u8 BGRX
// out   : generator input NHWC [H][W][64] in the packed channel order
//         ch = i*16 + j*3 + c for the warped HR pixel (4h+i, 4w+j, c),
//         ch 12,13,14 = current LR frame B,G,R, other spare slots zero.
// preWarpOut (may be null): the warped previous output itself, f16 [4H][4W][4], for
// the temporal filter below.
// outU8 / outStride (outU8 may be null): the output_flow model variant -- the launch also writes the BGRX
// frame [4H][4W] of the warped previous output, byte = trunc(clamp((v + 0.5) * 255, 0, 255)) of the value v
// stored in `out` (its type, widened to f32), X = 0.  4-byte aligned, any signed stride that is a multiple of
// 4; 16-byte stores where a row is 16-byte aligned, 8- or 4-byte ones otherwise.  Null: the launch is the
// plain kernel, which has no such parameter.
void launchWarpPack(DType dt, const void *state, const void *flow,
    const std::uint8_t *frame, std::ptrdiff_t frameStride, void *out, int outPitch, int H, int W, int PW,
    int padTop, int padLeft, const unsigned *sums, void *preWarpOut, std::uint8_t *outU8, std::ptrdiff_t outStride,
    hipStream_t stream);  // out at image pixel (0, 0), outPitch in pixels (0: W)

// The generator input of a flow-free model (flow_arch "none", remove_flow.py): the LR frame's B,G,R as
// slots 12..14 of each pixel's 64-slot record, converted exactly as launchWarpPack converts them.  One
// 16-byte store per pixel covers slots 8..15 ({0,0,0,0,B,G,R,0}); the other slots of `out` must already
// be zero (allocated zeroed, written by nothing else).  `frame` / `frameStride`: any address and any
// signed stride (byte loads where the pixel is not 4-byte aligned).
void launchLrPack(DType dt, const std::uint8_t *frame, std::ptrdiff_t frameStride, void *out, int outPitch, int H,
    int W, hipStream_t stream);  // out at image pixel (0, 0), outPitch in pixels (0: W)

// Temporal moving-average output filter with the scene-cut gate of
// scripts/inference/onnx/frame_moving_avg.py:146-302, every mode of that script: global or
// windowed gate (window in HR pixels), sign or tanh(gain * .) gate, L1 / L2 norm, limited
// pre_warp, luma weighting.  state: the new HR state written by the tail (f16 [4H][4W][4],
// generator output minus brightness), rewritten in place together with the u8 frame;
// acc: temporalAccWords(...) 64-bit words of scratch (one 32.32 fixed-point sum per window).
// The filtered value v mixes in pre_warp, which is not confined to +-0.5 (least of all with
// normalize_brightness, when the brightness moves between frames): the byte saturates,
// trunc(clamp((v + 0.5) * 255, 0, 255)), the fed-back state does not (the reference feeds back
// the unclipped tensor too; its own byte is a C++ float -> uint8_t cast, cuda_convert.cc.cu:76-81,
// which the language leaves undefined out of range).  A global sign gate that says "scene cut"
// leaves both as the tail wrote them.
struct TemporalParams {
	float strength, threshold, gain;
	int window;   // 0 = one global mean
	int l2, limit, luma;
};
std::size_t temporalAccWords(int H, int W, int window);
void launchTemporalFilter(void *state, const void *preWarp, std::uint8_t *outU8,
    std::ptrdiff_t outStride, int H, int W, const unsigned *sums, unsigned long long *acc,
    const TemporalParams &tp, hipStream_t stream);

// ---- generator tail ---------------------------------------------------------
// y     : [H][W][128] 16-bit = relu(BN(convT1)) with channel (a*2+b)*32 + o
// w2    : f32 [2][2][3][32] (convT2 kernel, keras layout), b2 f32 [3]
// frame : current LR frame u8 BGRX (bilinear x4 skip)
// stateOut : f16 [4H][4W][4]; outU8 : BGRX [4H][4W][4], X = 0
void launchTail(DType dt, const void *y, const float *w2, const float *b2,
    const std::uint8_t *frame, std::ptrdiff_t frameStride, void *stateOut,
    std::uint8_t *outU8, std::ptrdiff_t outStride, int H, int W, const unsigned *sums,
    hipStream_t stream);  // (the activation of convT1 is applied by the conv launch that makes y)

// Fused tail: both transposed convs on the matrix cores + tanh + skip + clip + pack.
// x: trunk addressed at pixel (0,0) with pitch xPitch (0 = dense); w1/b1: convT1 as a
// 1x1 conv 64->128 (packConvWeights, nb = 2) and its folded bias; w2: convT2 A fragments
// from packTailWeights(); b2 [3]; needs 64 trunk channels and 32 mid channels.
struct TailFusedLaunch {
	const void *x;
	int xPitch;
	const void *w1;
	const float *b1;
	const void *w2;
	const float *b2;
	const std::uint8_t *frame;
	std::ptrdiff_t frameStride;
	void *state;
	std::uint8_t *outU8;
	std::ptrdiff_t outStride;
	const unsigned *sums;
	int H, W;
	float slope;  // activation after convT1: < 0 = ReLU, else LeakyReLU with this negative slope
};
void launchTailFused(DType dt, const TailFusedLaunch &p, hipStream_t stream);

// ---- staging ----------------------------------------------------------------
// Row-wise device copy with signed strides (bottom-up frames).
void launchCopyRows(const std::uint8_t *src, std::ptrdiff_t srcStride, std::uint8_t *dst,
    std::ptrdiff_t dstStride, std::size_t rowBytes, std::size_t rows, hipStream_t stream);

// ---- frame formats beside BGRX <-> BGRX (colour_kernels.hip; docs/yuv_io.md) -------------------------------------------
// THE list of the frame formats: the values of JU_FMT_* (include/joshupscale_amd.h).  4:2:0: planes Y, U, V (I420 / YV12,
// I010) or Y, interleaved UV (NV12, P010); P010 / I010: 16-bit little-endian samples, the 10-bit value in the upper / the
// low bits.  From 16 on, 4:2:2 (chroma rows of full height) and 4:4:4: packed YUY2 / UYVY (ONE plane, 2 bytes per pixel),
// I422 and I210 (Y, U, V; I210 words as I010), P210 (Y, UV; words as P010), I444 and I410 (three full planes; I410 words as
// I010).  From 32 on, RGB (no colour space): packed BGR24 / RGB24 (3 bytes per pixel), RGBX, BGRX64 (four 16-bit words per
// pixel) and BGR96F (three f32 per pixel, 0..255) are ONE plane; RGBP8 / RGBP10 / RGBP16 / RGBPH / RGBPS are planes R, G, B
// of bytes, words (RGBP10: the value in the low 10 bits), f16 and f32 (0..1).  Packed 10-bit, ONE plane of little-endian
// words each: V210 (4:2:2; six pixels in four 32-bit words of three samples), Y210 (4:2:2; 16-bit words Y0 U Y1 V, words
// as P010), Y410 (4:4:4) and X2RGB10 / X2BGR10 (RGB): one 32-bit word of three samples per pixel, bits 30-31 unused.
enum class PixelFormat : int {
	Bgrx = 0, I420 = 1, Nv12 = 2, P010 = 3, I010 = 4,
	Yuy2 = 16, Uyvy = 17, I422 = 18, P210 = 19, I210 = 20, I444 = 24, I410 = 25,
	Bgr24 = 32, Rgb24 = 33, Rgbx = 34, Bgrx64 = 35, Rgbp8 = 36, Rgbp10 = 37, Rgbp16 = 38, Rgbph = 39, Rgbps = 40, Bgr96f = 41,
	X2bgr10 = 44, X2rgb10 = 45, V210 = 48, Y210 = 49, Y410 = 50
};
// (the same values as integers: what a launcher's `format` argument and a kernel's `template <int F>` parameter hold)
constexpr int fmt(PixelFormat f) { return static_cast<int>(f); }
constexpr int kI420 = fmt(PixelFormat::I420), kNv12 = fmt(PixelFormat::Nv12), kP010 = fmt(PixelFormat::P010),
              kI010 = fmt(PixelFormat::I010), kYuy2 = fmt(PixelFormat::Yuy2), kUyvy = fmt(PixelFormat::Uyvy),
              kI422 = fmt(PixelFormat::I422), kP210 = fmt(PixelFormat::P210), kI210 = fmt(PixelFormat::I210),
              kI444 = fmt(PixelFormat::I444), kI410 = fmt(PixelFormat::I410), kBgr24 = fmt(PixelFormat::Bgr24),
              kRgb24 = fmt(PixelFormat::Rgb24), kRgbx = fmt(PixelFormat::Rgbx), kBgrx64 = fmt(PixelFormat::Bgrx64),
              kRgbp8 = fmt(PixelFormat::Rgbp8), kRgbp10 = fmt(PixelFormat::Rgbp10), kRgbp16 = fmt(PixelFormat::Rgbp16),
              kRgbph = fmt(PixelFormat::Rgbph), kRgbps = fmt(PixelFormat::Rgbps), kBgr96f = fmt(PixelFormat::Bgr96f),
              kV210 = fmt(PixelFormat::V210), kY210 = fmt(PixelFormat::Y210), kY410 = fmt(PixelFormat::Y410),
              kX2rgb10 = fmt(PixelFormat::X2rgb10), kX2bgr10 = fmt(PixelFormat::X2bgr10);

// THE table of the frame formats beside BGRX: the C API, the engine and the launchers below classify a format through it
// alone.  planes: 3 planar (Y, U, V / R, G, B), 2 semi-planar (Y, UV), 1 packed (pixelBytes per pixel).
struct YuvFormatInfo {
	int value;
	const char *name;
	int sampling;     // 420, 422 or 444; 0: an RGB format (no colour space, no chroma planes)
	int planes;
	int bits;         // 8, or 10 in 16-bit words; RGB: 8, 10, 16 (words and f16) or 32 (f32)
	int sampleBytes;  // 1, 2 or 4: what a plane's address and stride must be a multiple of
	int pixelBytes;   // packed formats: bytes per pixel (2, 3, 4, 8 or 12), or kGroupedRow (V210: rows of whole 16-byte
	                  // groups of six pixels -- planeShape, frame_geometry.h); else 0
	constexpr bool rgb() const { return sampling == 0; }
	constexpr bool words10() const { return bits == 10 && sampling != 0; }  // 10-bit YUV words (not RGBP10): the 10-bit coefficients
	constexpr bool deep() const { return bits > 8; }  // more than the 8-bit frame holds: encodable from the f16 state
	constexpr bool perRow() const { return sampling != 420; }  // decode and encode run a strip per row (4:2:0: per row pair)
};
constexpr int kGroupedRow = -1;
inline constexpr YuvFormatInfo kFormatTable[] = {
    {kI420, "I420", 420, 3, 8, 1, 0},    {kNv12, "NV12", 420, 2, 8, 1, 0},    {kP010, "P010", 420, 2, 10, 2, 0},
    {kI010, "I010", 420, 3, 10, 2, 0},   {kYuy2, "YUY2", 422, 1, 8, 1, 2},    {kUyvy, "UYVY", 422, 1, 8, 1, 2},
    {kI422, "I422", 422, 3, 8, 1, 0},    {kP210, "P210", 422, 2, 10, 2, 0},   {kI210, "I210", 422, 3, 10, 2, 0},
    {kI444, "I444", 444, 3, 8, 1, 0},    {kI410, "I410", 444, 3, 10, 2, 0},   {kBgr24, "BGR24", 0, 1, 8, 1, 3},
    {kRgb24, "RGB24", 0, 1, 8, 1, 3},    {kRgbx, "RGBX", 0, 1, 8, 1, 4},      {kBgrx64, "BGRX64", 0, 1, 16, 2, 8},
    {kRgbp8, "RGBP8", 0, 3, 8, 1, 0},    {kRgbp10, "RGBP10", 0, 3, 10, 2, 0}, {kRgbp16, "RGBP16", 0, 3, 16, 2, 0},
    {kRgbph, "RGBPH", 0, 3, 16, 2, 0},   {kRgbps, "RGBPS", 0, 3, 32, 4, 0},   {kBgr96f, "BGR96F", 0, 1, 32, 4, 12},
    {kV210, "V210", 422, 1, 10, 4, kGroupedRow}, {kY210, "Y210", 422, 1, 10, 2, 4}, {kY410, "Y410", 444, 1, 10, 4, 4},
    {kX2rgb10, "X2RGB10", 0, 1, 10, 4, 4}, {kX2bgr10, "X2BGR10", 0, 1, 10, 4, 4}};
constexpr int kFormatValueEnd = kY410 + 1;  // (one past the largest value of the table)
inline const YuvFormatInfo *yuvFormatInfo(int value) {  // nullptr: not in the table
	for (const YuvFormatInfo &f : kFormatTable) {
		if (f.value == value) return &f;
	}
	return nullptr;
}
inline const YuvFormatInfo &formatInfo(int value) {
	const YuvFormatInfo *info = yuvFormatInfo(value);
	if (info == nullptr) throw std::invalid_argument("unknown frame format " + std::to_string(value));
	return *info;
}
inline const YuvFormatInfo &formatInfo(PixelFormat f) { return formatInfo(fmt(f)); }

// A frame's `colorspace` = JU_CS_* | JU_CHROMA_* (include/joshupscale_amd.h): the low byte is the matrix and range -- 0
// BT.601 limited, 1 BT.601 full, 2 BT.709 limited, 3 BT.709 full, 4 BT.2020 (non-constant luminance) limited, 5 BT.2020
// full -- and bits 8-9 the chroma siting: where chroma sample (i, j) sits among the luma samples at integer (x, y).  Left
// (2i, 2j + 1/2): MPEG-2 / H.264; centre (2i + 1/2, 2j + 1/2): JPEG / MPEG-1; top-left (2i, 2j): H.273 type 2.
constexpr int kChromaLeft = 0, kChromaCenter = 1, kChromaTopLeft = 2;
constexpr int kColourMatrixEnd = 6;  // (one past the largest matrix value)
struct ColourSpace {
	int matrix = 0, siting = kChromaLeft;
};
// THE split of the int, for the frame check, the coefficient functions and the launchers: why a value is refused ("" for
// a good one: then *cs, where given, is set), in the frame check's words -- `side`: "input " / "output " or ""
inline std::string colourSpaceFault(int colorspace, const std::string &side, ColourSpace *cs = nullptr) {
	if (colorspace < 0 || (colorspace >> 10) != 0) {
		return "unknown " + side + "colour space " + std::to_string(colorspace) + " (bits above bit 9 are set)";
	}
	if (((colorspace >> 8) & 3) > kChromaTopLeft) return "unknown " + side + "chroma siting " + std::to_string((colorspace >> 8) & 3);
	if ((colorspace & 0xff) >= kColourMatrixEnd) return "unknown " + side + "colour space " + std::to_string(colorspace & 0xff);
	if (cs != nullptr) *cs = ColourSpace{colorspace & 0xff, (colorspace >> 8) & 3};
	return std::string();
}
inline ColourSpace splitColourSpace(int colorspace) {
	ColourSpace cs;
	const std::string fault = colourSpaceFault(colorspace, "", &cs);
	if (!fault.empty()) throw std::invalid_argument(fault);
	return cs;
}
// the siting a format's kernels distinguish: 4:4:4 and RGB have none, 4:2:2 has the horizontal axis only (top-left = left)
inline int effectiveSiting(const YuvFormatInfo &info, int siting) {
	if (info.sampling == 420) return siting;
	return (info.sampling == 422 && siting == kChromaCenter) ? kChromaCenter : kChromaLeft;
}

// Planes of a frame: Y, U, V / R, G, B (planar), Y and one interleaved plane u (semi-planar; v unused) or y alone (packed:
// rows of pixelBytes x width bytes; V210: 16 x ceil(width / 6)).  Chroma planes have height / 2 (4:2:0) or height rows of width / 2 (4:2:0, 4:2:2;
// interleaved: width) or width (4:4:4) samples.  Pointers address the first logical row, strides are bytes and may be
// negative; addresses and strides are multiples of the sample size (1, 2 or 4 bytes), any alignment beyond that.
struct YuvPlanes {
	std::uint8_t *y = nullptr, *u = nullptr, *v = nullptr;
	std::ptrdiff_t yStride = 0, uStride = 0, vStride = 0;
};
// The three launches of the colour staging, for any format of the table (std::invalid_argument for another value).  Each
// chooses, from `colorspace` (splitColourSpace above; std::invalid_argument for a value it refuses), the coefficients and
// the kernel's siting; an RGB format's `colorspace` is not read.  4:2:0 needs an even width and height, 4:2:2 an even
// width.  The definitions are tests/chroma_siting_reference.py (every siting and matrix), which with the left siting is
// tests/yuv_reference.py, yuv10_reference.py (10-bit words; the 16-bit sample P of an encode) and
// yuv_sampled_reference.py (4:2:2 / 4:4:4), and rgb_reference.py (inputs reduced to the u8 frame the network consumes;
// 8-bit outputs permute the frame's bytes).
// planes -> BGRX rows (X = 0)
void launchDecodeFrame(int format, int colorspace, const YuvPlanes &src, std::uint8_t *dst, std::ptrdiff_t dstStride,
    int width, int height, hipStream_t stream);
// BGRX rows (X ignored; any alignment, signed stride) -> planes; the deep formats: P = 257 u8, u8 / 255, u8
void launchEncodeFrame(int format, int colorspace, const std::uint8_t *src, std::ptrdiff_t srcStride, const YuvPlanes &dst,
    int width, int height, hipStream_t stream);
// the dense f16 state [height][width][4] (B, G, R, 0; 16-byte aligned) -> planes, the deep formats only
// (std::invalid_argument for another): P = floor((s + 0.5) * 65536), saturated
void launchEncodeState(int format, int colorspace, const void *state, const YuvPlanes &dst, int width, int height,
    hipStream_t stream);
// the dense u16 frame [height][width][4] (B, G, R, unused; 8-byte aligned: what launchScaleState writes) -> planes, the
// deep formats only (std::invalid_argument for another): the sample is P itself -- 10-bit YUV as from the state, W16 = P,
// W10 = P >> 6, the unit floats f32(P) / 65535 (one division; RGBPH that as f16, to nearest even), BGR96F f32(P) / 257
// (tests/output_reference.py)
void launchEncodeFrame16(int format, int colorspace, const std::uint16_t *frame, const YuvPlanes &dst, int width, int height,
    hipStream_t stream);

// The inputs of a look-ahead pass (Engine::processFrames) that are not BGRX, decoded in one launch: item i of `count` (1 ..
// kFlowBatchMax) = format, planes, coefficients and BGRX destination of one frame; all frames width x height.  Per item
// the bytes of launchDecodeFrame.  YuvDecodeItems is the launch's by-value argument.
struct YuvDecode {  // x 65536, rounded half away from zero (tests/yuv_reference.py); oy = luma offset (0 full range)
	int ky, krv, kbu, kgu, kgv, oy;
};
struct YuvDecodeItem {
	YuvPlanes src;
	YuvDecode k;  // (an RGB item: not read)
	std::uint8_t *dst = nullptr;
	std::ptrdiff_t dstStride = 0;
	int format = 0;
	int siting = kChromaLeft;  // effectiveSiting of the frame (in what was padding: the item's size is unchanged)
};
struct YuvDecodeItems {
	YuvDecodeItem item[kFlowBatchMax];
};
static_assert(sizeof(YuvDecodeItems) <= 832, "the by-value argument of the items kernel must not grow");
// the item of one frame, coefficients included (the checks of launchDecodeFrame on format and colour space)
YuvDecodeItem yuvDecodeItem(int format, int colorspace, const YuvPlanes &src, std::uint8_t *dst, std::ptrdiff_t dstStride);
// (a per-row item in the pass: strips x height threads per item, of which a 4:2:0 item's upper half returns at once)
void launchYuv420ToBgrxItems(const YuvDecodeItems &items, int count, int width, int height, hipStream_t stream);
// The sized form (the members of a group pass, Engine::runGroupPass: a scaled member's input is its source size, the
// others' the model's): every item carries its own width and height.  The grid is sized for the largest item; the
// workgroups beyond an item's own extent return at once.  Per item the bytes of launchDecodeFrame at that item's size.
struct YuvDecodeSizedItems {
	YuvDecodeItem item[kFlowBatchMax];
	int width[kFlowBatchMax] = {};
	int height[kFlowBatchMax] = {};
};
static_assert(sizeof(YuvDecodeSizedItems) <= 896, "the by-value argument of the sized items kernel must not grow");
void launchYuvToBgrxItemsSized(const YuvDecodeSizedItems &items, int count, hipStream_t stream);

// ---- source stage (source_kernels.hip; docs/source_stage.md): sources of any size, masked pass-through ---------------
// One axis of the scaler, N source samples -> M destination samples, in integers (buildScaleAxis is the definition;
// tests/source_reference.py and tests/scale_filter_reference.py restate it): per destination index the first source
// index, the tap count (at most kScaleMaxTaps) and the taps, 16 bits each, summing to exactly 4096.  The filters are the
// values of JU_SCALE_* (include/joshupscale_amd.h): the triangle's taps are u16; the two cubic filters' taps can be
// negative and are read as i16, and their rows hold sum |q| <= kScaleAbsSumMax (what the signed kernels' widths rest on).
constexpr int kScaleMaxTaps = 33;
constexpr int kScaleTapPitch = kScaleMaxTaps + 1;  // u16 per destination index: the taps, then the tap count
constexpr int kSourceAxisMin = 2, kSourceAxisMax = 8192, kSourceRatioMax = 16;
constexpr int kScaleTriangle = 0, kScaleCatmullRom = 2, kScaleMitchell = 3;  // (1 is reserved and refused)
constexpr int kCubicDownMax = 8;       // a cubic filter's support is twice the triangle's: 33 taps at a factor of 8
constexpr int kScaleAbsSumMax = 6144;
inline bool scaleFilterKnown(int filter) { return filter == kScaleTriangle || filter == kScaleCatmullRom || filter == kScaleMitchell; }
// the largest N / M of a filter (M / N: kSourceRatioMax for all of them)
inline int scaleDownMax(int filter) { return filter == kScaleTriangle ? kSourceRatioMax : kCubicDownMax; }
// "" for a known filter, else the message ju_set_source_size / ju_set_output_size and their Python twins give
std::string scaleFilterProblem(int filter);
struct ScaleAxisHost {
	int n = 0, m = 0;
	int filter = kScaleTriangle;
	std::vector<int> start;            // [m]
	std::vector<std::uint16_t> taps;   // [m][kScaleTapPitch]; i16 in the same words for a cubic filter
};
// std::invalid_argument unless the filter is known, 1 <= n, m, m <= 16 n and n <= 16 m (triangle) or 8 m (cubic): the
// bounds that keep an axis at 33 taps
ScaleAxisHost buildScaleAxis(int n, int m, int filter = kScaleTriangle);
// The same limits as one message for ju_set_source_size and its Python twin: "" when srcW x srcH may feed a model of
// inW x inH through `filter`
std::string sourceSizeProblem(std::size_t srcW, std::size_t srcH, std::size_t inW, std::size_t inH, int filter = kScaleTriangle);
struct ScaleAxisDev {
	const int *start = nullptr;
	const std::uint16_t *taps = nullptr;
	int filter = kScaleTriangle;       // (the host's choice of kernel form; the kernels take the two pointers)
};
// BGRX rows of srcW x srcH -> BGRX rows of dstW x dstH (X = 0): out = (sum qy qx src + 2^23) >> 24 per channel, clamped
// to 0 .. 255 where an axis' filter is cubic (the signed form of the kernel; the triangle's form is unchanged).  Any
// byte alignment, signed strides.  x / y: the device copies of buildScaleAxis(srcW, dstW) / (srcH, dstH); spanX: the most
// source columns a tile of kScaleTileW destination columns reads (scaleSpan of the x axis).
constexpr int kScaleTileW = 32, kScaleTileH = 8;
int scaleSpan(const ScaleAxisHost &x);
void launchScaleBgrx(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, int srcH, std::uint8_t *dst,
    std::ptrdiff_t dstStride, int dstW, int dstH, const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX,
    hipStream_t stream);
// The sources of a look-ahead pass scaled in one launch (Engine::runBatch): item i of `count` (1 .. kFlowBatchMax) = the
// source and destination rows of one frame, any byte alignment and signed strides each; sizes, tables and spanX shared by
// all items.  Per item the bytes of launchScaleBgrx.  ScaleItems is the launch's by-value argument.
struct ScaleItem {
	const std::uint8_t *src = nullptr;
	std::ptrdiff_t srcStride = 0;
	std::uint8_t *dst = nullptr;
	std::ptrdiff_t dstStride = 0;
};
struct ScaleItems {
	ScaleItem item[kFlowBatchMax];
};
static_assert(sizeof(ScaleItems) <= 256, "the by-value argument of the items kernel must not grow");
void launchScaleBgrxItems(const ScaleItems &items, int count, int srcW, int srcH, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream);
// The sources of a group pass scaled in one launch (Engine::runGroupPass; docs/source_stage.md "Group passes"): the members
// differ in source size, filter and tables, so each carries its own -- source rows and width, both axes' tables, the pitch
// of its LDS tile and its kernel form -- and only the destination size, the model's input, is the launch's.  Per member
// the bytes of launchScaleBgrx.  ScaleMembers is the launch's by-value argument.
struct ScaleMember {
	const std::uint8_t *src = nullptr;
	std::ptrdiff_t srcStride = 0;
	std::uint8_t *dst = nullptr;
	std::ptrdiff_t dstStride = 0;
	const int *xStart = nullptr, *yStart = nullptr;
	const std::uint16_t *xTaps = nullptr, *yTaps = nullptr;
	int srcW = 0;
	int pitch = 0;   // words per row of the member's LDS tile: spanX + spanX / 32 + 1
	int cubic = 0;   // the signed form of the tile (Catmull-Rom, Mitchell)
	int reserved = 0;
};
struct ScaleMembers {
	ScaleMember member[kFlowBatchMax];
};
static_assert(sizeof(ScaleMembers) <= 640, "the by-value argument of the members kernel must not grow");
// one member's row of the table: std::invalid_argument for a NULL pointer, a width below 1, a span that is no multiple of
// 4, axes of two filters, or a tile beyond the 64 KB of LDS
ScaleMember scaleMember(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, std::uint8_t *dst, std::ptrdiff_t dstStride,
    const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX);
// bytes of dynamic LDS of a launch over members [0, count): the largest member's tile
std::size_t scaleMembersLds(const ScaleMembers &members, int count);
void launchScaleBgrxMembers(const ScaleMembers &members, int count, int dstW, int dstH, hipStream_t stream);
// The output stage's 16-bit path (docs/output_stage.md): the dense f16 state [srcH][srcW][4] (16-byte aligned) -> the dense
// u16 frame [dstH][dstW][4] (8-byte aligned; X = 0), out = (sum qy qx P + 2^23) >> 24 with P = floor((s + 0.5) * 65536)
// saturated, summed exactly (64 bits), clamped to 0 .. 65535 where an axis' filter is cubic.  x / y / spanX as for
// launchScaleBgrx.
void launchScaleState(const void *state, int srcW, int srcH, std::uint16_t *dst, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream);
// The limits of ju_set_output_size as one message shared with its Python twin: "" when outW x outH may be the output
// size of a model whose output is modelW x modelH (each axis 2 .. 16384, at most 16 times the model's and at least a
// 16th of it -- an 8th for a cubic filter; a known filter)
constexpr int kOutputAxisMin = 2, kOutputAxisMax = 16384;
std::string outputSizeProblem(std::size_t outW, std::size_t outH, std::size_t modelW, std::size_t modelH, int filter);
// ---- the alpha channel (alpha_kernels.hip; docs/alpha.md; tests/alpha_reference.py) ------------------------------------
// The modes of ju_set_alpha (JU_ALPHA_*): the slot stays 0, holds the format's top code, or holds the input frame's
// alpha scaled straight from the input frame's size to the output frame's size.
constexpr int kAlphaZero = 0, kAlphaOpaque = 1, kAlphaSource = 2;
// The limits of ju_set_alpha as one message shared with its Python twin, and what ju_set_source_size / ju_set_output_size
// ask before they change a size under JU_ALPHA_SOURCE: "" when `mode` and `filter` are known and -- in that mode -- the
// alpha scaler can go from the input frame inW x inH to the output frame outW x outH (each axis 2 .. 16384, the input at
// most 16 times the output -- 8 with a cubic filter -- and the output at most 16 times the input)
std::string alphaProblem(int mode, int filter, std::size_t inW, std::size_t inH, std::size_t outW, std::size_t outH);
// Where an alpha slot lies in rows of pixels: byte 3 of four-byte pixels (any byte alignment), word 3 of eight-byte pixels
// (2-byte aligned), bits 30-31 of 32-bit words (4-byte aligned); as a source also none -- the plane is 65535 everywhere
// and nothing is read.  ptr: the first logical row; stride: bytes, any sign.
constexpr int kAlphaByte = 0, kAlphaWord = 1, kAlphaBits = 2, kAlphaNone = 3;
struct AlphaRows {
	int kind = kAlphaNone;
	void *ptr = nullptr;
	std::ptrdiff_t stride = 0;
};
// One launch: the 16-bit alpha plane of `src` (257 a, the word, 21845 a, or 65535) scaled srcW x srcH -> dstW x dstH,
// A' = (sum qy qx A + 2^23) >> 24 (clamped to 0 .. 65535 where the filter is cubic), its code ((A' + 128) / 257, A',
// (A' + 10922) / 21845) stored into the slot of every pixel of `dst`; no other bit of the destination changes.  x / y /
// spanX as for launchScaleBgrx.  std::invalid_argument: an unknown kind, a NULL side, a stride shorter than a row, a
// misaligned side, or a tile beyond the LDS.
void launchAlphaScale(const AlphaRows &src, int srcW, int srcH, const AlphaRows &dst, int dstW, int dstH, const ScaleAxisDev &x,
    const ScaleAxisDev &y, int spanX, hipStream_t stream);
// One launch: the top code (255, 65535, 3) into the slot of every pixel of `dst`
void launchAlphaFill(const AlphaRows &dst, int dstW, int dstH, hipStream_t stream);
// Masked pass-through over the frame `gen` (outW x outH BGRX rows, rewritten in place): per pixel the point-sampled
// texel of `src` (srcW x srcH) and of `mask` (maskW x maskH), a = 765 - (Rm + Gm + Bm), out = (src a + gen (765 - a) +
// 382) / 765 per channel, X = 0; pixels with a == 0 are not rewritten.  Any byte alignment, signed strides.
void launchMaskBlend(std::uint8_t *gen, std::ptrdiff_t genStride, int outW, int outH, const std::uint8_t *src,
    std::ptrdiff_t srcStride, int srcW, int srcH, const std::uint8_t *mask, std::ptrdiff_t maskStride, int maskW,
    int maskH, hipStream_t stream);

// ---- tiled upscaling (tile_kernels.hip; docs/tiled.md; the layout: tile_geometry.h) -----------------------------------
// The tiles of one frame, row-major over the tile grid: tile k's dense BGRX image (16-byte aligned) and its origin in
// SOURCE pixels.  The by-value argument of both kernels.
struct TileSet {
	std::uint8_t *ptr[kTileMax] = {};
	int x[kTileMax] = {}, y[kTileMax] = {};
};
static_assert(sizeof(TileSet) <= 1024, "the by-value argument of the tile kernels must not grow");
// BGRX rows of the source (address and signed stride multiples of 4) -> the `count` dense tileW x tileH inputs, X = 0:
// tile k = the source's pixels from (x[k], y[k]) on.  One launch.
void launchTileSplit(const std::uint8_t *src, std::ptrdiff_t srcStride, const TileSet &tiles, int count, int tileW, int tileH,
    hipStream_t stream);
// The split of the frames of a look-ahead pass in ONE launch (tile_split_frames_kernel; docs/tiled.md "Look-ahead passes"):
// for f < frameCount (1 .. kFlowBatchMax) launchTileSplit's bytes of the source frames.src[f] / frames.stride[f] (each frame's
// own address and signed stride, multiples of 4, of any 16-byte phase) into tile k's input at
// tiles.ptr[k] + f * slotBytes (a multiple of 16).  The by-value argument: per-frame pointers and strides.
struct TileFrames {
	const std::uint8_t *src[kFlowBatchMax] = {};
	long long stride[kFlowBatchMax] = {};
};
void launchTileSplitFrames(const TileFrames &frames, int frameCount, const TileSet &tiles, std::size_t slotBytes, int count, int tileW,
    int tileH, hipStream_t stream);
// The split and the scene detector of the tiled stream in ONE launch (tile_split_scene_kernel; docs/tiled.md "Scene cuts"):
// the tile bytes of launchTileSplit, and over the source of srcW x srcH the sum, the decision and the record of
// launchSceneSad (SceneSadLaunch's prev .. resetMode; its src, stride and size are ignored) -- `prev` is the dense
// srcW x srcH kept frame, rewritten with the masked source (X = 0).  Every source pixel is counted by ONE tile, its owner:
// tile k owns [x[k], own.x1[k]) x [y[k], own.y1[k]) (tile_geometry.h tileOwnedEnds), which lies inside the tile.
struct TileOwn {
	int x1[kTileMax] = {}, y1[kTileMax] = {};
};
void launchTileSplitScene(const std::uint8_t *src, std::ptrdiff_t srcStride, int srcW, int srcH, const TileSet &tiles,
    const TileOwn &own, int count, int tileW, int tileH, const struct SceneSadLaunch &scene, hipStream_t stream);
// The nx x ny dense tile outputs (tileOutW pixels per row each) -> BGRX rows of outW x outH (address and signed stride
// multiples of 4; X = 0): out = (sum wy wx v + 32768) >> 16 per byte over the tiles the two tables name -- the device
// copies of TileAxis::table for the x and the y axis, one 32-bit word per output coordinate.  One launch.
void launchTileStitch(std::uint8_t *dst, std::ptrdiff_t dstStride, int outW, int outH, const TileSet &tiles, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, hipStream_t stream);
// The blend of the tiles' f16 STATES (docs/tiled.md "Deep outputs"; tests/tiled_deep_reference.py stitch16): `states` names
// the nx x ny dense states [..][tileOutW][4] f16 (B, G, R, unused; 16-byte aligned) by their ptr fields, origins as above
// -> the dense u16 frame [outH][outW][4] at dst16 (16-byte aligned; outW a multiple of 4; X = 0): per channel
// out16 = (sum wy wx P + 32768) >> 16 with P = floor((s + 0.5) * 65536) saturated, at most 65535 * 65536 + 32768 < 2^32.
// The layout launchScaleState writes and launchEncodeFrame16 reads.  One launch.
void launchTileStitchState(std::uint16_t *dst16, int outW, int outH, const TileSet &states, int nx, int ny, int tileOutW,
    const unsigned *xTable, const unsigned *yTable, hipStream_t stream);
// Blend and scale in ONE launch (docs/tiled.md "An output size"; tests/tiled_output_reference.py): the bytes of
// launchTileStitch into a frame of outW x outH followed by launchScaleBgrx to dstW x dstH -- that frame is formed in
// registers inside the scaler's vertical pass and never stored.  dst: BGRX rows at any byte alignment, signed stride, X = 0.
// x / y / spanX: the device copies of buildScaleAxis(outW, dstW) / (outH, dstH) and scaleSpan of the x axis; outW and
// tileOutW multiples of four pixels; the x table 16-byte aligned.  The scaler's tile and 1 KB of tile pointers and
// origins must fit the LDS (std::invalid_argument).
void launchTileStitchScale(std::uint8_t *dst, std::ptrdiff_t dstStride, int dstW, int dstH, int outW, int outH, const TileSet &tiles,
    int nx, int ny, int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y,
    int spanX, hipStream_t stream);
// The same over the tiles' f16 states: the words of launchTileStitchState followed by a 16-bit scale of that frame (the
// arithmetic of launchScaleState on its words P) -> the dense u16 frame [dstH][dstW][4] at dst16 (8-byte aligned; X = 0).
void launchTileStitchScaleState(std::uint16_t *dst16, int dstW, int dstH, int outW, int outH, const TileSet &states, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y, int spanX,
    hipStream_t stream);
// A tiled object's source mask (docs/tiled.md "A mask"; tests/tiled_mask_reference.py): launchMaskBlend's arithmetic on
// the BLENDED sample while it is in registers.  src: BGRX rows of the source, outW / 4 x outH / 4, whose texel under
// blended pixel (X, Y) is (X >> 2, Y >> 2); mask: BGRX rows of maskW x maskH, point sampled at floor((2 X + 1) maskW /
// (2 outW)) -- addresses and signed strides multiples of 4, 2 x blended extent x mask extent below 2^32 on both axes.
// [x0, x1) x [y0, y1): the box (mask_box.h), inside the blended frame; outside it the kernels read neither and take the
// unmasked kernels' path.
struct TileMask {
	const std::uint8_t *src = nullptr, *mask = nullptr;
	std::ptrdiff_t srcStride = 0, maskStride = 0;
	int maskW = 0, maskH = 0;
	int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
};
// launchTileStitch with the mask: masked = blend(stitch(tiles), src, mask), X = 0.  outW and outH multiples of four.
void launchTileStitchMask(std::uint8_t *dst, std::ptrdiff_t dstStride, int outW, int outH, const TileSet &tiles, int nx, int ny,
    int tileOutW, const unsigned *xTable, const unsigned *yTable, const TileMask &mask, hipStream_t stream);
// launchTileStitchScale with the mask applied to each blended pixel, at the blended size, BEFORE the scaler multiplies it.
void launchTileStitchMaskScale(std::uint8_t *dst, std::ptrdiff_t dstStride, int dstW, int dstH, int outW, int outH, const TileSet &tiles,
    int nx, int ny, int tileOutW, const unsigned *xTable, const unsigned *yTable, const ScaleAxisDev &x, const ScaleAxisDev &y,
    int spanX, const TileMask &mask, hipStream_t stream);

// *word += 1 (system scope) once everything enqueued before it on `stream` has completed: `word` is the device address of
// host-mapped memory (PinnedWords) that the host polls.  Host frames inside look-ahead passes (Engine::processBatch).
void launchSignalHost(unsigned *word, hipStream_t stream);

// ---- scene-cut detection (scene_kernels.hip; docs/scene_detect.md) ----------------------------------------------------
// SceneState: the detector's device memory, zero at a start.  acc / ticket: the sum being built and the workgroups
// that have added to it -- both back at zero when a launch ends.  resetNow: what scene_clear_kernel obeys.
struct SceneState {
	unsigned long long acc;
	unsigned ticket, resetNow;
	unsigned long long prevSad, frames, cuts;
};
// One decision, in host-mapped memory: a ring of kSceneRing records, and behind them ONE more whose step / sad hold the
// cumulative frames / cuts of the runtime (kSceneRing + 1 records in all).
struct SceneRecord {
	unsigned long long step, sad, score;
	unsigned cut, reserved;
};
constexpr int kSceneRing = 64;
constexpr int kSceneAxisMax = 1 << 15;
struct SceneSadLaunch {
	const std::uint8_t *src = nullptr;  // BGRX rows, 4-byte aligned, any signed stride of at least a row
	std::ptrdiff_t srcStride = 0;
	int width = 0, height = 0;
	std::uint32_t *prev = nullptr;  // dense width x height BGRX: read as c_{t-1}, rewritten as c_t
	SceneState *state = nullptr;
	SceneRecord *ring = nullptr;  // device address of the host-mapped records
	int slot = 0;
	std::uint64_t step = 0;
	int hasPrev = 0;  // bit 0: frame t-1 is in the detector's memory, bit 1: frame t-2 is
	unsigned thresholdMilli = 0;
	bool resetMode = false;  // a cut raises SceneState::resetNow
};
void launchSceneSad(const SceneSadLaunch &q, hipStream_t stream);
// The detector over the `items` frames of a look-ahead pass in ONE launch (scene_pass_kernel): item i against item i - 1,
// item 0 against the kept frame, the last item becomes the kept frame; the workgroup that draws the last ticket takes all
// the decisions in order -- SceneState::prevSad / frames / cuts carried from item to item and from before the pass, one
// ring record per item -- and leaves what the rest of the pass reads:
//   resetAt[i] = cut_i && resetMode       (the flag of frame i's scene_clear_kernel)
//   cutAt[i]   = the latest item <= i with resetAt set, else -1   (the first flow block's cut-aware history)
// ScenePassState: device memory, zero at creation; acc / ticket are back at zero when a launch ends.
struct ScenePassState {
	unsigned long long acc[kFlowBatchMax];
	unsigned ticket, reserved;
	unsigned resetAt[kFlowBatchMax];
	int cutAt[kFlowBatchMax];
};
// What changes between two replays of a captured pass, so no kernel argument: host-mapped memory the host writes in front
// of the launch (a pass is synchronous: nothing reads it while the host writes).
struct ScenePassDyn {
	unsigned long long stepBase;  // the record's `step` of item 0
	unsigned seen;                // frames in the detector's memory in front of item 0: 0, 1, or 2 for two and more
	unsigned thresholdMilli;
	unsigned slot;                // ring slot of item 0; item i takes (slot + i) % kSceneRing
	unsigned reserved;
};
struct ScenePassLaunch {
	int items = 0;  // 1 .. kFlowBatchMax
	const std::uint8_t *frames[kFlowBatchMax] = {};  // each: BGRX rows, 4-byte aligned, any signed stride of at least a row
	std::ptrdiff_t strides[kFlowBatchMax] = {};
	int width = 0, height = 0;
	std::uint32_t *prev = nullptr;  // the kept frame: read as item 0's predecessor, rewritten as the last item
	SceneState *state = nullptr;
	ScenePassState *pass = nullptr;
	const ScenePassDyn *dyn = nullptr;  // device address of the host-mapped block
	SceneRecord *ring = nullptr;
	bool resetMode = false;
};
void launchScenePass(const ScenePassLaunch &q, hipStream_t stream);
// The detector over the independent items of a group pass in ONE launch (scene_group_kernel; Engine::processGroup): item
// i is member i's frame against member i's OWN kept frame, state and ring -- the arithmetic and the decision of
// launchSceneSad per item, taken by the workgroup that draws the grid's last ticket (the first present item's
// SceneState::ticket; every acc and that ticket are back at zero when the launch ends).
// SceneGroupDyn: what varies between ticks, in the member's host-mapped memory, written by the host in front of the launch
// (a group pass is synchronous: nothing reads it while the host writes) and read by the kernel as three 64-bit words.
struct SceneGroupDyn {
	unsigned long long step;           // the record's `step`
	unsigned long long slotHasPrev;    // low word: the ring slot; high word: bit 0 frame t-1 is in the detector's memory, bit 1 frame t-2 is
	unsigned long long thresholdMode;  // low word: threshold_milli; high word: 2 = a cut raises SceneState::resetNow, else it reports
};
struct SceneGroupItem {
	const std::uint8_t *frame = nullptr;  // BGRX rows, 4-byte aligned, any signed stride of at least a row; nullptr: absent, skipped
	std::ptrdiff_t stride = 0;
	std::uint32_t *prev = nullptr;  // dense width x height BGRX: read as c_{t-1}, rewritten as c_t
	SceneState *state = nullptr;
	SceneRecord *ring = nullptr;       // device address of the member's host-mapped records
	const SceneGroupDyn *dyn = nullptr;  // device address of the member's host-mapped words
};
struct SceneGroupLaunch {
	int items = 0;  // 1 .. kFlowBatchMax, absent ones included; no launch when all are absent
	SceneGroupItem item[kFlowBatchMax];
	int width = 0, height = 0;  // of every item: the members of a pass share the model
};
void launchSceneGroup(const SceneGroupLaunch &q, hipStream_t stream);
// The conditional clear of all members of a group pass in ONE launch (scene_clear_items_kernel): for item i, if (*flag)
// a[0 .. aBytes) = b[0 .. bBytes) = 0, any alignment; an item with a null flag is absent.
struct SceneClearItem {
	const unsigned *flag = nullptr;
	void *a = nullptr;
	std::size_t aBytes = 0;
	void *b = nullptr;
	std::size_t bBytes = 0;
};
void launchSceneClearItems(const SceneClearItem *items, int n, hipStream_t stream);
// The conditional clear of all tiles of a tiled frame in ONE launch under ONE flag (scene_clear_tiles_kernel; docs/tiled.md
// "Scene cuts"): if (*flag) items[i].a[0 .. aBytes) = items[i].b[0 .. bBytes) = 0 for every i < n (1 .. kTileMax; any
// alignment; items[i].flag is not read).  Pointers and sizes of 64 tiles x 2 buffers do not fit kernel arguments: they go
// into a table of kTileMax SceneClearTile in host-mapped memory (tableHost / tableDev: its two addresses), rewritten here
// in front of the launch -- no earlier launch that reads the table may still be pending -- and read by a workgroup only
// behind a raised flag.
struct SceneClearTile {
	std::uint8_t *a, *b;
	long long aBytes, bBytes;
	int aChunks, bChunks;
};
void launchSceneClearTiles(const unsigned *flag, const SceneClearItem *items, int n, volatile SceneClearTile *tableHost,
    const SceneClearTile *tableDev, hipStream_t stream);
// The refusals of ju_set_scene_detect as one message ("" when mode and threshold are fine): mode 0 .. 2, and while the
// mode is not off a threshold of 1 .. 255000 thousandths of a code value
std::string sceneDetectProblem(int mode, std::uint32_t thresholdMilli);
// if (*flag) a[0 .. aBytes) = b[0 .. bBytes) = 0: any alignment; `flag` is read by every workgroup once
void launchSceneClear(const unsigned *flag, void *a, std::size_t aBytes, void *b, std::size_t bBytes, hipStream_t stream);

// max |x| over n 16-bit elements, atomically folded into *out as the bit pattern of a
// non-negative float (the caller zeroes it per frame).  Calibration mode only.
void launchAbsMax(DType dt, const void *in, std::size_t n, unsigned *out, hipStream_t stream);

// 16-bit tensor -> f32 (debug read-back).
void launchToFloat(DType dt, const void *in, float *out, std::size_t n, hipStream_t stream);

}  // namespace ju
