// The program builder: which launches a frame runs.  buildProgram(set) writes m_Program[set] stage by stage -- input,
// flow net, warp, generator head, tower, tail, temporal filter -- and addFlowAutoencoder writes the flow auto-encoder's
// launches for the per-frame program and for the look-ahead and group passes (engine_passes.cpp).  Everything is read
// when the program is BUILT but `io` and `sb` of ProgramBuild, `*flowSlot` of the warp and towerVariant(): those are read
// when a step runs (or is captured).
#include "engine.h"

#include <algorithm>
#include <cstdlib>
#include <stdexcept>

namespace ju {

namespace {
int padTo16(int c) { return (c + 15) / 16 * 16; }
}  // namespace

// What the stages of buildProgram share; a step's launch keeps a copy.  Through `io` and `sb` a launch reads what is
// known only when it RUNS (or is captured): the frames of the call (m_IO: the staging buffers or the caller's) and the
// recurrent state of its binding set.  Everything else is as of the build.
struct Engine::ProgramBuild {
	std::vector<Step> *prog;
	int set;
	DType dt;
	int H, W, PH, PW, padTop, padLeft;  // the frame, the padded flow input and its border (models.py:783-787)
	const FrameIO *io;
	const StateBind *sb;
	// normalize_brightness: three integer channel sums per frame, consumed by the pack,
	// warp and tail kernels (models.py:772-779, 802-803, 809-810) -- in a flow-free model the flag touches
	// nothing: it shifts only the flow input, pre_warp and the fed-back state, none of which exists
	const unsigned *sums;
	// The u8 frame the generator's writers produce (the fused tail of the resident tower, the tails, the temporal
	// filter): the caller's frame -- or, in the output_flow variant (outputSelect pre_warp), a scratch frame
	// nobody reads: there the warp step writes the caller's frame, and everything the generator does for the state
	// stays exactly the plain model's.  The tower kernels are not edited for it; the price is their 4H x 4W x 4
	// store into the scratch.  Read at launch (capture) time, like io.
	std::uint8_t *discard;
	std::uint8_t *genOutU8() const { return discard ? discard : io->out; }
	std::ptrdiff_t genOutStride() const { return discard ? static_cast<std::ptrdiff_t>(W) * 16 : io->outStride; }
	// the five fields of a fused tail that are known at launch time only, for the tail as a launch of its own
	// (TailFusedLaunch) and inside the resident tower's (ResidentTowerParams)
	template <class Launch>
	void bindTail(Launch *l) const {
		l->state = sb->out;
		l->frame = io->in;
		l->frameStride = io->inStride;
		l->outU8 = genOutU8();
		l->outStride = genOutStride();
	}
	const char *trunk = "trunk_a";  // where the tower leaves its output
	bool tailInTower = false;       // the resident tower wrote the HR state and the frame
};

// The walk of addFlowAutoencoder over the units: the tensor the next launch reads, its item stride and resolution.
struct Engine::FlowBuild {
	Engine *e;
	std::vector<Step> *prog;
	int set, items;
	bool group, cut, batch;  // batch: a pass's launches, on the batch tensors
	Operand cur;
	long curItem;
	int h, w;
	bool upsampleNext = false;  // `cur` is half resolution: the next conv upsamples it
	void *tensor(const std::string &n) const { return (batch ? e->m_BatchTensors : e->m_Tensors).at(n).buf.get(); }
	// bytes of ONE frame's tensor: the item stride of a look-ahead launch
	long itemBytes(const std::string &n) const {
		const Tensor &t = e->m_Tensors.at(n);
		return static_cast<long>(t.count) * (t.isF32 ? 4 : 2);
	}
	// (the flow net's tensors are dense: a zero pitch in either set of tensors)
	void read(const std::string &n) {
		cur = Operand{tensor(n), 0};
		curItem = itemBytes(n);
	}
};

// Which units of the flow auto-encoder (models.py:334-481) run as one launch each.
void Engine::planFlowUnits() {
	m_FlowUnits.clear();
	const ModelConfig &c = m_Config;
	if (c.flowArch != 0) return;
	const int nb = static_cast<int>(c.flowFilters.size()) / 2;
	const bool hasHeadConv = c.flowFilters.size() % 2 != 0;
	m_FlowUnits.resize(2 * nb + 1);
	if (!m_FlowFused) return;
	int cin = 3 * c.numFlowInputs;
	int h = c.paddedHeight(), w = c.paddedWidth();
	bool prevUps = false;  // the previous unit ends with a bilinear x2
	for (int i = 0; i < 2 * nb; ++i) {
		const int f = c.flowFilters[i];
		const bool pool = i < nb;
		if (prevUps) {
			h *= 2;
			w *= 2;
		}
		FlowUnit &u = m_FlowUnits[i];
		const bool even = h % 2 == 0 && w % 2 == 0;
		if ((!pool || (m_FusedPool && even)) && (!prevUps || even)) {
			if (prevUps && m_FusedUpsample && flowBlockSupported(padTo16(cin), f, true, pool, false, h, w)) {
				u.fused = u.upsIn = true;
			} else if (flowBlockSupported(padTo16(cin), f, false, pool, false, h, w)) {
				u.fused = true;
			}
		}
		if (pool) {
			h /= 2;
			w /= 2;
		}
		prevUps = !pool;
		cin = f;
	}
	if (hasHeadConv) {  // flow/conv_1 (BN, act) + flow/conv_2 (bias, 32 channels, f16 flow head)
		if (prevUps) {
			h *= 2;
			w *= 2;
		}
		const int f = c.flowFilters.back();
		FlowUnit &u = m_FlowUnits[2 * nb];
		const bool even = h % 2 == 0 && w % 2 == 0;
		if (f == 32) {
			if (prevUps && even && m_FusedUpsample && flowBlockSupported(padTo16(cin), f, true, false, true)) {
				u.fused = u.upsIn = true;
			} else if (flowBlockSupported(padTo16(cin), f, false, false, true)) {
				u.fused = true;
			}
		}
	}
}

bool Engine::flowConvIsFused(const std::string &name) const {
	if (m_Config.flowArch != 0 || m_FlowUnits.empty()) return false;
	const int nb = static_cast<int>(m_Config.flowFilters.size()) / 2;
	if (name == "flow/conv_1" || name == "flow/conv_2") return m_FlowUnits[2 * nb].fused;
	if (name.rfind("flow/block_", 0) == 0) {
		const int k = std::atoi(name.c_str() + 11);
		return k >= 1 && k <= 2 * nb && m_FlowUnits[k - 1].fused;
	}
	return false;
}

// the flow net's first block builds the packed tensor itself when it runs as one launch
bool Engine::flowPacksInBlock() const {
	const ModelConfig &c = m_Config;
	return m_PackInBlock && c.flowArch == 0 && !m_FlowUnits.empty() && m_FlowUnits[0].fused &&
	       3 * c.numFlowInputs <= 16 && !c.flowFilters.empty() && c.flowFilters[0] == 32;
}

void Engine::addConvStep(std::vector<Step> *prog, const std::string &tag, const std::string &wname, Operand in,
    Operand res, Operand out, int H, int W, const ConvOpt &opt) {
	auto it = m_Convs.find(wname);
	if (it == m_Convs.end()) throw std::logic_error("missing conv weights " + wname);
	const ConvWeights &cw = it->second;
	ConvParams p{};
	p.in = in.ptr;
	p.wgt = cw.w.get();
	p.bias = cw.bias.as<float>();
	p.res = res.ptr;
	p.out = out.ptr;
	p.inPitch = in.pitch;
	p.resPitch = res.pitch;
	p.outPitch = out.pitch;
	p.H = H;
	p.W = W;
	p.cin = cw.cinP;
	p.cout = cw.cout;
	p.taps = cw.taps;
	{  // the layer's activation (models.py:24-27): the flow net and the generator each have their own
		const bool flowLayer = wname.rfind("flow/", 0) == 0;
		const int act = flowLayer ? m_Config.flowActivation : m_Config.genActivation;
		p.relu = opt.relu ? (act == 1 ? 2 : 1) : 0;
		p.slope = flowLayer ? m_Config.flowNegativeSlope : m_Config.genNegativeSlope;
	}
	p.outHead = opt.outHead ? 1 : 0;
	p.nb = cw.nb;
	p.rw = cw.rw;
	if (opt.pool) {  // the pooled epilogue pairs the two rows of a wave
		p.pool = 1;
		p.rw = 2;
	}
	p.plan = &m_Plan;
	p.upsample = opt.upsample ? 1 : 0;
	if (opt.upsample) {
		// + the low-resolution patch: with rw = 2 the workgroup needs 96 KB of LDS and
		// only one fits a CU (measured 21 us against 16 us); 4-row tiles (74 KB) keep two
		p.rw = 1;
	}
	const DType dt = m_DType;
	Step s;
	s.tag = tag;
	s.flops = 2.0 * H * W * cw.taps * cw.cinReal * cw.cout * std::max(opt.item.items, 1);
	if (opt.item.items > 1) {  // a look-ahead launch: the layer of `items` frames (split-K convolutions only)
		p.items = opt.item.items;
		p.inItemBytes = opt.item.in;
		p.outItemBytes = opt.item.out;
		// (split-K and generic convolutions have an item dimension; the tower kernel and residual inputs do not)
		if (opt.tower || p.res != nullptr) throw std::logic_error("look-ahead: no batched form of " + wname);
	}
	if (opt.tower) {
		s.run = [dt, p](hipStream_t st) { launchConvTower(dt, p, st); };
	} else if (cw.splitK && convSplitKSupported(p)) {
		if (!m_Zeros.get()) m_Zeros = DeviceBuffer(256);  // (DeviceBuffer memory starts zeroed)
		const void *zeros = m_Zeros.get();
		s.run = [dt, p, zeros](hipStream_t st) { launchConvSplitK(dt, p, zeros, st); };
	} else {
		s.run = [dt, p](hipStream_t st) { launchConv(dt, p, st); };
	}
	prog->push_back(std::move(s));
}

// ---- the flow auto-encoder ----

// one launch for a whole block (both convs, pool, preceding upsample) where planned: reads f.cur at f.h x f.w
void Engine::addFlowBlockStep(FlowBuild &f, const std::string &convA, const std::string &convB,
    const std::string &outName, bool pool, bool outHead, int act2) {
	const ConvWeights &wa = m_Convs.at(convA), &wb = m_Convs.at(convB);
	const DType dt = m_DType;
	FlowBlockLaunch fb{};
	fb.in = f.cur.ptr;
	fb.w1 = wa.w.get();
	fb.b1 = wa.bias.as<float>();
	fb.w2 = wb.w.get();
	fb.b2 = wb.bias.as<float>();
	fb.out = f.tensor(outName);
	fb.H = f.h;
	fb.W = f.w;
	fb.cin = wa.cinP;
	fb.cmid = wa.cout;
	fb.upsample = f.upsampleNext;
	fb.pool = pool;
	fb.outHead = outHead;
	fb.act1 = m_Config.flowActivation == 1 ? 2 : 1;
	fb.act2 = act2;
	fb.slope = m_Config.flowNegativeSlope;
	fb.plan = &m_Plan;
	fb.items = f.items;
	fb.inItemBytes = f.curItem;
	fb.outItemBytes = f.itemBytes(outName);
	const double flops =
	    f.items * 2.0 * f.h * f.w * 9.0 * (double(wa.cinReal) * wa.cout + double(wb.cinReal) * wb.cout);
	f.upsampleNext = false;
	if (flowPacksInBlock() && convA == "flow/block_1/conv_1") return addPackingFlowBlockStep(f, fb, flops);
	f.prog->push_back({"flow", flops, [dt, fb](hipStream_t s) { launchFlowBlock(dt, fb, s); }});
}

// The first block where it builds the packed input itself: the frame history of binding set f.set, or in a pass the
// frames of m_Pass (submitBatch).
void Engine::addPackingFlowBlockStep(FlowBuild &f, FlowBlockLaunch fb, double flops) {
	const ModelConfig &c = m_Config;
	const DType dt = m_DType;
	fb.packPrev = m_Packed[f.set].get();
	fb.packOut = m_Packed[f.set ^ 1].get();
	fb.frameH = c.frameHeight;
	fb.frameW = c.frameWidth;
	fb.padTop = (c.paddedHeight() - c.frameHeight) / 2;  // models.py:783-787
	fb.padLeft = (c.paddedWidth() - c.frameWidth) / 2;
	fb.numInputs = c.numFlowInputs;
	fb.sums = c.normalizeBrightness ? m_TailB2.as<unsigned>() + 4 : nullptr;
	if (f.group) {  // every item the next frame of its own stream: its history from / to that stream's buffers
		fb.packPrev = nullptr;
		fb.packOut = nullptr;
		fb.independentItems = true;
	}
	if (f.cut) fb.cutAt = m_ScenePassDev.as<ScenePassState>()->cutAt;
	const FrameIO *io = &m_IO;
	const PassFrame *pass = m_Pass;
	const int items = f.items;
	const bool group = f.group;
	f.prog->push_back({"flow", flops, [dt, fb, io, pass, items, group](hipStream_t s) {
		                   FlowBlockLaunch l = fb;  // the caller's frames are known at launch time only
		                   l.packFrame = io->in;
		                   l.packFrameStride = io->inStride;
		                   for (int i = 0; i < items && (items > 1 || group); ++i) {
			                   l.packFrames[i] = pass[i].io.in;
			                   l.packFrameStrides[i] = pass[i].io.inStride;
			                   if (group) {
				                   l.packPrevs[i] = pass[i].groupPrev;
				                   l.packOuts[i] = pass[i].groupOut;
			                   }
		                   }
		                   launchFlowBlock(dt, l, s);
	                   }});
}

// What follows decoder block i + 1, whose output a_2 has half the resolution of what reads it: the next unit expands
// it while staging (a one-launch unit planned so), the convolution that follows folds the bilinear x2 into its own
// staging, or upsample2 runs as a launch.
void Engine::addDecoderUpsample(FlowBuild &f, int i) {
	const ModelConfig &c = m_Config;
	const DType dt = m_DType;
	const int nb = static_cast<int>(c.flowFilters.size()) / 2;
	const int filters = c.flowFilters[i];
	const std::string n = "flow/block_" + std::to_string(i + 1);
	const std::string next = i + 1 < 2 * nb ? "flow/block_" + std::to_string(i + 2) + "/conv_1"
	                         : (c.flowFilters.size() % 2 ? "flow/conv_1" : "");  // not the head
	// a convolution folds the expansion in when it stages its input once (cout = 32: every cout-group workgroup
	// would repeat the expansion; measured: a loss already with two groups) and reads 64-channel chunks
	const auto conv = m_Convs.find(next);
	const bool convFolds = m_FusedUpsample && conv != m_Convs.end() && filters % 64 == 0 && conv->second.nb == 1 &&
	                       conv->second.cout <= 32;
	const FlowUnit &unit = m_FlowUnits[i + 1];  // (the head's unit is there whether the model has a head conv or not)
	if (unit.fused ? unit.upsIn : convFolds) {
		f.upsampleNext = true;
		f.read(n + "/a_2");
	} else {
		const void *src = f.tensor(n + "/a_2");
		void *dst = f.tensor(n + "/resample");
		const int h = f.h, w = f.w, items = f.items;
		f.prog->push_back({"flow", 0.0,
		    [=](hipStream_t s) { launchUpsample2(dt, src, dst, h, w, filters, s, items); }});
		f.read(n + "/resample");
	}
	f.h *= 2;
	f.w *= 2;
}

// The flow auto-encoder (models.py:334-481) as launches: `items` = 1 for the per-frame program of binding set `set`,
// > 1 for a look-ahead pass -- the same launches over `items` consecutive frames (grid.z), on the batch tensors, the
// first block reading the frames of m_Pass (submitBatch).  A look-ahead pass exists only where every launch of
// the plan has an item dimension (the one-launch blocks and the split-K convolutions): std::logic_error otherwise.
void Engine::addFlowAutoencoder(std::vector<Step> *prog, int set, int items, bool group, bool cut) {
	const ModelConfig &c = m_Config;
	const DType dt = m_DType;
	FlowBuild f{this, prog, set, items, group, cut, items > 1 || group, Operand{m_Packed[set ^ 1].get(), 0}, 0, c.paddedHeight(), c.paddedWidth()};
	auto noBatch = [&](const char *what) {
		if (f.batch) throw std::logic_error(std::string("look-ahead: no batched form of ") + what);
	};
	if (f.batch && (!flowPacksInBlock() || c.normalizeBrightness)) noBatch("the input packing");
	// a convolution launched on its own: reads f.cur, expanding it where it is half resolution, and leaves `out` to read
	auto convStep = [&](const std::string &name, const std::string &out, ConvOpt opt) {
		opt.upsample = f.upsampleNext;
		opt.item = ItemStride{items, f.curItem, f.itemBytes(out)};
		addConvStep(prog, "flow", name, f.cur, Operand{}, Operand{f.tensor(out), 0}, f.h, f.w, opt);
		f.upsampleNext = false;
		f.read(out);
	};
	const int nb = static_cast<int>(c.flowFilters.size()) / 2;
	const int flowAct = c.flowActivation == 1 ? 2 : 1;
	ConvOpt relu, head;
	relu.relu = head.outHead = true;
	for (int i = 0; i < 2 * nb; ++i) {
		const std::string n = "flow/block_" + std::to_string(i + 1);
		const bool pool = i < nb;
		if (m_FlowUnits[i].fused) {
			if (f.upsampleNext != m_FlowUnits[i].upsIn) throw std::logic_error("flow plan out of step");
			addFlowBlockStep(f, n + "/conv_1", n + "/conv_2", pool ? n + "/resample" : n + "/a_2", pool, false, flowAct);
		} else {
			convStep(n + "/conv_1", n + "/a_1", relu);
			ConvOpt second = relu;
			second.pool = pool && m_FusedPool;
			convStep(n + "/conv_2", second.pool ? n + "/resample" : n + "/a_2", second);
			if (pool && !m_FusedPool) {
				noBatch("the pooling launch");
				const void *src = f.tensor(n + "/a_2");  // dense tensors
				void *dst = f.tensor(n + "/resample");
				const int h = f.h, w = f.w, filters = c.flowFilters[i];
				prog->push_back({"flow", 0.0, [=](hipStream_t s) { launchMaxPool2(dt, src, dst, h, w, filters, s); }});
			}
		}
		if (pool) {
			f.h /= 2;
			f.w /= 2;
			f.read(n + "/resample");
		} else {
			addDecoderUpsample(f, i);
		}
	}
	if (c.flowFilters.size() % 2) {
		if (m_FlowUnits[2 * nb].fused) {  // flow/conv_1 + flow/conv_2 -> the f16 flow head, one launch
			if (f.upsampleNext != m_FlowUnits[2 * nb].upsIn) throw std::logic_error("flow plan out of step");
			return addFlowBlockStep(f, "flow/conv_1", "flow/conv_2", "flow", false, true, 0);
		}
		convStep("flow/conv_1", "flow/a_1", relu);
	}
	if (f.upsampleNext) throw std::logic_error("flow head cannot take a half-resolution input");
	convStep("flow/conv_2", "flow", head);
}

// ---- the per-frame program ----

void Engine::buildProgram(int set) {
	const ModelConfig &c = m_Config;
	m_Program[set].clear();
	// the recurrent state this program reads / writes: m_State[set] -> m_State[set ^ 1], read at launch (capture)
	// time -- a look-ahead pass binds its frames' programs to its own chain of state buffers (submitBatch)
	// (a flow-free model: one scratch state that nothing reads -- the tail still writes its HR output there)
	m_StateBind[set].in = m_State[c.recurrent() ? set : 0].get();
	m_StateBind[set].out = m_State[c.recurrent() ? set ^ 1 : 0].get();
	const int H = c.frameHeight, W = c.frameWidth, PH = c.paddedHeight(), PW = c.paddedWidth();
	ProgramBuild b{&m_Program[set], set, m_DType, H, W, PH, PW, (PH - H) / 2, (PW - W) / 2, &m_IO, &m_StateBind[set],
	    c.normalizeBrightness && c.recurrent() ? m_TailB2.as<unsigned>() + 4 : nullptr,
	    c.outputsPreWarp() ? m_DiscardFrame.as<std::uint8_t>() : nullptr};
	addInputSteps(b);
	addFlowNetSteps(b);
	addWarpStep(b);
	addGeneratorHeadSteps(b);
	addTowerSteps(b);
	addTailSteps(b);
	addTemporalStep(b);
	m_TrunkOut = b.trunk;
}

void Engine::addInputSteps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (!c.recurrent()) {
		// ---- flow-free model (remove_flow.py): no flow net, no warp, no frame history -- ONE staging
		// launch writes the LR frame into the generator input, then the generator as below ----
		const Operand genIn = operand("gen_in");
		b.prog->push_back({"lr_pack", 0.0,
		    [b, genIn](hipStream_t s) { launchLrPack(b.dt, b.io->in, b.io->inStride, genIn.ptr, genIn.pitch, b.H, b.W, s); }});
	}
	if (b.sums) {
		unsigned *sumsOut = m_TailB2.as<unsigned>() + 4;
		b.prog->push_back({"pack", 0.0, [b, sumsOut](hipStream_t s) { launchFrameSums(b.io->in, b.io->inStride, b.H, b.W, sumsOut, s); }});
	}
	// (the flow net's first block builds the packed tensor itself when it runs as one launch)
	if (!flowPacksInBlock() && c.recurrent()) {
		const void *packedIn = m_Packed[b.set].get();
		void *packedOut = m_Packed[b.set ^ 1].get();
		const int nIn = c.numFlowInputs;
		b.prog->push_back({"pack", 0.0, [b, packedIn, packedOut, nIn](hipStream_t s) {
			                   launchPackFrames(b.dt, b.io->in, b.io->inStride, packedIn, packedOut, b.H, b.W, b.PH, b.PW, b.padTop,
			                       b.padLeft, nIn, b.sums, s);
		                   }});
	}
}

// one launch for a 64-filter residual block outside the resident tower
void Engine::addResBlockStep(std::vector<Step> *prog, const std::string &tag, const std::string &block, Operand in,
    Operand out, int bh, int bw, int activation, float slope) {
	const ConvWeights &wa = m_Convs.at(block + "/conv_1"), &wb = m_Convs.at(block + "/conv_2");
	const DType dt = m_DType;
	FlowBlockLaunch fb{};
	fb.in = in.ptr;
	fb.inPitch = in.pitch;
	fb.w1 = wa.wBlock.get();
	fb.b1 = wa.bias.as<float>();
	fb.w2 = wb.wBlock.get();
	fb.b2 = wb.bias.as<float>();
	fb.out = out.ptr;
	fb.outPitch = out.pitch;
	fb.H = bh;
	fb.W = bw;
	fb.cin = fb.cmid = 64;
	fb.residual = true;
	fb.plan = &m_Plan;
	fb.act1 = fb.act2 = activation == 1 ? 2 : 1;
	fb.slope = slope;
	prog->push_back({tag, 2.0 * bh * bw * 9.0 * 64 * 64 * 2, [dt, fb](hipStream_t s) { launchFlowBlock(dt, fb, s); }});
}

// What the generator's resident tower and the flow-resnet's fill alike (in, out and a tail are the caller's).
ResidentTowerParams Engine::residentTowerParams(const ResidentTower &t, int H, int W, int nLayers, int activation,
    float slope) {
	ResidentTowerParams rp{};
	rp.hasHead = 1;
	rp.weights = t.w.get();
	rp.bias = t.b.as<float>();
	rp.mailbox = t.mail.get();
	rp.counters = t.flags.as<unsigned>();
	rp.error = m_ResErrorDev;
	rp.debug = m_Tensors.at("tower_profile").buf.get();
	rp.H = H;
	rp.W = W;
	rp.GX = t.GX;
	rp.GY = t.GY;
	rp.RH = t.RH;
	rp.nLayers = nLayers;
	rp.leaky = activation == 1 ? 1 : 0;
	rp.slope = slope;
	return rp;
}

void Engine::addFlowNetSteps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (!c.recurrent()) return;  // (no flow net)
	if (c.flowArch == 0) return addFlowAutoencoder(b.prog, b.set, 1);  // (with its head)
	const Operand body = m_ResidentFlow ? addResidentFlowResnet(b) : addLayeredFlowResnet(b);
	ConvOpt head;
	head.outHead = true;
	addConvStep(b.prog, "flow", "flow/conv_2", body, Operand{}, operand("flow"), b.PH, b.PW, head);
}

// flow-resnet body = conv_1 + residual blocks, 64 filters: ONE launch of the
// resident tower kernel (own mailbox and publish counters)
Engine::Operand Engine::addResidentFlowResnet(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	const void *packedOut = m_Packed[b.set ^ 1].get();
	void *in64 = m_Tensors.at("flow/in64").buf.get();
	b.prog->push_back({"flow", 0.0, [b, packedOut, in64](hipStream_t s) { launchExpandChannels(b.dt, packedOut, in64, b.PH * b.PW, s); }});
	ResidentTowerParams rp =
	    residentTowerParams(m_FlowTower, b.PH, b.PW, 1 + 2 * c.flowResBlocks, c.flowActivation, c.flowNegativeSlope);
	rp.in = in64;
	rp.inPitch = b.PW;
	rp.out = operand("flow/trunk").ptr;
	b.prog->push_back({"flow", 2.0 * b.PH * b.PW * 9.0 * (3.0 * c.numFlowInputs * 64 + 64.0 * 64 * 2 * c.flowResBlocks),
	    [b, rp](hipStream_t s) { launchResidentTower(b.dt, rp, s); }});
	return operand("flow/trunk");
}

// the same body layer by layer: one launch per residual block (64 filters) or per convolution
Engine::Operand Engine::addLayeredFlowResnet(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	const Operand none{};
	ConvOpt relu;
	relu.relu = true;
	addConvStep(b.prog, "flow", "flow/conv_1", Operand{m_Packed[b.set ^ 1].get(), 0}, none, operand("flow/x0"), b.PH, b.PW, relu);
	const char *xs[2] = {"flow/x0", "flow/x1"};
	int a = 0;
	for (int i = 0; i < c.flowResBlocks; ++i, a ^= 1) {
		const std::string n = "flow/block_" + std::to_string(i + 1);
		if (m_BlockFused && c.flowResFilters == 64) {
			addResBlockStep(b.prog, "flow", n, operand(xs[a]), operand(xs[a ^ 1]), b.PH, b.PW, c.flowActivation, c.flowNegativeSlope);
			continue;
		}
		addConvStep(b.prog, "flow", n + "/conv_1", operand(xs[a]), none, operand("flow/t"), b.PH, b.PW, relu);
		addConvStep(b.prog, "flow", n + "/conv_2", operand("flow/t"), operand(xs[a]), operand(xs[a ^ 1]), b.PH, b.PW, relu);
	}
	return operand(xs[a]);
}

// ---- warp + space-to-depth + concat ----
void Engine::addWarpStep(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (!c.recurrent()) return;
	m_FlowCur = m_Tensors.at("flow").buf.get();
	const void *const *flowSlot = &m_FlowCur;  // (a look-ahead pass points it at its frame's field)
	// the generator input lives in the tower layout (zero border = conv_1's padding), so that conv_1 can run
	// on the tower's per-layer kernel wherever it is a launch of its own (8-bit towers, per-block towers)
	const Operand genIn = operand("gen_in");
	void *preWarp = c.temporalStrength > 0.0f ? m_Tensors.at("pre_warp").buf.get() : nullptr;
	b.prog->push_back({"warp", 0.0, [b, flowSlot, genIn, preWarp](hipStream_t s) {
		                   // (output_flow variant: this launch also writes the caller's frame, from the record it stores)
		                   launchWarpPack(b.dt, b.sb->in, *flowSlot, b.io->in, b.io->inStride, genIn.ptr, genIn.pitch, b.H, b.W, b.PW,
		                       b.padTop, b.padLeft, b.sums, preWarp, b.discard ? b.io->out : nullptr, b.discard ? b.io->outStride : 0, s);
	                   }});
}

// ---- generator ----
// calibration mode (JU_CALIBRATE=1, tools/calibrate.py): one launch per convolution, and
// after each the largest |output| of the layer folded into tower_profile[layer] -- works
// for every geometry and activation, unlike the resident kernel's in-kernel maxima
void Engine::addCalibStep(std::vector<Step> *prog, int layer, const std::string &tensor) {
	if (!m_Calibrate) return;
	const DType dt = m_DType;
	const Tensor &t = m_Tensors.at(tensor);
	const void *src = t.buf.get();
	const std::size_t n = t.count;
	unsigned *dst = m_Tensors.at("tower_profile").buf.as<unsigned>() + layer;
	prog->push_back({"calib", 0.0, [=](hipStream_t s) { launchAbsMax(dt, src, n, dst, s); }});
}

void Engine::addGeneratorHeadSteps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (m_Calibrate) {
		void *profile = m_Tensors.at("tower_profile").buf.get();
		const std::size_t bytes = (1 + 2 * static_cast<std::size_t>(c.genBlocks)) * 4;
		b.prog->push_back({"calib", 0.0, [=](hipStream_t s) { JU_HIP(hipMemsetAsync(profile, 0, bytes, s)); }});
	}
	if (m_Resident && !m_Fp8Tower) return;  // (the 16-bit resident tower runs conv_1 as its layer 0)
	// (64-filter generators: conv_tower_kernel -- 38 instead of 51 us at 640x448; other widths: the generic kernel)
	ConvOpt head;
	head.relu = true;
	head.tower = c.genFilters == 64 && !m_Calibrate;
	addConvStep(b.prog, "gen_head", "generator/conv_1", operand("gen_in"), Operand{}, operand("trunk_a"), b.H, b.W, head);
	addCalibStep(b.prog, 0, "trunk_a");
}

void Engine::addTowerSteps(ProgramBuild &b) {
	if (m_Resident && m_Fp8Tower) {
		addResidentTower8Step(b);
	} else if (m_Resident) {
		addResidentTowerStep(b);
	} else if (m_Fp8Tower) {
		addLayeredTower8Steps(b);
	} else {
		addLayeredTowerSteps(b);
	}
}

// the 8-bit tower in one launch: trunk_a (conv_1's output) -> trunk_b
void Engine::addResidentTower8Step(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	ResidentTower8Params rp{};
	rp.in = m_Tensors.at("trunk_a").buf.get();
	rp.out = m_Tensors.at("trunk_b").buf.get();
	rp.weights = m_Fp8TowerW.get();
	rp.scaleA = m_Fp8TowerScaleA.as<int>();
	rp.bias = m_Fp8TowerBias.as<float>();
	rp.scaleB = m_Fp8TowerScaleB.as<int>();
	rp.outMul = m_Fp8TowerMul.as<float>();
	rp.mailbox = m_GenTower.mail.get();
	rp.counters = m_GenTower.flags.as<unsigned>();
	rp.error = m_ResErrorDev;
	rp.H = b.H;
	rp.W = b.W;
	rp.GX = m_GenTower.GX;
	rp.GY = m_GenTower.GY;
	rp.RH = m_GenTower.RH;
	rp.nLayers = 2 * c.genBlocks;
	rp.leaky = c.genActivation == 1 ? 1 : 0;
	rp.slope = c.genNegativeSlope;
	rp.debug = m_Tensors.at("tower_profile").buf.get();
	b.prog->push_back({"tower", 2.0 * b.H * b.W * 9.0 * 64.0 * 64 * 2 * c.genBlocks,
	    [b, rp](hipStream_t s) { launchResidentTower8(b.dt, rp, s); }});
	b.trunk = "trunk_b";
}

// The fused tail's launch but for what ProgramBuild::bindTail adds when it runs: reads x, writes the HR state and the
// frame.  slope: the activation after convT1 (< 0: ReLU).
TailFusedLaunch Engine::fusedTail(Operand x, float slope, const unsigned *sums) {
	const ConvWeights &cw = m_Convs.at("generator/conv_trans_1");
	TailFusedLaunch tf{};
	tf.x = x.ptr;
	tf.xPitch = x.pitch;
	tf.w1 = cw.w.get();
	tf.b1 = cw.bias.as<float>();
	tf.w2 = m_TailW2Frag.get();
	tf.b2 = m_TailB2.as<float>();
	tf.sums = sums;
	tf.H = m_Config.frameHeight;
	tf.W = m_Config.frameWidth;
	tf.slope = slope;
	return tf;
}

// one launch for the whole tower -- with the tail on its LDS-resident last layer where the model allows
void Engine::addResidentTowerStep(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	ResidentTowerParams rp =
	    residentTowerParams(m_GenTower, b.H, b.W, 1 + 2 * c.genBlocks, c.genActivation, c.genNegativeSlope);
	rp.in = operand("gen_in").ptr;  // tower layout [..][pitch][64] at image pixel (0, 0); conv_1 is layer 0 of the launch
	rp.inPitch = operand("gen_in").pitch;
	rp.out = operand("trunk_b").ptr;
	b.tailInTower = m_FusedTail && m_TailInTower && c.genFilters == 64 && c.genActivation == 0;
	TailFusedLaunch tf{};  // (debug variants of the tower kernel have no fused-tail form: separate launch)
	if (b.tailInTower) {
		tf = fusedTail(operand("trunk_b"), -1.0f, b.sums);
		rp.tailW1 = tf.w1;
		rp.tailB1 = tf.b1;
		rp.tailW2 = tf.w2;
		rp.tailB2 = tf.b2;
		rp.sums = tf.sums;
	}
	b.prog->push_back({"tower",
	    2.0 * b.H * b.W * 9.0 * ((c.recurrent() ? 51.0 : 3.0) * 64 + 64.0 * 64 * 2 * c.genBlocks) +
	        (b.tailInTower ? 2.0 * b.H * b.W * (64.0 * 128 + 4 * 4 * 32 * 3) : 0.0),
	    [b, rp, tf](hipStream_t s) {
		    ResidentTowerParams r = rp;
		    if (r.tailW1 != nullptr && towerVariant() != 0) {
			    // a diagnostic variant of the kernel (plain schedule, calibration, phase profile,
			    // ablations): it writes the trunk, and the same tail code runs as its own launch
			    r.tailW1 = nullptr;
			    launchResidentTower(b.dt, r, s);
			    TailFusedLaunch t = tf;
			    b.bindTail(&t);
			    launchTailFused(b.dt, t, s);
			    return;
		    }
		    if (r.tailW1 != nullptr) b.bindTail(&r);  // caller's frames are known at launch time only
		    launchResidentTower(b.dt, r, s);
	    }});
	b.trunk = "trunk_b";
}

// the 8-bit tower per block or per convolution:
// stream (fp16, trunk_a, updated in place) + e4m3 copies x8 / t8 of the conv inputs
void Engine::addLayeredTower8Steps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	void *streamBuf = m_Tensors.at("trunk_a").buf.get();
	void *x8 = m_Fp8X.get(), *t8 = m_Fp8T.get();
	const int e0 = m_Fp8Exp[0];
	const bool leaky8 = c.genActivation == 1;
	b.prog->push_back({"tower", 0.0,
	    [b, streamBuf, x8, e0, leaky8](hipStream_t s) { launchQuantizeTower(b.dt, streamBuf, x8, b.H, b.W, e0, leaky8, s); }});
	for (int i = 0; i < c.genBlocks && m_BlockFused; ++i) {
		// one launch per block: the e4m3 stream copy ping-pongs between the two tensors
		const std::string n = "generator/block_" + std::to_string(i + 1);
		const Fp8Conv &q1 = m_Fp8Convs.at(n + "/conv_1"), &q2 = m_Fp8Convs.at(n + "/conv_2");
		Fp8BlockLaunch fb{};
		fb.in8 = (i & 1) ? t8 : x8;
		fb.out8 = (i & 1) ? x8 : t8;
		fb.stream = streamBuf;
		fb.w1 = q1.w.get();
		fb.w2 = q2.w.get();
		fb.scaleA1 = q1.scaleA.as<int>();
		fb.scaleA2 = q2.scaleA.as<int>();
		fb.b1 = m_Convs.at(n + "/conv_1").bias.as<float>();
		fb.b2 = m_Convs.at(n + "/conv_2").bias.as<float>();
		fb.inExp = m_Fp8Exp[2 * i];
		fb.midExp = m_Fp8Exp[2 * i + 1];
		fb.outExp = (i + 1 < c.genBlocks) ? m_Fp8Exp[2 * i + 2] : 0;  // (the last copy has no reader)
		fb.H = b.H;
		fb.W = b.W;
		fb.leaky = leaky8 ? 1 : 0;
		fb.slope = c.genNegativeSlope;
		b.prog->push_back({"tower", 2.0 * b.H * b.W * 9.0 * 64 * 64 * 2, [b, fb](hipStream_t s) { launchResBlockFp8(b.dt, fb, s); }});
	}
	for (int i = 0; i < c.genBlocks && !m_BlockFused; ++i) {
		const std::string n = "generator/block_" + std::to_string(i + 1);
		for (int j = 0; j < 2; ++j) {
			const std::string name = n + (j ? "/conv_2" : "/conv_1");
			const Fp8Conv &q = m_Fp8Convs.at(name);
			Fp8TowerParams fp{};
			fp.in8 = j ? t8 : x8;
			fp.weights = q.w.get();
			fp.scaleA = q.scaleA.as<int>();
			fp.bias = m_Convs.at(name).bias.as<float>();
			fp.stream = j ? streamBuf : nullptr;
			fp.out8 = j ? x8 : t8;
			fp.inExp = m_Fp8Exp[2 * i + j];
			// the last block's e4m3 copy has no reader; any exponent will do
			fp.outExp = (2 * i + j + 1 < 2 * c.genBlocks) ? m_Fp8Exp[2 * i + j + 1] : 0;
			fp.H = b.H;
			fp.W = b.W;
			fp.leaky = leaky8 ? 1 : 0;
			fp.slope = c.genNegativeSlope;
			b.prog->push_back({"tower", 2.0 * b.H * b.W * 9.0 * 64 * 64, [b, fp](hipStream_t s) { launchConvTowerFp8(b.dt, fp, s); }});
		}
	}
}

// the 16-bit tower per block (64 filters) or per convolution, the trunk ping-ponging between trunk_a and trunk_b
void Engine::addLayeredTowerSteps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	const char *xs[2] = {"trunk_a", "trunk_b"};
	int a = 0;
	ConvOpt conv;
	conv.relu = conv.tower = true;
	for (int i = 0; i < c.genBlocks; ++i, a ^= 1) {
		const std::string n = "generator/block_" + std::to_string(i + 1);
		if (m_BlockFused && c.genFilters == 64) {
			addResBlockStep(b.prog, "tower", n, operand(xs[a]), operand(xs[a ^ 1]), b.H, b.W, c.genActivation, c.genNegativeSlope);
			continue;
		}
		addConvStep(b.prog, "tower", n + "/conv_1", operand(xs[a]), Operand{}, operand("trunk_t"), b.H, b.W, conv);
		addCalibStep(b.prog, 2 * i + 1, "trunk_t");
		addConvStep(b.prog, "tower", n + "/conv_2", operand("trunk_t"), operand(xs[a]), operand(xs[a ^ 1]), b.H, b.W, conv);
		addCalibStep(b.prog, 2 * i + 2, xs[a ^ 1]);
	}
	b.trunk = xs[a];
}

void Engine::addTailSteps(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (b.tailInTower) {
		// (nothing: the resident tower wrote the HR state and the frame)
	} else if (m_FusedTail && c.genFilters == 64) {
		const TailFusedLaunch tf = fusedTail(operand(b.trunk), c.genActivation == 1 ? c.genNegativeSlope : -1.0f, b.sums);
		b.prog->push_back({"tail", 2.0 * b.H * b.W * (64.0 * 128 + 4 * 4 * 32 * 3), [b, tf](hipStream_t s) {
			                   TailFusedLaunch t = tf;
			                   b.bindTail(&t);
			                   launchTailFused(b.dt, t, s);
		                   }});
	} else {
		ConvOpt relu;
		relu.relu = true;
		addConvStep(b.prog, "tail", "generator/conv_trans_1", operand(b.trunk), Operand{}, operand("tail_y"), b.H, b.W, relu);
		const void *y = m_Tensors.at("tail_y").buf.get();
		const float *w2 = m_TailW2.as<float>();
		const float *b2 = m_TailB2.as<float>();
		b.prog->push_back({"tail", 2.0 * (2 * b.H) * (2 * b.W) * 4 * 32 * 3, [b, y, w2, b2](hipStream_t s) {
			                   launchTail(b.dt, y, w2, b2, b.io->in, b.io->inStride, b.sb->out, b.genOutU8(), b.genOutStride(), b.H,
			                       b.W, b.sums, s);
		                   }});
	}
}

// ---- optional output filter (frame_moving_avg.py): replaces the clip output for
// both of its consumers, the u8 frame and the fed-back state ----
void Engine::addTemporalStep(ProgramBuild &b) {
	const ModelConfig &c = m_Config;
	if (!(c.temporalStrength > 0.0f)) return;
	const void *preWarp = m_Tensors.at("pre_warp").buf.get();
	unsigned long long *acc = m_TemporalAcc.as<unsigned long long>();
	const TemporalParams tp{c.temporalStrength, c.temporalThreshold, c.temporalGain, c.temporalWindow,
	    c.temporalL2 ? 1 : 0, c.temporalLimit ? 1 : 0, c.temporalLuma ? 1 : 0};
	b.prog->push_back({"temporal", 0.0, [b, preWarp, acc, tp](hipStream_t s) {
		                   launchTemporalFilter(b.sb->out, preWarp, b.genOutU8(), b.genOutStride(), b.H, b.W, b.sums, acc, tp, s);
	                   }});
}

}  // namespace ju
