#include "engine.h"

#include <cstdio>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>

#include "dev_switch.h"
#include "fp8.h"
#include "graphics.h"
#include "log.h"

namespace ju {

namespace {
thread_local int g_DryLaunches = 0;
}
bool launchesAreDry() { return g_DryLaunches > 0; }
DryLaunchScope::DryLaunchScope() { ++g_DryLaunches; }
DryLaunchScope::~DryLaunchScope() { --g_DryLaunches; }

Engine::Tensor &Engine::addTensor(
    const std::string &name, std::size_t count, bool f32, bool state) {
	Tensor t;
	t.buf = DeviceBuffer(count * (f32 ? 4 : 2));
	t.count = count;
	t.isF32 = f32;
	t.isState = state;
	auto res = m_Tensors.emplace(name, std::move(t));
	if (!res.second) throw std::logic_error("duplicate tensor " + name);
	return res.first->second;
}

Engine::Tensor &Engine::addTowerTensor(const std::string &name, int H, int W, int C) {
	Tensor &t = addTensor(name, towerPixels(H, W) * C);
	t.towerH = H;
	t.towerW = W;
	t.towerC = C;
	return t;
}

Engine::Operand Engine::operand(const std::string &name) {
	Tensor &t = m_Tensors.at(name);
	Operand o;
	o.ptr = t.buf.get();
	if (t.towerC) {
		o.pitch = towerPitch(t.towerW);
		o.ptr = t.buf.as<unsigned char>() + towerOrigin(t.towerW) * t.towerC * 2;
	}
	return o;
}

namespace {
// Runtimes of this process per device, and the completion event of the frame submitted
// last by one that uses the resident tower (Engine::chainBegin / chainEnd).
struct DeviceChain {
	// Held by an engine from its wait on `last` until its own completion event is recorded,
	// so that wait, launches and record are ONE step per device: two threads driving two
	// resident runtimes cannot both pass the wait against the same previous frame.
	std::mutex mutex;
	int engines = 0;
	const void *lastOwner = nullptr;
	hipEvent_t last = nullptr;
};
std::mutex g_ChainMapMutex;
std::map<int, DeviceChain> g_Chains;  // (map nodes never move: references stay valid)
DeviceChain &chainOf(int device) {
	std::lock_guard<std::mutex> lock(g_ChainMapMutex);
	return g_Chains[device];
}
}  // namespace

std::unique_lock<std::mutex> Engine::chainBegin(bool resident) {
	DeviceChain &c = chainOf(m_Device);
	std::unique_lock<std::mutex> lock(c.mutex);
	if (c.engines > 1 && resident && c.last != nullptr && c.lastOwner != this) {
		JU_HIP(hipStreamWaitEvent(m_Stream, c.last, 0));
	}
	return lock;
}

void Engine::chainEnd(std::unique_lock<std::mutex> &lock, bool resident) {
	DeviceChain &c = chainOf(m_Device);
	if (c.engines > 1 && resident) {
		m_FrameDone.record(m_Stream);
		c.last = m_FrameDone.get();
		c.lastOwner = this;
	}
	lock.unlock();
}

Engine::ConvWeights &Engine::addConv(const std::string &name, const FoldedConv &f,
    const std::vector<int> &cinMap, int H, int W) {
	ConvWeights cw;
	// generator conv_1 (64 padded input channels) runs as layer 0 of the resident tower
	const bool towerLayer = name.rfind("generator/block_", 0) == 0 || name == "generator/conv_1";
	// flow-resnet with 64 filters: its blocks are packed like the generator's tower
	const bool flowTower = m_Config.flowArch == 1 && m_Config.flowResFilters == 64;
	const bool flowBlock = flowTower && name.rfind("flow/block_", 0) == 0;
	if ((towerLayer && f.cout == 64) || flowBlock || name == "generator/conv_trans_1") {
		cw.nb = 2;  // the tower kernels and the fused tail read the 64-cout-block layout
		cw.rw = 2;
	} else if (flowConvIsFused(name)) {
		cw.nb = 1;  // flow_block_kernel: one 32-cout block of fragments per wave
		cw.rw = 1;
	} else if (m_FlowFused && name.rfind("flow/", 0) == 0 && f.taps == 9 && (cinMap.size() == 128 || cinMap.size() == 256) &&
	           f.cout % 32 == 0 && H * W <= 32768) {
		cw.nb = 1;  // conv_splitk_kernel (the coarse levels of the flow net): 32-cout blocks of fragments
		cw.rw = 1;
		cw.splitK = true;
	} else {
		convTiling(H, W, f.cout, &cw.nb, &cw.rw);
		// JU_CONV_TILE (developer switch): another of the kernel's tile forms where the layer has it -- here, so that the
		// weights are packed for the same nb (a pooled / upsampling layer still gets the rw it needs: addConvStep)
		if ((m_Plan.convNb == 1 || m_Plan.convNb == 2) && (m_Plan.convRw == 1 || m_Plan.convRw == 2) &&
		    f.cout % (32 * m_Plan.convNb) == 0) {
			cw.nb = m_Plan.convNb;
			cw.rw = m_Plan.convRw;
		}
	}
	const auto packed = packConvWeights(f, cinMap, cw.nb, m_DType);
	cw.w = DeviceBuffer(packed.size() * 2);
	cw.w.upload(packed.data(), packed.size() * 2);
	cw.bias = DeviceBuffer(f.bias.size() * 4);
	cw.bias.upload(f.bias.data(), f.bias.size() * 4);
	if (f.cin == 64 && f.cout == 64 && f.taps == 9 &&
	    (name.rfind("generator/block_", 0) == 0 || flowBlock)) {
		const auto blk = packConvWeights(f, cinMap, 1, m_DType);
		cw.wBlock = DeviceBuffer(blk.size() * 2);
		cw.wBlock.upload(blk.data(), blk.size() * 2);
	}
	cw.cinP = static_cast<int>(cinMap.size());
	cw.cout = f.cout;
	cw.taps = f.taps;
	cw.cinReal = f.cin;
	if (m_Fp8Tower && name.rfind("generator/block_", 0) == 0 && f.cout == 64 && f.cin == 64) {
		const Fp8ConvWeights q = packFp8TowerWeights(f);
		m_Fp8Folded.emplace(name, f);
		Fp8Conv dev;
		dev.w = DeviceBuffer(q.w.size());
		dev.w.upload(q.w.data(), q.w.size());
		dev.scaleA = DeviceBuffer(q.scaleA.size() * 4);
		dev.scaleA.upload(q.scaleA.data(), q.scaleA.size() * 4);
		m_Fp8Convs.emplace(name, std::move(dev));
	}
	// the resident tower's own copy of its layers' weights, in the fragment order of ITS MFMA shape (the per-block and
	// per-convolution kernels keep reading cw.w / cw.wBlock)
	auto residentPack = [&](const std::vector<int> &map64) {
		return residentTowerM16() ? packTowerWeightsM16(f, map64, m_DType) : packConvWeights(f, map64, 2, m_DType);
	};
	if (towerLayer && f.cout == 64 && cinMap.size() == 64) {  // tower layers, in execution order
		const auto w = residentPack(cinMap);
		m_GenTower.hostW.insert(m_GenTower.hostW.end(), w.begin(), w.end());
		m_GenTower.hostB.insert(m_GenTower.hostB.end(), f.bias.begin(), f.bias.end());
	} else if (towerLayer) {  // (other generator widths never run the resident kernel; kept for the layer count)
		m_GenTower.hostW.insert(m_GenTower.hostW.end(), packed.begin(), packed.end());
		m_GenTower.hostB.insert(m_GenTower.hostB.end(), f.bias.begin(), f.bias.end());
	}
	if (flowBlock) {
		const auto w = residentPack(cinMap);
		m_FlowTower.hostW.insert(m_FlowTower.hostW.end(), w.begin(), w.end());
		m_FlowTower.hostB.insert(m_FlowTower.hostB.end(), f.bias.begin(), f.bias.end());
	} else if (flowTower && name == "flow/conv_1") {
		// layer 0 of the flow tower reads 64-channel records: same kernel, input
		// channels 12.. are zero (the per-layer path keeps its own 16-channel packing)
		std::vector<int> map64(64, -1);
		for (int k = 0; k < f.cin && k < 64; ++k) map64[k] = k;
		const auto head = residentPack(map64);
		m_FlowTower.hostW.insert(m_FlowTower.hostW.end(), head.begin(), head.end());
		m_FlowTower.hostB.insert(m_FlowTower.hostB.end(), f.bias.begin(), f.bias.end());
	}
	auto res = m_Convs.emplace(name, std::move(cw));
	if (!res.second) throw std::logic_error("duplicate conv " + name);
	return res.first->second;
}

void Engine::buildWeights(const ModelFile &model) {
	// fold + check on the host (model.cpp), then tile, pack and upload layer by layer
	for (const ConvSpec &s : foldModel(model)) addConv(s.name, s.conv, s.cinMap, s.H, s.W);
	{
		const TensorView &k2 = model.tensor("generator/conv_trans_2/kernel", {2, 2, 3, 32});
		const TensorView &b2 = model.tensor("generator/conv_trans_2/bias", {3});
		m_TailW2 = DeviceBuffer(k2.count * 4);
		m_TailW2.upload(k2.data, k2.count * 4);
		m_TailB2 = DeviceBuffer(48);  // convT2 bias (3 f32) + from byte 16: the frame's channel sums (3 x 64 bits)
		m_TailB2.upload(b2.data, 12);
		const auto frag = packTailWeights(k2.data, m_DType);
		m_TailW2Frag = DeviceBuffer(frag.size() * 2);
		m_TailW2Frag.upload(frag.data(), frag.size() * 2);
	}
}

Engine::Engine(int device, const void *blob, std::size_t size, int dtypeOverride)
    : m_Device(device) {
	// Like TensorRTBackend (tensorrt_backend.cc:118), the engine is built on the
	// CURRENT device; the caller (c_api.cpp) selects it for the call.
	int current = -1;
	JU_HIP(hipGetDevice(&current));
	if (current != device) throw std::logic_error("Engine must be created with its device current");
	ModelFile model(blob, size);
	m_Config = model.config();
	const ModelConfig &c = m_Config;
	int dt = dtypeOverride >= 0 ? dtypeOverride : c.computeDtype;
	// (the identity a group pass checks its members against: processGroup)
	m_ModelDigest = 14695981039346656037ull;  // FNV-1a, 64 bit
	for (std::size_t i = 0; i < size; ++i) {
		m_ModelDigest = (m_ModelDigest ^ static_cast<const unsigned char *>(blob)[i]) * 1099511628211ull;
	}
	m_DtypeOverride = dt;
	if (dt == 2) {
		// JU_DTYPE_FP8: the 64->64 block convolutions run on e4m3 operands (fp8.h); the
		// residual stream and every other layer stay fp16
		if (c.genFilters != 64 || c.genBlocks < 1) {
			throw std::invalid_argument("fp8 tower needs a 64-filter generator with at least one residual block");
		}
		m_Fp8Tower = true;
		dt = kF16;
	}
	if (dt != kF16 && dt != kBF16) throw std::invalid_argument("Unsupported compute dtype");
	m_DType = static_cast<DType>(dt);
	readSwitches();
	planFlowUnits();
	buildWeights(model);  // (in front of the towers' set-up, which uploads the layers addConv collected)
	setUpResidentTowers();
	allocateBuffers(model);
	buildProgram(0);
	buildProgram(1);
	bindStaging();
	warmUpAndCapture();
}

namespace {
bool switchIs(Dev which, const char *word) {
	const char *v = devSwitch(which);
	return v && std::string(v) == word;
}
}  // namespace

// The switches of the program's paths and of how frames are submitted (the towers' own: setUpResidentTowers).
void Engine::readSwitches() {
	m_FusedTail = !switchIs(Dev::Tail, "split");
	// The fused tail runs INSIDE the resident tower launch wherever that kernel is used with a
	// ReLU generator (its last layer is in LDS: the trunk is never written or re-read, one launch
	// less).  Bit-identical to the separate launch (same row code); round 2 measured +0.5-1 % and
	// kept it opt-in, under round 3's steady-state timing it is +0.9 % at 480x270 and +1.9 % for
	// psp-fast (tools/submit_overhead.py, three A/B rounds), so it is the default now.
	// JU_TAIL=fused: the separate tail_fused_kernel launch; JU_TAIL=split: the two-kernel tail.
	m_TailInTower = !switchIs(Dev::Tail, "fused") && !switchIs(Dev::Tail, "split");
	m_PackInBlock = !switchIs(Dev::Pack, "split");  // JU_PACK=split: pack_frames_kernel as its own launch
	m_FusedPool = !switchIs(Dev::Pool, "split");
	m_FusedUpsample = !switchIs(Dev::Upsample, "split");
	// (JU_UPSAMPLE=split keeps the one-launch blocks: the decoder's take their non-upsampling form behind an
	// upsample2_kernel launch -- planFlowUnits)
	m_FlowFused = !switchIs(Dev::FlowConv, "generic");
	// The launch plan switches (kernels.h DevPlan), read HERE and nowhere else: the launch descriptors carry them, so two
	// runtimes of one process can run different plans.  devSwitch() is null for every one of them in the product library.
	if (const char *e = devSwitch(Dev::FlowTile)) m_Plan.flowTile = std::atoi(e);
	if (const char *e = devSwitch(Dev::ResBlock)) m_Plan.resBlock = std::string(e) == "plain" ? 1 : (std::string(e) == "tile" ? 2 : 0);
	if (const char *e = devSwitch(Dev::ConvDbuf)) m_Plan.convStages = (e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : -1;
	if (const char *e = devSwitch(Dev::SplitKPlan)) {  // <rows>[x<blocks>]
		m_Plan.splitkRows = std::atoi(e);
		if (const char *x = std::strchr(e, 'x')) m_Plan.splitkBlocks = std::atoi(x + 1);
	}
	if (const char *e = devSwitch(Dev::ConvTile)) {  // <nb>x<rw>
		m_Plan.convNb = std::atoi(e);
		if (const char *x = std::strchr(e, 'x')) m_Plan.convRw = std::atoi(x + 1);
	}
	if (devSwitchesExist()) m_Plan.log = &m_PlanLog;
	const char *direct = devSwitch(Dev::Direct);
	m_PreferDirect = !(direct && direct[0] == '0');
	if (const char *retry = std::getenv("JU_RESIDENT_RETRY")) m_RetryBase = static_cast<unsigned>(std::atoi(retry));
	const char *directGraph = devSwitch(Dev::DirectGraph);
	m_DirectGraph = !(directGraph && directGraph[0] == '0');
	if (const char *spin = devSwitch(Dev::SyncSpinUs)) m_SpinUs = static_cast<unsigned>(std::atoi(spin));
	// frames per look-ahead pass of processBatch (1 = frame by frame)
	if (const char *la = std::getenv("JU_LOOKAHEAD")) m_BatchMax = std::min(std::max(std::atoi(la), 1), kFlowBatchMax);
}

// One resident tower, where it is wanted and the H x W frame has a geometry of one co-resident workgroup per region: the
// layers addConv collected go to the device, beside a mailbox and the publish counts.  The host copy goes either way.
bool Engine::setUpResidentTower(ResidentTower *t, bool wanted, int H, int W, int cus, bool leaky) {
	const bool on = wanted && residentTowerGeometry(H, W, cus, &t->GX, &t->GY, &t->RH);
	if (on) {
		t->w = DeviceBuffer(t->hostW.size() * 2);
		t->w.upload(t->hostW.data(), t->hostW.size() * 2);
		t->b = DeviceBuffer(t->hostB.size() * 4);
		t->b.upload(t->hostB.data(), t->hostB.size() * 4);
		// (`activation: lrelu`: twice the slots -- the epoch travels beside the values)
		const bool eightBit = m_Fp8Tower && t == &m_GenTower;
		t->mail = DeviceBuffer(eightBit ? residentMailboxBytes8(t->GX, t->GY, leaky) : residentMailboxBytes(t->GX, t->GY, leaky));
		t->flags = DeviceBuffer(residentCounterBytes(t->GX, t->GY));  // publish counts per region
	}
	t->hostW.clear();
	t->hostW.shrink_to_fit();
	return on;
}

// ---- resident towers: each needs 64 filters and one co-resident workgroup per region ----
void Engine::setUpResidentTowers() {
	const ModelConfig &c = m_Config;
	int cus = 0;
	JU_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m_Device));
	bool wanted = !switchIs(Dev::Tower, "layers") && !switchIs(Dev::Tower, "convs");
	m_BlockFused = !switchIs(Dev::Tower, "convs");
	const char *calib = devSwitch(Dev::Calibrate);
	m_Calibrate = calib && calib[0] == '1';
	if (m_Calibrate) {
		if (m_Fp8Tower) throw std::invalid_argument("calibration mode: calibrate the fp16 / bf16 engine, not the 8-bit one");
		wanted = false;
		m_BlockFused = false;
	}
	m_Resident = m_ResidentCapable = setUpResidentTower(&m_GenTower, wanted && c.genFilters == 64 && c.genBlocks >= 1,
	    c.frameHeight, c.frameWidth, cus, c.genActivation == 1);
	if (m_Resident) {
		m_ResError = PinnedWords(64);
		m_ResErrorDev = m_ResError.device();
	}
	if (switchIs(Dev::Flow, "convs")) m_BlockFused = false;
	const bool flowWanted = m_Resident && !switchIs(Dev::Flow, "layers") && !switchIs(Dev::Flow, "convs") && c.flowArch == 1 &&
	                        c.flowResFilters == 64 && c.flowResBlocks >= 1 && 3 * c.numFlowInputs <= 64;
	m_ResidentFlow = m_ResidentFlowCapable =
	    setUpResidentTower(&m_FlowTower, flowWanted, c.paddedHeight(), c.paddedWidth(), cus, c.flowActivation == 1);
}

// ---- buffers (all zero-initialised) ----
void Engine::allocateBuffers(const ModelFile &model) {
	const ModelConfig &c = m_Config;
	const int H = c.frameHeight, W = c.frameWidth;
	const int PH = c.paddedHeight(), PW = c.paddedWidth();
	const std::size_t lr = static_cast<std::size_t>(H) * W;
	const std::size_t plr = static_cast<std::size_t>(PH) * PW;
	m_InStage = DeviceBuffer(lr * 4);
	m_OutStage = DeviceBuffer(lr * 16 * 4);
	m_RawStage = DeviceBuffer(lr * 16 * 4);
	if (c.outputsPreWarp()) m_DiscardFrame = DeviceBuffer(lr * 16 * 4);  // (buildProgram: where the generator's frame goes)
	// 10-bit outputs come from the f16 state wherever the state the step leaves is the frame in float: not with
	// normalize_brightness (the state is output_raw - b; flow-free models ignore the flag) nor in the output_flow
	// variant (the frame is pre_warp)
	m_HbdFromState = !(c.normalizeBrightness && c.recurrent()) && !c.outputsPreWarp();
	// host YUV frames (ju_process_frame): their planes, rows padded to 64 bytes
	m_YuvInStage = DeviceBuffer(yuvStageBytes(kFormatTable, W, H));
	m_YuvOutStage = DeviceBuffer(yuvStageBytes(kFormatTable, 4 * W, 4 * H));
	if (!c.recurrent()) {
		// flow-free: no frame history, no flow tensors, no state ping-pong -- one scratch state for the tail's
		// HR output, which nothing reads; gen_in's slots other than 12..14 stay zero for good (lr_pack)
		m_State[0] = DeviceBuffer(lr * 16 * 4 * 2);
	} else {
		for (int i = 0; i < 2; ++i) {
			m_State[i] = DeviceBuffer(lr * 16 * 4 * 2);  // f16 [4H][4W][4]
			m_Packed[i] = DeviceBuffer(plr * 16 * 2);     // [PH][PW][16]
		}
	}
	if (!c.recurrent()) {
		// (no flow net)
	} else if (c.flowArch == 0) {
		const int nb = static_cast<int>(c.flowFilters.size()) / 2;
		std::size_t px = plr;
		for (int i = 0; i < 2 * nb; ++i) {
			const std::string n = "flow/block_" + std::to_string(i + 1);
			const std::size_t f = c.flowFilters[i];
			addTensor(n + "/a_1", px * f);
			addTensor(n + "/a_2", px * f);
			px = i < nb ? px / 4 : px * 4;
			addTensor(n + "/resample", px * f);
		}
		if (c.flowFilters.size() % 2) addTensor("flow/a_1", px * c.flowFilters.back());
	} else {
		if (m_ResidentFlow) {
			addTensor("flow/in64", plr * 64);  // [PH][PW][64]: ch 0..15 = the packed flow input, rest zero
			addTowerTensor("flow/trunk", PH, PW, 64);
		}
		addTensor("flow/x0", plr * c.flowResFilters);
		addTensor("flow/x1", plr * c.flowResFilters);
		addTensor("flow/t", plr * c.flowResFilters);
	}
	if (c.recurrent()) addTensor("flow", plr * 32, false, true);  // the flow head: f16 whatever the compute type
	addTowerTensor("gen_in", H, W, 64);
	if (c.temporalStrength > 0.0f) {
		addTensor("pre_warp", lr * 16 * 4);  // f16 [4H][4W][4]
		m_TemporalAcc = DeviceBuffer(8 * temporalAccWords(H, W, c.temporalWindow));
	}
	addTowerTensor("trunk_a", H, W, c.genFilters);
	addTowerTensor("trunk_b", H, W, c.genFilters);
	addTowerTensor("trunk_t", H, W, c.genFilters);
	if (m_Fp8Tower) {
		m_Fp8X = DeviceBuffer(towerPixels(H, W) * 64);
		m_Fp8T = DeviceBuffer(towerPixels(H, W) * 64);
		// activation ranges: optional calibration tensor, else one fixed scale (fp8.h)
		m_Fp8Exp.assign(2 * static_cast<std::size_t>(c.genBlocks), fp8ActivationExponent(kFp8DefaultAmax));
		if (model.has("generator/fp8_amax")) {
			const TensorView &am = model.tensor("generator/fp8_amax", {2 * c.genBlocks});
			for (int i = 0; i < 2 * c.genBlocks; ++i) m_Fp8Exp[i] = fp8ActivationExponent(am.data[i]);
		}
		if (m_ResidentCapable) packResidentTower8();
		m_Fp8Folded.clear();
	}
	addTensor("tail_y", lr * 128);
	addTensor("tower_profile", 256 * 4 * 8 * 2, true);  // u64 cycle sums of the diagnostic tower variant
}

// operands of the one-launch 8-bit tower, convolution by convolution
void Engine::packResidentTower8() {
	const int L = 2 * m_Config.genBlocks;
	std::vector<unsigned char> w;
	std::vector<int> scaleA, scaleB(L);
	std::vector<float> bias, mul(L + 1);
	for (int i = 0; i < L; ++i) {
		const std::string name = "generator/block_" + std::to_string(i / 2 + 1) + (i % 2 ? "/conv_2" : "/conv_1");
		const Fp8ConvWeights q = packFp8TowerWeights(m_Fp8Folded.at(name));
		w.insert(w.end(), q.w.begin(), q.w.end());
		scaleA.insert(scaleA.end(), q.scaleA.begin(), q.scaleA.end());
		const std::vector<float> &b = m_Fp8Folded.at(name).bias;
		bias.insert(bias.end(), b.begin(), b.end());
		scaleB[i] = 127 - m_Fp8Exp[i];
		mul[i] = std::ldexp(1.0f, i + 1 < L ? m_Fp8Exp[i + 1] : 0);  // (the last copy has no reader)
	}
	mul[L] = std::ldexp(1.0f, m_Fp8Exp[0]);
	auto up = [](DeviceBuffer *d, const void *src, std::size_t n) {
		*d = DeviceBuffer(n);
		d->upload(src, n);
	};
	up(&m_Fp8TowerW, w.data(), w.size());
	up(&m_Fp8TowerScaleA, scaleA.data(), scaleA.size() * 4);
	up(&m_Fp8TowerBias, bias.data(), bias.size() * 4);
	up(&m_Fp8TowerScaleB, scaleB.data(), scaleB.size() * 4);
	up(&m_Fp8TowerMul, mul.data(), mul.size() * 4);
}

void Engine::captureFrameGraphs() {
	for (int s = 0; s < 2; ++s) {
		m_Graph[s] = GraphExec::capture(m_Stream, [&] {
			for (const Step &st : m_Program[s]) st.run(m_Stream);
		});
	}
}

// The eager warm-up of both programs on the staging buffers, then their graphs.
void Engine::warmUpAndCapture() {
	const int H = m_Config.frameHeight, W = m_Config.frameWidth;
	const char *noGraph = std::getenv("JU_NO_GRAPH");
	const bool useGraph = !(noGraph && noGraph[0] == '1');
	// From here on this engine launches kernels.  It joins its device's chain first and holds
	// the chain's lock until it is ready: the eager passes below run the resident tower, which
	// must not overlap a frame of another resident runtime on this device (each wants a
	// workgroup on every CU).  Frames those runtimes have in flight are waited for once, here
	// (they record completion events only while more than one engine exists).
	DeviceChain &chain = chainOf(m_Device);
	std::lock_guard<std::mutex> chainLock(chain.mutex);
	++chain.engines;
	try {
		if (chain.engines > 1) JU_HIP(hipDeviceSynchronize());
		// One eager pass per binding set: sets the kernels' dynamic-LDS attributes
		// and surfaces launch errors before anything is captured.
		m_UseGraph = false;
		// JU_TRACE_STEPS=<file> (developer switch): every launch of this eager pass is appended to the file BEFORE it
		// runs and waited for after -- the last line names the kernel behind a GPU memory fault, which the runtime
		// otherwise reports asynchronously and without a name
		const char *trace = devSwitch(Dev::TraceSteps);
		const bool traceSync = !devSwitch(Dev::TraceNoSync);  // (JU_TRACE_NOSYNC=1: the list only)
		for (int s = 0; s < 2; ++s) {
			int k = 0;
			for (const Step &st : m_Program[s]) {
				if (trace) {
					if (std::FILE *f = std::fopen(trace, "a")) {
						std::fprintf(f, "%dx%d dtype %d%s set %d step %d %s\n", W, H, static_cast<int>(m_DType), m_Fp8Tower ? " fp8" : "", s, k,
						    st.tag.c_str());
						std::fclose(f);
					}
				}
				st.run(m_Stream);
				if (trace && traceSync) m_Stream.synchronize();
				++k;
			}
		}
		m_Stream.synchronize();
		if (const unsigned code = takeResidentError()) {
			fallbackToLayers(code);
			for (int s = 0; s < 2; ++s) {
				for (const Step &st : m_Program[s]) st.run(m_Stream);
			}
			m_Stream.synchronize();
		}
		reset();
		m_UseGraph = useGraph;
		if (m_UseGraph) {
			captureFrameGraphs();
			m_Stream.synchronize();
		}
		std::ostringstream ss;
		ss << "engine ready: " << W << "x" << H << " -> " << 4 * W << "x" << 4 * H << ", "
		   << (m_DType == kF16 ? "fp16" : "bf16") << ", " << m_Program[0].size()
		   << " launches/frame, tower=" << (m_Resident ? "resident" : "per-layer")
		   << ", graph=" << (m_UseGraph ? "on" : "off");
		logMessage(LogLevel::Info, "Engine", ss.str());
	} catch (...) {
		--chain.engines;  // (no destructor runs for a half-built engine)
		throw;
	}
}

Engine::~Engine() {
	try {
		DeviceGuard g(m_Device);
		(void)hipStreamSynchronize(m_Stream);
		DeviceChain &c = chainOf(m_Device);
		std::lock_guard<std::mutex> lock(c.mutex);
		if (c.lastOwner == this) {  // (its event dies with this engine; the work behind it is done)
			c.last = nullptr;
			c.lastOwner = nullptr;
		}
		if (c.engines > 0) --c.engines;
	} catch (...) {
	}
}

unsigned Engine::takeResidentError() {
	volatile unsigned *word = m_ResError.host();
	if (word == nullptr || *word == 0) return 0;
	const unsigned code = *word;
	*word = 0;
	return code;
}

// The resident tower needs every workgroup co-resident (one per CU).  When a bounded
// neighbour wait expires -- CUs masked off or taken by another process -- the engine
// does not stay broken: it switches to the per-layer tower kernels for good.
void Engine::fallbackToLayers(unsigned code) {
	std::ostringstream ss;
	ss << "resident tower kernel: a bounded wait on a neighbouring workgroup expired (code 0x"
	   << std::hex << code << std::dec << "); " << m_GenTower.GX * m_GenTower.GY
	   << " workgroups are not all co-resident on this device. Switching to the per-layer tower "
	      "kernels (slower)";
	++m_Fallbacks;
	m_CleanFrames = 0;
	// retry after 512, 2048, 8192, ... clean frames
	m_RetryAfter = m_RetryBase ? std::min<std::uint64_t>(std::uint64_t(m_RetryBase) << (2 * std::min(m_Fallbacks - 1, 8u)), 1u << 30) : 0;
	if (m_RetryAfter) ss << "; the resident kernel will be tried again after " << m_RetryAfter << " frames";
	logMessage(LogLevel::Warning, "Engine", ss.str());
	m_Resident = false;
	m_ResidentFlow = false;
	dropAllGraphs();  // they replay the resident program
	zeroResidentMailboxes();  // the aborted launch left the slot epochs of the regions out of step: start them over
	m_Stream.synchronize();
	dropGraphsAndRebuild();
	if (m_UseGraph) {
		// One eager pass FIRST: the per-layer tower kernels have never been launched on
		// this device, and their first launch sets the dynamic-LDS attribute
		// (hipFuncSetAttribute) -- not something to do inside a stream capture; launch
		// errors also surface here.  Only the CURRENT binding set's program, on the staging
		// buffers: it writes scratch tensors and the OUTPUT half of the state ping-pong,
		// which the caller's re-run overwrites; the other set's program (same kernels,
		// other pointers) would overwrite the INPUT half the re-run still needs.
		AtExit restore{[this, keep = m_IO] { m_IO = keep; }};
		bindStaging();
		for (const Step &st : m_Program[m_Idx]) st.run(m_Stream);
		m_Stream.synchronize();
		captureFrameGraphs();
		m_Stream.synchronize();
	}
}

void Engine::zeroResidentMailboxes() {
	for (const ResidentTower *t : {&m_GenTower, &m_FlowTower}) {
		t->mail.zeroAsync(m_Stream);
		t->flags.zeroAsync(m_Stream);
	}
}

// the graphs of the staging buffers go, and both programs are written again for the towers now in use
void Engine::dropGraphsAndRebuild() {
	for (int s = 0; s < 2; ++s) {
		m_Graph[s] = GraphExec();
		buildProgram(s);
	}
}

// Back to the one-launch tower after enough clean frames on the fallback path.
void Engine::restoreResident() {
	m_Stream.synchronize();
	m_Resident = true;
	m_ResidentFlow = m_ResidentFlowCapable;
	m_CleanFrames = 0;
	dropAllGraphs();
	zeroResidentMailboxes();
	dropGraphsAndRebuild();
	if (m_UseGraph) {  // (the resident kernels ran before: nothing sets an attribute inside the capture)
		AtExit restore{[this, keep = m_IO] { m_IO = keep; }};
		bindStaging();
		captureFrameGraphs();
	}
	m_Stream.synchronize();
	logMessage(LogLevel::Info, "Engine", "trying the resident tower kernel again");
}

void Engine::maybeRestoreResident() {
	if (!m_Resident && m_ResidentCapable && m_RetryAfter != 0 && ++m_CleanFrames >= m_RetryAfter) {
		restoreResident();
	}
}

void Engine::reset() {
	DeviceGuard g(m_Device);
	if (m_Config.recurrent()) {  // (a flow-free model has no state: nothing to zero)
		for (int i = 0; i < 2; ++i) {
			m_State[i].zeroAsync(m_Stream);
			m_Packed[i].zeroAsync(m_Stream);
		}
	}
	m_Stream.synchronize();
	m_Idx = 0;
	m_Scene.restart();  // the scene detector has no predecessor after a reset; its setting and its step count stay
}

FrameSize Engine::frameSize() const {
	const auto w = static_cast<std::size_t>(m_Config.frameWidth);
	const auto h = static_cast<std::size_t>(m_Config.frameHeight);
	return {w, h, w * 4, h * 4};
}

bool Engine::directEligible(const Frame &in, const Frame &out) const {
	const FrameSize fs = frameSize();
	const auto inRow = static_cast<std::ptrdiff_t>(fs.inputWidth * 4);
	const auto outRow = static_cast<std::ptrdiff_t>(fs.outputWidth * 4);
	return m_PreferDirect && in.location == Location::Device && out.location == Location::Device &&
	       in.ptr != nullptr && out.ptr != nullptr && in.width == fs.inputWidth && in.height == fs.inputHeight &&
	       out.width == fs.outputWidth && out.height == fs.outputHeight &&
	       (in.stride >= inRow || -in.stride >= inRow) && (out.stride >= outRow || -out.stride >= outRow) &&
	       (reinterpret_cast<std::uintptr_t>(in.ptr) % 4 == 0) && in.stride % 4 == 0 &&
	       (reinterpret_cast<std::uintptr_t>(out.ptr) % 8 == 0) && out.stride % 8 == 0;
}

void Engine::replayOrRun(CachedGraph &e, bool registered, const std::function<void()> &launches) {
	// a registered unit whose graph was dropped (fallback / return to the resident kernel) is captured again at once;
	// an unknown tuple at its second sighting -- a caller that hands over a fresh pointer every frame never pays a
	// capture, and a pass's first sighting, eager, also sets the dynamic-LDS attribute of a tile height its launch
	// sizes choose for the first time, which must not happen inside a capture
	if (!e.graph.valid() && (++e.seen >= 2 || registered)) {
		e.graph = GraphExec::capture(m_Stream, launches);  // records the launches (nothing executes here) ...
		++m_InlineCaptures;
	}
	if (e.graph.valid()) {  // ... and replay
		e.graph.launch(m_Stream);
		++m_GraphReplays;
		return;
	}
	launches();
	++m_EagerRuns;
}

int Engine::prepareGraph(CachedGraph &e, const std::function<void()> &launches) {
	if (e.graph.valid()) return 0;
	e.graph = GraphExec::capture(m_Stream, launches);
	++m_PreparedCaptures;
	return 1;
}

void Engine::dropAllGraphs() {
	m_DirectGraphs.dropGraphs();  // (the registered pairs stay registered)
	m_BatchGraphs.clear();
}

int Engine::prepareFrames(const Frame &in, const Frame &out) {
	DeviceGuard g(m_Device);
	const FrameSize fs = frameSize();
	if (sourceStage() || m_AlphaMode != 0) {  // every frame goes through the staging buffers, whose graphs exist
		checkFrame(anyOf(in), true);
		checkFrame(anyOf(out), false);
		return 0;
	}
	if (in.location != Location::GraphicsResource &&
	    (in.ptr == nullptr || in.width != fs.inputWidth || in.height != fs.inputHeight)) {
		throw std::invalid_argument("prepareFrames: input image must be exactly " + std::to_string(fs.inputWidth) + "x" +
		                            std::to_string(fs.inputHeight));
	}
	if (out.location != Location::GraphicsResource &&
	    (out.ptr == nullptr || out.width != fs.outputWidth || out.height != fs.outputHeight)) {
		throw std::invalid_argument("prepareFrames: output image must be exactly " + std::to_string(fs.outputWidth) +
		                            "x" + std::to_string(fs.outputHeight));
	}
	if (!directEligible(in, out) || !m_UseGraph || !m_DirectGraph) return 0;  // staged frames: graphs exist already
	DirectKey key{in.ptr, in.stride, out.ptr, out.stride, 0};
	m_DirectGraphs.registerUnit(key);
	std::unique_lock<std::mutex> chain = chainBegin(m_Resident);  // (no capture while another engine's constructor drains the device)
	AtExit restore{[this, keep = m_IO] { m_IO = keep; }};
	m_IO.in = static_cast<const std::uint8_t *>(in.ptr);
	m_IO.inStride = in.stride;
	m_IO.out = static_cast<std::uint8_t *>(out.ptr);
	m_IO.outStride = out.stride;
	int captured = 0;
	for (key.idx = 0; key.idx < 2; ++key.idx) {
		captured += prepareGraph(m_DirectGraphs.use(key), [this, idx = key.idx] { runSteps(idx); });
	}
	return captured;
}

// Binding set idx's launches against m_IO, in stream order (recorded when m_Stream is capturing).
// ONE graph per frame: replaying the first launches as a graph of their own, so that the GPU
// starts while the CPU still submits the rest, was measured and lost 0.5-0.8 % (1943-1947 against
// 1926-1933 frames/s, tools/submit_overhead.py): hipGraphLaunch already streams its packets, and
// the second graph costs a boundary
void Engine::runSteps(int idx) {
	for (const Step &st : m_Program[idx]) st.run(m_Stream);
}

void Engine::runProgram() {
	if (m_UseGraph && !m_DirectIO && m_Graph[m_Idx].valid()) {
		m_Graph[m_Idx].launch(m_Stream);
		++m_GraphReplays;
		return;
	}
	if (m_UseGraph && m_DirectIO && m_DirectGraph) {
		const DirectKey key{m_IO.in, m_IO.inStride, m_IO.out, m_IO.outStride, m_Idx};
		return replayOrRun(m_DirectGraphs.use(key), m_DirectGraphs.registered(key), [this] { runSteps(m_Idx); });
	}
	runSteps(m_Idx);
	++m_EagerRuns;
}

void Engine::bindStaging() {
	const FrameSize fs = frameSize();
	m_IO.in = m_InStage.as<std::uint8_t>();
	m_IO.inStride = static_cast<std::ptrdiff_t>(fs.inputWidth) * 4;
	m_IO.out = m_OutStage.as<std::uint8_t>();
	m_IO.outStride = static_cast<std::ptrdiff_t>(fs.outputWidth) * 4;
}

void Engine::submit(const Frame &in, const Frame &out) {
	// Device-resident frames: the kernels read the caller's input and write the caller's
	// output directly (any signed stride), no staging copies.
	m_DirectIO = directEligible(in, out);
	// The per-device chain lock covers the wait on the previous resident frame, the program's launches
	// (and an inline graph capture) and the completion record -- NOT the staging copies: a pageable
	// host-to-device copy blocks its caller, and would block every other runtime of the device with it
	// (advisor, round 3).  They are ordered by the stream; a copy kernel beside another runtime's
	// resident tower merely waits for a free CU or delays a workgroup's start by microseconds.
	if (m_DirectIO) {
		m_IO.in = static_cast<const std::uint8_t *>(in.ptr);
		m_IO.inStride = in.stride;
		m_IO.out = static_cast<std::uint8_t *>(out.ptr);
		m_IO.outStride = out.stride;
	} else {
		bindStaging();
		stageIn(in);
		// With the scene detector on, what stageOut would refuse behind the step is refused here, in front of the
		// detector: a refused frame must not reach it (it would overwrite the kept frame, count a step and, at a cut,
		// clear the inputs of a step that then does not happen).  Off: as ju_process always behaved.  (A graphics
		// resource's own extent is known only when it is mapped, in stageOut.)
		if (m_Scene.mode() != 0) checkFrame(anyOf(out), false, "processImage");
	}
	sceneStep();
	{
		std::unique_lock<std::mutex> chain = chainBegin(m_Resident);
		runProgram();
		chainEnd(chain, m_Resident);
	}
	if (!m_DirectIO) {
		const FrameSize fs = frameSize();
		stageOut(out, fs.outputWidth, fs.outputHeight, m_OutStage.as<std::uint8_t>(), m_RawStage.as<std::uint8_t>());
	}
	m_Idx ^= 1;  // state ping-pong (tensorrt_backend.cc:277)
}

void Engine::submitAny(const AnyFrame &in, const AnyFrame &out) {
	if (staged(in, out)) {
		submitFrame(in, out);
	} else {
		submit(in.bgrx, out.bgrx);
	}
}

void Engine::enqueue(const AnyFrame &in, const AnyFrame &out) {
	DeviceGuard g(m_Device);
	checkPair(in, out);
	submitAny(in, out);
}

namespace {
std::atomic<int> g_StepRerun{0};
}  // namespace
void setStepRerun(int on) { g_StepRerun = on; }

void Engine::runSynchronous(const AnyFrame &in, const AnyFrame &out) {
	const std::uint64_t alphaFrames = m_AlphaFrames;
	submitAny(in, out);
	m_Stream.synchronizeSpin(m_SpinUs);
	const unsigned code = takeResidentError();
	if (code || g_StepRerun.load(std::memory_order_relaxed)) {
		// the frame's inputs (previous state, frame history) are intact: the step only
		// wrote the other half of the ping-pong -- run it again on the per-layer path
		// (submit() flipped m_Idx; the re-run needs the same binding set again.  If the
		// fallback or the re-run throws, the failed frame must not count as a step either.)
		m_Idx ^= 1;
		if (sourceStage()) --m_SourceFrames;  // (submitFrame counts the frame again)
		m_AlphaFrames = alphaFrames;
		if (code) fallbackToLayers(code);  // (else the debug switch: the frame was sound)
		// the scene detector ran with the first submission: its decision stands, the kept frame is this frame already
		// and, after a cut, the cleared inputs are still in place (the step wrote the other half only)
		m_SceneRerun = true;
		try {
			submitAny(in, out);
		} catch (...) {
			m_SceneRerun = false;
			throw;
		}
		m_SceneRerun = false;
		m_Stream.synchronize();
	} else {
		maybeRestoreResident();
	}
}

void Engine::process(const AnyFrame &in, const AnyFrame &out) {
	DeviceGuard g(m_Device);
	checkPair(in, out);
	runSynchronous(in, out);
}

void Engine::synchronize() {
	DeviceGuard g(m_Device);
	m_Stream.synchronize();
	if (const unsigned code = takeResidentError()) {
		fallbackToLayers(code);
		throw std::runtime_error(
		    "resident tower kernel failed (workgroups not co-resident); the frames enqueued since "
		    "the last ju_synchronize are invalid. The runtime now uses the per-layer path: "
		    "ju_reset and continue");
	}
}

std::vector<std::string> Engine::tensorNames() const {
	std::vector<std::string> names = {"trunk"};
	if (m_Config.recurrent()) names.insert(names.begin(), {"state", "flow_in"});
	for (const auto &kv : m_Tensors) names.push_back(kv.first);
	return names;
}

std::size_t Engine::readTensor(const std::string &name, float *dst, std::size_t capacity) {
	DeviceGuard g(m_Device);
	const void *src = nullptr;
	std::size_t count = 0;
	bool f32 = false;
	const Tensor *tw = nullptr;
	DType dt = m_DType;
	const std::size_t lr = static_cast<std::size_t>(m_Config.frameHeight) * m_Config.frameWidth;
	if (!m_Config.recurrent() && (name == "state" || name == "flow_in")) {
		throw std::invalid_argument("unknown tensor " + name + " (a flow-free model has no recurrent state)");
	}
	if (name == "state") {  // the state the NEXT frame will read = last output_raw
		src = m_State[m_Idx].get();
		count = lr * 16 * 4;
		dt = kF16;
	} else if (name == "flow_in") {
		src = m_Packed[m_Idx].get();
		count = static_cast<std::size_t>(m_Config.paddedHeight()) * m_Config.paddedWidth() * 16;
	} else {
		const std::string key = name == "trunk" ? m_TrunkOut : name;
		auto it = m_Tensors.find(key);
		if (it == m_Tensors.end()) throw std::invalid_argument("unknown tensor " + name);
		src = it->second.buf.get();
		count = it->second.count;
		f32 = it->second.isF32;
		if (it->second.isState) dt = kF16;
		if (it->second.towerC) tw = &it->second;
	}
	const std::size_t outCount =
	    tw ? static_cast<std::size_t>(tw->towerH) * tw->towerW * tw->towerC : count;
	if (dst == nullptr) return outCount;
	if (capacity < outCount) throw std::invalid_argument("readTensor: buffer too small");
	m_Stream.synchronize();
	if (f32) {
		JU_HIP(hipMemcpy(dst, src, count * 4, hipMemcpyDeviceToHost));
	} else {
		DeviceBuffer tmp(count * 4);
		launchToFloat(dt, src, tmp.as<float>(), count, m_Stream);
		m_Stream.synchronize();
		if (tw) {  // strip the zero border of the tower layout: dense [H][W][C] out
			const std::size_t rowElems = static_cast<std::size_t>(tw->towerW) * tw->towerC;
			JU_HIP(hipMemcpy2D(dst, rowElems * 4,
			    tmp.as<float>() + towerOrigin(tw->towerW) * tw->towerC,
			    static_cast<std::size_t>(towerPitch(tw->towerW)) * tw->towerC * 4, rowElems * 4,
			    tw->towerH, hipMemcpyDeviceToHost));
		} else {
			JU_HIP(hipMemcpy(dst, tmp.get(), count * 4, hipMemcpyDeviceToHost));
		}
	}
	return outCount;
}

// What flopsOf and timeSteps are asked for: "<tag>[#k][@frame|@pass]".
// "flow#3" = only the 4th step tagged "flow" (per-layer timing); "tower@frame" = the steps
// tagged "tower" timed INSIDE whole frames (every step of the frame runs, events bracket the
// tagged launches): the kernel in the clock / cache context of the real workload, which is
// what a kernel trace of the benchmark averages -- back-to-back launches of the tower alone
// draw more power and read 4-5 % slower on the same box
// "tower@pass" = the same inside look-ahead passes of JU_LOOKAHEAD frames (processBatch): there the towers of
// consecutive frames follow one another with only the warp in between; "flow@pass": the pass's flow launches
// (each covers all frames of the pass)
struct Engine::StepSpec {
	std::string tag;
	int only = -1;
	bool inFrame = false, inPass = false;
	explicit StepSpec(std::string spec) {
		std::size_t at = spec.find("@frame");
		if (at != std::string::npos) {
			inFrame = true;
		} else if ((at = spec.find("@pass")) != std::string::npos) {
			inPass = true;
		}
		if (at != std::string::npos) spec = spec.substr(0, at);
		const std::size_t hash = spec.find('#');
		tag = spec.substr(0, hash);
		if (hash != std::string::npos) only = std::atoi(spec.c_str() + hash + 1);
	}
	// the steps of `prog` it names, in order
	std::vector<const Step *> of(const std::vector<Step> &prog) const {
		std::vector<const Step *> steps;
		int k = 0;
		for (const Step &s : prog) {
			if (tag.empty() || s.tag == tag) {
				if (only < 0 || k == only) steps.push_back(&s);
				++k;
			}
		}
		return steps;
	}
};

double Engine::flopsOf(const std::string &tagSpec) const {
	const StepSpec spec(tagSpec);
	// ("flow@pass": the pass's flow launches, each over all its frames -- once timeSteps has planned them)
	const auto passFlow = m_BatchFlow.find({m_BatchMax, 0});
	const bool inPassFlow = spec.inPass && spec.tag == "flow" && passFlow != m_BatchFlow.end();
	double f = 0.0;
	for (const Step *s : spec.of(inPassFlow ? passFlow->second : m_Program[0])) f += s->flops;
	return f;
}

namespace {
// the mean of `count` intervals, each between an event and the one recorded after it
double meanOfPairs(const std::vector<std::unique_ptr<Event>> &ev, double count) {
	double sum = 0.0;
	for (std::size_t i = 0; i + 1 < ev.size(); i += 2) sum += static_cast<double>(Event::elapsedMs(*ev[i], *ev[i + 1]));
	return ev.empty() ? 0.0 : sum / count;
}
}  // namespace

double Engine::timeSteps(const std::string &tagSpec, int iters, int *launches) {
	DeviceGuard g(m_Device);
	const StepSpec spec(tagSpec);
	const bool inFrame = spec.inFrame, inPass = spec.inPass;
	if (inPass && (m_BatchMax < 2 || !batchPlanned(m_BatchMax))) throw std::invalid_argument("timeSteps: this model has no look-ahead passes");
	const bool passFlow = inPass && spec.tag == "flow";
	const std::vector<const Step *> steps = spec.of(passFlow ? m_BatchFlow.at({m_BatchMax, m_Idx}) : m_Program[m_Idx]);
	if (launches) *launches = static_cast<int>(steps.size());
	if (steps.empty() || iters <= 0) return 0.0;
	bindStaging();
	double ms = 0.0;
	std::unique_lock<std::mutex> chain = chainBegin(m_Resident);  // (the timed launches may be resident towers)
	if (inPass) {
		const int n = m_BatchMax, set = m_Idx;
		m_PassStage = 0;  // (a plain pass, whatever the pass bound last carried: nothing of it is left to launch on)
		for (int i = 0; i < n; ++i) {  // (every frame of the pass on the staging buffers)
			m_Pass[i] = PassFrame{};
			m_Pass[i].io = m_Pass[i].ends = m_IO;
		}
		std::vector<std::unique_ptr<Event>> ev;
		const std::function<void(const Step &, bool)> around = [&](const Step &s, bool) {
			if (std::find(steps.begin(), steps.end(), &s) == steps.end()) return;
			ev.emplace_back(new Event());
			ev.back()->record(m_Stream);
		};
		runBatch(set, n);  // warm
		for (int i = 0; i < iters; ++i) runBatch(set, n, &around);
		chainEnd(chain, m_Resident);
		m_Stream.synchronize();
		ms = meanOfPairs(ev, static_cast<double>(ev.size()) / 2);
	} else if (inFrame) {
		auto isTimed = [&](const Step *s) { return std::find(steps.begin(), steps.end(), s) != steps.end(); };
		for (const Step &s : m_Program[m_Idx]) s.run(m_Stream);  // warm
		std::vector<std::unique_ptr<Event>> ev;
		for (int i = 0; i < iters; ++i) {
			for (const Step &s : m_Program[m_Idx]) {
				const bool timed = isTimed(&s);
				if (timed) {
					ev.emplace_back(new Event());
					ev.back()->record(m_Stream);
				}
				s.run(m_Stream);
				if (timed) {
					ev.emplace_back(new Event());
					ev.back()->record(m_Stream);
				}
			}
		}
		chainEnd(chain, m_Resident);
		m_Stream.synchronize();
		ms = meanOfPairs(ev, static_cast<double>(iters) * steps.size());
	} else {
		for (const Step *s : steps) s->run(m_Stream);  // warm
		Event t0, t1;
		t0.record(m_Stream);
		for (int i = 0; i < iters; ++i) {
			for (const Step *s : steps) s->run(m_Stream);
		}
		t1.record(m_Stream);
		chainEnd(chain, m_Resident);
		t1.synchronize();
		ms = static_cast<double>(Event::elapsedMs(t0, t1)) / (static_cast<double>(iters) * steps.size());
	}
	// The timed launches ran outside the frame sequence: scratch tensors, the output
	// staging buffer and (with JU_TAIL=tower) the recurrent state were overwritten.  Start
	// the stream from a clean state again, and do not leave a bounded-wait failure of the
	// resident tower behind for the next process() to trip over.
	const unsigned code = takeResidentError();
	if (code) fallbackToLayers(code);  // (also zeroes the mailboxes: the aborted launch left the slot epochs out of step)
	reset();
	if (code) {
		std::ostringstream ss;
		ss << "timeSteps: the resident tower kernel reported a bounded-wait timeout (code 0x" << std::hex
		   << code << "); the timing is invalid";
		throw std::runtime_error(ss.str());
	}
	return ms;
}

double Engine::stat(const std::string &key) const {
	if (key == "graph_replays") return static_cast<double>(m_GraphReplays);
	if (key == "eager_runs") return static_cast<double>(m_EagerRuns);
	if (key == "graph_captures") return static_cast<double>(m_InlineCaptures);
	if (key == "prepared_captures") return static_cast<double>(m_PreparedCaptures);
	if (key == "registered_pairs") return static_cast<double>(m_DirectGraphs.registeredUnits());
	if (key == "recurrent") return m_Config.recurrent() ? 1.0 : 0.0;  // 0: a flow-free model (stateless)
	if (key == "output_select") return static_cast<double>(m_Config.outputSelect);  // 1: the output_flow variant (pre_warp)
	if (key == "resident_tower") return m_Resident ? 1.0 : 0.0;
	if (key == "resident_flow") return m_ResidentFlow ? 1.0 : 0.0;
	if (key == "tower_fast") {  // the generator's resident tower runs the fast schedule (16-bit models, every region of its shape)
		return (m_Resident && !m_Fp8Tower && residentTowerFast() && !m_Calibrate &&
		        residentTowerFastGeometry(m_Config.frameHeight, m_Config.frameWidth, m_GenTower.GX, m_GenTower.GY, m_GenTower.RH)) ? 1.0 : 0.0;
	}
	if (key == "tower_unit_rows") {  // rows of the resident tower's work unit: 4 = the fast schedule's row-quad form (ReLU towers), else 2
		const bool fast = stat("tower_fast") != 0.0;
		return (fast && m_Config.genActivation != 1) ? static_cast<double>(residentTowerUnitRows(m_Config.frameHeight, m_Config.frameWidth, m_GenTower.GX, m_GenTower.GY, m_GenTower.RH)) : 2.0;
	}
	if (key == "fallbacks") return static_cast<double>(m_Fallbacks);
	if (key == "lookahead_frames") return static_cast<double>(m_BatchFrames);  // frames that went through look-ahead passes
	if (key == "lookahead_host_frames") return static_cast<double>(m_BatchHostFrames);  // ... of them with a host image
	if (key == "hbd_from_state") return m_HbdFromState ? 1.0 : 0.0;  // 10-bit outputs: from the f16 state (1) / the u8 frame (0)
	if (key == "lookahead_yuv_frames") return static_cast<double>(m_BatchYuvFrames);  // ... of them with a YUV side
	if (key == "lookahead_max") return static_cast<double>(m_BatchMax);
	if (key == "source_scaled") return m_SrcScale.set() ? 1.0 : 0.0;
	if (key == "output_scaled") return m_OutScale.set() ? 1.0 : 0.0;
	if (key == "source_filter") return static_cast<double>(m_SrcScale.filter());  // (0 while off: the setters clear it)
	if (key == "output_filter") return static_cast<double>(m_OutScale.filter());
	if (key == "source_mask") return m_Mask.on() ? 1.0 : 0.0;
	if (key == "alpha_mode") return static_cast<double>(m_AlphaMode);
	if (key == "alpha_filter") return static_cast<double>(m_AlphaFilter);
	if (key == "alpha_frames") return static_cast<double>(m_AlphaFrames);  // frames whose alpha slot the alpha kernels wrote
	if (key == "alpha_lookahead") return m_AlphaLookahead ? 1.0 : 0.0;
	if (key == "alpha_group") return m_AlphaGroup ? 1.0 : 0.0;
	if (key == "lookahead_alpha_frames") return static_cast<double>(m_BatchAlphaFrames);  // ... of them inside look-ahead passes
	if (key == "group_alpha_frames") return static_cast<double>(m_GroupAlphaFrames);  // ... of them inside group passes
	if (key == "source_stage_frames") return static_cast<double>(m_SourceFrames);  // frames through the source stage
	if (key == "group_frames") return static_cast<double>(m_GroupFrames);  // frames that went through group passes
	if (key == "group_yuv_frames") return static_cast<double>(m_GroupYuvFrames);  // ... of them with a non-BGRX side
	if (key == "scene_group") return m_SceneGroup ? 1.0 : 0.0;
	if (key == "scene_group_frames") return static_cast<double>(m_SceneGroupFrames);  // detector steps taken inside group passes
	if (key == "scene_mode") return static_cast<double>(m_Scene.mode());
	if (key == "scene_lookahead") return m_SceneLookahead ? 1.0 : 0.0;
	if (key == "scene_pass_frames") return static_cast<double>(m_ScenePassFrames);
	if (key == "stage_lookahead") return m_StageLookahead ? 1.0 : 0.0;
	if (key == "lookahead_staged_frames") return static_cast<double>(m_BatchStagedFrames);  // ... of them under a stage setting
	if (key == "stage_group") return m_StageGroup ? 1.0 : 0.0;
	if (key == "group_staged_frames") return static_cast<double>(m_GroupStagedFrames);  // group-pass frames under a stage setting
	// (the detector's own counters, as of the steps that have completed: the decision writes them to host-mapped memory)
	if (key == "scene_frames" || key == "scene_cuts") return static_cast<double>(m_Scene.total(key == "scene_cuts"));
	if (key == "scene_detector_runs") return static_cast<double>(m_SceneRuns);  // launches of the detector (tests: once per step)
	if (key == "launches_per_frame") return static_cast<double>(m_Program[0].size());
	if (key == "tower_variant") return static_cast<double>(towerVariant());  // (developer switch, tests)
	if (key == "direct_graphs") return static_cast<double>(m_DirectGraphs.validGraphs());
	throw std::invalid_argument("unknown stat " + key);
}

}  // namespace ju
