// dev_switch.h: compiled once per library flavour (Makefile).  Without JU_TEST_HOOKS -- libJoshUpscale.so -- no developer
// switch exists: no name, no getenv.
#include "dev_switch.h"

#ifdef JU_TEST_HOOKS
#include <cstddef>
#include <cstdlib>
#endif

namespace ju {

#ifdef JU_TEST_HOOKS
const char *devSwitch(Dev which) {
	// (in the order of the enum; an array without a stated size, so that a switch added to one of the two and not to
	// the other does not compile)
	static const char *const kNames[] = {
	    "JU_TAIL", "JU_PACK", "JU_POOL", "JU_UPSAMPLE", "JU_FLOW_CONV", "JU_TOWER", "JU_CALIBRATE", "JU_FLOW", "JU_DIRECT",
	    "JU_DIRECT_GRAPH", "JU_SYNC_SPIN_US", "JU_TRACE_STEPS", "JU_TRACE_NOSYNC", "JU_RES_BLOCK", "JU_FLOW_TILE",
	    "JU_FLOW_WIDE", "JU_WAVE_PRIO", "JU_CONV_DBUF", "JU_TOWER_FAST", "JU_FP8_GRID", "JU_FP8_BLOCK", "JU_SPLITK_PLAN",
	    "JU_CONV_TILE",
	};
	static_assert(sizeof(kNames) / sizeof(kNames[0]) == static_cast<std::size_t>(Dev::Count),
	    "kNames must name every switch of Dev, in its order");
	const int i = static_cast<int>(which);
	if (i < 0 || i >= static_cast<int>(Dev::Count)) return nullptr;
	return std::getenv(kNames[i]);
}
bool devSwitchesExist() {
	return true;
}
#else
const char *devSwitch(Dev) {
	return nullptr;
}
bool devSwitchesExist() {
	return false;
}
#endif

}  // namespace ju
