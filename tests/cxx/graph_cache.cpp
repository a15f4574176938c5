// ju::GraphCache (joshupscale_amd/csrc/graph_cache.h) alone, on the host (tests/test_cxx_graph_cache.py builds this with
// -fsanitize=address,undefined and compares what it prints with a model of the policy written there).  Both of the
// engine's instantiations over one use clock, with a graph that counts its lives: `p` the frame pairs (key: in out idx;
// the unit is the key with idx = 0), `t` the pass tuples (key: n frames of id stage scene; the unit is the key).
// Arguments: maxUnregistered maxRegistered, of both caches.  Standard input: a script of operations --
//   p u <in> <out> <idx>    use(key), one more sighting          t u <n> <id stage scene>...
//   p c <in> <out> <idx>    use(key), and a graph captured unless there is one   t c <n> ...
//   p r <in> <out>          registerUnit                          t r <n> ...
//   p d / t d               dropGraphs()
//   p x / t x               clear()
//   t L <cap>               eraseIf(longer than cap)      t S   eraseIf(front().stage != 0)      t N   eraseIf(front().scene != 0)
// After every operation one line: the cache's entries in key order as key g<graph there> s<seen> u<lastUse>, its
// registered units, validGraphs() and registeredUnits(), graphs made and destroyed so far.  At the end, with both caches
// gone: every graph made was destroyed exactly once and none is alive, or the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "graph_cache.h"

namespace {

int g_Made = 0, g_Destroyed = 0, g_Twice = 0;
std::set<int> g_Alive;

struct FakeGraph {  // move-only, as GraphExec is
	int id = 0;
	FakeGraph() = default;
	static FakeGraph capture() {
		FakeGraph g;
		g.id = ++g_Made;
		g_Alive.insert(g.id);
		return g;
	}
	FakeGraph(const FakeGraph &) = delete;
	FakeGraph &operator=(const FakeGraph &) = delete;
	FakeGraph(FakeGraph &&o) noexcept : id(o.id) { o.id = 0; }
	FakeGraph &operator=(FakeGraph &&o) noexcept {
		if (this != &o) {
			reset();
			id = o.id;
			o.id = 0;
		}
		return *this;
	}
	~FakeGraph() { reset(); }
	void reset() {
		if (id == 0) return;
		if (g_Alive.erase(id) == 0) ++g_Twice;
		++g_Destroyed;
		id = 0;
	}
	bool valid() const { return id != 0; }
};

struct PairKey {
	int in, out, idx;
	bool operator<(const PairKey &o) const { return std::tie(in, out, idx) < std::tie(o.in, o.out, o.idx); }
};
struct PairOf {
	PairKey operator()(PairKey key) const {
		key.idx = 0;
		return key;
	}
};
struct FrameKey {
	int id, stage, scene;
	bool operator<(const FrameKey &o) const { return std::tie(id, stage, scene) < std::tie(o.id, o.stage, o.scene); }
};
using TupleKey = std::vector<FrameKey>;

std::string text(const PairKey &k) {
	return "(" + std::to_string(k.in) + "," + std::to_string(k.out) + "," + std::to_string(k.idx) + ")";
}
std::string text(const TupleKey &k) {
	std::string s = "<";
	for (const FrameKey &f : k) s += std::to_string(f.id) + "." + std::to_string(f.stage) + "." + std::to_string(f.scene) + ";";
	return s + ">";
}

int number() {
	int v = 0;
	if (std::scanf("%d", &v) != 1) std::exit(2);
	return v;
}
void read(PairKey *k, bool unit) {
	k->in = number();
	k->out = number();
	k->idx = unit ? 0 : number();
}
void read(TupleKey *k, bool) {
	const int n = number();
	k->clear();
	for (int i = 0; i < n; ++i) {
		FrameKey f{};
		f.id = number(), f.stage = number(), f.scene = number();
		k->push_back(f);
	}
}

template <typename Cache>
void show(char name, const Cache &c) {
	std::printf("%c entries:", name);
	for (const auto &kv : c.entries()) {
		std::printf(" %s g%d s%u u%llu", text(kv.first).c_str(), kv.second.graph.valid() ? 1 : 0, kv.second.seen,
		    static_cast<unsigned long long>(kv.second.lastUse));
	}
	std::printf(" units:");
	for (const auto &u : c.units()) std::printf(" %s", text(u).c_str());
	std::printf(" valid=%zu registered=%zu made=%d destroyed=%d\n", c.validGraphs(), c.registeredUnits(), g_Made, g_Destroyed);
}

// the operations both caches share; false: not one of them
template <typename Cache, typename Key>
bool common(Cache &c, char op, Key *key) {
	if (op == 'u' || op == 'c') {
		read(key, false);
		auto &e = c.use(*key);
		++e.seen;
		if (op == 'c' && !e.graph.valid()) e.graph = FakeGraph::capture();
	} else if (op == 'r') {
		read(key, true);
		c.registerUnit(*key);
	} else if (op == 'd') {
		c.dropGraphs();
	} else if (op == 'x') {
		c.clear();
	} else {
		return false;
	}
	return true;
}

}  // namespace

int main(int argc, char **argv) {
	if (argc != 3) return 2;
	const std::size_t maxUnregistered = std::strtoul(argv[1], nullptr, 10), maxRegistered = std::strtoul(argv[2], nullptr, 10);
	{
		std::uint64_t clock = 0;
		ju::GraphCache<PairKey, FakeGraph, PairOf> pairs(clock, maxUnregistered, maxRegistered);
		ju::GraphCache<TupleKey, FakeGraph, ju::UnitIsKey> tuples(clock, maxUnregistered, maxRegistered);
		char which, op;
		while (std::scanf(" %c %c", &which, &op) == 2) {
			if (which == 'p') {
				PairKey key{};
				if (!common(pairs, op, &key)) return 2;
				show('p', pairs);
			} else if (which == 't') {
				TupleKey key;
				if (common(tuples, op, &key)) {
				} else if (op == 'L') {
					const int cap = number();
					tuples.eraseIf([cap](const TupleKey &k) { return static_cast<int>(k.size()) > cap; });
				} else if (op == 'S') {
					tuples.eraseIf([](const TupleKey &k) { return !k.empty() && k.front().stage != 0; });
				} else if (op == 'N') {
					tuples.eraseIf([](const TupleKey &k) { return !k.empty() && k.front().scene != 0; });
				} else {
					return 2;
				}
				show('t', tuples);
			} else {
				return 2;
			}
		}
	}
	std::printf("end made=%d destroyed=%d alive=%zu twice=%d\n", g_Made, g_Destroyed, g_Alive.size(), g_Twice);
	if (g_Made != g_Destroyed || !g_Alive.empty() || g_Twice != 0) return 3;
	std::printf("graph_cache ok\n");
	return 0;
}
