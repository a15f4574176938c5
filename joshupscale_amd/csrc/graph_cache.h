// The cache of captured graphs: which graph a call replays, which ones stay, which ones go.  One definition for the
// engine's two caches -- the per-frame graphs of device frame pairs and the graphs of look-ahead passes (engine.h) -- over
// one use clock.  Plain C++: no HIP (tests/cxx/graph_cache.cpp instantiates it with a graph that counts its lives).
//
// A key names everything a graph bakes in.  unitOf(key) names what a caller registers: a frame PAIR stands for the graphs
// of both binding sets (the key with idx = 0), a pass tuple for itself.  Entries of registered units are exempt from the
// least-recently-used eviction and are captured at their first sighting (Engine::replayOrRun); the registered units have
// a cap of their own, under which the unit whose graphs were used least recently goes with all of them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <set>

namespace ju {

template <typename Graph>
struct GraphEntry {
	Graph graph;
	unsigned seen = 0;  // sightings so far without a graph (the caller counts: first eager, second captured)
	std::uint64_t lastUse = 0;
};

template <typename Key, typename Graph, typename UnitOf>
class GraphCache {
public:
	using Entry = GraphEntry<Graph>;

	// clock: the use clock, shared by every cache that holds it; maxUnregistered: entries of units nobody registered
	// (least recently used out); maxRegistered: registered units
	GraphCache(std::uint64_t &clock, std::size_t maxUnregistered, std::size_t maxRegistered)
	    : m_Clock(clock), m_MaxUnregistered(maxUnregistered), m_MaxRegistered(maxRegistered) {}

	// The entry of `key`, made if need be, stamped with the clock.  A new entry -- whatever its own unit -- first evicts
	// the least recently used entry of an unregistered unit (ties: the first in key order) while maxUnregistered of
	// those exist; it never evicts a registered unit's.
	Entry &use(const Key &key) {
		auto it = m_Entries.find(key);
		if (it == m_Entries.end()) {
			if (m_Entries.size() >= m_MaxUnregistered) {
				std::size_t unregistered = 0;
				auto victim = m_Entries.end();
				for (auto j = m_Entries.begin(); j != m_Entries.end(); ++j) {
					if (registered(j->first)) continue;
					++unregistered;
					if (victim == m_Entries.end() || j->second.lastUse < victim->second.lastUse) victim = j;
				}
				if (unregistered >= m_MaxUnregistered && victim != m_Entries.end()) m_Entries.erase(victim);
			}
			it = m_Entries.try_emplace(key).first;
		}
		it->second.lastUse = ++m_Clock;
		return it->second;
	}

	bool registered(const Key &key) const { return m_Registered.count(m_UnitOf(key)) != 0; }

	// A caller that keeps registering new units and never the old ones again: at the cap the unit whose entries were
	// used least recently is forgotten with all of them -- a unit's recency is its entries' latest use, 0 without
	// entries; ties: the first in key order.
	void registerUnit(const Key &unit) {
		if (m_Registered.count(unit)) return;
		if (!m_Registered.empty() && m_Registered.size() >= m_MaxRegistered) {
			std::map<const Key *, std::uint64_t> used;
			for (const auto &kv : m_Entries) {
				auto r = m_Registered.find(m_UnitOf(kv.first));
				if (r == m_Registered.end()) continue;
				std::uint64_t &u = used[&*r];
				if (kv.second.lastUse > u) u = kv.second.lastUse;
			}
			auto victim = m_Registered.begin();
			std::uint64_t oldest = ~std::uint64_t(0);
			for (auto it = m_Registered.begin(); it != m_Registered.end(); ++it) {
				auto u = used.find(&*it);
				const std::uint64_t recency = u == used.end() ? 0 : u->second;
				if (recency < oldest) {
					oldest = recency;
					victim = it;
				}
			}
			for (auto it = m_Entries.begin(); it != m_Entries.end();) {
				const auto &unitOfEntry = m_UnitOf(it->first);
				const bool ofVictim = !(unitOfEntry < *victim) && !(*victim < unitOfEntry);
				it = ofVictim ? m_Entries.erase(it) : std::next(it);
			}
			m_Registered.erase(victim);
		}
		m_Registered.insert(unit);
	}

	// Every entry goes, the graphs with them; the registered units stay -- their graphs are captured again at their
	// first sighting.
	void dropGraphs() { m_Entries.clear(); }
	// ... and the registrations with them
	void clear() {
		m_Entries.clear();
		m_Registered.clear();
	}
	// The entries whose key `pred` names go, and their units are registered no longer.
	template <typename Pred>
	void eraseIf(Pred pred) {
		for (auto it = m_Entries.begin(); it != m_Entries.end();) {
			if (pred(it->first)) {
				m_Registered.erase(m_UnitOf(it->first));
				it = m_Entries.erase(it);
			} else {
				++it;
			}
		}
		for (auto it = m_Registered.begin(); it != m_Registered.end();) {
			it = pred(*it) ? m_Registered.erase(it) : std::next(it);
		}
	}

	std::size_t validGraphs() const {
		std::size_t n = 0;
		for (const auto &kv : m_Entries) n += kv.second.graph.valid() ? 1 : 0;
		return n;
	}
	std::size_t registeredUnits() const { return m_Registered.size(); }
	const std::map<Key, Entry> &entries() const { return m_Entries; }
	const std::set<Key> &units() const { return m_Registered; }

private:
	std::uint64_t &m_Clock;
	std::size_t m_MaxUnregistered, m_MaxRegistered;
	UnitOf m_UnitOf;
	std::map<Key, Entry> m_Entries;
	std::set<Key> m_Registered;
};

// unitOf of a cache whose keys are registered one by one
struct UnitIsKey {
	template <typename Key>
	const Key &operator()(const Key &key) const {
		return key;
	}
};

}  // namespace ju
