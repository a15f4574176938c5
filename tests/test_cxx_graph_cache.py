"""joshupscale_amd/csrc/graph_cache.h (which captured graph a call replays, which ones stay, which ones go: the engine's
cache of device frame pairs and its cache of look-ahead passes) from a stand-alone host program, tests/cxx/graph_cache.cpp,
under the address and undefined-behaviour sanitizers.  No GPU, no HIP header: the header is plain C++ and the program's
graph only counts its lives.  The expectation is the model below, written from the policy:

  use(key)        finds or makes the entry and stamps it with the shared clock.  Before it makes one: while the entries
                  of unregistered units number maxUnregistered or more, the least recently used of THOSE goes (ties: the
                  first in key order).  An entry of a registered unit is never evicted by a use.
  registerUnit    a new unit at the cap of maxRegistered first forgets the unit whose entries were used least recently
                  (the latest use of its entries, 0 without entries; ties: the first in key order), with all its entries.
  dropGraphs      every entry goes; the registered units stay.          clear      the registered units too.
  eraseIf(pred)   the entries pred names go, and their units are registered no longer.

The caps are small (4 and 3): the policy does not depend on them.  Every graph made must be destroyed exactly once and
none may be alive when the caches are gone (the program's exit status).  The last test holds the same script against a
transcription of the rule the pass cache had before it shared this component, under which a miss on an unregistered key
evicts a registered graph whenever the registered entries stand at their cap: the script tells the two apart."""

import os
import subprocess

from helpers import ROOT

MAX_UNREGISTERED, MAX_REGISTERED = 4, 3


def pair_unit(key):
    return (key[0], key[1], 0)


def tuple_unit(key):
    return key


class Model:
    def __init__(self, clock, unit_of):
        self.clock, self.unit_of = clock, unit_of
        self.entries, self.units = {}, set()        # key -> [graph there, seen, last use]

    def use(self, key, capture):
        if key not in self.entries:
            loose = [k for k in sorted(self.entries) if self.unit_of(k) not in self.units]
            if len(loose) >= MAX_UNREGISTERED and loose:
                del self.entries[min(loose, key=lambda k: self.entries[k][2])]     # (min: the first of equals)
            self.entries[key] = [0, 0, 0]
        self.clock[0] += 1
        e = self.entries[key]
        e[1], e[2] = e[1] + 1, self.clock[0]
        made = 1 if capture and not e[0] else 0
        e[0] = 1 if capture else e[0]
        return made

    def recency(self, unit):
        return max([e[2] for k, e in self.entries.items() if self.unit_of(k) == unit], default=0)

    def register(self, unit):
        if unit in self.units:
            return
        if self.units and len(self.units) >= MAX_REGISTERED:
            victim = min(sorted(self.units), key=self.recency)
            self.erase(lambda k: self.unit_of(k) == victim)
            self.units.discard(victim)
        self.units.add(unit)

    def erase(self, pred):
        """Returns nothing; the graphs destroyed are counted by the caller from the entries before and after."""
        for k in [k for k in self.entries if pred(k)]:
            self.units.discard(self.unit_of(k))
            del self.entries[k]
        self.units = {u for u in self.units if not pred(u)}

    def graphs(self):
        return sum(e[0] for e in self.entries.values())


def key_text(key):
    if isinstance(key[0], tuple):
        return "<" + "".join("%d.%d.%d;" % f for f in key) + ">"
    return "(%d,%d,%d)" % key


def expected(ops):
    clock = [0]
    caches = {"p": Model(clock, pair_unit), "t": Model(clock, tuple_unit)}
    made = destroyed = 0
    lines = []
    for which, op, *args in ops:
        c = caches[which]
        before = c.graphs()
        if op in "uc":
            captured = c.use(args[0], op == "c")
            made += captured
            before += captured
        elif op == "r":
            c.register(args[0])
        elif op == "d":
            c.entries.clear()
        elif op == "x":
            c.entries.clear()
            c.units.clear()
        elif op == "L":
            c.erase(lambda k: len(k) > args[0])
        elif op == "S":
            c.erase(lambda k: k[0][1] != 0)
        elif op == "N":
            c.erase(lambda k: k[0][2] != 0)
        else:
            raise AssertionError(op)
        destroyed += before - c.graphs()
        lines.append("%s entries:%s units:%s valid=%d registered=%d made=%d destroyed=%d" % (
            which, "".join(" %s g%d s%d u%d" % (key_text(k), *c.entries[k]) for k in sorted(c.entries)),
            "".join(" " + key_text(u) for u in sorted(c.units)), c.graphs(), len(c.units), made, destroyed))
    return lines + ["end made=%d destroyed=%d alive=0 twice=0" % (made, made), "graph_cache ok"]


def tokens(ops):
    out = []
    for which, op, *args in ops:
        out += [which, op]
        for a in args:
            if isinstance(a, int):
                out.append(a)
            elif isinstance(a[0], tuple):
                out += [len(a)] + [x for f in a for x in f]
            else:
                out += list(a[:2] if op == "r" else a)
    return " ".join(str(t) for t in out)


def tup(*ids, stage=0, scene=0):
    return tuple((i, stage, scene) for i in ids)


def defect_script():
    """The registered cap full, fewer than MAX_UNREGISTERED unregistered entries, then misses on fresh unregistered keys."""
    ops = []
    for k in range(MAX_REGISTERED):
        ops += [("t", "r", tup(10 + k, 20 + k)), ("t", "c", tup(10 + k, 20 + k))]
    ops += [("t", "u", tup(30 + k, 40 + k)) for k in range(MAX_UNREGISTERED - 1)]
    return ops


def script():
    ops = []
    # the unregistered LRU at its cap: four pairs seen, the first refreshed, a fifth evicts the second; equal last uses do
    # not occur under one clock, so the tie rule is met through units without entries below
    ops += [("p", "u", (k, 100, k % 2)) for k in range(4)]
    ops += [("p", "c", (0, 100, 0)), ("p", "u", (4, 100, 0)), ("p", "c", (5, 100, 1))]
    # the pairs' unit: one registration covers both binding sets; registered entries are exempt and do not count
    ops += [("p", "r", (7, 200, 0)), ("p", "c", (7, 200, 0)), ("p", "c", (7, 200, 1)), ("p", "r", (7, 200, 0))]
    ops += [("p", "u", (k, 101, 1)) for k in range(5)]
    # an entry that was there before its pair was registered becomes exempt
    ops += [("p", "r", (4, 101, 0)), ("p", "c", (4, 101, 0))] + [("p", "u", (k, 102, 0)) for k in range(4)]
    # dropGraphs keeps the registrations; a registered pair with no entries counts as oldest when the cap is reached:
    # (4, 101) and the new (8, 200) both have none -- the first in key order goes
    ops += [("p", "d",), ("p", "c", (7, 200, 1)), ("p", "r", (8, 200, 0)), ("p", "r", (9, 200, 0))]
    # the registered cap: the unit whose graphs were used least recently goes with BOTH its entries
    ops += [("p", "c", (8, 200, 0)), ("p", "c", (8, 200, 1)), ("p", "c", (9, 200, 0)), ("p", "c", (9, 200, 1)), ("p", "c", (7, 200, 0)),
            ("p", "u", (8, 200, 1)), ("p", "r", (3, 300, 0)), ("p", "c", (3, 300, 1)), ("p", "u", (9, 200, 0)), ("p", "u", (9, 200, 1))]
    # clear forgets the registrations: the pair's next sighting is an unregistered one
    ops += [("p", "x",), ("p", "u", (7, 200, 0)), ("p", "c", (7, 200, 0))]
    # the tuples: the unit is the key; the two caches share the clock
    ops += [("t", "c", tup(1, 2, 3, 4)), ("t", "c", tup(1, 2)), ("t", "r", tup(5, 6, 7)), ("t", "c", tup(5, 6, 7)),
            ("t", "r", tup(1, 2, 3, 4)), ("t", "c", tup(8, 9, stage=3)), ("t", "r", tup(8, 9, 10, stage=5)), ("t", "c", tup(8, 9, 10, stage=5)),
            ("t", "c", tup(1, 2, scene=1)), ("t", "u", tup(1, 2, scene=2))]
    # each eraseIf predicate, over registered and unregistered entries; an erased registered unit is forgotten
    ops += [("t", "N",), ("t", "S",), ("t", "L", 3), ("t", "c", tup(1, 2, 3, 4)), ("t", "L", 2), ("t", "L", 1)]
    # the registered cap of the tuples, then the defect case, then everything goes with graphs alive
    ops += [("t", "r", tup(k, k + 1)) for k in range(50, 50 + MAX_REGISTERED + 1)]
    ops += [("t", "x",)] + defect_script() + [("p", "c", (1, 1, 1))]
    return ops


def run_program(tmp_path, ops):
    exe = str(tmp_path / "graph_cache")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cxx", "graph_cache.cpp"), "-o", exe])
    out = subprocess.run([exe, str(MAX_UNREGISTERED), str(MAX_REGISTERED)], input=tokens(ops), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n")


def test_graph_cache_host_program(tmp_path):
    ops = script()
    got, want = run_program(tmp_path, ops), expected(ops)
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)
    # the script reaches what it is meant to reach, read from the model's own lines
    state = dict(zip(range(len(ops)), want))
    at = {name: next(i for i, op in enumerate(ops) if op[:2] == name) for name in (("p", "d"), ("p", "x"), ("t", "N"), ("t", "S"))}
    assert "registered=2" in state[at[("p", "d")]] and "valid=0" in state[at[("p", "d")]] and "entries: units:" in state[at[("p", "d")]]
    assert state[at[("p", "x")]].startswith("p entries: units: valid=0 registered=0")
    evicted = [i for i in range(1, len(ops)) if ops[i][1] == "u" and want[i].count(" g") <= want[i - 1].count(" g")
               and ops[i][0] == ops[i - 1][0]]
    assert evicted, "no use at the unregistered cap"
    both = next(i for i, op in enumerate(ops) if op == ("p", "r", (3, 300, 0)))
    assert "(9,200,0)" in want[both - 1] and "(9,200,1)" in want[both - 1] and "(9,200" not in want[both]   # both entries went
    empty_first = next(i for i, op in enumerate(ops) if op == ("p", "r", (9, 200, 0)))
    assert " (4,101,0)" in want[empty_first - 1].split("units:")[1] and " (4,101,0)" not in want[empty_first].split("units:")[1]
    for name in (("t", "N"), ("t", "S")):
        assert want[at[name]].count(" g") < want[at[name] - 1].count(" g")
        assert int(want[at[name]].split("registered=")[1].split()[0]) <= int(want[at[name] - 1].split("registered=")[1].split()[0])
    assert int(want[at[("t", "S")]].split("registered=")[1].split()[0]) < int(want[at[("t", "S")] - 1].split("registered=")[1].split()[0])
    assert int(want[-2].split("made=")[1].split()[0]) > 20


class PassCacheBefore:
    """The pass cache's rule before: registration is a flag in the entry; a miss counts the registered entries and evicts
    ONE entry -- from the unregistered ones at their cap, else from the registered ones once THEIR cap is reached."""

    def __init__(self):
        self.entries, self.clock = {}, 0             # key -> {"graph", "seen", "last", "registered"}

    def entry(self, key):
        if key not in self.entries:
            registered = sum(e["registered"] for e in self.entries.values())
            if len(self.entries) - registered >= MAX_UNREGISTERED or registered >= MAX_REGISTERED:
                from_registered = len(self.entries) - registered < MAX_UNREGISTERED
                among = [k for k in sorted(self.entries) if self.entries[k]["registered"] == from_registered]
                if among:
                    del self.entries[min(among, key=lambda k: self.entries[k]["last"])]
            self.entries[key] = {"graph": 0, "seen": 0, "last": 0, "registered": False}
        self.clock += 1
        self.entries[key]["last"] = self.clock
        return self.entries[key]


def test_a_miss_on_an_unregistered_key_never_costs_a_registered_graph(tmp_path):
    ops = defect_script()
    got, want = run_program(tmp_path, ops), expected(ops)
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)
    misses = [i for i, op in enumerate(ops) if op[1] == "u"]
    assert len(misses) == MAX_UNREGISTERED - 1 >= 2 and misses[0] == 2 * MAX_REGISTERED
    registered = [key_text(op[2]) for op in ops if op[1] == "r"]
    for i in misses:                                  # every registered graph in place after every miss, in the program's output
        assert all(" %s g1 " % r in got[i] for r in registered), got[i]
        assert " valid=%d registered=%d " % (MAX_REGISTERED, MAX_REGISTERED) in got[i] and got[i].endswith("destroyed=0")
    # the rule of before over the same script: the first miss finds the registered entries at their cap and evicts the
    # one used least recently (the count is then below the cap, so the later misses spare the rest -- until a caller
    # registers again)
    old = PassCacheBefore()
    left = []
    for _, op, key in ops:
        if op == "r":
            continue                                   # (prepareBatch: the entry first, then the flag)
        e = old.entry(key)
        if op == "c":
            e["graph"], e["registered"] = 1, True
        left.append(sum(e["registered"] and e["graph"] for e in old.entries.values()))
    assert left[MAX_REGISTERED - 1] == MAX_REGISTERED
    assert left[MAX_REGISTERED:] == [MAX_REGISTERED - 1] * len(misses), left
    assert key_text(next(op[2] for op in ops if op[1] == "r")) not in [key_text(k) for k in old.entries]   # the oldest one
