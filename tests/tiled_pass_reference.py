"""Where the look-ahead passes of a tiled call start (docs/tiled.md "Look-ahead passes"): the restatement of
csrc/tile_pass_plan.h.  A call of ``count`` consecutive frames runs as consecutive passes of at most ``cap`` frames; frame
``j`` may not share a pass with an earlier frame ``i`` of it that it clashes with (an input plane of one over an output
plane of the other).  Greedy: a frame starts a new pass when the running one is full or holds a frame it clashes with."""

CAP_MAX = 8


def clamp_cap(frames):
    return min(max(int(frames), 1), CAP_MAX)


def plan(count, cap, clash=None):
    """The indices at which passes start; ``clash``: a set of pairs ``(i, j)``, ``i < j``, that cannot share a pass."""
    clash = clash or set()
    cap = max(cap, 1)
    starts, start = [], 0
    for j in range(count):
        if j == 0 or j - start >= cap or any((i, j) in clash for i in range(start, j)):
            start = j
            starts.append(j)
    return starts


def passes(count, cap, clash=None):
    """The passes as ``(first frame, frames)``."""
    starts = plan(count, cap, clash) + [count]
    return [(a, b - a) for a, b in zip(starts, starts[1:])]


def matrix(count, clash):
    """``clash`` as the row-major ``count x count`` byte matrix the hook takes."""
    m = bytearray(count * count)
    for i, j in clash:
        m[i * count + j] = 1
    return bytes(m)


def cases():
    """(count, cap, clash): counts 0 .. 20 under caps 1 .. 8 without a clash, with ONE clash at every position (each pair
    of neighbours, and pairs two and five apart), and with clashes in a row."""
    out = []
    for count in range(21):
        for cap in range(1, 9):
            out.append((count, cap, set()))
    for count in (2, 3, 8, 9, 11, 20):
        for cap in (1, 2, 3, 8):
            for j in range(1, count):
                out.append((count, cap, {(j - 1, j)}))
                if j >= 2:
                    out.append((count, cap, {(j - 2, j)}))
                if j >= 5:
                    out.append((count, cap, {(j - 5, j)}))
            out.append((count, cap, {(j - 1, j) for j in range(1, count)}))             # every neighbour: passes of one
            out.append((count, cap, {(j - 1, j) for j in range(1, min(count, 4))}))      # three in a row, then free
            out.append((count, cap, {(j - 1, j) for j in range(max(count - 3, 1), count)}))
            out.append((count, cap, {(i, j) for j in range(count) for i in range(j) if (i + j) % 3 == 0}))
    return out
