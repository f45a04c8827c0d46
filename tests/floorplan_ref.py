"""BOTS floorplan restated in Python: the oracle of the floorplan tests.

The serial search of the reference (test/performance-regression/full-apps/bots/
floorplan/floorplan.ref.c: starts() :73-127, lay_down() :135-150, read_inputs()
:159-195, add_cell() :230-328 of the HClib port floorplan.c) with two changes
that no fixture can see: lay_down is a rectangle-intersection test against the
cells already placed (the board holds nothing else), and a rectangle that
leaves the 64 x 64 board does not fit (the reference indexes past the board
there). Such candidates are counted, and every fixture has none.

A cell table is a list of n tuples (shapes, left, above, next), entry i - 1 for
cell i, shapes a list of (rows, cols); left / above name a cell, 0 the dummy
cell (top = bot = 0, lhs = rhs = -1) and -1 nothing. A placement is one
(shape, top, lhs) per cell, in cell order.
"""
import sys

ROWS = COLS = 64
DUMMY = (0, 0, -1, -1)  # top, bot, lhs, rhs of cell 0


def read_input(path):
    """(cells, solution) of a file in the reference's format; solution is -1
    where the file does not end in one."""
    v = [int(w) for w in open(path).read().split()]
    n, p, cells = v[0], 1, []
    for _ in range(n):
        k = v[p]
        shapes = [(v[p + 1 + 2 * j], v[p + 2 + 2 * j]) for j in range(k)]
        p += 1 + 2 * k
        cells.append((shapes, v[p], v[p + 1], v[p + 2]))
        p += 3
    return cells, (v[p] if p < len(v) else -1)


def write_input(path, cells, solution=None):
    with open(path, "w") as f:
        f.write("%d\n" % len(cells))
        for shapes, left, above, nxt in cells:
            f.write("%d\n" % len(shapes))
            for r, c in shapes:
                f.write("%d %d\n" % (r, c))
            f.write("%d %d %d\n" % (left, above, nxt))
        if solution is not None:
            f.write("%d\n" % solution)


def chain(cells):
    """The cell ids in the order the search places them: 1, next(1), ..."""
    out, c = [], 1
    while c != 0:
        out.append(c)
        c = cells[c - 1][3]
    return out


def starts(rows, cols, L, A):
    """The north-west corners starts() allows a rows x cols shape whose left /
    above cells have the rectangles L / A (None: no such dependence)."""
    if L is not None and A is not None:
        top, lhs = A[1] + 1, L[3] + 1
        bot, rhs = top + rows, lhs + cols  # the reference's loose touch test
        if top <= L[1] and bot >= L[0] and lhs <= A[3] and rhs >= A[2]:
            return [(top, lhs)]
        return []
    if L is not None:
        top = max(L[0] - rows + 1, 0)
        bot = min(L[1], ROWS)
        return [(top + i, L[3] + 1) for i in range(bot - top + 1)]
    lhs = max(A[2] - cols + 1, 0)
    rhs = min(A[3], COLS)
    return [(A[1] + 1, lhs + i) for i in range(rhs - lhs + 1)]


def _deps(cells, cid, rect):
    _, left, above, _ = cells[cid - 1]
    return (rect[left] if left >= 0 else None), (rect[above] if above >= 0 else None)


def search(cells, bound0=ROWS * COLS, prune_to=None, collect=False):
    """The serial search in the reference's order (shapes outermost, then the
    starts() locations). With prune_to None a candidate that is not the last
    cell expands iff its area is below the running minimum, which starts at
    bound0 (the reference); with prune_to = c it expands iff area < c, whatever
    has been found. hist[d] = candidates of the d-th cell of the chain that were
    laid down; tasks = candidates spawned; offboard = candidates that left the
    board; touch_pass / touch_fail = shapes of a cell with both dependences
    whose touch test held / failed (no candidate: the branch is dead). With
    collect, `optimal` lists every complete placement of minimum area."""
    n = len(cells)
    order = chain(cells)
    st = {"min": bound0, "fp": (0, 0), "best": None, "tasks": 0, "laid": 0, "complete": 0, "offboard": 0,
          "improvements": 0, "touch_pass": 0, "touch_fail": 0}
    hist = [0] * (n + 1)
    optimal = []
    rect = {0: DUMMY}
    placed = []  # (cell, shape, top, lhs)

    def add_cell(d, fr, fc):
        cid = order[d]
        shapes = cells[cid - 1][0]
        L, A = _deps(cells, cid, rect)
        others = [rect[c] for c in order[:d]]
        last = d + 1 == n
        for i, (rows, cols) in enumerate(shapes):
            nws = starts(rows, cols, L, A)
            if L is not None and A is not None:
                st["touch_pass" if nws else "touch_fail"] += 1
            for top, lhs in nws:
                st["tasks"] += 1
                bot, rhs = top + rows - 1, lhs + cols - 1
                if bot >= ROWS or rhs >= COLS:
                    st["offboard"] += 1
                    continue
                if any(not (o[1] < top or o[0] > bot or o[3] < lhs or o[2] > rhs) for o in others):
                    continue
                st["laid"] += 1
                hist[d + 1] += 1
                r, c = max(fr, bot + 1), max(fc, rhs + 1)
                area = r * c
                if last:
                    st["complete"] += 1
                    if collect and area <= st["min"]:
                        if area < st["min"]:
                            del optimal[:]
                        optimal.append(sorted(placed + [(cid, i, top, lhs)]))
                    if area < st["min"]:
                        st["min"], st["fp"] = area, (r, c)
                        st["best"] = sorted(placed + [(cid, i, top, lhs)])
                        st["improvements"] += 1
                elif area < (st["min"] if prune_to is None else prune_to):
                    rect[cid] = (top, bot, lhs, rhs)
                    placed.append((cid, i, top, lhs))
                    add_cell(d + 1, r, c)
                    placed.pop()
                    del rect[cid]

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 200))
    add_cell(0, 0, 0)
    out = {"min_area": st["min"], "footprint": list(st["fp"]), "hist": hist, "tasks": st["tasks"],
           "laid": st["laid"], "complete": st["complete"], "offboard": st["offboard"],
           "improvements": st["improvements"], "touch_pass": st["touch_pass"], "touch_fail": st["touch_fail"],
           "placements": [list(p[1:]) for p in st["best"]] if st["best"] else None}
    if collect:
        out["optimal"] = [[list(p[1:]) for p in pl] for pl in optimal]
    return out


COUNTS = ("tasks", "laid", "complete", "hist")


def bounds(cells):
    """{"opt", "footprint", "offboard", "U", "L"}: U the exhaustive search (the
    bound held at 4096), L the search in which a candidate expands iff
    area < opt, the final optimum. MIN_AREA >= opt at every moment of every
    schedule, so every pruned run expands at least L's candidates and at most
    U's. (L need not reach the optimum itself: a partial placement whose area is
    already opt expands in a real run only while the bound is above opt.)"""
    u = search(cells, prune_to=ROWS * COLS)
    l = search(cells, prune_to=u["min_area"])
    return {"opt": u["min_area"], "footprint": u["footprint"], "offboard": u["offboard"],
            "U": {k: u[k] for k in COUNTS}, "L": {k: l[k] for k in COUNTS}}


def board_of(cells, placements):
    """The 64 x 64 board of cell ids (row-major list) of a placement."""
    b = [0] * (ROWS * COLS)
    for cid, (s, top, lhs) in enumerate(placements, 1):
        rows, cols = cells[cid - 1][0][s]
        for r in range(top, top + rows):
            for c in range(lhs, lhs + cols):
                b[r * COLS + c] = cid
    return b


def check_placement(cells, placements, footprint, board):
    """None if `placements` is a complete legal floorplan with that footprint
    and board, else what is wrong with it."""
    n = len(cells)
    if len(placements) != n:
        return "%d placements for %d cells" % (len(placements), n)
    rect = {0: DUMMY}
    for cid in chain(cells):
        s, top, lhs = placements[cid - 1]
        shapes, left, above, _ = cells[cid - 1]
        if not 0 <= s < len(shapes):
            return "cell %d: shape %d of %d" % (cid, s, len(shapes))
        rows, cols = shapes[s]
        L, A = _deps(cells, cid, rect)
        if (top, lhs) not in starts(rows, cols, L, A):
            return "cell %d: (%d, %d) is no start of shape %d" % (cid, top, lhs, s)
        bot, rhs = top + rows - 1, lhs + cols - 1
        if top < 0 or lhs < 0 or bot >= ROWS or rhs >= COLS:
            return "cell %d leaves the board" % cid
        for o, r in rect.items():
            if o and not (r[1] < top or r[0] > bot or r[3] < lhs or r[2] > rhs):
                return "cells %d and %d overlap" % (o, cid)
        rect[cid] = (top, bot, lhs, rhs)
    fp = [max(r[1] for r in rect.values()) + 1, max(r[3] for r in rect.values()) + 1]
    if list(footprint) != fp:
        return "footprint %s, bounding box %s" % (list(footprint), fp)
    if board is not None and list(board) != board_of(cells, placements):
        return "the board is not the cells' rectangles"
    return None
