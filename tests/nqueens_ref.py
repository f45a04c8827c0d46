"""Python restatement of the reference's two N-Queens call trees, written from
its recursion — a board array and ok() as the reference writes them — and not
from the device's column masks:

  bots  test/performance-regression/full-apps/bots/nqueens/nqueens.c:125-182:
        nqueens(n, j, a) with j < n opens a finish and spawns n tasks; task i
        copies the board, sets b[j] = i and, if ok(j + 1, b), is the call
        nqueens(n, j + 1, b); the call sums csols[].
  flat  test/performance-regression/full-apps/nqueens.cpp:41-60: the call tests
        ok() itself and spawns an async only for a placement that passes.

With a task depth d (the BOTS manual cutoff, nqueens.ref.c:99-123) a call with
j >= d is nqueens_ser: the same search with no task and no finish; d = 0 or
d >= n means every call spawns.

reference(n, form, d) -> {"solutions", "tasks", "scopes", "hist"}: tasks are
the asyncs, scopes the finishes the calls open (the one outer finish of either
form is not counted), hist[j] = P(n, j), the number of valid prefixes of
length j.

Up to n = TREE_MAX the call tree itself is run, task by task, with the
reference's ok(). Above it (ok() rescans the whole board for every task: n = 12
would take minutes) the counts come from P(n, j) — one depth-first search over
the board array — and the closed forms the trees obey, with m = min(d, n) and
d = 0 meaning n:
    bots: scopes = sum of P(n, j) over j < m, tasks = n * scopes
    flat: tasks = sum of P(n, j) over 1 <= j <= m, scopes = 0
tests/test_nqueens_host.py checks the two against each other for every n up to
TREE_MAX, both forms and every depth.
"""
import functools
import json
import os

from tests.conftest import GOLD

FORMS = ("bots", "flat")
TREE_MAX = 8


def golden_solutions():
    with open(os.path.join(GOLD, "nqueens_goldens.json")) as f:
        return json.load(f)["solutions"]


def ok(n, a):
    """nqueens.c:71-86: 1 if none of the first n queens conflict."""
    for i in range(n):
        p = a[i]
        for j in range(i + 1, n):
            q = a[j]
            if q == p or q == p - (j - i) or q == p + (j - i):
                return 0
    return 1


def task_depth(n, d):
    return n if d == 0 or d > n else d


class _Tree:
    def __init__(self, n, d):
        self.n = n
        self.m = task_depth(n, d)
        self.tasks = self.scopes = 0
        self.hist = [0] * (n + 1)
        self.hist[0] = 1

    def ser(self, j, a):
        """nqueens_ser (nqueens.c:88-112)."""
        if self.n == j:
            return 1
        s = 0
        for i in range(self.n):
            a[j] = i
            if ok(j + 1, a):
                self.hist[j + 1] += 1
                s += self.ser(j + 1, a)
        return s

    def bots(self, j, a):
        """nqueens (nqueens.c:125-161) with its task body (:162-182) inline."""
        if self.n == j:
            return 1
        if j >= self.m:
            return self.ser(j, a)
        self.scopes += 1  # the finish the call's tasks end in
        csols = [0] * self.n
        for i in range(self.n):
            self.tasks += 1
            b = a[:j] + [i] + [0] * (self.n - j - 1)
            if ok(j + 1, b):
                self.hist[j + 1] += 1
                csols[i] = self.bots(j + 1, b)
        return sum(csols)

    def flat(self, depth, a):
        """nqueens_kernel (nqueens.cpp:41-60); the return value stands for the
        atomic counter's increments below this call."""
        if self.n == depth:
            return 1
        if depth >= self.m:
            return self.ser(depth, a)
        s = 0
        for i in range(self.n):
            b = a[:depth] + [i] + [0] * (self.n - depth - 1)
            if ok(depth + 1, b):  # (nqueens.cpp's own ok() returns the opposite flag, `failed`, and tests !failed)
                self.hist[depth + 1] += 1
                self.tasks += 1
                s += self.flat(depth + 1, b)
        return s


@functools.lru_cache(maxsize=None)
def tree(n, form, d):
    """The call tree itself (n <= TREE_MAX)."""
    if form not in FORMS:
        raise ValueError(form)
    if n > TREE_MAX:
        raise ValueError("the call tree is run up to n = %d only" % TREE_MAX)
    t = _Tree(n, d)
    sol = (t.bots if form == "bots" else t.flat)(0, [0] * n)
    return {"solutions": sol, "tasks": t.tasks, "scopes": t.scopes, "hist": tuple(t.hist)}


@functools.lru_cache(maxsize=None)
def prefix_counts(n):
    """P(n, j) for j = 0..n: a depth-first search that keeps the board array a[]
    and, beside it, which columns and diagonals its queens hold, so that the
    test of one more queen is three look-ups (what ok() decides for a prefix
    that was valid before the queen went on)."""
    hist = [0] * (n + 1)
    a = [0] * n
    col = [False] * n
    up = [False] * (2 * n)   # i + j
    dn = [False] * (2 * n)   # i - j + n

    def go(j):
        hist[j] += 1
        if j == n:
            return
        for i in [i for i in range(n) if not (col[i] or up[i + j] or dn[i - j + n])]:
            a[j] = i
            col[i] = up[i + j] = dn[i - j + n] = True
            go(j + 1)
            col[i] = up[i + j] = dn[i - j + n] = False

    go(0)
    return tuple(hist)


def closed_form(n, form, d):
    if form not in FORMS:
        raise ValueError(form)
    hist = prefix_counts(n)
    m = task_depth(n, d)
    if form == "bots":
        scopes = sum(hist[:m])
        tasks = n * scopes
    else:
        scopes, tasks = 0, sum(hist[1:m + 1])
    return {"solutions": hist[n], "tasks": tasks, "scopes": scopes, "hist": hist}


def reference(n, form="bots", d=0):
    """Computed once per case and shared; the results are immutable."""
    r = tree(n, form, d) if n <= TREE_MAX else closed_form(n, form, d)
    return dict(r, hist=list(r["hist"]))
