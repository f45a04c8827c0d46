"""A Python restatement of BOTS sort's call tree (the reference's
test/performance-regression/full-apps/bots/sort/sort.ref.c:315-423): cilksort's
four-way split, cilkmerge's binary split with binsplit, and the input generator
(:93-97, :425-446). One difference, on purpose: the empty-range copy of
cilkmerge moves high1 - low1 + 1 keys (the reference's memcpy, :344, is one
short and mis-sorts e.g. descending input).

The sorted result is unique, and the call tree is a function of the input and
the two cutoffs alone, so the device sort (hclib_hip_sort_i64) is held to both:
its output to the array, its task counts to the counts here.

A helper, not a test module."""
import functools
import sys

import numpy as np

COUNTS = ("sort_leaf", "sort_split", "merge_leaf", "merge_split", "merge_empty")

# (n, merge_cutoff, sort_cutoff)
CASES = [(4, 2, 4), (5, 2, 4), (1000, 2048, 2048), (2047, 2048, 2048), (2048, 2048, 2048), (8191, 2048, 2048),
         (4099, 2, 4), (4099, 16, 64), (40000, 64, 256), (40000, 2048, 2048)]
INPUTS = ("bots", "ascending", "descending", "equal", "five_values", "random_int64")


def my_rand_stream(n):
    """my_srand(1), then n draws of my_rand (:93-102), unsigned long = 64 bits."""
    r, out = 1, []
    for _ in range(n):
        r = (r * 1103515245 + 12345) & 0xFFFFFFFFFFFFFFFF
        out.append(r)
    return out


def bots_input(n):
    """fill_array + scramble_array (:425-446)."""
    a = list(range(n))
    for i, r in enumerate(my_rand_stream(n)):
        j = r % n
        a[i], a[j] = a[j], a[i]
    return np.array(a, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _input(name, n):
    if name == "bots":
        a = bots_input(n)
    elif name == "ascending":
        a = np.arange(n, dtype=np.int64)
    elif name == "descending":
        a = np.arange(n, 0, -1, dtype=np.int64)
    elif name == "equal":
        a = np.full(n, 7, dtype=np.int64)
    elif name == "five_values":
        a = np.random.default_rng(n).integers(0, 5, n, dtype=np.int64)
    elif name == "random_int64":
        info = np.iinfo(np.int64)
        rng = np.random.default_rng(n + 1)
        a = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
        # the extremes, several times each: the device leaf sort pads with the maximum
        where = rng.permutation(n)[:min(n, 6)]
        a[where[0::2]] = info.max
        a[where[1::2]] = info.min
    else:
        raise KeyError(name)
    a.setflags(write=False)
    return a


def make_input(name, n):
    """A fresh, writable copy of input `name` of n keys."""
    return _input(name, n).copy()


class _Tree:
    def __init__(self, keys, merge_cutoff, sort_cutoff):
        n = len(keys)
        self.arr = [list(keys), [None] * n]  # the array, tmp
        self.mc, self.sc = merge_cutoff, sort_cutoff
        self.counts = dict.fromkeys(COUNTS, 0)
        self.merge_depth = 0

    @staticmethod
    def binsplit(val, s, low, high):  # :292-312
        while low != high:
            mid = low + ((high - low + 1) >> 1)
            if val <= s[mid]:
                high = mid - 1
            else:
                low = mid
        return low - 1 if s[low] > val else low

    def merge(self, src, low1, high1, low2, high2, lowdest, depth=0):  # cilkmerge_par, :315-376
        s, d = self.arr[src], self.arr[1 - src]
        self.merge_depth = max(self.merge_depth, depth)
        if high2 - low2 > high1 - low1:
            low1, low2 = low2, low1
            high1, high2 = high2, high1
        if high2 < low2:
            self.counts["merge_empty"] += 1
            k = high1 - low1 + 1  # the reference copies high1 - low1
            d[lowdest:lowdest + k] = s[low1:low1 + k]
            return
        if high2 - low2 < self.mc:
            self.counts["merge_leaf"] += 1
            m = sorted(s[low1:high1 + 1] + s[low2:high2 + 1])  # seqmerge's result
            d[lowdest:lowdest + len(m)] = m
            return
        self.counts["merge_split"] += 1
        split1 = (high1 - low1 + 1) // 2 + low1
        split2 = self.binsplit(s[split1], s, low2, high2)
        lowsize = split1 - low1 + split2 - low2
        d[lowdest + lowsize + 1] = s[split1]
        self.merge(src, low1, split1 - 1, low2, split2, lowdest, depth + 1)
        self.merge(src, split1 + 1, high1, split2 + 1, high2, lowdest + lowsize + 2, depth + 1)

    def sort(self, low, size):  # cilksort_par, :378-423 (tmp at the same offsets)
        if size < self.sc:
            self.counts["sort_leaf"] += 1
            self.arr[0][low:low + size] = sorted(self.arr[0][low:low + size])  # seqquick's result
            return
        self.counts["sort_split"] += 1
        q = size // 4
        a, b, c, d = low, low + q, low + 2 * q, low + 3 * q
        self.sort(a, q)
        self.sort(b, q)
        self.sort(c, q)
        self.sort(d, size - 3 * q)
        self.merge(0, a, a + q - 1, b, b + q - 1, a)
        self.merge(0, c, c + q - 1, d, low + size - 1, c)
        self.merge(1, a, c - 1, c, a + size - 1, a)


def cilksort(keys, merge_cutoff=2048, sort_cutoff=2048):
    """(sorted int64 array, counts) of the call tree over `keys`. counts holds
    the five COUNTS plus what the device program derives from them: tasks (one
    per SORT, per MERGE_PHASE continuation and per merge call), finishes (two
    scopes per sort split and the root's outer one), check_ins (two per merge
    split), promises (one per scope) and wait_nodes (one per split scope)."""
    if merge_cutoff < 2 or sort_cutoff < 4:
        raise ValueError("cilksort: merge_cutoff >= 2 and sort_cutoff >= 4")
    t = _Tree([int(x) for x in keys], merge_cutoff, sort_cutoff)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 20000))
    try:
        t.sort(0, len(keys))
    finally:
        sys.setrecursionlimit(old)
    c = dict(t.counts)
    merges = c["merge_leaf"] + c["merge_split"] + c["merge_empty"]
    c["tasks"] = c["sort_leaf"] + 2 * c["sort_split"] + merges
    c["wait_nodes"] = 2 * c["sort_split"]
    c["finishes"] = c["promises"] = 2 * c["sort_split"] + 1  # and the root's outer finish
    c["check_ins"] = 2 * c["merge_split"]
    c["merge_depth"] = t.merge_depth
    return np.array(t.arr[0], dtype=np.int64), c


@functools.lru_cache(maxsize=None)
def reference(name, n, merge_cutoff, sort_cutoff):
    """cilksort of input `name`, computed once and shared (do not modify)."""
    out, counts = cilksort(_input(name, n), merge_cutoff, sort_cutoff)
    out.setflags(write=False)
    return out, counts
