"""BkdTree (bkd.h / bkd.cc) restated in numpy as bookkeeping over ids plus brute-force answers: the expectation of the forest
tests, pinned to the reference's compiled sources by tests/golden/make_golden_bkd.py.

State: a bucket size b, a buffer (ids in insertion order, fewer than b), slots (each a list of live ids; [] is an empty
slot).  A point's id is the running insertion counter.  Dist2 is the reference's (dx*dx + dy*dy) + dz*dz in fp64.

What is pinned and what is free ("Dynamic kd-forest"): layouts as id sets per slot and the buffer as a
sequence, every d2, ids where the answer is unique; for equidistant points or identical copies inside one container the model
returns the set of admissible ids."""
import math

import numpy as np

REMOVE_D2 = 0.000000001
DBL_MAX = float(np.finfo(np.float64).max)


def dist2(P, q):
    d = np.asarray(P, np.float64).reshape(-1, 3) - np.asarray(q, np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def ctor_slots(n, b):
    """BkdTree(pts, n, b): max(1.0, ceil(log2(n / b))), n / b an integer division; n < b gives log2(0) = -inf and one slot"""
    v = n // b
    return int(max(1.0, math.ceil(math.log2(v)) if v > 0 else -math.inf))


class Model:
    def __init__(self, b, pts=None):
        self.b = int(b)
        self.xyz = np.zeros((0, 3))
        self.buf = []
        self.slots = []
        self._cache = None      # per container (ids, coordinates) as arrays, for the queries; dropped by every change
        if pts is not None:
            pts = np.asarray(pts, np.float64).reshape(-1, 3)
            self.xyz = pts.copy()
            self.slots = [[] for _ in range(ctor_slots(len(pts), self.b) - 1)] + [list(range(len(pts)))]

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def insert(self, pts):
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        first = len(self.xyz)
        self._cache = None
        self.xyz = np.concatenate([self.xyz, pts])
        for i in range(first, first + len(pts)):
            self.buf.append(i)
            if len(self.buf) == self.b:
                self._merge()
        return first

    def _merge(self):
        i = 0
        while i < len(self.slots) and self.slots[i]:
            i += 1
        if i == len(self.slots):
            self.slots.append([])
        merged = [x for s in self.slots[:i] for x in s] + self.buf
        for k in range(i):
            self.slots[k] = []
        self.slots[i] = merged
        self.buf = []

    def containers(self):
        """(ids) of the buffer, then of every slot: the order remove looks in"""
        return [self.buf] + self.slots

    def remove_candidates(self, p):
        """(container, ids): the lowest container (0: the buffer, s + 1: slot s) with a live point within 1e-9 of p and the
        ids there at the smallest such distance; (None, []) when nothing matches"""
        for c, ids in enumerate(self.containers()):
            if not ids:
                continue
            d = dist2(self.xyz[ids], p)
            if d.min() < REMOVE_D2:
                return c, [ids[j] for j in np.nonzero(d == d.min())[0]]
        return None, []

    def remove(self, p, chosen=None):
        """one request.  chosen: the id an implementation took -- it must be admissible and is the one that goes; None: the
        first candidate.  Returns the removed id or -1."""
        c, cand = self.remove_candidates(p)
        if c is None:
            assert chosen in (None, -1), "removed id %r where nothing matches" % (chosen,)
            return -1
        if chosen is None:
            chosen = cand[0]
        assert chosen in cand, "removed id %d, admissible in container %d: %s" % (chosen, c, cand)
        self._cache = None
        self.containers()[c].remove(chosen)
        return chosen

    def layout(self):
        """(live counts per slot, sorted ids per slot, the buffer as a sequence)"""
        return [len(s) for s in self.slots], [sorted(s) for s in self.slots], list(self.buf)

    def size(self):
        return len(self.buf) + sum(len(s) for s in self.slots)

    def live_ids(self):
        return [x for s in self.slots for x in s] + self.buf

    # ---- queries, brute force ----------------------------------------------------------------------------------------
    def _arrays(self):
        """[(ids, coordinates)] of the slots, then of the buffer"""
        if self._cache is None:
            self._cache = [(np.array(c, np.int64), self.xyz[c].reshape(-1, 3)) for c in self.slots + [self.buf]]
        return self._cache

    def find_closest(self, q, maxdist2):
        """(d2, admissible ids): every slot answers its nearest point with Dist2 < maxdist2, a later slot replaces the result
        only with a strictly smaller distance; the buffer is then scanned against the best so far -- DBL_MAX when no tree
        point was found (Q1).  (-1.0, []) when nothing is found"""
        best, ids = None, []
        arr = self._arrays()
        for s, X in arr[:-1]:
            if not len(s):
                continue
            d = dist2(X, q)
            m = d.min()
            if m < maxdist2 and (best is None or m < best):
                best, ids = m, s[d == m].tolist()
        s, X = arr[-1]
        if len(s):
            d = dist2(X, q)
            m = d.min()
            if m < (DBL_MAX if best is None else best):
                best, ids = m, s[d == m].tolist()
        return (-1.0, []) if best is None else (float(best), ids)

    def knn(self, q, k):
        """the min(k, size) smallest distances, ascending, and per position the ids at that distance"""
        arr = self._arrays()
        ids = np.concatenate([a[0] for a in arr]) if arr else np.zeros(0, np.int64)
        if not len(ids):
            return np.zeros(0), []
        d = dist2(np.concatenate([a[1] for a in arr]), q)
        o = np.argsort(d, kind="stable")
        ds = d[o]
        lo, hi = np.searchsorted(ds, ds[:k], "left"), np.searchsorted(ds, ds[:k], "right")
        return ds[:k], [sorted(ids[o[a:b]].tolist()) for a, b in zip(lo, hi)]

    def fixed_range(self, q, r2):
        """the ids: slot points with Dist2 < r2, buffer points with Dist2 <= r2 (Q2)"""
        out = []
        arr = self._arrays()
        for s, X in arr[:-1]:
            if len(s):
                out += s[dist2(X, q) < r2].tolist()
        s, X = arr[-1]
        if len(s):
            out += s[dist2(X, q) <= r2].tolist()
        return sorted(out)
