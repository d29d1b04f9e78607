"""BkdTree (include/slam6d/bkd.h): the dynamic kd-forest over the C ABI's tdtk_forest_* (include/tdtk_hip.h).  Points are
named by their id, the running insertion counter, where the reference hands out pointers."""
import ctypes as C

import numpy as np

from ._capi import check, dptr, f64, iptr, lib

_u64p = C.POINTER(C.c_uint64)
MAX_SLOTS = 32


def plan(counts, fill, bucket, m):
    """tdtk_forest_plan (host only): what inserting m points one at a time does to a forest with these live counts per slot
    and this buffer fill.  Returns (counts, segs, buffer, merges): the final counts, per final slot its segments (kind, a, b)
    -- 0: the live points of old slot a (b of them), 1: the new points [a, b), 2: the old buffer (b points) --, the final
    buffer as (old buffer kept, a, b), and the number of merges."""
    cin = np.ascontiguousarray(counts, np.uint64)
    cout = np.zeros(MAX_SLOTS, np.uint64)
    ns, nsegs, merges = C.c_int(0), C.c_size_t(0), C.c_uint64(0)
    buf = np.zeros(3, np.uint64)
    cap = 4 * MAX_SLOTS + 8
    while True:
        segs = np.zeros((cap, 4), np.int64)
        rc = lib().tdtk_forest_plan(cin.ctypes.data_as(_u64p), len(cin), int(fill), int(bucket), int(m), C.byref(ns),
                                    cout.ctypes.data_as(_u64p), segs.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(nsegs),
                                    buf.ctypes.data_as(_u64p), C.byref(merges))
        if rc == 0 or nsegs.value <= cap:
            check(rc)
            break
        cap = nsegs.value
    per = [[] for _ in range(ns.value)]
    for j, kind, a, b in segs[:nsegs.value].tolist():
        per[j].append((kind, a, b))
    return cout[:ns.value].astype(np.int64).tolist(), per, (bool(buf[0]), int(buf[1]), int(buf[2])), int(merges.value)


class BkdTree:
    """BkdTree(bucketsize) or BkdTree(pts, bucketsize), as the reference's two constructors."""

    def __init__(self, pts_or_bucket, bucketsize=None, device=0):
        h = C.c_void_p()
        if bucketsize is None:
            check(lib().tdtk_forest_create(int(pts_or_bucket), device, C.byref(h)))
        else:
            pts = f64(pts_or_bucket).reshape(-1, 3)
            check(lib().tdtk_forest_create_from_points(dptr(pts), len(pts), int(bucketsize), device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().tdtk_forest_destroy(self._h)
            self._h = None

    __del__ = close

    def insert(self, pts):
        """one point or [m][3]; returns the ids given, in order"""
        pts = f64(pts).reshape(-1, 3)
        first = C.c_int32(0)
        check(lib().tdtk_forest_insert(self._h, dptr(pts), len(pts), C.byref(first)))
        return np.arange(first.value, first.value + len(pts), dtype=np.int32)

    def last_insert(self):
        """tdtk_forest_last_insert: the stages of the last insert call, ms, and what it built"""
        ms = np.zeros(6)
        check(lib().tdtk_forest_last_insert(self._h, dptr(ms)))
        return {"plan_ms": ms[0], "gather_ms": ms[1], "build_ms": ms[2], "total_ms": ms[3], "slots_built": int(ms[4]), "merges": int(ms[5])}

    def remove(self, pts):
        """pts: one point or [m][3] -- BkdTree::remove for each in order; or a boolean mask over ids (a peopleremover or
        collision mask): the points whose id is marked go.  Returns the removed ids [m], -1 where nothing matched."""
        a = np.asarray(pts)
        if a.dtype == np.bool_:
            ids, xyz = self.collectPts()
            if len(a) < (ids.max() + 1 if len(ids) else 0):
                a = np.concatenate([a, np.zeros(ids.max() + 1 - len(a), np.bool_)])
            a = xyz[a[ids]]
        a = f64(a).reshape(-1, 3)
        out = np.empty(len(a), np.int32)
        check(lib().tdtk_forest_remove(self._h, dptr(a), len(a), iptr(out)))
        return out

    def info(self):
        """(live points per slot, buffer fill, size, slots whose tree keeps its leaves in a table)"""
        counts = np.zeros(MAX_SLOTS, np.uint64)
        ns, fill, size, tab = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().tdtk_forest_info(self._h, C.byref(ns), counts.ctypes.data_as(_u64p), C.byref(fill), C.byref(size), C.byref(tab)))
        return (counts[:ns.value].astype(np.int64).tolist(), int(fill.value), int(size.value),
                [s for s in range(ns.value) if tab.value >> s & 1])

    def size(self):
        return self.info()[2]

    def collect(self, slot):
        """(ids, xyz) of the live points of one slot, or of the buffer in insertion order (slot = -1)"""
        n = C.c_uint64(0)
        lib().tdtk_forest_collect(self._h, slot, None, None, 0, C.byref(n))
        ids = np.empty(n.value, np.int32)
        xyz = np.empty((n.value, 3))
        check(lib().tdtk_forest_collect(self._h, slot, iptr(ids), dptr(xyz), n.value, C.byref(n)))
        return ids, xyz

    def collectPts(self):
        """BkdTree::collectPts: the slots in order, then the buffer -- (ids, xyz)"""
        parts = [self.collect(s) for s in range(len(self.info()[0]))] + [self.collect(-1)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def FindClosest(self, q, maxdist2):
        """(ids, d2) for the queries q [K][3]; -1 / -1.0: nothing found"""
        q = f64(q).reshape(-1, 3)
        idx = np.empty(len(q), np.int32)
        d2 = np.empty(len(q))
        check(lib().tdtk_forest_find_closest(self._h, dptr(q), len(q), float(maxdist2), iptr(idx), dptr(d2)))
        return idx, d2

    def kNearestNeighbors(self, q, k):
        """(ids [K][k], d2 [K][k]), ascending, -1 / -1.0 behind the points there are"""
        q = f64(q).reshape(-1, 3)
        idx = np.empty((len(q), k), np.int32)
        d2 = np.empty((len(q), k))
        check(lib().tdtk_forest_knn(self._h, dptr(q), len(q), int(k), iptr(idx), dptr(d2)))
        return idx, d2

    def fixedRangeSearch(self, q, sqRad2):
        """CSR lists (offsets [K+1], ids, d2), as KDtree.fixedRangeSearchBatch"""
        q = f64(q).reshape(-1, 3)
        offsets = np.zeros(len(q) + 1, np.uint64)
        total = C.c_uint64(0)
        cap = max(32 * len(q), 1)
        while True:
            idx = np.empty(cap, np.int32)
            d2 = np.empty(cap)
            rc = lib().tdtk_forest_fixed_range(self._h, dptr(q), len(q), float(sqRad2), offsets.ctypes.data_as(_u64p), iptr(idx),
                                               dptr(d2), cap, C.byref(total))
            if rc == 0:
                break
            if total.value <= cap:
                check(rc)
            cap = int(total.value)
        n = int(total.value)
        return offsets, idx[:n].copy(), d2[:n].copy()
