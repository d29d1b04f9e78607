"""Generates tests/golden/k19_bkd.npz: the dynamic kd-forest (BkdTree) pinned to the reference's compiled sources.

    python tests/golden/make_golden_bkd.py          (needs the reference checkout: $TDTK_REF, default /root/reference)

src/slam6d/bkd.cc, kd.cc and searchTree.cc are compiled as they are, next to a driver of our own (DRIVER below), into a
temporary directory, with the flags of oracle/build_ref.sh and one stand-in header, slam6d/scan.h = "class Scan;".  Nothing of
it is committed or left under oracle/.  The driver never destroys a BkdTree: ~BkdTree calls tree->~KDtree() on the
uninitialised pointers of empty slots.  bkd.cc's unimplemented methods have no return statement and are never called.

What the fixture holds is the model's answer (tests/bkd_model.py); the generator asserts, for every case it may run the
reference on, reference == model in the sense of DESIGN.md section 4, "Dynamic kd-forest": layouts as id sets per slot and the
buffer as a sequence, remove counts, every d2, ids where unique, k-NN distance lists, fixed-radius lists as id sets.  On every
random-cloud case all candidate distances of every query are distinct (asserted), so nothing there is compared "up to ties";
on the lattice, copies and degenerate cases the admissible ids are stored and the reference's answer must be among them.  An
ulp-thin box prune that made the reference miss its true neighbour would show up as reference != model: choose another seed.
The emptied-leaf case is never run through the reference (its _CollectPts tests npts, not isleaf, and is undefined there).

A case is a script: ops [n][3] = (code, a, b) over the case's arrays -- INS: insert P[a:b] (one call on the device, one point
at a time in the reference and the model); REM: remove R[a:b] in order (one call); CHK: the layout; QRY: the queries Q at this
state."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import bkd_model  # noqa: E402

OUT = os.path.join(_HERE, "k19_bkd.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")
MAX_BYTES = 300 * 1000
INS, REM, CHK, QRY = 0, 1, 2, 3
HUGE = 1e300

# the flags of oracle/build_ref.sh
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=8 -DMAX_OPENMP_NUM_THREADS=512 -w".split()

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "slam6d/bkd.h"

// a forest over pointers into one array of the caller's (`store`, [n][3]): a point's id is its row.  Never destroyed
extern "C" void* rb_new(int b) { return new BkdTree(b); }
extern "C" void* rb_new_pts(double* store, int n, int b)
{
  double** pts = new double*[n];
  for (int i = 0; i < n; i++) pts[i] = store + 3 * (size_t)i;
  return new BkdTree(pts, n, b);
}
extern "C" void rb_insert(void* t, double* p) { ((BkdTree*)t)->insert(p); }
extern "C" int rb_remove(void* t, double* p) { return ((BkdTree*)t)->remove(p); }
extern "C" long rb_size(void* t) { return (long)((BkdTree*)t)->size(); }
extern "C" int rb_info(void* t, char* out, int cap)
{
  const std::string s = ((BkdTree*)t)->info();
  strncpy(out, s.c_str(), cap - 1);
  out[cap - 1] = 0;
  return (int)s.size();
}
extern "C" long rb_collect(void* t, const double* store, long* ids)
{
  std::vector<double*> v = ((BkdTree*)t)->collectPts();
  for (size_t i = 0; i < v.size(); i++) ids[i] = (long)((v[i] - store) / 3);
  return (long)v.size();
}
extern "C" long rb_find_closest(void* t, double* q, double maxdist2, const double* store)
{
  double* r = ((BkdTree*)t)->FindClosest(q, maxdist2);
  return r ? (long)((r - store) / 3) : -1;
}
extern "C" int rb_knn(void* t, double* q, int k, double* out)
{
  std::vector<Point> v = ((BkdTree*)t)->kNearestNeighbors(q, k);
  for (size_t i = 0; i < v.size(); i++) { out[3 * i] = v[i].x; out[3 * i + 1] = v[i].y; out[3 * i + 2] = v[i].z; }
  return (int)v.size();
}
extern "C" long rb_range(void* t, double* q, double r2, double* out, long cap)
{
  std::vector<Point> v = ((BkdTree*)t)->fixedRangeSearch(q, r2);
  for (size_t i = 0; i < v.size() && (long)i < cap; i++) { out[3 * i] = v[i].x; out[3 * i + 1] = v[i].y; out[3 * i + 2] = v[i].z; }
  return (long)v.size();
}
"""


# ---- the cases ----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, b, P, ops, ctor=0, R=None, Q=None, md2=(), ks=(), r2=(), ref=True, ties=False, sets=None):
        self.name, self.b, self.ctor, self.ref, self.ties = name, b, ctor, ref, ties
        self.sets = ties if sets is None else sets       # store the admissible ids of every tied answer
        self.P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)      # the first `ctor` rows go to the constructor
        self.R = np.ascontiguousarray(R if R is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
        self.Q = np.ascontiguousarray(Q if Q is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
        self.ops = [tuple(o) for o in ops]
        self.md2, self.ks, self.r2 = tuple(md2), tuple(ks), tuple(r2)


def _cloud(seed, n):
    return np.random.default_rng(seed).uniform(-10.0, 10.0, (n, 3))


def _queries(seed, n, P):
    """uniform in +-12, every fourth one a stored point's coordinates"""
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-12.0, 12.0, (n, 3))
    if len(P):
        Q[::4] = P[rng.integers(0, len(P), len(Q[::4]))]
    return Q


def layout_totals(b):
    return [0, 1, b - 1, b, b + 1, 2 * b, 3 * b, 4 * b - 1, 4 * b, 16 * b - 1, 16 * b] + ([1003] if b == 20 else [])


def ragged(total, b):
    """the sizes of ragged calls adding up to total: 1, b-1, b+1, 7b+2, ..."""
    out, pat, i = [], [1, b - 1, b + 1, 7 * b + 2, 2, 3 * b], 0
    while sum(out) < total:
        out.append(min(max(pat[i % len(pat)], 1), total - sum(out)))
        i += 1
    return out


def cases():
    cs = []
    # 1. layouts, with queries on three of them
    for b in (3, 20):
        for n in layout_totals(b):
            P = _cloud(1000 + 31 * b + n, n)
            q = n in (4 * b - 1, 16 * b)
            mid = 4.0
            cs.append(Case("lay_b%d_n%d" % (b, n), b, P, [(INS, 0, n), (CHK, 0, 0)] + ([(QRY, 0, 0)] if q else []),
                           Q=_queries(7 + n, 120, P) if q else None, md2=(1e-3, mid, HUGE),
                           ks=[k for k in (1, 5, b + 2, n + 3) if k <= 64], r2=(mid, 9.0)))
    # 2. the constructor, then inserts until a merge takes the large tree into an appended slot
    for b, n in [(3, 1), (3, 2), (3, 3), (3, 6), (3, 7), (3, 30), (20, 1003)]:
        S = bkd_model.ctor_slots(n, b)
        more = b * 2 ** (S - 1)
        P = _cloud(2000 + 17 * b + n, n + more)
        cs.append(Case("ctor_b%d_n%d" % (b, n), b, P,
                       [(CHK, 0, 0), (INS, n, n + more // 2), (CHK, 0, 0), (QRY, 0, 0), (INS, n + more // 2, n + more), (CHK, 0, 0)],
                       ctor=n, Q=_queries(50 + n, 100, P[:n]), md2=(1e-3, 4.0, HUGE), ks=(1, 5, b + 2), r2=(4.0,)))
    # 3. remove
    for b in (3, 20):
        n = 3 * b + b - 1                      # slots [b, 2b], b - 1 in the buffer
        P = _cloud(3000 + b, n)
        R = np.array([P[3 * b], P[0], P[1], P[1], P[2], P[2], [100.0, 100.0, 100.0], P[2 * b], P[n - 1]])
        cs.append(Case("rm_basic_b%d" % b, b, P,
                       [(INS, 0, n), (CHK, 0, 0), (REM, 0, 1), (REM, 1, 2), (CHK, 0, 0), (REM, 2, 4), (REM, 4, 5), (REM, 5, 6), (REM, 6, 7),
                        (CHK, 0, 0), (REM, 7, 9), (CHK, 0, 0), (QRY, 0, 0)],
                       R=R, Q=_queries(60 + b, 200, P), md2=(1e-3, 4.0, HUGE), ks=(1, 5, b + 2), r2=(4.0,)))
    # copies of one coordinate in the buffer, slot 0 and slot 2; two copies inside slot 2 (b = 3: 12 -> slot 2, 3 -> slot 0, 1 -> buffer)
    P = _cloud(3100, 16)
    X, Y = np.array([1.5, -2.25, 3.0]), np.array([-4.0, 0.5, 0.125])
    P[0] = P[12] = P[15] = X
    P[1] = P[2] = Y
    R = np.array([X, X, X, X, Y, Y, Y])
    cs.append(Case("rm_copies_b3", 3, P, [(INS, 0, 16), (CHK, 0, 0), (REM, 0, 4), (CHK, 0, 0), (REM, 4, 7), (CHK, 0, 0), (QRY, 0, 0)],
                   R=R, Q=np.concatenate([[X, Y], _queries(61, 40, P)]), md2=(1e-3, 4.0, HUGE), ks=(1, 5), r2=(4.0,), ties=True))
    # all points of slot 0 go: the slot becomes empty and the next merge lands in it
    P = _cloud(3200, 12)
    cs.append(Case("rm_empty_slot_b3", 3, P, [(INS, 0, 9), (CHK, 0, 0), (REM, 0, 3), (CHK, 0, 0), (QRY, 0, 0), (INS, 9, 12), (CHK, 0, 0)],
                   R=P[6:9].copy(), Q=_queries(62, 60, P), md2=(1e-3, 4.0, HUGE), ks=(1, 5), r2=(4.0,)))
    # 4. a leaf emptied completely, the tree merged later: three points far from the other nine are a leaf of the 12-point tree in
    # slot 2 whatever the order (the centroid split puts them alone on one side).  Model only
    P = _cloud(3300, 24)
    P[3:6] = np.array([[1000.0, 1.0, 2.0], [1001.0, -1.0, 0.5], [1002.0, 0.0, -2.0]])
    cs.append(Case("rm_leaf_b3", 3, P, [(INS, 0, 12), (CHK, 0, 0), (REM, 0, 3), (CHK, 0, 0), (QRY, 0, 0), (INS, 12, 24), (CHK, 0, 0), (QRY, 0, 0)],
                   R=P[3:6].copy(), Q=np.concatenate([P[3:6] + 0.25, _queries(63, 60, P)]), md2=(1e-3, 4.0, HUGE), ks=(1, 5, 24), r2=(4.0,),
                   ref=False))
    # 5. the lattice: the 3 x 3 x 3 grid in the trees (slot 3: 24, slot 0: 3), (3,0,0) and (0,3,0) in the buffer
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float64)
    P = np.concatenate([g, [[3.0, 0.0, 0.0], [0.0, 3.0, 0.0]]])
    Q = np.concatenate([[[-1.0, 0.0, 0.0],      # (0,0,0) at exactly 1: not found at maxdist2 = 1, then the buffer however far (Q1)
                         [3.0, 1.0, 0.0],       # r2 = 1: (3,0,0) in the buffer at exactly 1 taken, (2,1,0) in a tree at exactly 1 left out (Q2)
                         [10.0, 10.0, 10.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5]],
                        g + np.array([0.5, 0.0, 0.0]), g[::3] + np.array([0.0, -1.0, 0.0])])
    cs.append(Case("lattice_b3", 3, P, [(INS, 0, 29), (CHK, 0, 0), (QRY, 0, 0)], Q=Q, md2=(1.0, 2.0, HUGE), ks=(1, 5, 32), r2=(1.0, 2.0, 4.0),
                   ties=True))
    # 6. degenerate: 200 copies of one coordinate among 50 others; three copies go
    rng = np.random.default_rng(3600)
    P = _cloud(3601, 250)
    Z = np.array([2.5, 2.5, -1.0])
    P[rng.permutation(250)[:200]] = Z
    cs.append(Case("degenerate_b20", 20, P, [(INS, 0, 250), (CHK, 0, 0), (REM, 0, 3), (CHK, 0, 0), (QRY, 0, 0)], R=np.array([Z, Z, Z]),
                   Q=np.concatenate([[Z], _queries(64, 20, P)]), md2=(1e-3, HUGE), ks=(1, 64), r2=(1e-6, 4.0), ties=True, sets=False))
    # 7. mixed: 20 000 points by ragged inserts, 500 removes interleaved
    n = 20000
    P = _cloud(3700, n)
    rng = np.random.default_rng(3701)
    ops, R, a, step = [], [], 0, 0
    for sz in _mixed_calls(n):
        ops.append((INS, a, a + sz))
        a += sz
        step += 1
        if step % 4 == 0 and len(R) < 500:
            pick = rng.integers(0, a, 25)           # stored points, some of them gone already (those requests match nothing)
            ops.append((REM, len(R), len(R) + 25))
            R += [P[i] for i in pick]
    ops += [(CHK, 0, 0), (QRY, 0, 0)]
    cs.append(Case("mixed_b20", 20, P, ops, R=np.array(R), Q=_queries(65, 3000, P), md2=(4.0,), ks=(5,), r2=(1.0,)))
    return cs


def _mixed_calls(n):
    """ragged call sizes that reach n in about a hundred calls"""
    pat, out, i = [1, 19, 21, 142, 777, 5, 400, 60, 1003, 20], [], 0
    while sum(out) < n:
        out.append(min(pat[i % len(pat)], n - sum(out)))
        i += 1
    return out


# ---- the model's answers of a case: what the fixture holds --------------------------------------------------------------------------
def expected(case, m, i, out, stats=None):
    """the answers of the queries of op i at the model's state, into out"""
    pre = "%s_q%d_" % (case.name, i)
    Q = case.Q
    for j, md in enumerate(case.md2):
        r = [m.find_closest(q, md) for q in Q]
        if case.ties:
            out[pre + "fc%d_d2" % j] = np.array([x[0] for x in r])      # (a random cloud: Dist2 of the id, which is unique there)
        out[pre + "fc%d_id" % j] = np.array([x[1][0] if len(x[1]) == 1 else -1 for x in r], np.int32)
        if case.sets:
            out[pre + "fc%d_toff" % j] = np.concatenate([[0], np.cumsum([len(x[1]) for x in r])]).astype(np.int32)
            out[pre + "fc%d_tids" % j] = np.array([y for x in r for y in x[1]], np.int32)
        if stats is not None:
            stats["q1"] += sum(1 for x in r if x[0] > md)
    for k in case.ks:
        r = [m.knn(q, k) for q in Q]
        d2 = np.full((len(Q), k), -1.0)
        ids = np.full((len(Q), k), -1, np.int32)
        for qi, (d, t) in enumerate(r):
            d2[qi, :len(d)] = d
            ids[qi, :len(d)] = [x[0] if len(x) == 1 else -1 for x in t]
        if case.ties:
            out[pre + "knn%d_d2" % k] = d2          # (a random cloud: Dist2 of the ids, which are unique there)
        out[pre + "knn%d_id" % k] = ids
        if case.sets:
            flat = [x for _, t in r for x in t]
            out[pre + "knn%d_toff" % k] = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int32)
            out[pre + "knn%d_tids" % k] = np.array([y for x in flat for y in x], np.int32)
    for j, r2 in enumerate(case.r2):
        r = [m.fixed_range(q, r2) for q in Q]
        out[pre + "rng%d_off" % j] = np.concatenate([[0], np.cumsum([len(x) for x in r])]).astype(np.int32)
        out[pre + "rng%d_ids" % j] = np.array([y for x in r for y in x], np.int32)
    if stats is not None and not case.ties:
        live = np.array(m.live_ids())
        for q in Q:
            d = bkd_model.dist2(m.xyz[live], q)
            assert len(np.unique(d)) == len(d), "%s: equidistant candidates on a random cloud" % case.name


def compute_case(case, out, stats=None, ref=None):
    """the model's layouts, remove results and answers of one case into out; with ref (a RefForest) the reference beside it"""
    def on(code, i, m):
        if code == CHK:
            counts, ids, buf = m.layout()
            out["%s_c%d_counts" % (case.name, i)] = np.array(counts, np.int64)
            out["%s_c%d_ids" % (case.name, i)] = np.array([x for s in ids for x in s], np.int32)
            out["%s_c%d_buf" % (case.name, i)] = np.array(buf, np.int32)
            if ref:
                ref.check_layout(case, m, i)
        elif code == QRY:
            expected(case, m, i, out, stats)
            if ref:
                ref.check_queries(case, m, i, out)

    m = bkd_model.Model(case.b, case.P[:case.ctor]) if case.ctor else bkd_model.Model(case.b)
    if ref:
        ref.start(case)
    for i, (code, a, b) in enumerate(case.ops):
        if code == INS:
            m.insert(case.P[a:b])
            if ref:
                ref.insert(case.P[a:b])
        elif code == REM:
            ids, cont = [], []
            for p in case.R[a:b]:
                c, cand = m.remove_candidates(p)
                cont.append(-1 if c is None else c)
                ids.append(m.remove(p))
            out["%s_r%d_id" % (case.name, i)] = np.array(ids, np.int32)
            out["%s_r%d_cont" % (case.name, i)] = np.array(cont, np.int32)
            if ref:
                got = ref.remove(case.R[a:b])
                assert got == [1 if x >= 0 else 0 for x in ids], (case.name, i, got, ids)
            if stats is not None:
                stats["removed"] += sum(x >= 0 for x in ids)
                stats["unmatched"] += sum(x < 0 for x in ids)
        on(code, i, m)
    return m


# ---- the reference ------------------------------------------------------------------------------------------------------------
def have_ref():
    return all(os.path.isfile(os.path.join(REF, "src", "slam6d", f)) for f in ("bkd.cc", "kd.cc", "searchTree.cc"))


_lib = None
_tmp = None


def ref_lib():
    """bkd.cc + kd.cc + searchTree.cc + DRIVER, built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="k19_ref_")
        d = _tmp.name
        os.makedirs(os.path.join(d, "standin", "slam6d"))
        with open(os.path.join(d, "standin", "slam6d", "scan.h"), "w") as f:
            f.write("class Scan;\n")
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        inc = ["-I" + os.path.join(d, "standin"), "-I" + os.path.join(REF, "include"),
               "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10")]
        objs = []
        for src in [os.path.join(REF, "src", "slam6d", f) for f in ("bkd.cc", "kd.cc", "searchTree.cc")] + [os.path.join(d, "driver.cc")]:
            o = os.path.join(d, os.path.basename(src) + ".o")
            subprocess.check_call(["g++"] + FLAGS + inc + ["-c", src, "-o", o])
            objs.append(o)
        so = os.path.join(d, "libk19.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-o", so] + objs)
        L = C.CDLL(so)
        L.rb_new.restype = L.rb_new_pts.restype = C.c_void_p
        L.rb_new.argtypes = [C.c_int]
        L.rb_new_pts.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rb_insert.argtypes = [C.c_void_p, C.c_void_p]
        L.rb_remove.argtypes = [C.c_void_p, C.c_void_p]
        L.rb_size.restype = C.c_long
        L.rb_size.argtypes = [C.c_void_p]
        L.rb_info.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.rb_collect.restype = C.c_long
        L.rb_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rb_find_closest.restype = C.c_long
        L.rb_find_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        L.rb_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rb_range.restype = C.c_long
        L.rb_range.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_long]
        _lib = L
    return _lib


class RefForest:
    """the reference's BkdTree over one case, compared with the model as the script goes"""

    def __init__(self):
        self.L = ref_lib()
        self.keep = []          # the stores the (never destroyed) forests point into

    def start(self, case):
        self.store = case.P.copy()
        self.keep.append(self.store)
        self.n = case.ctor
        self.h = self.L.rb_new_pts(self.store.ctypes.data, case.ctor, case.b) if case.ctor else self.L.rb_new(case.b)

    def insert(self, pts):
        for _ in range(len(pts)):
            self.L.rb_insert(self.h, self.store[self.n:].ctypes.data)
            self.n += 1

    def remove(self, pts):
        out = []
        for p in pts:
            p = np.ascontiguousarray(p)
            out.append(int(self.L.rb_remove(self.h, p.ctypes.data)))
        return out

    def layout(self):
        buf = C.create_string_buffer(1 << 16)
        self.L.rb_info(self.h, buf, len(buf))
        text = buf.value.decode()
        fill = int(re.search(r"Buffer \[(\d+)/", text).group(1))
        counts = [int(x) for x in re.findall(r"Tree \d+: (\d+) pts", text)]
        ids = np.zeros(sum(counts) + fill + 8, np.int64)
        n = self.L.rb_collect(self.h, self.store.ctypes.data, ids.ctypes.data)
        assert n == sum(counts) + fill == self.L.rb_size(self.h), (n, counts, fill)
        ids = ids[:n].tolist()
        per, a = [], 0
        for c in counts:
            per.append(sorted(ids[a:a + c]))
            a += c
        return counts, per, ids[a:]

    def check_layout(self, case, m, i):
        counts, per, buf = self.layout()
        mc, mp, mb = m.layout()
        assert counts == mc and buf == mb, (case.name, i, counts, mc, buf, mb)
        if case.ties:       # copies: which of them went is free, where they are is not
            key = lambda ids: sorted(map(tuple, m.xyz[ids].tolist()))       # noqa: E731
            assert [key(x) for x in per] == [key(x) for x in mp], (case.name, i)
        else:
            assert per == mp, (case.name, i)

    def check_queries(self, case, m, i, out):
        pre = "%s_q%d_" % (case.name, i)
        L, xyz = self.L, m.xyz
        tmp = np.zeros((len(xyz) + 8, 3))
        for qi, q in enumerate(case.Q):
            q = np.ascontiguousarray(q)
            for j, md in enumerate(case.md2):
                got = int(L.rb_find_closest(self.h, q.ctypes.data, md, self.store.ctypes.data))
                d2, adm = m.find_closest(q, md)
                if got < 0:
                    assert not adm, (case.name, i, qi, md)
                else:
                    assert bkd_model.dist2(xyz[got], q)[0] == d2, (case.name, i, qi, md, got, adm)
                    if len(adm) == 1:
                        assert got == adm[0], (case.name, i, qi, md, got, adm)
                    else:
                        assert tuple(xyz[got]) in {tuple(xyz[a]) for a in adm}, (case.name, i, qi, md, got, adm)
            for k in case.ks:
                n = L.rb_knn(self.h, q.ctypes.data, k, tmp.ctypes.data)
                d, tied = m.knn(q, k)
                assert n == len(d), (case.name, i, qi, k, n, len(d))
                assert np.array_equal(bkd_model.dist2(tmp[:n], q), d), (case.name, i, qi, k)
                for row, t in zip(tmp[:n], tied):
                    assert tuple(row) in {tuple(xyz[a]) for a in t}, (case.name, i, qi, k)
            for j, r2 in enumerate(case.r2):
                n = L.rb_range(self.h, q.ctypes.data, r2, tmp.ctypes.data, len(tmp))
                want = m.fixed_range(q, r2)
                assert n == len(want), (case.name, i, qi, r2, n, len(want))
                assert sorted(map(tuple, tmp[:n].tolist())) == sorted(map(tuple, xyz[want].tolist())), (case.name, i, qi, r2)


def compute(with_ref=None):
    """every array of the fixture; with_ref (default: where the checkout is) asserts reference == model on the way"""
    if with_ref is None:
        with_ref = have_ref()
    out = {}
    stats = {"q1": 0, "removed": 0, "unmatched": 0, "ref_cases": 0}
    ref = RefForest() if with_ref else None
    for case in cases():
        use = ref if (ref and case.ref) else None
        compute_case(case, out, stats, use)
        stats["ref_cases"] += use is not None
    check_not_vacuous(out, stats)
    return out, stats


def check_not_vacuous(out, stats):
    assert stats["q1"] > 100, stats            # Q1 answers: a buffer point beyond maxdist2
    assert stats["removed"] > 400 and stats["unmatched"] > 10, stats
    lat = "lattice_b3_q2_"
    # (-1,0,0) at maxdist2 = 1: (0,0,0) at exactly 1 is not found; the answer is a buffer point at 16 + 0 + 0 or further
    assert out[lat + "fc0_d2"][0] > 1.0
    # (3,1,0) at r2 = 1: (3,0,0) of the buffer (id 27) is in the list, (2,1,0) of a tree (id 21) is not
    o = out[lat + "rng0_off"]
    l1 = out[lat + "rng0_ids"][o[1]:o[2]].tolist()
    assert 27 in l1 and 21 not in l1, l1


def save(z, path=OUT):
    """np.savez_compressed with nothing in the file that depends on when it was written"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k in sorted(z):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(z[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


def load(path=OUT):
    return dict(np.load(path))


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/bkd.cc, kd.cc, searchTree.cc)" % REF)
    z, stats = compute(True)
    save(z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes); %s" % (OUT, len(z), size, stats))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:8]:
        print("  %-40s %s %s" % (k, z[k].dtype, z[k].shape))
    assert size <= MAX_BYTES, size
