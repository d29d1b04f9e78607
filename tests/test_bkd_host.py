"""The dynamic kd-forest (BkdTree: tdtk_forest_*, 3dtk_amd.BkdTree): the CPU tier.  The model (tests/bkd_model.py) against the
fixture k19_bkd.npz, which tests/golden/make_golden_bkd.py pins to the reference's compiled bkd.cc; the host-only insert plan
(tdtk_forest_plan) against every layout of the fixture; the lane code of forest_lane.h compiled for the host, on kd_build.cpp's
host trees, against the fixture's remove and query cases; the resource remarks of the forest kernels; and the forest's queries
against the tree walks of query_lane.h on the same host tree, which pins that the point policy is all that separates them."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import bkd_model
import host_lane
from bkd_replay import replay, ways

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def mk():
    return _load("make_golden_bkd")


@pytest.fixture(scope="module")
def fx(mk):
    return mk.load()


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_model_equals_the_fixture(mk, fx):
    out = {}
    for case in mk.cases():
        mk.compute_case(case, out)
    assert sorted(out) == sorted(fx)
    for k in out:
        assert out[k].dtype == fx[k].dtype and np.array_equal(out[k], fx[k]), k
    assert os.path.getsize(mk.OUT) <= mk.MAX_BYTES


def test_fixture_equals_the_reference(mk, fx):
    """every case but the 20 000-point one (the generator runs that one too) through the reference's compiled sources"""
    if not mk.have_ref():
        pytest.skip("no reference checkout (src/slam6d/bkd.cc)")
    ref = mk.RefForest()
    n = 0
    for case in mk.cases():
        if not case.ref or len(case.P) > 5000:
            continue
        out = {}
        mk.compute_case(case, out, None, ref)
        for k in out:
            assert np.array_equal(out[k], fx[k]), k
        n += 1
    assert n >= 35


def test_fixture_is_not_vacuous(mk, fx):
    names = {c.name for c in mk.cases()}
    for b in (3, 20):
        for n in mk.layout_totals(b):
            assert "lay_b%d_n%d" % (b, n) in names
    # the cascade through four slots into an appended one: 16b - 1 -> 16b
    assert fx["lay_b3_n47_c1_counts"].tolist() == [3, 6, 12, 24] and len(fx["lay_b3_n47_c1_buf"]) == 2
    assert fx["lay_b3_n48_c1_counts"].tolist() == [0, 0, 0, 0, 48] and len(fx["lay_b3_n48_c1_buf"]) == 0
    # 1003 single inserts at bucket 20
    assert fx["lay_b20_n1003_c1_counts"].tolist() == [0, 40, 0, 0, 320, 640] and len(fx["lay_b20_n1003_c1_buf"]) == 3
    # the constructor's empty slots, and the large tree taken into an appended slot
    assert fx["ctor_b3_n30_c0_counts"].tolist() == [0, 0, 0, 30] and fx["ctor_b3_n30_c5_counts"].tolist() == [0, 0, 0, 0, 54]
    assert fx["ctor_b3_n2_c0_counts"].tolist() == [2]
    # the same point twice: (1, 0) in one call and in two; copies: buffer, slot 0, slot 2, then nothing; two copies in one slot
    assert (fx["rm_basic_b3_r5_id"] >= 0).tolist() == [True, False]
    assert (fx["rm_basic_b3_r6_id"] >= 0).tolist() == [True] and (fx["rm_basic_b3_r7_id"] >= 0).tolist() == [False]
    assert fx["rm_copies_b3_r2_cont"].tolist() == [0, 1, 3, -1] and fx["rm_copies_b3_r4_cont"].tolist() == [3, 3, -1]
    # a slot emptied by removes, the next merge lands in it
    assert fx["rm_empty_slot_b3_c3_counts"].tolist() == [0, 6] and fx["rm_empty_slot_b3_c6_counts"].tolist() == [3, 6]
    # the emptied leaf's tree collected by a later merge
    assert fx["rm_leaf_b3_c3_counts"].tolist() == [0, 0, 9] and fx["rm_leaf_b3_c6_counts"].tolist() == [0, 0, 0, 21]
    # 200 copies, three gone: 197 within the small radius of the copies' own coordinate
    o = fx["degenerate_b20_q4_rng0_off"]
    assert o[1] - o[0] == 197 and (fx["degenerate_b20_q4_knn64_d2"][0] == 0.0).all()
    assert sum(int((v >= 0).sum()) for k, v in fx.items() if k.startswith("mixed_b20_r") and k.endswith("_id")) > 400


# ---- the insert plan -----------------------------------------------------------------------------------------------------
class PlanForest:
    """the forest's bookkeeping driven by tdtk_forest_plan alone: slots and the buffer as id lists"""

    def __init__(self, bkd, b, n_ctor):
        self.bkd, self.b, self.next = bkd, b, n_ctor
        self.buf, self.slots = [], []
        self.merges = 0
        if n_ctor:
            self.slots = [[] for _ in range(bkd_model.ctor_slots(n_ctor, b) - 1)] + [list(range(n_ctor))]

    def insert(self, m):
        counts, segs, (keep, a, b), merges = self.bkd.plan([len(s) for s in self.slots], len(self.buf), self.b, m)
        assert len(counts) == len(segs)
        new = []
        for j, ss in enumerate(segs):
            ids = []
            for kind, x, y in ss:
                if kind == 0:
                    assert len(self.slots[x]) == y
                    ids += self.slots[x]
                elif kind == 1:
                    ids += list(range(self.next + x, self.next + y))
                else:
                    assert y == len(self.buf)
                    ids += self.buf
            assert len(ids) == counts[j]
            new.append(ids)
        self.buf = (self.buf if keep else []) + list(range(self.next + a, self.next + b))
        self.slots = new
        self.next += m
        self.merges += merges

    def remove(self, ids):
        for i in ids:
            for c in [self.buf] + self.slots:
                if i in c:
                    c.remove(i)

    def layout(self):
        return [len(s) for s in self.slots], [x for s in self.slots for x in sorted(s)], list(self.buf)


def test_plan_gives_every_layout_of_the_fixture(tdtk, mk, fx):
    bkd = __import__("importlib").import_module("3dtk_amd.bkd")
    checked = 0
    for case in mk.cases():
        for way in ("one", "single", "ragged") if case.name.startswith("lay_") else ("one",):
            f = PlanForest(bkd, case.b, case.ctor)
            for i, (code, a, b) in enumerate(case.ops):
                if code == mk.INS:
                    for m in dict(ways(mk, case, a, b))[way]:
                        f.insert(m)
                elif code == mk.REM:
                    f.remove([x for x in fx["%s_r%d_id" % (case.name, i)].tolist() if x >= 0])
                elif code == mk.CHK:
                    counts, ids, buf = f.layout()
                    pre = "%s_c%d_" % (case.name, i)
                    assert counts == fx[pre + "counts"].tolist(), (case.name, way, i)
                    assert ids == fx[pre + "ids"].tolist() and buf == fx[pre + "buf"].tolist(), (case.name, way, i)
                    checked += 1
            assert len(f.buf) < case.b
    assert checked > 100
    # 100 000 points into an empty forest at b = 20: 5 000 merges, a handful of slots to build
    counts, segs, buf, merges = bkd.plan([], 0, 20, 100000)
    assert merges == 5000 and sum(counts) == 100000 and buf == (False, 100000, 100000)
    assert sum(1 for c in counts if c) == bin(5000).count("1")
    assert sorted((x, y) for s in segs for kind, x, y in s if kind == 1 or pytest.fail("only new points"))[0][0] == 0
    assert sum(y - x for s in segs for _, x, y in s) == 100000 and all(len(s) <= 1 for s in segs)


def test_plan_refuses_an_impossible_state(tdtk):
    bkd = __import__("importlib").import_module("3dtk_amd.bkd")
    with pytest.raises(tdtk.TdtkError):
        bkd.plan([3], 3, 3, 1)          # a buffer holds fewer than b points
    with pytest.raises(tdtk.TdtkError):
        bkd.plan([], 0, 0, 1)


def test_header_exports_and_mirror_name_the_entry_points(tdtk):
    capi = __import__("importlib").import_module("3dtk_amd._capi")
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    for sym in ("tdtk_forest_create", "tdtk_forest_create_from_points", "tdtk_forest_insert", "tdtk_forest_remove", "tdtk_forest_info",
                "tdtk_forest_collect", "tdtk_forest_find_closest", "tdtk_forest_knn", "tdtk_forest_fixed_range", "tdtk_forest_plan"):
        assert sym in capi.EXPORTS and hasattr(tdtk.lib(), sym)
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    assert "tdtk_forest_destroy" in capi.EXPORTS
    for m in ("insert", "remove", "size", "info", "collectPts", "FindClosest", "kNearestNeighbors", "fixedRangeSearch"):
        assert hasattr(tdtk.BkdTree, m)


def test_forest_kernels_spill_nothing():
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "forest.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (forest.resource.txt is written by the Makefile)")
    blocks = [b for b in open(path).read().split("remark: Function Name: ")[1:] if "k_forest" in b.split()[0]]
    assert len(blocks) >= 13, [b.split()[0] for b in blocks]
    for b in blocks:
        for key in ("VGPRs Spill", "SGPRs Spill"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (b.split()[0], key)


# ---- the lane code on the host -----------------------------------------------------------------------------------------------
# forest_lane.h as it stands under host_lane_shim.h, over kd_build.cpp's host trees: a slot is built over the points handed to
# it (live and, behind them in the bookkeeping below, removed ones), relabelled with the forest ids, the removed ones marked
_HOST_FOREST = r"""
#include "forest_lane.h"
struct HF { std::vector<HostTree*> trees; std::vector<KdPoint> buf; ForestArgs a; };
extern "C" void* hf_create(int bucket, int nslots, const long* off, const double* xyz, const int* ids, int nbuf, const double* bxyz,
                           const int* bids) {
  HF* h = new HF; h->a = ForestArgs{}; h->a.nslots = nslots;
  for (int s = 0; s < nslots; s++) {
    const long n = off[s + 1] - off[s];
    HostTree* T = nullptr;
    if (n) {
      T = new HostTree; std::string err;
      if (!build_tree(xyz + 3 * off[s], (size_t)n, bucket, *T, err)) return nullptr;
      for (KdPoint& p : T->pts) { p.orig = ids[off[s] + p.orig]; p.pad = FOREST_UNCLAIMED; }     // (ids: -1 where the point was removed)
      ForestSlot& d = h->a.slot[s];
      d.nodes = T->nodes.data(); d.pts = T->pts.data(); d.leaf_tab = T->table_mode ? T->leaf_tab.data() : nullptr;
      d.root_ref = T->root_ref; d.cb = T->cb; d.cmask = (1u << T->cb) - 1; d.n = (uint32_t)n;
    }
    h->trees.push_back(T);
  }
  for (int i = 0; i < nbuf; i++) { KdPoint p; p.x = bxyz[3 * i]; p.y = bxyz[3 * i + 1]; p.z = bxyz[3 * i + 2]; p.orig = bids[i]; p.pad = 0; h->buf.push_back(p); }
  h->a.buf = h->buf.data(); h->a.nbuf = (uint32_t)nbuf;
  return h;
}
extern "C" void hf_destroy(void* p) { HF* h = (HF*)p; for (HostTree* t : h->trees) delete t; delete h; }
extern "C" void hf_closest(void* p, const double* q, int nq, double md2, int* id, double* d2) {
  HF* h = (HF*)p;
  for (int i = 0; i < nq; i++) { HostStack st; forest_find_closest(h->a, q[3 * i], q[3 * i + 1], q[3 * i + 2], md2, st, id[i], d2[i]); }
}
extern "C" void hf_knn(void* p, const double* q, int nq, int k, int* ids, double* d2) {
  HF* h = (HF*)p;
  std::vector<double> ld(k); std::vector<uint32_t> ls(k);
  for (int i = 0; i < nq; i++) {
    ListLds<1> L; L.ld = ld.data(); L.ls = ls.data(); L.init(k);
    HostStack st;
    forest_knn(h->a, q[3 * i], q[3 * i + 1], q[3 * i + 2], L, st);
    for (int j = 0; j < k; j++) { const bool v = L.dist(j) >= 0.0; ids[i * k + j] = v ? (int)L.slot(j) : -1; d2[i * k + j] = v ? L.dist(j) : -1.0; }
  }
}
extern "C" long hf_range(void* p, const double* q, int nq, double r2, long* off, int* ids, long cap) {
  HF* h = (HF*)p;
  long w = 0;
  for (int i = 0; i < nq; i++) {
    off[i] = w;
    auto emit = [&](int32_t id, double) { if (w < cap) ids[w] = id; ++w; };
    HostStack st;
    forest_fixed_range(h->a, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, st, emit);
  }
  off[nq] = w;
  return w;
}
extern "C" int hf_remove_find(void* p, const double* q, int* cont) {
  HF* h = (HF*)p;
  HostStack st; int32_t c = -1; uint32_t pos = 0;
  if (!forest_remove_find(h->a, q[0], q[1], q[2], st, c, pos)) { *cont = -1; return -1; }
  *cont = c;
  KdPoint* pt = forest_point(h->a, c, pos);
  const int id = pt->orig;
  pt->orig = FOREST_DEAD;
  return id;
}
"""


class HostForest:
    """the bookkeeping of api_forest.cpp in Python (the plan decides what is rebuilt; a removed point stays in its tree), with
    the lane code of forest_lane.h doing every walk"""

    def __init__(self, L, bkd, case):
        self.L, self.bkd, self.b, self.xyz = L, bkd, case.b, np.zeros((0, 3))
        self.built, self.dead, self.buf, self.h = [], set(), [], None         # built: per slot the ids it was built over
        if case.ctor:
            self.xyz = case.P[:case.ctor].copy()
            self.built = [[] for _ in range(bkd_model.ctor_slots(case.ctor, case.b) - 1)] + [list(range(case.ctor))]

    def live(self, s):
        return [i for i in self.built[s] if i not in self.dead]

    def insert(self, pts):
        first = len(self.xyz)
        self.xyz = np.concatenate([self.xyz, pts])
        counts, segs, (keep, a, b), _ = self.bkd.plan([len(self.live(s)) for s in range(len(self.built))], len(self.buf), self.b, len(pts))
        new = []
        for j, ss in enumerate(segs):
            if ss == [(0, j, counts[j])]:
                new.append(self.built[j])          # untouched: removed points and all
                continue
            ids = []
            for kind, x, y in ss:
                ids += self.live(x) if kind == 0 else list(range(first + x, first + y)) if kind == 1 else self.buf
            new.append(ids)
        self.buf = (self.buf if keep else []) + list(range(first + a, first + b))
        self.built = new
        self.close()

    def handle(self):
        if self.h is None:
            off = np.concatenate([[0], np.cumsum([len(s) for s in self.built])]).astype(np.int64)
            flat = np.array([i for s in self.built for i in s], np.int64)
            ids = np.where(np.isin(flat, list(self.dead)), -1, flat).astype(np.int32) if len(flat) else np.zeros(0, np.int32)
            xyz = np.ascontiguousarray(self.xyz[flat]) if len(flat) else np.zeros((0, 3))
            bids = np.array(self.buf, np.int32)
            bxyz = np.ascontiguousarray(self.xyz[self.buf]) if self.buf else np.zeros((0, 3))
            self.keep = (off, ids, xyz, bids, bxyz)
            self.h = self.L.hf_create(self.b, len(self.built), off.ctypes.data, xyz.ctypes.data, ids.ctypes.data, len(bids),
                                      bxyz.ctypes.data, bids.ctypes.data)
            assert self.h
        return self.h

    def close(self):
        if self.h is not None:
            self.L.hf_destroy(self.h)
            self.h = None

    def remove(self, pts):
        out, conts = [], []
        for p in np.ascontiguousarray(pts):
            c = C.c_int(0)
            i = self.L.hf_remove_find(self.handle(), p.ctypes.data, C.byref(c))
            out.append(i)
            conts.append(c.value)
            if i >= 0:
                self.dead.add(i)
                if c.value == 0:
                    self.buf.remove(i)
                    self.close()
                elif not self.live(c.value - 1):
                    self.built[c.value - 1] = []       # a tree whose count reaches 0 becomes an empty slot
                    self.close()
        return out, conts

    def layout(self):
        return ([len(self.live(s)) for s in range(len(self.built))], [x for s in range(len(self.built)) for x in sorted(self.live(s))],
                list(self.buf))

    def find_closest(self, Q, md2):
        idx, d2 = np.empty(len(Q), np.int32), np.empty(len(Q))
        self.L.hf_closest(self.handle(), Q.ctypes.data, len(Q), md2, idx.ctypes.data, d2.ctypes.data)
        return idx, d2

    def knn(self, Q, k):
        idx, d2 = np.empty((len(Q), k), np.int32), np.empty((len(Q), k))
        self.L.hf_knn(self.handle(), Q.ctypes.data, len(Q), k, idx.ctypes.data, d2.ctypes.data)
        return idx, d2

    def fixed_range(self, Q, r2):
        off = np.zeros(len(Q) + 1, np.int64)
        cap = 64 * len(Q) + 64
        while True:
            ids = np.empty(cap, np.int32)
            n = self.L.hf_range(self.handle(), Q.ctypes.data, len(Q), r2, off.ctypes.data, ids.ctypes.data, cap)
            if n <= cap:
                return off, ids[:n]
            cap = n


def test_lane_code_compiled_for_the_host_equals_the_fixture(tdtk, mk, fx, tmp_path):
    bkd = __import__("importlib").import_module("3dtk_amd.bkd")
    L = host_lane.build(_HOST_FOREST, tmp_path, "hf")
    L.hf_create.restype = C.c_void_p
    L.hf_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.hf_destroy.argtypes = [C.c_void_p]
    L.hf_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    L.hf_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hf_range.restype = C.c_long
    L.hf_range.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_long]
    L.hf_remove_find.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    n = 0
    for case in mk.cases():
        if len(case.P) > 5000:
            continue        # (the 20 000-point case: the GPU tier's)
        f = HostForest(L, bkd, case)
        replay(mk, case, fx, f)
        f.close()
        n += 1
    assert n >= 36


# ---- the forest's queries are the tree walks under the point policy --------------------------------------------------------------
# One host tree as a forest of one slot with an empty buffer, beside the same tree as QueryArgs: forest_knn / forest_fixed_range /
# forest_find_closest of forest_lane.h against knn_walk / range_walk of query_lane.h under the default policy, the slots mapped
# through orig.  kd_build.cpp packs the leaves of a cloud this small; `table` re-encodes the leaf references as leaf ids, as the
# build does where start and count do not fit in 30 bits.
_HOST_PAIR = r"""
#include "forest_lane.h"
struct HP { HostTree T; std::vector<int32_t> orig; ForestArgs f; };
extern "C" void* hp_create(const double* xyz, int n, int bucket, int table) {
  HP* h = new HP; std::string err;
  if (!build_tree(xyz, (size_t)n, bucket, h->T, err) || h->T.table_mode) return nullptr;
  HostTree& T = h->T;
  if (table) {
    auto by_id = [&](uint32_t ref) -> uint32_t {
      if (!(ref & REF_LEAF)) return ref;
      const uint32_t start = (ref & REF_VAL) >> T.cb;
      for (uint32_t id = 0; id < T.leaf_tab.size(); id++)
        if ((uint32_t)T.leaf_tab[id].start == start) return (ref & (REF_LEAF | REF_AXIS)) | id;
      abort();
    };
    T.root_ref = by_id(T.root_ref);
    for (KdNode& nd : T.nodes) { nd.c1 = by_id(nd.c1); nd.c2 = by_id(nd.c2); }
    T.table_mode = true;
  }
  for (KdPoint& p : T.pts) { h->orig.push_back(p.orig); p.pad = FOREST_UNCLAIMED; }
  h->f = ForestArgs{}; h->f.nslots = 1;
  ForestSlot& d = h->f.slot[0];
  d.nodes = T.nodes.data(); d.pts = T.pts.data(); d.leaf_tab = table ? T.leaf_tab.data() : nullptr;
  d.root_ref = T.root_ref; d.cb = T.cb; d.cmask = (1u << T.cb) - 1; d.n = (uint32_t)n;
  return h;
}
extern "C" void hp_destroy(void* p) { delete (HP*)p; }
// dead [n] by input index: the forest sees the point removed; the tree walks below do not look at orig
extern "C" void hp_mark_dead(void* p, const unsigned char* dead) {
  HP* h = (HP*)p;
  for (size_t s = 0; s < h->T.pts.size(); s++) h->T.pts[s].orig = dead[h->orig[s]] ? FOREST_DEAD : h->orig[s];
}
extern "C" void hp_knn(void* p, int forest, const double* q, int nq, int k, int* ids, double* d2) {
  HP* h = (HP*)p;
  QueryArgs a = host_args(h->T);
  std::vector<double> ld(k); std::vector<uint32_t> ls(k);
  for (int i = 0; i < nq; i++) {
    ListLds<1> L; L.ld = ld.data(); L.ls = ls.data(); L.init(k);
    HostStack st;
    if (forest) forest_knn(h->f, q[3 * i], q[3 * i + 1], q[3 * i + 2], L, st);
    else knn_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], L, st);
    for (int j = 0; j < k; j++) {
      const bool v = L.dist(j) >= 0.0;
      ids[i * k + j] = !v ? -1 : forest ? (int)L.slot(j) : h->orig[L.slot(j)];
      d2[i * k + j] = v ? L.dist(j) : -1.0;
    }
  }
}
extern "C" long hp_range(void* p, int forest, const double* q, int nq, double r2, long* off, int* ids, double* d2, long cap) {
  HP* h = (HP*)p;
  QueryArgs a = host_args(h->T);
  long w = 0;
  for (int i = 0; i < nq; i++) {
    off[i] = w;
    auto femit = [&](int32_t id, double md) { if (w < cap) { ids[w] = id; d2[w] = md; } ++w; };
    auto temit = [&](const KdPoint&, uint32_t slot, double md) { if (w < cap) { ids[w] = h->orig[slot]; d2[w] = md; } ++w; };
    HostStack st;
    if (forest) forest_fixed_range(h->f, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, st, femit);
    else range_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, st, temit);
  }
  off[nq] = w;
  return w;
}
extern "C" void hp_closest(void* p, const double* q, int nq, double md2, int* id, double* d2) {
  HP* h = (HP*)p;
  for (int i = 0; i < nq; i++) { HostStack st; forest_find_closest(h->f, q[3 * i], q[3 * i + 1], q[3 * i + 2], md2, st, id[i], d2[i]); }
}
"""


class _Pair:
    def __init__(self, L, pts, bucket, table):
        self.L, self.pts = L, np.ascontiguousarray(pts)
        self.h = L.hp_create(self.pts.ctypes.data, len(pts), bucket, int(table))
        assert self.h

    def close(self):
        self.L.hp_destroy(self.h)

    def mark_dead(self, dead):
        dead = np.ascontiguousarray(dead, np.uint8)
        self.L.hp_mark_dead(self.h, dead.ctypes.data)

    def knn(self, forest, Q, k):
        ids, d2 = np.empty((len(Q), k), np.int32), np.empty((len(Q), k))
        self.L.hp_knn(self.h, int(forest), Q.ctypes.data, len(Q), k, ids.ctypes.data, d2.ctypes.data)
        return ids, d2

    def range(self, forest, Q, r2):
        off, cap = np.zeros(len(Q) + 1, np.int64), len(Q) * len(self.pts)
        ids, d2 = np.empty(cap, np.int32), np.empty(cap)
        n = self.L.hp_range(self.h, int(forest), Q.ctypes.data, len(Q), r2, off.ctypes.data, ids.ctypes.data, d2.ctypes.data, cap)
        assert n <= cap
        return off, ids[:n], d2[:n]

    def closest(self, Q, md2):
        ids, d2 = np.empty(len(Q), np.int32), np.empty(len(Q))
        self.L.hp_closest(self.h, Q.ctypes.data, len(Q), md2, ids.ctypes.data, d2.ctypes.data)
        return ids, d2


def _first_minimum(off, ids, d2):
    """per list its first entry of smallest d2 (FindClosest takes a point on strict '<': the first visited wins a tie, and it visits
    the range walk's nodes in the range walk's order), -1 / -1.0 for an empty list"""
    bi, bd = np.full(len(off) - 1, -1, np.int32), np.full(len(off) - 1, -1.0)
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            j = off[i] + int(np.argmin(d2[off[i]:off[i + 1]]))
            bi[i], bd[i] = ids[j], d2[j]
    return bi, bd


def _filtered(off, ids, d2, keep):
    m = keep[ids]
    noff = np.concatenate([[0], np.cumsum([int(m[off[i]:off[i + 1]].sum()) for i in range(len(off) - 1)])]).astype(np.int64)
    return noff, ids[m], d2[m]


def test_forest_queries_are_the_tree_walks_under_the_point_policy(tmp_path):
    mg = _load("make_golden_knn")
    L = host_lane.build(_HOST_PAIR, tmp_path, "hp")
    L.hp_create.restype = C.c_void_p
    L.hp_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.hp_destroy.argtypes = [C.c_void_p]
    L.hp_mark_dead.argtypes = [C.c_void_p, C.c_void_p]
    L.hp_knn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hp_range.restype = C.c_long
    L.hp_range.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.hp_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    clouds = mg.k8_clouds()
    checked = 0
    for name in ("uniform", "duplicates"):
        pts, Q, _, r2 = clouds[name]
        pts, Q = np.ascontiguousarray(pts), np.ascontiguousarray(Q)
        live = np.arange(len(pts)) % 2 == 0                          # every second point goes
        every = np.broadcast_to(np.arange(len(pts)), (len(Q), len(pts)))
        D = np.sort(np.where(live[None, :], mg.dist2(pts, Q[:, None, :], every), np.inf), axis=1)     # the live points by brute force
        for table in (False, True):
            t = _Pair(L, pts, 5, table)
            full = {}
            # nothing removed: the same rows, ids, distances and order
            for k in (1, 10, 33):
                fi, fd = t.knn(True, Q, k)
                ti, td = t.knn(False, Q, k)
                assert np.array_equal(fi, ti) and np.array_equal(fd, td), (name, table, k)
                assert (fi[:, 0] >= 0).all()
                checked += 1
            for rad in (r2, 9.0 * r2):
                full[rad] = t.range(False, Q, rad)
                got = t.range(True, Q, rad)
                assert all(np.array_equal(g, w) for g, w in zip(got, full[rad])), (name, table, rad)
                assert len(full[rad][1]) > len(Q)
                ci, cd = t.closest(Q, rad)
                wi, wd = _first_minimum(*full[rad])
                assert np.array_equal(ci, wi) and np.array_equal(cd, wd), (name, table, rad)
                checked += 1
            # every second point removed: the live subset of the same lists, and nothing else
            t.mark_dead(~live)
            for rad in (r2, 9.0 * r2):
                want = _filtered(*full[rad], live)
                got = t.range(True, Q, rad)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, table, rad)
                assert 0 < len(want[1]) < len(full[rad][1])
                ci, cd = t.closest(Q, rad)
                wi, wd = _first_minimum(*want)
                assert np.array_equal(ci, wi) and np.array_equal(cd, wd), (name, table, rad)
                # the tree walk under the default policy still lists the removed points
                assert all(np.array_equal(g, w) for g, w in zip(t.range(False, Q, rad), full[rad]))
                checked += 1
            for k in (1, 10, 33):
                fi, fd = t.knn(True, Q, k)
                assert (fi >= 0).all() and live[fi].all(), (name, table, k)
                assert np.array_equal(fd, mg.dist2(pts, Q[:, None, :], fi)) and np.array_equal(fd, D[:, :k]), (name, table, k)
                assert all(len(set(r)) == k for r in fi.tolist())
                checked += 1
            t.close()
    assert checked == 2 * 2 * (3 + 2 + 2 + 3)
