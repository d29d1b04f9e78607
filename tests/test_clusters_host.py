"""Radius clustering (tdtk_cluster_radius): the CPU tier.  The per-lane device code (3dtk_amd/csrc/cluster_lane.h) compiled
for the host runs over kd_build.cpp's host tree against the fixture k15_clusters.npz, in several item orders and under loads
that return stale values; the fixture against the live reference; the evidence for the deviation from
segment_colliding.cc's bookkeeping; the exports and the resource remarks of the k_cluster kernels."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import host_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mg():
    spec = importlib.util.spec_from_file_location("make_golden_clusters", os.path.join(G, "make_golden_clusters.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fx(mg):
    return np.load(mg.OUT)


# ---- the per-lane device code on the host --------------------------------------------------------------------------------
# The atomic shims, then cluster_lane.h as it stands.  Every cell of parent[] keeps its history.  With `stale` set the
# relaxed load returns a randomly chosen EARLIER value of the cell (seeded), the CAS acts on the current value and returns
# it: what a lane on another XCD may see of a cell inside one launch, executed where it can be reproduced.  The steps behind
# the link step run behind a launch boundary on the device and read current values here.
_HOST_LANE = r"""
#define __HIP_MEMORY_SCOPE_AGENT 0
struct ParentShim {
  const uint32_t* base = nullptr; size_t n = 0; bool stale = false; uint64_t rng = 1;
  std::vector<std::vector<uint32_t>> hist;
  uint64_t stale_reads = 0;
  bool owns(const uint32_t* p) const { return base && p >= base && p < base + n; }
  void record(const uint32_t* p, uint32_t v) { if (owns(p)) hist[p - base].push_back(v); }
  uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
};
static ParentShim g_ps;
static inline uint32_t __hip_atomic_load(const uint32_t* p, int, int) {
  if (g_ps.stale && g_ps.owns(p)) {
    const std::vector<uint32_t>& h = g_ps.hist[p - g_ps.base];
    const uint32_t v = h[g_ps.next() % h.size()];
    if (v != *p) ++g_ps.stale_reads;
    return v;
  }
  return *p;
}
static inline void __hip_atomic_store(uint32_t* p, uint32_t v, int, int) { *p = v; g_ps.record(p, v); }
static inline uint32_t atomicCAS(uint32_t* p, uint32_t cmp, uint32_t v) {
  const uint32_t o = *p; if (o == cmp) { *p = v; g_ps.record(p, v); } return o;
}
static inline uint32_t atomicMin(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
#include "cluster_lane.h"

// order [n]: the slots in the order their link items run.  Returns n_clusters; stale_reads: loads that returned an old value
extern "C" long hc_cluster(void* tp, double r2, const uint8_t* subset, const double* normals, double min_cos, uint32_t min_size,
                           const int64_t* order, int stale, uint64_t seed, int32_t* labels, int32_t* first, uint32_t* sizes,
                           uint64_t* stale_reads) {
  HostTree& T = *(HostTree*)tp;
  const size_t n = T.pts.size();
  std::vector<uint32_t> parent(n), ckey(n), csize(n), cflag(n + 1, 0u), cnum(n + 1, 0u);
  QueryArgs a = host_args(T);
  a.n = n; a.r2 = r2; a.subset = subset; a.cnormals = normals; a.min_cos = min_cos; a.min_size = min_size;
  a.parent = parent.data(); a.ckey = ckey.data(); a.csize = csize.data(); a.cflag = cflag.data(); a.cnum = cnum.data();
  a.labels = labels; a.cfirst = first; a.csizes_out = sizes;
  for (size_t s = 0; s < n; s++) cluster_init_item(a, (uint32_t)s);
  g_ps = ParentShim();
  g_ps.base = parent.data(); g_ps.n = n; g_ps.stale = stale != 0; g_ps.rng = seed * 2 + 1;
  g_ps.hist.resize(n);
  for (size_t s = 0; s < n; s++) g_ps.hist[s].push_back((uint32_t)s);
  HostStack st;
  if (r2 > 0) for (size_t i = 0; i < n; i++) cluster_link_item(a, (uint32_t)order[i], st);
  if (stale_reads) *stale_reads = g_ps.stale_reads;
  // every value a cell ever held is <= its index and, once hooked, below it
  for (size_t s = 0; s < n; s++)
    for (size_t k = 0; k < g_ps.hist[s].size(); k++)
      if (g_ps.hist[s][k] > s || (k > 0 && g_ps.hist[s][k] >= s)) return -1;
  g_ps.stale = false;
  for (size_t s = 0; s < n; s++) cluster_flatten_item(a, (uint32_t)s);
  for (size_t s = 0; s < n; s++) cluster_flag_item(a, (uint32_t)s);
  uint32_t run = 0;
  for (size_t i = 0; i <= n; i++) { cnum[i] = run; run += cflag[i]; }
  for (size_t s = 0; s < n; s++) cluster_label_item(a, (uint32_t)s);
  g_ps = ParentShim();
  return (long)cnum[n];
}
"""


@pytest.fixture(scope="module")
def hl(tmp_path_factory):
    L = host_lane.build(_HOST_LANE, tmp_path_factory.mktemp("hc"), "hc")
    vp = C.c_void_p
    L.hc_cluster.restype = C.c_long
    L.hc_cluster.argtypes = [vp, C.c_double, vp, vp, C.c_double, C.c_uint32, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]
    return L


def _orders(n):
    """ascending, descending and three random orders of the items"""
    out = [np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)[::-1].copy()]
    for seed in (11, 12, 13):
        out.append(np.random.default_rng(seed).permutation(n).astype(np.int64))
    return out


def _run(L, h, n, r2, order, stale, seed=1, subset=None, normals=None, min_cos=0.0, min_size=1):
    labels = np.full(n, -7, np.int32)
    first = np.full(n, -7, np.int32)
    sizes = np.zeros(n, np.uint32)
    sr = C.c_uint64(0)
    sub = None if subset is None else np.ascontiguousarray(subset, np.uint8)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    k = L.hc_cluster(h, float(r2), None if sub is None else sub.ctypes.data, None if nrm is None else nrm.ctypes.data,
                     float(min_cos), int(min_size), order.ctypes.data, int(stale), seed, labels.ctypes.data, first.ctypes.data,
                     sizes.ctypes.data, C.byref(sr))
    assert k >= 0, "a parent cell held a value above its index, or its own index after it was hooked"
    return labels, k, first[:k], sizes[:k], int(sr.value)


def _check(mg, want, got, key):
    labels, k, first, sizes, _ = got
    assert np.array_equal(labels, want), key
    n, wf, ws = mg.of_labels(want)
    assert k == n and np.array_equal(first, wf) and np.array_equal(sizes, ws), key


def _small_and_chains(mg, fx):
    """(key, points, bucket, r2, expected labels or None where the fixture holds a CRC)"""
    for key, pts, b, r2 in mg.small_cases():
        yield key, pts, b, r2, fx[key + "_labels"]
    for key, name, b, r2, kw in mg.large_cases():
        if name.startswith("chains"):
            yield key, mg.large_cloud(name), b, r2, None


def test_device_lane_code_on_the_host_equals_the_fixture_in_every_order(mg, fx, hl):
    """every small case and both chains, five item orders each, with current and with stale loads"""
    trees, n_cases, stale_total = {}, 0, 0
    for key, pts, b, r2, want in _small_and_chains(mg, fx):
        pts = np.ascontiguousarray(pts)
        tk = (re.sub(r"_b\d+_r\d+$", "", key), b)
        if tk not in trees:
            trees[tk] = hl.host_tree_create(pts.ctypes.data, len(pts), b)
            assert trees[tk]
        for o, order in enumerate(_orders(len(pts))):
            for stale in (0, 1):
                got = _run(hl, trees[tk], len(pts), r2, order, stale, seed=100 * o + 7)
                if want is not None:
                    _check(mg, want, got, (key, o, stale))
                else:
                    assert got[1] == int(fx[key + "_n"][0]) and int(mg.crc(got[0])[0]) == int(fx[key + "_crc"][0]), (key, o, stale)
                    assert got[3].max() == int(fx[key + "_max"][0])
                stale_total += got[4] if stale else 0
        n_cases += 1
    for h in trees.values():
        hl.host_tree_destroy(h)
    assert n_cases == 6 * 3 * 3 + 3 * 2 + 2
    assert stale_total > 10_000          # the stale runs did read old values


def test_chains_are_two_long_paths_under_a_random_numbering(mg, fx):
    pts = mg.chains_cloud()
    assert len(pts) == 5000 and int(fx["chains_n"][0]) == 2 and int(fx["chains_max"][0]) == 2500
    assert int(fx["chains_bridge_n"][0]) == 1 and int(fx["chains_bridge_max"][0]) == 5001
    assert len(mg.chains_cloud(True)) == 5001


def test_subset_normals_and_min_size_on_the_host(mg, fx, hl):
    """the predicates of the emitter and the renumbering: mix with every third point masked out (the fixture's labels come
    from a reference tree over the kept points alone), mix with min_size, and the crossing planes with and without normals"""
    mix = np.ascontiguousarray(mg.mix_cloud())
    planes, nrm = mg.normals_cloud()
    h = hl.host_tree_create(mix.ctypes.data, len(mix), 20)
    hp = hl.host_tree_create(planes.ctypes.data, len(planes), 20)
    asc, rnd = _orders(len(mix))[0], _orders(len(mix))[3]
    for stale, order in ((0, asc), (1, rnd)):
        for j, r2 in enumerate(mg.MIX_R2):
            for key, kw in (("mix_r%d" % j, {}), ("mix_r%d_subset" % j, {"subset": mg.mix_subset()})):
                labels, k, first, sizes, _ = _run(hl, h, len(mix), r2, order, stale, **kw)
                assert k == int(fx[key + "_n"][0]) and int(mg.crc(labels)[0]) == int(fx[key + "_crc"][0]), (key, stale)
                n2, f2, s2 = mg.of_labels(labels)
                assert k == n2 and np.array_equal(first, f2) and np.array_equal(sizes, s2), (key, stale)
                if kw:
                    assert (labels[~mg.mix_subset()] == -1).all() and (labels[mg.mix_subset()] >= 0).all()
        key = "mix_r0_min%d" % mg.MIX_MIN_SIZE
        labels, k, first, sizes, _ = _run(hl, h, len(mix), mg.MIX_R2[0], order, stale, min_size=mg.MIX_MIN_SIZE)
        assert k == int(fx[key + "_n"][0]) and int(mg.crc(labels)[0]) == int(fx[key + "_crc"][0])
        assert sizes.min() >= mg.MIX_MIN_SIZE and (labels == -1).any() and (np.diff(first) > 0).all()
        porder = _orders(len(planes))[3 if stale else 0]
        for key, kw in (("normals_plain", {}), ("normals_cos10", {"normals": nrm, "min_cos": mg.NORMALS_COS})):
            labels, k, first, sizes, _ = _run(hl, hp, len(planes), mg.NORMALS_R2, porder, stale, **kw)
            assert k == int(fx[key + "_n"][0]) and int(mg.crc(labels)[0]) == int(fx[key + "_crc"][0]), key
    hl.host_tree_destroy(h)
    hl.host_tree_destroy(hp)
    assert int(fx["normals_plain_n"][0]) == 1 and int(fx["normals_cos10_n"][0]) >= 2


def test_a_nan_normal_gives_no_edge_and_a_radius_of_zero_no_walk(mg, hl):
    pts = np.ascontiguousarray(mg.k8_clouds()["uniform"][0])
    h = hl.host_tree_create(pts.ctypes.data, len(pts), 5)
    order = _orders(len(pts))[0]
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    plain = _run(hl, h, len(pts), 36.0, order, 0)
    assert plain[1] == 1
    same = _run(hl, h, len(pts), 36.0, order, 0, normals=nrm, min_cos=1.0)
    assert np.array_equal(same[0], plain[0])
    nrm[10] = np.nan
    cut = _run(hl, h, len(pts), 36.0, order, 0, normals=nrm, min_cos=0.0)
    assert cut[1] == 2 and cut[0][10] == 1 and list(cut[2]) == [0, 10] and list(cut[3]) == [len(pts) - 1, 1]
    for r2 in (0.0, -1.0):
        labels, k, first, sizes, _ = _run(hl, h, len(pts), r2, order, 0)
        assert k == len(pts) and np.array_equal(labels, np.arange(len(pts))) and (sizes == 1).all()
    hl.host_tree_destroy(h)


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_fixture_equals_the_reference(mg):
    """every array from a fresh run over the reference's library"""
    if not mg.have_ref():
        pytest.skip("no reference library (oracle/_ref/libref3dtk.so)")
    z = np.load(mg.OUT)
    got, stats = mg.compute()
    mg.check_not_vacuous(stats)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key]), key


def test_fixture_shapes(mg, fx):
    n = 0
    for key, pts, b, r2 in mg.small_cases():
        labels = fx[key + "_labels"]
        assert labels.dtype == np.int32 and labels.shape == (len(pts),) and labels.min() >= 0
        k, first, sizes = mg.of_labels(labels)
        assert (np.diff(first) > 0).all() and sizes.sum() == len(pts) and first[0] == 0
        n += 1
    assert n == 6 * 3 * 3 + 3 * 2
    for b in mg.BUCKETS:
        # '<' is strict: at sqRad2 = 1 the unit lattice is all singletons, one ulp above it is one component
        assert fx["lattice16_b%d_r0_labels" % b].max() == 4095 and fx["lattice16_b%d_r1_labels" % b].max() == 0
    assert [int(fx["mix_r%d_n" % j][0]) for j in range(3)] == [4789, 1252, 1]
    assert [int(fx["mix_r%d_max" % j][0]) for j in range(3)] == [259, 16633, 20000]
    assert int(fx["deep_b1_crc"][0]) == int(fx["deep_b20_crc"][0])          # the bucket size does not matter
    assert int(fx["table_max"][0]) >= 40_000
    assert os.path.getsize(mg.OUT) < 200_000


def test_labels_do_not_depend_on_the_bucket_size(mg, fx):
    for name in mg.SMALL:
        for j in range(3):
            a = [fx["%s_b%d_r%d_labels" % (name, b, j)] for b in mg.BUCKETS]
            assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2]), (name, j)


def test_segment_colliding_bookkeeping_loses_members(mg, fx):
    """the recorded evidence for the deviation include/tdtk_hip.h states: segment_colliding.cc:55-102 restated line for
    line, over the same lists (the reference's own where its library is here, else Dist2 < sqRad2 in ascending order), does
    not leave the components of its own relation on the `uniform` cloud: line 77 clears the list line 76 has just appended
    to when the neighbour is the point itself, and line 100 clears group2points[it], indexed by a point, where the merged
    group was meant"""
    pts = np.ascontiguousarray(mg.k8_clouds()["uniform"][0])
    r2 = mg.SMALL_R2["uniform"][1]
    want = fx["uniform_b20_r1_labels"]
    if mg.have_ref():
        lists = mg.ref_lists(pts, 20, r2)
    else:
        d = pts[:, None, :] - pts[None, :, :]
        near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < r2
        lists = [np.flatnonzero(row) for row in near]
    # the lists are the relation the fixture's components are made of
    ei = np.concatenate([np.full(len(l), i) for i, l in enumerate(lists)])
    ej = np.concatenate(lists)
    assert np.array_equal(mg.canonical(mg.components(len(pts), ei, ej))[0], want)
    true_groups = sorted(tuple(np.flatnonzero(want == c)) for c in range(want.max() + 1))
    for shuffle in (False, True):
        ls = lists
        if shuffle:
            rng = np.random.default_rng(5)
            ls = [rng.permutation(l) for l in lists]
        g2p, p2g = mg.segment_colliding_loop(len(pts), ls)
        groups = sorted(tuple(sorted(set(g))) for g in g2p if len(g))
        assert groups != true_groups
        # members are lost: the groups that are written out do not even cover the cloud
        assert len(set().union(*[set(g) for g in g2p])) < len(pts)
        # and point2group is no partition into the components either
        assert len(set(p2g)) != len(true_groups) or any(len({p2g[i] for i in g}) != 1 for g in true_groups)


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_header_exports_and_mirror_name_the_entry_point(tdtk):
    from importlib import import_module
    capi = import_module("3dtk_amd._capi")
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    so = os.path.join(ROOT, "3dtk_amd", "lib3dtk_hip.so")
    nm = subprocess.run(["nm", "-D", so], capture_output=True, text=True).stdout if os.path.exists(so) else None
    for sym in ("tdtk_cluster_radius", "tdtk_cluster_grid_cap"):
        assert sym in capi.EXPORTS
        assert re.search(r"\bint %s\(" % sym, hdr), sym
        if nm is not None:
            assert re.search(r" T %s$" % sym, nm, re.M), sym
    assert hasattr(tdtk.KDtree, "clusters") and hasattr(tdtk, "segment_colliding")
    # the header states the relation, the numbering, the deviation with its two lines, and whose the normals predicate is
    text = " ".join(hdr.split())
    for phrase in ("Dist2(p_i, p_j) < sqRad2", "smallest member index", "line 77", "line 100", "segment_colliding.cc:55-102",
                   "THIS LIBRARY'S OWN"):
        assert phrase in text, phrase


def test_rejections_need_no_device(tdtk):
    """checked before anything is launched or written: NULL tree, labels or n_clusters"""
    L = tdtk.lib()
    labels = np.full(4, -7, np.int32)
    n = C.c_uint64(99)
    assert L.tdtk_cluster_radius(None, 1.0, None, None, 0.0, 1, labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n), None,
                                 None) == -1
    assert (labels == -7).all() and n.value == 99


def test_cluster_kernels_spill_nothing():
    """no spills; the link kernel has the scratch every walking kernel of query.hip has (the call frame of the lane stack's
    out-of-line overflow path, k_range_count's figure), the passes without a walk none"""
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "query.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (query.resource.txt is written by the Makefile)")
    all_blocks = open(path).read().split("remark: Function Name: ")[1:]

    def scratch(b):
        return int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))

    frame = [scratch(b) for b in all_blocks if "k_range_count" in b.split()[0]]
    assert len(frame) == 1
    blocks = [b for b in all_blocks if "k_cluster" in b.split()[0]]
    names = [b.split()[0] for b in blocks]
    assert sum("k_cluster_link" in n for n in names) == 1 and sum("k_cluster_pass" in n for n in names) == 4, names
    for b in blocks:
        name = b.split()[0]
        for key in ("VGPRs Spill", "SGPRs Spill"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, key)
        assert scratch(b) == (frame[0] if "k_cluster_link" in name else 0), name
