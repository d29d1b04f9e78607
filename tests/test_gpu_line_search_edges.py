"""The branches of the search for the point nearest to a line that no other test executes: kd_search_dir in kernels.hip,
launched as k_search<256, 8, false, DIRMODE, ...> by tdtk_find_closest_along_dir (raw directions) and by pairing mode 1 of
tdtk_get_pt_pairs (the normal normalised on the device and rotated into the tree frame).  A lane's second and later trips
through its workgroup's slab, leaf table mode, the stack at full depth on every lane of an 80-level tree, arithmetic where
the reference's answer is an accident of its walk (d < 0 by rounding, non-unit / zero / non-finite directions, non-finite
queries, every odd maxdist2), batch sizes around the launch geometry, the optional d2 and the NULL refusals, degenerate
normals in mode 1, and the order of calls on the context's shared workspaces.

Every comparison of idx and d2 is exact, against the oracle (oracle/oracle.c; tests/test_line_search_reference_host.py pins
it to the reference's compiled tree on these very cases) and also against that tree itself where oracle/_ref travelled.
The inputs come from tests/line_search_cases.py.  Each test first asserts the precondition that makes it reach its branch."""
import ctypes as C

import numpy as np
import pytest

import line_search_cases as L

pytestmark = pytest.mark.gpu
TDTK_EINVAL = -1


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(a, b):
    return a.dtype == b.dtype and L.equal(a, b)


def _check(orc, c, idx, d2, ref_stride=1):
    """the compared rows of a whole-batch answer against the oracle (idx and d2) and the reference tree (idx); returns the
    oracle's (idx, d2) of those rows"""
    rows = slice(None) if c["rows"] is None else c["rows"]
    q, u = L.compared(c)
    oi, od = orc.Tree(c["model"], c["bucket"]).find_closest_along_dir(q, u, c["maxdist2"])
    assert _same(idx[rows], oi), c["name"]
    assert _same(d2[rows], od), c["name"]
    if orc.have_ref():
        s = slice(None, None, ref_stride)
        want = orc.RefTree(c["model"], c["bucket"]).find_closest_along_dir(q[s], u[s], c["maxdist2"])
        assert _same(idx[rows][s], want), c["name"]
    return oi, od


# ---- 1. a lane's second and later trips -----------------------------------------------------------------------------------
def test_more_queries_than_one_per_lane(tdtk, orc, gpu):
    """search_grid() caps the grid at 16 workgroups per CU, search_plain_body gives each ceil(K / nb) sorted queries and
    walks them 256 at a time: with K = 16 CUs 256 + 70,001 every workgroup makes a second trip (per = 274 on 256 CUs), the
    last slabs start beyond K and the one before them is clipped"""
    cu = _cu()
    c = L.trips(cu)
    q, u, md2 = c["q"], c["dirs"], c["maxdist2"]
    K = len(q)
    nb = L.SEARCH_WG_PER_CU * cu
    assert K > nb * L.SEARCH_BLOCK
    per = -(-K // nb)
    assert per > L.SEARCH_BLOCK and (nb - 1) * per >= K      # a second trip everywhere; a last slab with lo >= K
    kd = tdtk.KDtree(c["model"], c["bucket"])
    idx, d2 = kd.FindClosestAlongDirBatch(q, u, md2)
    oi, _ = _check(orc, c, idx, d2)
    hit, miss = L.shares(oi)
    print("trips: K %d, sampled rows %d, with a partner %.3f" % (K, len(oi), hit))
    assert hit >= 0.1 and miss >= 0.1
    hit, miss = L.shares(idx)
    assert hit >= 0.1 and miss >= 0.1
    # batch invariance: 50,000 queries alone are one trip per lane
    assert 50_000 <= nb * L.SEARCH_BLOCK
    for s in (0, (K - 50_000) // 2, K - 50_000):
        i1, d1 = kd.FindClosestAlongDirBatch(q[s:s + 50_000], u[s:s + 50_000], md2)
        assert _same(i1, idx[s:s + 50_000]) and _same(d1, d2[s:s + 50_000]), s
    sh = c["shuffle"]
    i2, dd2 = kd.FindClosestAlongDirBatch(q[sh], u[sh], md2)
    assert _same(i2, idx[sh]) and _same(dd2, d2[sh])


# ---- 2. the stack at full depth on every lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [1, 20])
def test_deep_tree_every_lane_on_the_overflow_stack(tdtk, orc, gpu, bucket):
    """kd_search_dir never prunes by the split plane: it pushes the other child at every inner node it enters, so a query
    stacks the whole root-to-leaf path -- 80 levels here, of which 8 are in LDS.

    Why sp stays inside the overflow area.  kd_build.cpp counts depth from 1 at the root and max_depth is the deepest
    work item's, i.e. the deepest leaf's level D (the device builder reports the same number: kd.verify()).  A walk holds
    at most one entry per inner node on the path to the leaf it is in, that is at most D - 1 entries, pushed at
    sp = 0 .. D - 2.  LaneStack<256, 8>::push sends sp >= 8 to level sp - 8 <= D - 10 of the overflow area, which
    prepare_overflow_in allocates with need = D - 1 - SEARCH_SD_MIN = D - 5 levels (it is sized for the shallowest LDS
    stack of any search kernel, 4) of search_max_lanes(K) >= search_grid(K) x 256 lanes each; the kernel's stride is
    gridDim x 256 and its column blockIdx x 256 + threadIdx.  So the largest offset is below need x lanes."""
    have = orc.have_ref()
    c = L.deep(have, bucket)
    assert len(c["q"]) == (2_400 if have else 300)
    kd = tdtk.KDtree(c["model"], bucket)
    info = kd.info()
    print("deep cloud, bucket %d: max_depth %d" % (bucket, info["max_depth"]))
    assert info["max_depth"] >= 4 * 16 and info["max_depth"] - 1 > L.SEARCH_SD
    assert kd.verify() == [0, 0, 0, 0]
    idx, d2 = kd.FindClosestAlongDirBatch(c["q"], c["dirs"], c["maxdist2"])
    # (far out in the geometric part the reference's walk prunes nothing: 3 to 4 ms per query on the CPU.  The reference
    # library answers every fourth row here, all of them in the host tier.)
    oi, od = _check(orc, c, idx, d2, ref_stride=4)
    ng = len(c["q"]) // 3                                        # deep_queries: the geometric part comes first
    assert (np.abs(c["q"][:ng]).max(1) > 50).sum() > ng // 2 and (oi[:ng] >= 0).sum() > ng // 2
    assert (od < 0).any() and (oi < 0).any()


# ---- 3. leaf table mode ----------------------------------------------------------------------------------------------------
def test_table_mode_lines_through_a_leaf_of_copies(tdtk, orc, gpu):
    c = L.table()
    assert len(c["q"]) <= 2_000
    kd = tdtk.KDtree(c["model"], c["bucket"])
    info = kd.info()
    # kd_build.cpp's packing rule: (start << cb) | count must fit in 30 bits, else the leaves go through leaf_tab
    assert int(info["n_points"]).bit_length() + int(info["max_leaf_points"]).bit_length() > 30
    assert info["max_leaf_points"] >= len(c["copies"]) and kd.verify() == [0, 0, 0, 0]
    idx, d2 = kd.FindClosestAlongDirBatch(c["q"], c["dirs"], c["maxdist2"])
    oi, _ = _check(orc, c, idx, d2)
    assert np.isin(oi[c["through"]], c["copies"]).sum() >= 8         # 40,000 equal d: the first in walk order
    assert (~np.isin(oi[c["beside"]], c["copies"])).sum() >= 8


# ---- 4. arithmetic where the reference's answer is an accident of its walk ---------------------------------------------------
WHOLE = [n for n in L.FIND_CLOSEST_NAMES if n.split("_")[0] in ("on", "directions", "nonfinite", "maxdist2")]


@pytest.mark.parametrize("name", WHOLE)
def test_reference_arithmetic_bit_for_bit(tdtk, orc, gpu, name):
    """on_the_line: d of the point on the line rounds to 0 or below, from then on sqrt(best) is -0 or NaN and the sphere
    test prunes next to nothing or nothing.  directions: used as given (a long one gives d = -huge, NaN compares false
    everywhere, an infinite component gives -inf or NaN); axis-aligned on the lattice: rows of points at the same d, the
    first in walk order wins.  nonfinite_q: NaN / +-inf / 1e160 / -1e200 coordinates pass the counting sort first.
    maxdist2: 0, negative, 1e-300, +inf, 1e300 (lim * lim overflows: every node is entered), NaN."""
    c = L.find_closest_case(name, orc.have_ref())
    kd = tdtk.KDtree(c["model"], c["bucket"])
    with np.errstate(all="ignore"):
        idx, d2 = kd.FindClosestAlongDirBatch(c["q"], c["dirs"], c["maxdist2"])
        oi, od = _check(orc, c, idx, d2)
    hit = oi >= 0
    if name.startswith("on_the_line"):
        assert (od < 0).sum() >= 100 and (od == 0).sum() >= 100 and hit.all()
    elif name == "directions_uniform":
        assert hit[c["planted"]].any() and (~hit[c["planted"]]).any() and (od < -1.0).any()
    elif name == "directions_lattice":
        assert hit[c["axis"]].sum() >= 100 and (od == 0).any()
    elif name == "nonfinite_q":
        assert not hit[c["nan"]].any() and hit[c["ordinary"]].any()
        io, do = kd.FindClosestAlongDirBatch(c["q"][c["ordinary"]], c["dirs"][c["ordinary"]], c["maxdist2"])
        assert _same(io, idx[c["ordinary"]]) and _same(do, d2[c["ordinary"]])
    elif name in ("maxdist2_inf", "maxdist2_1e+300"):
        assert hit.all()
    elif name in ("maxdist2_-1.0", "maxdist2_nan"):
        assert not hit.any() and _same(d2, np.full(len(d2), c["maxdist2"]))
    else:
        assert hit.any() and (~hit).any()                           # 0.0 and 1e-300: a d of 0 or below still passes


# ---- 5. batch sizes around the launch geometry ---------------------------------------------------------------------------------
def test_batch_sizes_optional_d2_and_null_arguments(tdtk, orc, gpu):
    """nb is rounded up to a multiple of 8 with a minimum of 8: most workgroups are empty, one has a ragged tail"""
    lib = tdtk.lib()
    c = L.sizes()
    q, u, md2 = c["q"], c["dirs"], c["maxdist2"]
    assert len(q) == max(L.SIZES)
    kd = tdtk.KDtree(c["model"], c["bucket"])
    idx, d2 = kd.FindClosestAlongDirBatch(q, u, md2)
    oi, od = _check(orc, c, idx, d2)
    assert (oi >= 0).any() and (oi < 0).any()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for K in L.SIZES:
        qk, uk = np.ascontiguousarray(q[:K]), np.ascontiguousarray(u[:K])
        i1, d1 = kd.FindClosestAlongDirBatch(qk, uk, md2)
        assert _same(i1, idx[:K]) and _same(d1, d2[:K]), K
        assert _same(i1, oi[:K]) and _same(d1, od[:K]), K
        got = np.full(K, -7, np.int32)
        assert lib.tdtk_find_closest_along_dir(kd._h, dp(qk), dp(uk), K, md2, ip(got), None) == 0
        assert _same(got, idx[:K]), K
    assert lib.tdtk_find_closest_along_dir(kd._h, None, None, 0, md2, None, None) == 0
    K = 65
    qk, uk = np.ascontiguousarray(q[:K]), np.ascontiguousarray(u[:K])
    for h, a, b, with_idx in ((None, qk, uk, True), (kd._h, None, uk, True), (kd._h, qk, None, True), (kd._h, qk, uk, False)):
        got, gd = np.full(K, -7, np.int32), np.full(K, -7.0)
        rc = lib.tdtk_find_closest_along_dir(h, dp(a) if a is not None else None, dp(b) if b is not None else None, K, md2,
                                             ip(got) if with_idx else None, dp(gd))
        assert rc == TDTK_EINVAL and (got == -7).all() and (gd == -7.0).all()
    # (the calls above left the tree and the workspaces as they were)
    i1, d1 = kd.FindClosestAlongDirBatch(q, u, md2)
    assert _same(i1, idx) and _same(d1, d2)


# ---- 6. pairing mode 1 ---------------------------------------------------------------------------------------------------------
def _mode1_equal(got, want):
    assert got["n"] == want["n"]
    for k in ("idx", "p1", "p2", "pn"):
        assert _same(got[k], want[k]), k


@pytest.mark.parametrize("name", L.MODE1_NAMES)
def test_mode1_degenerate_normals_and_ties(tdtk, orc, gpu, name):
    """normals_mode1: the normal is normalised on the device: a zero normal gives 0 / 0, one of size 1e-200 underflows its
    length to 0 (x / 0), one of size 1e160 or 1e200 overflows it (u = 0: a closest-point search), 1e-160 squares to
    denormals.  normals_mode1_lattice: every step up to the walk is exact and whole rows of lattice points are at the same
    d, so the pair is the first point in the reference's walk order."""
    c = L.mode1_case(name)
    N = len(c["q"])
    assert not np.array_equal(c["A"], np.eye(4).reshape(16))
    if name == "normals_mode1":
        assert len(c["model"]) == 60_000 and N == 40_000
    kd = tdtk.KDtree(c["model"], c["bucket"])
    with np.errstate(all="ignore"):
        got = kd.getPtPairs(c["A"], c["q"], c["dirs"], 0, N, max_dist_match2=c["maxdist2"], pairing_mode=1)
        want = orc.Tree(c["model"], c["bucket"]).get_pt_pairs(c["A"], c["q"], c["dirs"], 0, N, 1, c["maxdist2"])
        _mode1_equal(got, want)
        if orc.have_ref():
            _mode1_equal(got, orc.RefTree(c["model"], c["bucket"]).get_pt_pairs(c["A"], c["q"], c["dirs"], 1, c["maxdist2"]))
    hit, miss = L.shares(want["idx"])
    print("%s: %d rows, %d pairs" % (name, N, want["n"]))
    if name == "normals_mode1":
        assert hit >= 0.1 and miss >= 0.1
        pl = want["idx"][c["planted"]]
        assert (pl >= 0).any() and (pl < 0).any()
    else:
        assert L.equal(np.abs(want["pn"]).sum(1), np.ones(want["n"]))
        assert L.tied_rows(c["model"], c["local"][want["idx"] >= 0], want["pn"]) >= 500


def test_mode1_more_queries_than_one_per_lane(tdtk, orc, gpu):
    cu = _cu()
    c = L.trips(cu)
    data, nr, md2, A = c["data"], c["dirs"], c["maxdist2"], c["A"]
    K = len(data)
    assert K > L.SEARCH_WG_PER_CU * cu * L.SEARCH_BLOCK
    kd = tdtk.KDtree(c["model"], c["bucket"])
    T = orc.Tree(c["model"], c["bucket"])
    with np.errstate(all="ignore"):
        got = kd.getPtPairs(A, data, nr, 0, K, max_dist_match2=md2, pairing_mode=1)
        assert got["n"] == int((got["idx"] >= 0).sum()) == len(got["p1"])
        for s in (0, (K - 30_000) // 2, K - 30_000):
            want = T.get_pt_pairs(A, data, nr, s, s + 30_000, 1, md2)
            assert _same(got["idx"][s:s + 30_000], want["idx"]), s
            first = int((got["idx"][:s] >= 0).sum())                    # the pair list is compact, in query order
            for k in ("p1", "p2", "pn"):
                assert _same(got[k][first:first + want["n"]], want[k]), (s, k)
        again = kd.getPtPairs(A, data, nr, 0, K, max_dist_match2=md2, pairing_mode=1, want_pairs=False)
        assert bytes(again["_raw"]) == bytes(got["_raw"]) and _same(again["idx"], got["idx"])
        pl = c["planted"]
        want = T.get_pt_pairs(A, data[pl], nr[pl], 0, len(pl), 1, md2)
        assert _same(got["idx"][pl], want["idx"])
        assert (want["idx"] >= 0).any() and (want["idx"] < 0).any()
        if orc.have_ref():
            rows = c["rows"]
            ref = orc.RefTree(c["model"], c["bucket"]).get_pt_pairs(A, data[rows], nr[rows], 1, md2)
            assert _same(got["idx"][rows], ref["idx"])
    hit, miss = L.shares(got["idx"])
    print("trips in mode 1: K %d, %d pairs" % (K, got["n"]))
    assert hit >= 0.1 and miss >= 0.1


# ---- 7. call order ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before_them(tdtk, orc, gpu):
    """the line search shares WS_QX .. WS_DZ, WS_KPOS, WS_ORDER, WS_HIST and the overflow buffers with the k-NN, range and
    closest-point searches (the overflow area is not asked for by a shallow tree, the others grow by free-and-reallocate):
    each call gives what it gave first, whatever ran in between"""
    d = L.deep(False, 20)
    t = L.trips(_cu())
    deep, shallow, tiny = tdtk.KDtree(d["model"], 20), tdtk.KDtree(t["model"], 20), tdtk.KDtree(t["model"][:150], 20)
    # 80 levels; a dozen (the last few pushes of a line search overflow); no overflow area asked for at all
    assert deep.info()["max_depth"] >= 4 * 16 > shallow.info()["max_depth"] > 5 >= tiny.info()["max_depth"]
    Qs, Us = t["q"][:300_000], t["dirs"][:300_000]
    calls = {
        "dir_deep": lambda: deep.FindClosestAlongDirBatch(d["q"], d["dirs"], d["maxdist2"]),
        "dir_big": lambda: shallow.FindClosestAlongDirBatch(Qs, Us, t["maxdist2"]),
        "dir_few": lambda: shallow.FindClosestAlongDirBatch(Qs[:9], Us[:9], 1.0),
        "dir_tiny": lambda: tiny.FindClosestAlongDirBatch(Qs[:9], Us[:9], 4.0),
        "mode1": lambda: (lambda g: (g["idx"], g["p1"], g["pn"]))(
            shallow.getPtPairs(t["A"], t["data"][:50_000], Us[:50_000], 0, 50_000, max_dist_match2=t["maxdist2"], pairing_mode=1)),
        "knn": lambda: shallow.kNearestNeighborsBatch(Qs, 10),
        "knn_deep": lambda: deep.kNearestNeighborsBatch(d["q"], 33),
        "range": lambda: shallow.fixedRangeSearchBatch(Qs[:50_000], 1.0),
        "closest": lambda: shallow.FindClosestBatch(Qs, 1.0),
        "closest_deep": lambda: deep.FindClosestBatch(d["q"], 25.0),
    }
    with np.errstate(all="ignore"):
        first = {name: f() for name, f in calls.items()}
        oi, od = orc.Tree(d["model"], 20).find_closest_along_dir(d["q"], d["dirs"], d["maxdist2"])
        assert _same(first["dir_deep"][0], oi) and _same(first["dir_deep"][1], od)
        order = ["dir_deep", "knn", "dir_few", "closest", "dir_big", "range", "dir_few", "knn_deep", "dir_big", "closest_deep",
                 "dir_deep", "dir_tiny", "mode1", "knn", "dir_deep", "range", "mode1", "closest", "dir_big", "dir_tiny", "knn_deep",
                 "dir_deep", "closest_deep", "dir_big"]
        assert set(order) == set(calls)
        for step, name in enumerate(order):
            got = calls[name]()
            assert len(got) == len(first[name])
            for a, b in zip(got, first[name]):
                assert _same(a, b), (step, name)
