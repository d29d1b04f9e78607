"""k nearest within a radius on the paths the k12 cases never reach: the CPU tier.  The fixture k13_knn_range_edges.npz
(tests/golden/make_golden_knn_range_edges.py) against the reference's compiled kd.cc, the device walk compiled for the host
against every stored row, count, CRC and walk record, the preconditions that make the GPU tier's cases reach their branches
(asserted from those records), brute force on the clouds where it can stand in, and a mutation check: five wrong versions of
knn_range_walk / leaf_span, each of which at least one k13 case must catch."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import host_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def ge():
    return _load("make_golden_knn_range_edges")


@pytest.fixture(scope="module")
def fx(ge):
    return ge.load()


@pytest.fixture(scope="module")
def all_cases(ge):
    return ge.cases()


@pytest.fixture(scope="module")
def base_lib(ge, tmp_path_factory):
    return ge.host_lib(tmp_path_factory.mktemp("hwe"))


@pytest.fixture(scope="module")
def trees(ge, base_lib, all_cases):
    """kd_build.cpp's tree of every case (a HostTree is plain data: the mutated libraries below walk the same trees)"""
    return {c.name: ge.HostWalk(base_lib, c.pts, c.bucket) for c in all_cases}


@pytest.fixture(scope="module")
def walks(trees, all_cases):
    """the device walk compiled for the host on every stored (case, radius, k), computed once"""
    out = {}
    for c in all_cases:
        for ri, r2 in enumerate(c.r2s):
            for k in c.ks:
                out[(c.name, ri, k)] = trees[c.name].search(c.Q, k, r2)
    return out


def _case_mismatch(ge, fx, c, ri, k, got, records=True):
    """what of one stored (case, radius, k) the walk's result `got` does not reproduce (None: everything)"""
    idx, d2, cnt, sp, fl, big = got
    if not np.array_equal(cnt, fx.counts(c, ri, k)):
        return "counts"
    if c.store_rows:
        rep = fx.rows(c, ri, k)
        have = idx >= 0
        if not (np.array_equal(have, rep >= 0) and np.array_equal(c.pts[idx[have]], c.pts[rep[have]])):
            return "rows"
    elif ge.crc_rows(ge.coords_of(c.pts, idx), cnt) != fx.crc(c, ri, k):
        return "crc"
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(idx >= 0, ge.MR.G8.dist2(c.pts, c.Q[:, None, :], idx), -1.0)
    if not np.array_equal(d2, want):
        return "d2"
    if records:
        if not np.array_equal(np.minimum(sp, 255), fx.maxsp(c, ri, k)):
            return "max_sp"
        if not (np.array_equal(fl, fx.filled(c, ri, k)) and np.array_equal(big, fx.big(c, ri, k))):
            return "flags"
    return None


# ---- the fixture and the reference, the fixture and the device walk -----------------------------------------------------
def test_fixture_equals_the_live_reference(ge, base_lib):
    if not (ge.MR.have_lib() or ge.MR.have_ref()):
        pytest.skip("neither oracle/_ref/libref_kd.so nor the reference checkout (src/slam6d/kd.cc)")
    z = np.load(ge.OUT)
    got = ge.compute(base_lib)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key]), key
    assert os.path.getsize(ge.OUT) <= os.path.getsize(ge.K9)


def test_device_walk_compiled_for_the_host_reproduces_k13(ge, fx, all_cases, walks):
    n = 0
    for c in all_cases:
        for ri in range(len(c.r2s)):
            for k in c.ks:
                assert _case_mismatch(ge, fx, c, ri, k, walks[(c.name, ri, k)]) is None, (c.name, ri, k)
                n += 1
    assert n == sum(len(c.r2s) * len(c.ks) for c in all_cases) and n > 1000


# ---- non-vacuity: the recorded walks reach the branches the GPU tier is about -----------------------------------------
def test_deep_cases_live_on_the_overflow_stack(ge, fx, all_cases, trees):
    """The stack's HBM overflow starts above Q_SD entries.  knn_range_walk pushes a far child only when its plane lies within
    the radius, and a level's split value on this cloud is the centroid of what is left, about 1e-5 of the radius peeled at
    that level: DEEP_R2's 9 and 400 never reach Q_SD entries at bucket 20 (61 of 300 queries at bucket 1, measured), and 1e30
    -- a radius of 1e15 -- pushes only at the levels whose shell lies inside it.  Recorded, bucket 1 / 20, k = 3 .. 64: at
    1e30, 212-223 / 204-219 of the 300 queries pass Q_SD, of the 100 queries of the geometric part 12-23 / 9-19 (the others
    lie further out than 1e15 and meet no plane within it); at DEEP_FINITE_R2 = 1e200, which is above every squared distance
    of the cloud so that every far child is pushed, 293-299 / 285-296 of all and 93-99 / 85-96 of the geometric part, with
    up to 82 / 77 entries.  So "at least 100 queries" is asserted at both radii, "at least half of the geometric part" where
    every far child is pushed."""
    deep = [c for c in all_cases if c.kind == "deep"]
    assert [c.bucket for c in deep] == list(ge.ME.DEEP_BUCKETS)
    for c in deep:
        assert trees[c.name].max_depth >= 4 * ge.Q_SD and not trees[c.name].table_mode
        assert c.r2s == (ge.DEEP_FINITE_R2, ge.HUGE) and np.isfinite(c.r2s[0])
        with np.errstate(over="ignore"):
            assert c.r2s[0] > ge.all_d2(c.pts, c.Q[:1]).max() * 4      # every plane test passes
        for ri in range(2):
            for k in c.ks:
                sp = fx.maxsp(c, ri, k)
                over, geo = int((sp > ge.Q_SD).sum()), int((sp[:c.ngeo] > ge.Q_SD).sum())
                print("%s r2 %g k %d: max_sp > Q_SD for %d of %d queries, %d of the %d geometric ones; largest %d"
                      % (c.name, c.r2s[ri], k, over, len(sp), geo, c.ngeo, sp.max()))
                assert over >= 100, (c.name, ri, k)
                if ri == 0:
                    assert 2 * geo >= c.ngeo, (c.name, k)
                assert sp.max() >= 24                                      # well into the overflow area, not one entry


def test_table_case_runs_through_the_leaf_of_copies(ge, fx, all_cases, trees):
    """Table mode, the leaf of 40,000 equal distances.  A list that is offered one copy is offered 40,000 >= k of them and
    fills: count < k together with copies in the list cannot happen on this cloud (asserted as big => filled); the short
    lists of a table-mode tree are those of queries far from the copies."""
    (c,) = [c for c in all_cases if c.kind == "table"]
    t = trees[c.name]
    assert t.table_mode and t.max_leaf >= ge.ME.TABLE_COPIES and t.big_count == t.max_leaf
    assert int(len(c.pts)).bit_length() + int(t.max_leaf).bit_length() > 30       # kd_build.cpp's packing rule
    rep_copy = int(c.copies.min())
    best_only = best_mixed = short_bands = 0
    for ri in range(len(c.r2s)):
        for k in c.ks:
            rows, cnt, big, fl = fx.rows(c, ri, k), fx.counts(c, ri, k), fx.big(c, ri, k), fx.filled(c, ri, k)
            is_copy = rows == rep_copy
            # (a full list of nearer blob points may be offered a copy and drop it: the rows with copies are among `big`)
            assert big[is_copy.any(1)].all() and fl[big].all(), (ri, k)
            only = is_copy.all(1)
            mixed = is_copy.any(1) & ~only
            # blob points in front of the copies, or behind them
            front = mixed & ~is_copy[:, 0]
            print("table r2 %g k %d: %d lists of copies only, %d mixed (%d with blob points in front), %d short and not empty"
                  % (c.r2s[ri], k, only.sum(), mixed.sum(), front.sum(), ((cnt > 0) & (cnt < k)).sum()))
            best_only, best_mixed = max(best_only, int(only.sum())), max(best_mixed, int(mixed.sum()))
            short_bands += int(((cnt > 0) & (cnt < k)).any())
    assert best_only >= 16 and best_mixed >= 8 and short_bands >= 1


def test_lattice_case_has_ties_and_queries_on_split_planes(ge, fx, all_cases, trees):
    lat = [c for c in all_cases if c.kind == "lattice"]
    assert [c.bucket for c in lat] == list(ge.ME.LATTICE_BUCKETS) and lat[0].r2s == ge.ME.LATTICE_R2
    c = lat[0]
    D = ge.all_d2(c.pts, c.Q)
    fills = 0
    for ri, r2 in enumerate(c.r2s):
        at, below = (D == r2).any(1), (D < r2).any(1)
        assert (at & below).any(), r2
        # ... together with a list that fills mid-walk: full lists whose ball holds more than k points (none at r2 = 1: a
        # query with a point at distance 1 is a lattice point and has itself alone inside)
        for k in c.ks:
            fills += int((fx.filled(c, ri, k) & ((D < r2).sum(1) > k) & at).sum())
    print("lattice: %d (radius, k, query) with a point at d2 == r2 and a list that filled before the ball was through" % fills)
    assert fills >= 100
    val, axis = trees[c.name].splits()                    # bucket 1
    on = np.zeros(len(c.Q), bool)
    for a in range(3):
        on |= np.isin(c.Q[:, a], val[axis == a])
    print("lattice: %d of %d stored queries lie on a split value of the bucket-1 tree" % (on.sum(), len(on)))
    assert on.sum() >= 200


def test_short_cases_cover_every_band(ge, fx, all_cases):
    short = [c for c in all_cases if c.kind == "short"]
    bands = ((1, 4), (5, 10), (11, 20), (21, 32), (33, 64))
    seen = {b: set() for b in bands}
    for c in short:
        for k in c.ks:
            b = [b for b in bands if b[0] <= k <= b[1]][0]
            seen[b].add("<" if c.M < k else ("=" if c.M == k else ">"))
            assert (fx.counts(c, 0, k) == min(c.M, k)).all(), (c.name, k)          # the radius that holds everything
            half = fx.counts(c, 1, k)
            assert (half <= min(c.M, k)).all()
        if c.M >= 9:
            inball = (ge.all_d2(c.pts, c.Q) < c.r2s[1]).mean()
            assert 0.3 < inball < 0.7, (c.name, inball)                               # "about half the cloud"
    assert all(s == {"<", "=", ">"} for s in seen.values()), seen


# ---- brute force where it can stand in ------------------------------------------------------------------------------------
def test_brute_force_agrees_with_the_rows(ge, fx, all_cases, walks):
    """the d2 row is the min(k, count) smallest Dist2 < r2, ascending, and count = min(k, |ball|): trips (the host walk's rows,
    which reproduce the stored CRCs), table, lattice and short.  Not the deep cloud: far out the reference's box test
    rounds away the query's own leaf, there only the reference is the authority."""
    n = 0
    for c in all_cases:
        if c.kind in ("deep", "nonfinite"):
            continue
        sel = np.arange(0, len(c.Q), 4) if c.kind == "trips" else np.arange(len(c.Q))
        D = np.vstack([np.sort(ge.all_d2(c.pts, c.Q[sel[s:s + 50]]), axis=1)[:, :65] for s in range(0, len(sel), 50)])
        D = np.pad(D, ((0, 0), (0, 65 - D.shape[1])), constant_values=np.inf)      # (65 > every k)
        for ri, r2 in enumerate(c.r2s):
            inball = (D < r2).sum(1)
            for k in c.ks:
                idx, d2, cnt = walks[(c.name, ri, k)][:3]
                assert np.array_equal(cnt[sel], np.minimum(inball, k)), (c.name, ri, k)
                m = np.arange(k)[None, :] < cnt[sel][:, None]
                assert np.array_equal(np.where(m, d2[sel], -1.0), np.where(m, D[:, :k], -1.0)), (c.name, ri, k)
                n += 1
    assert n == sum(len(c.r2s) * len(c.ks) for c in all_cases if c.kind not in ("deep", "nonfinite")) and n > 900


# ---- mutation check: the new cases can fail --------------------------------------------------------------------------------
# (name, the text of query_lane.h to replace, its replacement, inside knn_range_walk only?)  Never run on a GPU.
MUTATIONS = (
    ("near child on myd > 0", "const bool first = myd >= 0.0;", "const bool first = myd > 0.0;", True),
    ("skip on md > r2", "if (md >= r2) continue;", "if (md > r2) continue;", True),
    ("bound always r2", "const double bound = L.full() ? L.kth : r2;", "const double bound = r2;", True),
    ("far child pushed on myd*myd < bound", "if (myd * myd < r2) st.push", "if (myd * myd < bound) st.push", True),
    ("leaf_span ignores leaf_tab", "if (a.leaf_tab) {", "if (false) {", False),
)
# What each mutation is caught by.  "far child pushed on myd*myd < bound" cannot change a row: bound is r2 until the list is
# full, and then a far child beyond the k-th distance holds no point nearer than its plane -- the original walk pops it and
# its box test or its leaf's "kth <= md" drops everything.  It is a different walk with the same answer, and is caught by the
# recorded stack heights alone (k12 records none).


def _mutated_lib(ge, tmp, i, old, new, walk_only):
    csrc = os.path.join(ROOT, "3dtk_amd", "csrc")
    d = tmp / ("m%d" % i)
    d.mkdir()
    text = open(os.path.join(csrc, "query_lane.h")).read()
    a = text.index("__device__ void knn_range_walk") if walk_only else 0
    b = text.index("// calculateNormal (normals.cc") if walk_only else len(text)
    assert text[a:b].count(old) == 1, old
    (d / "query_lane.h").write_text(text[:a] + text[a:b].replace(old, new) + text[b:])
    shutil.copy(os.path.join(ROOT, "tests", "host_lane_shim.h"), d / "host_lane_shim.h")     # includes the copy beside it
    return ge.host_lib(d, "mut%d" % i)


def _k12_mismatch(mr, f12, L):
    """the first k12 case the library's walk does not reproduce (rows, counts), or None"""
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        pts, Q = np.ascontiguousarray(pts), np.ascontiguousarray(Q)
        for b in mr.BUCKETS:
            h = L.host_tree_create(pts.ctypes.data, len(pts), b)
            try:
                for ri, r2 in enumerate(f12.radii(name)):
                    for k in mr.KS:
                        idx = np.empty((len(Q), k), np.int32); d2 = np.empty((len(Q), k)); cnt = np.empty(len(Q), np.int32)
                        sp = np.empty(len(Q), np.int32); fl = np.empty(len(Q), np.uint8); bg = np.empty(len(Q), np.uint8)
                        L.hw_search(h, Q.ctypes.data, len(Q), k, r2, idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data,
                                    sp.ctypes.data, fl.ctypes.data, bg.ctypes.data)
                        rep, have = f12.rows(name, ri, b, k), idx >= 0
                        if not (np.array_equal(cnt, f12.counts(name, ri, b, k)) and np.array_equal(have, rep >= 0)
                                and np.array_equal(pts[idx[have]], pts[rep[have]])):
                            return (name, b, ri, k)
            finally:
                L.host_tree_destroy(h)
    return None


def test_every_mutation_of_the_walk_fails_a_k13_case(ge, fx, all_cases, trees, base_lib, tmp_path):
    mr = ge.MR
    f12 = mr.load()
    assert _k12_mismatch(mr, f12, base_lib) is None
    table = []
    for i, (name, old, new, walk_only) in enumerate(MUTATIONS):
        L = _mutated_lib(ge, tmp_path, i, old, new, walk_only)
        rows_fail, record_fail = [], []
        for c in all_cases:
            if c.kind == "trips":
                continue                      # (second trips are the device's lanes: on the host the cloud adds nothing)
            why = set()
            for ri, r2 in enumerate(c.r2s):
                for k in c.ks:
                    got = trees[c.name].search(c.Q, k, r2, L)
                    w = _case_mismatch(ge, fx, c, ri, k, got)
                    if w:
                        why.add(w)
            if why - {"max_sp", "flags"}:
                rows_fail.append(c.name)
            elif why:
                record_fail.append(c.name)
        k12 = _k12_mismatch(mr, f12, L)
        table.append((name, rows_fail, record_fail, k12))
        print("mutation %-38s rows/counts fail: %s; records only: %s; k12: %s"
              % (name, _brief(rows_fail), _brief(record_fail), "caught at %s" % (k12,) if k12 else "MISSED"))
    for name, rows_fail, record_fail, k12 in table:
        assert rows_fail or record_fail, name
    by = {name: (rows_fail, record_fail, k12) for name, rows_fail, record_fail, k12 in table}
    assert any(k12 is None for _, _, _, k12 in table)                     # k12 alone misses at least one of them
    assert by["leaf_span ignores leaf_tab"][2] is None and "table_b20" in by["leaf_span ignores leaf_tab"][0]
    assert by["far child pushed on myd*myd < bound"][0] == [] and by["far child pushed on myd*myd < bound"][1]
    for name in ("near child on myd > 0", "skip on md > r2"):
        assert by[name][0], name                                           # these change rows, and k13 sees it


def _brief(names):
    kinds = sorted({n.split("_")[0] for n in names})
    return "%d cases (%s)" % (len(names), ", ".join(kinds)) if names else "none"
