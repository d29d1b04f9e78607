"""Generator of k15_clusters.npz: the connected components of the fixed-radius graph (tdtk_cluster_radius), every
neighbour list from the reference's own compiled KDtreeIndexed::fixedRangeSearch (oracle/_ref/libref3dtk.so) through
make_golden_collision.ColRef.range_at, turned into canonical labels by a plain union-find here.

    python tests/golden/make_golden_clusters.py     (needs oracle/_ref: a build() where the reference checkout exists)

Canonical labels: a component's key is its smallest member; components below min_size are dropped (-1); the kept ones
are numbered in ascending key order; a point outside the subset has -1.

  small cases  six k8 clouds x buckets (1, 5, 20) x three radii (well below, near and well above the radius at which the
               cloud grows together) and the 16^3 integer lattice at sqRad2 = 1.0 and nextafter(1.0, 2.0): full int32 labels
  large cases  mix (20,000 uniform points, radii 3.0, 3.5, 6.0; also with every third point masked out, against a
               reference tree over the kept points alone, and with min_size 5), chains (two interleaved helices of 2,500
               points in shuffled order, and the same with one bridge point), deep at buckets 1 and 20, table, nonfinite (the
               clouds of make_golden_knn_edges.py) and normals (two crossing planes): n_clusters and the CRC-32 of the labels
A tree cannot hold a point with a NaN or infinite coordinate (tdtk_tree_create refuses it; the reference's constructor does
not return on a NaN), so `nonfinite` is that generator's cloud, whose points are finite.
Clouds are seeded and regenerated, none is stored.  Identical points share one call of the reference (the list depends on
the coordinates alone): `table` has 40,000 copies of one point.

Also imported by the tests, so that the fixture and the live reference are checked the same way."""
import importlib.util
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k15_clusters.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgc = _load("make_golden_collision")
ColRef, k8_clouds, BUCKETS, have_ref = mgc.ColRef, mgc.k8_clouds, mgc.BUCKETS, mgc.have_ref
me = _load("make_golden_knn_edges")

SMALL = ("uniform", "duplicates", "lattice", "clusters", "seven", "one")
# sqRad2 per small cloud: well below / near / well above the radius at which the cloud becomes one piece
SMALL_R2 = {"uniform": (1.0, 4.0, 36.0), "duplicates": (0.09, 1.0, 9.0), "lattice": (1.0, float(np.nextafter(1.0, 2.0)), 9.0),
            "clusters": (2.0e-5, 4.0e-4, 1.0), "seven": (0.01, 0.5, 16.0), "one": (0.01, 1.0, 100.0)}
LATTICE_R2 = (1.0, float(np.nextafter(1.0, 2.0)))      # '<' is strict: all singletons, then one component
MIX_R2 = (9.0, 12.25, 36.0)          # radii 3.0, 3.5, 6.0
MIX_MIN_SIZE = 5
CHAIN_R = 1.0
DEEP_R2 = 2.25
NORMALS_R2 = 0.09
NORMALS_COS = float(np.cos(np.deg2rad(10.0)))
LARGE = ("mix", "chains", "deep", "table", "nonfinite", "normals")


# ---- clouds ---------------------------------------------------------------------------------------------------------
def lattice16():
    return me.lattice_cloud()[0]


def mix_cloud():
    return np.random.default_rng(1).uniform(0, 100, (20_000, 3))


def mix_subset():
    """every third point masked out"""
    return (np.arange(20_000) % 3) != 0


def chains_cloud(bridge=False):
    """two interleaved helices of 2,500 points about the z axis, half a turn apart (radius 0.75 r, rise 5 r per turn):
    consecutive points 0.9 r of arc apart, the helices 1.5 r or more from each other everywhere; with `bridge`, one more
    point on the axis, 0.75 r from point 100 of either helix.  Shuffled."""
    r = CHAIN_R
    R, pitch = 0.75 * r, 5.0 * r
    per_turn = np.hypot(2 * np.pi * R, pitch)
    n = 2_500
    t = np.arange(n) * (0.9 * r / per_turn) * 2 * np.pi
    a = np.column_stack([R * np.cos(t), R * np.sin(t), pitch * t / (2 * np.pi)])
    b = np.column_stack([R * np.cos(t + np.pi), R * np.sin(t + np.pi), pitch * t / (2 * np.pi)])
    pts = np.vstack([a, b])
    if bridge:
        pts = np.vstack([pts, [[0.0, 0.0, a[100, 2]]]])
    perm = np.random.default_rng(77).permutation(len(pts))
    return np.ascontiguousarray(pts[perm])


def normals_cloud():
    """4,000 points on the planes z = 0 and x = 0, which cross; normals (0,0,1) and (1,0,0), a tenth sign-flipped"""
    rng = np.random.default_rng(404)
    a = np.column_stack([rng.uniform(-2, 2, 2_000), rng.uniform(-2, 2, 2_000), np.zeros(2_000)])
    b = np.column_stack([np.zeros(2_000), rng.uniform(-2, 2, 2_000), rng.uniform(-2, 2, 2_000)])
    pts = np.vstack([a, b])
    nrm = np.vstack([np.tile([0.0, 0.0, 1.0], (2_000, 1)), np.tile([1.0, 0.0, 0.0], (2_000, 1))])
    nrm[rng.random(4_000) < 0.1] *= -1.0
    perm = rng.permutation(4_000)
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(nrm[perm])


def large_cloud(name):
    if name == "mix":
        return mix_cloud()
    if name == "chains":
        return chains_cloud()
    if name == "chains_bridge":
        return chains_cloud(True)
    if name == "deep":
        return me.deep_cloud()[0]
    if name == "table":
        return me.table_cloud()[0]
    if name == "nonfinite":
        return me.nonfinite_cloud()[0]
    if name == "normals":
        return normals_cloud()[0]
    raise KeyError(name)


# ---- the reference's lists, and the union-find --------------------------------------------------------------------------
def ref_edges(pts, bucket, r2, tree=None):
    """(i, j) for every j != i of fixedRangeSearch(p_i, r2).  Identical points share one call: the list depends on the
    coordinates alone, so a copy i of the point u that was asked has u's list, which holds u -- the edge (i, u) stands for it"""
    tree = tree or ColRef(pts, bucket)
    P = tree.pts
    base = P.ctypes.data
    _, rep, inv = np.unique(P, axis=0, return_index=True, return_inverse=True)
    rep_of = rep[inv.reshape(-1)]
    ei, ej = [], []
    holds_itself = np.zeros(len(P), bool)
    for u in rep:
        lst = tree.range_at(base + 24 * int(u), float(r2))
        holds_itself[u] = (lst == u).any()
        ei.append(np.full(len(lst), u, np.int64))
        ej.append(lst)
    copies = np.flatnonzero((rep_of != np.arange(len(P))) & holds_itself[rep_of])
    ei, ej = np.concatenate(ei + [copies]), np.concatenate(ej + [rep_of[copies]])
    keep = ei != ej
    return ei[keep], ej[keep]


def components(n, ei, ej):
    """union-find over the edges: root[i], the smallest member of i's component.  Every round hooks the larger of an edge's
    two roots under the smaller one and flattens the forest again"""
    parent = np.arange(n, dtype=np.int64)
    while len(ei):
        ri, rj = parent[ei], parent[ej]
        lo, hi = np.minimum(ri, rj), np.maximum(ri, rj)
        m = lo != hi
        if not m.any():
            break
        np.minimum.at(parent, hi[m], lo[m])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def canonical(root, nodes=None, min_size=1):
    """(labels int32, n_clusters, first int32, sizes uint32) of the partition root[] over the nodes (a bool mask; None: all)"""
    n = len(root)
    nodes = np.ones(n, bool) if nodes is None else np.asarray(nodes, bool)
    labels = np.full(n, -1, np.int32)
    keys, counts = np.unique(root[nodes], return_counts=True)
    kept = counts >= max(int(min_size), 1)
    keys, counts = keys[kept], counts[kept]
    number = np.full(n, -1, np.int64)
    number[keys] = np.arange(len(keys))
    labels[nodes] = number[root[nodes]]
    return labels, len(keys), keys.astype(np.int32), counts.astype(np.uint32)


def of_labels(labels):
    """(n_clusters, first, sizes) a set of canonical labels implies"""
    members = np.flatnonzero(labels >= 0)
    n = int(labels.max()) + 1 if len(members) else 0
    first = np.full(n, len(labels), np.int64)
    np.minimum.at(first, labels[members], members)
    return n, first.astype(np.int32), np.bincount(labels[members], minlength=n).astype(np.uint32)


def reference_labels(pts, bucket, r2, subset=None, normals=None, min_cos=0.0, min_size=1):
    """the canonical labels from the live reference.  subset: a reference tree over the kept points ALONE, mapped back"""
    pts = np.ascontiguousarray(pts, np.float64)
    n = len(pts)
    if subset is None:
        ei, ej = ref_edges(pts, bucket, r2)
    else:
        kept = np.flatnonzero(subset)
        si, sj = ref_edges(np.ascontiguousarray(pts[kept]), bucket, r2)
        ei, ej = kept[si], kept[sj]
    if normals is not None:
        a, b = normals[ei], normals[ej]
        with np.errstate(invalid="ignore"):
            c = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
            ok = c >= min_cos
        ei, ej = ei[ok], ej[ok]
    return canonical(components(n, ei, ej), subset, min_size)


# ---- segment_colliding.cc:55-102, restated as written ---------------------------------------------------------------------
def segment_colliding_loop(n, lists):
    """the reference's bookkeeping over the lists (lists[i]: fixedRangeSearch(p_i) in its order), line for line; returns
    (group2points, point2group)"""
    group2points = [[i] for i in range(n)]
    point2group = list(range(n))
    for i in range(n):
        current_group = point2group[i]
        neighbours = [int(v) for v in lists[i]]
        smallest_group = n
        for it in neighbours:
            if point2group[it] < smallest_group:
                smallest_group = point2group[it]
        if smallest_group >= i:
            for it in neighbours:
                group2points[current_group].append(it)            # :76
                group2points[point2group[it]].clear()             # :77
                point2group[it] = current_group                   # :78
            continue
        for it in neighbours:
            current_group = point2group[it]
            if current_group == smallest_group:
                continue
            group2points[smallest_group].extend(group2points[current_group])      # :96
            for it2 in group2points[current_group]:
                point2group[it2] = smallest_group                 # :98
            group2points[it].clear()                              # :100
    return group2points, point2group


def ref_lists(pts, bucket, r2):
    tree = ColRef(pts, bucket)
    base = tree.pts.ctypes.data
    return [tree.range_at(base + 24 * i, float(r2)) for i in range(len(pts))]


# ---- the fixture ------------------------------------------------------------------------------------------------------
def crc(labels):
    return np.array([zlib.crc32(np.ascontiguousarray(labels, "<i4").tobytes())], np.uint32)


def small_cases():
    """(key, points, bucket, r2) of every small case"""
    clouds = k8_clouds()
    for name in SMALL:
        for b in BUCKETS:
            for j, r2 in enumerate(SMALL_R2[name]):
                yield "%s_b%d_r%d" % (name, b, j), clouds[name][0], b, r2
    for b in BUCKETS:
        for j, r2 in enumerate(LATTICE_R2):
            yield "lattice16_b%d_r%d" % (b, j), lattice16(), b, r2


def large_cases():
    """(key, cloud name, bucket, r2, keyword arguments of reference_labels)"""
    for j, r2 in enumerate(MIX_R2):
        yield "mix_r%d" % j, "mix", 20, r2, {}
        yield "mix_r%d_subset" % j, "mix", 20, r2, {"subset": mix_subset()}
    yield "mix_r0_min%d" % MIX_MIN_SIZE, "mix", 20, MIX_R2[0], {"min_size": MIX_MIN_SIZE}
    yield "chains", "chains", 20, CHAIN_R * CHAIN_R, {}
    yield "chains_bridge", "chains_bridge", 20, CHAIN_R * CHAIN_R, {}
    for b in me.DEEP_BUCKETS:
        yield "deep_b%d" % b, "deep", b, DEEP_R2, {}
    yield "table", "table", 20, me.TABLE_R2[0], {}
    yield "nonfinite", "nonfinite", 20, me.NONFINITE_R2, {}
    yield "normals_plain", "normals", 20, NORMALS_R2, {}
    yield "normals_cos10", "normals", 20, NORMALS_R2, {"normals": normals_cloud()[1], "min_cos": NORMALS_COS}


def compute():
    z, stats = {}, []
    for key, pts, b, r2 in small_cases():
        labels, n, first, sizes = reference_labels(pts, b, r2)
        z[key + "_labels"] = labels
        stats.append((key, len(pts), n, int(sizes.max())))
    clouds = {}
    for key, name, b, r2, kw in large_cases():
        if name not in clouds:
            clouds[name] = large_cloud(name)
        labels, n, first, sizes = reference_labels(clouds[name], b, r2, **kw)
        z[key + "_n"] = np.array([n], np.uint64)
        z[key + "_crc"] = crc(labels)
        z[key + "_max"] = np.array([sizes.max() if n else 0], np.uint32)
        stats.append((key, len(clouds[name]), n, int(sizes.max()) if n else 0))
    return z, stats


def check_not_vacuous(stats):
    s = {k: (n, c, big) for k, n, c, big in stats}
    for name in SMALL:
        if name in ("one",):
            continue
        for b in BUCKETS:
            lo, mid, hi = (s["%s_b%d_r%d" % (name, b, j)] for j in range(3))
            # fewer and fewer components (the lattice goes from all singletons to one piece within an ulp of sqRad2)
            assert lo[1] > mid[1] >= hi[1] >= 1 and (mid[1] > hi[1] or name == "lattice"), (name, b, lo, mid, hi)
    for b in BUCKETS:
        assert s["lattice16_b%d_r0" % b][1] == 4096 and s["lattice16_b%d_r1" % b][1:] == (1, 4096)     # '<' is strict
    assert s["mix_r0"][1] > s["mix_r1"][1] > s["mix_r2"][1] == 1
    assert s["chains"][1:] == (2, 2500) and s["chains_bridge"][1:] == (1, 5001)
    assert s["normals_plain"][1] == 1 and s["normals_cos10"][1] >= 2 and s["normals_cos10"][2] >= 1900
    assert s["table"][2] >= me.TABLE_COPIES


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    if not have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    import time
    t0 = time.time()
    z, stats = compute()
    for s in stats:
        print(s)
    check_not_vacuous(stats)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes, %.1f s)" % (OUT, len(z), os.path.getsize(OUT), time.time() - t0))
