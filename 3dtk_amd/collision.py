"""collision_model (src/collision/collision_model.cc) on the device: a point model moves along a trajectory through an
environment scan; every environment point it touches is marked and gets a penetration depth.  A thin mirror of the
reference's three steps over tdtk_collision_mark / tdtk_collision_depth_closest / tdtk_collision_depth_axis; the queries
are generated on the device from (frame, model point), nothing of size frames x model points exists on the host."""
import ctypes as C

import numpy as np

from ._capi import lib, check, dptr, f64
from .slam6d import KDtree

CTYPE1, CTYPE2, CTYPE3 = 1, 2, 3     # spheres at every frame, segments between frames, everything collides


def read_trajectory(path):
    """read_trajectory (collision_model.cc:185-221): one pose per line, 16 numbers, right-handed and row-major; returns
    [F][16], the internal column-major matrices (the permutation and the signs of lines 202-217)."""
    src = (5, 9, 1, 13, 6, 10, 2, 14, 4, 8, 0, 12, 7, 11, 3, 15)
    sgn = np.array([1, -1, -1, -1, -1, 1, 1, -1, -1, 1, 1, 1, -1, 1, 1, 1], np.float64)
    rows = []
    with open(path) as f:
        for line in f:
            tmp = np.zeros(16)
            vals = line.split()[:16]
            if not vals:
                continue
            tmp[:len(vals)] = [float(v) for v in vals]
            rows.append(tmp[list(src)] * sgn)
    return np.array(rows, np.float64).reshape(-1, 16)


def _frames(trajectory):
    return np.ascontiguousarray(np.asarray(trajectory, np.float64).reshape(-1, 16))


def handle_pointcloud(pointmodel, environment, trajectory, radius, cmethod, bucketSize=20, device=0):
    """handle_pointcloud (collision_model.cc:312-430): (colliding [M] bool over the environment's points, num_colliding).
    cmethod 1: a sphere of `radius` around every model point at every frame; 2: around the segment every model point sweeps
    between consecutive frames; 3: everything collides.  `environment` is [M][3], or a KDtree already built over it."""
    cmethod = int(cmethod)
    tree = environment if isinstance(environment, KDtree) else None
    if cmethod == CTYPE3:
        n = tree.n if tree is not None else len(f64(environment).reshape(-1, 3))
        return np.ones(n, bool), n
    if tree is None:
        tree = KDtree(environment, bucketSize, device)
    model = f64(pointmodel).reshape(-1, 3)
    fr = _frames(trajectory)
    mask = np.zeros(tree.n, np.uint8)
    num = C.c_uint64(0)
    check(lib().tdtk_collision_mark(tree._h, dptr(model), len(model), dptr(fr), len(fr), float(radius), cmethod,
                                    mask.ctypes.data, C.byref(num)))
    return mask.astype(bool), int(num.value)


def segment_colliding(environment, colliding=None, sqRad2=20.0, bucketSize=20, device=0):
    """segment_colliding (src/collision/segment_colliding.cc:55-102): the colliding points in groups, every point joined
    with the points of fixedRangeSearch(p, sqRad2) around it (the default 20 is the literal of line 61).  Returns the groups
    as arrays of ascending environment indices, in ascending order of their smallest member: the connected components of
    that relation (tdtk_cluster_radius), not what the reference's bookkeeping leaves of them (include/tdtk_hip.h).
    `environment` is [M][3] or a KDtree over it; `colliding` [M] the mask of handle_pointcloud (None: every point)."""
    tree = environment if isinstance(environment, KDtree) else KDtree(environment, bucketSize, device)
    labels, n = tree.clusters(sqRad2, subset=colliding)
    members = np.flatnonzero(labels >= 0)
    order = members[np.argsort(labels[members], kind="stable")]
    counts = np.bincount(labels[members], minlength=n)
    return np.split(order, np.cumsum(counts)[:-1]) if n else []


def calculate_collidingdist(environment, colliding, bucketSize=20, device=0, want_unreached=False):
    """calculate_collidingdist (collision_model.cc:637-712): for every colliding point, in ascending index, the float
    distance to the nearest non-colliding point (1000.0 where none lies within 1000; want_unreached: how many)."""
    env = f64(environment).reshape(-1, 3)
    mask = np.ascontiguousarray(np.asarray(colliding).astype(bool).astype(np.uint8))
    if len(mask) != len(env):
        raise ValueError("colliding must have one entry per environment point")
    dist = np.full(int(mask.sum()), 1000.0, np.float32)
    unreached = C.c_uint64(0)
    check(lib().tdtk_collision_depth_closest(dptr(env), len(env), mask.ctypes.data, int(bucketSize), int(device),
                                             dist.ctypes.data, C.byref(unreached)))
    return (dist, int(unreached.value)) if want_unreached else dist


def calculate_collidingdist2(pointmodel, environment, trajectory, colliding, radius, bucketSize=20, device=0):
    """calculate_collidingdist2 (collision_model.cc:714-800): for every colliding point, by compact index, the float
    penetration depth along the model's y axis (sqrt(1000) where no query reached it)."""
    env = f64(environment).reshape(-1, 3)
    mask = np.ascontiguousarray(np.asarray(colliding).astype(bool).astype(np.uint8))
    if len(mask) != len(env):
        raise ValueError("colliding must have one entry per environment point")
    model = f64(pointmodel).reshape(-1, 3)
    fr = _frames(trajectory)
    dist = np.full(int(mask.sum()), 1000.0, np.float32)
    check(lib().tdtk_collision_depth_axis(dptr(env), len(env), mask.ctypes.data, dptr(model), len(model), dptr(fr), len(fr),
                                          float(radius), int(bucketSize), int(device), dist.ctypes.data))
    return dist
