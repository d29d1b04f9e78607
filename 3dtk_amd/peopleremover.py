"""peopleremover (src/peopleremover/peopleremover.cc) on the device: dynamic objects are removed from a set of registered
scans by free-space carving on a voxel grid.  A thin mirror over tdtk_voxel_walk / tdtk_peopleremover; the command line,
scan reading and the .3d / mask writers stay with the caller, --maxrange-method normals and --reduce are not covered."""
import ctypes as C

import numpy as np

from ._capi import lib, check, dptr, f64

# parse_cmdline's defaults, common.cc:432-435
VOXEL_SIZE, DIFF, CLUSTER_SIZE = 10.0, 0, 5


def walk_voxels(starts, ends, voxel_size, device=0):
    """walk_voxels (common.cc:112-306) for every ray starts[i] -> ends[i]: (offsets [m+1], voxels [total][3] int32), ray i
    owning voxels[offsets[i]:offsets[i+1]] -- every call the reference makes to its visitor, in order, repeats included."""
    a = f64(starts).reshape(-1, 3)
    b = f64(ends).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError("starts and ends differ in shape")
    m = len(a)
    offsets = np.zeros(m + 1, np.uint64)
    total = C.c_uint64(0)
    op = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib().tdtk_voxel_walk(device, dptr(a), dptr(b), m, float(voxel_size), op, None, 0, C.byref(total))
    if total.value == 0:
        check(rc)
        return offsets, np.zeros((0, 3), np.int32)
    vox = np.empty((total.value, 3), np.int32)      # the count pass refused with "cap < total": fill
    check(lib().tdtk_voxel_walk(device, dptr(a), dptr(b), m, float(voxel_size), op, vox.ctypes.data_as(C.POINTER(C.c_int32)),
                                total.value, C.byref(total)))
    return offsets, vox


def _origins(poses_or_origins):
    p = f64(poses_or_origins)
    if p.ndim == 2 and p.shape[1] == 3:
        return np.ascontiguousarray(p)
    p = p.reshape(-1, 16)                              # transMatOrg, column-major: the scanner position is its translation
    return np.ascontiguousarray(p[:, 12:15])


def peopleremover(scans, poses_or_origins, voxel_size=VOXEL_SIZE, diff=DIFF, cluster_size=CLUSTER_SIZE,
                  no_subvoxel_accuracy=False, ray_ends=None, want_free=False, device=0):
    """scans: one [n_i][3] array per scan, in the global frame (after transformAll(transMatOrg)); poses_or_origins: [S][3]
    scanner positions or [S][16] transMatOrg.  ray_ends: None or one [n_i][3] array per scan, where that point's ray stops
    (the caller's shortened rays).  Returns (masks, counts): masks[i] [n_i] bool, True where the reference writes the point
    to the dynamic file; counts: occupied, freed, free_after_clustering, half_free -- what the reference prints -- and
    visits; with want_free also counts["free_voxels"] [k][3] int32 in std::set order.  The reference's range filter
    setRangeFilter(-1, voxel_diagonal) is the caller's: read_uos(path, min_dist=voxel_size * sqrt(3)) applies it."""
    pts = [f64(s).reshape(-1, 3) for s in scans]
    org = _origins(poses_or_origins)
    if len(org) != len(pts):
        raise ValueError("%d scans but %d origins" % (len(pts), len(org)))
    offs = np.zeros(len(pts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pts])
    n = int(offs[-1])
    xyz = np.ascontiguousarray(np.concatenate(pts)) if pts else np.zeros((0, 3))
    ends = None
    if ray_ends is not None:
        ends = np.ascontiguousarray(np.concatenate([f64(e).reshape(-1, 3) for e in ray_ends]))
        if ends.shape != xyz.shape:
            raise ValueError("ray_ends and scans differ in shape")
    dyn = np.zeros(n, np.uint8)
    info = np.zeros(5, np.uint64)
    L = lib()

    def call(free, cap):
        return L.tdtk_peopleremover(device, dptr(xyz), offs.ctypes.data_as(C.POINTER(C.c_uint64)), dptr(org), dptr(ends),
                                    len(pts), float(voxel_size), int(diff), int(cluster_size), 0 if no_subvoxel_accuracy else 1,
                                    dyn.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    free.ctypes.data_as(C.POINTER(C.c_int32)) if free is not None else None, cap,
                                    info.ctypes.data_as(C.POINTER(C.c_uint64)))
    check(call(None, 0))
    counts = dict(zip(("occupied", "freed", "free_after_clustering", "half_free", "visits"), (int(v) for v in info)))
    if want_free:
        free = np.empty((counts["free_after_clustering"], 3), np.int32)
        if len(free):
            check(call(free, len(free)))
        counts["free_voxels"] = free
    masks = [dyn[int(offs[i]):int(offs[i + 1])].astype(bool) for i in range(len(pts))]
    return masks, counts


def last_timings():
    """HIP-event times of this thread's last peopleremover call, ms: occupancy build, walk, cluster + half-free +
    classification, first upload to last download"""
    ms = np.zeros(4)
    check(lib().tdtk_peopleremover_timings(dptr(ms)))
    return dict(zip(("build_ms", "walk_ms", "post_ms", "total_ms"), ms.tolist()))


def synthetic_room(n_scans, points_per_scan, half=300.0, box=40.0, seed=0, moving=True):
    """A box room [-half, half]^3 scanned from n_scans positions along a line, with a cube of edge `box` that stands
    somewhere else in every scan (moving) or in scan 1 only: (scans, origins).  Every point is where a random ray from the
    scanner first hits the cube or a wall, so the geometry is what a scanner would see.  The workload of
    tools/query_bench.py --only-peopleremover and of the fixture's room cases."""
    rng = np.random.default_rng(seed)
    scans, origins = [], []
    for i in range(n_scans):
        t = (i + 0.5) / n_scans
        o = np.array([(t - 0.5) * half, -0.4 * half + 0.13 * half * t, -0.5 * half + 7.0])
        d = rng.normal(size=(points_per_scan, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        with np.errstate(divide="ignore"):
            tw = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf)).min(axis=1)
        hit = tw
        if moving or i == 1:
            c = np.array([(0.8 * t - 0.4) * half if moving else 0.1 * half, 0.35 * half, -0.5 * half + 60.0])
            lo, hi = c - box / 2, c + box / 2
            with np.errstate(divide="ignore", invalid="ignore"):
                t1, t2 = (lo - o) / d, (hi - o) / d
            tn, tf = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
            on_box = (tn <= tf) & (tn > 0)
            hit = np.where(on_box, np.minimum(tn, tw), tw)
        scans.append(np.ascontiguousarray(o + d * hit[:, None]))
        origins.append(o)
    return scans, np.array(origins)
