"""A Python restatement of the voxel grid's key arithmetic (3dtk_amd/csrc/voxel_lane.h: vox_key, the brick key, vox_hash) and
of what follows from it alone: a brick's home slot, the slots an open-addressing table with linear probing ends up using, the
26-connected components of a voxel set.  tests/golden/make_golden_peopleremover_paths.py selects its directed cases with it,
tests/test_peopleremover_paths_host.py compares it with the lane code's and states with it what each case reaches."""
import numpy as np

VOX_BIAS = 1 << 20
M64 = (1 << 64) - 1


def vox_key(x, y, z):
    ux, uy, uz = int(x) + VOX_BIAS, int(y) + VOX_BIAS, int(z) + VOX_BIAS
    return ((ux >> 2) << 44) | ((uy >> 2) << 25) | ((uz >> 2) << 6) | ((ux & 3) << 4) | ((uy & 3) << 2) | (uz & 3)


def brick_key(bx, by, bz):
    """the key >> 6 of every voxel whose coordinates, floor-divided by 4, are (bx, by, bz)"""
    return vox_key(4 * bx, 4 * by, 4 * bz) >> 6


def vox_hash(k):
    k = int(k)
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def home(bk, slots):
    return (vox_hash(bk) & 0xFFFFFFFF) & (slots - 1)


def slots_for(n_bricks):
    """the table's size: a power of two, at least 64, at most half full"""
    slots = 64
    while slots < 2 * n_bricks:
        slots <<= 1
    return slots


def insert_all(bkeys, slots):
    """{slot: brick key} after inserting the keys in this order"""
    table = {}
    for bk in bkeys:
        h = home(bk, slots)
        while h in table:
            h = (h + 1) & (slots - 1)
        table[h] = bk
    return table


def probe_length(table, bk, slots):
    """slots a lookup of bk reads, its last one (the brick's, or the empty one) included; whether a read went from slot
    slots - 1 on to slot 0"""
    h, reads, wrapped = home(bk, slots), 1, False
    while h in table and table[h] != bk:
        wrapped |= h == slots - 1
        h = (h + 1) & (slots - 1)
        reads += 1
    return reads, wrapped


def voxels_of(points, vs):
    """[n][3] int64 by floor division: the cases these tests state something about hold no coordinate where the reference's
    py_div differs from it (the occupied count of the fixture is compared with the count this gives)"""
    return np.floor(np.asarray(points, np.float64) / vs).astype(np.int64)


def bricks_of(voxels):
    return {(int(v[0]) >> 2, int(v[1]) >> 2, int(v[2]) >> 2) for v in np.asarray(voxels).reshape(-1, 3)}


def components(voxels):
    """the 26-connected components of a set of voxels: a list of lists of (x, y, z)"""
    vox = [tuple(int(c) for c in v) for v in np.asarray(voxels).reshape(-1, 3)]
    index = {v: i for i, v in enumerate(vox)}
    parent = list(range(len(vox)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    nb = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) > (0, 0, 0)]
    for v, i in index.items():
        for d in nb:
            j = index.get((v[0] + d[0], v[1] + d[1], v[2] + d[2]))
            if j is not None:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = {}
    for v, i in index.items():
        out.setdefault(find(i), []).append(v)
    return list(out.values())
