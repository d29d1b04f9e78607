"""Generator of k18_peopleremover_paths.npz: the reference's free-space carving (compiled exactly as
make_golden_peopleremover.py compiles it, whose Ref, stand-in build, digest, packing and writer are imported) on the cases
that reach what exists on the device only -- the kernels around the lane code, the device's fmod and fp64 division:

  a  chain*      bricks chosen by their home slot, so that the table's probe chain runs over the last slot back to slot 0,
                 and rays through missing bricks whose lookup has to walk that chain to its end
  b  bricks32/33 the table exactly half full (64 slots) and one brick past it (128 slots)
  c  plane, line, stairs, comps600   free components of thousands of voxels over many blocks, at cluster_size == size and
                 size + 1; 600 components of 3, 4 and 5 voxels at cluster_size 4, each across a brick boundary
  d  n255 .. n513, voxels256, bricks256, one_voxel, one_point, scans9, stack300_*, room3_cbig
                 item counts on the kernels' block boundaries, degenerate occupancies, the clamps of diff and cluster_size
  e  rand000 .. rand255, halffree_x_sub*, corner_x   small clouds around the origin: 26- and 124-neighbourhoods across
                 brick boundaries and across zero
  f  walk lists  voxel sizes 7.3, 0.07, 1e-3, 2^-3, 1e3; uniform, eighth-voxel lattice, k * vs boundaries, coordinates
                 near the packable limit
  g  one ray of about 60 000 visits: its count (the 2^32 guard of the walk query is tested with copies of it)
  h  room8x8193  65 544 points: sort, scans and compaction over many blocks

    python tests/golden/make_golden_peopleremover_paths.py          (needs the reference checkout, as the other generator)

The inputs are not stored: the case functions rebuild them from fixed seeds, the fixture holds a digest of every case's input
arrays.  All cases of a kind share a few concatenated arrays (an archive member per case and array would cost more than the
results).  Also imported by the tests."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(_HERE))
import make_golden_peopleremover as gold            # noqa: E402
import voxel_keys as vk                             # noqa: E402

OUT = os.path.join(_HERE, "k18_peopleremover_paths.npz")
MAX_BYTES = gold.MAX_BYTES
_case, _through = gold._case, gold._through
BIG = 1 << 40                                        # a diff and a cluster_size beyond 32 bits
VS5 = (0.1, 1.0 / 3.0, 1.0, 7.3, 10.0)
N_RANDOM = 256
E_FREED, E_CLUSTERED, E_HALF = 1000, 300, 500       # what tier e has to reach, summed over its scenes


def _centres(vox, vs):
    return (np.asarray(vox, np.float64).reshape(-1, 3) + 0.5) * vs


def _floor_at(o0, cen, z):
    """where the ray from o0 through each of cen reaches height z"""
    k = (z - o0[2]) / (cen[:, 2] - o0[2])
    return o0 + (cen - o0) * k[:, None]


# ---- a, b: scenes made for the brick table --------------------------------------------------------------------------------
CUBE = [(x, y, z) for x in range(-4, 4) for y in range(-4, 4) for z in range(-4, 4)]
OUTER = [(x, y, z) for x in range(-8, 8) for y in range(-8, 8) for z in range(-8, 8) if max(abs(x + .5), abs(y + .5), abs(z + .5)) > 4]
TABLE_O0 = np.array([3.0, -7.0, 50000.0])
TABLE_FLOOR_Z = -345.0                               # voxel -35: below every brick of CUBE and OUTER


def table_scene(name, targets, empties, fillers, n_bricks, exact):
    """voxel size 10.  Scan 1 holds the voxels `targets` (and one voxel in as many of the bricks `fillers` as it takes to
    bring the scene to n_bricks bricks); scan 0, high above, looks through every target and through voxel (1, 1, 1) of every
    brick of `empties` at a floor below them all."""
    vs = 10.0
    cen = _centres(targets, vs)
    through = np.concatenate([cen, _centres([(4 * b[0] + 1, 4 * b[1] + 1, 4 * b[2] + 1) for b in empties], vs).reshape(-1, 3)])
    floor = _floor_at(TABLE_O0, through, TABLE_FLOOR_Z)
    held = [cen]
    count = lambda: len(vk.bricks_of(vk.voxels_of(np.concatenate([floor] + held), vs)))      # noqa: E731
    for b in fillers:
        if count() >= n_bricks:
            break
        held.append(_centres([(4 * b[0] + 1, 4 * b[1] + 2, 4 * b[2] + 1)], vs))
    assert count() == n_bricks if exact else count() <= n_bricks, (name, count())
    return _case(name, [floor, np.concatenate(held)], [TABLE_O0, [-4000.0, -3000.0, 55.0]], vs=vs, cluster=1, subvoxel=False)


def chain_selection(slots):
    """(bricks of CUBE whose home slot is slots - 1, 0 or 1; bricks of OUTER whose home slot is slots - 1)"""
    want = (slots - 1, 0, 1)
    chain = [b for b in CUBE if vk.home(vk.brick_key(*b), slots) in want]
    empties = [b for b in OUTER if vk.home(vk.brick_key(*b), slots) == slots - 1]
    return chain, empties


def chain_case(slots):
    rng = np.random.default_rng(1800 + slots)
    chain, empties = chain_selection(slots)
    targets = []
    for b in chain:                                  # one to three voxels of each
        inside = {tuple(int(c) for c in rng.integers(0, 4, 3)) for _ in range(int(rng.integers(1, 4)))}
        targets += [(4 * b[0] + i, 4 * b[1] + j, 4 * b[2] + k) for i, j, k in sorted(inside)]
    if slots == 64:
        return table_scene("chain64", targets, empties[:3], [], 32, exact=False)
    used = set(chain)
    return table_scene("chain128", targets, empties[:3], [b for b in CUBE if b not in used], 33, exact=True)


def bricks_case(n_bricks):
    targets = [(4 * bx + 1, 1, 1) for bx in (-2, -1, 0, 1)]
    fillers = [(bx, 1, 0) for bx in range(-16, 17)]
    return table_scene("bricks%d" % n_bricks, targets, [], fillers, n_bricks, exact=True)


# ---- c: large free components ---------------------------------------------------------------------------------------------
def shape_voxels(shape):
    if shape == "plane":
        return [(x, y, 5) for x in range(-20, 28) for y in range(-20, 28)]
    if shape == "line":
        return [(x, 0, 5) for x in range(-1500, 1500)]
    if shape == "stairs":
        return [(i, i, i) for i in range(-700, 700)]
    out = []                                         # comps600: rows along x of 3, 4 and 5 voxels, each from x = 2 (mod 4) on
    for k in range(600):
        x0, y0 = 8 * (k % 30) - 78, 3 * (k // 30) - 20
        out += [(x0 + j, y0, 5) for j in range(3 + k % 3)]
    return out


SHAPES = (("plane", 2304), ("line", 3000), ("stairs", 1400))


def held_and_looked_through(name, vox, cluster, o0):
    """scan 1, far away in -x / -y, holds the voxels; scan 0 looks through each of them at a floor beyond (clusters_c*)"""
    cen = _centres(vox, 10.0)
    o0 = np.array(o0, np.float64)
    floor = np.array([_through(o0, c, 1.03) for c in cen])
    return _case(name, [floor, cen], [o0, [-40000.0, -30000.0, 55.0]], cluster=cluster, subvoxel=False)


def component_cases():
    out = []
    for shape, size in SHAPES:
        vox = shape_voxels(shape)
        assert len(vox) == size
        for cl in (size, size + 1):
            out.append(held_and_looked_through("%s_c%d" % (shape, cl), vox, cl, [55.0, 35.0, 50000.0]))
    out.append(held_and_looked_through("comps600_c4", shape_voxels("comps600"), 4, [55.0, 35.0, 5000.0]))
    return out


# ---- d, e: small clouds ---------------------------------------------------------------------------------------------------
def random_scene(rng, name, sizes=None):
    """a cloud 3-13 voxels wide, centred within 6 voxels of the origin, uniform or on the quarter-voxel lattice"""
    vs = float(VS5[int(rng.integers(len(VS5)))])
    if sizes is None:
        S = int(rng.integers(2, 7))
        sizes = rng.integers(0, 60, S)
        sizes[rng.random(S) < 0.15] = 0
        if sizes.sum() == 0:
            sizes[int(rng.integers(S))] = int(rng.integers(1, 60))
    S = len(sizes)
    width, centre = rng.uniform(3.0, 13.0), rng.uniform(-6.0, 6.0, 3)
    lattice = rng.random() < 0.5

    def snap(u):
        return np.round(u * 4.0) / 4.0 if lattice else u
    scans = [snap(centre + rng.uniform(-width / 2, width / 2, (int(n), 3))) * vs for n in sizes]
    origins = snap(centre + rng.uniform(-15.0, 15.0, (S, 3))) * vs
    diff = int((0, 1, 2, 10)[int(rng.integers(4))])
    cluster = int(rng.integers(1, 7))
    subvoxel = bool(rng.random() < 0.5)
    ends = None
    if rng.random() < 0.3:
        ends = [o + (s - o) * rng.uniform(0.6, 1.3, (len(s), 1)) for s, o in zip(scans, origins)]
    return _case(name, scans, origins, vs=vs, diff=diff, cluster=cluster, subvoxel=subvoxel, ends=ends)


def random_cases():
    rng = np.random.default_rng(1818)
    return [random_scene(rng, "rand%03d" % i) for i in range(N_RANDOM)]


def neighbourhood_cases():
    out = []
    # halffree_sub* of the first fixture moved by (-1, -1, -2) voxels: v = (-1, -1, 3) is freed, w = (1, -1, 3), at distance
    # 2 in another brick across zero, holds scans 1 and 2
    d = np.array([-10.0, -10.0, -20.0])
    v, w = np.array([5.0, 5.0, 55.0]) + d, np.array([25.0, 5.0, 55.0]) + d
    o0 = np.array([5.0, 5.0, 5000.0]) + d
    sc0 = np.array([_through(o0, v, 1.03)])
    sc1 = np.array([v, w + (1.0, 1.0, 1.0)])
    sc2 = np.array([w, w + (-2.0, 2.0, 0.5)])
    for sub in (True, False):
        out.append(_case("halffree_x_sub%d" % sub, [sc0, sc1, sc2], [o0, np.array([-2000.0, 5.0, 55.0]) + d,
                                                                     np.array([25.0, 3000.0, 55.0]) + d], cluster=1, subvoxel=sub))
    # two voxels that touch by the corner at the origin only
    cen = _centres([(-1, -1, -1), (0, 0, 0)], 10.0)
    o0 = np.array([55.0, 35.0, 5000.0])
    out.append(_case("corner_x", [np.array([_through(o0, c, 1.03) for c in cen]), cen], [o0, [-400.0, -300.0, 55.0]], cluster=2,
                     subvoxel=False))
    return out


def boundary_cases():
    out = []
    for n in (255, 256, 257, 512, 513):
        case = random_scene(np.random.default_rng(18000 + n), "n%d" % n, sizes=np.array([n // 3, n // 3, n - 2 * (n // 3)]))
        out.append(dict(case, diff=0, cluster=2, subvoxel=True))       # so that every stage has something to do
    # exactly 256 voxels; exactly 256 bricks: an 8 x 8 x 4 block of them across zero, 300 points of 3 scans
    org = np.array([[-20.0, 0.5, 0.25], [0.5, 25.0, 3.0], [10.0, 10.5, 30.0]])
    for name, vs, cell in (("voxels256", 1.0, 1), ("bricks256", 0.1, 4)):
        rng = np.random.default_rng(18256 + cell)
        cells = np.array([(x, y, z) for x in range(-3, 5) for y in range(-5, 3) for z in range(-2, 2)])
        pick = np.concatenate([np.arange(256), rng.integers(0, 256, 44)])
        vox = cells[pick] * cell + rng.integers(0, cell, (300, 3))
        pts = (vox + rng.uniform(0.2, 0.8, (300, 3))) * vs
        scan = rng.integers(0, 3, 300)
        out.append(_case(name, [pts[scan == s] for s in range(3)], org * vs * cell, vs=vs, cluster=2))
    rng = np.random.default_rng(18001)
    one = (np.array([3.0, -2.0, 1.0]) + rng.uniform(0.05, 0.95, (20, 3))) * 10.0
    out.append(_case("one_voxel", [one[5 * s:5 * s + 5] for s in range(4)],
                     [[-95.0, 3.0, 7.0], [200.0, -20.0, 15.0], [35.0, -15.0, 400.0], [36.0, 300.0, 12.0]]))
    out.append(_case("one_point", [[[12.0, -7.0, 3.0]]], [[-50.0, 20.0, 5.0]]))
    # more scans than points; scans 0, 3, 4, 8 (and 6) are empty.  Scan 5 looks along x through the voxels of scans 1 and 2.
    e = np.zeros((0, 3))
    scans = [e, _centres([(2, 0, 0)], 10.0), _centres([(4, 0, 0)], 10.0), e, e, _centres([(8, 0, 0)], 10.0), e,
             _centres([(-3, 2, 0)], 10.0), e]
    org = rng.uniform(-300.0, 300.0, (9, 3))
    org[5] = [-45.0, 5.0, 5.0]
    out.append(_case("scans9", scans, org, cluster=1))
    # 300 scans hold one voxel, one more looks through it: free with diff 0, within every larger window.  The looking scan is
    # the last one, so that the window's lower end is what decides (a lower end of current - 2^40 cut to 32 bits would be
    # the scan itself); in stack300_first_dbig it is the first one, and the upper end decides
    cen = _centres([(2, 3, 4)], 10.0)[0]
    o0 = np.array([25.0, 35.0, 5000.0])
    phi = rng.uniform(0.0, 2.0 * np.pi, 300)
    look = [np.array([_through(o0, cen, 1.03)])]
    hold = [(cen + rng.uniform(-4.5, 4.5, 3)).reshape(1, 3) for _ in range(300)]
    org = np.stack([cen[0] + 500.0 * np.cos(phi), cen[1] + 500.0 * np.sin(phi), np.full(300, cen[2])], axis=1)
    for diff in (0, 1, 150, BIG):
        out.append(_case("stack300_d%s" % ("big" if diff == BIG else diff), hold + look, np.concatenate([org, [o0]]), diff=diff,
                         cluster=1))
    out.append(_case("stack300_first_dbig", look + hold, np.concatenate([[o0], org]), diff=BIG, cluster=1))
    scans, org = gold._pr().synthetic_room(3, 2500, moving=False, seed=3)
    out.append(_case("room3_cbig", scans, org, cluster=BIG))
    return out


def pipeline_cases():
    out = [chain_case(64), chain_case(128), bricks_case(32), bricks_case(33)]
    out += component_cases() + boundary_cases() + random_cases() + neighbourhood_cases()
    scans, org = gold._pr().synthetic_room(8, 8193, seed=18)
    out.append(_case("room8x8193", scans, org))
    return out


# ---- f, g: walks -------------------------------------------------------------------------------------------------------------
WALK_VS = (7.3, 0.07, 1e-3, 2.0 ** -3, 1e3)
WALK_KINDS = ("uniform", "lattice8", "boundary", "far")


def walk_cases():
    """[(name, voxel_size, starts [64][3], ends [64][3])]"""
    rng = np.random.default_rng(1819)
    out = []
    for vs in WALK_VS:
        for kind in WALK_KINDS:
            if kind == "uniform":
                s, e = rng.uniform(-30.0, 30.0, (64, 3)), rng.uniform(-30.0, 30.0, (64, 3))
            elif kind == "lattice8":
                s = rng.integers(-240, 241, (64, 3)) / 8.0
                d = rng.integers(-240, 241, (64, 3)) / 8.0
                d[rng.random((64, 3)) < 0.2] = 0.0
                e = s + d
            elif kind == "boundary":
                k = rng.integers(-300, 301, (64, 3))
                s, e = k.astype(np.float64), (k + rng.integers(-9, 10, (64, 3))).astype(np.float64)
            else:
                s = rng.choice((-1.0, 1.0), (64, 3)) * rng.uniform(0.5e6, 1.04e6, (64, 3))
                d = rng.normal(size=(64, 3))
                e = s + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.0, 12.0, (64, 1))
            out.append(("%s_v%g" % (kind, vs), vs, s * vs, e * vs))
    return out


LONG_RAY = np.array([[-11000.7, -9000.3, -10000.9], [11000.2, 10000.4, 9000.6]])       # voxel size 1


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def case_sha(case):
    return gold.digest(case["scans"] + [case["origins"]] + (case["ends"] or []))


def compute():
    z = {}
    walks = walk_cases()
    counts, vox = zip(*(gold.Ref.walk(s, e, vs) for _, vs, s, e in walks))
    first, codes = gold.pack_lists(np.concatenate(counts), np.concatenate(vox))
    z["walk_names"] = np.array([w[0] for w in walks])
    z["walk_m"] = np.array([len(c) for c in counts], np.int32)
    z["walk_counts"] = np.concatenate(counts).astype(np.int32)
    z["walk_first"], z["walk_codes"] = first, codes
    z["walk_sha"] = np.array([gold.digest([s, e]) for _, _, s, e in walks], np.uint64)
    z["long_ray"] = LONG_RAY
    z["long_count"] = np.uint64(gold.ref_lib().pr_walk(LONG_RAY[0].ctypes.data, LONG_RAY[1].ctypes.data, 1.0, 0, None))
    cases = pipeline_cases()
    res = {c["name"]: gold.Ref.run(c) for c in cases}
    z["run_names"] = np.array([c["name"] for c in cases])
    z["run_npts"] = np.array([len(res[c["name"]][0]) for c in cases], np.int32)
    z["run_dyn"] = np.packbits(np.concatenate([res[c["name"]][0] for c in cases]))
    z["run_nfree"] = np.array([len(res[c["name"]][1]) for c in cases], np.int32)
    z["run_free"] = np.ascontiguousarray(np.concatenate([res[c["name"]][1] for c in cases]).astype(np.int32).T)
    z["run_info"] = np.stack([res[c["name"]][2] for c in cases]).astype(np.uint64)
    z["run_sha"] = np.array([case_sha(c) for c in cases], np.uint64)
    check_cases({c["name"]: c for c in cases}, res)
    return z


class Fixture:
    def __init__(self, z):
        self.z = z
        self.walk_at = {str(n): i for i, n in enumerate(z["walk_names"])}
        self.run_at = {str(n): i for i, n in enumerate(z["run_names"])}
        counts = z["walk_counts"].astype(np.int64)
        self.walk_vox = gold.unpack_lists(counts, z["walk_first"], z["walk_codes"])
        self.ray0 = np.concatenate([[0], np.cumsum(z["walk_m"].astype(np.int64))])
        self.vox0 = np.concatenate([[0], np.cumsum(counts)])
        self.dyn = np.unpackbits(z["run_dyn"])
        self.pt0 = np.concatenate([[0], np.cumsum(z["run_npts"].astype(np.int64))])
        self.free0 = np.concatenate([[0], np.cumsum(z["run_nfree"].astype(np.int64))])
        self.long_ray, self.long_count = z["long_ray"], int(z["long_count"])

    def walk(self, name):
        """(counts [m] int64, voxels [total][3] int64)"""
        i = self.walk_at[name]
        r0, r1 = self.ray0[i], self.ray0[i + 1]
        return self.z["walk_counts"][r0:r1].astype(np.int64), self.walk_vox[self.vox0[r0]:self.vox0[r1]]

    def walk_sha(self, name):
        return self.z["walk_sha"][self.walk_at[name]]

    def run(self, case):
        """(dynamic [n] uint8, free [k][3] int64, info [5] uint64)"""
        i = self.run_at[case["name"]]
        assert self.z["run_sha"][i] == case_sha(case), "the inputs of %s are not the ones the fixture was made from" % case["name"]
        assert self.z["run_npts"][i] == sum(len(s) for s in case["scans"])
        return (self.dyn[self.pt0[i]:self.pt0[i + 1]], self.z["run_free"][:, self.free0[i]:self.free0[i + 1]].T.astype(np.int64),
                self.z["run_info"][i])


def load(path=OUT):
    return Fixture(dict(np.load(path)))


# ---- what the cases are there for -----------------------------------------------------------------------------------------
def table_facts(case):
    """of a scene of voxel size 10: (bricks, slots, {slot: key} of the table, the same after two other insertion orders)"""
    bricks = sorted(vk.bricks_of(vk.voxels_of(np.concatenate(case["scans"]), case["vs"])))
    keys = sorted(vk.brick_key(*b) for b in bricks)
    slots = vk.slots_for(len(keys))
    rng = np.random.default_rng(7)
    return bricks, slots, vk.insert_all(keys, slots), [vk.insert_all(keys[::-1], slots), vk.insert_all([keys[i] for i in rng.permutation(len(keys))], slots)]


def check_cases(cases, res):
    """cases {name: case}, res {name: (dyn, free, info)} -- the reference's results, or the fixture's"""
    fr = lambda n: set(map(tuple, res[n][1].tolist()))     # noqa: E731
    info = lambda n: [int(v) for v in res[n][2]]           # noqa: E731  occupied, freed, after clustering, half-free, visits
    counts = lambda n: (sum(len(s) for s in cases[n]["scans"]), info(n)[0],      # noqa: E731
                        len(vk.bricks_of(vk.voxels_of(np.concatenate(cases[n]["scans"]), cases[n]["vs"]))))
    for n in cases:                                          # in the directed cases voxels_of counts what the reference counts
        if not (n.startswith("rand") or n.startswith("room") or n[1:].isdigit()):
            assert len({tuple(v) for v in vk.voxels_of(np.concatenate(cases[n]["scans"]), cases[n]["vs"]).tolist()}) == info(n)[0], n
    # a: the chain runs over the wrap whatever the order of insertion; lookups of missing bricks start inside it
    for slots, name, n_home in ((64, "chain64", (5, 3, 5)), (128, "chain128", None)):
        chain, empties = chain_selection(slots)
        homes = [vk.home(vk.brick_key(*b), slots) for b in chain]
        if n_home:
            assert [homes.count(h) for h in (slots - 1, 0, 1)] == list(n_home), homes
        assert homes.count(slots - 1) >= 3 and len(empties) >= 3
        bricks, table_slots, table, others = table_facts(cases[name])
        assert table_slots == slots and (len(bricks) <= 32 if slots == 64 else len(bricks) == 33), (name, len(bricks))
        assert set(chain) <= set(bricks)
        run = 0                                              # occupied slots in a row from the first home slot on
        while (slots - 1 + run) % slots in table:
            run += 1
        assert run >= len(chain) and slots - 1 in table and 0 in table
        for t in others:
            assert set(t) == set(table) and sorted(t.values()) == sorted(table.values())
        assert any(vk.probe_length(t, t[s], slots)[1] for t in [table] + others for s in t)       # a brick found past the wrap
        floor = cases[name]["scans"][0]
        looked = 0
        for b in empties[:3]:
            assert b not in bricks
            reads, wrapped = vk.probe_length(table, vk.brick_key(*b), slots)
            assert reads == run + 1 and wrapped              # from the last slot through the whole chain to its empty end
            c = _centres([(4 * b[0] + 1, 4 * b[1] + 1, 4 * b[2] + 1)], 10.0)[0]
            t = (c[2] - TABLE_O0[2]) / (floor[:, 2] - TABLE_O0[2])
            looked += bool((np.abs(TABLE_O0 + (floor - TABLE_O0) * t[:, None] - c).max(axis=1) < 1e-6).any())
        assert looked >= 2
        held = {tuple(v) for v in vk.voxels_of(cases[name]["scans"][1], 10.0).tolist()}
        chain_vox = {v for v in held if (v[0] >> 2, v[1] >> 2, v[2] >> 2) in set(chain)}
        assert chain_vox <= fr(name) and len(chain_vox) >= len(chain)
    # b, d: the counts on the boundaries
    assert counts("bricks32")[2] == 32 and counts("bricks33")[2] == 33
    assert vk.slots_for(32) == 64 and vk.slots_for(33) == 128
    for n in (255, 256, 257, 512, 513):
        assert counts("n%d" % n)[0] == n and len(cases["n%d" % n]["scans"]) == 3
        assert info("n%d" % n)[1] > info("n%d" % n)[2] > 0 and info("n%d" % n)[3] > 0 and 0 < res["n%d" % n][0].sum() < n
    assert counts("voxels256")[1] == 256 and counts("bricks256")[2] == 256
    assert counts("one_voxel") == (20, 1, 1) and counts("one_point") == (1, 1, 1)
    assert [len(s) for s in cases["scans9"]["scans"]] == [0, 1, 1, 0, 0, 1, 0, 1, 0] and fr("scans9") == {(2, 0, 0), (4, 0, 0)}
    assert counts("stack300_d0")[:2] == (301, 2) and len(cases["stack300_d0"]["scans"]) == 301
    assert fr("stack300_d0") == {(2, 3, 4)} and res["stack300_d0"][0].sum() == 300
    for d in ("d1", "d150", "dbig", "first_dbig"):
        assert not fr("stack300_" + d) and not res["stack300_" + d][0].any()
    assert len(cases["stack300_d0"]["scans"][300]) == 1 and np.array_equal(cases["stack300_d0"]["scans"][300],
                                                                          cases["stack300_first_dbig"]["scans"][0])
    assert cases["stack300_dbig"]["diff"] == BIG and cases["stack300_first_dbig"]["diff"] == BIG and cases["room3_cbig"]["cluster"] == BIG
    assert info("room3_cbig")[1] > 0 and info("room3_cbig")[2] == 0 and info("room3_cbig")[3] == 0
    # c: one component of the stated size, kept at cluster_size == size, gone at size + 1
    for shape, size in SHAPES:
        vox = shape_voxels(shape)
        comps = vk.components(vox)
        assert len(comps) == 1 and len(comps[0]) == size
        assert fr("%s_c%d" % (shape, size)) == set(vox) and info("%s_c%d" % (shape, size))[1] >= size
        assert fr("%s_c%d" % (shape, size + 1)) == set() and info("%s_c%d" % (shape, size + 1))[1] >= size
    st = np.array(shape_voxels("stairs"))
    assert (np.diff(st, axis=0) == 1).all()                  # corners only
    comps = vk.components(shape_voxels("comps600"))
    assert sorted(len(c) for c in comps) == [3] * 200 + [4] * 200 + [5] * 200
    assert all(len(vk.bricks_of(c)) >= 2 for c in comps)
    assert 190 <= sum(1 for c in comps if max(v[0] for v in c) < 0) <= 210
    assert fr("comps600_c4") == {v for c in comps if len(c) >= 4 for v in c} and info("comps600_c4")[1] >= 2400
    # e
    rand = ["rand%03d" % i for i in range(N_RANDOM)]
    assert sum(info(n)[1] for n in rand) >= E_FREED
    assert sum(info(n)[1] - info(n)[2] for n in rand) >= E_CLUSTERED
    assert sum(info(n)[3] for n in rand) >= E_HALF
    assert {cases[n]["vs"] for n in rand} == set(VS5) and {cases[n]["subvoxel"] for n in rand} == {True, False}
    assert fr("halffree_x_sub1") == {(-1, -1, 3)} and info("halffree_x_sub1")[3] == 1 and info("halffree_x_sub0")[3] == 0
    assert res["halffree_x_sub1"][0].tolist() == [0, 1, 1, 0, 0] and res["halffree_x_sub0"][0].tolist() == [0, 1, 0, 0, 0]
    assert fr("corner_x") == {(-1, -1, -1), (0, 0, 0)} and info("corner_x")[1] == 2
    # h
    assert counts("room8x8193")[0] == 65544 and 0 < info("room8x8193")[2] < info("room8x8193")[1]


if __name__ == "__main__":
    if not gold.have_ref():
        raise SystemExit("needs the reference checkout at %s (src/peopleremover/common.cc)" % gold.REF)
    z = compute()
    gold.save(z, OUT)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:6]:
        print("  %-20s %s %s" % (k, z[k].dtype, z[k].shape))
    print("  visits of the walk lists %d, of the long ray %d" % (int(z["walk_counts"].sum()), int(z["long_count"])))
    assert size <= MAX_BYTES, size
