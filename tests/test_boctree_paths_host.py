"""The octree search tree on the paths tests/golden/k20_boctree_search.npz does not reach: the CPU tier.  The restatement
(tests/boctree_model.py) and the host build of the walk (oct_lane.h under tests/host_oct_shim.h) against
tests/golden/k22_boctree_paths.npz -- the reference's own compiled BOctTree<double> on clouds of 1 to 257 points, on runs of
exactly 10 and 11 at both ends of the sorted keys, on groups of more than 10 identical points, a planar cloud and a 21-level
tree that is searched -- and the walk as a program of its own (tests/oct_walk_main.cc) under -fsanitize=undefined, on every
batch of both fixtures and at the refusal bound itself, where x + closest_v is 2^31 - 2."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import boctree_model as bm

gen = bm.load_generator("make_golden_boctree_paths")
gen20 = bm.generator()
CASES = [(name, voxel, early) for name, variants in gen.CASES for voxel, early in variants]


@pytest.fixture(scope="module")
def fx():
    return gen.load()


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    return bm.host_lane(tmp_path_factory.mktemp("oct_host"))


def test_fixture_is_what_the_generator_says(fx):
    """under the size bound; the clouds, queries and radii are the generator's; the cases and nothing else"""
    assert os.path.getsize(gen.OUT) <= gen.MAX_BYTES
    c = gen.clouds()
    q = gen.queries(c)
    keys = set()
    for name, variants in gen.CASES:
        assert bm.same_bits(fx.cloud(name), c[name]), name
        assert bm.same_bits(fx.queries(name), q[name][0]) and tuple(fx.z[name + "_maxd2"]) == q[name][1], name
        keys |= {name + "_q", name + "_maxd2"} | ({name + "_sha256"} if name in gen.NOT_STORED else {name, name + "_g"})
        if name + "_q_g" in fx.z:
            keys.add(name + "_q_g")
        for voxel, early in variants:
            got = fx.batches(name, voxel, early)
            assert len(got) == len(q[name][1])
            for qq, maxd2, pos, d2, leaves in got:
                assert len(pos) == len(d2) == len(leaves) == len(qq)
            keys |= {gen.prefix(name, voxel, early) + k for k in ("scalars", "counts", "leaf", "pos", "d2", "leaves")}
    assert keys == set(fx.z)
    assert len(CASES) == 5 * len(gen.SWEEP_N) + 11 and [len(c["sweep_n%d" % n]) for n in gen.SWEEP_N] == list(gen.SWEEP_N)


@pytest.mark.parametrize("name,voxel,early", CASES)
def test_model_and_host_lane_equal_fixture(fx, lane, name, voxel, early):
    """the restatement's scalars, counts and leaf order are the reference's; the host walk's point, Dist2 and leaves scanned
    are the reference's by bits, no query left out"""
    m = bm.model_of(fx, name, voxel, early)
    bm.check_model_equals_fixture(fx, m, name, voxel, early)
    assert bm.check_lane_equals_batches(lane, m, fx, name, voxel, early) == len(fx.queries(name)) * len(fx.z[name + "_maxd2"])


def test_the_cases_reach_what_they_are_there_for(fx):
    """on the restatement (which the test above ties to the reference): runs of exactly 10 and 11 at sorted position 0 and
    n - 1; groups of more than 10 identical points as leaves at full depth behind a chain of single children; 21 levels"""
    for name, (n_lo, n_hi) in gen.ENDS:
        lv = gen.leaves_of(bm.model_of(fx, name, 0.5, 1))
        assert (lv[0][:2] == (0, 10)) == (n_lo == 10) and (lv[-1][1] == 10) == (n_hi == 10)
    m = bm.model_of(fx, "heavy", 0.125, 1)
    lv, pts = gen.leaves_of(m), fx.cloud("heavy")[m.leaf]
    full = max(d for _, _, d in lv)
    for cnt, p in gen.HEAVY_GROUPS:
        (a, k, d), = [x for x in lv if (pts[x[0]:x[0] + x[1]] == p).all(1).any()]
        assert k == cnt and (d == full) == (cnt > 10)
    m = bm.model_of(fx, "eleven", 0.001, 1)
    assert len(m.nodes) == 11 and all(bin(int(v) & 0xFF).count("1") == 1 for v in m.nodes[:10, 0])         # one child per node: lo == hi at every level
    m = bm.model_of(fx, "deep", gen.DEEP_VOXEL, 0)
    assert m.max_depth == 22 and gen.leaf_depths(m).max() == 21


def test_fixture_equals_the_reference():
    """the generator, run again on the live reference, gives the stored arrays"""
    if not gen.have_ref():
        pytest.skip("no reference checkout (src/slam6d/Boctree.cc)")
    z = np.load(gen.OUT)
    got = gen.compute()
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].dtype == z[k].dtype and got[k].shape == z[k].shape, k
        same = bm.same_bits(got[k], z[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], z[k])
        assert same, k


# ---- the bound: what the entry points admit may not let x +- closest_v leave int32 ---------------------------------------------
def test_the_bound_refuses_what_could_leave_int32(lane):
    """every case the rule refuses is refused by oct_host_find, every other is answered; an admitted |x| + closest_v stays
    at 2^31 - 2 or below"""
    m = bm.bound_tree()
    for tag, q, maxd2, admitted in bm.bound_cases(m):
        got = bm.lane_find(lane, m, q, maxd2)
        assert (got is not None) == admitted, tag
        if admitted:
            x = np.trunc((q + m.add) * m.mult)
            assert np.abs(x).max() + int(bm.bound_cv(m, maxd2)) <= 2 ** 31 - 2


# ---- the walk as a program of its own, under the undefined-behaviour sanitizer ------------------------------------------------
def _job(m, q, maxd2):
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    assert m.pts.dtype.itemsize == 32 and m.nodes.dtype == np.uint32
    return b"".join([struct.pack("<3q", len(m.nodes), len(m.pts), len(q)), struct.pack("<5d", *m.add, m.mult, maxd2),
                     struct.pack("<iI", int(m.largest_index), int(m.top_bit)), m.nodes.tobytes(), m.pts.tobytes(), q.tobytes()])


def _answer(j, got):
    if got is None:
        return ["job %d refused" % j]
    slot, d2, leaves = got
    return ["job %d %d" % (j, len(slot))] + ["%d %016x %d" % (s, b, l) for s, b, l in zip(slot, np.ascontiguousarray(d2).view(np.uint64), leaves)]


def test_walk_runs_clean_under_the_sanitizer_as_a_program_of_its_own(fx, lane, tmp_path):
    """tests/oct_walk_main.cc, built with -fsanitize=undefined -fno-sanitize-recover=all and run as a child process, on every
    batch of k20 and k22 and on the bound cases: exit status 0, its output the shared library's walk"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "oct_walk")
    csrc = os.path.join(bm.ROOT, "3dtk_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=all"]
    # whether this g++ can link the sanitizer's runtime at all: a program with nothing in it that could fail otherwise
    probe = str(tmp_path / "probe.cc")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + flags + [probe, "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode:
        pytest.skip("g++ cannot link the sanitizer runtime: " + (r.stderr.strip().splitlines() or ["no message"])[-1])
    r = subprocess.run(["g++"] + flags + ["-I" + os.path.join(bm.ROOT, "include"), "-I" + csrc, "-I" + os.path.join(bm.ROOT, "tests"),
                                          os.path.join(bm.ROOT, "tests", "oct_walk_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    jobs, want = [], []

    def add(m, q, maxd2):
        want.extend(_answer(len(jobs), bm.lane_find(lane, m, q, maxd2)))
        jobs.append(_job(m, q, maxd2))
    fx20 = gen20.load()
    for f, cases in ((fx20, fx20.cases()), (fx, CASES)):
        for name, voxel, early in cases:
            m = bm.model_of(f, name, voxel, early)
            for qq, maxd2, _, _, _ in f.batches(name, voxel, early):
                add(m, qq, maxd2)
            if f is fx20 and (name, voxel, early) in set(gen20.EDGE_CASES):
                for q1, maxd2, _, _, _ in f.edge(name, voxel, early):
                    add(m, q1[None], maxd2)
    n_fixture = len(jobs)
    mb = bm.bound_tree()
    for tag, q, maxd2, admitted in bm.bound_cases(mb):
        add(mb, q, maxd2)
    path = str(tmp_path / "jobs.bin")
    with open(path, "wb") as fh:
        fh.write(b"".join(jobs))
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr
    got = r.stdout.split("\n")
    assert got[-1] == "" and got[:-1] == want
    assert n_fixture == sum(len(f.batches(*c)) for f, cs in ((fx20, fx20.cases()), (fx, CASES)) for c in cs) + 2 * gen20.EDGE_QUERIES * len(gen20.EDGE_CASES)
    assert sum(w.endswith("refused") for w in want) == sum(not a for _, _, _, a in bm.bound_cases(mb))
