"""The counted instantiations of the ANN normals kernel (ann.hip, k_ann_normals<KMAX, true>), which bench.py's roofline takes the
launch's algorithmic bytes from and no other test launches: with tdtk_visit_counting on, counters 4, 5 and 6 are the oracle's
summed splitting-node visits, leaf-point visits and the number of queries, and lists and normals are bit-equal to the same call
with counting off."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RPOS = [3.0, -2.0, 10.0]


def _cloud(name):
    rng = np.random.default_rng(2110)
    if name == "exp_line":
        return np.outer(2.0 ** np.arange(60), [1.0, 0.5, 0.25])      # depth 59 > the 12 LDS levels: the spill columns under COUNT
    n = {"uniform3000": 3000, "uniform2000": 2000, "second_trip": 1024 * 256 + 193}[name]
    return rng.uniform(-100.0, 100.0, (n, 3))


# second_trip: more points than the grid's 1024 x 256 threads -- 193 lanes make a second grid-stride trip, the last wave is partial
@pytest.mark.parametrize("name,k,eps", [("uniform3000", 10, 1.0), ("exp_line", 10, 1.0), ("uniform2000", 16, 1.0),
                                        ("uniform2000", 32, 0.3), ("second_trip", 10, 1.0)])
def test_counted_kernel_tallies_the_oracles_visits(tdtk, orc, gpu, name, k, eps):
    p = _cloud(name)
    L = tdtk.lib()
    _, _, want = orc.AnnTree(p).ksearch(p, k, eps, want_visits=True)
    plain, pknn = tdtk.calculateNormalsApxKNN(p, k, RPOS, eps, want_knn=True)
    c = (C.c_uint64 * 8)()
    assert L.tdtk_visit_counting(gpu, 1) == 0
    try:
        counted, cknn = tdtk.calculateNormalsApxKNN(p, k, RPOS, eps, want_knn=True)
        assert L.tdtk_visit_counters(gpu, c) == 0
    finally:
        L.tdtk_visit_counting(gpu, 0)
    assert (c[4], c[5], c[6]) == (want[0], want[1], len(p))
    assert np.array_equal(cknn, pknn) and np.array_equal(counted, plain, equal_nan=True)
