"""CPU tier of the device tree build's hand-over decisions: every cloud of tests/build_path_model.py still takes the path
its row names.  The exact level profile comes from the host builder (host_tree_levels: no device), the path from the
decision rule restated in build_path_model.predict.  test_gpu_tree_build_paths.py then asks the device build whether it
took that path; this file is what keeps each case on it when a constant, a generator or numpy's streams change.

The table (levels, counts and the finisher mask as the host profile gives them; "k x more": k times "one more level";
a refused look: largest node / nodes of the level):

| row                        | cloud                        | bucket | path                                                                 |
|----------------------------|------------------------------|--------|----------------------------------------------------------------------|
| retry                      | lopsided(50000, 20000, 901)  | 20     | planned 6, 4 x more; by levels from 10 (11900 / 1010, cap 1024); look 12 refused for both (7895 / 3544); handed at 14: 186 nodes, largest 870, full only |
| retry-then-count-alone     | same                         | 7      | look 12 refused for both (7895 / 3988), look 14 by the count alone (870 / 4002); handed at 16: 564 nodes, largest 257 |
| count-alone                | lopsided(126000, 5000, 901)  | 20     | 4 x more; by levels from 10 (4378 / 1024); look 12: 3259 fits, 4076 nodes > 1024; handed at 14: 462 nodes, largest 2478 |
| tables-exactly-full        | lopsided(127000, 4000, 901)  | 20, 7  | 4 x more; handed at 10 with fin_nodes == fin_cap == 1024, largest 3569 (15 under FIN_LDS); no retry |
| retry-into-three-finishers | lopsided(240000, 60000, 905) | 20     | planned 8, 3 x more; by levels from 11 (34074 / 2048, cap 2343); look 13 refused for both; handed at 15: 1824 nodes, largest 1949: wave + half + full |
| retry-into-wave-alone      | same                         | 7      | look 13 refused for both, look 15 by the count alone (1949 / 31188); handed at 17: 1808 nodes, largest 237: wave only |
| retry-into-wave-and-half   | lopsided(270000, 30000, 905) | 7      | looks 13 and 15 refused for both; handed at 17: 1726 nodes, largest 670: wave + half |
| 31-level-guard             | comb_on_top(500)             | 20, 7  | planned 5, 25 x more up to level 30, where the guard sends it by levels; looks 32 and 34 refused by the size alone; handed at 36: 16 nodes, largest 3369 |
| deep-inside-the-tables     | comb_in_field(200, 8.0, 900) | 20, 6  | handed at 5 (32 nodes, largest 1298); the tree has 80 / 88 levels: 74 / 82 below level 5; no redo |
| deeper-than-the-tables     | comb_in_field(400, 4.0, 900) | 20, 7  | handed at 5 (32 nodes, largest 1369); 108 / 114 levels: 102 / 108 below level 5, more than the 96 the tables hold: redone by levels |
| tables-exactly-deep        | comb_in_field(374, 4.0, 900) | 20     | handed at 5 (32 nodes, largest 1351); 102 levels: exactly the 96 below level 5 that the tables hold; no redo |
| one-level-deeper-than-...  | comb_in_field(375, 4.0, 900) | 20     | the same with 103 levels, 97 below level 5: redone by levels |
| bucket-bound               | the "retry" cloud            | 6, 5   | 6: planned 6 (handed at 16: 618 nodes, largest 257); 5: no finisher planned |
"""
import numpy as np
import pytest

import build_path_model as B

NONE = None
# planned, handed, more, retried, refused_size, refused_count, fin_nodes, fin_maxn, finishers, redone, fin_cap
TABLE = {
    ("retry", 20): (6, 14, 4, 1, 1, 1, 186, 870, 4, 0, 1024),
    ("retry-then-count-alone", 7): (6, 16, 4, 1, 1, 2, 564, 257, 4, 0, 1024),
    ("count-alone", 20): (6, 14, 4, 1, 0, 1, 462, 2478, 4, 0, 1024),
    ("tables-exactly-full", 20): (6, 10, 4, 0, 0, 0, 1024, 3569, 4, 0, 1024),
    ("tables-exactly-full", 7): (6, 10, 4, 0, 0, 0, 1024, 3569, 4, 0, 1024),
    ("retry-into-three-finishers", 20): (8, 15, 3, 1, 1, 1, 1824, 1949, 7, 0, 2343),
    ("retry-into-wave-alone", 7): (8, 17, 3, 1, 1, 2, 1808, 237, 1, 0, 2343),
    ("retry-into-wave-and-half", 7): (8, 17, 3, 1, 2, 2, 1726, 670, 3, 0, 2343),
    ("31-level-guard", 20): (5, 36, 25, 1, 2, 0, 16, 3369, 4, 0, 1024),
    ("31-level-guard", 7): (5, 36, 25, 1, 2, 0, 16, 3369, 4, 0, 1024),
    ("deep-inside-the-tables", 20): (5, 5, 0, 0, 0, 0, 32, 1298, 4, 0, 1024),
    ("deep-inside-the-tables", 6): (5, 5, 0, 0, 0, 0, 32, 1298, 4, 0, 1024),
    ("deeper-than-the-tables", 20): (5, NONE, 0, 0, 0, 0, 32, 1369, 4, 1, 1024),
    ("deeper-than-the-tables", 7): (5, NONE, 0, 0, 0, 0, 32, 1369, 4, 1, 1024),
    ("tables-exactly-deep", 20): (5, 5, 0, 0, 0, 0, 32, 1351, 4, 0, 1024),
    ("one-level-deeper-than-the-tables", 20): (5, NONE, 0, 0, 0, 0, 32, 1351, 4, 1, 1024),
    ("bucket-bound", 6): (6, 16, 4, 1, 1, 2, 618, 257, 4, 0, 1024),
    ("bucket-bound", 5): (NONE, NONE, 0, 0, 0, 0, 0, 0, 0, 0, 1024),
}
FIELDS = ("planned_level", "handed_level", "more_levels", "retried", "refused_size", "refused_count", "fin_nodes", "fin_maxn",
          "finishers", "redone_by_levels", "fin_cap")
# levels of the tree, and the profile (largest node, nodes) of the levels the path turns on
PROFILE = {
    ("retry", 20): (19, {10: (11900, 1010), 12: (7895, 3544), 14: (870, 186)}),
    ("retry-then-count-alone", 7): (21, {12: (7895, 3988), 14: (870, 4002), 16: (257, 564)}),
    ("count-alone", 20): (21, {10: (4378, 1024), 12: (3259, 4076), 14: (2478, 462)}),
    ("retry-into-three-finishers", 20): (21, {11: (34074, 2048), 13: (20772, 8002), 15: (1949, 1824)}),
    ("retry-into-wave-alone", 7): (22, {13: (20772, 8178), 15: (1949, 31188), 17: (237, 1808)}),
    ("retry-into-wave-and-half", 7): (23, {13: (17955, 8180), 15: (13286, 32290), 17: (670, 1726)}),
    ("31-level-guard", 20): (45, {30: (40050, 2), 32: (40020, 2), 34: (10836, 4), 36: (3369, 16)}),
    ("31-level-guard", 7): (48, {30: (40050, 8), 32: (40020, 8), 34: (10836, 8), 36: (3369, 16)}),
    ("deep-inside-the-tables", 20): (80, {}),
    ("deep-inside-the-tables", 6): (88, {}),
    ("deeper-than-the-tables", 20): (108, {}),
    ("deeper-than-the-tables", 7): (114, {}),
    ("tables-exactly-deep", 20): (5 + 1 + B.FIN_LV, {}),
    ("one-level-deeper-than-the-tables", 20): (5 + 2 + B.FIN_LV, {}),
}


@pytest.mark.parametrize("row,name,bucket", B.ROWS, ids=B.ROW_IDS)
def test_every_cloud_takes_the_path_its_row_names(tdtk, row, name, bucket):
    p = B.cloud(name)
    nseg, maxn = tdtk.host_tree_levels(p, bucket)
    # the profile is the tree's: every node and bucket counted once, one entry per level, the root holds every point
    _, st = tdtk.host_tree_layout(p, bucket)
    assert int(nseg.sum(dtype=np.uint64)) == st["internal"] + st["leaves"] and len(nseg) == st["depth"]
    assert (nseg[0], maxn[0]) == (1, len(p)) and nseg.min() >= 1 and int(maxn[1:].max()) < len(p)
    got = B.predict(nseg, maxn, len(p), bucket)
    assert got == dict(zip(FIELDS, TABLE[(row, bucket)])), got
    if (row, bucket) in PROFILE:
        levels, at = PROFILE[(row, bucket)]
        assert len(nseg) == levels
        assert {l: (int(maxn[l]), int(nseg[l])) for l in at} == at
    if row == "31-level-guard":
        assert p.max() == 2.0 ** 499 and np.isfinite(3 * p.max() ** 2)            # every square finite
    if row == "deeper-than-the-tables":
        with np.errstate(over="ignore"):
            assert 8.4e270 < p.max() < 8.5e270 and not np.isfinite(p.max() ** 2)   # extents square to infinity


def test_host_tree_levels_of_small_trees_and_errors(tdtk):
    """A single bucket is one level; a profile deeper than the caller's arrays is still counted; errors as host_tree_layout's."""
    nseg, maxn = tdtk.host_tree_levels(np.array([[1.0, 2.0, 3.0]]), 20)
    assert nseg.tolist() == [1] and maxn.tolist() == [1]
    p = np.random.default_rng(1).uniform(-1, 1, (1000, 3))
    nseg, maxn = tdtk.host_tree_levels(p, 1)
    _, st = tdtk.host_tree_layout(p, 1)
    assert len(nseg) == st["depth"] and int(nseg.sum()) == st["internal"] + st["leaves"] and maxn[-1] == 1
    assert nseg[1] == 2 and maxn[1] >= 500
    short = tdtk.host_tree_levels(p, 1, cap=3)       # the wrapper asks again with room for every level
    assert np.array_equal(short[0], nseg) and np.array_equal(short[1], maxn)
    with pytest.raises(tdtk.TdtkError):
        tdtk.host_tree_levels(np.zeros((0, 3)), 20)
    with pytest.raises(tdtk.TdtkError):
        tdtk.host_tree_levels(np.zeros((5, 3)), 0)
