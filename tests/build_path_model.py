"""The hand-over decisions of the device tree build (build.hip: make_build_plan, size_up_hand_over, look, hand_over,
enqueue_finishers; build_finish.inc: the finishers' tables), restated in plain Python over the exact level profile of the
host builder's tree (host_tree_levels) -- and the clouds that reach each outcome.  Shared by test_build_path_host.py
(CPU: does every cloud still take the path its row names?) and test_gpu_tree_build_paths.py (GPU: did the build take it?)."""
import functools

import numpy as np

FIN_LDS, FIN_LDS_HALF, FW_CAP, FIN_LV = 3584, 1792, 512, 96      # build_finish.inc
FIN_HANDOFF, FIN_HANDOFF_WAVE, FIN_HANDOFF_WAVE_FROM = 2048, 384, 2000000
BUILD_MAX_LEVELS = 4096                                          # build.hip


def fin_cap_of(M):
    return min(max(M // 128, 1024), 65536)


def predict(nseg, maxn, M, bucket):
    """(nseg, maxn): nodes per level and the largest of each (host_tree_levels).  Returns what KDtree.build_path() reports,
    without `respeculated` (that one is about the arithmetic of the sums, not about the shape of the tree)."""
    levels, cap = len(nseg), fin_cap_of(M)
    L = 0
    while (M >> L) > (FIN_HANDOFF_WAVE if M >= FIN_HANDOFF_WAVE_FROM else FIN_HANDOFF):
        L += 1
    r = dict(planned_level=L if (bucket >= 6 and L < 31 and (1 << L) <= cap) else None, handed_level=None, more_levels=0,
             retried=0, refused_size=0, refused_count=0, fin_nodes=0, fin_maxn=0, finishers=0, redone_by_levels=0, fin_cap=cap)
    lv = r["planned_level"]
    while lv is not None and lv < levels:                 # (a tree that ends above the level is done by levels)
        n, mx = int(nseg[lv]), int(maxn[lv])
        if r["retried"]:                                   # a look of the retry
            if mx <= FIN_LDS and n <= cap and lv + FIN_LV + 3 < BUILD_MAX_LEVELS:
                r["handed_level"] = lv
                break
            r["refused_size"] += mx > FIN_LDS
            r["refused_count"] += n > cap
            lv += 2
        elif mx > FIN_LDS and 2 * n <= cap and lv + 1 < 31:
            r["more_levels"] += 1
            lv += 1
        elif mx > FIN_LDS or n > cap:
            r["retried"] = 1
            lv += 2
        else:
            r["handed_level"] = lv
            break
    h = r["handed_level"]
    if h is not None:
        r["fin_nodes"], r["fin_maxn"] = n, mx
        staged, covered = n > 1024, 0
        if staged:
            r["finishers"], covered = 1, FW_CAP
            if mx > covered:
                r["finishers"], covered = r["finishers"] | 2, FIN_LDS_HALF
        if mx > covered:
            r["finishers"] |= 4
        if levels - 1 - h > FIN_LV:                        # more levels below the hand-over than the tables hold: by levels again
            r["redone_by_levels"], r["handed_level"] = 1, None
    return r


# ---- the clouds ---------------------------------------------------------------------------------------------------
def multi(rng, n): return rng.normal(0, 1, (n, 3)) * 10.0 ** rng.integers(-6, 1, (n, 1))
def lopsided(nu, nc, seed):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-1000, 1000, (nu, 3)), multi(rng, nc) + [300, -200, 50]])
    return np.ascontiguousarray(p[rng.permutation(len(p))])
def comb_in_field(k, ratio, e):          # a geometric comb inside one cell of a field of scale 2^e
    rng = np.random.default_rng(904)
    p = np.concatenate([rng.uniform(-1, 1, (40000, 3)) * 2.0 ** e, np.outer(ratio ** np.arange(k), [1.0, 0.5, 0.25])])
    return np.ascontiguousarray(p[rng.permutation(len(p))])
def comb_on_top(k):                      # a comb that the top levels peel off, a few points per level
    rng = np.random.default_rng(906)
    p = np.concatenate([rng.uniform(-1000, 1000, (40000, 3)), np.outer(2.0 ** np.arange(k), [1.0, 0.5, 0.25])])
    return np.ascontiguousarray(p[rng.permutation(len(p))])


CLOUDS = {
    "lopsided-50k-20k": lambda: lopsided(50000, 20000, 901),
    "lopsided-126k-5k": lambda: lopsided(126000, 5000, 901),
    "lopsided-127k-4k": lambda: lopsided(127000, 4000, 901),
    "lopsided-240k-60k": lambda: lopsided(240000, 60000, 905),
    "lopsided-270k-30k": lambda: lopsided(270000, 30000, 905),
    "comb-on-top-500": lambda: comb_on_top(500),
    "comb-in-field-200": lambda: comb_in_field(200, 8.0, 900),
    "comb-in-field-400": lambda: comb_in_field(400, 4.0, 900),
    # the finishers' tables hold FIN_LV + 1 = 97 levels of a subtree, its root's and 96 below it: with 374 teeth the tree
    # (bucket 20) has exactly 96 levels below level 5, with 375 it has 97
    "comb-in-field-374": lambda: comb_in_field(374, 4.0, 900),
    "comb-in-field-375": lambda: comb_in_field(375, 4.0, 900),
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    p = CLOUDS[name]()
    p.setflags(write=False)
    return p


# (row, cloud, bucket): the rows of the table in test_build_path_host.py
ROWS = [
    ("retry", "lopsided-50k-20k", 20),
    ("retry-then-count-alone", "lopsided-50k-20k", 7),
    ("count-alone", "lopsided-126k-5k", 20),
    ("tables-exactly-full", "lopsided-127k-4k", 20),
    ("tables-exactly-full", "lopsided-127k-4k", 7),
    ("retry-into-three-finishers", "lopsided-240k-60k", 20),
    ("retry-into-wave-alone", "lopsided-240k-60k", 7),
    ("retry-into-wave-and-half", "lopsided-270k-30k", 7),
    ("31-level-guard", "comb-on-top-500", 20),
    ("31-level-guard", "comb-on-top-500", 7),
    ("deep-inside-the-tables", "comb-in-field-200", 20),
    ("deep-inside-the-tables", "comb-in-field-200", 6),
    ("deeper-than-the-tables", "comb-in-field-400", 20),
    ("deeper-than-the-tables", "comb-in-field-400", 7),
    ("tables-exactly-deep", "comb-in-field-374", 20),
    ("one-level-deeper-than-the-tables", "comb-in-field-375", 20),
    ("bucket-bound", "lopsided-50k-20k", 6),
    ("bucket-bound", "lopsided-50k-20k", 5),
]
ROW_IDS = ["%s-b%d" % (r[0], r[2]) for r in ROWS]
