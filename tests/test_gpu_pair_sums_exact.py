"""Every producer of pair sums against the extended-precision reference of tests/pair_sums_ref.py, at the tolerance that
module derives from the data (see its docstring; nothing here is a chosen constant).

The producer is selected by the batch size alone in the product library (chunk sums inside k_search / k_search_g8, the
slab epilogue of k_search_refill, k_accum + k_final, their several-links forms) and by the lab library's switches where a
path exists only there.  Per case: the pair list equals the oracle's bit for bit, n is exact, every block `want` did not
ask for is exactly 0, every other quantity is inside its derived tolerance AND that tolerance is at most a tenth of what
leaving out one pair would change, and a second call returns the same bits.

Each case prints `pair-sums <producer> worst |error| / tolerance`; DESIGN.md section 4 records those figures."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import pair_sums_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
LUM_D = [0.02, -0.01, 0.015, 1e-4, -2e-4, 1.5e-4]

_pairs_cache = {}
_fin_cache = {}


def _case(orc, N, pattern="all", far=False, mode=0, seed=1):
    """inputs, the oracle's pair list and the accumulation point; computed once per (N, pattern, far, mode) and not
    modified by anyone (the big hand-over sizes are not kept)"""
    key = (N, pattern, far, mode, seed)
    if key in _pairs_cache:
        return _pairs_cache[key]
    c = R.make_inputs(N, pattern, far, seed)
    md2 = 0.5 if (mode == 1 and pattern != "none") else c["maxd2"]
    ref = orc.Tree(c["model"], 20).get_pt_pairs(c["A"], c["d"], c["nr"], 0, N, mode, md2)
    ref["unit"] = R.unit_normals(c["nr"][ref["idx"] >= 0])
    out = (c, md2, ref, R.shift_of(c["model"], c["A"]))
    if N <= 300001:
        _pairs_cache[key] = out
    return out


def _reference(key, ref, shift, mode, want, D):
    """Finished reference + its discrimination ratios, shared by the cases that have the same pairs and `want`"""
    k = (key, want, D is not None)
    if k not in _fin_cache:
        pn = ref["unit"] if mode == 0 else ref["pn"]
        fin = R.finished(ref["p1"], ref["p2"], pn, shift, want, D)
        _fin_cache[k] = (fin, R.discrimination(ref["p1"], ref["p2"], pn, shift, want, D, fin=fin))
    return _fin_cache[k]


def _run_get_pt_pairs(tdtk, kd, orc, producer, N, pattern="all", far=False, mode=0, want=0, D=None):
    c, md2, ref, shift = _case(orc, N, pattern, far, mode)
    got = kd.getPtPairs(c["A"], c["d"], c["nr"], 0, N, max_dist_match2=md2, pairing_mode=mode, want=want, lum_D=D)
    assert got["n"] == ref["n"] and np.array_equal(got["idx"], ref["idx"])
    assert np.array_equal(got["p1"], ref["p1"]) and np.array_equal(got["p2"], ref["p2"])
    if mode != 0:
        assert np.array_equal(got["pn"], ref["pn"])
    elif want & tdtk.WANT_NAPX:
        assert np.array_equal(got["pn"], ref["unit"])     # the reference leaves PtPair's normal unset in mode 0
    else:
        assert not np.any(got["pn"])
    if pattern == "none":
        assert ref["n"] == 0
    elif pattern == "one":
        assert ref["n"] == 1 and ref["idx"][-1] >= 0
    elif pattern == "half":
        assert not np.any(ref["idx"][:N // 2] >= 0) and ref["n"] > 0.75 * (N - N // 2)
    elif pattern == "window":
        assert 0 < ref["n"] <= 100 and not np.any(ref["idx"][:-100] >= 0)
    else:
        assert ref["n"] > 0.75 * N                # (along the normal, pairing mode 1, fewer queries find a partner)
    fin, disc = _reference((N, pattern, far, mode), ref, shift, mode, want, D)
    R.check_struct(got["_raw"], fin, disc, producer)
    again = kd.getPtPairs(c["A"], c["d"], c["nr"], 0, N, max_dist_match2=md2, pairing_mode=mode, want=want, lum_D=D,
                          want_pairs=False)
    assert bytes(again["_raw"]) == bytes(got["_raw"]), producer      # the association is fixed: same bits every time


@pytest.fixture(scope="module")
def trees(tdtk, gpu):
    """the product library's tree over the model, near the origin and 1e6 away (built once)"""
    return {far: tdtk.KDtree(R.make_inputs(1, far=far)["model"], 20) for far in (False, True)}


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- base sums inside the search launch, by size --------------------------------------------------------------------
@pytest.mark.parametrize("N,pattern", [(1, "all"), (255, "all"), (257, "all"), (98303, "all")] +
                         [(5001, p) for p in R.PATTERNS])
def test_chunk_sums_of_k_search(tdtk, orc, trees, N, pattern):
    _run_get_pt_pairs(tdtk, trees[False], orc, "chunk sums, k_search", N, pattern)


@pytest.mark.parametrize("N", [98304, 262143])
@pytest.mark.parametrize("pattern", ["all", "half", "window"])
def test_chunk_sums_of_k_search_g8(tdtk, orc, trees, N, pattern):
    _run_get_pt_pairs(tdtk, trees[False], orc, "chunk sums, k_search_g8", N, pattern)


@pytest.mark.parametrize("N,pattern", [(262144, "all"), (262145, "all")] + [(300001, p) for p in R.PATTERNS])
def test_slab_epilogue_of_k_search_refill(tdtk, orc, trees, N, pattern):
    _run_get_pt_pairs(tdtk, trees[False], orc, "FUSE 3", N, pattern)


@pytest.mark.parametrize("which", ["last_fused", "minus_1", "first_k_accum"])
def test_base_sums_at_the_hand_over_to_k_accum(tdtk, orc, trees, which):
    """ceil(N / 256) < 28 num_cu keeps the sums inside the search launch: 28 num_cu 256 and that minus 1 are k_accum<0, 0>
    over more than one generation of waves, (28 num_cu - 1) 256 is the last size of the slab epilogue"""
    X = 28 * _cu() * 256
    N = {"last_fused": X - 256, "minus_1": X - 1, "first_k_accum": X}[which]
    _run_get_pt_pairs(tdtk, trees[False], orc, "FUSE 3" if which == "last_fused" else "k_accum<0,0> + k_final", N)


# ---- k_accum<WANT, PMODE> + k_final ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["all", "half"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("want", list(range(8)) + [R.WANT_GAPX, R.WANT_MOM2, "lum_D"])
def test_k_accum_matrix(tdtk, orc, trees, want, mode, pattern):
    D = LUM_D if want == "lum_D" else None
    want = R.WANT_LUM if want == "lum_D" else want
    # (want 0 in mode 0 is the chunk epilogue at this size; every other combination is k_accum)
    _run_get_pt_pairs(tdtk, trees[False], orc, "k_accum<%s,%d> + k_final" % (want, mode), 5001, pattern, False, mode, want, D)


def test_k_final_with_more_than_256_rows(tdtk, orc, trees):
    _run_get_pt_pairs(tdtk, trees[False], orc, "k_accum<7,0> + k_final, 257 rows", 257 * 1024, want=7)


@pytest.mark.parametrize("N", [5001, 300001])
@pytest.mark.parametrize("want", [0, 7])
def test_far_from_the_origin(tdtk, orc, trees, N, want):
    """cloud and pose 1e6 away: the tolerance is the one about the accumulation point, which a dropped or one-sided shift
    misses by six orders of magnitude (test_the_shift_is_what_makes_a_far_cloud_checkable)"""
    _run_get_pt_pairs(tdtk, trees[True], orc, "far, want %d, N %d" % (want, N), N, far=True, want=want)


# ---- several links in one call ----------------------------------------------------------------------------------------
def _links(tdtk, orc, specs):
    """one first scan (the model under a non-trivial dalignxf) and a second scan per (N, pattern, seed).  -> first tree
    handles, second handles, dalignxf per link, and per link the oracle's pairs"""
    base = R.make_inputs(1)
    first = tdtk.Scan([0, 0, 0], [0, 0, 0], base["model"])
    first.transform(base["A"], "INVALID")
    A = np.array(first.dalignxf, float)
    model = np.array(first.xyz_reduced_original)
    T = orc.Tree(model, 20)
    shift = R.shift_of(model, A)
    seconds, pairs = [], []
    for N, pattern, seed in specs:
        c = R.make_inputs(N, "all" if pattern == "away" else pattern, seed=seed)
        d = c["d"] + (R.AWAY if pattern == "away" else 0.0)
        sc = tdtk.Scan([0, 0, 0], [0, 0, 0], d)
        q = sc.get_xyz_reduced()
        seconds.append(sc)
        pairs.append(T.get_pt_pairs(A, q, None, 0, N, 0, 4.0))
    nl = len(specs)
    fh = (C.c_void_p * nl)(*[first.getSearchTree()._h for _ in specs])
    sh = (C.c_void_p * nl)(*[s.handle for s in seconds])
    dal = np.ascontiguousarray(np.stack([A] * nl))
    return dict(first=first, seconds=seconds, fh=fh, sh=sh, dal=dal, pairs=pairs, shift=shift, nl=nl)


LINK_SPECS = [(3000, "all", 11), (70001, "all", 12), (1, "all", 13), (3000, "away", 14)]


@pytest.fixture(scope="module")
def small_links(tdtk, orc, gpu):
    return _links(tdtk, orc, LINK_SPECS)


@pytest.mark.parametrize("want", [0, R.WANT_LUM, R.WANT_MOM2, R.WANT_GAPX])
def test_links_pair_sums(tdtk, orc, small_links, want):
    capi = import_module("3dtk_amd._capi")
    L = small_links
    assert L["pairs"][0]["n"] > 2700 and L["pairs"][1]["n"] > 63000 and L["pairs"][2]["n"] == 1 and L["pairs"][3]["n"] == 0

    def call():
        sums = (capi.PairSums * L["nl"])()
        capi.check(capi.lib().tdtk_links_pair_sums(L["nl"], L["fh"], capi.dptr(L["dal"]), L["sh"], 4.0, int(want), sums))
        return sums
    sums = call()
    for i, ref in enumerate(L["pairs"]):
        fin = R.finished(ref["p1"], ref["p2"], None, L["shift"], want)
        disc = R.discrimination(ref["p1"], ref["p2"], None, L["shift"], want, fin=fin)
        R.check_struct(sums[i], fin, disc, "links, want %d, link %d" % (want, i))
    assert bytes(call()) == bytes(sums)


def _check_lum_links(capi, L, producer):
    nl = L["nl"]

    def call():
        Cm = np.empty((nl, 36)); CD = np.empty((nl, 6)); m = (C.c_uint64 * nl)(); ss = np.empty(nl)
        capi.check(capi.lib().tdtk_lum_links(nl, L["fh"], capi.dptr(L["dal"]), L["sh"], 4.0, capi.dptr(Cm), capi.dptr(CD),
                                             m, capi.dptr(ss)))
        return Cm, CD, np.array(list(m)), ss
    Cm, CD, m, ss = call()
    for i, ref in enumerate(L["pairs"]):
        if "lum" not in ref:
            ref["lum"] = R.lum_link_and_one_less(ref["p1"], ref["p2"])
        (rm, MM, MZ, rss), (_, MM2, MZ2, rss2) = ref["lum"]
        assert int(m[i]) == rm and rm > 1000
        worst = 0.0
        # C = MM / ss and CD = MZ / ss as the library hands them out: MM = C ss, two more roundings (1 / ss, the product)
        for name, got, want, less in (("MM", Cm[i], MM, MM2), ("MZ", CD[i], MZ, MZ2), ("ss", ss[i:i + 1], [rss], [rss2])):
            for g, w, l in zip(np.asarray(got, float).ravel(), want, less):
                back = LD(g) * (LD(ss[i]) if name != "ss" else LD(1))
                tol = w.e + (2 * R.U * abs(w.v) if name != "ss" else 0)
                err = abs(back - w.v)
                if tol == 0:
                    assert err == 0, (producer, i, name)
                    continue
                worst = max(worst, float(err / tol))
                assert err <= tol, (producer, i, name, float(err / tol))
                assert abs(l.v - w.v) >= 10 * tol, (producer, i, name, "does not discriminate")
        print("pair-sums %-28s link %d worst |error| / tolerance = %.3f  (n = %d)" % (producer, i, worst, rm))
    again = call()
    for a, b in zip((Cm, CD, m, ss), again):
        assert np.array_equal(a, b), producer


BIG_LINK_SPECS = [(262144, "all", 21), (300001, "all", 22), (300001, "half", 23)]


def test_lum_links_summed_inside_the_search_launch(tdtk, orc, gpu):
    capi = import_module("3dtk_amd._capi")
    _check_lum_links(capi, _links(tdtk, orc, BIG_LINK_SPECS), "FUSE 5")


# ---- the producers only the lab library has ---------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", ["0", "1", "3"])
def test_lab_fuse_modes_at_the_fused_sizes(tdtk, orc, gpu, lab, monkeypatch, fuse):
    monkeypatch.setenv("TDTK_FUSE_SUMS", fuse)
    kd = tdtk.KDtree(R.make_inputs(1)["model"], 20)
    _run_get_pt_pairs(tdtk, kd, orc, "lab TDTK_FUSE_SUMS=" + fuse, 300001)


@pytest.mark.parametrize("env", [{"TDTK_LINK_FUSE": "0"}, {"TDTK_LINK_BATCH": "0"},
                                 {"TDTK_LINK_BATCH": "0", "TDTK_FUSE_LUM": "1"}], ids=lambda e: "+".join(sorted(e)))
def test_lab_ways_to_sum_a_lum_link(tdtk, orc, gpu, lab, monkeypatch, env):
    capi = import_module("3dtk_amd._capi")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = _links(tdtk, orc, [(300001, "all", 22), (300001, "half", 23)])
    _check_lum_links(capi, L, "lab " + " ".join("%s=%s" % kv for kv in sorted(env.items())))
