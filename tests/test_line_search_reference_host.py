"""CPU tier of the line-search edge cases (tests/line_search_cases.py): the oracle's FindClosestAlongDir and its
getPtPairs in pairing mode 1 against the reference's own compiled tree (oracle/_ref, where present) on every case the GPU
tier runs -- the oracle is what travels to the GPU machine, this file is what pins it -- and two properties of the
oracle's answers that need no library: the returned point's d recomputed in the reference's association, and brute force.

Measured here (oracle, 256 CUs assumed for `trips`): rows / with a partner / without / with d2 < 0
  trips 20,016 sampled of 1,118,577 / 8,027 / 11,989 / 8      deep_b1 2,400 / 2,234 / 166 / 174
  deep_b20 2,400 / 2,235 / 165 / 233                          table 600 / 224 / 376 / 25
  on_the_line_uniform 3,000 / 3,000 / 0 / 1,071               on_the_line_lattice 1,500 / 1,500 / 0 / 341
  directions_uniform 1,600 / 1,383 / 217 / 216                directions_lattice 1,200 / 1,140 / 60 / 0
  nonfinite_q 110 / 81 / 29 / 0                               sizes 2,049 / 1,985 / 64 / 0
  maxdist2 (64 rows each) 0.0: 1 / 63 / 1   -1.0: 0 / 64 / 64   1e-300: 5 / 59 / 1   inf, 1e300: 64 / 0 / 1   NaN: 0 / 64 / 0
  normals_mode1 40,000 rows, 21,485 pairs; normals_mode1_lattice 1,500 rows, 1,384 pairs; `trips` in mode 1: 7,864 pairs on the sampled rows
The file takes 43 s on the CPU with the reference library, 25 s of it the two deep cases (far out in the geometric
part neither walk prunes anything: 3 to 4 ms per query)"""
import numpy as np
import pytest

import line_search_cases as L

_answers = {}


def _need_ref(orc):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (no reference checkout on this box)")


def _oracle(orc, name):
    """(case, idx, d2 of the compared rows); the answers are computed once per case and left alone"""
    c = L.find_closest_case(name, orc.have_ref())
    if name not in _answers:
        q, u = L.compared(c)
        _answers[name] = orc.Tree(c["model"], c["bucket"]).find_closest_along_dir(q, u, c["maxdist2"])
    return (c,) + _answers[name]


@pytest.mark.parametrize("name", L.FIND_CLOSEST_NAMES)
def test_oracle_find_closest_along_dir_equals_reference(orc, name):
    _need_ref(orc)
    c, idx, _ = _oracle(orc, name)
    q, u = L.compared(c)
    want = orc.RefTree(c["model"], c["bucket"]).find_closest_along_dir(q, u, c["maxdist2"])
    assert L.equal(idx, want), name


@pytest.mark.parametrize("name", L.MODE1_NAMES + ("trips",))
def test_oracle_get_pt_pairs_mode1_equals_reference(orc, name):
    _need_ref(orc)
    if name == "trips":
        c = L.trips()
        data, nr = c["data"][c["rows"]], c["dirs"][c["rows"]]
    else:
        c = L.mode1_case(name)
        data, nr = c["q"], c["dirs"]
    with np.errstate(all="ignore"):
        got = orc.Tree(c["model"], c["bucket"]).get_pt_pairs(c["A"], data, nr, mode=1, maxdist2=c["maxdist2"])
        want = orc.RefTree(c["model"], c["bucket"]).get_pt_pairs(c["A"], data, nr, mode=1, maxdist2=c["maxdist2"])
    assert got["n"] == want["n"]
    for k in ("idx", "p1", "p2", "pn"):
        assert L.equal(got[k], want[k]), (name, k)
    hit, miss = L.shares(got["idx"])
    print("%s mode 1: %d rows, %d pairs" % (name, len(data), got["n"]))
    if name == "normals_mode1_lattice":      # the rotated, normalised normal is exact, whole rows of points tie
        assert L.equal(np.abs(got["pn"]).sum(1), np.ones(got["n"]))
        assert L.tied_rows(c["model"], c["local"][got["idx"] >= 0], got["pn"]) >= 500
    else:
        assert hit >= 0.1 and miss >= 0.1


@pytest.mark.parametrize("name", L.FIND_CLOSEST_NAMES)
def test_returned_d_is_the_references_expression(orc, name):
    """Len2(p2p) - sqr(Dot(p2p, dir)) of the returned point, sums left to right, is the oracle's d2 bit for bit; a row
    without a partner keeps maxdist2.  Also what each case promises about its own rows."""
    c, idx, d2 = _oracle(orc, name)
    q, u = L.compared(c)
    hit = idx >= 0
    print("%s: %d rows, %d with a partner, %d without, %d with d2 < 0, %d with d2 == 0"
          % (name, len(q), hit.sum(), (~hit).sum(), (d2 < 0).sum(), (d2 == 0).sum()))
    assert L.equal(d2[hit], L.line_d(c["model"], q, u, idx)[hit])
    assert L.equal(d2[~hit], np.full(int((~hit).sum()), c["maxdist2"]))
    if name == "trips":
        assert min(L.shares(idx)) >= 0.1
    if name.startswith("on_the_line"):
        assert (d2 < 0).sum() >= 100 and (d2 == 0).sum() >= 100
    if name == "table":
        assert np.isin(idx[c["through"]], c["copies"]).sum() >= 8
        assert (~np.isin(idx[c["beside"]], c["copies"])).sum() >= 8
    if name == "directions_lattice":
        assert hit[c["axis"]].sum() >= 100


# (deep_b1 and deep_b20 are left out: see below)
BRUTE_FORCE_NAMES = [n for n in L.FIND_CLOSEST_NAMES if not n.startswith("deep")]


@pytest.mark.parametrize("name", BRUTE_FORCE_NAMES)
def test_no_point_is_closer_than_the_returned_one(orc, name):
    """For rows with finite input and a unit direction (the first 2,000 of them), no model point has a smaller d than the
    returned one, and none has d < maxdist2 where nothing was returned.  This can legitimately fail only where rounding in
    the sphere test pruned a marginally better point, so it keeps the cases where the oracle has no such row: every case
    but deep_b1 and deep_b20 (86 and 18 of 2,000 rows there: with coordinates of 1e85 next to a core of size 100,
    |v|^2 - (v.u)^2 cancels to noise far larger than any radius)."""
    c, idx, d2 = _oracle(orc, name)
    q, u = L.compared(c)
    sel = np.nonzero(L.is_unit_finite(q, u))[0][:2_000]
    assert len(sel) >= min(64, len(q)) // 2
    best = L.brute_min_d(c["model"], q[sel], u[sel], chunk=max(1, 4_000_000 // len(c["model"])))
    got = np.where(idx[sel] >= 0, d2[sel], c["maxdist2"])
    assert not (best < got).any(), np.nonzero(best < got)[0][:10]
