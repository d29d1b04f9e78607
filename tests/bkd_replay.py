"""What the CPU tier (test_bkd_host.py) and the GPU tier (test_gpu_bkd.py) of the dynamic kd-forest share: a case's script of
tests/golden/make_golden_bkd.py replayed through an implementation, every layout, remove result and answer against the fixture
k19_bkd.npz.  An implementation has insert(pts), remove(pts) -> (ids, containers or None), layout() -> (counts, the ids of the
slots in order and sorted inside each, the buffer) and find_closest / knn / fixed_range over query arrays."""
import numpy as np

import bkd_model


def ways(mk, case, a, b):
    """the three ways an INS of a layout case is made: one call, one point per call, ragged calls"""
    n = b - a
    yield "one", [n]
    if case.name.startswith("lay_"):
        yield "single", [1] * n
        yield "ragged", mk.ragged(n, case.b)


def check_queries(case, fx, i, impl, xyz, live):
    """the answers of impl (find_closest / knn / fixed_range over arrays) at op i against the fixture; live: the ids in the forest"""
    pre = "%s_q%d_" % (case.name, i)
    Q = case.Q
    d2_of = lambda ids, q: np.where(ids >= 0, bkd_model.dist2(xyz[np.maximum(ids, 0)], q), -1.0)      # noqa: E731
    for j, md in enumerate(case.md2):
        idx, d2 = impl.find_closest(Q, md)
        want = fx[pre + "fc%d_id" % j]
        assert set(idx[idx >= 0].tolist()) <= live, (pre, j)
        if case.ties:
            assert np.array_equal(d2, fx[pre + "fc%d_d2" % j]), (pre, j)
            uniq = want >= 0
            assert np.array_equal(idx[uniq], want[uniq]), (pre, j)
            assert np.array_equal(idx < 0, d2 < 0), (pre, j)
            if case.sets:
                off, tids = fx[pre + "fc%d_toff" % j], fx[pre + "fc%d_tids" % j]
                for qi in np.nonzero(~uniq)[0]:
                    assert (idx[qi] < 0 and off[qi] == off[qi + 1]) or idx[qi] in tids[off[qi]:off[qi + 1]], (pre, j, qi)
        else:
            assert np.array_equal(idx, want), (pre, j)
        assert np.array_equal(d2, np.array([d2_of(idx[qi:qi + 1], Q[qi])[0] for qi in range(len(Q))])), (pre, j)
    for k in case.ks:
        idx, d2 = impl.knn(Q, k)
        want = fx[pre + "knn%d_id" % k]
        assert set(idx[idx >= 0].tolist()) <= live, (pre, k)
        for qi in range(len(Q)):
            row = idx[qi]
            assert np.array_equal(d2[qi], d2_of(row, Q[qi])), (pre, k, qi)
            have = row[row >= 0]
            assert len(set(have.tolist())) == len(have), (pre, k, qi)
            if case.ties:
                assert np.array_equal(d2[qi], fx[pre + "knn%d_d2" % k][qi]), (pre, k, qi)
                uniq = want[qi] >= 0
                assert np.array_equal(row[uniq], want[qi][uniq]), (pre, k, qi)
            else:
                assert np.array_equal(row, want[qi]), (pre, k, qi)
        if case.sets:
            off, tids = fx[pre + "knn%d_toff" % k], fx[pre + "knn%d_tids" % k]
            n_have = (fx[pre + "knn%d_d2" % k] >= 0).sum(1)
            pos = 0
            for qi in range(len(Q)):
                for j in range(n_have[qi]):
                    assert idx[qi, j] in tids[off[pos]:off[pos + 1]], (pre, k, qi, j)
                    pos += 1
    for j, r2 in enumerate(case.r2):
        off, ids = impl.fixed_range(Q, r2)[:2]
        assert set(ids.tolist()) <= live, (pre, j)
        woff, wids = fx[pre + "rng%d_off" % j], fx[pre + "rng%d_ids" % j]
        assert np.array_equal(np.asarray(off, np.int64), woff.astype(np.int64)), (pre, j)
        for qi in range(len(Q)):
            got = np.sort(ids[off[qi]:off[qi + 1]])
            if case.ties and not np.array_equal(got, wids[woff[qi]:woff[qi + 1]]):
                # copies: which of them is left is free, their coordinates are not
                key = lambda v: sorted(map(tuple, xyz[v].tolist()))      # noqa: E731
                assert key(got) == key(wids[woff[qi]:woff[qi + 1]]), (pre, j, qi)
            elif not case.ties:
                assert np.array_equal(got, wids[woff[qi]:woff[qi + 1]]), (pre, j, qi)


def replay(mk, case, fx, impl, calls=None):
    """the case's script through impl (insert / remove / layout / the three queries); every CHK, REM and QRY against the fixture.
    Where copies make ids free (case.ties) the model follows impl's choices and checks that each was admissible."""
    m = bkd_model.Model(case.b, case.P[:case.ctor]) if case.ctor else bkd_model.Model(case.b)
    for i, (code, a, b) in enumerate(case.ops):
        if code == mk.INS:
            p = a
            for n in (calls(a, b) if calls else [b - a]):
                impl.insert(case.P[p:p + n])
                p += n
            m.insert(case.P[a:b])
        elif code == mk.REM:
            got, conts = impl.remove(case.R[a:b])
            want, wcont = fx["%s_r%d_id" % (case.name, i)], fx["%s_r%d_cont" % (case.name, i)]
            assert [g >= 0 for g in got] == (want >= 0).tolist(), (case.name, i, got)
            if conts is not None:
                assert list(conts) == wcont.tolist(), (case.name, i)
            if not case.ties:
                assert list(got) == want.tolist(), (case.name, i)
            for p, g in zip(case.R[a:b], got):
                m.remove(p, int(g))            # asserts: the lowest container, the nearest point there
        elif code == mk.CHK:
            counts, ids, buf = impl.layout()
            mc, mi, mb = m.layout()
            assert counts == mc and ids == [x for s in mi for x in s] and buf == mb, (case.name, i)
            pre = "%s_c%d_" % (case.name, i)
            assert counts == fx[pre + "counts"].tolist() and len(buf) == len(fx[pre + "buf"]), (case.name, i)
            if not case.ties:
                assert ids == fx[pre + "ids"].tolist() and buf == fx[pre + "buf"].tolist(), (case.name, i)
        elif code == mk.QRY:
            check_queries(case, fx, i, impl, m.xyz, set(m.live_ids()))
    return m
