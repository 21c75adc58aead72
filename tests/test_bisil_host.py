"""The bisilhouette without a device: the restatement (bisil_ref) on a hand-computed 6 x 4 view and on edge cases,
the host combination of resnmtf_amd.bisil on stand-in silhouettes, and the k sweep of apply_resnmtf through a
stand-in runner (R/main.r:269-334)."""
import math
import warnings

import numpy as np
import pytest

import bisil_ref as B
import resnmtf_amd
from resnmtf_amd import api, bisil

# bicluster 0 = rows {0, 1, 2} x columns {0, 1}, bicluster 1 = rows {3, 4, 5} x columns {2, 3}
X = np.array([[1, 0, 0, 0],
              [2, 1, 0, 0],
              [4, 0, 0, 0],
              [0, 0, 1, 0],
              [0, 0, 2, 0],
              [0, 0, 4, 0]], dtype=np.float64)
RC = np.array([[1, 0], [1, 0], [1, 0], [0, 1], [0, 1], [0, 1]], dtype=np.float64)
CC = np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=np.float64)


def _s(a, b):
    return (b - a) / max(a, b)


def _hand(metric):
    """Silhouettes of X worked out by hand: rows of bicluster 0 on columns {0, 1} are (1, 0), (2, 1), (4, 0), the rows
    of bicluster 1 there are 0; columns of bicluster 0 on rows {0, 1, 2} are (1, 2, 4), (0, 1, 0), those of bicluster
    1 there are 0.  Bicluster 1 is 1-D: rows (1, 0), (2, 0), (4, 0) on columns {2, 3}, columns (1, 2, 4) and 0."""
    r5, r2, r21 = math.sqrt(5), math.sqrt(2), math.sqrt(21)
    if metric == "euclidean":
        rows0 = [_s((r2 + 3) / 2, 1), _s((r2 + r5) / 2, r5), _s((3 + r5) / 2, 4)]
        cols0 = [_s(math.sqrt(18), r21), _s(math.sqrt(18), 1)]
    elif metric == "manhattan":
        rows0 = [_s((2 + 3) / 2, 1), _s((2 + 3) / 2, 3), _s((3 + 3) / 2, 4)]
        cols0 = [_s(6, 7), _s(6, 1)]
    else:
        c = 1 - 2 / r5
        rows0 = [_s(c / 2, 1), _s(c, 1), _s(c / 2, 1)]
        cols0 = [_s(1 - 2 / r21, 1), _s(1 - 2 / r21, 1)]
    if metric == "cosine":
        rows1, cols1 = [1.0, 1.0, 1.0], [0.0, -1.0]
    else:
        rows1, cols1 = [_s(2, 1), _s(1.5, 2), _s(2.5, 4)], [0.0, -1.0]
    rs = np.zeros((6, 2)); cs = np.zeros((4, 2))
    rs[:3, 0] = rows0; rs[3:, 1] = rows1
    cs[:2, 0] = cols0; cs[2:, 1] = cols1
    return rs, cs


@pytest.mark.parametrize("metric", ["euclidean", "manhattan", "cosine"])
def test_hand_computed_6x4(metric):
    rs, cs = B.silhouettes(X, RC, CC, metric)
    hr, hc = _hand(metric)
    np.testing.assert_allclose(rs, hr, atol=1e-15)
    np.testing.assert_allclose(cs, hc, atol=1e-15)
    sigma = [0.5 * (hr[:3, 0].mean() + hc[:2, 0].mean()), 0.5 * (hr[3:, 1].mean() + hc[2:, 1].mean())]
    assert bisil.view_score(RC, CC, rs, cs) == pytest.approx(np.mean(sigma), abs=1e-15)
    assert bisil.score([RC], [CC], metric, sil=lambda v, rc, cc, d: B.silhouettes(X, rc, cc, d)) == \
        pytest.approx(np.mean(sigma), abs=1e-15)
    assert B.bisil([X], [RC], [CC], metric) == pytest.approx(np.mean(sigma), abs=1e-15)


def test_singleton_and_empty_biclusters():
    rng = np.random.default_rng(1)
    x = rng.random((8, 6))
    rc = np.zeros((8, 3)); cc = np.zeros((6, 3))
    rc[0, 0] = 1; cc[:3, 0] = 1                 # singleton I_0
    rc[1:5, 1] = 1; cc[3:, 1] = 1
    cc[:, 2] = 1                                 # no rows: inactive
    rs, cs = B.silhouettes(x, rc, cc, "euclidean")
    assert rs[0, 0] == 0.0                       # |I_k| = 1
    assert not rs[:, 2].any() and not cs[:, 2].any()
    assert np.all(rs[5:, :] == 0)                # non-members
    assert rs[1:5, 1].any()


def test_single_active_bicluster_scores_zero():
    x = np.random.default_rng(2).random((7, 5))
    rc = np.zeros((7, 2)); cc = np.zeros((5, 2))
    rc[:4, 0] = 1; cc[:3, 0] = 1; rc[4:, 1] = 1          # bicluster 1 has no columns
    rs, cs = B.silhouettes(x, rc, cc, "manhattan")
    assert not rs.any() and not cs.any()                  # no l left for b
    assert bisil.view_score(rc, cc, rs, cs) == 0.0


def test_overlap_excludes_self_from_b():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [5.0, 0.0], [6.0, 0.0]])
    rc = np.array([[1, 0], [1, 1], [0, 1], [0, 1]], dtype=np.float64)     # row 1 is in both
    cc = np.array([[1, 1], [1, 1]], dtype=np.float64)
    rs, _ = B.silhouettes(x, rc, cc, "euclidean")
    # row 1 in bicluster 0: a = d(1, 0) = 1; b = mean over I_1 \ {1} = (4 + 5) / 2 -- not over I_1 with itself
    assert rs[1, 0] == pytest.approx(_s(1.0, 4.5), abs=1e-15)
    # row 1 in bicluster 1: a = mean(4, 5); b over I_0 \ {1} = {0}: 1
    assert rs[1, 1] == pytest.approx(_s(4.5, 1.0), abs=1e-15)


def test_zero_norm_cosine():
    assert B.dist([0, 0], [0, 0], "cosine") == 0.0
    assert B.dist([0, 0], [1, 2], "cosine") == 1.0
    assert B.dist([1, 0], [0, 3], "cosine") == pytest.approx(1.0)
    x = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    rc = np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=np.float64)
    cc = np.ones((2, 2))
    rs, _ = B.silhouettes(x, rc, cc, "cosine")
    np.testing.assert_allclose(rs[:, 0], [1.0, 1.0, 0.0, 0.0])           # a = 0 (both zero), b = 1 (one zero)
    np.testing.assert_allclose(rs[2:, 1], [1.0, 1.0], atol=1e-15)        # parallel: a = 0, b = 1


def test_overall_is_the_mean_of_non_zero_view_scores():
    assert bisil.overall([0.0, 0.0]) == 0.0
    assert bisil.overall([0.4, 0.0, 0.2]) == pytest.approx(0.3)
    assert bisil.overall([0.5, -0.5]) == 0.0                               # the sum is 0
    assert bisil.overall([0.5, -0.25, 0.0]) == pytest.approx(0.125)


def test_host_combination_on_stand_in_silhouettes():
    rc = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], dtype=np.float64)
    cc = np.array([[1, 0, 1], [0, 1, 0], [0, 1, 0]], dtype=np.float64)    # bicluster 2 has no rows
    rs = np.array([[0.2, 0, 0], [0.4, 0, 0], [0, -0.1, 0], [0, 0.3, 0]])
    cs = np.array([[0.6, 0, 0], [0, 0.5, 0], [0, 0.1, 0]])
    want = 0.5 * (0.5 * (0.3 + 0.6) + 0.5 * (0.1 + 0.3))
    assert bisil.view_score(rc, cc, rs, cs) == pytest.approx(want)
    calls = []

    def stand_in(v, r, c, d):
        calls.append((v, d))
        return (rs, cs) if v == 0 else (np.zeros_like(rs), np.zeros_like(cs))

    assert bisil.score([rc, rc], [cc, cc], "manhattan", sil=stand_in) == pytest.approx(want)   # view 1 scores 0
    assert calls == [(0, "manhattan"), (1, "manhattan")]
    with pytest.raises(ValueError, match="shapes"):
        bisil.view_score(rc, cc, rs[:, :2], cs)
    with pytest.raises(ValueError, match="distance"):
        bisil.score([rc], [cc], "chebyshev", sil=stand_in)
    with pytest.raises(ValueError, match="engine"):
        bisil.score([rc], [cc], "euclidean")


def _runner(scores, log=None):
    def run(k):
        if log is not None:
            log.append(k)
        return {"bisil": scores[k], "k": k, "row_clusters": [np.ones((20, k))], "col_clusters": [np.ones((12, k))]}
    return run


_DATA = [np.abs(np.random.default_rng(0).standard_normal((20, 12)))]


def _sweep(scores, log=None, **kw):
    kw = {"k_min": 3, "k_max": 6, "spurious": False, "stability": False, "k_sweep": True, "return_sweep": True, **kw}
    return resnmtf_amd.apply_resnmtf(_DATA, sweep_runner=_runner(scores, log), **kw)


def test_sweep_first_maximum_wins():
    log = []
    res = _sweep({3: 0.2, 4: 0.5, 5: 0.5, 6: 0.1}, log)
    assert res["k"] == 4                                   # which.max: the first of the tied maxima
    assert log == [3, 4, 5, 6]
    assert res["k_sweep"] == {"k": [3, 4, 5, 6], "bisil": [0.2, 0.5, 0.5, 0.1]}


def test_sweep_extends_while_the_largest_k_wins():
    log = []
    res = _sweep({3: 0.1, 4: 0.2, 5: 0.3, 6: 0.4, 7: 0.5, 8: 0.45}, log)
    assert log == [3, 4, 5, 6, 7, 8]
    assert res["k"] == 7
    assert res["k_sweep"]["k"] == [3, 4, 5, 6, 7, 8]


def test_sweep_stops_at_the_cap_with_a_warning():
    log = []
    data = [np.abs(np.random.default_rng(1).standard_normal((20, 5)))]   # cap = min(ncol, 64) = 5
    with pytest.warns(UserWarning, match="stops at k = 5"):
        res = resnmtf_amd.apply_resnmtf(data, k_min=3, k_max=4, spurious=False, stability=False, k_sweep=True,
                                        return_sweep=True, sweep_runner=_runner({3: 0.1, 4: 0.2, 5: 0.3}, log))
    assert log == [3, 4, 5] and res["k"] == 5


def test_sweep_forwards_remove_unstable(monkeypatch):
    seen = {}

    def fake_stability_check(data, results, k, *args, **kwargs):
        seen["k"] = k
        seen["remove_unstable"] = args[-1]
        return {"res": results, "relevance": None}

    monkeypatch.setattr(api, "stability_check", fake_stability_check)
    res = _sweep({3: 0.2, 4: 0.6, 5: 0.1, 6: 0.3}, stability=True, remove_unstable=False)
    assert seen == {"k": [4], "remove_unstable": False}
    assert res["res"]["k"] == 4
    _sweep({3: 0.2, 4: 0.6, 5: 0.1, 6: 0.3}, stability=True)
    assert seen["remove_unstable"] is True


def test_sweep_argument_errors():
    run = _runner({})
    for k_min, k_max in ((5, 5), (6, 3)):
        with pytest.raises(ValueError, match="k_max must be greater than k_min"):
            resnmtf_amd.apply_resnmtf(_DATA, k_min=k_min, k_max=k_max, spurious=False, stability=False, k_sweep=True,
                                      sweep_runner=run)
    with pytest.raises(ValueError, match="k_min must be a positive integer"):
        resnmtf_amd.apply_resnmtf(_DATA, k_min=2.5, k_max=4, spurious=False, stability=False, k_sweep=True, sweep_runner=run)
    with pytest.raises(ValueError, match="k_max must be a numeric"):
        resnmtf_amd.apply_resnmtf(_DATA, k_max="8", spurious=False, stability=False, k_sweep=True, sweep_runner=run)
    with pytest.raises(ValueError, match="ranks"):
        resnmtf_amd.apply_resnmtf(_DATA, k_min=3, k_max=13, spurious=False, stability=False, k_sweep=True, sweep_runner=run)
    with pytest.raises(ValueError, match="distance"):
        resnmtf_amd.apply_resnmtf(_DATA, distance="chebyshev", spurious=False, stability=False, k_sweep=True,
                                  sweep_runner=run)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.apply_resnmtf(_DATA, stability=False, k_sweep=True, sweep_runner=run)
    with pytest.raises(ValueError, match="no_clusts"):
        resnmtf_amd.apply_resnmtf(_DATA, spurious=False, stability=False, no_clusts=True, k_sweep=True, sweep_runner=run)
    import scipy.sparse
    with pytest.raises(NotImplementedError, match="sparse"):
        resnmtf_amd.apply_resnmtf([scipy.sparse.random(20, 12, density=0.5, random_state=0, format="csc")],
                                  spurious=False, stability=False, k_sweep=True, sweep_runner=run)
    with pytest.raises(NotImplementedError, match="sparse"):
        resnmtf_amd.res_nmtf_inner([scipy.sparse.random(20, 12, density=0.5, random_state=0, format="csc")], None, None,
                                   k_vec=[3], spurious=False, score_bisil=True)
    with pytest.raises(NotImplementedError, match="k sweep"):               # without the opt-in: as before
        resnmtf_amd.apply_resnmtf(_DATA, stability=False, spurious=False)
