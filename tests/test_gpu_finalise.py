"""``resnmtf_finalise`` on constructed factors against ``oracle.normalisation_check`` + ``binary_clusters``.

``set_factors`` with F, S, G built on the host (tests/data_ref.py: ``finalise_case``), then ``finalise``; no sweep runs,
so the comparison the sweep tests forgive ("identical except entries on the 1/n threshold") is the one made here:

* F / G outputs: ``max |got / ref - 1| <= (2 len + 2) 2^-53`` (``data_ref.factor_bar``: the device's and the oracle's
  column sum, each of at most ``len`` non-negative terms in its own order, and one division);
* S output: ``(2 n + 2 m + 4) 2^-53`` (``data_ref.s_bar``);
* the cluster matrices: identical to the reference.  Entries of the normalised factor within the F / G bar of 1 / len
  could fall on either side; the inputs are chosen so that NO entry lies in that band unless a case puts it there on
  purpose (asserted, on the CPU as well: tests/test_data_ref_host.py), and the cases that do (an all-equal column, with
  and without one entry raised by an ulp) have column sums that are exact in any order -- so nothing is excused.

The constructed cases are those no factorisation run produces: a non-identity ``relations`` at k = 17 and 64, a tie in
an S column (the first maximum wins, like which.max), an all-zero S column (relation 0), two S columns with one
arg-max (a duplicated row-cluster column), an entry exactly on 1 / n under the strict ``>``, and a dead F column (NaN
output column, zero S column, zero cluster column -- the oracle agrees).

Out of scope: S with non-finite entries.  R's ``which.max`` skips NaN, NumPy's ``argmax`` returns the first NaN and the
kernel's ``v > best`` never selects one; the three differ, and the loop never hands finalise such an S.

Measured on the MI355X (printed as ``MEASURED ...``): F 4.4e-16 (bar 5.7e-14, random_257x300_k17), G 4.4e-16 (bar
6.7e-14, same case), S 7.8e-16 (bar 4.0e-13, perm_diag_k64).
"""
import numpy as np
import pytest

import data_ref as D
from resnmtf_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", D.FINALISE_IDS)
def test_finalise_matches_the_oracle(cid):
    c = D.finalise_case(cid)
    n, m, k = c["n"], c["m"], c["k"]
    rf, rs, rg, rrc, rcc = D.finalise_reference(c["F"], c["S"], c["G"])
    # the excuse list: band entries a case did not put there on purpose -- there are none
    assert int(D.threshold_band(rf, n).sum()) == c["band"] and int(D.threshold_band(rg, m).sum()) == 0
    with Engine([n], [m], [k]) as e:
        e.set_factors(0, c["F"], c["S"], c["G"])
        f, s, g, rc, cc = e.finalise(0)
        again = e.finalise(0)
    for a, b in zip((f, s, g, rc, cc), again):                      # (finalise changes nothing on the handle)
        assert np.array_equal(a, b, equal_nan=True)
    failures = []
    for name, got, ref, bar in (("F", f, rf, D.factor_bar(n)), ("G", g, rg, D.factor_bar(m)), ("S", s, rs, D.s_bar(n, m))):
        worst, nz, nan = D.nan_stat(got, ref)
        print(f"MEASURED {cid} {name}: {worst:.3e} (bar {bar:.3e})")
        if worst > bar or nz or nan:
            failures.append(f"{name}: max |got / ref - 1| = {worst:.3e} (bar {bar:.3e}), {nz} non-zero where the reference "
                            f"is zero, {nan} NaN on one side only")
    assert not failures, "\n".join(failures)
    assert np.array_equal(cc, rcc), f"column clusters differ in {np.count_nonzero(cc != rcc)} entries"
    assert np.array_equal(rc, rrc), (f"row clusters differ in {np.count_nonzero(rc != rrc)} entries, columns "
                                     f"{sorted(set(np.nonzero(rc != rrc)[1].tolist()))}")
    # what the case is about, stated on the device's own output
    rel = np.argmax(s, axis=0)
    for j, i in c["relations"].items():
        assert rel[j] == i
    kind = c["kind"]
    if kind == "same_arg_max":
        assert np.array_equal(rc[:, 1], rc[:, 7]) and rc[:, 1].any()
    if kind == "zero_s_column":
        assert np.all(s[:, 5] == 0.0)
    if kind == "equal_f_column":
        assert np.all(f[:, 6] == 1.0 / n) and not rc[:, 10].any()
    if kind == "equal_f_column_one_ulp":
        assert rc[:, 10].sum() == 1.0 and rc[D.ULP_ROW, 10] == 1.0
    if kind == "zero_f_column":
        assert np.isnan(f[:, 4]).all() and np.all(s[:, 4] == 0.0) and not rc[:, 11].any()
