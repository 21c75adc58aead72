"""The host reference of one sweep (tests/sweep_ref.py) without a GPU: fed the oracle's own intermediates it must BE
the oracle's sweep, bit for bit, and its 2-byte quantiser must match hand-computed cases."""
import numpy as np
import pytest

from helpers import coupled_problem
from oracle import resnmtf_oracle as O
from resnmtf_amd import synth
from sweep_ref import fp16_split, half_image, half_scale, quantise, rel_stat, step_reference


def _oracle_sweep(prob, sweeps_before=2):
    """(before, after, err) of the oracle's own sweep number sweeps_before + 1."""
    rn, cn = prob.row_names, prob.col_names
    if rn is None:
        rn, cn = O.give_names(prob.data, prob.phi, prob.psi)
    ri, ci = O.reorder_data(rn), O.reorder_data(cn)
    f, s, g = [a.copy() for a in prob.init_f], [a.copy() for a in prob.init_s], [a.copy() for a in prob.init_g]
    lam, mu = O.explicit_init_lm(f, g)
    for _ in range(sweeps_before):
        f, s, g, lam, mu = O.update_matrices(prob.data, f, s, g, lam, mu, prob.phi, prob.xi, prob.psi, ri, ci, rn, cn)
    before = list(zip(f, s, g, lam, mu))
    f1, s1, g1, lam1, mu1 = O.update_matrices(prob.data, f, s, g, lam, mu, prob.phi, prob.xi, prob.psi, ri, ci, rn, cn)
    norms = np.array([np.linalg.norm(d, "fro") ** 2 for d in prob.data])
    err = O.calculate_error(prob.data, f1, s1, g1, norms)
    return before, list(zip(f1, s1, g1, lam1, mu1)), err, rn, cn


def _problems():
    yield "one view", synth.make_problem([(70, 50)], 4)
    yield "two views phi psi xi", synth.make_problem([(60, 40), (60, 40)], 3, phi=1.5, psi=0.7, xi=0.4)
    yield "two views partial names", coupled_problem([(50, 40), (45, 35)], 3, seed=3, phi_w=1.0, psi_w=0.5, xi_w=0.3)
    yield "three views partial + NA", coupled_problem([(50, 30), (40, 36), (44, 33)], 4, seed=5, phi_w=2.0, psi_w=1.0,
                                                       xi_w=0.5, na_pairs=((0, 2),))
    yield "three views, xi only", coupled_problem([(30, 20), (30, 25), (35, 20)], 2, seed=9, xi_w=1.0)


@pytest.mark.parametrize("name,prob", list(_problems()), ids=[p[0] for p in _problems()])
def test_step_reference_is_the_oracle_sweep_bitwise(name, prob):
    before, after, err, rn, cn = _oracle_sweep(prob)
    ref = step_reference(prob.data, before, after, prob.phi, prob.xi, prob.psi, rn, cn)
    for v in range(len(prob.data)):
        for i, key in enumerate(("f", "s", "g", "lam", "mu")):
            assert np.array_equal(ref[key][v], after[v][i]), f"{name}: {key} of view {v}"
    assert np.array_equal(ref["err"], err)


def test_step_reference_names_the_step():
    """A wrong device F is an F-step failure of exactly its size; the later steps' references are recomputed from it."""
    prob = synth.make_problem([(60, 40), (60, 40)], 3, phi=1.0)
    before, after, _, rn, cn = _oracle_sweep(prob)
    bad = [list(a) for a in after]
    bad[0][0] = bad[0][0].copy(); bad[0][0][5, 1] *= 1.001
    ref = step_reference(prob.data, before, bad, prob.phi, prob.xi, prob.psi, rn, cn)
    assert rel_stat(bad[0][0], ref["f"][0])[0] == pytest.approx(1e-3, rel=1e-6)
    for key, i in (("g", 2), ("s", 1), ("lam", 3)):      # (the oracle's own later steps came from the right F)
        assert rel_stat(after[0][i], ref[key][0])[0] > 0
    assert rel_stat(after[0][4], ref["mu"][0])[0] == 0      # (mu reads G alone)


def test_rel_stat_zero_entries():
    ref = np.array([[0.0, 2.0], [1.0, 0.0]])
    assert rel_stat(np.array([[0.0, 2.002], [0.999, 0.0]]), ref) == (pytest.approx(1e-3), 0)
    assert rel_stat(np.array([[1e-30, 2.0], [1.0, 0.0]]), ref)[1] == 1
    # non-finite entries are failures whatever the bar
    assert rel_stat(np.array([[0.0, np.nan], [1.0, 0.0]]), ref)[0] == np.inf
    assert rel_stat(np.array([[0.0, 2.0], [np.inf, 0.0]]), ref)[0] == np.inf
    assert rel_stat(np.array([[np.nan, 2.0], [1.0, 0.0]]), ref)[1] == 1
    assert rel_stat(np.array([np.nan]), np.array([1.0]))[0] > 1e300


def test_fp16_split_hand_cases():
    """The two-piece fp16 form of a factor entry: exact where hi + lo hold it, 2^-22 relative while lo is normal, and
    the absolute floor of the subnormal lo below b = 2^-16."""
    assert fp16_split(np.array([1.0, 0.5, 2.0 ** -20]))[:3].tolist() == [1.0, 0.5, 2.0 ** -20]
    assert fp16_split(np.array([1.0 + 2.0 ** -20]))[0] == 1.0 + 2.0 ** -20         # hi = 8192, lo = 2^-7 (normal)
    b = 1.0 + 2.0 ** -11 + 2.0 ** -23                                                # one bit below the 22 the pieces hold
    assert fp16_split(np.array([b]))[0] == 1.0 + 2.0 ** -11
    b = 2.0 ** -20 * (1.0 + 2.0 ** -20)                                             # lo = 2^-27: below fp16's 2^-24 floor
    assert fp16_split(np.array([b]))[0] == 2.0 ** -20
    assert fp16_split(np.array([b]))[0] != np.float32(b)


def test_u16_quantiser_hand_cases():
    x = np.array([[1.0, 0.5], [0.25, 0.0]], dtype=np.float32)
    scale = half_scale(x, True)
    assert scale == np.float32(65535.0)
    # 32767.5 and 16383.75: round half to even, and to nearest
    assert quantise(x, scale, True).tolist() == [[65535, 32768], [16384, 0]]
    # the clip at 65535, and ties to even
    assert quantise(np.array([2.0, 2.5, 3.5, 0.4999], np.float32), np.float32(65535.0), True)[0] == 65535
    assert quantise(np.array([2.5, 3.5, 0.5, 1.5], np.float32), np.float32(1.0), True).tolist() == [2, 4, 0, 2]
    assert quantise(np.array([65535.4, 65535.6, 70000.0], np.float32), np.float32(1.0), True).tolist() == [65535] * 3
    # scale from the largest entry: 65535 / max in f32
    y = np.array([[3.0, 1.0]], dtype=np.float32)
    assert half_scale(y, True) == np.float32(np.float32(65535.0) / np.float32(3.0))


def test_fp16_quantiser_hand_cases():
    one = np.float32(1.0)
    # ties to even: spacing 2 in [2048, 4096), 2^-10 in [1, 2)
    got = quantise(np.array([2049.0, 2051.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -12], np.float32), one, False)
    assert got.astype(np.float64).tolist() == [2048.0, 2052.0, 1.0, 1 + 2.0 ** -9, 1.0]
    # the power-of-two scale puts the largest entry in [2^13, 2^14)
    assert half_scale(np.array([1.0], np.float32), False) == np.float32(2.0 ** 13)
    assert half_scale(np.array([0.75, 0.1], np.float32), False) == np.float32(2.0 ** 14)
    assert half_scale(np.array([3e-4], np.float32), False) * np.float32(3e-4) >= 2.0 ** 13


@pytest.mark.parametrize("u16", [False, True])
def test_half_image_takes_the_scale_out(u16):
    x = np.array([[1.0, 0.3], [0.0, 0.7]])
    img, rel = half_image(x, u16)
    x32 = x.astype(np.float32)
    scale = half_scale(x32, u16)
    q = quantise(x32, scale, u16).astype(np.float64)
    assert np.array_equal(img, q / np.float64(scale))
    assert rel == pytest.approx(np.linalg.norm(img - x32.astype(np.float64)) / np.linalg.norm(x), rel=1e-15)
    assert img[0, 0] == 1.0 and img[1, 0] == 0.0
    assert 0 < rel < (2.0 ** -16 if u16 else 2.0 ** -11)
