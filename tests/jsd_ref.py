"""Literal fp64 NumPy restatement of the reference's spurious-bicluster scoring, the yardstick of resnmtf_jsd_pairs and
``resnmtf_amd.spurious``: ``bw.nrd0``, type-7 quantiles, ``BinDist``, ``stats::density`` (R <= 4.3, ``old.coords =
TRUE``, the FFT form as R writes it), ``approx``, ``jsd_calc`` (``R/utils.r:95-106``), ``get_thresholds`` /
``check_biclusters`` (``R/obtain_bicl.r:80-133``) and the removal step of ``obtain_biclusters`` (``:176-188``).
Indices are 0-based; every loop follows R's order."""
from __future__ import annotations

import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
M_1_SQRT_2PI = 0.398942280401432677939946059934


def quantile7(x, p):
    """``quantile(x, p, type = 7)``: index = 1 + (n - 1) p on the sorted vector."""
    xs = np.sort(np.asarray(x, dtype=np.float64))
    n = len(xs)
    index = 1.0 + (n - 1) * p
    lo, hi = math.floor(index), math.ceil(index)
    qs = xs[lo - 1]
    if index > lo and xs[hi - 1] != qs:
        h = index - lo
        qs = (1.0 - h) * qs + h * xs[hi - 1]
    return float(qs)


def sd(x):
    """``sd(x)``: R's mean with its refinement step (src/library/stats/src/cov.c), then the n - 1 sum of squares; a
    constant column gets exactly 0, which bw.nrd0's fallbacks test."""
    x = np.asarray(x, dtype=np.float64)
    m = np.sum(x) / len(x)
    m = m + np.sum(x - m) / len(x)
    return math.sqrt(float(np.sum((x - m) ** 2)) / (len(x) - 1))


def bw_nrd0(x):
    x = np.asarray(x, dtype=np.float64)
    if len(x) < 2:
        raise ValueError("need at least 2 data points")
    hi = sd(x)
    lo = min(hi, (quantile7(x, 0.75) - quantile7(x, 0.25)) / 1.34)
    if lo == 0:
        lo = hi
        if lo == 0:
            lo = abs(float(x[0]))
            if lo == 0:
                lo = 1.0
    return 0.9 * lo * len(x) ** (-0.2)


def seq_len_out(frm, to, n):
    """``seq.int(from, to, length.out = n)`` (src/main/seq.c: the symmetric form)."""
    out = np.empty(n)
    out[0] = frm
    if n > 1:
        out[n - 1] = to
    if n > 2:
        by = (to - frm) / (n - 1)
        for i in range(1, n - 1):
            out[i] = frm + i * by if i < n // 2 else to - (n - 1 - i) * by
    return out


def dnorm(x, sigma):
    """``stats::dnorm(x, 0, sigma)`` (nmath/dnorm.c)."""
    out = np.empty(len(x))
    lim = math.sqrt(-2 * math.log(2) * (-1021 + 1 - 53))
    for i, xi in enumerate(x):
        v = abs(xi / sigma)
        if v >= 2 * math.sqrt(DBL_MAX):
            out[i] = 0.0
        elif v < 5:
            out[i] = M_1_SQRT_2PI * math.exp(-0.5 * v * v) / sigma
        elif v > lim:
            out[i] = 0.0
        else:
            x1 = math.ldexp(float(np.rint(math.ldexp(v, 16))), -16)
            x2 = v - x1
            out[i] = M_1_SQRT_2PI / sigma * (math.exp(-0.5 * x1 * x1) * math.exp((-0.5 * x2 - x1) * x2))
    return out


def bin_dist(x, w, lo, up, n):
    """``BinDist`` (stats/src/massdist.c): length 2n, upper half zero."""
    y = np.zeros(2 * n)
    ixmin, ixmax = 0, n - 2
    xdelta = (up - lo) / (n - 1)
    for xi, wi in zip(x, w):
        xpos = (xi - lo) / xdelta
        ix = math.floor(xpos)
        fx = xpos - ix
        if ixmin <= ix <= ixmax:
            y[ix] += wi * (1 - fx)
            y[ix + 1] += wi * fx
        elif ix == -1:
            y[0] += wi * fx
        elif ix == ixmax + 1:
            y[ix] += wi * (1 - fx)
    return y


def approx(xs, ys, xout):
    """``approx(xs, ys, xout)`` (linear, rule = 1; stats/src/approx.c's bisection)."""
    out = np.empty(len(xout))
    n = len(xs)
    for k, v in enumerate(xout):
        i, j = 0, n - 1
        if v < xs[i] or v > xs[j]:
            out[k] = np.nan
            continue
        while i < j - 1:
            ij = (i + j) // 2
            if v < xs[ij]:
                j = ij
            else:
                i = ij
        if v == xs[j]:
            out[k] = ys[j]
        elif v == xs[i]:
            out[k] = ys[i]
        else:
            out[k] = ys[i] + (ys[j] - ys[i]) * ((v - xs[i]) / (xs[j] - xs[i]))
    return out


def _kords(lo, up, bw, n=512):
    kords = seq_len_out(0.0, 2 * (up - lo), 2 * n)
    kords[n + 1:2 * n] = -kords[n - 1:0:-1]                  # kords[(n + 2):(2 * n)] <- -kords[n:2]
    return dnorm(kords, bw)


def density(x, frm=None, to=None, n=512, cut=3, bw=None, direct=False):
    """``stats::density(x, from, to)`` with the defaults (gaussian, bw.nrd0, n = 512, cut = 3), R <= 4.3's coordinates.
    ``direct=True``: the convolution as the direct Toeplitz sum instead of the FFT form.  Returns (x, y)."""
    x = np.asarray(x, dtype=np.float64)
    nx = len(x)
    bw = bw_nrd0(x) if bw is None else bw
    frm = float(np.min(x)) - cut * bw if frm is None else frm
    to = float(np.max(x)) + cut * bw if to is None else to
    lo, up = frm - 4 * bw, to + 4 * bw
    y = bin_dist(x, np.full(nx, 1.0 / nx), lo, up, n)
    kords = _kords(lo, up, bw, n)
    if direct:
        d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
        conv = kords[d] @ y[:n]
    else:
        conv = np.real(np.fft.ifft(np.fft.fft(y) * np.conj(np.fft.fft(kords))))[:n]   # fft(., inverse = TRUE) / length(y)
    conv = np.maximum(0.0, conv)
    xords = seq_len_out(lo, up, n)
    xout = seq_len_out(frm, to, n)
    return xout, approx(xords, conv, xout)


def jsd(p, q):
    """``philentropy::JSD(rbind(p, q), unit = "log2", est.prob = "empirical")``."""
    P = p / np.sum(p)
    Q = q / np.sum(q)
    PQ = P + Q
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = np.where((P == 0) | (PQ == 0), 0.0, P * np.log2(2 * P / PQ))
        t2 = np.where((Q == 0) | (PQ == 0), 0.0, Q * np.log2(2 * Q / PQ))
    return 0.5 * (float(np.sum(t1)) + float(np.sum(t2)))


def column_stats(x):
    """What the scoring keeps of one column: the column sorted ascending with -0 as +0, ``bw.nrd0(x)`` and ``max(x)``."""
    x = np.asarray(x, dtype=np.float64)
    return np.sort(x) + 0.0, bw_nrd0(x), float(np.max(x))


def pair_stages(x1, x2):
    """``jsd_calc`` with its stages: both sides' densities on ``seq(0, max_val, 512)`` after the zeroing beyond the side's
    own maximum (un-normalised), and the value."""
    max_val = max(float(np.max(x1)), float(np.max(x2)))
    d1x, d1y = density(x1, 0.0, max_val)
    d2x, d2y = density(x2, 0.0, max_val)
    d1y[d1x > np.max(x1)] = 0.0
    d2y[d2x > np.max(x2)] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):     # a density that sums to 0: NaN, as in R
        return d1y, d2y, jsd(d1y, d2y)


def jsd_calc(x1, x2):
    return pair_stages(x1, x2)[2]


def bin_keys(x, M):
    """``floor(xpos)`` of every entry of ``x`` in ``BinDist`` as ``density(x, 0, M)`` calls it (512 bins from
    ``-4 bw`` to ``M + 4 bw``): keys 0 .. 510 feed bins ix and ix + 1, key -1 feeds bin 0 only, anything lower nothing."""
    x = np.asarray(x, dtype=np.float64)
    bw = bw_nrd0(x)
    lo, up = 0.0 - 4 * bw, M + 4 * bw
    xdelta = (up - lo) / 511
    return np.array([math.floor((xi - lo) / xdelta) for xi in x], dtype=np.int64)


def density_mode(scores):
    """``dens <- stats::density(scores); dens$x[which.max(dens$y)]``."""
    x, y = density(scores)
    return float(x[int(np.argmax(y))])


def null_pairs(K, R):
    """calculate_f_shuffle_jsd's order: j = 1..R-1, k, l = j+1..R, m -- as (repeat j, column k, repeat l, column m)."""
    return [(j, k, l, m) for j in range(R - 1) for k in range(K) for l in range(j + 1, R) for m in range(K)]


def get_thresholds(f_mess, n_views, jsd_fn=jsd_calc):
    R, K = len(f_mess), f_mess[0][0].shape[1]
    avg, mx = [], []
    for i in range(n_views):
        scores = np.array([jsd_fn(f_mess[j][i][:, k], f_mess[l][i][:, m]) for j, k, l, m in null_pairs(K, R)])
        avg.append(float(np.mean(scores)))
        mx.append(density_mode(scores))
    return np.array(avg), np.array(mx)


def check_biclusters(output_f, f_mess, jsd_fn=jsd_calc):
    n_views, K = len(output_f), output_f[0].shape[1]
    avg, mx = get_thresholds(f_mess, n_views, jsd_fn)
    score = np.zeros((n_views, K))
    for i in range(n_views):
        noise = np.concatenate([f[i] for f in f_mess], axis=1)
        for k in range(K):
            score[i, k] = np.mean([jsd_fn(output_f[i][:, k], noise[:, y]) for y in range(noise.shape[1])])
    return {"score": score, "avg_threshold": avg, "max_threshold": mx}


def removal(row_clusters, col_clusters, output_s, check):
    """obtain_biclusters :176-188 on clusters already reordered by relations (as res_nmtf_inner returns them)."""
    rows = [np.array(r, dtype=np.float64) for r in row_clusters]
    cols = [np.array(c, dtype=np.float64) for c in col_clusters]
    masks = []
    for i in range(len(rows)):
        relations = np.argmax(output_s[i], axis=0)
        indices = (check["score"][i] < check["max_threshold"][i]) | (check["score"][i] == 0)
        new = indices[relations]
        rows[i][:, new] = 0.0
        cols[i][:, new] = 0.0
        masks.append(new)
    return rows, cols, np.array(masks)
