"""The column pool of the JSD stage tests (tests/test_jsd_cases_host.py on the CPU, tests/test_gpu_jsd_stages.py on the
device) and its fp64 references from the NumPy restatement (tests/jsd_ref.py).  Every column is there for a branch of
csrc/resnmtf_jsd.hip.inc that the plain uniform / F-like columns never take; the host test asserts, from the restatement
alone, that each still reaches it.  References are computed once per size and shared (read-only) by every test."""
import functools

import numpy as np

import jsd_ref as J

NAMES = ("uniform", "flike", "const", "zeros", "iqr0", "mostly_zero", "few_levels", "tiny_scale", "signed", "all_negative",
         "neg_zero", "ascending", "descending", "outlier")
# tile = 2048 entries (one full tile, a one-entry right run at 2049 / 6145 / 8193, two full tiles, a lone left run that
# becomes a one-entry right run one width later at 8193); jsd_bin's chunk length ceil(n / 512) steps at 512 -> 513 and
# 1024 -> 1025; (n - 1) / 4 integral (the quartiles are entries) and not (they are interpolated)
SIZES = (2, 3, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6145, 8193)
LARGE_N = 100_000            # 49 tiles, six merge widths, chunk length 196, key 510 (outlier)
LARGE_NAMES = ("uniform", "flike", "outlier", "signed", "few_levels")
N_BINS = 512
TILE = 2048


def pool(n, seed):
    """n x 14, the columns of NAMES in order."""
    rng = np.random.default_rng(seed)
    c = {}
    c["uniform"] = rng.random(n)
    f = rng.random(n) ** 6
    c["flike"] = f / f.sum()
    c["const"] = np.full(n, 0.37)
    c["zeros"] = np.zeros(n)
    x = rng.random(n)                                   # IQR = 0, sd > 0: bw.nrd0's second fallback (lo = sd)
    x[rng.permutation(n)[:int(np.ceil(0.8 * n))]] = 0.25
    c["iqr0"] = x
    x = rng.random(n) ** 3
    x[rng.permutation(n)[:int(np.ceil(0.85 * n))]] = 0.0
    c["mostly_zero"] = x
    c["few_levels"] = np.round(6.0 * rng.random(n)) / 6.0 * 0.8      # 7 levels: bin runs over many whole chunks
    c["tiny_scale"] = rng.random(n) * 1e-6
    c["signed"] = 0.3 * rng.standard_normal(n) + 0.2    # negative entries: bin key -1 and the low clamp
    c["all_negative"] = -rng.random(n) - 0.1            # a density that is zeroed everywhere: NaN, as in R
    x = rng.random(n)
    x[rng.permutation(n)[:n // 2]] = -0.0
    c["neg_zero"] = x
    c["ascending"] = np.sort(rng.random(n))
    c["descending"] = np.sort(rng.random(n))[::-1].copy()
    x = rng.random(n) * 1e-3                            # one far maximum: bin key 510 at n >= 10 000
    x[int(rng.integers(n))] = 1.0
    c["outlier"] = x
    return np.stack([c[name] for name in NAMES], axis=1)


def all_pairs(n_cols):
    return np.array([(a, b) for a in range(n_cols) for b in range(n_cols)], dtype=np.int32)


class Reference:
    """The restatement's stages for a pool: ``sorted`` n x C, ``bw`` and ``mx`` per column, and per pair of ``pairs``
    the two zeroed densities ``dens`` P x 2 x 512 and the value ``val`` (NaN where R gives NaN)."""

    def __init__(self, cols, pairs):
        self.cols, self.pairs = cols, pairs
        st = [J.column_stats(cols[:, c]) for c in range(cols.shape[1])]
        self.sorted = np.stack([s[0] for s in st], axis=1)
        self.bw = np.array([s[1] for s in st])
        self.mx = np.array([s[2] for s in st])
        # pair_stages, with one side's density computed once per (column, max_val): it depends on nothing else
        memo = {}

        def side(c, max_val):
            if (c, max_val) not in memo:
                dx, dy = J.density(cols[:, c], 0.0, max_val)
                dy[dx > np.max(cols[:, c])] = 0.0
                memo[(c, max_val)] = dy
            return memo[(c, max_val)]

        self.dens = np.empty((len(pairs), 2, N_BINS))
        self.val = np.empty(len(pairs))
        for p, (a, b) in enumerate(pairs):
            max_val = max(float(np.max(cols[:, a])), float(np.max(cols[:, b])))
            self.dens[p, 0], self.dens[p, 1] = side(int(a), max_val), side(int(b), max_val)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.val[p] = J.jsd(self.dens[p, 0], self.dens[p, 1])
        for a in (self.cols, self.sorted, self.bw, self.mx, self.dens, self.val):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(n):
    """The pool of size n (seed n), all 14 x 14 ordered pairs."""
    cols = pool(n, n)
    return Reference(cols, all_pairs(cols.shape[1]))


@functools.lru_cache(maxsize=None)
def large_reference():
    cols = pool(LARGE_N, LARGE_N)[:, [NAMES.index(name) for name in LARGE_NAMES]].copy()
    return Reference(cols, all_pairs(cols.shape[1]))


def iqr_and_sd(x):
    return J.quantile7(x, 0.75) - J.quantile7(x, 0.25), J.sd(x)


def whole_chunk_runs(keys_sorted):
    """{key: the longest stretch of consecutive chunks of jsd_bin (ceil(n / 512) sorted entries each) that hold that key
    and no other}."""
    n = len(keys_sorted)
    L = -(-n // N_BINS)
    best, run_key, run_len = {}, None, 0
    for t in range(-(-n // L)):
        ch = keys_sorted[t * L:min(n, (t + 1) * L)]
        k = int(ch[0]) if ch[0] == ch[-1] else None
        run_len = run_len + 1 if (k is not None and k == run_key) else (1 if k is not None else 0)
        run_key = k
        if k is not None:
            best[k] = max(best.get(k, 0), run_len)
    return best
