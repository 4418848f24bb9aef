"""Extended-precision reference of the weighted quantiles (trpl_weighted_quantiles*, include/trpl.h) and the inputs its tests
share: tests/test_quantiles_host.py proves reference and inputs on the CPU, tests/test_gpu_quantiles.py holds the kernels to
them.  A helper, not a test; nothing here imports the product package.

Per column: the used rows (weight finite and > 0) sorted by key, keys equal as numbers joined into one tie group, the groups'
cumulative weights cum_g in numpy.longdouble (64-bit mantissa on x86-64), sw = the last of them.
    FIRST_ABOVE: the key of the first group with cum_g > q sw;   LAST_BELOW: the key of the last group with cum_g < q sw (NaN
    if there is none).
A NaN key in a used row, or no used row, gives NaN.

The device forms the same sums in fp64 in another order.  An n-term fp64 sum of non-negative terms is within n 2^-53 of the
exact one relative to the sum, and q sw inherits sw's error plus one rounding, so the device may place a group whose cum_g
lies within  delta = 4 n 2^-53 sw  of q sw on the other side of q sw.  Such a (column, request) pair is AMBIGUOUS: the device's
result may be the selection at q sw - delta or the one at q sw + delta (the two neighbouring distinct keys); every other
result must equal the reference key with ==.  At most CAP of a case's pairs may be ambiguous -- asserted before anything is
compared, and proven for every input family on the CPU."""
import functools

import numpy as np

LD = np.longdouble
FIRST_ABOVE, LAST_BELOW = 1, 2                 # TRPL_Q_FIRST_ABOVE, TRPL_Q_LAST_BELOW (the host test compares them with the header)
CAP = 0.01


def used_rows(W):
    W = np.asarray(W, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(W) & (W > 0)


def default_rules(q):
    return [LAST_BELOW if v < 0.5 else FIRST_ABOVE for v in q]


def _pick(keys, cum, th, rule):
    if rule == FIRST_ABOVE:
        i = int(np.searchsorted(cum, th, side="right"))               # the first cum > th
        return keys[i] if i < len(keys) else np.nan
    i = int(np.searchsorted(cum, th, side="left")) - 1                # the last cum < th
    return keys[i] if i >= 0 else np.nan


def reference(Y, W, q, rule):
    """Y (ncols, >= n) keys, W (n,) weights, K requests -> dict(want (K, ncols), ambiguous (K, ncols) bool, below / above
    (K, ncols): the selections at q sw -+ delta)."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    W = np.asarray(W, dtype=np.float64)
    n, K, ncols = W.size, len(q), Y.shape[0]
    used = used_rows(W)
    w = W[used].astype(LD)
    out = {k: np.full((K, ncols), np.nan) for k in ("want", "below", "above")}
    out["ambiguous"] = np.zeros((K, ncols), dtype=bool)
    if not used.any():
        return out
    for c in range(ncols):
        y = Y[c, :n][used]
        if np.isnan(y).any():
            continue
        y = y + 0.0                                                    # -0.0 and +0.0 are one point
        order = np.argsort(y, kind="stable")
        ys, cw = y[order], np.cumsum(w[order])
        last = np.flatnonzero(np.append(ys[1:] != ys[:-1], True))      # the last row of every tie group
        keys, cum = ys[last], cw[last]
        sw = cum[-1]
        delta = 4 * n * LD(2.0) ** -53 * sw
        for k in range(K):
            t = LD(q[k]) * sw
            out["want"][k, c] = _pick(keys, cum, t, rule[k])
            out["below"][k, c] = _pick(keys, cum, t - delta, rule[k])
            out["above"][k, c] = _pick(keys, cum, t + delta, rule[k])
            out["ambiguous"][k, c] = bool(np.any(np.abs(cum - t) <= delta))
    return out


def _same(a, b):
    with np.errstate(invalid="ignore"):
        return (a == b) | (np.isnan(a) & np.isnan(b))


def within_cap(ref):
    return ref["ambiguous"].mean() <= CAP


def mismatches(got, ref):
    """The (request, column) pairs where `got` breaks the rule of the module docstring (the cap is asserted first)."""
    assert within_cap(ref), "more than %g of the pairs are ambiguous: %d of %d" % (CAP, ref["ambiguous"].sum(), ref["ambiguous"].size)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref["want"].shape, (got.shape, ref["want"].shape)
    ok = np.where(ref["ambiguous"], _same(got, ref["below"]) | _same(got, ref["above"]), _same(got, ref["want"]))
    return [(int(k), int(c), float(got[k, c]), float(ref["want"][k, c])) for k, c in zip(*np.nonzero(~ok))]


def credible_interval_literal(X, P):
    """utils.py:185-196, restated: sort by value, cumulate the probabilities, the last point whose cumulative probability is
    below 0.025 and the first whose cumulative probability is above 0.975."""
    order = np.argsort(X)
    xs = np.asarray(X)[order]
    cs = np.cumsum(np.asarray(P)[order])
    return xs[np.where(cs < 0.025)[0][-1]], xs[np.where(cs > 0.975)[0][0]]


# ------------------------------------------------------------------------------------------------ inputs
WEIGHTS = ("uniform", "decades", "sparse", "one_row", "unused")
KEYS = ("random", "ties", "constant", "inf", "zeros", "nan_unused", "nan_used")
REQUESTS = {1: ([0.5], [FIRST_ABOVE]),
            3: ([0.025, 0.5, 0.975], [LAST_BELOW, FIRST_ABOVE, FIRST_ABOVE]),
            8: ([0.025, 0.025, 0.16, 0.5, 0.5, 0.84, 0.975, 0.975],
                [LAST_BELOW, FIRST_ABOVE, LAST_BELOW, LAST_BELOW, FIRST_ABOVE, FIRST_ABOVE, LAST_BELOW, FIRST_ABOVE])}


def shape_list(block, stage):
    """The column lengths at which the kernels can go wrong: one and two rows, a wave and its neighbours, a workgroup's
    stride and its neighbours, a third round of the stride, and both sides of the staged / streamed threshold."""
    return [1, 2, 63, 64, 65, block - 1, block, block + 1, 2 * block + 1, stage - 1, stage, stage + 1]


def weights_family(kind, n, seed):
    """Random weights -- never equal ones, whose cumulative sums hit q n exactly.  Every family has at least one used row."""
    rng = np.random.default_rng([seed, n, WEIGHTS.index(kind)])
    if kind == "uniform":
        W = rng.random(n) + 1e-3
    elif kind == "decades":                                           # log-uniform over 20 decades: a few rows carry the sum
        W = 10.0 ** rng.uniform(-20, 0, n)
    elif kind == "sparse":                                            # 90 % exactly zero
        W = rng.random(n) + 1e-3
        W[rng.random(n) < 0.9] = 0.0
    elif kind == "one_row":
        W = np.zeros(n)
    else:                                                             # non-finite and negative weights: unused rows
        W = rng.random(n) + 1e-3
        bad = rng.random(n) < 0.3
        W[bad] = rng.choice([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0], int(bad.sum()))
    if not used_rows(W).any():
        W[rng.integers(n)] = 0.75
    return W


def keys_family(kind, ncols, n, ldy, W, seed):
    """(Y (ncols, ldy), W): the padding ldy - n holds NaN -- nothing may read it.  Two families adjust the weights: nan_unused
    makes up to three rows unused and puts NaN there, nan_used puts a NaN into a used row of the first and the last column."""
    rng = np.random.default_rng([seed, ncols, n, KEYS.index(kind)])
    W = np.array(W, dtype=np.float64)
    Y = np.full((ncols, ldy), np.nan)
    v = rng.normal(size=(ncols, n))
    if kind == "ties":
        v = rng.integers(0, 7, (ncols, n)).astype(np.float64)
    elif kind == "constant":
        v = np.repeat(np.arange(ncols, dtype=np.float64)[:, None] - 0.5, n, axis=1)
    elif kind == "inf":
        v[rng.random((ncols, n)) < 0.1] = np.inf
        v[rng.random((ncols, n)) < 0.1] = -np.inf
    elif kind == "zeros":
        v = rng.choice([-0.0, 0.0, -1.0, 1.0], (ncols, n))
    elif kind == "nan_unused" and n > 1:
        rows = rng.choice(n, min(3, n - 1), replace=False)
        W[rows] = [0.0, np.nan, -1.0][:len(rows)]
        if not used_rows(W).any():
            W[np.setdiff1d(np.arange(n), rows)[0]] = 0.5
        v[:, rows] = np.nan
    elif kind == "nan_used":
        row = np.flatnonzero(used_rows(W))[-1]
        v[0, row] = v[-1, row] = np.nan
    Y[:, :n] = v
    return Y, W


@functools.lru_cache(maxsize=None)
def case(n, ncols, pad, K, wkind, kkind, seed=0):
    """One input with its reference, computed once per session and shared: (Y, W, q, rule, ref).  Treat as read-only."""
    W = weights_family(wkind, n, seed)
    Y, W = keys_family(kkind, ncols, n, n + pad, W, seed)
    q, rule = REQUESTS[K]
    for a in (Y, W):
        a.setflags(write=False)
    return Y, W, q, rule, reference(Y, W, q, rule)


def shape_cases(n):
    """The cases the shape test runs at column length n: every ncols x padding, the request sets and the weight families taken
    in turn (random keys: the shapes are what varies)."""
    out = []
    for a, ncols in enumerate((1, 3, 257)):
        for b, pad in enumerate((0, 3)):
            i = 2 * a + b + n
            out.append((n, ncols, pad, (1, 3, 8)[i % 3], WEIGHTS[i % len(WEIGHTS)], "random"))
    return out


def family_cases(block):
    """Every weight family x every key family at three rounds of the workgroup's stride plus one row, K = TRPL_Q_MAX."""
    return [(2 * block + 1, 3, 3, 8, wk, kk) for wk in WEIGHTS for kk in KEYS]
