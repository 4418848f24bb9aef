"""Plain numpy restatement of the refinement generations (trpl_refine_*, include/trpl.h; trpl_amd.refine): Philox4x32-10, the
box-kernel draw, the mixture density as the sequential loop over the parents, systematic resampling on np.longdouble cumulative
sums, the deterministic-mixture weights, and the driver of the scheme.  No device, no library: the tests compare against this."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011): counter (..., 4) and key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def res53(x, y):
    """genrand_res53: two 32-bit words -> a double in [0, 1)."""
    return ((x >> np.uint32(5)).astype(np.float64) * 67108864.0 + (y >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0


def uniforms(total, A, seed, generation):
    """xi (total, A): child n, call j -> dimensions 2j, 2j + 1; key (seed low, seed high), counter (n low, n high, j, generation)."""
    n = np.arange(total, dtype=np.uint64)
    xi = np.empty((total, A))
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    for j in range((A + 1) // 2):
        ctr = np.stack([(n & MASK).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32), np.full(total, j, dtype=np.uint32),
                        np.full(total, generation, dtype=np.uint32)], axis=-1)
        r = philox4x32_10(ctr, key)
        xi[:, 2 * j] = res53(r[:, 0], r[:, 1])
        if 2 * j + 1 < A:
            xi[:, 2 * j + 1] = res53(r[:, 2], r[:, 3])
    return xi


def active_columns(minX, maxX, flags=0):
    """Columns with minX != maxX that are not the target of a set override (bit 0: column 2, bit 1: 6, bit 2: 8)."""
    minX, maxX = np.asarray(minX, dtype=np.float64), np.asarray(maxX, dtype=np.float64)
    target = {c for bit, c in ((1, 2), (2, 6), (4, 8)) if flags & bit and (c != 2 or minX.size > 3)}
    return np.array([c for c in range(minX.size) if minX[c] != maxX[c] and c not in target], dtype=np.int64)


def unit_coords(X, minX, maxX, do_log, flags=0):
    act = active_columns(minX, maxX, flags)
    U = np.empty((X.shape[0], act.size))
    for d, c in enumerate(act):
        if do_log[c]:
            l, lh = np.log10(minX[c]), np.log10(maxX[c])
            U[:, d] = (np.log10(X[:, c]) - l) / (lh - l)
        else:
            U[:, d] = (X[:, c] - minX[c]) / (maxX[c] - minX[c])
    return U, act


def from_unit(U, minX, maxX, do_log, flags=0):
    """X (S, ncol) by the sampler's expressions: linear, 10 ** (l + (lh - l) u), fixed columns copied, overrides last."""
    minX, maxX = np.asarray(minX, dtype=np.float64), np.asarray(maxX, dtype=np.float64)
    act = active_columns(minX, maxX, flags)
    ncol = minX.size
    X = np.full((U.shape[0], ncol), np.nan)
    for c in range(ncol):
        if minX[c] == maxX[c]:
            X[:, c] = minX[c]
    for d, c in enumerate(act):
        if do_log[c]:
            l, lh = np.log10(minX[c]), np.log10(maxX[c])
            X[:, c] = np.power(10.0, l + (lh - l) * U[:, d])
        else:
            X[:, c] = minX[c] + (maxX[c] - minX[c]) * U[:, d]
    if flags & 1 and ncol > 3:
        X[:, 2] = X[:, 3]
    if flags & 2 and ncol > 6:
        X[:, 6] = X[:, 5]
    if flags & 4 and ncol > 8:
        X[:, 8] = X[:, 7]
    return X


def boxes(c, h):
    """a, b (K, A) and inv_vol (K,): [max(0, c - h), min(1, c + h)], the product in ascending d and one division."""
    c = np.asarray(c, dtype=np.float64)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (c.shape[1],))
    a, b = np.maximum(0.0, c - h), np.minimum(1.0, c + h)
    vol = np.ones(c.shape[0])
    for d in range(c.shape[1]):
        vol = vol * (b[:, d] - a[:, d])
    return a, b, 1.0 / vol


def draw_unit(a, b, m, n_uniform, seed, generation):
    """U2 (n_uniform + K m, A): u = min(b, a + (b - a) xi); child n_uniform + j belongs to parent j mod K."""
    K, A = a.shape
    total = n_uniform + K * m
    xi = uniforms(total, A, seed, generation)
    par = (np.arange(total) - n_uniform) % K
    lo = np.where((np.arange(total) < n_uniform)[:, None], 0.0, a[par])
    hi = np.where((np.arange(total) < n_uniform)[:, None], 1.0, b[par])
    return np.minimum(hi, lo + (hi - lo) * xi)


def density(U, a, b, inv_vol):
    """B[s] = sum over k in ascending order of inv_vol[k] for the closed boxes that hold U[s]: the sequential loop."""
    U = np.asarray(U, dtype=np.float64)
    B = np.zeros(U.shape[0])
    for k in range(a.shape[0]):
        inside = np.all((U >= a[k]) & (U <= b[k]), axis=1)
        B[inside] = B[inside] + inv_vol[k]
    return B


def used_weights(W):
    W = np.asarray(W, dtype=np.float64)
    return np.where(W > 0, W, 0.0)                               # NaN and <= 0 count as 0


def resample(W, K, offset=0.5):
    """Systematic resampling on np.longdouble cumulative sums.  Returns idx (K,), margin (K,): the distance of each threshold to
    the nearest cumulative value, relative to the total, and stats = (sw, sum w^2, sw^2 / sum w^2)."""
    w = used_weights(W).astype(np.longdouble)
    cum = np.cumsum(w)
    sw = cum[-1] if w.size else np.longdouble(0)
    if not sw > 0:
        return np.full(K, -1, dtype=np.int64), np.full(K, np.inf), (0.0, 0.0, 0.0)
    t = (np.arange(K).astype(np.longdouble) + np.longdouble(offset)) / np.longdouble(K) * sw
    idx = np.searchsorted(cum, t, side="right").astype(np.int64)
    idx = np.minimum(idx, w.size - 1)
    below = np.where(idx > 0, cum[np.maximum(idx - 1, 0)], np.longdouble(0))
    margin = np.minimum(np.abs(cum[idx] - t), np.where(idx > 0, np.abs(t - below), np.inf)) / sw
    sq = np.sum(w * w)
    return idx, margin.astype(np.float64), (float(sw), float(sq), float(sw * sw / sq))


def log_ratio(U, S1, proposals):
    """ln r(u), r = (S1 + sum_g [n_uniform_g + m_g B_g(u)]) / S_total; proposals: dicts of a, b, inv_vol, m, n_uniform."""
    num = np.full(U.shape[0], float(S1))
    total = float(S1)
    for p in proposals:
        num = num + (float(p["n_uniform"]) + float(p["m"]) * density(U, p["a"], p["b"], p["inv_vol"]))
        total += p["n_uniform"] + p["a"].shape[0] * p["m"]
    return np.log(num / total)


def normalize(LL):
    """Weights that sum to 1 (utils.py:157-166 without its constant lift)."""
    w = np.exp(LL - np.nanmax(LL))
    w = np.where(np.isnan(w), 0.0, w)
    return w / w.sum()


def ess(W):
    w = used_weights(W)
    return float(w.sum() ** 2 / np.sum(w * w))


def bandwidth(U, W, S1):
    """h_d = clip(max(sqrt 3 sd_d ESS^(-1 / (A + 4)), S1^(-1 / A) / 2), 0, 1 / 2)."""
    A = U.shape[1]
    w = used_weights(W)
    w = w / w.sum()
    mean = w @ U
    sd = np.sqrt(w @ (U - mean) ** 2)
    return np.clip(np.maximum(np.sqrt(3.0) * sd * ess(w) ** (-1.0 / (A + 4)), 0.5 * S1 ** (-1.0 / A)), 0.0, 0.5)


def run(loglik_unit, U1, rounds, K, m, n_uniform, tf=1.0, seed=1, h=None, offset=0.5):
    """The scheme on unit coordinates with any loglik_unit(U) -> LL.  Returns dict(U, LL, LLc, ess (per round, cumulative union),
    proposals)."""
    S1 = U1.shape[0]
    U, LL = U1, loglik_unit(U1)
    props, esses = [], []
    LLc = LL - tf * log_ratio(U, S1, props)
    esses.append(ess(normalize(LLc / tf)))
    for g in range(2, 2 + rounds):
        W = normalize(LLc / tf)
        idx, _, _ = resample(W, K, offset)
        hh = bandwidth(U, W, S1) if h is None else h
        a, b, iv = boxes(U[idx], hh)
        props.append(dict(a=a, b=b, inv_vol=iv, m=m, n_uniform=n_uniform, seed=seed, generation=g))
        U2 = draw_unit(a, b, m, n_uniform, seed, g)
        U, LL = np.concatenate([U, U2]), np.concatenate([LL, loglik_unit(U2)])
        LLc = LL - tf * log_ratio(U, S1, props)
        esses.append(ess(normalize(LLc / tf)))
    return dict(U=U, LL=LL, LLc=LLc, ess=esses, proposals=props, S1=S1)


def gaussian_toy(sd=0.08, A=3):
    """The toy of the scheme's tests: an isotropic Gaussian of deviation sd centred in the unit cube.  Returns (loglik_unit,
    evidence): the integral of exp(LL) over the cube, a product of error functions."""
    from math import erf, pi, sqrt

    def loglik_unit(U):
        return -0.5 * np.sum(((U - 0.5) / sd) ** 2, axis=1)

    one = sd * sqrt(2.0 * pi) * erf(0.5 / (sd * sqrt(2.0)))
    return loglik_unit, one ** A


def evidence(res):
    """mean(exp(LL) / r) over the union: exp(LLc) at tf = 1."""
    return float(np.mean(np.exp(res["LLc"])))


# ---- inputs shared by the host and the device tests of the resampling
PATTERNS = ("equal", "first", "last", "sparse", "nan_neg", "decades", "zero")
MARGIN = 1e-12                                                   # a draw whose threshold is this close to a cumulative value is excused
OFFSET = 0.3141592653589793                                      # the tests' offset: 0.5 puts thresholds of equal weights ON cumulative values


def weight_pattern(name, S, seed=0):
    """The weight vectors of the resampling tests: equal weights, one non-zero weight first / last, 99 % exact zeros, NaN and
    negative entries, weights spanning 300 decades, all zero."""
    rng = np.random.default_rng([seed, S, PATTERNS.index(name)])
    if name == "equal":
        return np.full(S, 0.37)
    if name in ("first", "last"):
        w = np.zeros(S)
        w[0 if name == "first" else S - 1] = 2.5
        return w
    if name == "sparse":
        w = np.where(rng.random(S) < 0.01, rng.random(S), 0.0)
        w[rng.integers(S)] = 0.5                                 # never empty
        return w
    if name == "nan_neg":
        w = rng.random(S) + 0.01
        kind = rng.integers(0, 4, S)
        w[kind == 1] = np.nan
        w[kind == 2] *= -1.0
        w[rng.integers(S)] = 0.7                                 # never empty (S = 1: this entry)
        return w
    if name == "decades":
        return 10.0 ** rng.uniform(-300.0, 0.0, S)
    return np.zeros(S)
