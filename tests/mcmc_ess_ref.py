"""Plain numpy restatement of the autocovariance sums and of the effective sample size (trpl_mcmc_autocov*, include/trpl.h;
trpl_amd.mcmc.autocov / autocov_pool / ess_from_sums / Chains.ess): the sequential loops for mean, s and pooled, the estimator
written out per column, and an AR(1) generator.  No device, no library: the tests compare against this."""
import numpy as np


def autocov(H, t0, t1, L, Q=None):
    """(mean (Q,), s (L, Q)): mean = (sum of H[t], t ascending from +0.0) / m; s[l] = sum over t = t0 .. t1 - 1 - l, ascending, from
    +0.0, of e[t] * e[t + l] with e = H - mean: subtract, multiply, add, one rounding each."""
    H = np.asarray(H, dtype=np.float64)
    Q = H.shape[1] if Q is None else Q
    acc = np.zeros(Q)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(t0, t1):
            acc = acc + H[t, :Q]
        mean = acc / float(t1 - t0)
        e = H[t0:t1, :Q] - mean
        s = np.zeros((L, Q))
        for l in range(L):
            for t in range(t1 - t0 - l):
                s[l] = s[l] + e[t] * e[t + l]
    return mean, s


def pool(s, M, A):
    """pooled (L, A): sum over c = 0 .. M - 1, ascending, from +0.0, of s[:, c A + a]."""
    s = np.asarray(s, dtype=np.float64)
    pooled = np.zeros((s.shape[0], A))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(M):
            pooled = pooled + s[:, c * A:(c + 1) * A]
    return pooled


def geyer(rho, Mm):
    """(tau, K, truncated) of one column's rho (L,): pairs P_k = rho[2k] + rho[2k + 1]; K the first k where P_k > 0 fails, else
    L // 2 (truncated); running minimum; tau = max(-1 + 2 sum_{k < K} P_k, 1 / log10(M m)).  Written with scalars, one pair at a
    time."""
    L = len(rho)
    K, total, low = L // 2, 0.0, np.inf
    truncated = True
    for k in range(L // 2):
        p = rho[2 * k] + rho[2 * k + 1]
        if not p > 0.0:
            K, truncated = k, False
            break
        low = min(low, p)
        total += low
    return max(-1.0 + 2.0 * total, 1.0 / np.log10(Mm)), K, truncated


def rho_from_sums(mean, m2, pooled, m):
    """(rho (L, A), var_plus (A,)) from the sums of M sequences of m steps: mean, m2 (M, A), pooled (L, A)."""
    M = mean.shape[0]
    W = np.mean(m2 / (m - 1), axis=0)
    Bm = np.var(mean, axis=0, ddof=1) if M > 1 else 0.0
    var_plus = (m - 1) / m * W + Bm
    rho = 1.0 - (W - pooled / float(M * m)) / var_plus
    rho[0] = 1.0
    return rho, var_plus


def ess(X, L):
    """(ess (A,), dict) of sequences X (m, M, A) -- M sequences of m steps -- with L lags, everything by the loops above."""
    m, M, A = X.shape
    mean, s = autocov(X.reshape(m, M * A), 0, m, L)
    pooled = pool(s, M, A)
    rho, var_plus = rho_from_sums(mean.reshape(M, A), s[0].reshape(M, A), pooled, m)
    out = [geyer(rho[:, a], M * m) for a in range(A)]
    tau = np.array([o[0] for o in out])
    return M * m / tau, dict(tau=tau, var_plus=var_plus, rho=rho, K=np.array([o[1] for o in out]),
                             truncated=np.array([o[2] for o in out]), mean=mean, m2=s[0], pooled=pooled)


def split_ess(V, burn, L):
    """Chains.ess's arrangement on a history V (n, C, D): the halves [burn, burn + n2), [burn + n2, burn + 2 n2) as 2 C sequences of
    n2 steps, the sums of each half by the loops, the pooled sums added half 0 + half 1."""
    n, C, D = V.shape
    n2 = (n - burn) // 2
    H = np.ascontiguousarray(V, dtype=np.float64).reshape(n, C * D)
    parts = [autocov(H, burn + k * n2, burn + (k + 1) * n2, L) for k in (0, 1)]
    mean = np.concatenate([p[0].reshape(C, D) for p in parts])
    m2 = np.concatenate([p[1][0].reshape(C, D) for p in parts])
    pooled = pool(parts[0][1], C, D) + pool(parts[1][1], C, D)
    rho, var_plus = rho_from_sums(mean, m2, pooled, n2)
    out = [geyer(rho[:, a], 2 * C * n2) for a in range(D)]
    tau = np.array([o[0] for o in out])
    return 2 * C * n2 / tau, dict(tau=tau, var_plus=var_plus, rho=rho, K=np.array([o[1] for o in out]),
                                  truncated=np.array([o[2] for o in out]))


def ar1(phi, m, M, seed, A=1):
    """(m, M, A): stationary AR(1) sequences x[t] = phi x[t - 1] + sqrt(1 - phi^2) eps of unit variance, whose integrated
    autocorrelation time is (1 + phi) / (1 - phi)."""
    rng = np.random.default_rng([seed, int(round(phi * 1000)), m, M])
    eps = rng.normal(size=(m, M, A))
    x = np.empty((m, M, A))
    x[0] = eps[0]
    c = np.sqrt(1.0 - phi * phi)
    for t in range(1, m):
        x[t] = phi * x[t - 1] + c * eps[t]
    return x


# The statistical case of tests/test_mcmc_ess_host.py: 32 sequences x 256 steps, 128 lags, seeds 0 .. 7.  The ratio tau / ((1 + phi) /
# (1 - phi)) of the restatement over the eight seeds, mean and standard deviation (ddof 1), computed once by
# `python tests/mcmc_ess_ref.py`; the package's value is gated at mean +- 5 sd.
AR1_SHAPE = dict(m=256, M=32, L=128, seeds=tuple(range(8)))
AR1_RATIO = {0.0: (0.991726, 0.019584), 0.5: (0.977150, 0.046828)}


def ar1_ratios(phi):
    out = []
    for seed in AR1_SHAPE["seeds"]:
        _, info = ess(ar1(phi, AR1_SHAPE["m"], AR1_SHAPE["M"], seed), AR1_SHAPE["L"])
        out.append((info["tau"][0] / ((1.0 + phi) / (1.0 - phi)), bool(info["truncated"][0])))
    return out


if __name__ == "__main__":
    for phi in (0.0, 0.5, 0.9):
        r = ar1_ratios(phi)
        v = np.array([x[0] for x in r])
        print("phi=%g: ratios %s truncated %s mean %.6f sd %.6f" % (phi, np.round(v, 4), [x[1] for x in r], v.mean(), v.std(ddof=1)))
