"""Plain numpy restatement of the oriented refinement proposals (trpl_refine_affine, trpl_refine_draw_oriented, include/trpl.h;
trpl_amd.refine with oriented=True): the orientation in numpy.linalg on fp64, the two triangular products as explicit ascending-j
loops (no dot: the device's order of operations), the oriented draw on tests/refine_ref.py's Philox, the density by refine_ref's
sequential loop on the transformed points, and the driver.  No device, no library: the tests compare against this."""
import numpy as np

import refine_ref as rr


def floor_variance(S1, A):
    """(S1^(-1/A) / 2)^2 / 3: the variance of a uniform box of the axis-parallel scheme's floor half-width."""
    return (0.5 * float(S1) ** (-1.0 / A)) ** 2 / 3.0


def orientation(U, W, S1, shrink=None):
    """dict(c, L, M, logdet, h, lam, ess) of the samples U (S, A) under the weights W: weighted mean and covariance, the diagonal
    floor, Sigma_s = (1 - lam) Sigma + lam diag(Sigma) with lam = clip((A + 1) / ESS, 0, 1) unless shrink is given, L = chol(Sigma_s),
    M = L^-1, h_d = sqrt(3) ESS^(-1 / (A + 4))."""
    U = np.asarray(U, dtype=np.float64)
    A = U.shape[1]
    w = rr.used_weights(W)
    w = w / w.sum()
    c = w @ U
    D = U - c
    Sigma = (D * w[:, None]).T @ D
    ess = rr.ess(w)
    return orient(c, Sigma, ess, S1, A, shrink)


def orient(c, Sigma, ess, S1, A, shrink=None):
    """The host part of the orientation, from the mean, the covariance and the effective sample size."""
    Sigma = np.array(Sigma, dtype=np.float64)
    d = np.maximum(np.diag(Sigma), floor_variance(S1, A))
    Sigma[np.arange(A), np.arange(A)] = d
    lam = float(np.clip((A + 1) / ess, 0.0, 1.0)) if shrink is None else float(shrink)
    Sigma_s = (1.0 - lam) * Sigma + lam * np.diag(d)
    L = np.linalg.cholesky(Sigma_s)
    M = np.tril(np.linalg.inv(L))
    h = np.full(A, np.sqrt(3.0) * ess ** (-1.0 / (A + 4)))
    return dict(c=np.array(c, dtype=np.float64), L=L, M=M, logdet=float(np.sum(np.log(np.diag(L)))), h=h, lam=lam, ess=float(ess))


def affine(U, M, c):
    """Z = M (U - c): z_i = sum_{j <= i} M_ij * (u_j - c_j), j ascending from +0.0 -- subtract, multiply, add.  Only j <= i of M
    is read."""
    U = np.asarray(U, dtype=np.float64)
    S, A = U.shape
    D = U - np.asarray(c, dtype=np.float64)
    Z = np.empty((S, A))
    for i in range(A):
        s = np.zeros(S)
        for j in range(i + 1):
            s = s + M[i, j] * D[:, j]
        Z[:, i] = s
    return Z


def from_z(Z, L, c):
    """U = c + L Z: u_i = c_i + sum_{j <= i} L_ij * z_j, j ascending from +0.0."""
    Z = np.asarray(Z, dtype=np.float64)
    S, A = Z.shape
    U = np.empty((S, A))
    for i in range(A):
        s = np.zeros(S)
        for j in range(i + 1):
            s = s + L[i, j] * Z[:, j]
        U[:, i] = c[i] + s
    return U


def boxes(zc, h, logdet):
    """a, b (K, A), inv_vol (K,) of the parents zc in z: [zc - h, zc + h], not clipped; inv_vol = 1 / (prod_d 2 h_d * exp(logdet)),
    the product in ascending d, the same for every parent."""
    zc = np.asarray(zc, dtype=np.float64)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (zc.shape[1],))
    vol = 1.0
    for d in range(zc.shape[1]):
        vol = vol * (2.0 * h[d])
    return zc - h, zc + h, np.full(zc.shape[0], 1.0 / (vol * np.exp(logdet)))


def draw(zc, h, L, c, m, n_uniform, seed, generation):
    """(Z2, U2, inside) of the n_uniform + K m children: box child of parent k = j mod K: z = zc_k + h (2 xi - 1), u = c + L z; a
    uniform child: u = xi and a row of NaN in Z2.  inside (int32): every u_d in [0, 1]."""
    zc = np.asarray(zc, dtype=np.float64)
    K, A = zc.shape
    total = n_uniform + K * m
    xi = rr.uniforms(total, A, seed, generation)
    par = (np.arange(total) - n_uniform) % K
    uni = np.arange(total) < n_uniform
    Z2 = zc[par] + np.asarray(h, dtype=np.float64) * (2.0 * xi - 1.0)
    U2 = from_z(Z2, L, c)
    Z2[uni] = np.nan
    U2[uni] = xi[uni]
    inside = np.all((U2 >= 0.0) & (U2 <= 1.0), axis=1).astype(np.int32)
    return Z2, U2, inside


def density(U, p):
    """B_g(u) of one proposal (a dict of a, b, inv_vol and, when oriented, M and c): refine_ref's sequential loop on the
    transformed points."""
    Zg = affine(U, p["M"], p["c"]) if p.get("M") is not None else U
    return rr.density(Zg, p["a"], p["b"], p["inv_vol"])


def log_ratio(U, S1, proposals):
    """ln r(u), r = (S1 + sum_g [n_uniform_g + m_g B_g(u)]) / S_total, every generation transformed by its own (M, c)."""
    num = np.full(U.shape[0], float(S1))
    total = float(S1)
    for p in proposals:
        num = num + (float(p["n_uniform"]) + float(p["m"]) * density(U, p))
        total += p["n_uniform"] + p["a"].shape[0] * p["m"]
    return np.log(num / total)


def make_proposal(U, W, S1, K, m, n_uniform, seed, generation, offset=0.5, shrink=None):
    idx, _, _ = rr.resample(W, K, offset)
    o = orientation(U, W, S1, shrink)
    zc = affine(U[idx], o["M"], o["c"])
    a, b, iv = boxes(zc, o["h"], o["logdet"])
    return dict(a=a, b=b, inv_vol=iv, m=m, n_uniform=n_uniform, seed=seed, generation=generation, zc=zc, **o)


def run(loglik_unit, U1, rounds, K, m, n_uniform, tf=1.0, seed=1, offset=0.5, shrink=None):
    """The oriented scheme on unit coordinates.  A child outside the cube is not evaluated: LL = -inf, and it counts in S_total.
    Returns dict(U, LL, LLc, inside, ess, proposals, S1, outside (the share per generation), lam)."""
    S1 = U1.shape[0]
    U, LL = U1, loglik_unit(U1)
    inside = np.ones(S1, dtype=np.int32)
    props, esses, outside, lams = [], [], [], []
    LLc = LL - tf * log_ratio(U, S1, props)
    esses.append(rr.ess(rr.normalize(LLc / tf)))
    for g in range(2, 2 + rounds):
        W = rr.normalize(LLc / tf)
        p = make_proposal(U, W, S1, K, m, n_uniform, seed, g, offset, shrink)
        props.append(p)
        _, U2, in2 = draw(p["zc"], p["h"], p["L"], p["c"], m, n_uniform, seed, g)
        LL2 = np.full(U2.shape[0], -np.inf)
        LL2[in2 == 1] = loglik_unit(U2[in2 == 1])
        U, LL, inside = np.concatenate([U, U2]), np.concatenate([LL, LL2]), np.concatenate([inside, in2])
        LLc = LL - tf * log_ratio(U, S1, props)
        esses.append(rr.ess(rr.normalize(LLc / tf)))
        outside.append(float(np.mean(in2 == 0)))
        lams.append(p["lam"])
    return dict(U=U, LL=LL, LLc=LLc, inside=inside, ess=esses, proposals=props, S1=S1, outside=outside, lam=lams)


def correlated_toy(sd, rho, A=3):
    """A Gaussian centred in the unit cube, deviation sd in every dimension, correlation rho between dimensions 0 and 1.  Returns
    (loglik_unit, evidence): the Gaussian's normalisation (2 pi)^(A/2) sd^A sqrt(1 - rho^2) -- the mass outside the cube is below
    1e-12 for sd <= 0.0675 (7.4 deviations to every face)."""
    C = np.eye(A)
    C[0, 1] = C[1, 0] = rho
    P = np.linalg.inv(C * sd * sd)

    def loglik_unit(U):
        D = np.asarray(U, dtype=np.float64) - 0.5
        return -0.5 * np.einsum("si,ij,sj->s", D, P, D)

    return loglik_unit, float((2.0 * np.pi) ** (0.5 * A) * sd ** A * np.sqrt(1.0 - rho * rho))


def evidence(res):
    """mean(exp(LL) / r) over the union, the outside children counted as zeros: exp(LLc) at tf = 1."""
    return float(np.mean(np.exp(res["LLc"])))
