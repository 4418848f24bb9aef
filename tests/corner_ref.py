"""Host restatement of the corner (trpl_corner*, include/trpl.h; TEST INFRASTRUCTURE ONLY): the plotted columns in
np.longdouble, the exclusion, the histograms by oracle.posterior.bin_index with numpy.add.at in ascending sample order, and the
densities by the arithmetic of the reference's marginalize_1D / marginalize_2D.  tests/golden/corner_ref.npz pins it to the
reference's own functions (tools/gen_corner_golden.py); tests/highprec.hist (exact sums) is the accuracy check."""
import numpy as np

from oracle.posterior import bin_index, edges as bin_edges, normalize

LD = np.longdouble
NAMES = ("n0", "p0", "mun", "mup", "B", "Sf", "Sb", "CN", "CP", "taun", "taup", "lambda", "mag_offset",
         "tau_eff", "tau_rad", "Sf+Sb", "mu'", "epsilon", "taun+taup")            # position = TRPL_COL_* code
PRIMARY = 13

# the survey's parameter box in the user's units (parallel_bayes_gpu.py:86-92) with the columns it fixes opened up a little, so
# that every column of the corner varies
BOX_LO = np.array([1e8, 1e14, 1.0, 1.0, 1e-11, 0.1, 0.1, 1e-30, 1e-30, 1.0, 1.0, 0.05, -0.5])
BOX_HI = np.array([1e9, 1e16, 50.0, 50.0, 1e-9, 100.0, 100.0, 1e-28, 1e-28, 1000.0, 2000.0, 0.2, 0.5])
BOX_LOG = np.array([1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0])


def draw(seed, S):
    """S samples of the box from the legacy RandomState(seed), column by column (bayeslib.random_grid's order), then the
    log-likelihoods LL = -6 U(0, 1) from the same stream.  A flat surface on purpose: numpy.histogram, which the reference's
    marginalize_1D calls with explicit edges, forms a weighted bin as a DIFFERENCE of cumulative sums of the sorted weights, an
    absolute error near S 2^-53 of the total mass in every bin (measured here: 2.5e-15 of the total), so a comparison to rtol
    1e-10 means something only where every occupied bin holds more than ~1e-4 of the mass -- a single sample's weight here."""
    rng = np.random.RandomState(seed)
    cols = []
    for lo, hi, lg in zip(BOX_LO, BOX_HI, BOX_LOG):
        cols.append(10 ** rng.uniform(np.log10(lo), np.log10(hi), S) if lg else rng.uniform(lo, hi, S))
    X = np.ascontiguousarray(np.stack(cols, axis=1))
    LL = -6.0 * rng.uniform(0.0, 1.0, S)
    return X, LL


def pairs(D):
    """utils.py:103-106: for i, py / for j, px / if i > j: (px, py) -- as (x column, y column) index pairs."""
    out = []
    for i in range(D):
        for j in range(D):
            if i > j:
                out.append((j, i))
    return out


def secondary(X, code, thickness, dtype=LD):
    """secondary_parameters.py:9-57 in `dtype`, LI_tau_eff as DEFINED (CP = X[:, 8]; the call of utils.py:61-62 leaves it out)."""
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    one, th = dtype(1), dtype(thickness)
    n0, p0, mun, mup, B, Sf, Sb, CN, CP, taun, taup, lam, m = X.T
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = dtype(2) / (one / mun + one / mup)
        t_r = one / (B * p0) * dtype(1e9)
        if code == 13:
            t_aug = one / (CP * (p0 * p0)) * dtype(1e9)
            Dif = mu * dtype(0.0257) / one * dtype(1e14) / dtype(1e9)
            pi2 = dtype(np.pi) * dtype(np.pi)
            tau_surf = (th / ((Sf + Sb) * dtype(0.01))) + (th * th / (pi2 * Dif))
            return one / (one / t_r + one / t_aug + one / tau_surf + one / taun)
        return {14: t_r, 15: Sf + Sb, 16: mu, 17: one / lam, 18: taun + taup}[code]


def column(X, code, thickness=2000.0, log=False, dtype=LD):
    """The plotted values of one column code, in `dtype` (a primary column is X's own)."""
    v = np.asarray(X, dtype=np.float64)[:, code].astype(dtype) if code < PRIMARY else secondary(X, code, thickness, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log10(v) if log else v


def columns(X, codes, thickness=2000.0, dolog=None, dtype=LD):
    dolog = [0] * len(codes) if dolog is None else dolog
    return np.stack([column(X, c, thickness, bool(g), dtype) for c, g in zip(codes, dolog)])


def keep_mask(X, excl_lo, excl_hi):
    """utils.py:145-155 on the raw values; a NaN limit means the column is not tested, a NaN value fails its test."""
    X = np.asarray(X, dtype=np.float64)
    keep = np.ones(len(X), dtype=bool)
    if excl_lo is None:
        return keep
    for c in range(PRIMARY):
        if excl_lo[c] == excl_lo[c]:
            with np.errstate(invalid="ignore"):
                keep &= np.logical_and(X[:, c] <= excl_hi[c], X[:, c] >= excl_lo[c])
    return keep


def llk(X, LL, excl_lo, excl_hi):
    """(LLk, kept) of trpl_corner_columns_dev."""
    out = np.where(keep_mask(X, excl_lo, excl_hi), np.asarray(LL, dtype=np.float64), np.nan)
    return out, int(np.count_nonzero(~np.isnan(out)))


def keys(V, lo, hi, bins):
    """The bin of every value of every column (-1: dropped), oracle.posterior.bin_index against the reference's edges."""
    V = np.asarray(V, dtype=np.float64)
    return np.stack([bin_index(V[d].copy(), bin_edges(lo[d], hi[d], bins)) for d in range(V.shape[0])])


def hist(V, W, lo, hi, bins, want_pairs=True):
    """(h1 [D][bins], c1 [D][bins], h2 [pairs][bins][bins] or None) as trpl_corner_hist_dev defines them: a sample enters the
    weighted sums iff its weight is finite and > 0 and the counts iff its weight is not NaN; every weighted bin is summed one
    sample at a time in ascending sample index from +0.0, which is what numpy.add.at does."""
    V = np.asarray(V, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    D = V.shape[0]
    k = keys(V, lo, hi, bins)
    with np.errstate(invalid="ignore"):
        used = (W > 0) & (W < np.inf)
    counted = ~np.isnan(W)
    h1, c1 = np.zeros((D, bins)), np.zeros((D, bins))
    for d in range(D):
        ok = used & (k[d] >= 0)
        np.add.at(h1[d], k[d][ok], W[ok])
        ok = counted & (k[d] >= 0)
        c1[d] = np.bincount(k[d][ok], minlength=bins)
    h2 = None
    if want_pairs and D > 1:
        pp = pairs(D)
        h2 = np.zeros((len(pp), bins * bins))
        for p, (j, i) in enumerate(pp):
            ok = used & (k[j] >= 0) & (k[i] >= 0)
            np.add.at(h2[p], k[j][ok] * bins + k[i][ok], W[ok])
        h2 = h2.reshape(len(pp), bins, bins)
    return h1, c1, h2


def density_1d(raw, cnt, e, correct):
    """marginalize_1D, utils.py:246-262, from the raw sums and counts."""
    marP = raw / (np.diff(e) * raw.sum())
    if correct:
        corr = np.zeros_like(marP)
        nz = cnt != 0
        corr[nz] = marP[nz] / cnt[nz]
        marP = corr / np.sum(np.diff(e) * corr)
    return marP


def density_2d(raw, ex, ey):
    """marginalize_2D, utils.py:278."""
    return raw / (np.outer(np.diff(ex), np.diff(ey)) * raw.sum())


def corner(X, LL, names, limits, bins, tf, thickness, dolog, exclude):
    """plot() of marginalization_visual.py:500-609 up to the drawing, restated: returns dict(kept, W, V, h1d {name: density},
    h2d {(px, py): density}).  limits: name -> (lo, hi) in plotted units; the exclusion is on the raw values of the enabled
    primary columns (10 ** limit for a log-scaled one, plotutils.py:19-23 before :56-59)."""
    codes = [NAMES.index(n) for n in names]
    lg = [n in dolog for n in names]
    lo = np.array([limits[n][0] for n in names], dtype=np.float64)
    hi = np.array([limits[n][1] for n in names], dtype=np.float64)
    elo = ehi = None
    if exclude:
        elo, ehi = np.full(PRIMARY, np.nan), np.full(PRIMARY, np.nan)
        for d, c in enumerate(codes):
            if c < PRIMARY:
                elo[c], ehi[c] = (10.0 ** lo[d], 10.0 ** hi[d]) if lg[d] else (lo[d], hi[d])
    LLk, kept = llk(X, LL, elo, ehi)
    ok = ~np.isnan(LLk)
    W = np.full(len(LLk), np.nan)
    W[ok] = normalize(LLk[ok] / tf)                              # the reference drops the samples, then normalises
    V = columns(X, codes, thickness, lg).astype(np.float64)
    h1, c1, h2 = hist(V, W, lo, hi, bins)
    e = [bin_edges(lo[d], hi[d], bins) for d in range(len(names))]
    h1d = {n: density_1d(h1[d], c1[d], e[d], codes[d] >= PRIMARY or "mu" in n) for d, n in enumerate(names)}
    h2d = {(names[j], names[i]): density_2d(h2[p], e[j], e[i]) for p, (j, i) in enumerate(pairs(len(names)))}
    return dict(kept=kept, W=W, V=V, h1d=h1d, h2d=h2d, LLk=LLk, raw=(h1, c1, h2), lo=lo, hi=hi, elo=elo, ehi=ehi)


def ulp_margin(v, points):
    """The smallest distance, in ulp of the point, from any finite value of v to any of `points`."""
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    best = np.inf
    for p in np.asarray(points, dtype=np.float64):
        if v.size:
            best = min(best, float(np.min(np.abs(v - p)) / np.spacing(abs(p) if p != 0 else 1.0)))
    return best


def emulate_hist_kernel(kx, ky, W, bins, waves=4):
    """hist_kernel of csrc/corner.hip restated lane by lane (slow: test sizes only).  kx, ky: the key bytes of the x and the y
    column (255 = dropped; ky None for a 1-D histogram).  Tiles of 64 samples in order; wave w owns the x bins
    [w * xpw, (w + 1) * xpw); the lanes of a wave that add to the same bin are ranked by lane with a match over the bits of the
    wave-local key, and round r adds the lanes of rank r.  Returns the bins, [x bin][y bin] flattened."""
    S = len(W)
    pair = ky is not None
    ybins = bins if pair else 1
    out = np.zeros(bins * ybins)
    xpw = (bins + waves - 1) // waves
    nbits = 0
    while (1 << nbits) < xpw * ybins:
        nbits += 1
    for t in range((S + 63) // 64):
        for wave in range(waves):
            x0 = wave * xpw
            lanes = []
            for lane in range(64):
                s = t * 64 + lane
                a, b, w = (int(kx[s]), int(ky[s]) if pair else 0, W[s]) if s < S else (255, 255 if pair else 0, np.nan)
                add = a != 255 and b != 255 and x0 <= a < x0 + xpw and w > 0 and w < np.inf
                lanes.append((add, (a - x0) * ybins + b if add else 0, a * ybins + b, w))
            pend = [ln[0] for ln in lanes]
            if not any(pend):
                continue                                         # the ballot that skips a tile
            rank = []
            for lane, (add, key, _, _) in enumerate(lanes):
                m = list(pend)
                for bit in range(nbits):                         # one ballot per bit of the key
                    has = [(ln[1] >> bit) & 1 == 1 for ln in lanes]
                    mine = (key >> bit) & 1
                    m = [mm and (h if mine else not h) for mm, h in zip(m, has)]
                rank.append(sum(m[:lane]) if add else -1)
            r = 0
            while True:
                for lane, (_, _, at, w) in enumerate(lanes):
                    if rank[lane] == r:
                        out[at] = out[at] + w
                if not any(x > r for x in rank):
                    break
                r += 1
    return out
