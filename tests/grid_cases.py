"""The cases of tests/test_gpu_stepper_grids.py and their CPU reference: one small window at every grid size the one-system
stepper is compiled for, two films, observations on and off the grid, a weight vector, and everything the GPU tests compare
with -- built from the CPU oracle alone (oracle.pvsim / fastlog / prob / simulate_loglik) and, for esum and the weighted sums,
from the oracle's log10 PL in numpy.longdouble.  tests/test_grid_cases_host.py proves on the CPU the conditions the GPU tests
rely on (everything converges, nothing near the cancellation floor, forced_max finds a cap, no cut decision on a knife edge).
Plain module: no fixtures, nothing of the product but `workloads`."""
import functools
import math

import numpy as np

SIZES = (4, 8, 16, 32, 64, 128, 256, 512)
LAYOUT_SIZES = (4, 64, 128)        # one size per FAST node layout: W = L < 64 lanes, one row per lane, the LDS history ring
S, T, DT = 5, 150, 0.025           # 151 columns: two full 64-column batches of the FAST sink and a ragged third
TIME = T * DT
FILMS = ("thick", "thin")          # workloads.power_scan(L): three curves at 2000 nm; one 311 nm film
SEED_X, SEED_OBS, SEED_W = 5, 19, 23
NOISE = 0.05
FLOOR = 1e-4                       # TRPL_PL_FLOOR_EXCESS
# Where forced_max has a value.  The 311 nm film spreads the systems' largest step counts widely at every size (10 .. 20 at
# L = 4); on the 2000 nm film at L <= 16 they are consecutive small integers (4, 5, 6 at L = 4) for every sample seed tried
# (1 .. 399), so no cap keeps two counts clear of every system: the forced non-convergence runs on the thin film at every size
# and on the thick film from L = 32 on.  The condition itself is never relaxed.
FORCED_CASES = tuple((L, "thin") for L in SIZES) + tuple((L, "thick") for L in SIZES if L >= 32)


def nthreads():
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, 16))


def _workloads():
    import trpl_amd
    return trpl_amd.workloads, trpl_amd.UNIT_CONVERSIONS


def film(name, L):
    """(init_params (C, L), lengths (C,))"""
    w, _ = _workloads()
    if name == "thick":
        return w.power_scan(L)
    return np.stack([w.beer_lambert(w.POWER_SCAN_A_CM3[1], 311.0, L)]), np.array([311.0])


def samples():
    return _workloads()[0].samples(S, seed=SEED_X)


def bracket(sim_t, times):
    """The bracketing of scipy's linear interpolation (bayeslib.py:189): hi = clip(searchsorted, 1, n - 1), lo = hi - 1."""
    hi = np.clip(np.searchsorted(sim_t, times), 1, len(sim_t) - 1)
    return hi, times - sim_t[hi - 1], sim_t[hi] - sim_t[hi - 1]


def n_on(c):
    return T + 1 - 3 * c           # 151 / 148 / 145: ragged, the last two end inside the third batch


def times_off(C):
    """Sorted uniform times, 140 + 7 c per curve, one exactly at 0 and one exactly at Time."""
    rng = np.random.default_rng(SEED_OBS)
    out = []
    for c in range(C):
        t = np.sort(rng.uniform(0.0, TIME, 140 + 7 * c))
        t[0], t[-1] = 0.0, TIME
        out.append(t)
    return out


def weights(n, c):
    """One exact 0, one power of two, random positive values over three decades."""
    rng = np.random.default_rng(SEED_W + c)
    w = 10.0 ** rng.uniform(-1.5, 1.5, n)
    w[n // 3], w[70 % n] = 0.0, 0.25
    return w


def forced_max(step_iters):
    """An iteration cap MAX for a batch with per-step iteration counts step_iters (systems, steps): at least one system has a
    step needing >= MAX + 2 iterations, at least one never needs more than MAX - 1, and no system's largest step count lies in
    [MAX, MAX + 1] -- so an iteration more or less on a knife-edge convergence test cannot change which systems are flagged."""
    m = np.asarray(step_iters).reshape(-1, np.asarray(step_iters).shape[-1]).max(axis=1)
    for cap in range(int(m.min()) + 1, int(m.max()) - 1):
        if (m >= cap + 2).any() and (m <= cap - 1).any() and not ((m >= cap) & (m <= cap + 1)).any():
            return cap
    raise ValueError("no iteration cap splits this batch away from a knife edge: largest step counts %s" % sorted(m.tolist()))


def _sums(y, mag, obs, w):
    """Longdouble sums of one curve: e = y + mag - obs per system; returns sse, esum, sum|e|, weighted sse, esum, sum w|e|."""
    e = (y + mag[:, None].astype(np.longdouble)) - obs[None, :].astype(np.longdouble)
    wl = w[None, :].astype(np.longdouble)
    f = lambda a: np.asarray(a.sum(axis=1), dtype=np.longdouble)
    return dict(e=e, sse=f(e * e), esum=f(e), abs=f(np.abs(e)), wsse=f(wl * e * e), wesum=f(wl * e), wabs=f(wl * np.abs(e)))


@functools.lru_cache(maxsize=None)
def solution(L, name, MAX=10000):
    """The oracle's PL of every system of the film: list over curves of oracle.pvsim's dict (with step_iters)."""
    import oracle
    ini, lens = film(name, L)
    X = samples()
    return [oracle.pvsim(X[:, :12], lens[c], TIME, L, T, ini[c], MAX=MAX, want_step_iters=True, nthreads=nthreads())
            for c in range(len(lens))]


@functools.lru_cache(maxsize=None)
def marked(L, name, normalize=False):
    """log10 PL of workloads.MARKED_POINT per curve: what the observations are made from."""
    import oracle
    w, unit = _workloads()
    ini, lens = film(name, L)
    mark = (w.MARKED_POINT * unit)[None, :-1]
    out = []
    for c in range(len(lens)):
        pl = oracle.pvsim(mark, lens[c], TIME, L, T, ini[c])["plI"][0]
        out.append(np.log10(pl / pl[0] if normalize else pl))
    return out


def observations(L, name, offgrid, normalize=False):
    """(times or None, obs): the marked point's log10 PL (interpolated off the grid) plus seeded noise."""
    lgm = marked(L, name, normalize)
    rng = np.random.default_rng(SEED_OBS + 1)
    sim_t = np.linspace(0, TIME, T + 1)
    if not offgrid:
        return None, [lgm[c][:n_on(c)] + NOISE * rng.standard_normal(n_on(c)) for c in range(len(lgm))]
    times = times_off(len(lgm))
    return times, [np.interp(times[c], sim_t, lgm[c]) + NOISE * rng.standard_normal(len(times[c])) for c in range(len(lgm))]


@functools.lru_cache(maxsize=None)
def reference(L, name, offgrid=False, normalize=False, f32=False):
    """Everything the GPU tests compare with, for one size, film and observation set.  P and sse as the reference evaluates
    them: on the grid oracle.fastlog + oracle.prob on the oracle's PL (as conftest.long_window does), off the grid
    oracle.simulate_loglik curve by curve (scipy griddata, bayeslib.py:184-191); normalize and f32 restate bayeslib.py:150-154
    and :137.  esum, the weighted sums and the running sums `run` (system, column: the sum of the first i + 1 squared errors)
    are longdouble sums over the oracle's log10 PL (float64 PL only)."""
    import oracle
    ini, lens = film(name, L)
    C = len(lens)
    X = samples()
    mag = np.ascontiguousarray(X[:, -1])
    sol = solution(L, name)
    times, obs = observations(L, name, offgrid, normalize)
    dtype = np.float32 if f32 else np.float64
    sim_t = np.linspace(0, TIME, T + 1)
    sse = np.zeros((C, S))
    for c in range(C):
        if offgrid:
            sse[c] = -oracle.simulate_loglik(X, ini[c:c + 1], lens[c:c + 1], TIME, L, T, [([times[c]], [obs[c]])], pl_dtype=dtype,
                                             normalize=normalize, nthreads=nthreads())[0]
            continue
        pl = sol[c]["plI"].astype(dtype)
        if f32:
            pl = oracle.pvsim(X[:, :12], lens[c], TIME, L, T, ini[c], dtype=np.float32, nthreads=nthreads())["plI"]
        if normalize:
            pl = (pl.T / pl.T[0]).T.astype(dtype)
        lg = np.ascontiguousarray(pl[:, :len(obs[c])]).copy()
        oracle.fastlog(lg)
        Pc = np.zeros(S)
        oracle.prob(Pc, lg, obs[c], mag)
        sse[c] = -Pc
    P = np.zeros(S)
    for c in range(C):
        P = P + (0.0 - sse[c])
    out = dict(L=L, film=name, ini=ini, lens=lens, X=X, C=C, times=times, obs=obs, n=[len(o) for o in obs], P=P, sse=sse, sol=sol,
               wts=[weights(len(o), c) for c, o in enumerate(obs)])
    if f32:
        return out
    sums, run, max_lg = [], [], 0.0
    for c in range(C):
        pl = sol[c]["plI"].astype(np.longdouble)
        lg = np.log10(pl / pl[:, :1] if normalize else pl)
        if offgrid:
            hi, dx, h = bracket(sim_t, times[c])
            y = ((lg[:, hi] - lg[:, hi - 1]) / h) * dx + lg[:, hi - 1]
        else:
            y = lg[:, :len(obs[c])]
        s = _sums(y, mag, obs[c], out["wts"][c])
        sums.append(s)
        run.append(np.cumsum(s["e"] * s["e"], axis=1))
        max_lg = max(max_lg, float(np.abs(lg).max()), float(np.abs(obs[c]).max()))
    out.update(sums=sums, run=run, max_lg=max_lg, wsum=np.array([math.fsum(w) for w in out["wts"]]))
    return out


def excess_scale(X, length, L):
    """B L n0 p0 in the units of PL (tests/gpu_common.py: excess_scale)."""
    return X[:, 4] * L * X[:, 0] * X[:, 1] * (length / L)


def cut_level(ref):
    """A level between the systems' final sums: the geometric mean of the two adjacent sorted final sse values with the widest
    relative gap among the middle half -- at least a quarter of the systems on either side."""
    v = np.sort(ref["sse"].ravel())
    q = len(v) // 4
    i = q + int(np.argmax(v[q + 1:len(v) - q + 1] / v[q:len(v) - q])) if len(v) - 2 * q > 0 else len(v) // 2
    return float(np.sqrt(v[i] * v[i + 1]))


def cut_plan(ref, level, gate):
    """What the reference's running sums dictate for trpl_loglik_cut at `level` (include/trpl.h: the test runs after every
    64-column batch the sink adds, the final partial one included): per (curve, system) the number of leading observations at
    which the system stops (-1: never), and whether any tested sum lies within `gate` (relative) of the level -- a decision
    the GPU's rounding may take either way."""
    C = ref["C"]
    col = np.full((C, S), -1, dtype=np.int64)
    edge = np.zeros((C, S), dtype=bool)
    for c in range(C):
        n = ref["n"][c]
        for k in sorted(set(list(range(64, n, 64)) + [n])):
            v = np.asarray(ref["run"][c][:, k - 1], dtype=np.float64)
            edge[c] |= (col[c] < 0) & (np.abs(v - level) <= gate * level)
            col[c] = np.where((col[c] < 0) & (v > level), k, col[c])
    return col, edge
