"""trpl_nuisance_reduce without a device (the host form is plain host code): against its NumPy restatement bit for bit with the
maximum in all three mag modes, against the three existing calls it is defined by (trpl_irf_bank_profile, trpl_mag_grid_w,
trpl_mag_profile_w), the special cells, the marginal inside the header's bound of an extended-precision value, every refusal in
the header's order, and the ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import abi_header as H
import nuisance_ref as N
from conftest import ROOT
from irf_ref import same_bits

INF, NAN = np.inf, np.nan
MODES = [N.FIXED, N.GRID, N.PROFILE]


def _offsets(mode, M):
    return N.OFFSETS[:M].copy() if mode == N.GRID else None


# ------------------------------------------------------------------------------------------------ the maximum, bit for bit
@pytest.mark.parametrize("mode,M", [(N.FIXED, 1), (N.PROFILE, 1), (N.GRID, 1), (N.GRID, 5)])     # M = 1 without a grid
@pytest.mark.parametrize("J", [1, 3, 9])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("S", [1, 5])
def test_the_maximum_is_the_restatement_bit_for_bit(trpl, S, Cn, J, M, mode):
    sse, esum, wsum = N.moments(Cn, J, S, seed=100 * S + 10 * Cn + J)
    off = _offsets(mode, M)
    v, dm = N.cells(sse, esum, wsum, mode, off)
    want = N.greatest(v, dm)
    P, best, mag = N.host(trpl, sse, esum, wsum, mode, off)
    assert same_bits(P, want[0]) and np.array_equal(best, want[1]) and same_bits(mag, want[2])
    assert same_bits(N.host(trpl, sse, esum, wsum, mode, off, outputs=False)[0], P)           # best and best_mag are optional
    if mode == N.FIXED:
        assert same_bits(N.host(trpl, sse, None, wsum, mode)[0], P)               # FIXED does without esum
        assert same_bits(mag[best >= 0], np.zeros(int((best >= 0).sum())))        # and its offset is +0.0
    if S > 1:
        assert P[1] == -INF and best[1] == -1 and np.isnan(mag[1])                # every cell flagged
    assert (best[0] // M != 0) if J > 1 else (P[0] == -INF and best[0] == -1)     # the flagged cell of sample 0 never wins


def test_special_cells(trpl):
    sse, esum, wsum = N.moments(3, 3, 5, seed=7)
    # an exact tie: the first cell wins, in every mode
    for mode in MODES:
        off = _offsets(mode, 5)
        M = 5 if mode == N.GRID else 1
        s2, e2 = sse.copy(), esum.copy()
        s2[:, 2, 2], e2[:, 2, 2] = s2[:, 0, 2] * 4.0, e2[:, 0, 2]                 # response 2 is worse: the tie of 0 and 1 decides
        P, best, _ = N.host(trpl, s2, e2, wsum, mode, off)
        assert best[2] // M == 0
    # the clamp: sample 3's quadratic is negative at -0.5 in every curve, so the cell is exactly -0.0 ... +0.0 - 0.0 = +0.0
    P, best, mag = N.host(trpl, sse, esum, wsum, N.GRID, N.OFFSETS)
    assert P[3] == 0.0 and not np.signbit(P[3]) and best[3] == 0 and mag[3] == -0.5
    v, _ = N.cells(sse, esum, wsum, N.GRID, N.OFFSETS)
    raw = sum((sse[c, 0, 3] + (2.0 * -0.5) * esum[c, 0, 3]) + wsum[c] * 0.25 for c in range(3))
    assert raw < -1.0 and v[0, 3] == 0.0
    # a NaN sse is never the greatest (FIXED), and is -inf under the grid rule
    assert N.host(trpl, sse, esum, wsum, N.FIXED)[1][4] != 2
    # a curve without weight: it adds its sse and no quadratic term; all curves without weight: nothing to fit
    w0 = wsum.copy()
    w0[1] = 0.0
    for mode in (N.GRID, N.PROFILE):
        off = _offsets(mode, 5)
        got, want = N.host(trpl, sse, esum, w0, mode, off), N.greatest(*N.cells(sse, esum, w0, mode, off))
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    P, best, mag = N.host(trpl, sse, esum, np.zeros(3), N.PROFILE)
    assert P[2] == 0.0 and not np.signbit(P[2]) and best[2] == 0 and np.isnan(mag[2])
    assert P[1] == -INF and best[1] == -1                                          # flagged all the same


# ------------------------------------------------------------------------------------------------ the three anchors
@pytest.mark.parametrize("J", [1, 3, 9])
def test_fixed_is_the_bank_profile_of_the_summed_curves(trpl, J):
    Cn, S = 3, 5
    sse, esum, wsum = N.moments(Cn, J, S, seed=J)
    sse[:, J - 1, 0] = 0.0                                                         # a zero total is +0.0, as P -= sse from zeros leaves it
    Pb = np.zeros((J, S))
    for c in range(Cn):
        Pb -= sse[c]                                                               # irf.loglik_bank's P
    best, P = np.empty(S, dtype=np.int32), np.empty(S)
    trpl._abi.check(trpl._abi.lib().trpl_irf_bank_profile(Pb.ctypes.data, J, S, best.ctypes.data, P.ctypes.data))
    got = N.host(trpl, sse, esum, wsum, N.FIXED)
    assert same_bits(got[0], P) and np.array_equal(got[1], best)
    assert got[0][0] == 0.0 and not np.signbit(got[0][0]) and got[1][0] == J - 1


@pytest.mark.parametrize("fractional", [False, True], ids=["n_obs", "wsum"])
def test_grid_with_one_response_is_mag_grid_w(trpl, fractional):
    Cn, S, M = 3, 5, 5
    sse, esum, wsum = N.moments(Cn, 1, S, seed=11)
    if fractional:
        wsum = wsum * 0.37 + 0.013
    s2, e2 = np.ascontiguousarray(sse[:, 0]), np.ascontiguousarray(esum[:, 0])
    rows = np.zeros((M, S))
    lib = trpl._abi.lib()
    trpl._abi.check(lib.trpl_mag_grid_w(s2.ctypes.data, e2.ctypes.data, wsum.ctypes.data, S, Cn, N.OFFSETS.ctypes.data, M, rows.ctypes.data))
    if not fractional:
        counts, rows_n = wsum.astype(np.int64), np.zeros((M, S))
        trpl._abi.check(lib.trpl_mag_grid(s2.ctypes.data, e2.ctypes.data, counts.ctypes.data, S, Cn, N.OFFSETS.ctypes.data, M, rows_n.ctypes.data))
        assert same_bits(rows_n, rows)
    for m in range(M):                                                             # a grid of one offset returns the cell itself
        P, best, mag = N.host(trpl, sse, esum, wsum, N.GRID, N.OFFSETS[m:m + 1])
        assert same_bits(P, rows[m]) and np.all(mag[best == 0] == N.OFFSETS[m])
    from test_gpu_irf_bank import profile_ref
    best, P = profile_ref(rows)
    got = N.host(trpl, sse, esum, wsum, N.GRID, N.OFFSETS)
    assert same_bits(got[0], P) and np.array_equal(got[1], best)


@pytest.mark.parametrize("fractional", [False, True], ids=["n_obs", "wsum"])
def test_profile_response_by_response_is_mag_profile_w(trpl, fractional):
    Cn, J, S = 3, 3, 5
    sse, esum, wsum = N.moments(Cn, J, S, seed=13)
    if fractional:
        wsum = wsum * 0.37 + 0.013
    lib = trpl._abi.lib()
    Pj, dj = np.zeros((J, S)), np.full((J, S), -7.0)
    for j in range(J):
        s2, e2 = np.ascontiguousarray(sse[:, j]), np.ascontiguousarray(esum[:, j])
        trpl._abi.check(lib.trpl_mag_profile_w(s2.ctypes.data, e2.ctypes.data, wsum.ctypes.data, S, Cn, 0, dj[j].ctypes.data, Pj[j].ctypes.data))
        one = N.host(trpl, np.ascontiguousarray(sse[:, j:j + 1]), np.ascontiguousarray(esum[:, j:j + 1]), wsum, N.PROFILE)
        assert same_bits(one[0], Pj[j])
        assert same_bits(one[2][one[1] == 0], dj[j][one[1] == 0]) and np.all(np.isnan(dj[j][one[1] == -1]))
    from test_gpu_irf_bank import profile_ref
    best, P = profile_ref(Pj)
    got = N.host(trpl, sse, esum, wsum, N.PROFILE)
    assert same_bits(got[0], P) and np.array_equal(got[1], best)
    win = best >= 0
    assert same_bits(got[2][win], dj[best[win], np.flatnonzero(win)]) and np.all(np.isnan(got[2][~win]))


# ------------------------------------------------------------------------------------------------ the marginal
def _prior(J, M, seed):
    """Non-uniform log weights that sum to one, with one excluded cell (where there is more than one)."""
    w = np.random.default_rng(seed).uniform(0.2, 1.0, J * M)
    if J * M > 1:
        w[J * M // 2] = 0.0
    with np.errstate(divide="ignore"):
        return np.log(w / w.sum())


def check_marginal(lib, got, sse, esum, wsum, mode, off, tf, logw):
    """What every marginal is held to: best is the restatement's, P is inside the header's bound of the extended-precision value,
    and lies between the greatest v + tf logw and that + tf ln(J M)."""
    v, dm = N.cells(sse, esum, wsum, mode, off)
    n = len(v)
    want = N.marginal(v, dm, tf, logw)
    assert np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    R, B = N.marginal_exact(v, tf, logw)
    bnd = N.bound(lib, tf, B, n, R)
    assert N.inside(got[0], R, bnd), np.abs(got[0] - R.astype(np.float64)).max()
    assert N.inside(want[0], R, bnd)                                               # the fp64 restatement obeys it too
    with np.errstate(invalid="ignore"):
        top = v.astype(N.LD) + N.LD(tf) * (np.zeros(n) if logw is None else np.asarray(logw)).astype(N.LD)[:, None]
    top = np.where(np.isnan(top), -INF, top).max(axis=0)
    fin = np.isfinite(R)
    assert np.array_equal(fin, np.isfinite(top))
    assert np.all(top[fin] - bnd[fin] <= got[0][fin]) and np.all(got[0][fin] <= top[fin] + tf * math.log(n) + bnd[fin])
    return bnd


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tf", [0.5, 1.0, 10.0])
@pytest.mark.parametrize("J,M", [(1, 1), (3, 5), (9, 5)])
def test_the_marginal_is_inside_the_bound_of_the_extended_value(trpl, J, M, tf, mode):
    if mode != N.GRID:
        M = 1
    Cn, S = 3, 5
    sse, esum, wsum = N.moments(Cn, J, S, seed=J + M)
    off = _offsets(mode, M)
    lib = trpl._abi.lib()
    for logw in (None, _prior(J, M, seed=J)):
        got = N.host(trpl, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=logw)
        bnd = check_marginal(lib, got, sse, esum, wsum, mode, off, tf, logw)
        assert bnd[np.isfinite(got[0])].max() < 1e-11                              # the bound is a sharp one at these sizes
        assert same_bits(N.host(trpl, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=logw, outputs=False)[0], got[0])
        if S > 1:
            assert got[0][1] == -INF and got[1][1] == -1 and np.isnan(got[2][1])
    if J * M > 1:                                                                  # the excluded cell never wins, whatever its value
        logw = _prior(J, M, seed=J)
        assert not np.any(N.host(trpl, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=logw)[1] == J * M // 2)


def test_the_marginal_with_cells_800_apart(trpl):
    # a = v / tf: the cells of a sample lie 800 apart, so every term but the greatest underflows to exactly 0 and P = the greatest v
    J, S, tf = 4, 3, 0.5
    sse = np.empty((1, J, S))
    sse[0] = (400.0 * np.arange(J))[:, None] + np.array([3.0, 7.5, 0.25])
    sse[0, :, 2] = sse[0, ::-1, 2]                                                 # the greatest comes last in sample 2
    esum, wsum = np.zeros((1, J, S)), np.array([10.0])
    got = N.host(trpl, sse, esum, wsum, N.FIXED, marg=True, tf=tf)
    assert same_bits(got[0], np.array([-3.0, -7.5, -0.25])) and got[1].tolist() == [0, 0, 3]
    check_marginal(trpl._abi.lib(), got, sse, esum, wsum, N.FIXED, None, tf, None)
    # with a prior the greatest a is not the greatest v
    logw = np.array([-INF, -5.0, -1.0, -2.0])
    got = N.host(trpl, sse, esum, wsum, N.FIXED, marg=True, tf=tf, logw=logw)
    assert got[1].tolist() == [1, 1, 3]
    check_marginal(trpl._abi.lib(), got, sse, esum, wsum, N.FIXED, None, tf, logw)
    # equal cells: the marginal of n equal cells under the uniform prior is the cell
    sse[:] = 2.0
    uni = np.full(J, -math.log(J))
    got = N.host(trpl, sse, esum, wsum, N.FIXED, marg=True, tf=tf, logw=uni)
    assert np.allclose(got[0], -2.0, rtol=0, atol=1e-14) and not got[1].any()


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = ("trpl_nuisance_max_offsets", "trpl_nuisance_bound", "trpl_nuisance_reduce_dev", "trpl_nuisance_reduce")


def test_header_binding_and_library_agree(trpl):
    text = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the sentences below
    A = trpl._abi
    lib = A.lib()
    for name in NEW:
        assert name in A.SIGNATURES and hasattr(lib, name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    define = H.defines().__getitem__
    assert define("TRPL_NUISANCE_MAX_OFFSETS") == A.NUISANCE_MAX_OFFSETS == lib.trpl_nuisance_max_offsets() == 64
    assert [define("TRPL_NUISANCE_" + n) for n in ("MAG_FIXED", "MAG_GRID", "MAG_PROFILE", "MARGINAL")] \
        == [A.NUISANCE_MAG_FIXED, A.NUISANCE_MAG_GRID, A.NUISANCE_MAG_PROFILE, A.NUISANCE_MARGINAL]
    assert lib.trpl_abi_version() == 5 == define("TRPL_ABI_VERSION")              # additive: the version stays
    # the bound is the header's expression
    u = 2.0 ** -53
    assert lib.trpl_nuisance_bound(2.0, 100.0, 45, -300.0) == u * (2.0 * (3.0 * 100.0 + 2.0 * 45 + 24.0) + 3.0 * 300.0)
    assert "u (tf (3 B + 2 n + 24) + 3 |R|)" in text
    # the three items have left the bank's out-of-scope sentence
    scope = re.findall(r"Out of scope:[^.]*\.", text.replace("\n *", ""))
    assert not any("log-sum-exp" in s or "trpl_mag_grid" in s or "irf_bank" in s for s in scope)


def test_every_refusal_names_its_argument_without_a_device(trpl):
    A = trpl._abi
    lib, E = A.lib(), A.ERR_ARG
    Cn, J, S, M = 2, 3, 4, 5
    sse, esum, wsum = N.moments(Cn, J, S, seed=1, special=False)
    off, logw = N.OFFSETS.copy(), np.zeros(J * M)
    P, best, mag = np.full(S, -7.0), np.full(S, -9, dtype=np.int32), np.full(S, -7.0)
    p = lambda a: a.ctypes.data
    G, F, PR, MG = A.NUISANCE_MAG_GRID, A.NUISANCE_MAG_FIXED, A.NUISANCE_MAG_PROFILE, A.NUISANCE_MARGINAL
    base = dict(sse=p(sse), esum=p(esum), wsum=p(wsum), S=S, C=Cn, J=J, off=p(off), M=M, logw=None, tf=1.0, flags=G, P=p(P), best=p(best),
                mag=p(mag))
    order = ("sse", "esum", "wsum", "S", "C", "J", "off", "M", "logw", "tf", "flags", "P", "best", "mag")
    host = lambda **kw: lib.trpl_nuisance_reduce(*[dict(base, **kw)[k] for k in order])
    dev = lambda **kw: lib.trpl_nuisance_reduce_dev(*[dict(base, **kw)[k] for k in order], None)
    msg = lambda: lib.trpl_last_error()
    fixed = dict(flags=F, off=None, M=1)

    def bad_at(a, i, value):
        b = a.copy()
        b[i] = value
        return b

    keep = [bad_at(wsum, 1, x) for x in (NAN, INF, -1.0)] + [bad_at(off, 2, x) for x in (NAN, INF, -INF)]
    # in the header's order; each case is at fault in its own argument only
    cases = [(dict(S=-1), b"S="), (dict(C=0), b"C="), (dict(C=A.MAG_MAX_CURVES + 1), b"TRPL_MAG_MAX_CURVES"), (dict(J=0), b"J="),
             (dict(J=A.IRF_BANK_MAX_RESPONSES + 1), b"TRPL_IRF_BANK_MAX_RESPONSES"), (dict(flags=3), b"flags"), (dict(flags=G | 0x4), b"flags"),
             (dict(flags=G | 0x100), b"flags"), (dict(M=0), b"M="), (dict(M=A.NUISANCE_MAX_OFFSETS + 1), b"TRPL_NUISANCE_MAX_OFFSETS"),
             (dict(flags=F, off=None, M=2), b"M="), (dict(flags=PR, off=None, M=0), b"M="), (dict(off=None), b"offsets"),
             (dict(flags=F, M=1), b"offsets"), (dict(flags=PR, M=1), b"offsets"), (dict(esum=None), b"esum"),
             (dict(flags=PR, off=None, M=1, esum=None), b"esum")]
    cases += [(dict(wsum=p(w)), b"wsum[1]") for w in keep[:3]] + [(dict(off=p(o)), b"offsets[2]") for o in keep[3:]]
    cases += [(dict(flags=G | MG, tf=x), b"tf=") for x in (0.0, -1.0, NAN, INF)]
    cases += [(dict(logw=p(logw)), b"logw"), (dict(fixed, logw=p(logw)), b"logw"), (dict(sse=None), b"sse is NULL"),
              (dict(wsum=None), b"wsum is NULL"), (dict(P=None), b"P is NULL")]
    for call in (dev, host):
        for kw, word in cases:
            assert call(**kw) == E and word in msg(), (kw, msg())
    for x in (NAN, INF):                                                           # the host form alone reads logw
        lw = bad_at(logw, 7, x)
        assert host(flags=G | MG, logw=p(lw)) == E and b"logw[7]" in msg()
    assert host(flags=G | MG, logw=p(bad_at(logw, 7, -INF))) == 0                 # -inf excludes a cell
    P[:], best[:], mag[:] = -7.0, -9, -7.0
    # the stated order: the first argument at fault is the one named
    chain = [("S", dict(S=-1), b"S="), ("C", dict(C=0), b"C="), ("J", dict(J=0), b"J="), ("flags", dict(flags=3), b"flags")]
    for i, (_, _, word) in enumerate(chain):
        kw = {}
        for _, one, _ in chain[i:]:
            kw.update(one)
        assert dev(M=0, esum=None, tf=NAN, P=None, **kw) == E and word in msg(), msg()
    assert dev(M=0, off=None, esum=None, wsum=p(keep[0]), P=None) == E and b"M=" in msg()
    assert dev(off=None, esum=None, wsum=p(keep[0]), P=None) == E and b"offsets" in msg()
    assert dev(esum=None, wsum=p(keep[0]), off=p(keep[3]), P=None) == E and b"esum" in msg()
    assert dev(wsum=p(keep[0]), off=p(keep[3]), P=None) == E and b"wsum" in msg()
    assert dev(off=p(keep[3]), flags=G | MG, tf=NAN, P=None) == E and b"offsets[2]" in msg()
    assert dev(flags=G | MG, tf=NAN, P=None) == E and b"tf=" in msg()
    assert dev(logw=p(logw), P=None) == E and b"logw" in msg()
    assert dev(sse=None, wsum=None, P=None) == E and b"sse" in msg()
    assert dev(wsum=None, P=None) == E and b"wsum" in msg()
    # no sample: a successful no-op in both forms, NULL pointers included
    for call in (dev, host):
        assert call(S=0) == 0 and call(S=0, sse=None, esum=p(esum), wsum=None, P=None, best=None, mag=None) == 0
        assert call(S=0, flags=F, off=None, M=1, sse=None, esum=None, wsum=None, P=None) == 0
    assert np.all(P == -7.0) and np.all(best == -9) and np.all(mag == -7.0)       # no refused call wrote anything


# ------------------------------------------------------------------------------------------------ the Python layer's own refusals
def test_loglik_nuisance_refuses_before_it_touches_a_device(trpl):
    w = trpl.workloads
    L, T = 32, 64
    ini, lens = w.power_scan(L)
    Time = T * 0.025
    p = dict(X=w.samples(4), init_params=ini[:2], lengths=lens[:2], Time=Time, L=L, T=T)
    bank = trpl.irf.gaussian_bank([0.2], [-0.025, 0.0, 0.025], Time / T)
    ncol_out = T + 1 - bank[1]
    obs = [np.zeros(ncol_out), np.zeros(5)]
    call = trpl.irf.loglik_nuisance
    for kw, word in ((dict(mag="best"), "mag"), (dict(mag=np.zeros(65)), "offsets"), (dict(mag=[0.0, NAN]), "finite"), (dict(mag=[]), "offsets"),
                     (dict(reduce="sum"), "reduce"), (dict(reduce="marginal", tf=0.0), "tf"), (dict(reduce="marginal", tf=NAN), "tf"),
                     (dict(log_prior=np.zeros(3)), "marginal"), (dict(reduce="marginal", log_prior=np.zeros(4)), "log_prior"),
                     (dict(reduce="marginal", log_prior=[0.0, NAN, 0.0]), "log_prior"), (dict(reduce="marginal", log_prior=[0.0, INF, 0.0]), "log_prior"),
                     (dict(reduce="marginal", mag=[0.0, 0.1], log_prior=np.zeros((2, 3))), "log_prior"), (dict(normalize=True), "self-normalisation"),
                     (dict(block=0), "block")):
        with pytest.raises(ValueError, match=word):
            call(obs=obs, bank=bank, **dict(p, **kw))
    with pytest.raises(ValueError, match="at least one observation"):
        call(obs=[np.zeros(5), np.zeros(0)], bank=bank, **p)
    with pytest.raises(ValueError, match="T \\+ 1 - k0"):
        call(obs=[np.zeros(ncol_out + 1), np.zeros(5)], bank=bank, **p)
    info = {}
    out = call(obs=obs, bank=bank, mag=[0.0, 0.1], reduce="marginal", keep_moments=True, info=info, **dict(p, X=np.zeros((0, 13))))
    assert out.shape == (0,) and info["cells"] == (3, 2) and info["best"].dtype == np.int32 and info["best_mag"].shape == (0,)
    assert info["sse"].shape == (3, 2, 0) and info["ncol_out"] == ncol_out
    info = {}
    call(obs=obs, bank=bank, info=info, **dict(p, X=np.zeros((0, 13))))
    assert "sse" not in info and info["cells"] == (3, 1)                          # the moments come down on request only
    assert "ONE tf" in call.__doc__ and "run_tempered" in call.__doc__ and "early_reject" in call.__doc__
