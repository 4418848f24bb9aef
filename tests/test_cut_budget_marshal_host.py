"""What driver.loglik(cut_budget=) hands to trpl_loglik_cut_budget, argument by argument -- no GPU: the recording stand-in of
tests/test_loglik_marshal_host.py takes the place of the loaded library.  The positions are written out from the prototype of
include/trpl.h, not computed by the code under test."""
import ctypes

import numpy as np
import pytest

import test_loglik_marshal_host as m

S, C = m.S, m.C
LAYOUT = dict(m._HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_hi=12, obs_dx=13, obs_h=14, obs_ld=15, n_obs=16, budget=17,
              curves_per_launch=18, cut_level=19, P=20, sse=21, cut_col=22, status=23, iters_total=24, floor_col=25, flags=26, device=27,
              seconds=28)
KEYS = m.PLAIN_KEYS | {"cut_col", "cut_fraction", "cut_level", "cut_samples"}


@pytest.fixture
def recorder(monkeypatch, trpl):
    monkeypatch.setitem(m.LAYOUT, "trpl_loglik_cut_budget", LAYOUT)
    monkeypatch.setitem(m.PEEK, "budget", (np.float64, S))                   # a pointer to S doubles
    monkeypatch.setitem(m.PEEK, "cut_level", (np.float64, C * S))
    rec = m.Recorder()
    monkeypatch.setattr(trpl._abi, "lib", lambda: rec)
    return rec


def _budget():
    b = np.random.default_rng(5).uniform(0.0, 50.0, S)
    b[1] = np.inf
    b[2] = 0.0
    return b


@pytest.mark.parametrize("off_grid", [False, True], ids=["grid", "times"])
@pytest.mark.parametrize("g", [None, 1, 2, 16])
def test_cut_budget_hands_the_library_every_argument_at_its_position(trpl, recorder, g, off_grid):
    A, drv = trpl._abi, trpl.driver
    X, ini, lengths, obs, sim_t, times, _ = m._problem()
    b = _budget()
    info = {}
    kw = {} if g is None else {"curves_per_launch": g}
    ret = drv.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, tol=m.TOL, MAX=m.MAX_ITER, normalize=True, kernel="single", info=info,
                     times=times if off_grid else None, device=m.DEVICE, cut_budget=b, **kw)
    assert [c[0] for c in recorder.calls] == ["trpl_loglik_cut_budget"]
    name, args, mem = recorder.calls[0]
    assert len(args) == len(A.SIGNATURES[name]) == len(LAYOUT) == 29 and sorted(LAYOUT.values()) == list(range(len(args)))
    assert set(info) == KEYS
    want = dict(S=S, C=C, Time=m.TIME, L=m.L, T=m.T, plT=1, tol=m.TOL, MAX=m.MAX_ITER, obs_ld=m.OBS_LD, flags=m.FLAGS, device=m.DEVICE,
                curves_per_launch=1 if g is None else g)
    for k, v in want.items():
        assert args[LAYOUT[k]] == v and not isinstance(args[LAYOUT[k]], bool), (k, args[LAYOUT[k]])
    assert isinstance(args[LAYOUT["seconds"]], type(ctypes.byref(ctypes.c_double()))) and info["seconds"] == 0.0
    assert [args[LAYOUT[k]] is None for k in ("obs_hi", "obs_dx", "obs_h")] == [not off_grid] * 3
    # the budget: a pointer to S doubles, never a float
    assert isinstance(args[LAYOUT["budget"]], int) and not isinstance(args[LAYOUT["budget"]], bool)
    assert np.array_equal(mem["budget"], b)
    # the levels are an output: info["cut_level"] is the array handed to the library, +inf until the library fills it
    assert args[LAYOUT["cut_level"]] == m._addr(info["cut_level"]) and info["cut_level"].shape == (C, S)
    assert info["cut_level"].dtype == np.float64 and info["cut_level"].flags.c_contiguous and np.all(mem["cut_level"] == np.inf)
    # the other outputs are the arrays info / the return value hand back
    assert args[LAYOUT["P"]] == m._addr(ret) and ret.shape == (S,) and not ret.any()
    for k in ("sse", "cut_col", "status", "iters_total", "floor_col"):
        assert args[LAYOUT[k]] == m._addr(info[k]) and info[k].shape == (C, S), k
    assert info["cut_col"].dtype == np.int32 and (info["cut_col"] == -1).all()
    assert info["cut_fraction"] == 0.0 and info["cut_samples"] == 0.0
    ptrs = [args[LAYOUT[k]] for k in ("budget", "cut_level", "P", "sse", "cut_col", "status", "iters_total", "floor_col")]
    assert len(set(ptrs)) == len(ptrs)
    # the inputs behind the pointers
    assert np.array_equal(mem["X"], X.ravel()) and np.array_equal(mem["dN"], ini.ravel())
    assert np.array_equal(mem["lengths"], lengths) and np.array_equal(mem["n_obs"], m.N_OBS)
    order = [np.argsort(t, kind="stable") for t in times] if off_grid else [np.arange(n) for n in m.N_OBS]
    assert np.array_equal(mem["obs"], m._padded([o[i] for o, i in zip(obs, order)], 0.0))
    if off_grid:
        br = [drv.bracket_times(sim_t, t[i]) for t, i in zip(times, order)]
        assert np.array_equal(mem["obs_hi"], m._padded([b_[0] for b_ in br], 1, np.int32))
        assert np.array_equal(mem["obs_dx"], m._padded([b_[1] for b_ in br], 0.0))
        assert np.array_equal(mem["obs_h"], m._padded([b_[2] for b_ in br], 1.0))


def test_cut_samples_counts_samples_with_any_cut_system(trpl, monkeypatch):
    """cut_samples from cut_col: a stand-in that marks systems (0, 1), (1, 1) and (1, 3) as cut."""
    rec = m.Recorder()
    monkeypatch.setitem(m.LAYOUT, "trpl_loglik_cut_budget", LAYOUT)

    class Marking:
        def __getattr__(self, name):
            inner = getattr(rec, name)

            def entry(*args):
                col = np.ctypeslib.as_array(ctypes.cast(args[LAYOUT["cut_col"]], ctypes.POINTER(ctypes.c_int32)), (C, S))
                col[0, 1], col[1, 1], col[1, 3] = 64, 0, 40
                return inner(*args)
            return entry
    monkeypatch.setattr(trpl._abi, "lib", lambda: Marking())
    X, ini, lengths, obs, *_ = m._problem()
    info = {}
    trpl.driver.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, info=info, cut_budget=np.full(S, 9.0))
    assert info["cut_fraction"] == 3.0 / (C * S) and info["cut_samples"] == 2.0 / S


def test_nothing_reaches_the_library_when_the_budget_is_refused(trpl, recorder):
    X, ini, lengths, obs, *_ = m._problem()
    for kw in (dict(cut_budget=np.ones(S + 1)), dict(cut_budget=np.full(S, -1.0)), dict(cut_budget=np.ones(S), curves_per_launch=0),
               dict(cut_budget=np.ones(S), sse_cut=1.0), dict(cut_budget=np.ones(S), cut_levels=np.ones(S))):
        with pytest.raises(ValueError):
            trpl.driver.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, **kw)
    assert not recorder.calls
    trpl.driver.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, cut_budget=np.full(S, np.inf))
    assert [c[0] for c in recorder.calls] == ["trpl_loglik_cut_budget"]
