"""What driver.loglik(cut_levels=) hands to trpl_loglik_cut_levels, argument by argument -- no GPU: the recording stand-in of
tests/test_loglik_marshal_host.py takes the place of the loaded library.  The positions are written out from the prototype of
include/trpl.h, not computed by the code under test."""
import ctypes

import numpy as np
import pytest

import test_loglik_marshal_host as m

S, C = m.S, m.C
LAYOUT = dict(m._HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_hi=12, obs_dx=13, obs_h=14, obs_ld=15, n_obs=16, cut_level=17, P=18,
              sse=19, cut_col=20, status=21, iters_total=22, floor_col=23, flags=24, device=25, seconds=26)
KEYS = m.PLAIN_KEYS | {"cut_col", "cut_fraction"}


@pytest.fixture
def recorder(monkeypatch, trpl):
    monkeypatch.setitem(m.LAYOUT, "trpl_loglik_cut_levels", LAYOUT)
    monkeypatch.setitem(m.PEEK, "cut_level", (np.float64, C * S))
    rec = m.Recorder()
    monkeypatch.setattr(trpl._abi, "lib", lambda: rec)
    return rec


def _levels(shape):
    lv = np.random.default_rng(3).uniform(0.0, 50.0, shape)
    lv.flat[1] = np.inf
    lv.flat[2] = 0.0
    return lv


@pytest.mark.parametrize("off_grid", [False, True], ids=["grid", "times"])
@pytest.mark.parametrize("shape", [(S,), (C, S)], ids=["per_sample", "per_system"])
def test_cut_levels_hands_the_library_every_argument_at_its_position(trpl, recorder, shape, off_grid):
    A, drv = trpl._abi, trpl.driver
    X, ini, lengths, obs, sim_t, times, _ = m._problem()
    lv = _levels(shape)
    info = {}
    ret = drv.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, tol=m.TOL, MAX=m.MAX_ITER, normalize=True, kernel="single", info=info,
                     times=times if off_grid else None, device=m.DEVICE, cut_levels=lv)
    assert [c[0] for c in recorder.calls] == ["trpl_loglik_cut_levels"]
    name, args, mem = recorder.calls[0]
    assert len(args) == len(A.SIGNATURES[name]) == len(LAYOUT) and sorted(LAYOUT.values()) == list(range(len(args)))
    assert set(info) == KEYS
    want = dict(S=S, C=C, Time=m.TIME, L=m.L, T=m.T, plT=1, tol=m.TOL, MAX=m.MAX_ITER, obs_ld=m.OBS_LD, flags=m.FLAGS, device=m.DEVICE)
    for k, v in want.items():
        assert args[LAYOUT[k]] == v, (k, args[LAYOUT[k]])
    assert isinstance(args[LAYOUT["seconds"]], type(ctypes.byref(ctypes.c_double()))) and info["seconds"] == 0.0
    assert [args[LAYOUT[k]] is None for k in ("obs_hi", "obs_dx", "obs_h")] == [not off_grid] * 3
    # the levels: (S,) is given to each curve, (C, S) goes as it is; a pointer, never a float
    assert isinstance(args[LAYOUT["cut_level"]], int) and not isinstance(args[LAYOUT["cut_level"]], bool)
    assert np.array_equal(mem["cut_level"].reshape(C, S), np.broadcast_to(lv, (C, S)))
    # the outputs are the arrays info / the return value hand back
    assert args[LAYOUT["P"]] == m._addr(ret) and ret.shape == (S,) and not ret.any()
    for k in ("sse", "cut_col", "status", "iters_total", "floor_col"):
        assert args[LAYOUT[k]] == m._addr(info[k]) and info[k].shape == (C, S), k
    assert info["cut_col"].dtype == np.int32 and (info["cut_col"] == -1).all() and info["cut_fraction"] == 0.0
    # the inputs behind the pointers
    assert np.array_equal(mem["X"], X.ravel()) and np.array_equal(mem["dN"], ini.ravel())
    assert np.array_equal(mem["lengths"], lengths) and np.array_equal(mem["n_obs"], m.N_OBS)
    order = [np.argsort(t, kind="stable") for t in times] if off_grid else [np.arange(n) for n in m.N_OBS]
    assert np.array_equal(mem["obs"], m._padded([o[i] for o, i in zip(obs, order)], 0.0))
    if off_grid:
        br = [drv.bracket_times(sim_t, t[i]) for t, i in zip(times, order)]
        assert np.array_equal(mem["obs_hi"], m._padded([b[0] for b in br], 1, np.int32))
        assert np.array_equal(mem["obs_dx"], m._padded([b[1] for b in br], 0.0))
        assert np.array_equal(mem["obs_h"], m._padded([b[2] for b in br], 1.0))


def test_python_refusals(trpl, recorder):
    drv = trpl.driver
    X, ini, lengths, obs, _, _, weights = m._problem()

    def call(**kw):
        return drv.loglik(X, ini, lengths, m.TIME, m.L, m.T, obs, **kw)
    lv = _levels((S,))
    with pytest.raises(ValueError, match="exclude each other"):
        call(cut_levels=lv, sse_cut=1.0)
    # refused with what sse_cut is refused with
    for word, kw in (("mag_grid", dict(mag_grid=[0.0])), ("mag_profile", dict(mag_profile=True)), ("weights", dict(weights=weights)),
                     ("devices", dict(devices=[0])), ("bundle", dict(bundle=2))):
        for cut in (dict(cut_levels=lv), dict(sse_cut=1.0)):
            with pytest.raises(ValueError, match="not available with %s" % word):
                call(**cut, **kw)
    for shape in ((S + 1,), (C, S + 1), (C + 1, S), (1, C, S), ()):
        with pytest.raises(ValueError, match="shape"):
            call(cut_levels=np.ones(shape))
    for bad in (np.nan, -1.0, -np.inf):
        arr = _levels((C, S))
        arr[1, 2] = bad
        with pytest.raises(ValueError, match=">= 0"):
            call(cut_levels=arr)
    assert not recorder.calls                                    # nothing reached the library
    call(cut_levels=np.full(S, np.inf))
    assert [c[0] for c in recorder.calls] == ["trpl_loglik_cut_levels"]


def test_run_refuses_nothing_new_and_passes_levels_per_solved_row(trpl):
    """mcmc.run(early_reject=True) needs a device for its proposals: here only its signature and its default."""
    import inspect
    sig = inspect.signature(trpl.mcmc.run)
    assert sig.parameters["early_reject"].default is False and list(sig.parameters)[-1] == "early_reject"
    assert inspect.signature(trpl.driver.loglik).parameters["cut_levels"].default is None
