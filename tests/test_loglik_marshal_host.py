"""What driver.loglik hands to the library, argument by argument, in every mode -- no GPU: a recording stand-in takes the
place of the loaded library, returns 0 from every entry point and keeps (name, args) and a copy of the host arrays behind the
pointers the test wants to read (they are locals of loglik, gone once it returns).

The expected positions below are written out from the prototypes of include/trpl.h, not computed by the code under test: a
slip of one position in a hand-built argument list reads the wrong buffer, and ctypes does not see it where the types match.
The test passes unchanged on the driver as it was before the call was built in one place: it states behaviour."""
import ctypes
import math

import numpy as np
import pytest

S, C, L, T, TIME = 5, 2, 32, 96, 2.4
N_OBS = (97, 40)
OBS_LD = 97
TOL, MAX_ITER, DEVICE = 6, 5000, 1
FLAGS = 0x20 | 0x4                      # kernel="single" (TRPL_FLAG_KERNEL_SINGLE) | normalize (TRPL_FLAG_NORMALIZE)
OFFSETS = [-0.25, 0.0, 0.5]

_HEAD = dict(X=0, S=1, C=2, lengths=3, Time=4, L=5, T=6)
# 0-based argument positions, from include/trpl.h
LAYOUT = {
    "trpl_loglik": dict(_HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_ld=12, n_obs=13, P=14, sse=15, status=16,
                        iters_total=17, floor_col=18, flags=19, device=20, seconds=21),
    "trpl_loglik_obs": dict(_HEAD, tol=7, MAX=8, dN=9, obs=10, obs_hi=11, obs_dx=12, obs_h=13, obs_ld=14, n_obs=15, P=16,
                            sse=17, status=18, iters_total=19, floor_col=20, flags=21, device=22, seconds=23),
    "trpl_loglik_moments": dict(_HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_hi=12, obs_dx=13, obs_h=14, obs_ld=15, n_obs=16,
                                P=17, sse=18, esum=19, status=20, iters_total=21, floor_col=22, flags=23, device=24, seconds=25),
    "trpl_loglik_weighted": dict(_HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, wts=12, obs_hi=13, obs_dx=14, obs_h=15, obs_ld=16,
                                 n_obs=17, P=18, sse=19, esum=20, status=21, iters_total=22, floor_col=23, flags=24, device=25,
                                 seconds=26),
    "trpl_loglik_cut": dict(_HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_hi=12, obs_dx=13, obs_h=14, obs_ld=15, n_obs=16,
                            sse_cut=17, P=18, sse=19, cut_col=20, status=21, iters_total=22, floor_col=23, flags=24, device=25,
                            seconds=26),
    "trpl_loglik_multi": dict(_HEAD, plT=7, tol=8, MAX=9, dN=10, obs=11, obs_hi=12, obs_dx=13, obs_h=14, obs_ld=15, n_obs=16,
                              P=17, sse=18, status=19, iters_total=20, floor_col=21, flags=22, devices=23, n_devices=24,
                              seconds=25),
    # trpl_mag_grid_w / trpl_mag_profile_w: the same positions, wsum (double) where n_obs (int64) is
    "trpl_mag_grid": dict(sse=0, esum=1, per_curve=2, S=3, C=4, offsets=5, M=6, P=7),
    "trpl_mag_profile": dict(sse=0, esum=1, per_curve=2, S=3, C=4, flags=5, best=6, P=7),
}
LAYOUT["trpl_mag_grid_w"] = LAYOUT["trpl_mag_grid"]
LAYOUT["trpl_mag_profile_w"] = LAYOUT["trpl_mag_profile"]

# host arrays copied at call time: argument name -> (dtype, number of elements)
_MAT = C * OBS_LD
PEEK = dict(X=(np.float64, S * 13), lengths=(np.float64, C), dN=(np.float64, C * L), obs=(np.float64, _MAT),
            wts=(np.float64, _MAT), obs_hi=(np.int32, _MAT), obs_dx=(np.float64, _MAT), obs_h=(np.float64, _MAT),
            n_obs=(np.int64, C), devices=(np.int32, 1), offsets=(np.float64, len(OFFSETS)))

PLAIN_KEYS = {"sse", "status", "iters_total", "floor_col", "seconds"}
MODES = {
    # name: (keywords, on-grid entry, off-grid entry, follow-up call, keys of info)
    "plain": ({}, "trpl_loglik", "trpl_loglik_obs", None, PLAIN_KEYS),
    "mag_grid": (dict(mag_grid=OFFSETS), "trpl_loglik_moments", "trpl_loglik_moments", "trpl_mag_grid", PLAIN_KEYS | {"esum", "P"}),
    "mag_profile": (dict(mag_profile=True), "trpl_loglik_moments", "trpl_loglik_moments", "trpl_mag_profile",
                    PLAIN_KEYS | {"esum", "P"}),
    "mag_profile_per_curve": (dict(mag_profile="per_curve"), "trpl_loglik_moments", "trpl_loglik_moments", "trpl_mag_profile",
                              PLAIN_KEYS | {"esum", "P"}),
    "weights": (dict(weights=True), "trpl_loglik_weighted", "trpl_loglik_weighted", None, PLAIN_KEYS | {"esum", "wsum", "P"}),
    "weights_mag_grid": (dict(weights=True, mag_grid=OFFSETS), "trpl_loglik_weighted", "trpl_loglik_weighted", "trpl_mag_grid_w",
                         PLAIN_KEYS | {"esum", "wsum", "P"}),
    "sse_cut": (dict(sse_cut=12.5), "trpl_loglik_cut", "trpl_loglik_cut", None, PLAIN_KEYS | {"cut_col", "cut_fraction"}),
    "devices": (dict(devices=[0]), "trpl_loglik_multi", "trpl_loglik_multi", None, PLAIN_KEYS),
}


def _read(addr, dtype, count):
    nbytes = count * np.dtype(dtype).itemsize
    return np.frombuffer(ctypes.string_at(addr, nbytes), dtype=dtype).copy()


class Recorder:
    """Stands in for the loaded library: every trpl_* entry point returns 0 and is recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("trpl_"):
            raise AttributeError(name)

        def entry(*args):
            lay = LAYOUT[name]
            width = (np.float64 if name.endswith("_w") else np.int64, C)
            mem = {k: _read(args[lay[k]], *PEEK.get(k, width)) for k in lay
                   if (k in PEEK or k == "per_curve") and args[lay[k]] is not None}
            self.calls.append((name, args, mem))
            return 0
        return entry


def _problem():
    rng = np.random.default_rng(11)
    X = rng.uniform(0.5, 2.0, (S, 13))
    ini = rng.uniform(1.0, 2.0, (C, L))
    lengths = np.array([2000.0, 311.0])
    obs = [rng.normal(size=n) for n in N_OBS]
    sim_t = np.linspace(0, TIME, T + 1)
    times = [rng.uniform(0.0, TIME, n) for n in N_OBS]                  # unsorted, off the grid
    assert all((np.diff(t) < 0).any() and not np.isin(t, sim_t).any() for t in times)
    weights = [rng.uniform(0.1, 3.0, n) for n in N_OBS]
    return X, ini, lengths, obs, sim_t, times, weights


def _padded(rows, fill, dtype=np.float64):
    m = np.full((C, OBS_LD), fill, dtype=dtype)
    for c, r in enumerate(rows):
        m[c, :len(r)] = r
    return m.ravel()


def _addr(a):
    return a.ctypes.data


@pytest.mark.parametrize("off_grid", [False, True], ids=["grid", "times"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_mode_hands_the_library_the_right_argument_at_every_position(trpl, monkeypatch, mode, off_grid):
    A, drv = trpl._abi, trpl.driver
    kw, on_entry, off_entry, follow, keys = MODES[mode]
    kw = dict(kw)
    X, ini, lengths, obs, sim_t, times, weights = _problem()
    if kw.get("weights"):
        kw["weights"] = weights
    rec = Recorder()
    monkeypatch.setattr(A, "lib", lambda: rec)
    info = {}
    dev_kw = {} if mode == "devices" else {"device": DEVICE}
    ret = drv.loglik(X, ini, lengths, TIME, L, T, obs, tol=TOL, MAX=MAX_ITER, normalize=True, kernel="single", info=info,
                     times=times if off_grid else None, **dev_kw, **kw)

    assert [c[0] for c in rec.calls] == [off_entry if off_grid else on_entry] + ([follow] if follow else [])
    for name, args, _ in rec.calls:
        assert len(args) == len(A.SIGNATURES[name]), name
    assert set(info) == keys

    name, args, mem = rec.calls[0]
    lay = LAYOUT[name]
    # every scalar at its position
    want = dict(S=S, C=C, Time=TIME, L=L, T=T, plT=1, tol=TOL, MAX=MAX_ITER, obs_ld=OBS_LD, flags=FLAGS, device=DEVICE,
                sse_cut=12.5, n_devices=1)
    for k, v in want.items():
        if k in lay:
            assert args[lay[k]] == v, (name, k, args[lay[k]])
    assert "plT" in lay or name == "trpl_loglik_obs"
    assert isinstance(args[lay["seconds"]], type(ctypes.byref(ctypes.c_double()))) and info["seconds"] == 0.0
    if name == "trpl_loglik_multi":
        assert np.array_equal(mem["devices"], [0])
    # the brackets: all NULL on the grid, all there off it
    if "obs_hi" in lay:
        assert [args[lay[k]] is None for k in ("obs_hi", "obs_dx", "obs_h")] == [not off_grid] * 3
    else:
        assert name == "trpl_loglik" and not off_grid
    # the outputs are the arrays info / the return value hand back
    P1 = info["P"] if "P" in keys else ret
    assert args[lay["P"]] == _addr(P1) and P1.shape == (S,)
    for k in ("sse", "esum", "cut_col", "status", "iters_total", "floor_col"):
        assert (k in lay) == (k in keys), (name, k)
        if k in lay:
            assert args[lay[k]] == _addr(info[k]) and info[k].shape == (C, S), (name, k)
    assert info["sse"].dtype == np.float64 and info["status"].dtype == np.int32 and info["iters_total"].dtype == np.int64 \
        and info["floor_col"].dtype == np.int32
    if mode == "sse_cut":
        assert info["cut_col"].dtype == np.int32 and (info["cut_col"] == -1).all() and info["cut_fraction"] == 0.0
    # the inputs behind the pointers
    assert np.array_equal(mem["X"], X.ravel()) and np.array_equal(mem["dN"], ini.ravel())
    assert np.array_equal(mem["lengths"], lengths) and np.array_equal(mem["n_obs"], N_OBS)
    order = [np.argsort(t, kind="stable") for t in times] if off_grid else [np.arange(n) for n in N_OBS]
    assert np.array_equal(mem["obs"], _padded([o[i] for o, i in zip(obs, order)], 0.0))
    assert ("wts" in lay) == ("weights" in kw)
    if "wts" in lay:
        assert np.array_equal(mem["wts"], _padded([w[i] for w, i in zip(weights, order)], 0.0))
        wsum = [math.fsum(w) for w in weights]
        assert np.array_equal(info["wsum"], wsum)
    if off_grid:
        br = [drv.bracket_times(sim_t, t[i]) for t, i in zip(times, order)]
        assert np.array_equal(mem["obs_hi"], _padded([b[0] for b in br], 1, np.int32))
        assert np.array_equal(mem["obs_dx"], _padded([b[1] for b in br], 0.0))
        assert np.array_equal(mem["obs_h"], _padded([b[2] for b in br], 1.0))

    if follow is None:
        assert ret is P1
        return
    # the follow-up over the moments: n_obs, or the sum of each curve's weights
    name2, args2, mem2 = rec.calls[1]
    lay2 = LAYOUT[name2]
    assert args2[lay2["sse"]] == _addr(info["sse"]) and args2[lay2["esum"]] == _addr(info["esum"])
    assert args2[lay2["S"]] == S and args2[lay2["C"]] == C
    if name2.endswith("_w"):
        assert np.array_equal(mem2["per_curve"], wsum) and mem2["per_curve"].dtype == np.float64
    else:
        assert np.array_equal(mem2["per_curve"], N_OBS) and mem2["per_curve"].dtype == np.int64
    if "offsets" in lay2:
        assert np.array_equal(mem2["offsets"], OFFSETS) and args2[lay2["M"]] == len(OFFSETS)
        assert ret.shape == (len(OFFSETS), S) and args2[lay2["P"]] == _addr(ret)
    else:
        per_curve = mode == "mag_profile_per_curve"
        best, Pp = ret
        assert args2[lay2["flags"]] == (1 if per_curve else 0)                      # TRPL_MAG_PER_CURVE
        assert best.shape == ((C, S) if per_curve else (S,)) and Pp.shape == (S,)
        assert args2[lay2["best"]] == _addr(best) and args2[lay2["P"]] == _addr(Pp)
    assert args2[lay2["P"]] != args[lay["P"]]
