"""Which entry points of the library trpl_amd.mcmc calls, and how often (run, run_tempered and the timed front ends).

run and run_tempered share one sweep loop, and each pair of front ends one marshaller.  The bit-identity tests cannot see a loop that
calls the wrong member of a pair: a rung kernel on one rung is its single-temperature kernel bit for bit.  So the library is
replaced here by a proxy that records the name of every entry point asked for and forwards to the real one.  The problem is tiny:
4 chains in a 3-column box with 2 active columns, 3 sweeps, a numpy likelihood that accepts cut_levels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, SWEEPS, SEED = 4, 3, 11
LO, HI, LG = np.array([0.0, 1.5, -1.0]), np.array([1.0, 1.5, 3.0]), np.zeros(3, dtype=np.int32)      # column 1 is fixed: A = 2


class _Recorder:
    """The library with a memory: every attribute asked for is noted by name and taken from the real library."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)

    def mcmc(self):
        return [n for n in self.names if n.startswith("trpl_mcmc_")]


@pytest.fixture
def recorded(gpu, monkeypatch):
    rec = _Recorder(gpu._abi.lib())
    monkeypatch.setattr(gpu._abi, "lib", lambda: rec)
    return rec


def _start(K=None):
    rng = np.random.default_rng(5)
    X0 = LO + (HI - LO) * rng.uniform(0.3, 0.7, ((C, 3) if K is None else (K, C, 3)))
    return X0, _toy(dict(calls=0, levelled=0))(X0.reshape(-1, 3)).reshape(X0.shape[:-1])


def _toy(seen):
    def loglik(X, cut_levels=None):
        seen["calls"] += 1
        seen["levelled"] += cut_levels is not None
        assert cut_levels is None or cut_levels.shape == (len(X),)
        return -np.sum((X - np.array([0.4, 1.5, 1.2])) ** 2, axis=1) / 0.05
    return loglik


@pytest.mark.parametrize("early_reject", (False, True))
@pytest.mark.parametrize("bounds", ("reject", "fold"))
def test_run_calls_the_single_temperature_entry_points(gpu, recorded, bounds, early_reject):
    X0, LL0 = _start()
    seen = dict(calls=0, levelled=0)
    gpu.mcmc.run(_toy(seen), X0, LL0, LO, HI, LG, sweeps=SWEEPS, tf=1.5, kind="de", seed=SEED, bounds=bounds, early_reject=early_reject)
    names = recorded.mcmc()
    assert set(names) <= {"trpl_mcmc_propose", "trpl_mcmc_levels", "trpl_mcmc_accept"}, names
    assert names.count("trpl_mcmc_propose") == names.count("trpl_mcmc_accept") == 2 * SWEEPS
    # one levels call per half-sweep that solves a proposal, i.e. per call of the likelihood; never without early_reject
    assert names.count("trpl_mcmc_levels") == (seen["calls"] if early_reject else 0) == seen["levelled"]
    assert 1 <= seen["calls"] <= 2 * SWEEPS and (bounds != "fold" or seen["calls"] == 2 * SWEEPS)


@pytest.mark.parametrize("swap_every", (1, 2))
def test_run_tempered_calls_the_rung_entry_points_and_the_swap(gpu, recorded, swap_every):
    X0, LL0 = _start(K=2)
    seen = dict(calls=0, levelled=0)
    gpu.mcmc.run_tempered(_toy(seen), X0, LL0, LO, HI, LG, [1.0, 4.0], sweeps=SWEEPS, swap_every=swap_every, kind="de", seed=SEED,
                          bounds="fold", early_reject=True)
    names = recorded.mcmc()
    assert set(names) == {"trpl_mcmc_propose_rungs", "trpl_mcmc_levels_rungs", "trpl_mcmc_accept_rungs", "trpl_mcmc_swap"}, names
    assert names.count("trpl_mcmc_propose_rungs") == names.count("trpl_mcmc_accept_rungs") == 2 * SWEEPS
    assert names.count("trpl_mcmc_levels_rungs") == seen["calls"] == 2 * SWEEPS
    assert names.count("trpl_mcmc_swap") == 2 * (SWEEPS // swap_every)


def test_run_tempered_walks_randomly_through_the_plain_propose(gpu, recorded):
    X0, LL0 = _start(K=2)
    gpu.mcmc.run_tempered(_toy(dict(calls=0, levelled=0)), X0, LL0, LO, HI, LG, [1.0, 4.0], sweeps=SWEEPS, kind="rw", scale=0.05, seed=SEED)
    names = recorded.mcmc()
    assert set(names) == {"trpl_mcmc_propose", "trpl_mcmc_accept_rungs", "trpl_mcmc_swap"}, names
    assert names.count("trpl_mcmc_propose") == 2 * SWEEPS


def test_a_ladder_of_one_is_never_swapped(gpu, recorded):
    X0, LL0 = _start()
    gpu.mcmc.run_tempered(_toy(dict(calls=0, levelled=0)), X0, LL0, LO, HI, LG, [1.5], sweeps=SWEEPS, seed=SEED)
    names = recorded.mcmc()
    assert set(names) == {"trpl_mcmc_propose_rungs", "trpl_mcmc_accept_rungs"}, names


def test_every_timed_front_end_reports_its_seconds(gpu, recorded):
    m = gpu.mcmc
    rng = np.random.default_rng(6)
    U = rng.uniform(0.3, 0.7, (C, 2))
    infos = {name: {} for name in ("propose", "propose_rungs", "reject_levels", "reject_levels_rungs", "accept", "accept_rungs", "swap",
                                   "chain_stats", "autocov", "autocov_pool")}
    Up, Xp, inside = m.propose(U, U[::-1].copy(), 0.5, 1e-3, 0, SEED, 0, LO, HI, LG, info=infos["propose"])
    m.propose_rungs(U, U[::-1].copy(), 2, 0.5, 1e-3, 0, SEED, 0, LO, HI, LG, info=infos["propose_rungs"])
    LL, LLp = -rng.uniform(0.0, 1.0, C), -rng.uniform(0.0, 1.0, C)
    m.reject_levels(LL, 1.5, 0, SEED, 0, info=infos["reject_levels"])
    m.reject_levels_rungs(LL, [1.0, 4.0], 0, SEED, 0, info=infos["reject_levels_rungs"])
    X = Xp.copy()
    m.accept(U, X, LL, Up, Xp, LLp, inside, 1.5, 0, SEED, 0, info=infos["accept"])
    m.accept_rungs(U, X, LL, Up, Xp, LLp, inside, [1.0, 4.0], 0, SEED, 0, info=infos["accept_rungs"])
    m.swap(U, X, LL, [1.0, 4.0], 0, 0, SEED, 0, info=infos["swap"])
    H = rng.uniform(0.0, 1.0, (8, C * 2))
    m.chain_stats(H, info=infos["chain_stats"])
    _, s = m.autocov(H, 3, info=infos["autocov"])
    m.autocov_pool(s, C, 2, info=infos["autocov_pool"])
    for name, info in infos.items():
        assert set(info) == {"seconds"} and np.isfinite(info["seconds"]) and info["seconds"] >= 0.0, (name, info)
    assert recorded.mcmc() == ["trpl_mcmc_" + n for n in ("propose", "propose_rungs", "levels", "levels_rungs", "accept", "accept_rungs",
                                                         "swap", "chain_stats", "autocov", "autocov_pool")]
