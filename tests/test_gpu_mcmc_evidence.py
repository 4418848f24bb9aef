"""The sums of the log-evidence estimates on the device (trpl_mcmc_evidence_sums*, csrc/mcmc_evidence.hip) against
tests/mcmc_evidence_ref.py, and the estimates of a tempered run against their analytic targets.

ext, the sum of LL and the count are BIT FOR BIT the restatement (a NaN matches a NaN); the four exponential sums are held to the
long-double form at mcmc_evidence_ref.sums_rtol: 1e-13, the gate tests/test_gpu_posterior_instances.py holds the device's tempered
weights to, + one rounding per addition on a path -- derived, not tuned.  The shapes are where the kernel can go wrong: one rung and
the most the kernel argument holds, a block of fewer values than threads, exactly as many, one more, several rounds with a ragged
last one, one block and several.  Every row of LL outside [t0, t1) is NaN, so a read outside poisons a rung; everything around ext
and sums is a sentinel that must stay.

The statistics: mcmc_evidence_ref's Gaussian toy, whose gates are 5 deviations of the numpy restatement of run_tempered over 8
seeds about the analytic targets (GA_RESTATEMENT, written down there; nothing is taken from the code under test)."""
import numpy as np
import pytest

import mcmc_evidence_ref as er
from test_gpu_mcmc import _cuda, _same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _dev_form(torch_dev, LL, tf, t0, t1, B):
    """(ext, sums) of the _dev form, written into the middle of sentinel buffers that are checked."""
    torch, dev = torch_dev
    K = LL.shape[0]
    ext = torch.full((K + 2, 2), SENTINEL, dtype=torch.float64, device="cuda")
    sums = torch.full((K + 2, B, er.NSUMS), SENTINEL, dtype=torch.float64, device="cuda")
    dev.mcmc_evidence_sums_device(_cuda(torch, LL), tf, t0, t1, ext[1:1 + K], sums[1:1 + K])
    torch.cuda.synchronize()
    ext, sums = ext.cpu().numpy(), sums.cpu().numpy()
    assert np.all(ext[0] == SENTINEL) and np.all(ext[-1] == SENTINEL) and np.all(sums[0] == SENTINEL) and np.all(sums[-1] == SENTINEL)
    return ext[1:1 + K], sums[1:1 + K]


def _against_the_restatement(got_ext, got, LL, tf, t0, t1, B, rtol):
    want_ext, want = er.sums(LL, tf, t0, t1, B)
    long = er.sums_long(LL, tf, t0, t1, B)
    assert _same_bits(got_ext, want_ext)
    assert _same_bits(got[:, :, 0], want[:, :, 0]) and _same_bits(got[:, :, 5], want[:, :, 5])
    worst = 0.0
    for slot in (1, 2, 3, 4):
        g, l = got[:, :, slot], long[:, :, slot]
        exact = ~np.isfinite(l) | (l == 0.0)                     # NaN, +inf and the sums that do not exist: the same value
        assert np.all((g[exact] == l[exact]) | (np.isnan(g[exact]) & np.isnan(l[exact]))), slot
        if (~exact).any():
            err = float(np.max(np.abs(g[~exact] - l[~exact]) / l[~exact]))
            worst = max(worst, err)
            assert err <= rtol, (slot, err, rtol)
    return worst


@pytest.mark.parametrize("C", er.CS)
@pytest.mark.parametrize("K", er.KS)
def test_sums_against_the_restatement(gpu, torch_dev, K, C):
    tf, w = er.case_ladder(K), er.case_w(C)
    rtol = er.sums_rtol(w, C)
    for B in er.BS:
        LL = er.case_LL(K, C, B)
        t0, t1 = er.T0, er.T0 + B * w
        assert np.isnan(LL[:, :t0]).all() and np.isnan(LL[:, t1:]).all() and LL.shape[1] > t1
        info = {}
        ext, sums = gpu.mcmc.evidence_sums(LL, tf, t0, t1, B, info=info)
        assert ext.shape == (K, 2) and sums.shape == (K, B, er.NSUMS) and info["seconds"] > 0.0
        assert np.isfinite(ext).all() and np.isfinite(sums).all()                       # the NaN rows did not show
        worst = _against_the_restatement(ext, sums, LL, tf, t0, t1, B, rtol)
        print("K=%d C=%d B=%d w=%d: worst relative error of an exponential sum %.2e (gate %.2e)" % (K, C, B, w, worst, rtol))
        assert np.all(sums[0, :, 1:3] == 0.0) and np.all(sums[-1, :, 3:5] == 0.0) and np.all(sums[:, :, 5] == w * C)
        dext, dsums = _dev_form(torch_dev, LL, tf, t0, t1, B)
        assert _same_bits(dext, ext) and _same_bits(dsums, sums)                        # the two forms, bit for bit
        again = gpu.mcmc.evidence_sums(LL, tf, t0, t1, B)
        assert _same_bits(again[0], ext) and _same_bits(again[1], sums)                 # and two calls


def test_equal_temperatures_give_the_count(gpu, torch_dev):
    """delta = 0 between rungs 0 and 1 and between 2 and 3: down of 0 and 2, up of 1 and 3 are the count exactly, -inf excluded."""
    K, C, B = 4, 257, 2
    tf = np.array([1.5, 1.5, 4.0, 4.0])
    LL = er.case_LL(K, C, B, seed=1)
    t0, t1 = er.T0, er.T0 + B * er.case_w(C)
    LL[1, t0, 5] = LL[2, t0 + 1, 7] = -np.inf
    ext, sums = gpu.mcmc.evidence_sums(LL, tf, t0, t1, B)
    _against_the_restatement(ext, sums, LL, tf, t0, t1, B, er.sums_rtol(er.case_w(C), C))
    n = er.case_w(C) * C
    count = np.full((K, B), float(n))
    count[1, 0] = count[2, 0] = n - 1
    assert np.array_equal(sums[:, :, 5], count)
    for k, slot in ((0, 3), (1, 1), (2, 3), (3, 1)):
        assert np.array_equal(sums[k, :, slot], count[k]) and np.array_equal(sums[k, :, slot + 1], count[k]), (k, slot)
    r = gpu.mcmc.log_evidence_ratios(ext, sums, tf)
    assert r["forward"][0] == r["reverse"][0] == r["forward"][2] == r["reverse"][2] == 0.0


def test_an_unsorted_ladder_minus_infinity_and_a_nan(gpu, torch_dev):
    """A ladder that rises and falls takes both centring branches; -inf follows the header's rule in both directions; one NaN makes
    its own rung NaN, every block of it, and no other."""
    K, C, B = 5, 1000, 2
    tf = np.array([2.0, 1.0, 3.0, 1.5, 6.0])
    w = er.case_w(C)
    LL = er.case_LL(K, C, B, seed=2)
    t0, t1 = er.T0, er.T0 + B * w
    rtol = er.sums_rtol(w, C)
    ext, sums = gpu.mcmc.evidence_sums(LL, tf, t0, t1, B)
    _against_the_restatement(ext, sums, LL, tf, t0, t1, B, rtol)
    d = er.deltas(tf)
    assert (d < 0).any() and (d > 0).any() and np.isfinite(sums).all()
    assert np.all(sums[:, :, 1] <= w * C) and np.all(sums[:, :, 3] <= w * C)            # no exponent is positive on either branch
    LL[1, t0 + 1, 3] = LL[2, t0, 999] = LL[2, t1 - 1, 0] = -np.inf
    LL[3, t0 + w, 17] = np.nan                                   # in block 1 only
    ext, sums = gpu.mcmc.evidence_sums(LL, tf, t0, t1, B)
    _against_the_restatement(ext, sums, LL, tf, t0, t1, B, rtol)
    assert np.isnan(ext[3]).all() and np.isnan(sums[3]).all()
    assert np.isfinite(ext[[0, 4]]).all() and np.isfinite(sums[[0, 4]]).all()
    assert ext[1, 1] == ext[2, 1] == -np.inf and np.isfinite(ext[[1, 2], 0]).all()
    assert sums[1, 0, 0] == -np.inf and np.isfinite(sums[1, 1, 0]) and np.all(sums[2, :, 0] == -np.inf)
    # rung 1: up has delta_0 = 1/2 - 1 < 0 -> +inf in the block of the -inf, down has -delta_1 = -(1 - 1/3) < 0 -> +inf
    assert sums[1, 0, 1] == sums[1, 0, 3] == np.inf and np.isfinite(sums[1, 1, 1:5]).all()
    # rung 2: up has delta_1 > 0 and down -delta_2 = -(1/3 - 1/1.5) > 0 -> the -inf gives +0.0 to both
    assert np.isfinite(sums[2, :, 1:5]).all() and np.all(sums[2, :, 5] == w * C - 1)
    dext, dsums = _dev_form(torch_dev, LL, tf, t0, t1, B)
    assert _same_bits(dext, ext) and _same_bits(dsums, sums)


@pytest.fixture(scope="module")
def gauss_run(gpu):
    """The Gaussian toy on the device, once: (Tempered, ladder, the base's LL)."""
    seed = er.GA_DEVICE_SEED
    U0, LL0 = er.gauss_start(seed)
    lo, hi, lg = er.GA_BOX
    ladder = gpu.mcmc.geometric_ladder(1.0, er.GA_HOT, er.GA_K)
    t = gpu.mcmc.run_tempered(er.gauss_loglik, U0, LL0, lo, hi, lg, ladder, sweeps=er.GA_SWEEPS, seed=seed, U0=U0)
    return t, ladder, er.gauss_base(seed)


def test_the_gaussian_toy_against_its_analytic_evidence(gpu, gauss_run):
    """forward and reverse against ln Z(1) - ln Z(8), ti against the trapezoid of the analytic E[LL] on the same ladder, and with the
    uniform base of 4096 draws at the hottest rung the absolute ln Z(1)."""
    t, ladder, base_LL = gauss_run
    gates = er.gauss_gates()
    r = t.log_evidence(burn=er.GA_BURN, blocks=er.GA_BLOCKS, base=(base_LL, er.GA_HOT))
    rec = er.GA_RESTATEMENT[er.GA_SEEDS.index(er.GA_DEVICE_SEED)]
    assert (r["dropped"], r["t0"], r["t1"], r["blocks"]) == (0, er.GA_BURN, er.GA_SWEEPS, er.GA_BLOCKS)
    print("base ln Z(%g) = %.6f +- %.4f (ess %.1f; analytic %.6f, restatement %.6f)"
          % (er.GA_HOT, r["base_ln_z"], r["base_se"], r["base_ess"], er.gauss_ln_z(er.GA_HOT), rec[3]))
    print("smallest term_ess %.4f" % r["term_ess"].min())
    for i, name in enumerate(("forward", "reverse", "ti")):
        target, margin = gates[name]
        print("%-7s total %.6f +- %.4f (target %.6f, gate %.4f, restatement %.6f)   ln Z(1) %.6f +- %.4f (target %.6f, gate %.4f)"
              % (name, r[name + "_total"], r[name + "_total_se"], target, margin, rec[i], r["ln_z"][name], r["ln_z_se"][name],
                 gates["ln_z_" + name][0], gates["ln_z_" + name][1]))
    for name in ("forward", "reverse", "ti"):
        target, margin = gates[name]
        assert abs(r[name + "_total"] - target) < margin, name
        assert 0.0 < r[name + "_total_se"] < margin                                     # a jackknife error of the size of the scatter
        target, margin = gates["ln_z_" + name]
        assert abs(r["ln_z"][name] - target) < margin, name
        assert r["ln_z"][name] == r["base_ln_z"] + r[name + "_total"]
    assert r["term_ess"].shape == (er.GA_K - 1, 2) and np.all(r["term_ess"] > 0.5) and np.all(r["term_ess"] <= 1.0)
    assert np.array_equal(r["N"], np.full(er.GA_K, (er.GA_SWEEPS - er.GA_BURN) * er.GA_C))
    with pytest.raises(ValueError, match="tf_hot_check"):
        t.log_evidence(burn=er.GA_BURN, base=(base_LL, 1.0))


def test_posterior_log_evidence_is_the_long_double_mean(gpu, gauss_run):
    """ln of the mean of exp(LL / tf - log_ratio) over the samples with no NaN at rtol 1e-12, at 7 temperatures from one scan, with
    and without a log-ratio; a NaN sample is left out of the mean and of its count and makes the two error figures NaN."""
    _, ladder, clean = gauss_run
    holed = clean.copy()
    holed[5] = np.nan
    lnr = 0.3 * np.random.default_rng(9).normal(size=clean.size)
    for LL in (clean, holed):
        keep = ~np.isnan(LL)
        for log_ratio in (None, lnr):
            ln_z, info = gpu.posterior.log_evidence(LL, ladder, log_ratio=log_ratio)
            assert ln_z.shape == info["ess"].shape == info["se"].shape == ladder.shape
            for k, tf in enumerate(ladder):
                e = LL[keep].astype(np.longdouble) / tf - (0.0 if log_ratio is None else lnr[keep].astype(np.longdouble))
                w = np.exp(e - e.max())
                want = float(np.log(np.mean(w)) + e.max())
                ess = float(np.sum(w) ** 2 / np.sum(w * w))
                assert abs(ln_z[k] - want) <= 1e-12 * abs(want), (k, ln_z[k], want)
                assert info["count"][k] == keep.sum()
                if keep.all():
                    assert abs(info["ess"][k] - ess) <= 1e-9 * ess
                    assert abs(info["se"][k] - np.sqrt(1.0 / ess - 1.0 / keep.sum())) <= 1e-9
                else:
                    assert np.isnan(info["ess"][k]) and np.isnan(info["se"][k])
            one, info1 = gpu.posterior.log_evidence(LL, float(ladder[-1]), log_ratio=log_ratio)
            assert isinstance(one, float) and one == ln_z[-1] and (info1["ess"] == info["ess"][-1] or not keep.all())


def test_a_ladder_of_one_has_no_ratio_and_makes_no_call(gpu, monkeypatch):
    U0, LL0 = er.gauss_start(3)
    lo, hi, lg = er.GA_BOX
    t = gpu.mcmc.run_tempered(er.gauss_loglik, U0, LL0, lo, hi, lg, [2.0], sweeps=12, seed=3, U0=U0)

    def no_call(*a, **k):
        raise AssertionError("evidence_sums was called for a ladder of one")

    monkeypatch.setattr(gpu.mcmc, "evidence_sums", no_call)
    r = t.log_evidence(blocks=5)
    assert (r["dropped"], r["t0"], r["t1"]) == (2, 2, 12)
    for name in ("forward", "reverse", "ti"):
        assert r[name + "_total"] == 0.0 and r[name].shape == (0,)
