"""TRPL_MCMC_FOLD (include/trpl.h) as tests/mcmc_fold_ref.py restates it, and its ABI with no device: the fold itself, the
invariance of the uniform distribution under the folded proposal (and that the gate sees a wrong boundary rule), the toy whose mass
lies against two faces of the cube, the seed of the device's end-to-end case, the refusals.  No GPU needed.

Measured with this stream on the face toy (256 chains, 400 sweeps, 200 dropped, de, seeds 0 .. 3):
    bounds="fold":    acceptance 0.445 .. 0.450, worst R-hat 1.047 .. 1.049, outside 0, folded 0.384 .. 0.387
    bounds="reject":  acceptance 0.261 .. 0.269, worst R-hat 1.082 .. 1.092, outside 0.390 .. 0.396
    largest distance from the analytic value in standard errors: fold 2.13, reject 2.61 (the gate is 5)
Chi-square of the uniform toy (20 bins, 5120 pooled coordinates, gate 63.68): fold at most 25.5, the clamp at least 7.0e3."""
import math
import re

import numpy as np
import pytest

import abi_header as H
import mcmc_fold_ref as fr
import mcmc_ref as mr
import test_mcmc_abi as abi_mcmc
import test_refine_abi as abi_refine
import test_refine_oriented_abi as abi_oriented

FOLD = 0x10


# ------------------------------------------------------------------ fold
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fold_keeps_the_bits_inside_the_unit_interval():
    v = np.array([-0.0, 0.0, 1.0, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0), 0.5, 2.0 ** -1074, 1.0 - 2.0 ** -53, 0.1, 0.9])
    v = np.concatenate([v, np.random.default_rng(0).random(1000)])
    assert np.array_equal(_bits(fr.fold(v)), _bits(v))
    assert np.signbit(fr.fold(np.array([-0.0]))[0])              # -0.0 >= 0.0: it stays, sign and all
    # the neighbours outside are folded: just below 0 and just above 1 come back inside
    below, above = np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0)
    got = fr.fold(np.array([below, above]))
    assert got[0] == 0.0 and got[1] == 2.0 - above and 0.0 <= got[1] < 1.0


def test_fold_exact_values():
    v = np.array([-0.25, 1.25, 2.5, -1.5, 3.75, -1e-300])
    want = np.array([0.25, 0.75, 0.5, 0.5, 0.25, 0.0])
    assert np.array_equal(fr.fold(v), want)
    assert np.array_equal(fr.fold(np.array([2.0, -2.0, 3.0, -1.0, 4.25, -3.75])), np.array([0.0, 0.0, 1.0, 1.0, 0.25, 0.25]))
    assert np.all(np.isnan(fr.fold(np.array([np.nan, np.inf, -np.inf]))))


def test_fold_lands_in_the_unit_interval():
    rng = np.random.default_rng(1)
    v = rng.normal(size=1_000_000) * 10.0 ** rng.uniform(-300, 300, 1_000_000)
    assert np.all(np.isfinite(v)) and np.abs(v).max() > 1e299 and np.abs(v).min() < 1e-299
    r = fr.fold(v)
    assert np.all((r >= 0.0) & (r <= 1.0))
    small = np.abs(v) < 50.0                                     # where the reflection can be written in closed form without loss
    k = np.floor(v[small] / 2.0)
    t = v[small] - 2.0 * k                                       # in [0, 2), exact for these magnitudes up to one rounding
    assert np.allclose(r[small], np.where(t > 1.0, 2.0 - t, t), rtol=0, atol=1e-14)


# ------------------------------------------------------------------ invariance of the uniform distribution
C, A = 256, 3
FLAT = dict(sweeps=40, pooled=20, bins=20)


def _chi2_sf_odd(x, k):
    """P(chi-square_k > x) for odd k, in closed form: erfc(sqrt(x / 2)) + exp(-x / 2) sum_{j = 0}^{(k - 3) / 2} (x / 2)^(j + 1/2) /
    Gamma(j + 3/2) (the regularised upper incomplete gamma function at a half-integer, by its recurrence)."""
    h = x / 2.0
    return math.erfc(math.sqrt(h)) + math.exp(-h) * sum(h ** (j + 0.5) / math.gamma(j + 1.5) for j in range((k - 1) // 2))


def _chi2_critical(k, tail):
    lo, hi = float(k), 100.0 * k                                 # the survival function falls from ~ 1/2 at k to 0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf_odd(mid, k) > tail else (lo, mid)
    return hi


# 20 bins with a known expectation: 19 degrees of freedom.  The gate is the value that a chi-square_19 variable exceeds with
# probability 1e-6, from the closed form above by bisection: 63.68 (checked below against the textbook values of the same function:
# 30.14 at tail 0.05, 43.82 at tail 0.001).
CHI2_GATE = _chi2_critical(FLAT["bins"] - 1, 1e-6)


def test_the_chi_square_gate_is_derived():
    assert abs(_chi2_critical(19, 0.05) - 30.144) < 1e-3 and abs(_chi2_critical(19, 0.001) - 43.820) < 1e-3
    assert abs(_chi2_sf_odd(CHI2_GATE, 19) - 1e-6) < 1e-12 and 63.67 < CHI2_GATE < 63.69


_flat = {}


def _flat_run(kind, rule=None):
    key = (kind, rule)
    if key not in _flat:
        lo, hi, lg = mr.CUBE
        U0 = mr.toy_start(C, 11)
        kw = dict(kind="rw", scale=0.7) if kind == "rw" else dict(kind="de", gamma=1.0)
        _flat[key] = fr.run(lambda X: np.zeros(X.shape[0]), U0, np.zeros(C), lo, hi, lg, sweeps=FLAT["sweeps"], seed=11, bounds="fold",
                            rule=rule, **kw)
    return _flat[key]


def _chi2(run):
    S = run["U"][-FLAT["pooled"]:].reshape(-1, A)
    assert np.all((S >= 0.0) & (S <= 1.0))
    n, bins = S.shape[0], FLAT["bins"]
    out = []
    for d in range(A):
        counts = np.bincount(np.minimum((S[:, d] * bins).astype(np.int64), bins - 1), minlength=bins)
        out.append(float(np.sum((counts - n / bins) ** 2) / (n / bins)))
    return np.array(out)


@pytest.mark.parametrize("kind", ("rw", "de"))
def test_a_flat_likelihood_moves_every_chain_in_every_sweep(kind):
    r = _flat_run(kind)
    assert r["accepted"].all() and r["outside"] == 0 and r["folded"] > 0
    print("flat, %s: folded %.3f" % (kind, r["folded"]))


@pytest.mark.parametrize("kind", ("rw", "de"))
def test_the_folded_proposal_leaves_the_uniform_distribution_invariant(kind):
    chi = _chi2(_flat_run(kind))
    print("flat, %s, fold: chi-square per dimension %s, gate %.2f" % (kind, chi, CHI2_GATE))
    assert np.all(chi < CHI2_GATE), chi


def _clamp(v):
    """A wrong boundary rule, for the gate to see: the face instead of the reflection."""
    return np.clip(v, 0.0, 1.0)


@pytest.mark.parametrize("kind", ("rw", "de"))
def test_the_gate_sees_a_clamp(kind):
    r = _flat_run(kind, _clamp)
    assert r["accepted"].all()
    chi = _chi2(r)
    print("flat, %s, clamp: chi-square per dimension %s, gate %.2f" % (kind, chi, CHI2_GATE))
    assert np.all(chi > CHI2_GATE), chi


# ------------------------------------------------------------------ the face toy
SWEEPS, BURN, SEEDS = 400, 200, (0, 1, 2, 3)
_face = {}


def _face_run(bounds, seed):
    key = (bounds, seed)
    if key not in _face:
        ll, mean, var = fr.toy_face()
        lo, hi, lg = mr.CUBE
        U0 = mr.toy_start(C, seed)
        r = fr.run(ll, U0, ll(U0), lo, hi, lg, sweeps=SWEEPS, seed=seed, bounds=bounds)
        K = r["U"][BURN:]                                        # (kept, C, A)
        m1, m2 = K.mean(axis=0), (K * K).mean(axis=0)            # per chain (C, A)
        z = []
        for per_chain, want in ((m1, fr.FACE_MEAN), (m2, fr.FACE_SECOND)):
            se = per_chain.std(axis=0, ddof=1) / np.sqrt(C)      # the gate calibrates itself on the spread of the chains
            z.append((per_chain.mean(axis=0) - want) / se)
        _face[key] = dict(z=np.array(z), accept=float(r["accepted"][BURN:].mean()), rhat=mr.rhat(r["U"], BURN), outside=r["outside"],
                          folded=r["folded"])
    return _face[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("bounds", ("fold", "reject"))
def test_both_boundary_rules_sample_the_face_toy(bounds, seed):
    """Per coordinate, the mean over the chains of the per-chain mean and of the per-chain second moment lie within 5 standard
    errors of the half-Gaussian's (coordinates 0 and 2) and the Gaussian's (coordinate 1) analytic values: both samplers are exact."""
    r = _face_run(bounds, seed)
    print("face toy, %s, seed %d: acceptance %.3f, worst R-hat %.3f, outside %.4f, folded %.4f, distance in standard errors: mean %s, "
          "second moment %s" % (bounds, seed, r["accept"], r["rhat"].max(), r["outside"], r["folded"], r["z"][0], r["z"][1]))
    assert np.all(np.abs(r["z"]) <= 5.0), r["z"]
    if bounds == "fold":
        assert r["outside"] == 0 and r["folded"] > 0
    else:
        assert r["outside"] > 0 and r["folded"] == 0


def test_the_seed_of_the_device_end_to_end_case_excuses_no_decision():
    U0, X0, LL0, ref = fr.e2e_reference()
    print("end to end, fold: smallest margin %.3g, acceptance %.3f, folded %.4f" % (ref["margin"], ref["accepted"].mean(), ref["folded"]))
    assert ref["margin"] > mr.E2E_MARGIN
    assert ref["outside"] == 0 and ref["folded"] > 0.05 and 0.05 < ref["accepted"].mean() < 0.7


# ------------------------------------------------------------------ the ABI, no device
def test_the_header_and_the_binding_agree(trpl):
    defs = H.defines()
    assert defs["TRPL_MCMC_FOLD"] == trpl._abi.MCMC_FOLD == FOLD
    assert defs["TRPL_ABI_VERSION"] == 5
    taken = defs["TRPL_BOX_EQUAL_MU"] | defs["TRPL_BOX_EQUAL_S"] | defs["TRPL_BOX_EQUAL_AUGER"]
    assert taken == 7 and not FOLD & (taken | 0x8)              # apart from the box bits and from the pinned refusal of 0x8


def test_the_flag_goes_as_far_as_the_device_and_other_bits_are_refused(trpl):
    Ab = trpl._abi
    lib = Ab.lib()
    keep, base = abi_mcmc._args()
    for form in ("propose", "propose_dev"):
        assert abi_mcmc._call(lib, form, dict(base, flags=FOLD)) in (Ab.OK, Ab.ERR_NODEVICE, Ab.ERR_HIP), (form, lib.trpl_last_error())
    # all three overrides with the bit: columns 2, 6, 8 are targets, so a nine-column box with three active columns
    lo = np.zeros(9)
    hi = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    lg = np.zeros(9, dtype=np.int32)
    wide = dict(base, ncol=9, lo=lo.ctypes.data, hi=hi.ctypes.data, do_log=lg.ctypes.data, A=3, flags=FOLD | 7)
    for form in ("propose", "propose_dev"):
        assert abi_mcmc._call(lib, form, wide) in (Ab.OK, Ab.ERR_NODEVICE, Ab.ERR_HIP), (form, lib.trpl_last_error())
    for flags in (0x8, 0x18, 0x20):
        for form in ("propose", "propose_dev"):
            assert abi_mcmc._call(lib, form, dict(base, flags=flags)) == Ab.ERR_ARG, (form, flags)
            assert b"flags=0x%x" % flags in lib.trpl_last_error(), (form, flags, lib.trpl_last_error())
    del keep, lo, hi, lg


def test_the_refinement_draws_refuse_the_flag(trpl):
    Ab = trpl._abi
    lib = Ab.lib()
    keep, base = abi_refine._args()
    for form in ("draw", "draw_dev", "unit", "unit_dev"):
        assert abi_refine._call(lib, form, dict(base, flags=FOLD)) == Ab.ERR_ARG, form
        assert b"flags=0x10" in lib.trpl_last_error(), (form, lib.trpl_last_error())
    keep2, base2 = abi_oriented._args()
    for form in ("draw", "draw_dev"):
        assert abi_oriented._call(lib, form, dict(base2, flags=FOLD)) == Ab.ERR_ARG, form
        assert b"flags=0x10" in lib.trpl_last_error(), (form, lib.trpl_last_error())
    del keep, keep2


def test_the_library_holds_the_fold_kernels(trpl):
    have = [int(n) for n in re.findall(r"trpl::mcmc::__device_stub__propose_fold_kernel<(\d+)>", H.demangled())]
    assert sorted(have) == list(range(1, 17)), sorted(have)


def test_run_refuses_an_unknown_bounds_before_the_likelihood(trpl):
    lo, hi, lg = np.zeros(3), np.ones(3), np.zeros(3, dtype=np.int32)

    def never(X):
        raise AssertionError("the likelihood was called")

    for bad in ("wrap", "", "Fold", None):
        with pytest.raises(ValueError, match="bounds"):
            trpl.mcmc.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=2, bounds=bad)
