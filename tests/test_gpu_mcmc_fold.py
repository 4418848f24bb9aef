"""TRPL_MCMC_FOLD on the device (propose_fold_kernel, csrc/mcmc.hip) against tests/mcmc_fold_ref.py.

Propose: Up and the codes of `inside` BIT FOR BIT the restatement (fmod is exact; the add and the subtract of the fold round once
each), the columns of Xp by the rule of tests/test_gpu_mcmc.py (log columns within its 4 ulp, everything else bit for bit); rows
that needed no fold carry the bits of the same call without the flag.  End to end: trpl_amd.mcmc.run(bounds="fold") on the face
toy against the restatement's run: the same decisions on every sweep and the same bits of U."""
import numpy as np
import pytest

import mcmc_fold_ref as fr
import mcmc_ref as mr
import refine_ref as rr
from test_gpu_mcmc import _check_columns, _propose_dev, _same_bits, _states
from test_gpu_refine import TOY_HI, TOY_LG, TOY_LO, _box_for

pytestmark = pytest.mark.gpu
FOLD = 0x10


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


@pytest.mark.parametrize("A", (1, 2, 3, 7, 16))
def test_folded_propose_against_the_restatement(gpu, torch_dev, A):
    assert gpu._abi.MCMC_FOLD == FOLD
    box = 0 if A == 16 else 7                                    # sixteen active columns leave no room for the overrides' targets
    flags = FOLD | box
    rng = np.random.default_rng(A)
    lo, hi, lg = _box_for(A, box, rng)
    assert rr.active_columns(lo, hi, box).size == A and lg.any()
    assert box == 0 or (np.any(lo == hi) and lo.size >= 9)       # a fixed column, and all three overrides apply
    seed = (0x1234567 << 32) | 0x89abcdef
    sim = {"override_equal_mu": bool(box & 1), "override_equal_s": bool(box & 2), "override_equal_auger": bool(box & 4)}
    # gamma 0.6 with the small jitter of tests/test_gpu_mcmc.py; gamma 2.5 with a jitter of up to 1.5: coordinates beyond [-1, 2],
    # which wrap more than once
    moves = ((0.6, rng.uniform(0.01, 0.05, A)), (2.5, rng.uniform(0.5, 1.5, A)))
    worst, codes, wrapped, rows = 0.0, np.zeros(3, dtype=np.int64), 0, 0
    for count in (1, 255, 256, 257, 1000):
        U = _states(rng, count, A)
        for P in (0, 2, 3, 1000):
            partners = rng.random((P, A)) if P else None
            for chain0 in (0, (1 << 32) + 5):
                for gamma, scale in moves:
                    step = 5
                    Up, Xp, inside = _propose_dev(torch_dev, U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags)
                    want_u, want_x, want_in = fr.propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, box, fold=True)
                    where = (count, P, chain0, gamma)
                    assert _same_bits(Up, want_u), where
                    assert np.array_equal(inside, want_in), where
                    worst = max(worst, _check_columns(Xp, want_x, lo, hi, lg, box))
                    live = inside != 0
                    assert np.all((Up[live] >= 0.0) & (Up[live] <= 1.0)), where
                    if count > 1:
                        assert inside[1] == 0 and np.isnan(Up[1, A - 1])          # a NaN coordinate: code 0
                    codes += np.bincount(inside, minlength=3)[:3]
                    raw, _ = mr.propose_unit(U, partners, gamma, scale, chain0, seed, step)
                    with np.errstate(invalid="ignore"):
                        wrapped += int(((raw < -1.0) | (raw > 2.0)).sum())
                    # the same call without the flag: a row that needed no fold has its bits, and is inside there
                    U0, X0, in0 = _propose_dev(torch_dev, U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, box)
                    plain = inside == 1
                    assert np.array_equal(in0 != 0, plain), where
                    assert _same_bits(Up[plain], U0[plain]) and _same_bits(Xp[plain], X0[plain]), where
                    rows += count
                    if count == 257 and P in (0, 3):
                        # a second call: the same bits; the host-buffer form: the same bits
                        again = _propose_dev(torch_dev, U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags)
                        assert _same_bits(again[0], Up) and _same_bits(again[1], Xp) and np.array_equal(again[2], inside)
                        Uh, Xh, ih = gpu.mcmc.propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, sim, fold=True)
                        assert _same_bits(Uh, Up) and _same_bits(Xh, Xp) and np.array_equal(ih, inside)
    print("folded propose A=%d: log columns within %.2f ulp; codes 0 / 1 / 2: %s of %d rows; %d coordinates beyond [-1, 2]"
          % (A, worst, codes, rows, wrapped))
    assert np.all(codes > 0)                                     # all three codes occurred
    assert wrapped > 0                                           # ... and a coordinate that wraps more than once


def test_the_face_toy_end_to_end_on_the_device(gpu):
    assert np.array_equal(mr.E2E_LO, TOY_LO) and np.array_equal(mr.E2E_HI, TOY_HI) and np.array_equal(mr.E2E_LG, TOY_LG)
    U0, X0, LL0, ref = fr.e2e_reference()
    assert ref["margin"] > mr.E2E_MARGIN                         # no decision near the margin: the device must decide the same
    calls = []

    def loglik(X):
        calls.append(X.shape[0])
        return fr.e2e_loglik(X)

    info = {}
    C, sweeps = fr.E2E["C"], fr.E2E["sweeps"]
    ch = gpu.mcmc.run(loglik, X0, LL0, TOY_LO, TOY_HI, TOY_LG, sweeps=sweeps, seed=fr.E2E["seed"], info=info, U0=U0, bounds="fold")
    assert ch.U.shape == (sweeps, C, 3)
    for t in range(sweeps):
        assert np.array_equal(ch.accept[t], ref["accepted"][t]), t
    assert _same_bits(ch.U, ref["U"])
    assert np.all((ch.U >= 0.0) & (ch.U <= 1.0))
    assert info["outside"] == 0 and sum(calls) == sweeps * C     # every proposal is solved
    assert info["folded"] == ref["folded"] and ref["folded"] > 0
    print("end to end, fold: acceptance %.3f, folded %.4f" % (np.mean(info["accept"]), info["folded"]))
