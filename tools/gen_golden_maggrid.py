#!/usr/bin/env python3
"""Generate tests/golden/lnp_maggrid.npz: the reference's own mag_grid likelihood, probs.lnP (probs.py:5-18), on the
reference PL already committed in tests/golden/pvsim_power.npz / pvsim_twothick.npz against seeded synthetic observations.

    python tools/gen_golden_maggrid.py [path-to-the-reference-checkout]

Puts oracle/refshim (the sequential stand-in for the absent numba) and the reference on sys.path, calls
probs.lnP(P, log10 plI + mag, values, mag_grid, sys.float_info.min, 1.0) once per curve and stores NUMBERS ONLY: the
observations, the per-sample offsets, the offset grid and P_ref[c][s][m] with lnP's constant n ln(pi) / 2 added back, so
that P_ref = - sum_i (log10 PL_i + mag_s + d_m - obs_i)^2.  Nothing under oracle/ changes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OFFSETS = np.linspace(-2.5, 2.5, 21)


def case(probs, name, seed):
    z = np.load(os.path.join(GOLDEN, name))
    pl = np.asarray(z["plI"], dtype=np.float64)                       # (C, S, n) reference PL
    C, S, n = pl.shape
    rng = np.random.default_rng(seed)
    lg = np.log10(pl)
    obs = lg[:, 0, :] + 0.3 + 0.05 * rng.standard_normal((C, n))      # the first sample's curve, shifted, with noise
    mag = rng.uniform(-1.0, 1.0, size=S)                              # X[:, 12]
    P_ref = np.zeros((C, S, len(OFFSETS)))
    for c in range(C):
        P = np.zeros((S, len(OFFSETS)))
        probs.lnP(P, lg[c] + mag[:, None], obs[c], OFFSETS, sys.float_info.min, 1.0)
        P_ref[c] = P + np.log(np.pi * 1.0) / 2 * n                    # lnP's constant, added back
    return obs, mag, P_ref


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TRPL_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
    import probs
    out = {"offsets": OFFSETS}
    for key, name, seed in (("power", "pvsim_power.npz", 1), ("twothick", "pvsim_twothick.npz", 2)):
        obs, mag, P_ref = case(probs, name, seed)
        out["obs_" + key], out["mag_" + key], out["P_ref_" + key] = obs, mag, P_ref
    np.savez(os.path.join(GOLDEN, "lnp_maggrid.npz"), **out)
    print("wrote lnp_maggrid.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
