"""Writes tests/golden/corner_ref.npz: the corner of a small synthetic run computed by the REFERENCE's own functions -- exclude,
the functions of secondary_parameters.py, np.log10, normalize, marginalize_1D, marginalize_2D (Visualization/utils.py,
secondary_parameters.py), called in the order of plot() (marginalization_visual.py:500-609), not through the Tk class.
The reference is imported where it lies (TRPL_REFERENCE, with oracle/refshim on the path for `statsmodels`, as
oracle/gen_golden.py does); without it this refuses to run.  The file holds data only: the seed, the limits, tf, kept and
the 1-D and 2-D densities.  X is not stored: tests/corner_ref.draw(seed, S) redraws it.

LI_tau_eff is called as it is DEFINED, with CP = X[:, 8] (the reference's own call, utils.py:61-62, leaves CP out and
cannot run).

The seed is the first for which the reference's own values satisfy: no plotted value within 64 ulp of a bin edge, no raw value
within 64 ulp of an exclusion limit (as held, or as 10 ** log10(limit)), and 25 % .. 90 % of the samples kept.
Usage: python tools/gen_corner_golden.py"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TRPL_REFERENCE", "/root/reference")
if not os.path.isfile(os.path.join(REF, "Visualization", "utils.py")):
    sys.exit("gen_corner_golden.py: reference checkout not found at %s -- refusing to run" % REF)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "Visualization"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import secondary_parameters as sp  # noqa: E402  (reference)
import utils as vis  # noqa: E402  (reference)

import corner_ref  # noqa: E402

# marginalization_visual.py:67-73
PARAM_ORDER = [r"$n_0$", r"$p_0$", r"$\mu_n$", r"$\mu_p$", r"$k^*$", r"$S_F$", r"$S_B$", r"$C_n$", r"$C_p$", r"$\tau_n$",
               r"$\tau_p$", r"$\lambda$", r"$m$", r"$\tau_{eff}$", r"$\tau_{rad}$", r"$(S_F+S_B)$", r"$\mu\prime$", r"$\epsilon$",
               r"$\tau_n+\tau_p$"]
SECONDARY = {p: i >= 13 for i, p in enumerate(PARAM_ORDER)}
TEX = dict(zip(corner_ref.NAMES, PARAM_ORDER))

S, BINS, TF, THICKNESS = 2048, 24, 2.0, 2000.0
ENABLED = ["p0", "mun", "taun", "tau_eff", "mu'", "Sf+Sb"]
DO_LOG = ["p0", "tau_eff"]
# the limits as the GUI holds them before loglimits(): raw values
RAW_LIMITS = {"p0": (2e14, 6e15), "mun": (2.5, 45.5), "taun": (50.5, 950.5), "tau_eff": (0.5, 300.0), "mu'": (2.0, 40.0),
              "Sf+Sb": (1.0, 150.0)}


def run(seed):
    X, LL = corner_ref.draw(seed, S)
    enabled = [TEX[n] for n in ENABLED]
    axis_limits = {TEX[n]: RAW_LIMITS[n] for n in ENABLED}
    # exclude_using_axis_limits, utils.py:48-52
    exclusion = {p: axis_limits[p] for p in enabled if not SECONDARY[p]}
    where, Xk = vis.exclude(X, exclusion, PARAM_ORDER)
    LLk = LL[where]
    cols = {p: np.array(Xk[:, i]) for i, p in enumerate(PARAM_ORDER) if not SECONDARY[p]}      # pack_X_param_indexable
    # calculate_secondary_params, utils.py:54-79
    mu_total = sp.mu_eff(cols[r"$\mu_n$"], cols[r"$\mu_p$"])
    cols[r"$\mu\prime$"] = mu_total
    cols[r"$\tau_{eff}$"] = sp.LI_tau_eff(cols[r"$k^*$"], cols[r"$p_0$"], cols[r"$\tau_n$"], cols[r"$S_F$"], cols[r"$S_B$"],
                                         cols[r"$C_p$"], THICKNESS, mu_total)
    cols[r"$(S_F+S_B)$"] = sp.s_eff(cols[r"$S_F$"], cols[r"$S_B$"])
    raw_cols = {p: cols[p].copy() for p in enabled}
    for n in DO_LOG:                                              # logX and loglimits, plotutils.py:56-59
        cols[TEX[n]] = np.log10(cols[TEX[n]])
        a = axis_limits[TEX[n]]
        axis_limits[TEX[n]] = (np.log10(a[0]), np.log10(a[1]))
    P = vis.normalize(LLk / TF)                                   # marginalization_visual.py:589-591
    h1 = np.stack([vis.marginalize_1D(P, axis_limits, BINS, SECONDARY, p, cols[p])[0] for p in enabled])
    h2 = []
    for i, py in enumerate(enabled):                              # utils.py:103-106
        for j, px in enumerate(enabled):
            if i > j:
                h2.append(vis.marginalize_2D(P, axis_limits, BINS, SECONDARY, (px, py), cols[px], cols[py])[0])
    kept = int(len(LLk))
    # the conditions, on the reference's own values
    margin = np.inf
    for p in enabled:
        lo, hi = axis_limits[p]
        margin = min(margin, corner_ref.ulp_margin(cols[p], lo + (hi - lo) * np.arange(BINS + 1) / BINS))
    for n in ENABLED:
        c = corner_ref.NAMES.index(n)
        if c < 13:
            a, b = RAW_LIMITS[n]
            pts = [a, b]
            if n in DO_LOG:
                pts += [10.0 ** np.log10(a), 10.0 ** np.log10(b)]
            margin = min(margin, corner_ref.ulp_margin(X[:, c], pts))
    ok = margin >= 64 and 0.25 * S <= kept <= 0.90 * S
    lo = np.array([axis_limits[TEX[n]][0] for n in ENABLED])
    hi = np.array([axis_limits[TEX[n]][1] for n in ENABLED])
    return ok, dict(seed=seed, S=S, bins=BINS, tf=TF, thickness=THICKNESS, names=np.array(ENABLED), do_log=np.array(DO_LOG), lo=lo,
                    hi=hi, kept=kept, h1=h1, h2=np.stack(h2), margin_ulp=margin)


if __name__ == "__main__":
    for seed in range(1000):
        ok, out = run(seed)
        if ok:
            break
    else:
        sys.exit("no seed satisfies the conditions")
    assert ok and out["margin_ulp"] >= 64 and 0.25 * S <= out["kept"] <= 0.90 * S
    path = os.path.join(ROOT, "tests", "golden", "corner_ref.npz")
    np.savez_compressed(path, **out)
    print("seed %d: kept %d of %d, smallest margin %.3g ulp -> %s (%d bytes)" % (out["seed"], out["kept"], S, out["margin_ulp"], path,
                                                                                os.path.getsize(path)))
