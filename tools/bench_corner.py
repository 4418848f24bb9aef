"""The corner against what a user has without it, in one process on one device.

    python tools/bench_corner.py [--S 131072] [--D 6 13 19] [--bins 96] [--reps 5] [--out profiles/corner_bench.jsonl]

corner:  corner_columns_device + posterior_weights_device + corner_hist_device on resident tensors: D columns, D 1-D histograms
         with counts and D (D - 1) / 2 2-D histograms.
parent:  the same result with the entry points that exist without the corner: the columns formed with torch (the secondary
         parameters by the expressions of secondary_parameters.py, log10), the exclusion as a NaN in the likelihoods,
         posterior_weights_device, and one posterior_hist_device call per histogram (2 D calls for the 1-D sums and counts,
         D (D - 1) / 2 for the pairs), each into a zeroed output.
Both on the same tensors in HBM (no uploads on either side: the per-call uploads of marginalize_1D / _2D would only add to the
parent).  Device events; warm-up of every timed call; the passes of the two interleaved, median of 3 passes of `reps` calls each.
One workgroup per histogram leaves most of the device idle at small D: the times say how much that costs.  Appends one JSON
line per D to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np   # noqa: E402
import torch         # noqa: E402
import trpl_amd      # noqa: E402
from trpl_amd import _abi, device as tdev, sampler as sm   # noqa: E402
from bench_quantiles import measure   # noqa: E402

ORDER = [1, 9, 13, 16, 15, 2, 3, 4, 5, 6, 7, 8, 10, 14, 17, 18, 0, 11, 12]          # the first D of these are enabled
LOGGED = {0, 1, 4, 5, 6, 7, 8, 11, 13, 14}


def torch_column(X, c, th):
    n0, p0, mun, mup, B, Sf, Sb, CN, CP, taun, taup, lam, m = X.unbind(1)
    if c < 13:
        return X[:, c]
    mu = 2 / (1 / mun + 1 / mup)
    t_r = 1 / (B * p0) * 1e9
    if c == 13:
        t_aug = 1 / (CP * p0 ** 2) * 1e9
        Dif = mu * 0.0257 / 1 * 1e14 / 1e9
        tau_surf = (th / ((Sf + Sb) * 0.01)) + (th ** 2 / (np.pi ** 2 * Dif))
        return 1 / (1 / t_r + 1 / t_aug + 1 / tau_surf + 1 / taun)
    return {14: t_r, 15: Sf + Sb, 16: mu, 17: 1 / lam, 18: taun + taup}[c]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=1 << 17)
    ap.add_argument("--D", type=int, nargs="+", default=[6, 13, 19])
    ap.add_argument("--bins", type=int, default=96)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, bins, th = a.S, a.bins, 2000.0
    lo = np.where(sm.DEFAULT_MINX == sm.DEFAULT_MAXX, sm.DEFAULT_MINX * 0.5, sm.DEFAULT_MINX)
    hi = np.where(sm.DEFAULT_MINX == sm.DEFAULT_MAXX, sm.DEFAULT_MAXX * 2.0 + 1.0, sm.DEFAULT_MAXX)
    lo = np.where(lo <= 0, 1e-3, lo)                             # every column positive: all of them can be logged
    X = torch.empty((S, 13), dtype=torch.float64, device=dev)
    tdev.sample_box_device(X, lo, hi, sm.DEFAULT_DO_LOG, seed=42)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    LL = -200.0 * torch.rand(S, dtype=torch.float64, device=dev, generator=g)       # weights over 87 decades: most of them > 0
    elo, ehi = np.full(13, np.nan), np.full(13, np.nan)
    elo[9], ehi[9] = 50.0, 950.0                                 # tau_n limited: ~10 % of the samples excluded
    wsp = tdev.posterior_workspace(1)
    for D in a.D:
        codes = ORDER[:D]
        dolog = [int(c in LOGGED) for c in codes]
        V = torch.empty((D, S), dtype=torch.float64, device=dev)
        LLk, W = torch.empty_like(LL), torch.empty_like(LL)
        kept = torch.zeros(1, dtype=torch.int64, device=dev)
        tdev.corner_columns_device(X, codes, V, do_log=dolog, thickness=th, excl_lo=elo, excl_hi=ehi, LL=LL, LLk=LLk, kept=kept)
        fin = torch.where(torch.isfinite(V), V, torch.nan)
        vlo = [float(v) for v in torch.nan_to_num(fin, nan=float("inf")).amin(1).cpu()]
        vhi = [float(v) for v in torch.nan_to_num(fin, nan=float("-inf")).amax(1).cpu()]
        npair = D * (D - 1) // 2
        h1 = torch.empty((D, bins), dtype=torch.float64, device=dev)
        c1 = torch.empty_like(h1)
        h2 = torch.empty((npair, bins, bins), dtype=torch.float64, device=dev)
        ws = tdev.corner_workspace(S, D)
        o1, oc, o2 = torch.empty_like(h1), torch.empty_like(h1), torch.empty_like(h2)
        pairs = [(j, i) for i in range(D) for j in range(i)]

        def corner():
            tdev.corner_columns_device(X, codes, V, do_log=dolog, thickness=th, excl_lo=elo, excl_hi=ehi, LL=LL, LLk=LLk, kept=kept)
            tdev.posterior_weights_device(LLk, 1.0, W, wsp)
            tdev.corner_hist_device(V, W, vlo, vhi, h1, ws, c1=c1, h2=h2)

        def parent():
            Vp = torch.stack([torch.log10(torch_column(X, c, th)) if lg else torch_column(X, c, th) for c, lg in zip(codes, dolog)])
            keep = (X[:, 9] <= ehi[9]) & (X[:, 9] >= elo[9])
            Lp = torch.where(keep, LL, torch.nan)
            Wp = torch.empty_like(LL)
            tdev.posterior_weights_device(Lp, 1.0, Wp, wsp)
            Wz = torch.nan_to_num(Wp, nan=0.0)                   # the old kernel adds every weight it is given
            Wc = (~torch.isnan(Wp)).to(torch.float64)
            o1.zero_(); oc.zero_(); o2.zero_()
            for d in range(D):
                tdev.posterior_hist_device(Vp[d], Wz, vlo[d], vhi[d], o1[d])
                tdev.posterior_hist_device(Vp[d], Wc, vlo[d], vhi[d], oc[d])
            for p, (j, i) in enumerate(pairs):
                tdev.posterior_hist_device(Vp[j], Wz, vlo[j], vhi[j], o2[p], y=Vp[i], ylo=vlo[i], yhi=vhi[i])

        ms, passes = measure({"corner": corner, "parent": parent}, a.reps)
        torch.cuda.synchronize()
        agree = float(((h1 - o1).abs() / o1.abs().clamp_min(1e-300)).max())
        line = {"bench": "corner", "device": torch.cuda.get_device_name(0), "S": S, "D": D, "bins": bins, "histograms": D + npair,
                "reps": a.reps, "kept": int(kept.item()), "nonzero_weights": int((W > 0).sum().item()), "ms": ms, "ms_passes": passes,
                "corner_over_parent": ms["corner"] / ms["parent"], "h1_max_rel_diff_to_parent": agree,
                "counts_equal": bool(torch.equal(c1, oc))}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
