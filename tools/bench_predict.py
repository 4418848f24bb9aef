#!/usr/bin/env python3
"""TRPL_FLAG_PREDICT against the default path, side by side: bench.py's fused workloads and event timing (bench.one_pass),
one JSON line per configuration with both modes' system-timesteps/s, likelihoods/s, mean inner iterations per step,
roofline fraction (268 L flops per iteration, as bench.py) and kernel name, and predict's PL error against the default path
on a seeded subset (the batch's first n_sub samples, the timed kernel, every column above TRPL_PL_FLOOR_EXCESS), by height
above the floor and against a tol-11 solution.
    python tools/bench_predict.py [--only NAME ...] [--n-sub 256] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the yardstick's own workloads and timing)

DT = 0.025
FLOOR = 1e-4                        # TRPL_PL_FLOOR_EXCESS
CONFIGS = [                         # name, workload, samples, L, T, tol
    ("power_scan_T8000", "power_scan", 65536, 128, 8000, 7),
    ("power_scan_T80000", "power_scan", 65536, 128, 80000, 7),
    ("twothick_T8000", "twothick", 65536, 128, 8000, 7),
    ("L512_tol7_T8000", "power_scan", 32768, 512, 8000, 7),
]


def pl_error(torch, tdev, trpl_amd, wl, dev, workload, S, L, T, tol, n_sub):
    """predict's PL against the default path's on the batch's first n_sub samples, per curve, on the kernel the timed pass ran
    (the variant pinned for the full batch of S samples), every column above TRPL_PL_FLOOR_EXCESS.  r = PL / (B L n0 p0) is a
    point's height above the floor in units of the equilibrium excess (the floor is r = 1e-4).  Reports the deviation per decade
    of r, the envelope constant each decade needs (max dev * r), and the worst points against a tol-11 solution of the same
    systems: which path is closer to the exact step solution where the two disagree most."""
    Time = T * DT
    ini, lens = wl.power_scan(L) if workload == "power_scan" else wl.twothick(L)
    Xh = wl.samples(n_sub)
    X = torch.from_numpy(np.ascontiguousarray(Xh[:, :12])).to(dev)
    ini_d = torch.from_numpy(ini).to(dev)
    base = trpl_amd._abi.pin_variant(0, S * len(lens), L, T)
    runs = (("default", base, tol), ("predict", base | trpl_amd.FLAG_PREDICT, tol), ("tol11", base, 11))
    devs, rs, e_d, e_p, where, flagged = [], [], [], [], [], {n: 0 for n, _, _ in runs}
    for c in range(len(lens)):
        out = {}
        for name, fl, tl in runs:
            pl = torch.empty((n_sub, T + 1), dtype=torch.float64, device=dev)
            st = torch.empty(n_sub, dtype=torch.int32, device=dev)
            tdev.solve_pl_device(X, lens[c], Time, L, T, ini_d[c].contiguous(), pl, status=st, tol=tl, flags=fl)
            torch.cuda.synchronize()
            out[name] = pl.cpu().numpy()
            flagged[name] += int((st != 0).sum().item())
        dx = lens[c] / L
        scale = Xh[:, 4] * L * Xh[:, 0] * Xh[:, 1] * dx                  # B L n0 p0 in PL units (tests/gpu_common.excess_scale)
        r = out["default"] / scale[:, None]
        ok = r >= FLOOR
        devs.append(np.abs(out["predict"][ok] / out["default"][ok] - 1))
        rs.append(r[ok])
        e_d.append(np.abs(out["default"][ok] / out["tol11"][ok] - 1))
        e_p.append(np.abs(out["predict"][ok] / out["tol11"][ok] - 1))
        si, ci = np.nonzero(ok)
        where.append(np.stack([np.full(si.size, c), si, ci], axis=1))
    d, r, ed, ep, w = (np.concatenate(v) for v in (devs, rs, e_d, e_p, where))
    decades = []
    for lo in (1e-4, 1e-3, 1e-2, 1e-1, 1.0):
        m = (r >= lo) & (r < lo * 10 if lo < 1.0 else np.isfinite(r))
        if m.any():
            decades.append({"r_from": lo, "r_to": lo * 10 if lo < 1.0 else None, "points": int(m.sum()),
                            "max": float(d[m].max()), "median": float(np.median(d[m])), "max_dev_times_r": float((d[m] * r[m]).max())})
    top = np.argsort(d)[::-1][:8]
    worst = [{"curve": int(w[i, 0]), "sample": int(w[i, 1]), "column": int(w[i, 2]), "r": float(r[i]), "dev": float(d[i]),
              "default_vs_tol11": float(ed[i]), "predict_vs_tol11": float(ep[i])} for i in top]
    return {"max": float(d.max()), "median": float(np.median(d)), "points": int(d.size),
            "max_dev_times_r": float((d * r).max()), "by_r_decade": decades, "worst_points": worst,
            "vs_tol11_max": {"default": float(ed.max()), "predict": float(ep.max())},
            "flagged": flagged,
            "against": "default path on the timed kernel (%s), the batch's first %d samples x %d curves, every PL column above "
                       "TRPL_PL_FLOOR_EXCESS; tol11 = the same kernel at tol 1e-11" % (
                           trpl_amd._abi.kernel_name(S * len(lens), L, T, base | trpl_amd.FLAG_PREDICT), n_sub, len(lens))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--n-sub", type=int, default=256)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--errors-only", action="store_true", help="only the PL-error characterisation (no timed passes)")
    args = ap.parse_args()
    import torch
    import trpl_amd
    from trpl_amd import device as tdev, workloads as wl
    dev = torch.device("cuda", 0)
    keep = ("system_timesteps_per_s", "likelihoods_per_s_at_T", "mean_inner_iterations_per_step", "roofline_frac",
            "roofline_achieved_tflops", "ms", "rocprof_name", "nonconverged", "finite_likelihoods")
    for name, workload, S, L, T, tol in CONFIGS:
        if args.only and name not in args.only:
            continue
        line = {"config": name, "workload": workload, "samples": S, "L": L, "T": T, "tol_exp": tol}
        for mode, fl in (("default", 0), ("predict", trpl_amd.FLAG_PREDICT)):
            line[mode] = {}
            if args.errors_only:
                continue
            torch.cuda.empty_cache()
            r = bench.one_pass(torch, tdev, trpl_amd, wl, dev, workload, S, L, T, DT, tol, flags=fl)
            line[mode] = {k: r[k] for k in keep}
        torch.cuda.empty_cache()
        line["predict"]["pl_rel_err_vs_default"] = pl_error(torch, tdev, trpl_amd, wl, dev, workload, S, L, T, tol,
                                                            args.n_sub)
        d, p = line["default"], line["predict"]
        if args.errors_only:
            print(json.dumps(line), flush=True)
            continue
        line["speedup"] = p["system_timesteps_per_s"] / d["system_timesteps_per_s"]
        line["iteration_ratio"] = p["mean_inner_iterations_per_step"] / d["mean_inner_iterations_per_step"]
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
