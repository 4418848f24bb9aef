#!/usr/bin/env python3
"""TRPL_FLAG_WEIGHTED against the moments call it is built on, side by side in one process: the default bench shape
(Power_scan x 65 536 samples x 3 curves, L = 128, T = 8000) through trpl_loglik_moments_dev and trpl_loglik_weighted_dev, with
and without TRPL_FLAG_PREDICT, the passes INTERLEAVED (moments, weighted, moments, weighted, ...) and timed with device
events, median of --reps.  One JSON line; the yardstick of the ratios is the moments call of the same run (the kernel the
library had before the weighted sink), never the weighted call itself.  Required: weighted_over_moments >= 0.97 (DESIGN.md
section 11); the exit status is 1 below it.
    python tools/bench_weighted.py [--samples 65536] [--steps 8000] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.025
REQUIRED = 0.97


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    import torch
    import trpl_amd
    from trpl_amd import device as tdev, workloads as wl
    dev = torch.device("cuda", 0)
    S, T, L = args.samples, args.steps, 128
    ini, lens = wl.power_scan(L)
    C = len(lens)
    X = torch.from_numpy(np.ascontiguousarray(wl.samples(S))).to(dev)
    ini_d = torch.from_numpy(np.ascontiguousarray(ini)).to(dev)
    obs = torch.from_numpy(np.ascontiguousarray(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * C))).to(dev)
    # a constant absolute sigma: the relative one grows along the decay (the shipped data's error column)
    u = np.stack([0.01 * 10.0 ** (2.0 * np.arange(T + 1) / T + 0.1 * c) for c in range(C)])
    wts = torch.from_numpy(np.ascontiguousarray(1.0 / (2.0 * u * u))).to(dev)
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    sse = torch.zeros((C, S), dtype=torch.float64, device=dev)
    esum = torch.zeros((C, S), dtype=torch.float64, device=dev)
    st = torch.zeros((C, S), dtype=torch.int32, device=dev)

    def moments(fl):
        tdev.loglik_moments_device(X, ini_d, lens, T * DT, L, T, obs, T + 1, P, sse, esum, st, flags=fl)

    def weighted(fl):
        tdev.loglik_weighted_device(X, ini_d, lens, T * DT, L, T, obs, wts, T + 1, P, sse, esum, st, flags=fl)

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*a); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    line = {"workload": "power_scan", "samples": S, "curves": C, "L": L, "T": T, "reps": args.reps, "required_ratio": REQUIRED}
    work = S * C * (T + 1)
    ok = True
    for mode, fl in (("default", 0), ("predict", trpl_amd.FLAG_PREDICT)):
        moments(fl); weighted(fl); torch.cuda.synchronize()                    # warm-up of both
        assert not st.any().item() and torch.isfinite(sse).all().item()
        tm, tw = [], []
        for _ in range(args.reps):                                             # interleaved
            tm.append(timed(moments, fl))
            tw.append(timed(weighted, fl))
        a, b = float(np.median(tm)), float(np.median(tw))
        ok = ok and a / b >= REQUIRED
        line[mode] = {"moments_system_timesteps_per_s": work / a, "weighted_system_timesteps_per_s": work / b,
                      "weighted_over_moments": a / b, "moments_s": tm, "weighted_s": tw,
                      "kernel": trpl_amd._abi.kernel_name(S * C, L, T, fl | trpl_amd._abi.FLAG_WEIGHTED)}
    line["pass"] = ok
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
