#!/usr/bin/env python3
"""TRPL_FLAG_MOMENTS against the plain fused likelihood, side by side in one process: the default bench shape (Power_scan x
65 536 samples x 3 curves, L = 128, T = 8000) through trpl_loglik_dev and trpl_loglik_moments_dev, with and without
TRPL_FLAG_PREDICT, the passes INTERLEAVED (plain, moments, plain, moments, ...) and timed with device events; then
trpl_mag_grid_dev at M = 32 offsets on the moments just produced, with its achieved fraction of HBM bandwidth (it streams
2 C S 8 B of moments in and M S 8 B of likelihoods in and out).  One JSON line; the yardstick of the ratios is the plain
call of the same run.
    python tools/bench_moments.py [--samples 65536] [--steps 8000] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.025
HBM_PEAK = 8.0e12                   # B/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--offsets", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    import torch
    import trpl_amd
    from trpl_amd import device as tdev, workloads as wl
    dev = torch.device("cuda", 0)
    S, T, L, M = args.samples, args.steps, 128, args.offsets
    ini, lens = wl.power_scan(L)
    C = len(lens)
    X = torch.from_numpy(np.ascontiguousarray(wl.samples(S))).to(dev)
    ini_d = torch.from_numpy(np.ascontiguousarray(ini)).to(dev)
    obs = torch.from_numpy(np.ascontiguousarray(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * C))).to(dev)
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    sse = torch.zeros((C, S), dtype=torch.float64, device=dev)
    esum = torch.zeros((C, S), dtype=torch.float64, device=dev)
    st = torch.zeros((C, S), dtype=torch.int32, device=dev)

    def plain(fl):
        tdev.loglik_device(X, ini_d, lens, T * DT, L, T, obs, T + 1, P, sse, st, flags=fl)

    def moments(fl):
        tdev.loglik_moments_device(X, ini_d, lens, T * DT, L, T, obs, T + 1, P, sse, esum, st, flags=fl)

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*a); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    line = {"workload": "power_scan", "samples": S, "curves": C, "L": L, "T": T, "reps": args.reps}
    work = S * C * (T + 1)
    for mode, fl in (("default", 0), ("predict", trpl_amd.FLAG_PREDICT)):
        plain(fl); moments(fl); torch.cuda.synchronize()                       # warm-up of both
        tp, tm = [], []
        for _ in range(args.reps):                                             # interleaved
            tp.append(timed(plain, fl))
            tm.append(timed(moments, fl))
        a, b = float(np.median(tp)), float(np.median(tm))
        line[mode] = {"plain_system_timesteps_per_s": work / a, "moments_system_timesteps_per_s": work / b,
                      "moments_over_plain": a / b, "plain_s": tp, "moments_s": tm,
                      "kernel": trpl_amd._abi.kernel_name(S * C, L, T, fl | trpl_amd._abi.FLAG_MOMENTS)}
    offs = np.linspace(-2.5, 2.5, M)
    Pg = torch.zeros((M, S), dtype=torch.float64, device=dev)
    n_obs = [T + 1] * C
    tdev.mag_grid_device(sse, esum, n_obs, offs, Pg); torch.cuda.synchronize()
    tg = [timed(tdev.mag_grid_device, sse, esum, n_obs, offs, Pg) for _ in range(max(5, args.reps))]
    g = float(np.median(tg))
    nbytes = 2 * C * S * 8 + 2 * M * S * 8
    line["mag_grid"] = {"M": M, "seconds": g, "bytes": nbytes, "GB_per_s": nbytes / g / 1e9, "hbm_fraction": nbytes / g / HBM_PEAK,
                        "likelihoods_per_s": M * S / g}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
