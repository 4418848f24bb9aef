#!/usr/bin/env python3
"""TRPL_FLAG_CUT against the plain fused likelihood, side by side in one process, device events, passes INTERLEAVED, median
of --reps.  Shape: Power_scan x 65 536 samples x 3 curves, L = 128, T = 8000 (the bench shape), default and TRPL_FLAG_PREDICT.
  1. OVERHEAD: trpl_loglik_dev against trpl_loglik_cut_dev at sse_cut = +inf (nothing is ever cut: the same work plus the
     compare per batch), synthetic observations as tools/bench_moments.py.  Required: cut / plain throughput >= 0.97, the bar of
     the moments and weighted sinks; exit status 1 below it.
  2. GAIN: the same shape against the shipped Balancedhighsurf observations (tests/golden/obs_balanced_full.csv.gz through
     dataio.get_data, as tools/e2e_production.py loads them, cut at the window).  The uncut pass's best total fixes
     sse_cut = exact_cut_margin(tf) + best_total for tf = 1 and the larger --tf values; recorded per tf: cut_fraction, the
     sum of iters_total cut / plain, the time ratio cut / plain, and how far the time ratio falls short of the iteration
     ratio (cut waves leave at batch boundaries, and a pair waits for its slower half).  No target: a measurement.
  3. LEVELS (--levels): trpl_loglik_cut_levels_dev with one value in every entry of cut_level against trpl_loglik_cut_dev at that
     sse_cut -- the same outputs bit for bit (asserted), so the ratio is the cost of reading the level per system: at +inf (nothing
     is cut) and at the median of the plain sse (half the systems are).  No target: a measurement.  --no-gain leaves out part 2.
  4. BUDGET (--budget; runs this part alone): trpl_loglik_cut_budget_dev with budget[s] = exact_cut_margin(tf) + best_total for
     every sample, curves_per_launch = 1 and = C, against the per-system call trpl_loglik_cut_dev at that level as sse_cut, in
     the same process with passes interleaved -- Power_scan against the shipped observations and Twothick x 6 curves against a
     straight line in log10 (no observations are shipped for it), default and TRPL_FLAG_PREDICT.  Recorded per (workload, mode,
     tf, g): cut_fraction, cut_samples, summed iters_total and seconds, each as a ratio budget / per-system.  With g = C the outputs
     are the per-system call's bit for bit (asserted).  No target: a measurement; serialising the curves costs parallelism.
One JSON line; the yardstick of every ratio is the plain call of the same run (part 4: the per-system call).
    python tools/bench_cut.py [--samples 65536] [--steps 8000] [--reps 3] [--tf 10,100] [--levels] [--no-gain] [--budget]
                              [--workloads power_scan,twothick] [--out FILE]"""
import argparse
import gzip
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

DT = 0.025
REQUIRED = 0.97


def shipped_observations(trpl_amd, T, C):
    """The shipped Balancedhighsurf observations cut at the window T * DT: (obs (C, ld), n_obs)."""
    work_dir = tempfile.mkdtemp(prefix="trpl_cut_")
    obs_csv = os.path.join(work_dir, "Balancedhighsurf_Power_scan_Observations.csv")
    with gzip.open(os.path.join(GOLDEN, "obs_balanced_full.csv.gz"), "rb") as fh, open(obs_csv, "wb") as out:
        out.write(fh.read())
    ic_flags = {"time_cutoff": T * DT, "select_obs_sets": None, "noise_level": None}
    e = trpl_amd.get_data([obs_csv], ic_flags, {"log_pl": True, "self_normalize": False}, scale_f=1e-23)[0]
    sim_t = np.linspace(0, T * DT, T + 1)
    n_real = [len(t) for t in e[0]]
    assert all(trpl_amd.is_grid_prefix(t, sim_t) for t in e[0]), "the shipped observation times are a prefix of the grid"
    obs_np = np.zeros((C, max(n_real)))
    for c in range(C):
        obs_np[c, :n_real[c]] = e[1][c]
    return obs_np, n_real


def budget_part(args, torch, trpl_amd, tdev, wl, exact_cut_margin, dev):
    S, T, L = args.samples, args.steps, 128
    tfs = [1.0] + [float(v) for v in args.tf.split(",") if v]
    line = {"part": "budget", "samples": S, "L": L, "T": T, "reps": args.reps, "yardstick": "trpl_loglik_cut_dev at the same level", "workloads": {}}

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*a); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for name in [w for w in args.workloads.split(",") if w]:
        ini, lens = wl.power_scan(L) if name == "power_scan" else wl.twothick(L)
        C = len(lens)
        if name == "power_scan":
            obs_np, n_obs = shipped_observations(trpl_amd, T, C)
            what = "obs_balanced_full.csv.gz via dataio.get_data, time_cutoff %g ns" % (T * DT)
        else:
            obs_np, n_obs = np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * C), [T + 1] * C
            what = "a straight line in log10, 18 - 0.2 t, on every grid point"
        X = torch.from_numpy(np.ascontiguousarray(wl.samples(S))).to(dev)
        ini_d = torch.from_numpy(np.ascontiguousarray(ini)).to(dev)
        obs = torch.from_numpy(np.ascontiguousarray(obs_np)).to(dev)
        P = torch.zeros(S, dtype=torch.float64, device=dev)
        sse, lv = (torch.zeros((C, S), dtype=torch.float64, device=dev) for _ in range(2))
        st, cc = (torch.zeros((C, S), dtype=torch.int32, device=dev) for _ in range(2))
        it = torch.zeros((C, S), dtype=torch.int64, device=dev)
        bd = torch.empty(S, dtype=torch.float64, device=dev)

        def plain(fl):
            P.zero_()
            tdev.loglik_device(X, ini_d, lens, T * DT, L, T, obs, n_obs, P, sse, st, iters_total=it, flags=fl)

        def per_system(fl, level):
            P.zero_()
            tdev.loglik_cut_device(X, ini_d, lens, T * DT, L, T, obs, n_obs, level, P, sse, cut_col=cc, status=st, iters_total=it, flags=fl)

        def budget(fl, g):
            P.zero_()
            tdev.loglik_cut_budget_device(X, ini_d, lens, T * DT, L, T, obs, n_obs, bd, lv, P, sse, curves_per_launch=g, cut_col=cc,
                                          status=st, iters_total=it, flags=fl)

        def counts():
            cut = cc >= 0
            return float(cut.double().mean()), float(cut.any(dim=0).double().mean()), int(it.sum())

        rec = {"curves": C, "observations": what, "n_obs": n_obs}
        for mode, fl in (("default", 0), ("predict", trpl_amd.FLAG_PREDICT)):
            plain(fl); torch.cuda.synchronize()
            total = sse.sum(dim=0)
            best_total = float(total[torch.isfinite(total)].min())
            rec[mode] = {"best_total": best_total, "plain_iters_total": int(it.sum()), "tf": {}}
            for tf in tfs:
                level = exact_cut_margin(tf) + best_total
                bd.fill_(level)
                per_system(fl, level); torch.cuda.synchronize()                                   # warm-up; the counts
                f0, s0, i0 = counts()
                want = (P.clone(), sse.clone(), cc.clone(), it.clone())
                out = {"level": level, "per_system": {"cut_fraction": f0, "cut_samples": s0, "iters_total": i0}}
                for g in (1, C):
                    budget(fl, g); torch.cuda.synchronize()
                    f1, s1, i1 = counts()
                    if g == C:
                        assert all(torch.equal(a, b) for a, b in zip(want, (P, sse, cc, it))), "one launch is the per-system call, bit for bit"
                    ty, tb = [], []
                    for _ in range(args.reps):                                                    # interleaved
                        ty.append(timed(per_system, fl, level))
                        tb.append(timed(budget, fl, g))
                    a, b = float(np.median(ty)), float(np.median(tb))
                    ratio = lambda x, y: x / y if y else None
                    out["g=%d" % g] = {"cut_fraction": f1, "cut_samples": s1, "iters_total": i1, "cut_fraction_ratio": ratio(f1, f0),
                                       "cut_samples_ratio": ratio(s1, s0), "iters_ratio": ratio(i1, i0), "time_ratio": b / a,
                                       "per_system_s": ty, "budget_s": tb}
                rec[mode]["tf"]["%g" % tf] = out
        line["workloads"][name] = rec
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tf", default="10,100", help="tempering factors measured beside tf = 1")
    ap.add_argument("--levels", action="store_true", help="also time trpl_loglik_cut_levels_dev at a uniform level array")
    ap.add_argument("--no-gain", action="store_true", help="leave out part 2")
    ap.add_argument("--budget", action="store_true", help="part 4 alone: trpl_loglik_cut_budget_dev against trpl_loglik_cut_dev")
    ap.add_argument("--workloads", default="power_scan,twothick", help="part 4: the workloads measured")
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    import torch
    import trpl_amd
    from trpl_amd import device as tdev, workloads as wl
    from trpl_amd.posterior import exact_cut_margin
    dev = torch.device("cuda", 0)
    S, T, L = args.samples, args.steps, 128
    if args.budget:
        return budget_part(args, torch, trpl_amd, tdev, wl, exact_cut_margin, dev)
    ini, lens = wl.power_scan(L)
    C = len(lens)
    X = torch.from_numpy(np.ascontiguousarray(wl.samples(S))).to(dev)
    ini_d = torch.from_numpy(np.ascontiguousarray(ini)).to(dev)
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    sse = torch.zeros((C, S), dtype=torch.float64, device=dev)
    st = torch.zeros((C, S), dtype=torch.int32, device=dev)
    it = torch.zeros((C, S), dtype=torch.int64, device=dev)
    cc = torch.zeros((C, S), dtype=torch.int32, device=dev)

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(*a); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    line = {"workload": "power_scan", "samples": S, "curves": C, "L": L, "T": T, "reps": args.reps, "required": REQUIRED}
    modes = (("default", 0), ("predict", trpl_amd.FLAG_PREDICT))

    # ---- 1. overhead ----
    obs = torch.from_numpy(np.ascontiguousarray(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * C))).to(dev)
    n_syn = [T + 1] * C

    def plain(fl, o, n):
        P.zero_()
        tdev.loglik_device(X, ini_d, lens, T * DT, L, T, o, n, P, sse, st, iters_total=it, flags=fl)

    def cut(fl, o, n, level):
        P.zero_()
        tdev.loglik_cut_device(X, ini_d, lens, T * DT, L, T, o, n, level, P, sse, cut_col=cc, status=st, iters_total=it, flags=fl)

    ok = True
    work = S * C * (T + 1)
    line["overhead"] = {}
    for mode, fl in modes:
        plain(fl, obs, n_syn); cut(fl, obs, n_syn, float("inf")); torch.cuda.synchronize()      # warm-up of both
        tp, tc = [], []
        for _ in range(args.reps):                                                                # interleaved
            tp.append(timed(plain, fl, obs, n_syn))
            tc.append(timed(cut, fl, obs, n_syn, float("inf")))
        a, b = float(np.median(tp)), float(np.median(tc))
        assert int((cc >= 0).sum()) == 0
        line["overhead"][mode] = {"plain_system_timesteps_per_s": work / a, "cut_system_timesteps_per_s": work / b,
                                  "cut_over_plain": a / b, "plain_s": tp, "cut_s": tc,
                                  "kernel": trpl_amd._abi.kernel_name(S * C, L, T, fl | trpl_amd._abi.FLAG_CUT)}
        ok = ok and a / b >= REQUIRED

    # ---- 3. the level call beside the scalar call at the same level ----
    if args.levels:
        lv = torch.empty((C, S), dtype=torch.float64, device=dev)

        def levels(fl, o, n):
            P.zero_()
            tdev.loglik_cut_levels_device(X, ini_d, lens, T * DT, L, T, o, n, lv, P, sse, cut_col=cc, status=st, iters_total=it, flags=fl)

        line["levels"] = {}
        for mode, fl in modes:
            plain(fl, obs, n_syn); torch.cuda.synchronize()
            rec = {}
            for what, level in (("inf", float("inf")), ("median", float(sse[st == 0].median()))):
                lv.fill_(level)
                cut(fl, obs, n_syn, level); torch.cuda.synchronize()
                want = (P.clone(), sse.clone(), cc.clone(), it.clone())
                levels(fl, obs, n_syn); torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(want, (P, sse, cc, it))), "the level call is the scalar call, bit for bit"
                ts, tl = [], []
                for _ in range(args.reps):                                                        # interleaved
                    ts.append(timed(cut, fl, obs, n_syn, level))
                    tl.append(timed(levels, fl, obs, n_syn))
                a, b = float(np.median(ts)), float(np.median(tl))
                rec[what] = {"level": level, "cut_fraction": float((cc >= 0).double().mean()), "levels_over_scalar_time": b / a,
                             "scalar_s": ts, "levels_s": tl}
            line["levels"][mode] = rec

    # ---- 2. gain against the shipped observations ----
    if args.no_gain:
        line["overhead_ok"] = ok
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")
        return 0 if ok else 1
    obs_np, n_real = shipped_observations(trpl_amd, T, C)
    obs_r = torch.from_numpy(obs_np).to(dev)
    tfs = [1.0] + [float(v) for v in args.tf.split(",") if v]
    line["gain"] = {"observations": "obs_balanced_full.csv.gz via dataio.get_data, time_cutoff %g ns" % (T * DT), "n_obs": n_real}
    for mode, fl in modes:
        plain(fl, obs_r, n_real); torch.cuda.synchronize()
        total = sse.sum(dim=0)
        best_total = float(total[torch.isfinite(total)].min())
        it_plain = int(it.sum())
        rec = {"best_total": best_total, "plain_iters_total": it_plain, "flagged": int((st != 0).sum()), "tf": {}}
        for tf in tfs:
            level = exact_cut_margin(tf) + best_total
            cut(fl, obs_r, n_real, level); torch.cuda.synchronize()                               # warm-up; the counts
            frac = float((cc >= 0).double().mean())
            it_cut = int(it.sum())
            tp, tc = [], []
            for _ in range(args.reps):
                tp.append(timed(plain, fl, obs_r, n_real))
                tc.append(timed(cut, fl, obs_r, n_real, level))
            a, b = float(np.median(tp)), float(np.median(tc))
            rec["tf"]["%g" % tf] = {"sse_cut": level, "cut_fraction": frac, "iters_cut_over_plain": it_cut / it_plain,
                                    "time_cut_over_plain": b / a, "time_minus_iters_ratio": b / a - it_cut / it_plain,
                                    "plain_s": tp, "cut_s": tc}
        line["gain"][mode] = rec
    line["overhead_ok"] = ok
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
