"""The posterior-predictive accumulation against the resident-PL likelihood, in one process on one device.

    python tools/bench_predictive.py [--rows 16384] [--ncol 80001] [--elem 4] [--zero 0.9] [--out profiles/predictive_bench.jsonl]

band:      one trpl_predictive_accumulate_dev over a [rows][ncol] PL matrix (ld = ncol: odd, rows only element-aligned), all
           rows used; then again with the fraction --zero of the weights exactly 0.0 (those rows are never read).
yardstick: trpl_loglik_from_pl_dev on the same matrix in the same run -- it reads the same bytes with one log10 per element.
Device events; two matrices are used in turn (each alone is many times the 256 MiB Infinity Cache); warm-up of every timed call;
the passes of the three measurements interleaved, median of 3 passes of `reps` calls each.  Reported: the bytes of the used
rows over the time, as a rate and as a fraction of the 8 TB/s peak.  Appends one JSON line to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import trpl_amd      # noqa: E402
from trpl_amd import device as tdev   # noqa: E402

PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--ncol", type=int, default=80001)
    ap.add_argument("--elem", type=int, default=4, choices=[4, 8])
    ap.add_argument("--zero", type=float, default=0.9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_bench.jsonl"))
    a = ap.parse_args()
    rows, ncol = a.rows, a.ncol
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    dt = torch.float32 if a.elem == 4 else torch.float64
    mats = []
    for _ in range(2):                                   # PL = 10^U(-12, 0): a decaying curve's range
        pl = torch.empty((rows, ncol), dtype=dt, device=dev)
        pl.uniform_(-12.0, 0.0, generator=g)
        pl.mul_(float(np.log(10.0))).exp_()
        mats.append(pl)
    mag = torch.rand(rows, dtype=torch.float64, device=dev, generator=g) * 6 - 3
    obs = torch.randn(ncol, dtype=torch.float64, device=dev, generator=g)
    W_all = torch.rand(rows, dtype=torch.float64, device=dev, generator=g) + 0.1
    W_all /= W_all.sum()
    keep = torch.rand(rows, dtype=torch.float64, device=dev, generator=g) >= a.zero
    W_few = torch.where(keep, W_all, torch.zeros_like(W_all))
    used_few = int(keep.sum().item())
    sse = torch.zeros(rows, dtype=torch.float64, device=dev)
    state = tdev.predictive_state(ncol)
    ws = tdev.predictive_workspace(rows, ncol, a.elem)
    turn = [0]

    def band(W):
        def run():
            turn[0] ^= 1
            tdev.predictive_accumulate_device(mats[turn[0]], W, state, ws, mag=mag)
        return run

    def yard():
        turn[0] ^= 1
        tdev.loglik_from_pl_device(mats[turn[0]], obs, mag, sse=sse)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    fns = {"band_all": band(W_all), "band_few": band(W_few), "loglik": yard}
    tdev.predictive_init_device(state)
    for fn in fns.values():                              # warm-up, on both matrices
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(3):                                   # interleaved passes
        for k, fn in fns.items():
            t[k].append(timed(fn, a.reps))
    ms = {k: float(np.median(v)) for k, v in t.items()}
    row_bytes = ncol * a.elem
    chunks = int(trpl_amd._abi.lib().trpl_predictive_chunks(rows, ncol, a.elem))
    line = {"bench": "predictive", "rows": rows, "ncol": ncol, "elem_bytes": a.elem, "device": torch.cuda.get_device_name(0),
            "chunks": chunks, "workspace_bytes": chunks * ncol * 40, "reps": a.reps, "ms": ms, "ms_passes": t,
            "band_all_used_bytes": rows * row_bytes, "band_all_TBps": rows * row_bytes / ms["band_all"] / 1e9,
            "band_all_fraction_of_peak": rows * row_bytes / ms["band_all"] / 1e9 / PEAK_TBS,
            "loglik_TBps": rows * row_bytes / ms["loglik"] / 1e9,
            "loglik_fraction_of_peak": rows * row_bytes / ms["loglik"] / 1e9 / PEAK_TBS,
            "band_all_over_loglik": ms["band_all"] / ms["loglik"],
            "zero_fraction": a.zero, "band_few_used_rows": used_few, "band_few_used_bytes": used_few * row_bytes,
            "band_few_TBps": used_few * row_bytes / ms["band_few"] / 1e9,
            "band_few_fraction_of_peak": used_few * row_bytes / ms["band_few"] / 1e9 / PEAK_TBS,
            "band_few_over_band_all": ms["band_few"] / ms["band_all"], "used_rows_fraction": used_few / rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
