"""The weighted quantiles against their yardsticks, in one process on one device.

    python tools/bench_quantiles.py [--form param|band] [--S 131072] [--D 19] [--n 1024] [--ncol 80001] [--elem 8]
                                    [--out profiles/quantiles_bench.jsonl]

param: trpl_weighted_quantiles_dev over V (D, S) with K = 2 (the credible interval of every parameter, one call);
       yardstick: device.credible_interval_device once per column on the same tensors (torch.sort + cumsum + two nonzero).
band:  trpl_predictive_gather_dev of a PL block (n, ncol) into the y store and trpl_weighted_quantiles_dev over the store with
       K = 3, timed separately; yardsticks: torch.sort(Y, dim=1) + cumsum + searchsorted on the same store for the selection,
       trpl_predictive_accumulate_dev on the source block (the same bytes read) for the gather.
Device events; two buffers are used in turn; warm-up of every timed call; the passes of the measurements interleaved, median
of 3 passes of `reps` calls each.  Appends one JSON line to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import trpl_amd      # noqa: E402
from trpl_amd import _abi, device as tdev   # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(fns, reps):
    for fn in fns.values():                              # warm-up, on both buffers
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(3):                                   # interleaved passes
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    return {k: float(np.median(v)) for k, v in t.items()}, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="param", choices=["param", "band"])
    ap.add_argument("--S", type=int, default=1 << 17)
    ap.add_argument("--D", type=int, default=19)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--ncol", type=int, default=80001)
    ap.add_argument("--elem", type=int, default=8, choices=[4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantiles_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    turn = [0]
    stage = int(_abi.lib().trpl_quantiles_stage_rows())
    line = {"bench": "quantiles", "form": a.form, "device": torch.cuda.get_device_name(0), "reps": a.reps, "stage_rows": stage}
    if a.form == "param":
        S, D = a.S, a.D
        Vs = [torch.randn((D, S), dtype=torch.float64, device=dev, generator=g) for _ in range(2)]
        W = torch.rand(S, dtype=torch.float64, device=dev, generator=g) + 1e-3
        W /= W.sum()
        out = torch.empty((2, D), dtype=torch.float64, device=dev)
        q, rule = [0.025, 0.975], [_abi.Q_LAST_BELOW, _abi.Q_FIRST_ABOVE]

        def ours():
            turn[0] ^= 1
            tdev.weighted_quantiles_device(Vs[turn[0]], W, q, out, rule=rule)

        def yard():
            turn[0] ^= 1
            for d in range(D):
                tdev.credible_interval_device(Vs[turn[0]][d], W)

        ms, passes = measure({"quantiles": ours, "credible_interval_device_per_column": yard}, a.reps)
        line.update(S=S, D=D, K=2, streamed=S > stage, ms=ms, ms_passes=passes,
                    quantiles_over_yardstick=ms["quantiles"] / ms["credible_interval_device_per_column"])
    else:
        n, ncol = a.n, a.ncol
        dt = torch.float32 if a.elem == 4 else torch.float64
        pls = []
        for _ in range(2):                               # PL = 10^U(-12, 0): a decaying curve's range
            pl = torch.empty((n, ncol), dtype=dt, device=dev)
            pl.uniform_(-12.0, 0.0, generator=g)
            pl.mul_(float(np.log(10.0))).exp_()
            pls.append(pl)
        mag = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 6 - 3
        W = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 1e-3
        W /= W.sum()
        Ys = [torch.empty((ncol, n), dtype=torch.float64, device=dev) for _ in range(2)]
        Wq = torch.empty(n, dtype=torch.float64, device=dev)
        out = torch.empty((3, ncol), dtype=torch.float64, device=dev)
        state, ws = tdev.predictive_state(ncol), tdev.predictive_workspace(n, ncol, a.elem)
        tdev.predictive_init_device(state)
        q = [0.025, 0.5, 0.975]
        qt = torch.tensor(q, dtype=torch.float64, device=dev)

        def gather():
            turn[0] ^= 1
            tdev.predictive_gather_device(pls[turn[0]], W, Ys[turn[0]], Wq, mag=mag)

        def accumulate():
            turn[0] ^= 1
            tdev.predictive_accumulate_device(pls[turn[0]], W, state, ws, mag=mag)

        def select():
            turn[0] ^= 1
            tdev.weighted_quantiles_device(Ys[turn[0]], Wq, q, out)

        def yard():
            turn[0] ^= 1
            ys, order = torch.sort(Ys[turn[0]], dim=1)
            cs = torch.cumsum(Wq[order], dim=1)
            idx = torch.searchsorted(cs, (qt * cs[:, -1:]).expand(ncol, 3).contiguous(), right=True).clamp_(max=n - 1)
            return torch.gather(ys, 1, idx)

        gather(); gather()                               # both stores hold keys before a selection is timed
        ms, passes = measure({"gather": gather, "accumulate": accumulate, "select": select, "sort_cumsum_searchsorted": yard}, a.reps)
        line.update(n=n, ncol=ncol, elem_bytes=a.elem, K=3, streamed=n > stage, ms=ms, ms_passes=passes,
                    store_bytes=ncol * n * 8, gather_over_accumulate=ms["gather"] / ms["accumulate"],
                    select_over_yardstick=ms["select"] / ms["sort_cumsum_searchsorted"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
