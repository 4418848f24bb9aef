"""The temperature scan against the loop it replaces, in one process on one device.

    python tools/bench_tf_scan.py [S] [D] [K] [--lr]     (defaults 2^17, 13, 64)

scan: one trpl_posterior_tf_scan_dev over K temperatures.  loop: K x (trpl_posterior_weights_dev + trpl_posterior_moments_dev),
the existing calls at the same temperatures (the yardstick of this same run).  Device events, the two passes interleaved,
median of 3 passes of `reps` calls each.  --lr adds a third interleaved row, one trpl_posterior_tf_scan_lr_dev (the scan with a
proposal log-ratio beside LL, uniform in [-3, 30]) at the same S, D, K: recorded as lr_ms and lr_over_scan, not gated (one more 8-byte
read per sample and phase, K maxima in place of one).  Appends one JSON line to profiles/tf_scan_bench.jsonl; exit status 1 when the scan
is slower than the loop."""
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
    with_lr = "--lr" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--lr"]
    S, D, K = (int(a) for a in (argv[:3] + ["131072", "13", "64"][len(argv[:3]):]))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    LL = -1e3 * torch.rand(S, dtype=torch.float64, device=dev, generator=g) ** 2
    V = torch.randn((D, S), dtype=torch.float64, device=dev, generator=g)
    tfs_h = np.geomspace(1e-2, 1e4, K)
    tfs = torch.from_numpy(tfs_h).to(dev)
    W = torch.empty_like(LL)
    ws_old = tdev.posterior_workspace(D)
    sums = torch.zeros(2 + D, dtype=torch.float64, device=dev)
    central = torch.zeros((D, D + 2), dtype=torch.float64, device=dev)
    ws = tdev.posterior_tf_scan_workspace(S, D, K)
    out = {n: torch.zeros((K, 4 if n == "stats" else D), dtype=torch.float64, device=dev) for n in ("stats", "mean", "var", "Q")}
    var_loop = torch.zeros((K, D), dtype=torch.float64, device=dev)

    def scan():
        tdev.posterior_tf_scan_device(LL, tfs, out["stats"], ws, V=V, mean=out["mean"], var=out["var"], Q=out["Q"])

    lnr = 33.0 * torch.rand(S, dtype=torch.float64, device=dev, generator=g) - 3.0
    zero = torch.zeros_like(LL)
    ws_lr = tdev.posterior_tf_scan_lr_workspace(S, D, K)
    out_lr = {n: torch.zeros((K, 6 if n == "stats" else D), dtype=torch.float64, device=dev) for n in ("stats", "mean", "var", "Q")}

    def scan_lr(ratio=lnr):
        tdev.posterior_tf_scan_lr_device(LL, ratio, tfs, out_lr["stats"], ws_lr, V=V, mean=out_lr["mean"], var=out_lr["var"], Q=out_lr["Q"])

    def loop(keep=False):
        for k in range(K):
            tdev.posterior_weights_device(LL, float(tfs_h[k]), W, ws_old)
            tdev.posterior_moments_device(V, W, sums, central, ws_old)
            if keep:                                     # (only in the untimed comparison: the timed loop is the two calls alone)
                var_loop[k] = torch.diagonal(central[:, :D]) / sums[0]

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    scan(); loop(keep=True)
    torch.cuda.synchronize()
    assert torch.equal(out["var"], var_loop), "the scan and the loop disagree"
    t_scan, t_loop, t_lr = [], [], []
    if with_lr:
        scan_lr(zero)
        torch.cuda.synchronize()
        assert torch.equal(out_lr["var"], out["var"]) and torch.equal(out_lr["Q"], out["Q"]), "a zero ratio does not give the scan's bits"
        scan_lr()
    for _ in range(3):                                   # interleaved passes
        t_scan.append(timed(scan, 20))
        if with_lr:
            t_lr.append(timed(scan_lr, 20))
        t_loop.append(timed(loop, 2))
    ms_scan, ms_loop = float(np.median(t_scan)), float(np.median(t_loop))
    # bytes a streaming implementation has to move: LL in every phase that forms weights (3) + the max phase, V twice
    scan_bytes = 8 * S * (4 + 2 * D)
    # the loop per temperature: weights = 2 reads of LL + write, read, write of W; moments = 2 x (W + D columns)
    loop_bytes = K * 8 * S * (5 + 2 * (1 + D))
    line = {"bench": "tf_scan", "S": S, "D": D, "K": K, "device": torch.cuda.get_device_name(0),
            "scan_ms": ms_scan, "loop_ms": ms_loop, "scan_ms_passes": t_scan, "loop_ms_passes": t_loop,
            "speedup": ms_loop / ms_scan,
            "scan_algorithmic_bytes": scan_bytes, "scan_TBps": scan_bytes / ms_scan / 1e9,
            "scan_fraction_of_peak": scan_bytes / ms_scan / 1e9 / PEAK_TBS,
            "loop_algorithmic_bytes": loop_bytes, "loop_TBps": loop_bytes / ms_loop / 1e9,
            "loop_fraction_of_peak": loop_bytes / ms_loop / 1e9 / PEAK_TBS}
    if with_lr:
        ms_lr = float(np.median(t_lr))
        lr_bytes = 8 * S * (8 + 2 * D)                   # LL and lnr in the four phases, V twice
        line.update({"lr_ms": ms_lr, "lr_ms_passes": t_lr, "lr_over_scan": ms_lr / ms_scan, "lr_algorithmic_bytes": lr_bytes,
                     "lr_TBps": lr_bytes / ms_lr / 1e9})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tf_scan_bench.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    if not ms_scan <= ms_loop:
        print("FAIL: the scan (%.3f ms) is slower than the loop (%.3f ms)" % (ms_scan, ms_loop))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
