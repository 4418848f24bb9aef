"""The three refinement kernels on resident tensors, in one process on one device.

    python tools/bench_refine.py [--S 131072 262144] [--K 1024 4096] [--A 10] [--m 32] [--reps 5] [--oriented] [--out profiles/refine_bench.jsonl]

resample: refine_resample_device of S posterior-like weights (most of them exactly 0) for K parents.
draw:     refine_draw_device of K * m box children + S / 8 uniform ones in the reference's box (A = 10 active columns).
density:  refine_density_device of S samples against the K boxes: the hot kernel, S * K box tests, each left at its first failing
          dimension.  Reported with the mean number of boxes that hold a sample.
--oriented times the two kernels of the oriented proposals instead, at the same shapes (bench "refine_oriented"):
affine:        refine_affine_device of the S samples, Z = M (U - c) with the orientation of the same weights (16 A bytes per sample).
draw_oriented: refine_draw_oriented_device of the same children in boxes around the parents in z; reported with the share outside.
density_z:     refine_density_device on Z against the boxes in z, for comparison with the axis-parallel line.
Device events around `reps` back-to-back calls after a warm-up, median of 3 interleaved passes (tools/bench_quantiles.measure).
Appends one JSON line per (S, K) to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np   # noqa: E402
import torch         # noqa: E402
import trpl_amd      # noqa: E402,F401
from trpl_amd import device as tdev, refine, sampler as sm   # noqa: E402
from bench_quantiles import measure   # noqa: E402


def oriented(a, dev, S, K, A, U, W, idx, stats, lo, hi, lg):
    """One line of the oriented kernels at (S, K): the orientation of the weights W on the host, then the three device calls."""
    o = refine.orientation(U.cpu().numpy(), W.cpu().numpy(), S)
    Z = torch.empty((S, A), dtype=torch.float64, device=dev)
    tdev.refine_affine_device(U, o["M"], o["c"], Z)
    zc = Z[idx].contiguous()
    a_h, b_h, iv_h = refine.boxes_oriented(zc.cpu().numpy(), o["h"], o["logdet"])
    ad, bd, ivd = (torch.from_numpy(x).to(dev) for x in (a_h, b_h, iv_h))
    nu = S // 8
    total = nu + K * a.m
    Z2 = torch.empty((total, A), dtype=torch.float64, device=dev)
    U2 = torch.empty((total, A), dtype=torch.float64, device=dev)
    X2 = torch.empty((total, 13), dtype=torch.float64, device=dev)
    ins = torch.empty(total, dtype=torch.int32, device=dev)
    B = torch.empty(S, dtype=torch.float64, device=dev)
    ms, passes = measure({
        "affine": lambda: tdev.refine_affine_device(U, o["M"], o["c"], Z),
        "draw_oriented": lambda: tdev.refine_draw_oriented_device(zc, o["h"], o["L"], o["c"], a.m, nu, 42, 2, lo, hi, lg, Z2, U2, X2, ins),
        "density_z": lambda: tdev.refine_density_device(Z, ad, bd, ivd, B)}, a.reps)
    torch.cuda.synchronize()
    return {"bench": "refine_oriented", "device": torch.cuda.get_device_name(0), "S": S, "K": K, "A": A, "m": a.m, "children": total,
            "reps": a.reps, "ess": float(stats[2].item()), "lam": o["lam"], "h_z": float(o["h"][0]), "ms": ms, "ms_passes": passes,
            "outside_share": float(1.0 - ins.double().mean().item()), "mean_boxes_per_sample": float((B / float(iv_h[0])).mean().item()),
            "affine_bytes_per_second": 16.0 * A * S / (ms["affine"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[1 << 17, 1 << 18])
    ap.add_argument("--K", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--A", type=int, default=10)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--h", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oriented", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
    A = len(refine.active_columns(lo, hi))
    if A != a.A:
        raise SystemExit("the reference's box has %d active columns" % A)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for S in a.S:
        U = torch.rand((S, A), dtype=torch.float64, device=dev, generator=g)
        # a posterior-like weight vector: a Gaussian of deviation 0.1 about the centre, far below fp64 for most samples
        W = torch.exp(-0.5 * (((U - 0.5) / 0.1) ** 2).sum(1) * 40.0)
        ws = tdev.refine_workspace(S)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        for K in a.K:
            idx = torch.empty(K, dtype=torch.int64, device=dev)
            tdev.refine_resample_device(W, idx, ws, stats=stats)
            if a.oriented:
                line = oriented(a, dev, S, K, A, U, W, idx, stats, lo, hi, lg)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
                print(json.dumps(line))
                continue
            a_h, b_h, iv_h = refine.boxes(U[idx].cpu().numpy(), a.h)
            ad, bd, ivd = (torch.from_numpy(x).to(dev) for x in (a_h, b_h, iv_h))
            nu = S // 8
            total = nu + K * a.m
            U2 = torch.empty((total, A), dtype=torch.float64, device=dev)
            X2 = torch.empty((total, 13), dtype=torch.float64, device=dev)
            B = torch.empty(S, dtype=torch.float64, device=dev)
            ms, passes = measure({
                "resample": lambda: tdev.refine_resample_device(W, idx, ws, stats=stats),
                "draw": lambda: tdev.refine_draw_device(ad, bd, a.m, nu, 42, 2, lo, hi, lg, U2, X2),
                "density": lambda: tdev.refine_density_device(U, ad, bd, ivd, B)}, a.reps)
            torch.cuda.synchronize()
            vol = float(np.mean(1.0 / iv_h))
            line = {"bench": "refine", "device": torch.cuda.get_device_name(0), "S": S, "K": K, "A": A, "m": a.m, "h": a.h, "children": total,
                    "reps": a.reps, "nonzero_weights": int((W > 0).sum().item()), "ess": float(stats[2].item()), "ms": ms, "ms_passes": passes,
                    "mean_boxes_per_sample": float((B * vol).mean().item()),
                    "density_box_tests_per_second": S * K / (ms["density"] * 1e-3)}
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
