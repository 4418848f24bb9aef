"""The instrument-response convolution (trpl_convolve_irf_dev) against its two floors, in one process on one device.

    python tools/bench_irf.py [--rows 65536] [--ncol 8001] [--taps 5,33,257,1024] [--route] [--bank] [--nuisance] [--out profiles/irf_bench.jsonl]

kernel:  one trpl_convolve_irf_dev over a [rows][ncol] PL matrix (ld = ncol: odd, rows only element-aligned) in fp64 and in fp32,
         per tap count K with k0 = K // 2: 3 warm-ups, then the median of 10 calls timed one by one with device events.  Beside
         the milliseconds: the HBM floor -- one read of the block and one write of the convolved block at the 8 TB/s peak -- and
         the fp64 floor -- two fp64 instructions per term (a product and an addition, no fused multiply-add by contract) at one
         64-wide fp64 instruction per 4 cycles and SIMD, 1024 SIMDs at 2.4 GHz -- and which of the two binds at that K.
--route: the resident route solve -> convolve -> likelihood at the default bench shape (Power_scan, 3 curves, L = 128, T = 8000,
         one block of 8192 samples) with a 33-tap Gaussian response, each of the three calls timed with device events per curve:
         the convolution's share of the route's seconds, and the route without it.
--bank:  trpl_loglik_irf_bank_dev beside the loop it replaces -- J x (trpl_convolve_irf_dev + trpl_loglik_moments_from_pl_dev) -- on
         the same [rows][ncol] matrix with dense on-grid observations (n_obs = ncol - k0), per K of --taps and J of --responses, both
         timed in this process as above.  Floors: the fp64 floor of the convolution at the observed columns, two instructions per
         term, times J; the HBM floor of ONE read of the block.  With --route also the resident route solve -> bank -> profile at
         the default bench shape with 33 taps and J = 16.  Lines go to profiles/irf_bank_bench.jsonl unless --out is given.
--nuisance: trpl_nuisance_reduce_dev over moments [3][J][rows] per J of --responses (default 8,32,256): FIXED + max, PROFILE + max and
         GRID (M = 16) + marginal, timed as above.  Floor: ONE read of the moments the shape needs (sse alone under FIXED) at the
         8 TB/s peak.  Beside FIXED + max the tail of irf.loglik_profile that it replaces, in wall-clock seconds in this process:
         the download of P (J, rows), its upload and trpl_irf_bank_profile_dev.  With --route also the resident route solve -> bank ->
         reduce at the default bench shape with J = 16: the reduction's share beside the solve.  Lines go to
         profiles/nuisance_bench.jsonl unless --out is given.
Appends one JSON line per measurement to --out."""
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

PEAK_BPS = 8.0e12
FP64_LANE_INSTR_PS = 256 * 4 * (64 / 4) * 2.4e9      # CUs x SIMDs x lanes per cycle x clock


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def bench_kernel(a, out):
    dev = torch.device("cuda", 0)
    rows, ncol = a.rows, a.ncol
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for dt in (torch.float64, torch.float32):
        elem = 8 if dt == torch.float64 else 4
        pl = torch.empty((rows, ncol), dtype=dt, device=dev)
        pl.uniform_(-12.0, 0.0, generator=g)
        pl.mul_(float(np.log(10.0))).exp_()                      # PL = 10^U(-12, 0): a decaying curve's range
        for K in a.taps:
            k0 = K // 2
            ncol_out = ncol - k0
            h = torch.from_numpy(np.random.default_rng(K).uniform(0.1, 1.0, K)).to(dev)
            cv = torch.empty((rows, ncol_out), dtype=dt, device=dev)
            for _ in range(3):
                tdev.convolve_irf_device(pl, h, k0, cv)
            torch.cuda.synchronize()
            ms = []
            for _ in range(10):
                e0, e1 = events()
                e0.record()
                tdev.convolve_irf_device(pl, h, k0, cv)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            nbytes = rows * (ncol + ncol_out) * elem
            terms = rows * ncol_out * K
            hbm_ms, fp64_ms = nbytes / PEAK_BPS * 1e3, 2 * terms / FP64_LANE_INSTR_PS * 1e3
            line = {"bench": "irf_kernel", "device": torch.cuda.get_device_name(0), "rows": rows, "ncol": ncol, "elem_bytes": elem, "K": K,
                    "k0": k0, "ms": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "hbm_floor_ms": hbm_ms,
                    "fp64_floor_ms": fp64_ms, "binding_floor": "hbm" if hbm_ms >= fp64_ms else "fp64",
                    "ms_over_binding_floor": med / max(hbm_ms, fp64_ms), "TBps": nbytes / med / 1e9}
            out(line)
        del pl, cv


def bench_route(a, out):
    dev = torch.device("cuda", 0)
    w = trpl_amd.workloads
    L, T, S = 128, 8000, a.samples
    Time = T * 0.025
    ini, lens = w.power_scan(L)
    X = w.samples(S)
    h, k0 = trpl_amd.irf.gaussian(0.188, Time / T, rel_cut=1e-6)
    X_d = torch.from_numpy(X).to(dev)
    mat, mag = X_d[:, :12].contiguous(), X_d[:, 12].contiguous()
    ini_d, h_d = torch.from_numpy(ini).to(dev), torch.from_numpy(h).to(dev)
    pl = torch.empty((S, T + 1), dtype=torch.float64, device=dev)
    cv = torch.empty((S, T + 1 - k0), dtype=torch.float64, device=dev)
    st = torch.zeros(S, dtype=torch.int32, device=dev)
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    obs = torch.zeros(T + 1 - k0, dtype=torch.float64, device=dev)
    runs = []
    for rep in range(1 + a.route_reps):                              # the first pass warms up
        t = {"solve": 0.0, "convolve": 0.0, "loglik": 0.0, "loglik_bare": 0.0}
        for c in range(3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            tdev.solve_pl_device(mat, lens[c], Time, L, T, ini_d[c].contiguous(), pl, status=st)
            ev[1].record()
            tdev.convolve_irf_device(pl, h_d, k0, cv)
            ev[2].record()
            tdev.loglik_from_pl_device(cv, obs, mag, P=P, status=st)
            ev[3].record()
            tdev.loglik_from_pl_device(pl, obs, mag, P=P, status=st)         # the route without the response reads the bare block
            ev[4].record()
            torch.cuda.synchronize()
            for k, (i, j) in zip(t, ((0, 1), (1, 2), (2, 3), (3, 4))):
                t[k] += ev[i].elapsed_time(ev[j]) / 1e3
        if rep:
            runs.append(t)
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    with_irf, without = med["solve"] + med["convolve"] + med["loglik"], med["solve"] + med["loglik_bare"]
    out({"bench": "irf_route", "device": torch.cuda.get_device_name(0), "workload": "Power_scan", "curves": 3, "L": L, "T": T, "samples": S,
         "K": int(len(h)), "k0": int(k0), "seconds": med, "route_with_irf_s": with_irf, "route_without_irf_s": without,
         "irf_share_of_route": med["convolve"] / with_irf, "reps": a.route_reps})


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = events()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def bench_bank(a, out):
    dev = torch.device("cuda", 0)
    rows, ncol = a.rows, a.ncol
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for dt in (torch.float64, torch.float32):
        elem = 8 if dt == torch.float64 else 4
        pl = torch.empty((rows, ncol), dtype=dt, device=dev)
        pl.uniform_(-12.0, 0.0, generator=g)
        pl.mul_(float(np.log(10.0))).exp_()
        mag = torch.zeros(rows, dtype=torch.float64, device=dev)
        for K in a.taps:
            k0 = K // 2
            n_obs = ncol - k0
            obs = torch.zeros(n_obs, dtype=torch.float64, device=dev)
            cv = torch.empty((rows, n_obs), dtype=dt, device=dev)
            for J in a.responses:
                H = torch.from_numpy(np.random.default_rng(K + J).uniform(0.1, 1.0, (J, K))).to(dev)
                sse = torch.empty((J, rows), dtype=torch.float64, device=dev)
                esum = torch.empty((J, rows), dtype=torch.float64, device=dev)

                def loop():
                    for j in range(J):
                        tdev.convolve_irf_device(pl, H[j], k0, cv)
                        tdev.loglik_moments_from_pl_device(cv, obs, mag, sse=sse[j], esum=esum[j])

                def bank():
                    tdev.loglik_irf_bank_device(pl, H, k0, obs, mag, sse, esum=esum)

                loop_ms, bank_ms = timed(loop), timed(bank)
                terms = rows * n_obs * K * J
                out({"bench": "irf_bank", "device": torch.cuda.get_device_name(0), "rows": rows, "ncol": ncol, "elem_bytes": elem, "K": K,
                     "k0": k0, "J": J, "n_obs": n_obs, "bank_ms": bank_ms[0], "bank_ms_min": bank_ms[1], "bank_ms_max": bank_ms[2],
                     "loop_ms": loop_ms[0], "loop_ms_min": loop_ms[1], "loop_ms_max": loop_ms[2], "loop_over_bank": loop_ms[0] / bank_ms[0],
                     "fp64_floor_ms": 2 * terms / FP64_LANE_INSTR_PS * 1e3, "hbm_floor_ms": rows * ncol * elem / PEAK_BPS * 1e3})
        del pl, cv


def bench_bank_route(a, out):
    dev = torch.device("cuda", 0)
    w = trpl_amd.workloads
    L, T, S, J = 128, 8000, a.samples, 16
    Time = T * 0.025
    dt = Time / T
    ini, lens = w.power_scan(L)
    X = w.samples(S)
    H, k0, _ = trpl_amd.irf.gaussian_bank([0.15, 0.188], np.linspace(-2 * dt, 2 * dt, 8), dt, rel_cut=1e-6)
    X_d = torch.from_numpy(X).to(dev)
    mat, mag = X_d[:, :12].contiguous(), X_d[:, 12].contiguous()
    ini_d, H_d = torch.from_numpy(ini).to(dev), torch.from_numpy(H).to(dev)
    pl = torch.empty((S, T + 1), dtype=torch.float64, device=dev)
    st = torch.zeros(S, dtype=torch.int32, device=dev)
    obs = torch.zeros(T + 1 - k0, dtype=torch.float64, device=dev)
    sse = torch.empty((3, J, S), dtype=torch.float64, device=dev)
    P = torch.zeros((J, S), dtype=torch.float64, device=dev)
    LL = torch.empty(S, dtype=torch.float64, device=dev)
    best = torch.empty(S, dtype=torch.int32, device=dev)
    runs = []
    for rep in range(1 + a.route_reps):
        t = {"solve": 0.0, "bank": 0.0, "profile": 0.0}
        P.zero_()
        for c in range(3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            tdev.solve_pl_device(mat, lens[c], Time, L, T, ini_d[c].contiguous(), pl, status=st)
            ev[1].record()
            tdev.loglik_irf_bank_device(pl, H_d, k0, obs, mag, sse[c], status=st)
            ev[2].record()
            torch.cuda.synchronize()
            P -= sse[c]
            t["solve"] += ev[0].elapsed_time(ev[1]) / 1e3
            t["bank"] += ev[1].elapsed_time(ev[2]) / 1e3
        e0, e1 = events()
        e0.record()
        tdev.irf_bank_profile_device(P, best, LL)
        e1.record()
        torch.cuda.synchronize()
        t["profile"] = e0.elapsed_time(e1) / 1e3
        if rep:
            runs.append(t)
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    total = sum(med.values())
    out({"bench": "irf_bank_route", "device": torch.cuda.get_device_name(0), "workload": "Power_scan", "curves": 3, "L": L, "T": T,
         "samples": S, "K": int(H.shape[1]), "k0": int(k0), "J": int(H.shape[0]), "seconds": med, "route_s": total,
         "bank_share_of_route": med["bank"] / total, "reps": a.route_reps})


def bench_nuisance(a, out):
    import time
    dev = torch.device("cuda", 0)
    S, C, M = a.rows, 3, 16
    wsum = [float(a.ncol)] * C
    offsets = np.linspace(-0.3, 0.3, M)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    P = torch.empty(S, dtype=torch.float64, device=dev)
    best = torch.empty(S, dtype=torch.int32, device=dev)
    bmag = torch.empty(S, dtype=torch.float64, device=dev)
    for J in a.responses:
        mean = torch.empty((C, J, S), dtype=torch.float64, device=dev).normal_(0.0, 0.1, generator=g)
        esum = mean * a.ncol
        sse = (mean * mean + 0.01) * a.ncol                           # moments of n_obs errors of about 0.1
        del mean
        lp = torch.full((J * M,), -float(np.log(J * M)), dtype=torch.float64, device=dev)
        shapes = (("fixed_max", dict(mag="fixed"), 1), ("profile_max", dict(mag="profile"), 2),
                  ("grid16_marginal", dict(mag=offsets, marginal=True, tf=10.0, log_prior=lp), 2))
        for name, kw, arrays in shapes:
            ms = timed(lambda: tdev.nuisance_reduce_device(sse, esum, wsum, P, best=best, best_mag=bmag, **kw))
            floor = arrays * C * J * S * 8 / PEAK_BPS * 1e3
            out({"bench": "nuisance_reduce", "device": torch.cuda.get_device_name(0), "shape": name, "S": S, "C": C, "J": J,
                 "M": M if name.startswith("grid") else 1, "ms": ms[0], "ms_min": ms[1], "ms_max": ms[2], "hbm_floor_ms": floor,
                 "ms_over_floor": ms[0] / floor})
        # the tail of irf.loglik_profile: P (J, S) comes down, is handed to the profile as a host array, goes up and is reduced
        Pb = torch.zeros((J, S), dtype=torch.float64, device=dev)
        for c in range(C):
            Pb -= sse[c]
        secs = []
        for _ in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = Pb.cpu().numpy()
            t1 = time.perf_counter()
            up = torch.from_numpy(host).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            tdev.irf_bank_profile_device(up, best, P)
            torch.cuda.synchronize()
            secs.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        med = [float(np.median([r[k] for r in secs[3:]])) for k in range(3)]
        out({"bench": "irf_profile_tail", "device": torch.cuda.get_device_name(0), "S": S, "J": J, "download_ms": med[0] * 1e3,
             "upload_ms": med[1] * 1e3, "profile_ms": med[2] * 1e3, "tail_ms": sum(med) * 1e3})
        del sse, esum, Pb


def bench_nuisance_route(a, out):
    dev = torch.device("cuda", 0)
    w = trpl_amd.workloads
    L, T, S = 128, 8000, a.samples
    Time = T * 0.025
    dt = Time / T
    ini, lens = w.power_scan(L)
    X = w.samples(S)
    H, k0, _ = trpl_amd.irf.gaussian_bank([0.15, 0.188], np.linspace(-2 * dt, 2 * dt, 8), dt, rel_cut=1e-6)
    J = H.shape[0]
    X_d = torch.from_numpy(X).to(dev)
    mat, mag = X_d[:, :12].contiguous(), X_d[:, 12].contiguous()
    ini_d, H_d = torch.from_numpy(ini).to(dev), torch.from_numpy(H).to(dev)
    pl = torch.empty((S, T + 1), dtype=torch.float64, device=dev)
    st = torch.zeros(S, dtype=torch.int32, device=dev)
    obs = torch.zeros(T + 1 - k0, dtype=torch.float64, device=dev)
    sse = torch.empty((3, J, S), dtype=torch.float64, device=dev)
    esum = torch.empty((3, J, S), dtype=torch.float64, device=dev)
    LL = torch.empty(S, dtype=torch.float64, device=dev)
    runs = []
    for rep in range(1 + a.route_reps):
        t = {"solve": 0.0, "bank": 0.0}
        for c in range(3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            tdev.solve_pl_device(mat, lens[c], Time, L, T, ini_d[c].contiguous(), pl, status=st)
            ev[1].record()
            tdev.loglik_irf_bank_device(pl, H_d, k0, obs, mag, sse[c], esum=esum[c], status=st)
            ev[2].record()
            torch.cuda.synchronize()
            t["solve"] += ev[0].elapsed_time(ev[1]) / 1e3
            t["bank"] += ev[1].elapsed_time(ev[2]) / 1e3
        for name, kw in (("reduce_fixed_max", dict()), ("reduce_profile_max", dict(mag="profile")),
                         ("reduce_grid16_marginal", dict(mag=np.linspace(-0.3, 0.3, 16), marginal=True, tf=10.0))):
            e0, e1 = events()
            e0.record()
            tdev.nuisance_reduce_device(sse, esum, [float(T + 1 - k0)] * 3, LL, **kw)
            e1.record()
            torch.cuda.synchronize()
            t[name] = e0.elapsed_time(e1) / 1e3
        if rep:
            runs.append(t)
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    out({"bench": "nuisance_route", "device": torch.cuda.get_device_name(0), "workload": "Power_scan", "curves": 3, "L": L, "T": T,
         "samples": S, "K": int(H.shape[1]), "k0": int(k0), "J": int(J), "seconds": med,
         "reduce_over_solve": {k: med[k] / med["solve"] for k in med if k.startswith("reduce")}, "reps": a.route_reps})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--ncol", type=int, default=8001)
    ap.add_argument("--taps", type=lambda s: [int(v) for v in s.split(",")], default=[5, 33, 257, 1024])
    ap.add_argument("--route", action="store_true")
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--route-reps", type=int, default=3)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--bank", action="store_true")
    ap.add_argument("--nuisance", action="store_true")
    ap.add_argument("--responses", type=lambda s: [int(v) for v in s.split(",")], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.responses is None:
        a.responses = [8, 32, 256] if a.nuisance else [1, 8, 32]
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "nuisance_bench.jsonl" if a.nuisance else "irf_bank_bench.jsonl" if a.bank else "irf_bench.jsonl")
    if a.bank and a.taps == [5, 33, 257, 1024]:
        a.taps = [5, 33, 257]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def out(line):
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)

    if a.nuisance:
        if not a.no_kernel:
            bench_nuisance(a, out)
        if a.route:
            bench_nuisance_route(a, out)
        return 0
    if a.bank:
        if not a.no_kernel:
            bench_bank(a, out)
        if a.route:
            bench_bank_route(a, out)
        return 0
    if not a.no_kernel:
        bench_kernel(a, out)
    if a.route:
        bench_route(a, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
