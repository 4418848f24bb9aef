#!/usr/bin/env python3
"""Where do the paired kernel's wave slots stand idle?  A -DTRPL_SLOT_TIMELINE=1 build of the library has lane 0 of every wave
record, per block it processes, {block, 100 MHz clock at start, at end, HW_ID | XCC_ID << 32}; this tool builds that variant
into a scratch directory (or takes one with --lib), runs ONE pass of the bench batch in a child process under a time limit and
writes profiles/slot_timeline_<tag>.json: busy fraction per slot, the gaps between consecutive blocks of a SIMD, work and finish
time per XCD, the drain, and the average resident waves per SIMD to set beside the PMC figure.

    python tools/slot_timeline.py --build-only --lib tools/ab/timeline.so      # where hipcc is
    python tools/slot_timeline.py --lib tools/ab/timeline.so --tag persistent  # on the GPU
    python tools/slot_timeline.py --lib tools/ab/timeline.so --tag classic --classic    # one block per wave, grid = blocks

The stamps cost two clock reads and one 32-byte store per ~50 ms block; the build's run time is still not a benchmark figure."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bayesian-inference-trpl_amd")
sys.path.insert(0, ROOT)
TICK_NS = 10.0            # wall_clock64: 100 MHz


def build(dest):
    work = tempfile.mkdtemp(prefix="trpl_timeline_")
    try:
        os.makedirs(os.path.join(work, "pkg"))
        os.makedirs(os.path.join(work, "include"))
        shutil.copytree(os.path.join(PKG, "csrc"), os.path.join(work, "pkg", "csrc"), ignore=shutil.ignore_patterns("build*"))
        shutil.copy(os.path.join(PKG, "Makefile"), os.path.join(work, "pkg"))
        shutil.copy(os.path.join(ROOT, "include", "trpl.h"), os.path.join(work, "include"))
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(work, "pkg"), "libtrpl_hip.so",
                               "EXTRA_DEFS=-DTRPL_SLOT_TIMELINE=1"])
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        shutil.copy(os.path.join(work, "pkg", "libtrpl_hip.so"), dest)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def analyse(rec, resident_grid):
    """rec: (nblk, 4) uint64 records.  Slots are (SIMD, wave id); a SIMD is (XCC, SE, SH, CU, SIMD) of the id words."""
    blk, t0, t1, hw = (rec[:, i] for i in range(4))
    assert np.array_equal(blk, np.arange(len(rec), dtype=np.uint64)), "a block without a record"
    xcc = (hw >> np.uint64(32)) & np.uint64(0xF)
    hwid = hw & np.uint64(0xFFFFFFFF)
    wave = (hwid & np.uint64(0xF)).astype(np.int64)
    simd_bits = hwid & np.uint64(0x30 | 0xF00 | 0x1000 | 0xE000)          # SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 15:13
    simd_key = (xcc.astype(np.int64) << 16) | simd_bits.astype(np.int64)
    start, end = int(t0.min()), int(t1.max())
    span = end - start
    s0 = t0.astype(np.int64) - start
    s1 = t1.astype(np.int64) - start
    dur = s1 - s0
    simds = np.unique(simd_key)
    out = {"blocks": int(len(rec)), "kernel_ms": span * TICK_NS * 1e-6, "simds_seen": int(len(simds)),
           "block_ms": {"mean": float(dur.mean() * TICK_NS * 1e-6), "min": float(dur.min() * TICK_NS * 1e-6),
                        "max": float(dur.max() * TICK_NS * 1e-6)},
           "avg_resident_waves_per_simd": float(dur.sum() / (len(simds) * span)),
           "avg_resident_waves_per_simd_of_1024": float(dur.sum() / (1024 * span))}
    # per SIMD: busy wave-time / (2 x span), gaps between a block's end and the next start in the SIMD's two-deep occupancy
    busy, gaps, last_end = [], [], []
    order = np.lexsort((s0, simd_key))
    k_sorted, s0s, s1s = simd_key[order], s0[order], s1[order]
    bounds = np.flatnonzero(np.diff(k_sorted)) + 1
    for a, b in zip(np.r_[0, bounds], np.r_[bounds, len(order)]):
        st, en = s0s[a:b], s1s[a:b]
        busy.append(float((en - st).sum() / (2.0 * span)))
        last_end.append(int(en.max()))
        # the SIMD holds two waves: the k-th start refills the slot freed by the earliest end not yet refilled
        ends = np.sort(en)
        nfill = len(st) - 2
        if nfill > 0:
            gaps.extend((st[2:] - ends[:nfill]).tolist())
    busy = np.array(busy)
    gaps = np.array(gaps, dtype=np.int64) if gaps else np.zeros(1, dtype=np.int64)
    out["slot_busy_fraction"] = {"mean": float(busy.mean()), "min": float(busy.min()), "p05": float(np.percentile(busy, 5)),
                                 "median": float(np.median(busy)), "max": float(busy.max())}
    g_us = gaps * TICK_NS * 1e-3
    out["refill_gap_us"] = {"count": int(len(gaps)), "mean": float(g_us.mean()), "median": float(np.median(g_us)),
                            "p95": float(np.percentile(g_us, 95)), "p99": float(np.percentile(g_us, 99)), "max": float(g_us.max()),
                            "negative": int((gaps < 0).sum()),
                            "total_share_of_slot_time": float(np.clip(gaps, 0, None).sum() / (2.0 * len(simds) * span))}
    # drain: from the first SIMD slot going idle for good to the end of the kernel
    ends_sorted = np.sort(s1)[::-1]
    nslots = 2 * len(simds)
    first_idle = int(ends_sorted[min(nslots, len(ends_sorted)) - 1])       # the end of the block that leaves the first slot unfilled
    tail = np.clip(span - np.sort(s1)[-min(nslots, len(s1)):], 0, None)
    out["drain"] = {"ms": (span - first_idle) * TICK_NS * 1e-6, "share_of_kernel": float((span - first_idle) / span),
                    "idle_slot_time_share": float(tail.sum() / (nslots * span))}
    out["start_skew_us"] = float((np.sort(s0)[min(nslots, len(s0)) - 1]) * TICK_NS * 1e-3)
    per_xcd = {}
    for x in np.unique(xcc):
        m = xcc == x
        per_xcd[str(int(x))] = {"blocks": int(m.sum()), "wave_ms": float(dur[m].sum() * TICK_NS * 1e-6),
                                "simds": int(len(np.unique(simd_key[m]))), "finish_ms": float(s1[m].max() * TICK_NS * 1e-6)}
    out["per_xcd"] = per_xcd
    out["wave_ids_seen"] = sorted(int(w) for w in np.unique(wave))
    out["resident_grid"] = resident_grid
    return out


def child(a):
    import ctypes
    import torch
    import trpl_amd
    from trpl_amd import device as tdev
    wl = trpl_amd.workloads
    lib = trpl_amd._abi.lib()
    lib.trpl_debug_slot_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.trpl_debug_slot_timeline.restype = None
    dev = torch.device("cuda:0")
    L, T, S = 128, a.T, a.S
    ini, lens = wl.twothick(L) if a.workload == "twothick" else wl.power_scan(L)
    C = len(lens)
    Time = T * 0.025
    X = torch.from_numpy(np.ascontiguousarray(wl.samples(S))).to(dev)
    ini_d = torch.from_numpy(ini).to(dev)
    mark = torch.from_numpy((wl.MARKED_POINT * trpl_amd.UNIT_CONVERSIONS)[None, :-1].copy()).to(dev)
    obs = torch.empty((C, T + 1), dtype=torch.float64, device=dev)
    for c in range(C):
        pl = torch.empty((1, T + 1), dtype=torch.float64, device=dev)
        tdev.solve_pl_device(mark, lens[c], Time, L, T, ini_d[c].contiguous(), pl, flags=trpl_amd.FLAG_STRICT, tol=7)
        obs[c] = torch.log10(pl[0])
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    sse = torch.empty((C, S), dtype=torch.float64, device=dev)
    status = torch.empty((C, S), dtype=torch.int32, device=dev)
    iters = torch.empty((C, S), dtype=torch.int64, device=dev)
    flags = trpl_amd._abi.pin_variant(0, S * C, L, T)
    nblk = ((S + 1) // 2) * C
    rec = torch.zeros((nblk, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib.trpl_debug_slot_timeline(rec.data_ptr(), 1 if a.classic else 0)
    tdev.loglik_device(X, ini_d, lens, Time, L, T, obs, [T + 1] * C, P, sse, status, iters, flags=flags, tol=7)
    torch.cuda.synchronize()
    lib.trpl_debug_slot_timeline(None, 0)
    props = torch.cuda.get_device_properties(0)
    out = analyse(rec.cpu().numpy().view(np.uint64), 2 * 4 * props.multi_processor_count)
    out.update({"workload": a.workload, "S": S, "C": C, "T": T, "launch": "one block per wave" if a.classic else "persistent",
                "non_converged": int((status != 0).sum().item()), "library": os.environ.get("TRPL_LIBRARY", "")})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("kernel_ms", "avg_resident_waves_per_simd", "simds_seen", "slot_busy_fraction",
                                          "refill_gap_us", "drain", "start_skew_us")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the -DTRPL_SLOT_TIMELINE=1 library (default: build one into a scratch directory)")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--tag", default="run")
    ap.add_argument("--classic", action="store_true", help="keep the launch at one block per wave (grid = blocks)")
    ap.add_argument("--S", type=int, default=65536)
    ap.add_argument("--T", type=int, default=8000)
    ap.add_argument("--workload", default="power_scan", choices=["power_scan", "twothick"])
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "slot_timeline_%s.json" % a.tag)
    if a.child:
        return child(a)
    scratch = None
    if a.build_only:
        build(a.lib or os.path.join(ROOT, "tools", "ab", "timeline.so"))
        return 0
    if a.lib is None:
        scratch = tempfile.mkdtemp(prefix="trpl_timeline_lib_")
        a.lib = os.path.join(scratch, "libtrpl_timeline.so")
        build(a.lib)
    try:
        env = dict(os.environ, TRPL_LIBRARY=os.path.abspath(a.lib), TRPL_AUTOBUILD="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tag", a.tag, "--S", str(a.S), "--T", str(a.T),
               "--workload", a.workload, "--out", a.out] + (["--classic"] if a.classic else [])
        return subprocess.run(cmd, env=env, timeout=a.timeout).returncode
    finally:
        if scratch:
            shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
