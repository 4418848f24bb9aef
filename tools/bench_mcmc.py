"""The three kernels of the ensemble Metropolis sampler on resident tensors, in one process on one device.

    python tools/bench_mcmc.py [--chains 65536] [--A 10] [--n 256] [--reps 5] [--fold] [--tempered [--rungs 16]] [--hastings] [--subspace] [--autocov] [--evidence]
                               [--out profiles/mcmc_bench.jsonl] [--label parent]
    python tools/bench_mcmc.py --host-loop [--out ...] [--label ...]

propose:     mcmc_propose_device of `chains` chains in the reference's box (A = 10 active columns), with `chains` partners
             (differential evolution: two gathered partner rows per chain), and the random walk for comparison.
             --fold adds the differential-evolution propose with TRPL_MCMC_FOLD at the same shape, on chains of which half lie
             within 1e-3 of a face of the cube, so that the fmod path of the fold runs; the unfolded call of the same process is
             propose_de.
accept:      mcmc_accept_device of the same chains, about a third of the proposals accepted.
--tempered:  the four kernels of parallel tempering at the same rows, cut into --rungs rungs on geometric_ladder(1, 64, rungs):
             propose_rungs (partners from the chain's own rung), accept_rungs and levels_rungs (a temperature per rung, beside
             levels, the scalar call) and swap (parity 0).
--hastings:  the four Metropolis-Hastings kernels at the same rows and the same --rungs rungs, beside the three
             rung kernels they extend, in the same process: propose_stretch beside propose_rungs, accept_h beside accept_rungs,
             levels_h beside levels_rungs, and prior_term (two Gaussian columns, the rest flat).
--subspace:  the subspace differential-evolution proposal at the same rows and the same --rungs rungs, beside
             propose_rungs in the same process: propose_subspace with the defaults of mcmc.run (3 pairs, 3 classes, e_width 0.05), and
             propose_subspace_anchor at the setting where it is propose_rungs bit for bit (one pair, one class, e_width 0).  The line
             records the mean number of pairs and of moved coordinates, from which the extra partner rows follow.
chain_stats: mcmc_chain_stats_device over a history of n steps of chains * A columns (one half of a split-R-hat: n / 2 steps).
--autocov:   the two kernels of the effective sample size over the same chains * A columns, at L = 64 and L = 512 lags:
             mcmc_autocov_device over one half of a history (max(n / 2, L) steps, so L = 64 runs on chain_stats' own range) and
             mcmc_autocov_pool_device over its s.  The line records beside each time the two floors it is to be read against
             (DESIGN.md section 28): H read once per lag tile and s written once at 6.1 TB/s, and two fp64 instructions per term
             at 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.
--evidence:  the sums of the log-evidence estimates (mcmc_evidence_sums_device) over the kept LL of 16 rungs on
             geometric_ladder(1, 64, 16) in 16 blocks, at 1024 chains x 100 steps (the oldest 4 trimmed, as Tempered.log_evidence
             trims them) and at 65536 chains x 128 steps, each beside its floor: the range of LL read twice at 6.1 TB/s.
--host-loop: nothing of the above.  Wall-clock seconds per sweep of mcmc.run and of mcmc.run_tempered (4 rungs on geometric_ladder(1, 64, 4))
             through the host-buffer calls, with a numpy toy likelihood: 256 chains, a unit box of A = 3 columns, 200 sweeps -- what
             the sampler's own Python and staging cost per sweep, the likelihood being next to nothing.  One warm-up of 10 sweeps,
             then the median of 3 interleaved passes.
--label:     a word that goes into the line as "label", to tell two builds' lines apart.
Device events around `reps` back-to-back calls after a warm-up, median of 3 interleaved passes (tools/bench_quantiles.measure).
Appends one JSON line to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch         # noqa: E402
import trpl_amd      # noqa: E402,F401
from trpl_amd import device as tdev, refine, sampler as sm   # noqa: E402
from bench_quantiles import measure   # noqa: E402


def host_loop():
    import time
    import numpy as np
    from trpl_amd import mcmc
    C, A, sweeps, K = 256, 3, 200, 4
    lo, hi, lg = np.zeros(A), np.ones(A), np.zeros(A, dtype=np.int32)

    def loglik(X, cut_levels=None):
        return -np.sum((X - 0.5) ** 2, axis=1) / 0.02

    U0 = np.random.default_rng(1).uniform(0.3, 0.7, (C, A))
    X0, ladder = U0.copy(), mcmc.geometric_ladder(1.0, 64.0, K)
    LL0 = loglik(X0)
    runs = {"run": lambda n: mcmc.run(loglik, X0, LL0, lo, hi, lg, sweeps=n, seed=1, U0=U0),
            "run_tempered": lambda n: mcmc.run_tempered(loglik, X0, LL0, lo, hi, lg, ladder, sweeps=n, seed=1, U0=U0)}
    passes = {name: [] for name in runs}
    for name, f in runs.items():
        f(10)
    for _ in range(3):
        for name, f in runs.items():
            t0 = time.perf_counter()
            f(sweeps)
            passes[name].append((time.perf_counter() - t0) / sweeps)
    return {"bench": "mcmc_host_loop", "chains": C, "A": A, "sweeps": sweeps, "rungs": K,
            "s_per_sweep": {name: sorted(p)[1] for name, p in passes.items()}, "s_per_sweep_passes": passes}


def write(a, line):
    if a.label:
        line["label"] = a.label
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-loop", action="store_true")
    ap.add_argument("--label", default=None)
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--A", type=int, default=10)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fold", action="store_true")
    ap.add_argument("--tempered", action="store_true")
    ap.add_argument("--rungs", type=int, default=16)
    ap.add_argument("--hastings", action="store_true")
    ap.add_argument("--subspace", action="store_true")
    ap.add_argument("--autocov", action="store_true")
    ap.add_argument("--evidence", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_bench.jsonl"))
    a = ap.parse_args()
    if a.host_loop:
        return write(a, host_loop())
    dev = torch.device("cuda", 0)
    lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
    A = len(refine.active_columns(lo, hi))
    if A != a.A:
        raise SystemExit("the reference's box has %d active columns" % A)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    C, ncol = a.chains, len(lo)
    f64 = dict(dtype=torch.float64, device=dev)
    U = torch.rand((C, A), generator=g, **f64) * 0.5 + 0.25
    partners = torch.rand((C, A), generator=g, **f64) * 0.5 + 0.25
    Up, Xp = torch.empty((C, A), **f64), torch.empty((C, ncol), **f64)
    inside = torch.empty(C, dtype=torch.int32, device=dev)
    gamma = 2.38 / (2.0 * A) ** 0.5
    tdev.mcmc_propose_device(U, partners, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Up, Xp, inside)
    X = Xp.clone()
    LL = -torch.rand(C, generator=g, **f64)
    LLp = LL + 2.0 * torch.randn(C, generator=g, **f64) - 1.0
    accepted = torch.empty(C, dtype=torch.int32, device=dev)
    H = torch.rand((a.n, C * A), generator=g, **f64)
    mean, m2 = torch.empty(C * A, **f64), torch.empty(C * A, **f64)
    # accept overwrites its chains, so it runs on copies.  Every call decides alike: a chain that took its proposal stands on it at
    # the next call (d = 0: taken again), one that refused refuses again (the same uniform) -- the same reads and writes each time
    Ua, Xa, LLa = U.clone(), X.clone(), LL.clone()
    calls = {
        "propose_de": lambda: tdev.mcmc_propose_device(U, partners, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Up, Xp, inside),
        "propose_rw": lambda: tdev.mcmc_propose_device(U, None, gamma, 0.05, 0, 42, 0, lo, hi, lg, Up, Xp, inside),
        "accept": lambda: tdev.mcmc_accept_device(Ua, Xa, LLa, Up, Xp, LLp, inside, 1.0, 0, 42, 0, accepted),
        "chain_stats": lambda: tdev.mcmc_chain_stats_device(H, 0, a.n // 2, mean, m2)}
    if a.fold:
        # every second chain within 1e-3 of a face in every coordinate: its proposal leaves the cube and is folded.  Outputs of its
        # own, so that accept reads what propose_de wrote, as without --fold
        Uf = U.clone()
        near = torch.rand((C // 2, A), generator=g, **f64) * 1e-3
        Uf[::2] = torch.where(torch.rand((C // 2, A), generator=g, **f64) < 0.5, near, 1.0 - near)
        Upf, Xpf, codes = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside)
        flags = trpl_amd._abi.MCMC_FOLD
        calls["propose_de_fold"] = lambda: tdev.mcmc_propose_device(Uf, partners, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Upf, Xpf, codes,
                                                                     flags=flags)
    if a.tempered:
        # the same rows as --rungs rungs of chains / rungs each: the partners of a chain come from its rung's block, the temperature
        # from the ladder.  accept and swap overwrite their chains, so they run on copies; the share of pairs a swap call
        # exchanges differs from call to call (an exchanged pair stands the other way round at the next), swapped_share is the last's
        K = a.rungs
        if C % K or C // K < 2:
            raise SystemExit("--chains must be a multiple of --rungs, two chains per rung at least")
        ladder = trpl_amd.mcmc.geometric_ladder(1.0, 64.0, K)
        Upr, Xpr, insr = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside)
        Ur, Xr, LLr, accr = U.clone(), X.clone(), LL.clone(), torch.empty_like(accepted)
        Us, Xs, LLs, swapped = U.clone(), X.clone(), LL.clone(), torch.empty_like(accepted)
        level = torch.empty(C, **f64)
        calls["propose_rungs"] = lambda: tdev.mcmc_propose_rungs_device(U, partners, C // K, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Upr, Xpr, insr)
        calls["accept_rungs"] = lambda: tdev.mcmc_accept_rungs_device(Ur, Xr, LLr, Up, Xp, LLp, inside, ladder, 0, 42, 0, accr)
        calls["levels"] = lambda: tdev.mcmc_levels_device(LL, 1.0, 0, 42, 0, level)
        calls["levels_rungs"] = lambda: tdev.mcmc_levels_rungs_device(LL, ladder, 0, 42, 0, level)
        calls["swap"] = lambda: tdev.mcmc_swap_device(Us, Xs, LLs, ladder, 0, 0, 42, 0, swapped)
    if a.hastings:
        K = a.rungs
        if C % K or C // K < 2:
            raise SystemExit("--chains must be a multiple of --rungs, two chains per rung at least")
        ladder_h = trpl_amd.mcmc.geometric_ladder(1.0, 64.0, K)
        Uph, Xph, insh, zh, lnq = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside), torch.empty(C, **f64), torch.empty(C, **f64)
        Uh, Xh, LLh, acch = U.clone(), X.clone(), LL.clone(), torch.empty_like(accepted)
        Ug, Xg, LLg, accg = U.clone(), X.clone(), LL.clone(), torch.empty_like(accepted)
        hterm, level_h, level_g = torch.randn(C, generator=g, **f64), torch.empty(C, **f64), torch.empty(C, **f64)
        pm, psd = [0.5] * A, [0.1, 0.2] + [float("inf")] * (A - 2)
        if not a.tempered:                                       # the kernels they extend, unless --tempered has them already
            Upg, Xpg, insg = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside)
            calls["propose_rungs"] = lambda: tdev.mcmc_propose_rungs_device(U, partners, C // K, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Upg, Xpg, insg)
            calls["accept_rungs"] = lambda: tdev.mcmc_accept_rungs_device(Ug, Xg, LLg, Up, Xp, LLp, inside, ladder_h, 0, 42, 0, accg)
            calls["levels_rungs"] = lambda: tdev.mcmc_levels_rungs_device(LL, ladder_h, 0, 42, 0, level_g)
        calls["propose_stretch"] = lambda: tdev.mcmc_propose_stretch_device(U, partners, C // K, 2.0, 0, 42, 0, lo, hi, lg, Uph, Xph, insh, zh, lnq)
        calls["accept_h"] = lambda: tdev.mcmc_accept_h_device(Uh, Xh, LLh, Up, Xp, LLp, inside, hterm, ladder_h, 0, 42, 0, acch)
        calls["levels_h"] = lambda: tdev.mcmc_levels_h_device(LL, hterm, ladder_h, 0, 42, 0, level_h)
        calls["prior_term"] = lambda: tdev.mcmc_prior_term_device(U, Up, pm, psd, lnq, lnq)
    if a.subspace:
        K = a.rungs
        if C % K or C // K < 2:
            raise SystemExit("--chains must be a multiple of --rungs, two chains per rung at least")
        Ups, Xps, inss, mask, sel = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside), torch.empty_like(inside), torch.empty_like(inside)
        tab, one = trpl_amd.mcmc.subspace_gamma_table(3, A), [[gamma] * A]
        if not (a.tempered or a.hastings):                       # the kernel it extends, unless another switch has it already
            Upq, Xpq, insq = torch.empty_like(Up), torch.empty_like(Xp), torch.empty_like(inside)
            calls["propose_rungs"] = lambda: tdev.mcmc_propose_rungs_device(U, partners, C // K, gamma, 1e-3, 0, 42, 0, lo, hi, lg, Upq, Xpq, insq)
        calls["propose_subspace_anchor"] = lambda: tdev.mcmc_propose_subspace_device(U, partners, C // K, one, 1e-3, 0, 42, 0, lo, hi, lg, Ups, Xps,
                                                                                     inss, mask, sel, ncr=1, e_width=0.0)
        calls["propose_subspace"] = lambda: tdev.mcmc_propose_subspace_device(U, partners, C // K, tab, 1e-3, 0, 42, 0, lo, hi, lg, Ups, Xps, inss,
                                                                              mask, sel)
    floors = {}
    if a.autocov:
        tile, Q = trpl_amd._abi.lib().trpl_mcmc_autocov_tile(), C * A
        for L in (64, 512):
            m = max(a.n // 2, L)
            Hl = H if m <= a.n else torch.rand((m, Q), generator=g, **f64)
            mean_l, s_l, pooled_l = torch.empty(Q, **f64), torch.empty((L, Q), **f64), torch.empty((L, A), **f64)
            calls["autocov_L%d" % L] = lambda Hl=Hl, m=m, mean_l=mean_l, s_l=s_l: tdev.mcmc_autocov_device(Hl, 0, m, mean_l, s_l)
            calls["autocov_pool_L%d" % L] = lambda s_l=s_l, pooled_l=pooled_l: tdev.mcmc_autocov_pool_device(s_l, C, A, pooled_l)
            terms = Q * sum(m - l for l in range(L))
            tiles = (L + tile - 1) // tile
            floors["autocov_L%d" % L] = {"steps": m, "terms": terms, "fp64_floor_ms": 2.0 * terms / (256 * 4 * 16 * 2.4e9) * 1e3,
                                         "hbm_floor_ms": 8.0 * Q * (tiles * m + m + L) / 6.1e12 * 1e3}
            floors["autocov_pool_L%d" % L] = {"hbm_floor_ms": 8.0 * L * (Q + A) / 6.1e12 * 1e3}
    if a.evidence:
        Ke, Be = 16, 16
        ladder_e = trpl_amd.mcmc.geometric_ladder(1.0, 64.0, Ke)
        for Ce, ne in ((1024, 100), (1 << 16, 128)):
            t0e = ne % Be
            LLe = -10.0 * torch.rand((Ke, ne, Ce), generator=g, **f64)
            ext_e, sums_e = torch.empty((Ke, 2), **f64), torch.empty((Ke, Be, trpl_amd._abi.MCMC_EVIDENCE_SUMS), **f64)
            name = "evidence_C%d_n%d" % (Ce, ne)
            calls[name] = lambda LLe=LLe, t0e=t0e, ne=ne, ext_e=ext_e, sums_e=sums_e: tdev.mcmc_evidence_sums_device(LLe, ladder_e, t0e, ne, ext_e,
                                                                                                                   sums_e)
            floors[name] = {"rungs": Ke, "blocks": Be, "steps": ne - t0e, "hbm_floor_ms": 2.0 * 8.0 * Ke * (ne - t0e) * Ce / 6.1e12 * 1e3}
    ms, passes = measure(calls, a.reps)
    torch.cuda.synchronize()
    line = {"bench": "mcmc", "device": torch.cuda.get_device_name(0), "chains": C, "A": A, "ncol": ncol, "n": a.n, "reps": a.reps, "ms": ms,
            "ms_passes": passes, "inside_share": float(inside.double().mean().item()), "accepted_share": float(accepted.double().mean().item()),
            "chain_stats_bytes_per_second": 2.0 * 8.0 * (a.n // 2) * C * A / (ms["chain_stats"] * 1e-3)}
    if a.fold:
        line["folded_share"] = float((codes == 2).double().mean().item())
    if a.tempered:
        line.update(rungs=a.rungs, swapped_share=float(swapped.double().mean().item()))
    if a.hastings:
        line.update(rungs=a.rungs, hastings=True, stretch_inside_share=float(insh.double().mean().item()),
                    accepted_h_share=float(acch.double().mean().item()))
    if a.subspace:                                               # the last call of the measurement is propose_subspace: its mask and sel
        dsel = sum(((mask >> d) & 1).double().mean().item() for d in range(A))
        line.update(rungs=a.rungs, subspace=True, subspace_mean_pairs=float((sel & 0xFF).double().mean().item()), subspace_mean_dsel=float(dsel),
                    subspace_over_rungs=ms["propose_subspace"] / ms["propose_rungs"],
                    subspace_anchor_over_rungs=ms["propose_subspace_anchor"] / ms["propose_rungs"])
    if a.autocov:
        line.update(autocov_tile=tile, autocov_floors={k: v for k, v in floors.items() if k.startswith("autocov")})
    if a.evidence:
        line.update(evidence_floors={k: v for k, v in floors.items() if k.startswith("evidence")})
    return write(a, line)


if __name__ == "__main__":
    sys.exit(main())
