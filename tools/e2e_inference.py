"""End-to-end on one GPU, everything device-resident: draw the parameter box (trpl_sample_box_dev), solve
and score every sample against observations synthesised at the reference's marked point
(Visualization/config.txt:57-68) with the fused kernel (trpl_loglik_dev), then the posterior core
(weights, moments, marginals).  Prints one JSON line.  Usage: python tools/e2e_inference.py [S] [T] [c] [--find-tf] [--predictive [--quantiles]] [--corner] [--refine [--rounds N] [--target-ess N] [--oriented [--shrink x]]] [--mcmc [--chains C] [--sweeps N] [--rw x] [--stretch [a]] [--subspace [--pairs n] [--ncr n] [--adapt-cr]] [--prior NAME=CENTER:WIDTH ...] [--fold] [--early-reject [sample]] [--tempered K [--tf-hot x] [--evidence]]] [--irf FWHM_NS [--irf-shifts LO:HI:N] [--irf-widths LO:HI:N] [--irf-reduce max|marginal] [--irf-mag fixed|profile]]
--find-tf adds, between likelihood and posterior, the temperature of largest uncertainty of every free parameter
(posterior.calc_max_uncertainty, utils.py:128-133, on the device temperature scan) as "max_uncertainty" in the output;
without it the output is unchanged.
--predictive adds, after the posterior, the posterior-predictive PL band of every curve (predictive.posterior_predictive: the
samples with a weight > 0 are re-solved and reduced on the device) as "predictive" -- mean, sqrt(var), lo, hi of log10 PL per
time column, the number of samples used, and the rms distance of the mean to the synthetic observations in units of
sqrt(var) -- and seconds["predictive"]; without it the output is unchanged.
--quantiles (with --predictive) adds the 2.5 % / 50 % / 97.5 % weighted quantiles of log10 PL per time column ("q2.5", "median",
"q97.5") and "inside_band", the share of the synthetic observations that lie inside [q2.5, q97.5].
--corner adds, at the end, the corner of the run (posterior.corner: the ten free parameters and five secondary ones -- tau_eff,
tau_rad, Sf+Sb, mu', taun+taup; epsilon = 1 / lambda is one number in this box, which fixes lambda -- 96 bins,
limits = the sampled box, every 1-D and 2-D marginal in one device call) as "corner": kept, the device seconds, and the mode of
every 1-D marginal -- and seconds["corner"], the call with its copies; without it the output is unchanged.
--refine [--rounds N] adds, at the end, N (default 1) refinement generations (trpl_amd.refine.run: parents resampled from the
posterior, box-kernel children, the fused likelihood on them, deterministic-mixture weights of the union) as "refine": the
effective sample size after every generation, the share of each generation's children with a weight > 0, the plain sum of the
union's weights over the samples with a finite likelihood, and the numbers of NaN weights and of NaN in LLc among those
samples -- and seconds["refine"]; without it the output is unchanged.
--target-ess N (with --refine) builds every generation's proposal at the lowest temperature at which the union so far has an
effective sample size of N (refine.run(target_ess=N): the temperature ladder, through the log-ratio scan) and adds "target_ess",
"tf_per_generation" and "ess_at_tf" (the union's effective sample size at the final temperature after each generation) to "refine";
tf per generation and the final effective sample size are printed.
--oriented (with --refine) draws every generation in boxes that are axis-parallel in the whitened coordinates of the union so far
(refine.run(oriented=True): DESIGN.md section 22) and adds "oriented", "outside_share_of_children" (the children that left the prior
box: never solved, weight 0) and "shrinkage_per_generation" to "refine"; --shrink x fixes the covariance shrinkage instead of
(A + 1) / ESS.
--find-tf with --refine also searches the temperature of largest uncertainty over the refined union, its proposal log-ratio kept
beside the likelihoods (posterior.calc_max_uncertainty(log_ratio=)), as refine["max_uncertainty"].
--mcmc [--chains C] [--sweeps N] adds, at the end, an ensemble Metropolis run on the fused likelihood (trpl_amd.mcmc: DESIGN.md section
23): C chains (default 1024) started from the importance run (mcmc.start) advance N sweeps (default 200) by differential-evolution
proposals at the run's temperature; the second half of the sweeps is kept.  "mcmc" holds the acceptance share, the share of
proposals that left the prior box, split-R-hat of every free parameter and its 2.5 / 50 / 97.5 % values from the chain beside
those of the importance run, which are printed; seconds["mcmc"].  --rw x uses a random walk of half-width x (unit coordinates)
instead.  --fold reflects a proposal that leaves the prior box back at its faces (mcmc.run(bounds="fold"): DESIGN.md section 25),
so that every proposal is solved; "mcmc" then gains "bounds" and "folded", the share of proposals that were reflected.  Without
--mcmc the output is unchanged, and so is "mcmc" without --fold.  "mcmc" also holds "ess": per free parameter the effective sample
size of the kept sweeps (Chains.ess: DESIGN.md section 28), the autocorrelation time tau in sweeps, whether the lags truncated the
sum (the ESS is then an upper bound) and the Monte-Carlo error of the mean in unit coordinates, printed beside R-hat.
--early-reject (with --mcmc) stops solving a proposal once its rejection is certain (mcmc.run(early_reject=True): DESIGN.md section
26; the chain is the same, bit for bit) and adds "early_reject" to "mcmc": the share of solved proposals that were cut and the
system-timesteps solved.  With or without it "mcmc" holds "system_timesteps", the solver iterations summed over every proposal, and
the same numbers are printed.  --early-reject sample spends each proposal's level as a budget across its curves instead
(mcmc.run(early_reject="sample"), trpl_loglik_cut_budget with one curve per launch; --curves-per-launch g for another grouping).
--tempered K (with --mcmc; composes with --fold and --early-reject) runs parallel tempering instead (mcmc.run_tempered: DESIGN.md section
27): K rungs of C chains each on mcmc.geometric_ladder(tf, tf_hot, K), every half-sweep still one call of the fused likelihood.
--tf-hot x sets the hottest temperature; the default is the temperature at which the importance run reaches an effective sample
size of 64 (posterior.tf_for_ess).  "mcmc" is the cold rung's, as without the flag; "tempered" beside it holds the ladder and, per
rung, acceptance and worst R-hat, the swap rates and the seconds, which are printed.
--evidence (with --tempered) adds the log-evidence estimates of the run (Tempered.log_evidence: DESIGN.md section 34): the
differences ln Z(tf) - ln Z(tf_hot) by stepping-stone sampling from the hotter and from the colder rung of each pair and by
thermodynamic integration, with their block-jackknife errors and the smallest term_ess, the base ln Z(tf_hot) of the importance run
(posterior.log_evidence at the hottest rung; with --prior its log-ratio is minus the sampler's unnormalised log prior) and the
absolute ln Z(tf) of each estimator, under "tempered" as "evidence" and printed side by side.
--stretch [a] (with --mcmc; not with --rw or --fold) proposes by the affine-invariant stretch move instead (mcmc.run(kind="stretch",
stretch_a=a), a defaulting to 2: DESIGN.md section 30).  --prior NAME=CENTER:WIDTH (with --mcmc; repeatable) puts a Gaussian prior on
the free parameter NAME (a name of sampler.PARAM_NAMES): CENTER in the units of the search box, WIDTH one standard deviation in the
same units on a linear parameter and in decades on a logarithmic one (mcmc.gaussian_prior).  "mcmc" then gains "stretch_a" and
"prior"; both compose with --early-reject and --tempered.
--subspace [--pairs n] [--ncr n] [--adapt-cr] (with --mcmc; not with --rw or --stretch) proposes by DREAM's subspace move instead
(mcmc.run(kind="subspace", pairs=n, ncr=n, adapt_cr=...): DESIGN.md section 33); it composes with --fold, --early-reject and --tempered.
"mcmc" then gains "subspace": pairs, ncr, the crossover shares pcr of the kept sweeps and mean_dsel, the mean number of coordinates
a proposal moved.
--irf FWHM_NS adds, at the end, the same importance run with the instrument response in the model (trpl_amd.irf: DESIGN.md section
35): a Gaussian response of that full width at half maximum on the run's time step (irf.gaussian), the observations the marked
point's curves convolved with it (what the detector would have recorded), every sample scored by irf.loglik (solve, convolve,
likelihood on the resident PL block).  "irf" holds the taps, the effective sample size and the 2.5 / 50 / 97.5 % values of every
free parameter beside those of the run without the response, which are printed -- recorded, not gated -- and seconds["irf"].
--irf-shifts LO:HI:N (ns) and --irf-widths LO:HI:N (ns; default: the one width of --irf) add the profile over a bank of responses
(irf.gaussian_bank, irf.loglik_profile: DESIGN.md section 36): the observations are the marked point's curves convolved with a
response of the bank that is NOT its centre (three quarters along each axis), every sample is scored by the profile and, beside it,
by irf.loglik with the response fixed at the bank's centre.  "irf_bank" holds the posterior-weighted distribution of the best
response, the effective sample sizes and the intervals of both runs, which are printed -- recorded, not gated.
--irf-reduce max|marginal and --irf-mag fixed|profile (beside --irf-shifts / --irf-widths; defaults max and fixed, the run above
unchanged) score every sample by irf.loglik_nuisance instead: the maximum or, at the run's tf and under the
uniform prior, the marginal over the bank, with the magnitude offset as it is or profiled per response.  The same lines are printed
for the chosen reduction; "irf_bank" also holds "reduce", "mag" and the posterior-weighted mean of the best offset.
"""
import json
import sys
import time

sys.path.insert(0, ".")
FIND_TF = "--find-tf" in sys.argv
PREDICTIVE = "--predictive" in sys.argv
QUANTILES = "--quantiles" in sys.argv
CORNER = "--corner" in sys.argv
REFINE = "--refine" in sys.argv
ROUNDS = 1
if "--rounds" in sys.argv:
    k = sys.argv.index("--rounds")
    ROUNDS = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
TARGET_ESS = None
if "--target-ess" in sys.argv:
    k = sys.argv.index("--target-ess")
    TARGET_ESS = float(sys.argv[k + 1])
    del sys.argv[k:k + 2]
ORIENTED = "--oriented" in sys.argv
SHRINK = None
if "--shrink" in sys.argv:
    k = sys.argv.index("--shrink")
    SHRINK = float(sys.argv[k + 1])
    del sys.argv[k:k + 2]
MCMC = "--mcmc" in sys.argv
FOLD = "--fold" in sys.argv
EVIDENCE = "--evidence" in sys.argv
EARLY = "--early-reject" in sys.argv
if EARLY and sys.argv.index("--early-reject") + 1 < len(sys.argv) and sys.argv[sys.argv.index("--early-reject") + 1] == "sample":
    del sys.argv[sys.argv.index("--early-reject") + 1]
    EARLY = "sample"
CURVES_PER_LAUNCH = 1
if "--curves-per-launch" in sys.argv:
    k = sys.argv.index("--curves-per-launch")
    CURVES_PER_LAUNCH = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
CHAINS, SWEEPS, RW, TEMPERED, TF_HOT = 1024, 200, None, 0, None
for flag, conv in (("--chains", int), ("--sweeps", int), ("--rw", float), ("--tempered", int), ("--tf-hot", float)):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        value = conv(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        if flag == "--chains":
            CHAINS = value
        elif flag == "--sweeps":
            SWEEPS = value
        elif flag == "--tempered":
            TEMPERED = value
        elif flag == "--tf-hot":
            TF_HOT = value
        else:
            RW = value
STRETCH = None
if "--stretch" in sys.argv:
    k = sys.argv.index("--stretch")
    try:
        STRETCH = float(sys.argv[k + 1])
        del sys.argv[k:k + 2]
    except (IndexError, ValueError):
        STRETCH = 2.0
        del sys.argv[k]
SUBSPACE = "--subspace" in sys.argv
ADAPT_CR = "--adapt-cr" in sys.argv
PAIRS, NCR = 3, 3
for flag in ("--pairs", "--ncr"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        PAIRS, NCR = (int(sys.argv[k + 1]), NCR) if flag == "--pairs" else (PAIRS, int(sys.argv[k + 1]))
        del sys.argv[k:k + 2]
IRF_FWHM = None
if "--irf" in sys.argv:
    k = sys.argv.index("--irf")
    IRF_FWHM = float(sys.argv[k + 1])
    del sys.argv[k:k + 2]
IRF_SHIFTS = IRF_WIDTHS = None
for flag in ("--irf-shifts", "--irf-widths"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        lo_, hi_, n_ = sys.argv[k + 1].split(":")
        grid_ = [float(lo_) + (float(hi_) - float(lo_)) * i / max(int(n_) - 1, 1) for i in range(int(n_))]
        IRF_SHIFTS, IRF_WIDTHS = (grid_, IRF_WIDTHS) if flag == "--irf-shifts" else (IRF_SHIFTS, grid_)
        del sys.argv[k:k + 2]
IRF_REDUCE, IRF_MAG = "max", "fixed"
for flag, allowed in (("--irf-reduce", ("max", "marginal")), ("--irf-mag", ("fixed", "profile"))):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        if sys.argv[k + 1] not in allowed:
            sys.exit("%s takes %s" % (flag, " or ".join(allowed)))
        IRF_REDUCE, IRF_MAG = (sys.argv[k + 1], IRF_MAG) if flag == "--irf-reduce" else (IRF_REDUCE, sys.argv[k + 1])
        del sys.argv[k:k + 2]
if (IRF_REDUCE, IRF_MAG) != ("max", "fixed") and IRF_SHIFTS is None and IRF_WIDTHS is None:
    sys.exit("--irf-reduce / --irf-mag need --irf-shifts or --irf-widths")
if (IRF_SHIFTS is not None or IRF_WIDTHS is not None) and IRF_FWHM is None:
    sys.exit("--irf-shifts / --irf-widths need --irf FWHM_NS")
PRIORS = {}
while "--prior" in sys.argv:
    k = sys.argv.index("--prior")
    name, spec = sys.argv[k + 1].split("=")
    PRIORS[name] = tuple(float(v) for v in spec.split(":"))
    del sys.argv[k:k + 2]
sys.argv = [a for a in sys.argv if a not in ("--find-tf", "--predictive", "--quantiles", "--corner", "--refine", "--oriented", "--mcmc", "--fold", "--early-reject", "--subspace", "--adapt-cr", "--evidence")]
import numpy as np
import torch
import trpl_amd
from trpl_amd import device as tdev, sampler as sm, workloads as wl

S = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = int(sys.argv[2]) if len(sys.argv) > 2 else 8000
c_val = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0e-4
L, dt = 128, 0.025
dev = torch.device("cuda", 0)
ini, lens = wl.power_scan(L)
C = len(lens)
lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


t0 = sync()
X = torch.empty((S, 13), dtype=torch.float64, device=dev)
tdev.sample_box_device(X, lo, hi, lg, seed=42)
t1 = sync()
ini_d = torch.from_numpy(ini).to(dev)
mark = torch.from_numpy((wl.MARKED_POINT * sm.UNIT_CONVERSIONS)[None, :-1].copy()).to(dev)
obs = torch.empty((C, T + 1), dtype=torch.float64, device=dev)
for c in range(C):
    pl = torch.empty((1, T + 1), dtype=torch.float64, device=dev)
    tdev.solve_pl_device(mark, lens[c], T * dt, L, T, ini_d[c].contiguous(), pl, flags=trpl_amd.FLAG_STRICT)
    obs[c] = torch.log10(pl[0])
P = torch.zeros(S, dtype=torch.float64, device=dev)
sse = torch.empty((C, S), dtype=torch.float64, device=dev)
status = torch.empty((C, S), dtype=torch.int32, device=dev)
iters = torch.empty((C, S), dtype=torch.int64, device=dev)
t2 = sync()
tdev.loglik_device(X, ini_d, lens, T * dt, L, T, obs, [T + 1] * C, P, sse, status, iters)
t3 = sync()
# posterior: temper by n_obs * c (marginalization_visual.py:589), weights, moments of the free parameters
n_obs = C * (T + 1)
cols = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
names = [sm.PARAM_NAMES[i] for i in cols]
Xc = X / torch.from_numpy(sm.UNIT_CONVERSIONS).to(dev)                    # back to the GUI's units
V = torch.stack([torch.log10(Xc[:, i]) if lg[i] else Xc[:, i] for i in cols]).contiguous()
W = torch.empty_like(P)
ws = tdev.posterior_workspace(len(cols))
sums = torch.zeros(2 + len(cols), dtype=torch.float64, device=dev)
central = torch.zeros((len(cols), len(cols) + 2), dtype=torch.float64, device=dev)
h = torch.zeros(32, dtype=torch.float64, device=dev)
t4 = sync()
tdev.posterior_weights_device(P, n_obs * c_val, W, ws)
tdev.posterior_moments_device(V, W, sums, central, ws)
tdev.posterior_hist_device(V[names.index("taun")], W, 1.0, 1000.0, h)
t5 = sync()
s, cen = sums.cpu().numpy(), central.cpu().numpy()
mean = s[2:] / s[0]
std = np.sqrt(np.diag(cen[:, :len(cols)]) / s[0])
truth = np.array([np.log10(wl.MARKED_POINT[i]) if lg[i] else wl.MARKED_POINT[i] for i in cols])
best = int(torch.argmax(P).item())
out = {
    "workload": "power_scan x %d samples, T=%d, observations synthesised at the marked point, c=%g" % (S, T, c_val),
    "seconds": {"sampler": t1 - t0, "solve_and_likelihood": t3 - t2, "posterior": t5 - t4},
    "nonconverged_systems": int((status != 0).sum().item()),
    "effective_sample_size": float(1.0 / s[1]),
    "max_loglik": float(P[best].item()), "median_loglik": float(torch.median(P).item()),
    "parameters": {n: {"truth": float(tr), "posterior_mean": float(m), "posterior_std": float(sd),
                       "best_sample": float(V[k, best].item())}
                   for k, (n, tr, m, sd) in enumerate(zip(names, truth, mean, std))},
    "taun_marginal_32_bins_1_to_1000": [float(v) for v in (h / h.sum()).cpu().numpy()],
}
if FIND_TF:
    from trpl_amd import posterior
    t6 = sync()
    info = {}
    unc = posterior.calc_max_uncertainty(dict(zip(names, V.cpu().numpy())), P.cpu().numpy(), n_obs, info=info)
    out["seconds"]["find_tf"] = sync() - t6
    out["max_uncertainty"] = {n: {"tf": tf, "Q": q, "at_edge": bool(info["at_edge"][n])} for n, (tf, q) in unc.items()}
    out["find_tf_scans"] = {"rounds": info["scans"], "device_scans": info["device_scans"]}
if PREDICTIVE:
    from trpl_amd import predictive
    t7 = sync()
    bands = predictive.posterior_predictive(X.cpu().numpy(), W.cpu().numpy(), ini, [list(lens), T * dt, L, T, 1],
                                            quantiles=(0.025, 0.5, 0.975) if QUANTILES else None)
    out["seconds"]["predictive"] = sync() - t7
    obs_h = obs.cpu().numpy()
    out["predictive"] = []
    for c, b in enumerate(bands):
        sd = np.sqrt(b["var"])
        with np.errstate(divide="ignore", invalid="ignore"):
            z = (b["mean"] - obs_h[c]) / sd
        z = z[np.isfinite(z)]                    # (a column on which every used sample agrees has no width)
        out["predictive"].append({"n_used": b["n_used"], "n_flagged": b["n_flagged"],
                                  "rms_distance_in_sigma": float(np.sqrt(np.mean(z * z))) if z.size else None,
                                  "times": b["times"].tolist(), "mean": b["mean"].tolist(), "std": sd.tolist(),
                                  "lo": b["lo"].tolist(), "hi": b["hi"].tolist()})
        if QUANTILES:
            lo_q, med, hi_q = b["quantile"]
            with np.errstate(invalid="ignore"):
                inside = (obs_h[c] >= lo_q) & (obs_h[c] <= hi_q)
            out["predictive"][-1].update({"q2.5": lo_q.tolist(), "median": med.tolist(), "q97.5": hi_q.tolist(),
                                          "inside_band": float(np.mean(inside))})
if CORNER:
    from trpl_amd import posterior
    t8 = sync()
    Xu, LLh = Xc.cpu().numpy(), P.cpu().numpy()
    enabled = names + ["tau_eff", "tau_rad", "Sf+Sb", "mu'", "taun+taup"]
    logged = [n for n, i in zip(names, cols) if lg[i]] + ["tau_eff", "tau_rad"]
    Vh = posterior.columns(Xu, enabled, thickness=float(lens[0]), do_log=logged)
    fin = np.where(np.isfinite(Vh), Vh, np.nan)
    limits = {n: (float(np.nanmin(fin[d])), float(np.nanmax(fin[d]))) for d, n in enumerate(enabled)}   # plotutils.py:25-33
    limits = {n: (a, b) if b > a else (a - 1.0, b + 1.0) for n, (a, b) in limits.items()}
    cinfo = {}
    cr = posterior.corner(Xu, LLh, enabled, limits, bin_count=96, tf=n_obs * c_val, thickness=float(lens[0]), do_log=logged, info=cinfo)
    out["seconds"]["corner"] = sync() - t8
    out["corner"] = {"kept": cr["kept"], "columns": len(enabled), "histograms": len(cr["h_1D"]) + len(cr["h_2D"]),
                     "device_seconds": cinfo["seconds"],
                     "mode": {n: float(0.5 * (e[int(np.argmax(d))] + e[int(np.argmax(d)) + 1])) for n, (d, e) in cr["h_1D"].items()}}
    print("corner: kept %d of %d, %d histograms in %.3f ms on the device" % (cr["kept"], S, out["corner"]["histograms"],
                                                                           1e3 * cinfo["seconds"]), file=sys.stderr)
if REFINE:
    from trpl_amd import posterior, refine
    t9 = sync()

    def fused(X2):                                               # the fused likelihood of a generation's children
        n = X2.shape[0]
        Xd = torch.from_numpy(np.ascontiguousarray(X2)).to(dev)
        P2 = torch.zeros(n, dtype=torch.float64, device=dev)
        tdev.loglik_device(Xd, ini_d, lens, T * dt, L, T, obs, [T + 1] * C, P2, torch.empty((C, n), dtype=torch.float64, device=dev))
        return P2.cpu().numpy()

    tf = n_obs * c_val
    K = max(1, min(1024, S // 32))
    rinfo = {}
    pop = refine.run(fused, X.cpu().numpy(), P.cpu().numpy(), lo, hi, lg, rounds=ROUNDS, K=K, m=28, n_uniform=max(1, S // 8), tf=tf,
                     seed=42, info=rinfo, target_ess=TARGET_ESS, **({"oriented": True, "shrink": SHRINK} if ORIENTED else {}))
    X_all, LLc = pop.corrected(tf)
    W_all = posterior.weights(LLc, tf)
    LL_all = np.concatenate(pop.LL)
    out["seconds"]["refine"] = sync() - t9
    out["refine"] = {"rounds": ROUNDS, "parents": K, "children_per_parent": 28, "n_uniform": max(1, S // 8), "samples": int(X_all.shape[0]),
                     "ess_per_generation": rinfo["ess"], "nonzero_share_of_children": rinfo["nonzero"],
                     "weight_sum": float(np.sum(W_all[np.isfinite(LL_all)])), "nan_weights_from_finite_ll": int(np.sum(np.isnan(W_all) & np.isfinite(LL_all))),
                     "nan_llc_from_finite_ll": int(np.sum(np.isnan(LLc) & np.isfinite(LL_all)))}
    print("refine: effective sample size per generation %s, share of children with a weight > 0 %s"
          % (["%.2f" % e for e in rinfo["ess"]], ["%.4f" % f for f in rinfo["nonzero"]]), file=sys.stderr)
    if ORIENTED:
        out["refine"].update(oriented=True, outside_share_of_children=rinfo["outside"], shrinkage_per_generation=rinfo["lam"])
        print("refine: oriented, share of children outside the prior box %s, shrinkage %s"
              % (["%.4f" % f for f in rinfo["outside"]], ["%.3f" % f for f in rinfo["lam"]]), file=sys.stderr)
    if TARGET_ESS is not None:
        out["refine"].update(target_ess=TARGET_ESS, tf_per_generation=rinfo["tfs"], ess_at_tf=rinfo["ess_at_tf"])
        print("refine: target %g, final tf %g; tf per generation %s; effective sample size at the final tf %s, final %.2f"
              % (TARGET_ESS, tf, ["%.6g" % t for t in rinfo["tfs"]], ["%.2f" % e for e in rinfo["ess_at_tf"]], rinfo["ess"][-1]),
              file=sys.stderr)
    if FIND_TF:                                                  # the temperature scan over the refined union: ln r beside LL
        t10 = sync()
        _, LL_u, lnr_u = pop.log_ratio()
        keep = ~np.isnan(LL_u)
        Xg = X_all[keep] / sm.UNIT_CONVERSIONS
        Vu = {n: (np.log10(Xg[:, i]) if lg[i] else Xg[:, i]) for n, i in zip(names, cols)}
        uinfo = {}
        unc = posterior.calc_max_uncertainty(Vu, LL_u[keep], n_obs, info=uinfo, log_ratio=lnr_u[keep])
        out["seconds"]["refine_find_tf"] = sync() - t10
        out["refine"]["max_uncertainty"] = {n: {"tf": t, "Q": q, "at_edge": bool(uinfo["at_edge"][n])} for n, (t, q) in unc.items()}
if MCMC:
    from trpl_amd import mcmc, posterior
    t11 = sync()

    work = {"iters": 0, "cut": 0, "solved": 0}

    def fused_chain(X2, cut_levels=None, cut_budget=None):                        # the fused likelihood of the proposals of one half-sweep
        n = X2.shape[0]
        Xd = torch.from_numpy(np.ascontiguousarray(X2)).to(dev)
        P2 = torch.zeros(n, dtype=torch.float64, device=dev)         # from zero: what early rejection's levels assume
        sse2 = torch.empty((C, n), dtype=torch.float64, device=dev)
        it2 = torch.empty((C, n), dtype=torch.int64, device=dev)
        if cut_budget is not None:                               # one level per proposal, spent across its curves
            bd = torch.from_numpy(np.ascontiguousarray(cut_budget)).to(dev)
            lv = torch.empty((C, n), dtype=torch.float64, device=dev)
            cc = torch.empty((C, n), dtype=torch.int32, device=dev)
            tdev.loglik_cut_budget_device(Xd, ini_d, lens, T * dt, L, T, obs, [T + 1] * C, bd, lv, P2, sse2, curves_per_launch=CURVES_PER_LAUNCH,
                                          cut_col=cc, iters_total=it2)
            work["cut"] += int((cc >= 0).any(dim=0).sum())
        elif cut_levels is None:
            tdev.loglik_device(Xd, ini_d, lens, T * dt, L, T, obs, [T + 1] * C, P2, sse2, iters_total=it2)
        else:                                                    # one level per proposal, given to each of its curves
            lv = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cut_levels, (C, n)))).to(dev)
            cc = torch.empty((C, n), dtype=torch.int32, device=dev)
            tdev.loglik_cut_levels_device(Xd, ini_d, lens, T * dt, L, T, obs, [T + 1] * C, lv, P2, sse2, cut_col=cc, iters_total=it2)
            work["cut"] += int((cc >= 0).any(dim=0).sum())
        work["iters"] += int(it2.sum())
        work["solved"] += n
        return P2.cpu().numpy()

    tf = n_obs * c_val
    X0, U0, LL0 = mcmc.start(X.cpu().numpy(), P.cpu().numpy(), CHAINS, lo, hi, lg, tf=tf)
    minfo = {}
    burn = SWEEPS // 2
    hastings = {}
    if STRETCH is not None:
        hastings.update(kind="stretch", stretch_a=STRETCH)
    if SUBSPACE:
        hastings.update(kind="subspace", pairs=PAIRS, ncr=NCR, adapt_cr=ADAPT_CR)
    if PRIORS:                                                   # centres and linear widths in the box's units, like lo and hi
        centre, width = np.array(lo, dtype=np.float64), np.full(len(lo), np.inf)
        for name, (c0, w0) in PRIORS.items():
            i = sm.PARAM_NAMES.index(name)
            centre[i], width[i] = c0 * sm.UNIT_CONVERSIONS[i], w0 if lg[i] else w0 * sm.UNIT_CONVERSIONS[i]
        hastings.update(prior=mcmc.gaussian_prior(centre, width, lo, hi, lg))
    opts = dict(sweeps=SWEEPS, seed=42, burn=burn, info=minfo, U0=U0, **({"kind": "rw", "scale": RW} if RW is not None else {}), **hastings,
                **({"bounds": "fold"} if FOLD else {}), **({"early_reject": EARLY} if EARLY else {}))
    if TEMPERED:
        hot_ess = None
        if TF_HOT is None:                                       # hot enough for the importance run to hold 64 effective samples
            Pn = P.cpu().numpy()
            TF_HOT, hot_ess = posterior.tf_for_ess(np.where(np.isnan(Pn), -np.inf, Pn), 64.0, lo=tf, hi=1e4 * tf)
        ladder = mcmc.geometric_ladder(tf, TF_HOT, TEMPERED)
        t_run = time.time()
        tempered = mcmc.run_tempered(fused_chain, X0, LL0, lo, hi, lg, ladder, **opts)
        t_run = time.time() - t_run
        rungs = [tempered.rung(k) for k in range(TEMPERED)]
        ch = rungs[0]
        rung_info = dict(minfo)
        minfo = {"accept": list(rung_info["accept"][:, 0]), "outside": float(rung_info["outside"][0]), "folded": float(rung_info["folded"][0])}
        if EARLY:
            minfo["early_reject"] = float(rung_info["early_reject"][0])
        minfo.update({k: rung_info[k] for k in ("pairs", "ncr", "pcr", "mean_dsel") if k in rung_info})
    else:
        t_run = time.time()
        ch = mcmc.run(fused_chain, X0, LL0, lo, hi, lg, tf=tf, **opts)
        t_run = time.time() - t_run
        print("mcmc: %.2f s, %.4f s per sweep" % (t_run, t_run / SWEEPS), file=sys.stderr)
    rhat = ch.rhat()
    Xs, Ws = ch.samples()
    Xg = Xs / sm.UNIT_CONVERSIONS
    Vs = np.ascontiguousarray(np.stack([np.log10(Xg[:, i]) if lg[i] else Xg[:, i] for i in cols]))
    qs = [0.025, 0.5, 0.975]
    q_chain = posterior.quantiles(Vs, Ws, qs)
    q_imp = posterior.quantiles(V.cpu().numpy(), W.cpu().numpy(), qs)
    out["seconds"]["mcmc"] = sync() - t11
    act = [int(i) for i in trpl_amd.refine.active_columns(lo, hi)]
    out["mcmc"] = {"chains": CHAINS, "sweeps": SWEEPS, "kept_sweeps": int(ch.U.shape[0]), "proposal": "rw %g" % RW if RW is not None else "stretch %g" % STRETCH if STRETCH is not None else "subspace" if SUBSPACE else "de",
                   "distinct_starts": int(np.unique(LL0).size),
                   "acceptance": float(np.mean(minfo["accept"])), "acceptance_kept": float(np.mean(minfo["accept"][burn:])),
                   "outside_share_of_proposals": minfo["outside"], "worst_rhat": float(np.nanmax(rhat)),
                   "rhat": {sm.PARAM_NAMES[c]: float(r) for c, r in zip(act, rhat)},
                   "max_loglik": float(ch.LL.max()), "median_loglik": float(np.median(ch.LL[-1])),
                   "quantiles": {n: {"truth": float(tr), "chain": [float(v) for v in q_chain[:, k]],
                                     "importance": [float(v) for v in q_imp[:, k]]} for k, (n, tr) in enumerate(zip(names, truth))}}
    out["mcmc"]["system_timesteps"] = work["iters"]
    if STRETCH is not None:
        out["mcmc"]["stretch_a"] = STRETCH
    if SUBSPACE:
        out["mcmc"]["subspace"] = {"pairs": minfo["pairs"], "ncr": minfo["ncr"], "pcr": [float(v) for v in minfo["pcr"]],
                                   "mean_dsel": float(minfo["mean_dsel"]), "adapt_cr": ADAPT_CR}
        print("mcmc: subspace, %d pairs, %d classes with shares %s%s: %.2f coordinates moved per proposal"
              % (PAIRS, NCR, ["%.3f" % v for v in minfo["pcr"]], " (adapted during the burn sweeps)" if ADAPT_CR else "", minfo["mean_dsel"]),
              file=sys.stderr)
    if PRIORS:
        out["mcmc"]["prior"] = {name: {"center": c0, "width": w0} for name, (c0, w0) in PRIORS.items()}
    if EARLY:
        out["mcmc"]["early_reject"] = {"cut_share_of_solved_proposals": work["cut"] / float(max(work["solved"], 1)),
                                       "levelled_share": minfo["early_reject"]}
    print("mcmc: early_reject=%s: %d proposals solved, %.4f of them cut, %d system-timesteps (solver iterations)"
          % (EARLY, work["solved"], work["cut"] / float(max(work["solved"], 1)), work["iters"]), file=sys.stderr)
    if FOLD:
        out["mcmc"].update(bounds="fold", folded=minfo["folded"])
        print("mcmc: bounds=fold, %.4f of the proposals reflected at a face" % minfo["folded"], file=sys.stderr)
    print("mcmc (%s): %d chains from %d distinct starts, %d sweeps: acceptance %.3f (kept half %.3f), outside the prior box %.4f, worst R-hat %.3f"
          % (out["mcmc"]["proposal"], CHAINS, out["mcmc"]["distinct_starts"], SWEEPS, out["mcmc"]["acceptance"],
             out["mcmc"]["acceptance_kept"], minfo["outside"], out["mcmc"]["worst_rhat"]), file=sys.stderr)
    ess, einfo = ch.ess()                                        # the kept sweeps as 2 C split sequences, every lag
    mcse = np.sqrt(einfo["var_plus"] / ess)
    out["mcmc"]["ess"] = {sm.PARAM_NAMES[c]: {"ess": float(e), "tau": float(t), "truncated": bool(tr), "mcse_unit": float(s)}
                          for c, e, t, tr, s in zip(act, ess, einfo["tau"], einfo["truncated"], mcse)}
    out["mcmc"]["kept_states"] = int(2 * (ch.U.shape[0] // 2) * CHAINS)
    for c, r, e, t, tr in zip(act, rhat, ess, einfo["tau"], einfo["truncated"]):
        print("mcmc: %-8s R-hat %.3f  ESS %9.1f of %d kept states  tau %8.2f sweeps%s"
              % (sm.PARAM_NAMES[c], r, e, out["mcmc"]["kept_states"], t, "  (truncated by the lags: ESS is an upper bound)" if tr else ""),
              file=sys.stderr)
    if TEMPERED:
        worst = [float(np.nanmax(r.rhat())) for r in rungs]
        out["mcmc"]["tempered"] = {"rungs": TEMPERED, "ladder": [float(v) for v in ladder], "tf_hot_ess": hot_ess,
                                   "acceptance": [float(v) for v in rung_info["accept"].mean(axis=0)], "worst_rhat": worst,
                                   "swap_rate": [float(v) for v in tempered.swap_rate], "seconds_run": t_run,
                                   "seconds_per_sweep": t_run / SWEEPS}
        for k in range(TEMPERED):
            print("mcmc: rung %2d  tf %10.4g  acceptance %.3f  worst R-hat %.3f  swap rate to the next %s"
                  % (k, ladder[k], out["mcmc"]["tempered"]["acceptance"][k], worst[k],
                     "%.3f" % tempered.swap_rate[k] if k + 1 < TEMPERED else "-"), file=sys.stderr)
        print("mcmc: tempered, %d rungs: %.2f s, %.4f s per sweep" % (TEMPERED, t_run, t_run / SWEEPS), file=sys.stderr)
        if EVIDENCE:
            Pn = P.cpu().numpy()
            base_lnr = None
            if PRIORS:                                           # the sampler's prior term, unnormalised: -ln p(u) of the base's draws
                Ub, _ = trpl_amd.refine.unit_coords(X.cpu().numpy(), lo, hi, lg)
                p_mean, p_sd = hastings["prior"]
                base_lnr = 0.5 * np.sum(((Ub - p_mean) / p_sd) ** 2, axis=1)
            ev = tempered.log_evidence(blocks=16, base=(np.where(np.isnan(Pn), -np.inf, Pn), TF_HOT, base_lnr))
            names3 = ("forward", "reverse", "ti")
            out["mcmc"]["tempered"]["evidence"] = {
                "blocks": ev["blocks"], "dropped_sweeps": ev["dropped"], "min_term_ess": float(ev["term_ess"].min()),
                "base_ln_z": ev["base_ln_z"], "base_se": ev["base_se"], "base_ess": ev["base_ess"],
                **{n: {"total": ev[n + "_total"], "total_se": ev[n + "_total_se"], "pairs": [float(v) for v in ev[n]],
                       "pairs_se": [float(v) for v in ev[n + "_se"]], "ln_z": ev["ln_z"][n], "ln_z_se": ev["ln_z_se"][n]} for n in names3}}
            print("evidence: base ln Z(tf_hot = %.4g) = %.4f +- %.4f (importance run, ess %.1f)" % (TF_HOT, ev["base_ln_z"], ev["base_se"], ev["base_ess"]),
                  file=sys.stderr)
            print("evidence: %d blocks of %d kept sweeps (%d dropped), smallest term_ess %.4f"
                  % (ev["blocks"], (ev["t1"] - ev["t0"]) // ev["blocks"], ev["dropped"], ev["term_ess"].min()), file=sys.stderr)
            for n in names3:
                print("evidence: %-7s ln Z(tf) - ln Z(tf_hot) = %12.4f +- %.4f   ln Z(tf = %.4g) = %12.4f +- %.4f"
                      % (n, ev[n + "_total"], ev[n + "_total_se"], tf, ev["ln_z"][n], ev["ln_z_se"][n]), file=sys.stderr)
            for k in range(TEMPERED - 1):
                print("evidence: pair %2d-%-2d  forward %11.4f +- %.4f  reverse %11.4f +- %.4f  ti %11.4f +- %.4f  term_ess %.4f %.4f"
                      % (k, k + 1, ev["forward"][k], ev["forward_se"][k], ev["reverse"][k], ev["reverse_se"][k], ev["ti"][k], ev["ti_se"][k],
                         ev["term_ess"][k, 0], ev["term_ess"][k, 1]), file=sys.stderr)
    for k, n in enumerate(names):
        print("mcmc: %-8s truth %9.4f | chain %9.4f %9.4f %9.4f | importance %9.4f %9.4f %9.4f"
              % ((n, truth[k]) + tuple(q_chain[:, k]) + tuple(q_imp[:, k])), file=sys.stderr)
if IRF_FWHM is not None:
    from trpl_amd import irf as tirf, posterior
    t12 = sync()
    resp = tirf.gaussian(IRF_FWHM, dt)
    n_conv = T + 1 - resp[1]
    seen = tirf.convolve(10.0 ** obs.cpu().numpy(), *resp)       # the marked point's curves as the detector records them
    LL_irf = tirf.loglik(X.cpu().numpy(), ini, lens, T * dt, L, T, [np.log10(seen[c]) for c in range(C)], resp)
    tf_irf = C * n_conv * c_val
    W_irf = posterior.weights(LL_irf, tf_irf)
    qs = [0.025, 0.5, 0.975]
    q_irf = posterior.quantiles(V.cpu().numpy(), W_irf, qs)
    q_bare = posterior.quantiles(V.cpu().numpy(), W.cpu().numpy(), qs)
    out["seconds"]["irf"] = sync() - t12
    ess_irf = float(1.0 / np.nansum(W_irf * W_irf))
    out["irf"] = {"fwhm_ns": IRF_FWHM, "taps": int(len(resp[0])), "k0": int(resp[1]), "columns": n_conv, "tf": tf_irf,
                  "effective_sample_size": ess_irf, "effective_sample_size_without": out["effective_sample_size"],
                  "max_loglik": float(np.nanmax(LL_irf)),
                  "quantiles": {n: {"truth": float(tr), "with_irf": [float(v) for v in q_irf[:, k]], "without": [float(v) for v in q_bare[:, k]]}
                                for k, (n, tr) in enumerate(zip(names, truth))}}
    print("irf: Gaussian of %g ns, %d taps: effective sample size %.2f (without the response %.2f), %.2f s"
          % (IRF_FWHM, len(resp[0]), ess_irf, out["effective_sample_size"], out["seconds"]["irf"]), file=sys.stderr)
    for k, n in enumerate(names):
        print("irf: %-8s truth %9.4f | with the response %9.4f %9.4f %9.4f | without %9.4f %9.4f %9.4f"
              % ((n, truth[k]) + tuple(q_irf[:, k]) + tuple(q_bare[:, k])), file=sys.stderr)
if IRF_FWHM is not None and (IRF_SHIFTS is not None or IRF_WIDTHS is not None):
    # the profile over a bank of responses: the detector's response is NOT the bank's centre
    t13 = sync()
    shifts = [0.0] if IRF_SHIFTS is None else IRF_SHIFTS
    widths = [IRF_FWHM] if IRF_WIDTHS is None else IRF_WIDTHS
    bank = tirf.gaussian_bank(widths, shifts, dt)
    Hb, kb, table = bank
    J = len(Hb)
    centre = (len(widths) // 2) * len(shifts) + len(shifts) // 2
    true_w, true_s = int(round(0.75 * (len(widths) - 1))), int(round(0.75 * (len(shifts) - 1)))
    j_true = true_w * len(shifts) + true_s
    if j_true == centre and J > 1:
        j_true = J - 1
    seen_b = tirf.convolve(10.0 ** obs.cpu().numpy(), Hb[j_true], kb)
    obs_b = [np.log10(seen_b[c]) for c in range(C)]
    binfo = {}
    Xh = X.cpu().numpy()
    tf_b = C * (T + 1 - kb) * c_val
    if (IRF_REDUCE, IRF_MAG) == ("max", "fixed"):
        LL_prof = tirf.loglik_profile(Xh, ini, lens, T * dt, L, T, obs_b, bank, info=binfo)
    else:
        LL_prof = tirf.loglik_nuisance(Xh, ini, lens, T * dt, L, T, obs_b, bank, mag=IRF_MAG, reduce=IRF_REDUCE, tf=tf_b, info=binfo)
    LL_fix = tirf.loglik(Xh, ini, lens, T * dt, L, T, obs_b, (Hb[centre], kb))
    W_prof, W_fix = posterior.weights(LL_prof, tf_b), posterior.weights(LL_fix, tf_b)
    ok = binfo["best"] >= 0
    share = np.bincount(binfo["best"][ok], weights=np.nan_to_num(W_prof[ok]), minlength=J)
    ess_prof, ess_fix = float(1.0 / np.nansum(W_prof * W_prof)), float(1.0 / np.nansum(W_fix * W_fix))
    q_prof = posterior.quantiles(V.cpu().numpy(), W_prof, [0.025, 0.5, 0.975])
    q_fix = posterior.quantiles(V.cpu().numpy(), W_fix, [0.025, 0.5, 0.975])
    out["seconds"]["irf_bank"] = sync() - t13
    out["irf_bank"] = {"responses": J, "taps": int(Hb.shape[1]), "k0": int(kb), "table": table.tolist(), "true_response": j_true,
                       "fixed_response": centre, "best_share": share.tolist(), "recovered_response": int(np.argmax(share)),
                       "effective_sample_size_profile": ess_prof, "effective_sample_size_fixed": ess_fix,
                       "quantiles": {n: {"truth": float(tr), "profile": [float(v) for v in q_prof[:, k]], "fixed": [float(v) for v in q_fix[:, k]]}
                                     for k, (n, tr) in enumerate(zip(names, truth))}}
    out["irf_bank"].update(reduce=IRF_REDUCE, mag=IRF_MAG)
    if "best_mag" in binfo:
        out["irf_bank"]["best_mag_mean"] = float(np.nansum(np.nan_to_num(W_prof[ok]) * np.nan_to_num(binfo["best_mag"][ok])))
        print("irf bank: reduce %s, mag %s at tf %g: posterior-weighted mean of the best offset %+.5f"
              % (IRF_REDUCE, IRF_MAG, tf_b, out["irf_bank"]["best_mag_mean"]), file=sys.stderr)
    print("irf bank: %d responses of %d taps; the detector's is %d (fwhm %g ns, shift %g ns), the fixed run uses %d (fwhm %g ns, shift %g ns)"
          % ((J, Hb.shape[1], j_true) + tuple(table[j_true]) + (centre,) + tuple(table[centre])), file=sys.stderr)
    print("irf bank: effective sample size %.2f with the profile, %.2f with the fixed response, %.2f s"
          % (ess_prof, ess_fix, out["seconds"]["irf_bank"]), file=sys.stderr)
    for j in np.argsort(-share)[:min(J, 8)]:
        print("irf bank: response %3d  fwhm %8.4f ns  shift %+9.5f ns  posterior share of best %.4f%s"
              % (j, table[j][0], table[j][1], share[j], "   <- the detector's" if j == j_true else ""), file=sys.stderr)
    for k, n in enumerate(names):
        print("irf bank: %-8s truth %9.4f | profile %9.4f %9.4f %9.4f | fixed response %9.4f %9.4f %9.4f"
              % ((n, truth[k]) + tuple(q_prof[:, k]) + tuple(q_fix[:, k])), file=sys.stderr)
print(json.dumps(out))
