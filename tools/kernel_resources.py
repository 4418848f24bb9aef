#!/usr/bin/env python3
"""Register / LDS / occupancy table of the stepper kernels from hipcc's kernel-resource-usage remarks.
    python tools/kernel_resources.py [pair fast strict mixed f32 predict_fast predict_strict predict_pair
                                       moments_fast moments_strict moments_pair moments_predict_fast
                                       moments_predict_strict moments_predict_pair weighted_fast weighted_strict
                                       weighted_pair weighted_predict_fast weighted_predict_strict weighted_predict_pair
                                       cut_fast cut_pair cut_predict_fast cut_predict_pair likelihood posterior posterior_scan predictive
                                       quantiles corner refine refine_oriented mcmc mcmc_hastings mcmc_subspace
                                       mcmc_evidence cut_budget irf irf_bank nuisance]
(cross-compiles, no GPU needed; a name is an object of the library without its stepper_ prefix: csrc/<name>.hip or
csrc/stepper_<name>.hip where that file exists, otherwise a variant of csrc/stepper_variants.hpp -- [sink_][predict_]unit --
which is stepper_[pair_]variant.hip with the switch of each of its words, as the Makefile compiles it; mcmc has the sampler's
accept and levels kernels in all three forms, hastings_accept_kernel and hastings_levels_kernel among them, mcmc_hastings the
stretch move and the prior term, mcmc_subspace the subspace proposal, mcmc_evidence the extrema and the sums of the log-evidence
estimates, irf the instrument-response convolution, whose LDS is dynamic and not in the table: 32 (n + n / 8 + 1) bytes with n = 518 + K,
irf_bank the likelihood against a bank of responses and the profile over it, all LDS static, nuisance the reduction over
responses x magnitude offsets: three mag modes, each with the maximum and with the marginal)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc")
SWITCHES = ("moments", "weighted", "cut", "predict", "strict")              # -DTRPL_STEPPER_<WORD>=1 of a variant's words
CONTRACT_OFF = ("likelihood", "posterior", "posterior_scan", "corner", "refine", "refine_oriented", "mcmc", "mcmc_hastings", "mcmc_subspace", "mcmc_evidence", "cut_budget", "irf", "irf_bank", "nuisance")                            # beside every stepper with the word "strict" (Makefile)


def unit(n):
    """(source, compiler flags) of the object `n`"""
    words = n.split("_")
    flags = ["-ffp-contract=" + ("off" if "strict" in words or n in CONTRACT_OFF else "on")]
    for src in (os.path.join(CSRC, "%s.hip" % n), os.path.join(CSRC, "stepper_%s.hip" % n)):
        if os.path.isfile(src):
            return src, flags
    src = os.path.join(CSRC, "stepper_pair_variant.hip" if words[-1] == "pair" else "stepper_variant.hip")
    return src, flags + ["-DTRPL_STEPPER_%s=1" % w.upper() for w in words if w in SWITCHES]


def main():
    names = sys.argv[1:] or ["pair", "fast", "strict", "hist32"]
    if "refine" in names and "refine_oriented" not in names:     # the refine group: both units of the refinement generations
        names.insert(names.index("refine") + 1, "refine_oriented")
    for n in names:
        src, flags = unit(n)
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950"] + flags +
                           ["-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
            name = b.split("\n")[0].split(" ")[0]
            g = lambda k: (re.search(k + r": (\d+)", b) or [None, "?"])[1]
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            print("%-14s %-78s VGPR %3s AGPR %3s spill %3s scratch %4s occ %s LDS %6s" % (
                n, dem[:78], g("VGPRs"), g("AGPRs"), g("VGPR Spill"), g(r"ScratchSize \[bytes/lane\]"),
                g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))


if __name__ == "__main__":
    main()
