"""stepper_kernel<L> (csrc/stepper_impl.hpp) at EVERY compiled grid size, L = 4 .. 512, in STRICT and FAST, through every sink
(PL store, plain likelihood, moments, weighted, cut) and with TRPL_FLAG_PREDICT -- each held to the CPU oracle or to longdouble
sums over the oracle's PL (tests/grid_cases.py), never only to another GPU result.  tests/test_grid_cases_host.py proves on the
CPU what is assumed here: everything converges, every column is far above the cancellation floor (no column and no system is
left out: above_floor(...).all() and floor_col == -1 are asserted), forced_max has a value, no cut decision is on a knife edge.

Gates (none of them new):
  PL, STRICT   the oracle bit for bit (RTOL_STRICT), status and iteration totals equal.
  PL, FAST     follows_iteration_path; 2000 nm film: RTOL_FAST on every column for L <= 128 (as test_pvsim_small_grids... of
               tests/test_gpu_stepper_parity.py), the header's envelope 1e-9 + TRPL_PL_ENVELOPE_K_L512 / r for L = 256, 512 (as
               tests/test_gpu_l512.py applies it; at 256 the stencil is less stiff, the constant is an upper bound); 311 nm
               film: 1e-9 + ENVELOPE_K[311.0] / r.  float32 output: 2^-23 STRICT, 2^-22 FAST (test_pvsim_float32_buffer...,
               test_fast_mode_plT...).
  P, sse       tests/test_gpu_likelihood.py's gates for the same comparison at L = 128: STRICT 1e-11 (test_fused_loglik_vs_
               reference_and_oracle, ..._real_data_and_offgrid_times), STRICT with normalize 1e-10 (..._twothick_normalize...),
               FAST 1e-8, float32 staging 2e-5 (test_paired_kernel_offgrid_observations_normalize_and_f32_staging_vs_oracle).
  esum, weighted sums   the derived bound of test_gpu_weighted.py::test_weighted_sums_against_numpy_within_the_derived_bound
               (its _depth, EPS): k eps sum w e^2 / k eps sum w |e|, plus 2 sqrt(wsum sse) d / wsum d for the per-column gap d
               of log10 PL between the two evaluations: FAST the PL gate above over ln 10 (4.4e-10 where K / r vanishes, as in
               these windows); both modes the roundings of forming one error in float64 against the longdouble reference,
               c eps max|lg| with c = 4 on the grid (log10 to 1 ulp, two additions, the reference's own) and 8 off it (two
               logs, the four operations of the interpolation).
  predict      STRICT + PREDICT within the header's 5e-5 of the oracle's default path on every column, same flagged systems;
               FAST + PREDICT follows STRICT + PREDICT under the PL gates (test_gpu_predict.py::test_fast_follows_strict_in_the_mode).
Measured worst error / allowance per size and film: printed, and in the record file test_stepper_grids.json."""
import math

import numpy as np
import pytest

import grid_cases as G
from gpu_common import (ENVELOPE_K, ENVELOPE_K_L512, RTOL_FAST, RTOL_STRICT, above_floor, excess_scale, follows_iteration_path,
                        record, relerr)
from test_gpu_cut import _check_against_plain
from test_gpu_moments import _same_outputs
from test_gpu_weighted import EPS, _depth

pytestmark = pytest.mark.gpu

MODES = {"strict": dict(strict=True), "single": dict(kernel="single")}
REC = {}


def _note(key, **figures):
    REC.setdefault(key, {}).update({k: float(v) for k, v in figures.items()})
    print("%s: %s" % (key, ", ".join("%s %.3g" % kv for kv in figures.items())))
    record("stepper_grids", REC)


def _allow(L, film, r):
    """FAST's allowance on |dPL / PL| per column, r = PL_ref / (B L n0p0) (the module docstring)."""
    if film == "thin":
        return 1e-9 + ENVELOPE_K[311.0] / r
    if L <= 128:
        return np.full_like(r, RTOL_FAST)
    return 1e-9 + ENVELOPE_K_L512 / r


def _check_pl(L, film, length, X, pl, want, strict, cols=slice(None), label=""):
    """Every column of `cols`; returns the worst error / allowance (0 for STRICT: equality)."""
    want = want[:, cols]
    pl = pl[:, cols]
    assert above_floor(want).all()
    if strict:
        assert np.array_equal(pl, want) and relerr(pl, want) <= RTOL_STRICT, label
        return 0.0
    r = want / excess_scale(X, length, L)[:, None]
    ratio = np.abs(pl / want - 1) / _allow(L, film, r)
    if film == "thick" and L <= 128:
        assert (ratio < 1.0).all(), (label, float(ratio.max()))
    else:
        assert (ratio <= 1.0).all(), (label, float(ratio.max()))
    return float(ratio.max())


def _env_lg(L, film, ref):
    """The PL gate of FAST as a gap of log10 PL: the largest allowance over the window's columns / ln 10."""
    worst = 0.0
    for c in range(ref["C"]):
        r = ref["sol"][c]["plI"] / excess_scale(ref["X"], ref["lens"][c], L)[:, None]
        worst = max(worst, float(np.max(_allow(L, film, r))))
    return worst / math.log(10.0)


# ------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_pl_mode_against_the_oracle(gpu, oracle, L, film):
    ini, lens = G.film(film, L)
    X = G.samples()
    sol = G.solution(L, film)
    variants = [(1, np.float64)] + ([(4, np.float64), (1, np.float32)] if L in G.LAYOUT_SIZES else [])
    worst = 0.0
    for c in range(len(lens)):
        for plT, dtype in variants:
            want = sol[c] if plT == 1 else oracle.pvsim(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], plT=plT)
            assert not want["status"].any() and want["plI"].shape == (G.S, G.T // plT + 1)
            for mode, kw in MODES.items():
                pl, st, it, _ = gpu.solve_pl(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], plT=plT, dtype=dtype, **kw)
                label = "L %d %s curve %d plT %d %s %s" % (L, film, c, plT, np.dtype(dtype).name, mode)
                assert pl.dtype == dtype and pl.shape == want["plI"].shape and np.array_equal(st, want["status"]), label
                if mode == "strict":
                    assert np.array_equal(it, want["iters_total"]), label
                else:
                    follows_iteration_path(it, want["iters_total"], label)
                if dtype == np.float32:
                    assert above_floor(want["plI"]).all()
                    if mode == "strict":                   # the oracle's own float32 buffer: the same two roundings, one ulp
                        w32 = oracle.pvsim(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], plT=plT, dtype=np.float32)["plI"]
                        gap = float(np.max(np.abs(pl - w32) / w32))
                    else:
                        gap = float(np.max(np.abs(pl.astype(np.float64) / want["plI"] - 1)))
                    assert gap <= (2.0 ** -23 if mode == "strict" else 2.0 ** -22), (label, gap)
                else:
                    worst = max(worst, _check_pl(L, film, lens[c], X, pl, want["plI"], mode == "strict", label=label))
    _note("L%d_%s" % (L, film), pl_fast_worst_over_allowance=worst)


# ------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("L,film", G.FORCED_CASES)
def test_forced_nonconvergence(gpu, L, film, mode):
    """MAX = forced_max(...): some systems flagged, some not, none within one iteration of the cap.  status is the oracle's; PL
    before the failing step under the gates of the PL test, NaN from it on; the unflagged systems keep the bits of the run at
    the default cap.  (In these windows the stiffest step is the first one: the flagged systems fail at step 0.)"""
    ini, lens = G.film(film, L)
    X = G.samples()
    sol = G.solution(L, film)
    cap = G.forced_max(np.concatenate([r["step_iters"] for r in sol]))
    forced = G.solution(L, film, MAX=cap)
    flagged = np.concatenate([r["status"] for r in forced]) != 0
    assert flagged.any() and not flagged.all()
    kw = MODES[mode]
    for c in range(len(lens)):
        want = forced[c]
        full, st0, _, _ = gpu.solve_pl(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], **kw)
        pl, st, it, _ = gpu.solve_pl(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], MAX=cap, **kw)
        assert not st0.any() and np.array_equal(st, want["status"]), (c, cap, st.tolist(), want["status"].tolist())
        for s in range(G.S):
            t = st[s] - 1 if st[s] else G.T + 1
            assert np.isnan(pl[s, t:]).all(), (c, s)
            if t:
                _check_pl(L, film, lens[c], X[s:s + 1], pl[s:s + 1], sol[c]["plI"][s:s + 1], mode == "strict", cols=slice(0, t))
            if not st[s]:
                assert pl[s].tobytes() == full[s].tobytes(), (c, s)
    print("L %d %s %s: MAX %d flags %d of %d systems, at steps %s" % (
        L, film, mode, cap, flagged.sum(), flagged.size, sorted(set((np.concatenate([r["status"] for r in forced])[flagged] - 1).tolist()))))


# ------------------------------------------------------------------------------------------------------- c
def _loglik(gpu, ref, L, mode, **kw):
    info = {}
    P = gpu.loglik(ref["X"], ref["ini"], ref["lens"], G.TIME, L, G.T, ref["obs"], times=ref["times"], info=info, **MODES[mode], **kw)
    return P, info


def _want_iters(ref, c):
    """The oracle's iteration total over the steps a likelihood launch takes: on the grid a curve stops after its last compared
    column (steps 0 .. n_obs - 1), off the grid the last observation sits at Time (every step)."""
    steps = ref["sol"][c]["step_iters"]
    return steps[:, :ref["n"][c] if ref["times"] is None else G.T + 1].sum(axis=1)


def _check_solve(ref, info, mode, label):
    for c in range(ref["C"]):
        want = ref["sol"][c]
        assert np.array_equal(info["status"][c], want["status"]) and not info["status"][c].any(), label
        if mode == "strict":
            assert np.array_equal(info["iters_total"][c], _want_iters(ref, c)), label
        else:
            follows_iteration_path(info["iters_total"][c], _want_iters(ref, c), label)
    assert (info["floor_col"] == -1).all(), label


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_fused_likelihood_plain_sink(gpu, L, film, mode, offgrid):
    variants = [dict()] + ([dict(normalize=True), dict(pl_f32=True)] if L in G.LAYOUT_SIZES else [])
    for v in variants:
        ref = G.reference(L, film, offgrid, normalize=bool(v.get("normalize")), f32=bool(v.get("pl_f32")))
        P, info = _loglik(gpu, ref, L, mode, **v)
        label = "L %d %s %s %s %s" % (L, film, mode, "offgrid" if offgrid else "ongrid", v)
        _check_solve(ref, info, mode, label)
        gate = 2e-5 if v.get("pl_f32") else (1e-8 if mode != "strict" else (1e-10 if v.get("normalize") else 1e-11))
        gP = float(np.max(np.abs(P - ref["P"]) / np.abs(ref["P"])))
        gs = float(np.max(np.abs(info["sse"] - ref["sse"]) / ref["sse"]))
        _note("L%d_%s" % (L, film), **{"loglik_%s_%s%s_P_over_gate" % (mode, "off" if offgrid else "on", "".join("_" + k for k in v)): gP / gate,
                                       "loglik_%s_%s%s_sse_over_gate" % (mode, "off" if offgrid else "on", "".join("_" + k for k in v)): gs / gate})
        assert gP < gate and gs < gate, (label, gP, gs, gate)


# ------------------------------------------------------------------------------------------------------- d
def _sum_bounds(L, film, ref, mode, offgrid, c, weighted):
    """(bound on sse, bound on esum) of curve c per system, against the longdouble sums (the module docstring)."""
    s = ref["sums"][c]
    n = ref["n"][c]
    k = _depth(n, mode == "strict")
    sse, ab, wsum = (s["wsse"], s["wabs"], ref["wsum"][c]) if weighted else (s["sse"], s["abs"], float(n))
    sse, ab = np.asarray(sse, dtype=float), np.asarray(ab, dtype=float)
    d = (8 if offgrid else 4) * EPS * ref["max_lg"] + (0.0 if mode == "strict" else _env_lg(L, film, ref))
    return k * EPS * sse + 2 * np.sqrt(wsum * sse) * d, k * EPS * ab + wsum * d


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_moments_and_weighted_sinks_against_the_longdouble_sums(gpu, L, film, mode, offgrid):
    ref = G.reference(L, film, offgrid)
    label = "L %d %s %s %s" % (L, film, mode, "offgrid" if offgrid else "ongrid")
    Pp, plain = _loglik(gpu, ref, L, mode)
    _, mom = _loglik(gpu, ref, L, mode, mag_grid=[0.0])
    _same_outputs(mom, plain, mom["P"], Pp)
    _check_solve(ref, mom, mode, label)
    _, wt = _loglik(gpu, ref, L, mode, weights=ref["wts"])
    _check_solve(ref, wt, mode, label)
    for k in ("status", "iters_total", "floor_col"):
        assert np.array_equal(wt[k], plain[k]), k
    assert np.array_equal(wt["wsum"], ref["wsum"])
    worst = 0.0
    for c in range(ref["C"]):
        s = ref["sums"][c]
        b2, b1 = _sum_bounds(L, film, ref, mode, offgrid, c, False)
        e2, e1 = np.abs(mom["sse"][c] - np.asarray(s["sse"], dtype=float)), np.abs(mom["esum"][c] - np.asarray(s["esum"], dtype=float))
        w2, w1 = _sum_bounds(L, film, ref, mode, offgrid, c, True)
        f2, f1 = np.abs(wt["sse"][c] - np.asarray(s["wsse"], dtype=float)), np.abs(wt["esum"][c] - np.asarray(s["wesum"], dtype=float))
        worst = max(worst, float((e2 / b2).max()), float((e1 / b1).max()), float((f2 / w2).max()), float((f1 / w1).max()))
        assert (e2 <= b2).all() and (e1 <= b1).all(), (label, c, "moments", float((e2 / b2).max()), float((e1 / b1).max()))
        assert (f2 <= w2).all() and (f1 <= w1).all(), (label, c, "weighted", float((f2 / w2).max()), float((f1 / w1).max()))
    _note("L%d_%s" % (L, film), **{"sums_%s_%s_worst_over_bound" % (mode, "off" if offgrid else "on"): worst})
    # a zero weight is an absent observation: inside a batch, on a batch boundary, in the last batch
    keep = [100, 64, 131][:ref["C"]]
    masked = [np.where(np.arange(len(w)) < k, w, 0.0) for w, k in zip(ref["wts"], keep)]
    _, got = _loglik(gpu, ref, L, mode, weights=masked)
    short = dict(ref, obs=[o[:k] for o, k in zip(ref["obs"], keep)],
                 times=None if ref["times"] is None else [t[:k] for t, k in zip(ref["times"], keep)])
    _, want = _loglik(gpu, short, L, mode, weights=[w[:k] for w, k in zip(ref["wts"], keep)])
    assert not got["status"].any() and not want["status"].any()
    assert np.array_equal(got["sse"], want["sse"]) and np.array_equal(got["esum"], want["esum"]), label


@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_cut_sink_stops_where_the_reference_sums_dictate(gpu, L, film, predict):
    """The level lies between the systems' final sums (grid_cases.cut_level).  A system is cut, and at the column, that the
    reference's running sums dictate; a column of slack would be allowed only where a tested sum is within the likelihood
    gate (1e-8) of the level, which happens for no system of the seeded inputs (asserted here and on the CPU).  The reported
    partial sum is the reference's running sum there within that gate; then test_gpu_cut.py's identity with the truncated
    plain call.  predict: the decisions are the default path's (5e-5 on PL moves a sum by far less than its distance to the
    level, asserted), the sums are held to STRICT + PREDICT's own within the gate."""
    ref = G.reference(L, film, False)
    level = G.cut_level(ref)
    col, edge = G.cut_plan(ref, level, 1e-8 if not predict else 1e-3)
    assert not edge.any()
    info = {}
    gpu.loglik(ref["X"], ref["ini"], ref["lens"], G.TIME, L, G.T, ref["obs"], info=info, sse_cut=level, kernel="single", predict=predict)
    assert not info["status"].any()
    assert np.array_equal(info["cut_col"], col), (L, film, info["cut_col"].tolist(), col.tolist())
    if not predict:
        worst = 0.0
        for c in range(ref["C"]):
            k = np.where(col[c] < 0, ref["n"][c], col[c])
            want = np.asarray(ref["run"][c][np.arange(G.S), k - 1], dtype=float)
            gap = np.abs(info["sse"][c] - want) / want
            worst = max(worst, float(gap.max()))
            assert (gap < 1e-8).all(), (L, film, c, float(gap.max()))
            assert ((info["floor_col"][c] == -1)).all()
        _note("L%d_%s" % (L, film), cut_partial_sse_over_gate=worst / 1e-8)
    _check_against_plain(gpu, ref["X"], ref["ini"], ref["lens"], G.T, ref["obs"], None, dict(kernel="single", predict=predict),
                         "L %d %s predict=%s" % (L, film, predict), L=L)


# ------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_predict_at_every_size(gpu, L, film):
    ini, lens = G.film(film, L)
    X = G.samples()
    sol = G.solution(L, film)
    worst = vs_default = 0.0
    it_default = it_predict = 0
    for c in range(len(lens)):
        ps, ss, its, _ = gpu.solve_pl(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], strict=True, predict=True)
        pf, sf, itf, _ = gpu.solve_pl(X[:, :12], lens[c], G.TIME, L, G.T, ini[c], kernel="single", predict=True)
        want = sol[c]
        assert np.array_equal(ss, want["status"]) and np.array_equal(sf, want["status"]) and not ss.any()
        follows_iteration_path(itf, its, "L %d %s curve %d" % (L, film, c))
        assert (ps > 0).all() and above_floor(ps).all()
        worst = max(worst, _check_pl(L, film, lens[c], X, pf, ps, False, label="L %d %s curve %d FAST + PREDICT" % (L, film, c)))
        assert above_floor(want["plI"]).all()
        gap = float(np.max(np.abs(ps / want["plI"] - 1)))
        vs_default = max(vs_default, gap)
        assert gap <= 5e-5, (L, film, c, gap)                               # include/trpl.h, TRPL_FLAG_PREDICT: every column
        it_default += int(want["iters_total"].sum())
        it_predict += int(its.sum())
    # the likelihood call of the plain-sink test with predict, plain and moments sinks, FAST against STRICT
    for offgrid in (False, True):
        ref = G.reference(L, film, offgrid)
        out = {}
        for mode in MODES:
            P, plain = _loglik(gpu, ref, L, mode, predict=True)
            _, mom = _loglik(gpu, ref, L, mode, predict=True, mag_grid=[0.0])
            _same_outputs(mom, plain, mom["P"], P)
            assert not plain["status"].any() and (plain["floor_col"] == -1).all()
            out[mode] = (P, mom)
        (Ps, ms), (Pf, mf) = out["strict"], out["single"]
        for c in range(ref["C"]):
            follows_iteration_path(mf["iters_total"][c], ms["iters_total"][c], "L %d %s predict loglik curve %d" % (L, film, c))
            b2, b1 = _sum_bounds(L, film, ref, "single", offgrid, c, False)
            assert (np.abs(mf["esum"][c] - ms["esum"][c]) <= b1).all() and (np.abs(mf["sse"][c] - ms["sse"][c]) <= b2).all(), (L, film, c)
        gP = float(np.max(np.abs(Pf - Ps) / np.abs(Ps)))
        gs = float(np.max(np.abs(mf["sse"] - ms["sse"]) / ms["sse"]))
        assert gP < 1e-8 and gs < 1e-8, (L, film, offgrid, gP, gs)
        # and against the reference's default path: the bound that follows from 5e-5 on every column
        delta = math.log10(1 + 5e-5)
        for c in range(ref["C"]):
            s = ref["sums"][c]
            bound = 2 * delta * np.asarray(s["abs"], dtype=float) + ref["n"][c] * delta ** 2
            assert (np.abs(ms["sse"][c] - np.asarray(s["sse"], dtype=float)) <= bound + 1e-11 * ms["sse"][c]).all(), (L, film, c)
    _note("L%d_%s" % (L, film), predict_fast_vs_strict_worst_over_allowance=worst, predict_strict_vs_default_oracle=vs_default,
          iterations_default_over_predict=it_default / it_predict)
