"""The rule of trpl_loglik_cut_budget (include/trpl.h) restated in numpy: the level of a launch of curves from a sample's budget B
for its total squared error and the reported sse of the curves before it.  Vectorised over the samples; every addition is one fp64
rounding, as in csrc/cut_budget.hip (built with -ffp-contract=off)."""
import numpy as np


def carried(sse_rows):
    """R: the sum of the rows in ascending order from +0.0, one rounding per addition.  sse_rows (c0, S) -> (S,)."""
    sse_rows = np.asarray(sse_rows, dtype=np.float64)
    R = np.zeros(sse_rows.shape[1:])
    for row in sse_rows:
        R = R + row
    return R


def level(B, R):
    """The level all curves of a launch run at.  B, R broadcastable arrays -> float64 array."""
    B, R = np.broadcast_arrays(np.asarray(B, dtype=np.float64), np.asarray(R, dtype=np.float64))
    out = np.full(B.shape, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(B) | np.isnan(R)
        free = nan | (B == np.inf)                                   # NaN: never cut; B = +inf: never cut, whatever R
        past = ~free & (R >= B)
        out[past] = -1.0
        todo = ~free & ~past
        l = np.maximum(B - R, 0.0)
        for _ in range(3):                                           # l0, its successor, the successor of that
            hit = todo & (R + l >= B)
            out[hit] = l[hit]
            todo &= ~hit
            l = np.nextafter(l, np.inf)
    return out


def levels(budget, sse, g):
    """cut_level (C, S) of a call with curves_per_launch = g that REPORTED sse (C, S): the rows of launch 0 get the budget, the
    rows c0 .. c0 + g - 1 of a later launch level(budget, carried(sse[:c0]))."""
    sse = np.asarray(sse, dtype=np.float64)
    C = sse.shape[0]
    out = np.empty(sse.shape)
    budget = np.asarray(budget, dtype=np.float64)
    for c0 in range(0, C, g):
        # launch 0 has nothing carried: the budget itself (a NaN budget never cuts)
        out[c0:c0 + g] = level(budget, carried(sse[:c0])) if c0 else np.where(np.isnan(budget), np.inf, budget)
    return out
