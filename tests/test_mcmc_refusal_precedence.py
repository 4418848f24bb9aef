"""Which of two refusals wins: trpl_mcmc_accept{,_rungs,_h}{,_dev} and trpl_mcmc_levels{,_rungs,_h}{,_dev} (include/trpl.h) with
every pair of simultaneous faults from FAULTS, one fault per refusal of the call's record.  Each call is TRPL_ERR_ARG and its
trpl_last_error() is the text of tests/golden/mcmc_refusal_precedence.json, recorded from the library as it was before the three forms
shared one record and one check each; `python tests/test_mcmc_refusal_precedence.py` records it again from the
library it finds.  The ABI tests hold each refusal alone; this holds their order.  No GPU needed."""
import itertools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mcmc_refusal_precedence.json")

# the arguments of each form in the entry point's order, before the tail (stream, or device and seconds)
ACCEPT = ("U", "X", "LL", "Up", "Xp", "LLp", "inside")
FORMS = {
    "accept": ACCEPT + ("count", "A", "ncol", "tf1", "chain0", "seed", "step", "accepted"),
    "accept_rungs": ACCEPT + ("count", "A", "ncol", "K", "group", "tf", "chain0", "seed", "step", "accepted"),
    "accept_h": ACCEPT + ("h", "count", "A", "ncol", "K", "group", "tf", "chain0", "seed", "step", "accepted"),
    "levels": ("LL", "count", "tf1", "chain0", "seed", "step", "level"),
    "levels_rungs": ("LL", "count", "K", "group", "tf", "chain0", "seed", "step", "level"),
    "levels_h": ("LL", "h", "count", "K", "group", "tf", "chain0", "seed", "step", "level"),
}
POINTERS = ("U", "X", "LL", "Up", "Xp", "LLp", "inside", "h", "accepted", "level", "tf")
BAD_LADDER = np.array([1.0, -2.0, 2.5, 0.5])                     # tf[1] refused
# name -> (the argument it spoils, its value): a form takes the faults whose argument it has (the last one only with K and group
# beside its count); two faults of one argument are no pair
FAULTS = dict([("K", ("K", 0)), ("group", ("group", 0)), ("group_blocks", ("group", (1 << 31) * 256)), ("tf[k]", ("tf", BAD_LADDER.ctypes.data)),
               ("count", ("count", 0)), ("count_blocks", ("count", (1 << 31) * 256)), ("A", ("A", 17)), ("chain0", ("chain0", -1)),
               ("ncol", ("ncol", 0)), ("tf", ("tf1", 0.0)), ("count!=K*group", ("count", 7))] +
              [(p + "=NULL", (p, None)) for p in POINTERS])


# the faultless call: the two arrays live as long as the module, so the addresses in BASE stay good
ZEROS = np.zeros(4096)
LADDER = np.array([1.0, 2.5, 2.5, 0.5])
BASE = dict({k: ZEROS.ctypes.data for k in ("U", "X", "LL", "Up", "Xp", "LLp", "inside", "h", "accepted", "level")}, count=8, A=3, ncol=4,
            tf1=1.5, K=4, group=2, tf=LADDER.ctypes.data, chain0=0, seed=7, step=2)


def cases(form, base=BASE):
    """(key, arguments) of every single fault and every pair of faults of `form`, each put into `base`"""
    mine = [(n, f) for n, f in FAULTS.items() if f[0] in FORMS[form] and (n != "count!=K*group" or "K" in FORMS[form])]
    for (na, (ka, va)), (nb, (kb, vb)) in itertools.combinations_with_replacement(mine, 2):
        if na != nb and ka == kb:
            continue
        yield (na if na == nb else na + " + " + nb), dict(base, **{ka: va, kb: vb})


def observe(abi, form, suffix, a):
    fn = getattr(abi.lib(), "trpl_mcmc_" + form + suffix)
    rc = fn(*[a[k] for k in FORMS[form]], *([None] if suffix else [0, None]))
    return rc, abi.lib().trpl_last_error().decode()


def test_the_fault_list_has_every_refusal_of_every_form():
    for form, args in FORMS.items():
        have = {f[0] for f in FAULTS.values()}
        assert {a for a in args if a not in ("seed", "step")} <= have, form         # seed and step are never refused
    assert len(FAULTS) == 22


def test_which_of_two_refusals_wins(trpl):
    A = trpl._abi
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(FORMS)
    for form in FORMS:
        got = dict(cases(form))
        assert sorted(got) == sorted(want[form]), form           # no case dropped, none added
        for key, a in got.items():
            for suffix in ("", "_dev"):
                rc, text = observe(A, form, suffix, a)
                assert rc == A.ERR_ARG, (form + suffix, key, rc)
                assert text == want[form][key], (form + suffix, key)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import trpl_amd
    out = {}
    for form in FORMS:
        out[form] = {}
        for key, a in cases(form):
            seen = {observe(trpl_amd._abi, form, suffix, a) for suffix in ("", "_dev")}
            assert len(seen) == 1 and next(iter(seen))[0] == trpl_amd._abi.ERR_ARG, (form, key, seen)
            out[form][key] = next(iter(seen))[1]
    json.dump(out, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print({f: len(c) for f, c in out.items()})
