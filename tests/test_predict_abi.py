"""TRPL_FLAG_PREDICT (include/trpl.h) without a device: the flag's value and bit, the kernel names a predict launch runs
and that the library contains them, the default names untouched, the refusals, and the Python layer's own refusal."""
import itertools
import re

import numpy as np
import pytest

import abi_header as H


def library_kernels(A):
    return set(re.findall(r"(trpl::(?:predict::)?(?:pair::|f32::)?stepper(?:_pair)?_kernel<[^>]*>)", H.demangled()))


def test_flag_value_is_one_free_bit(trpl):
    A = trpl._abi
    flags = {k: v for k, v in H.defines().items() if k.startswith("TRPL_FLAG_")}
    assert flags["TRPL_FLAG_PREDICT"] == A.FLAG_PREDICT == 0x100000
    p = A.FLAG_PREDICT
    assert p & (p - 1) == 0                                                  # a single bit
    assert p & (0xF << 8) == 0 and p & (0x7 << 14) == 0                      # outside TRPL_FLAG_BUNDLE and TRPL_FLAG_BDF_ORDER
    others = [v for k, v in flags.items() if k != "TRPL_FLAG_PREDICT"]
    assert len(others) >= 12 and all(v & p == 0 for v in others)
    assert A.flag_bundle(16, 4) & p == 0 and A.flag_bdf_order(5) & p == 0
    assert trpl._abi.lib().trpl_abi_version() == 5


@pytest.mark.parametrize("snap", [False, True])
def test_predict_kernel_names_exist_in_the_library(trpl, snap):
    A = trpl._abi
    have = library_kernels(A)
    tf = {False: "false", True: "true"}
    for L in (4, 8, 16, 32, 64, 128, 256, 512):
        for strict in (False, True):
            fl = A.FLAG_PREDICT | (A.FLAG_STRICT if strict else 0) | A.FLAG_KERNEL_SINGLE * (not strict)
            name = A.kernel_name(64, L, 8000, fl, snapshots=snap)
            assert name == "trpl::predict::stepper_kernel<%d, %s, %s, false, false, false>" % (L, tf[strict], tf[snap])
            assert name in have, name
            # the library's own choice at a small launch is the one-system kernel too
            assert A.kernel_name(64, L, 8000, A.FLAG_PREDICT | (A.FLAG_STRICT if strict else 0), snapshots=snap) == name
    for fl, opt in ((A.FLAG_KERNEL_PAIR, True), (A.FLAG_KERNEL_PAIR | A.FLAG_PAIR_ALWAYS_SEAM, False), (0, True)):
        name = A.kernel_name(196608, 128, 8000, fl | A.FLAG_PREDICT, snapshots=snap)
        assert name == "trpl::predict::pair::stepper_pair_kernel<true, %s, %s>" % (tf[snap], tf[opt])
        assert name in have, name


def test_default_kernel_names_are_unchanged(trpl):
    A = trpl._abi
    assert A.kernel_name(196608, 128, 8000) == "trpl::pair::stepper_pair_kernel<true, false, true>"
    assert A.kernel_name(64, 512, 8000) == "trpl::stepper_kernel<512, false, false, false, false, false>"
    assert A.kernel_name(64, 128, 8000, A.FLAG_STRICT, snapshots=True) == "trpl::stepper_kernel<128, true, true, false, false, false>"
    for L, fl, snap in itertools.product((4, 64, 128, 256, 512), (0, A.FLAG_STRICT, A.FLAG_KERNEL_SINGLE), (False, True)):
        assert "predict" not in A.kernel_name(10 ** 6, L, 8000, fl, snapshots=snap)
    # every predict kernel is a new symbol next to its counterpart: nothing renamed, nothing dropped
    have = library_kernels(A)
    base = {n for n in have if "predict" not in n}
    pred = have - base
    assert len(pred) == 8 * 2 * 2 + 4, sorted(pred)
    for n in pred:
        assert n.replace("predict::", "") in base, n


def test_refusals(trpl):
    A = trpl._abi
    P = A.FLAG_PREDICT
    cases = [(A.FLAG_FP32, A.ERR_ARG, 256), (A.FLAG_FP32 | A.FLAG_FP32_LONG, A.ERR_ARG, 256), (A.FLAG_MIXED, A.ERR_ARG, 256),
             (A.FLAG_HIST32, A.ERR_ARG, 512), (A.flag_bundle(2, 128), A.ERR_UNSUPPORTED, 128),
             (A.flag_bundle(3, 128) | A.FLAG_STRICT, A.ERR_UNSUPPORTED, 128), (A.flag_bundle(4, 64), A.ERR_UNSUPPORTED, 64)]
    for fl, code, L in cases:
        with pytest.raises(A.TrplError) as e:
            A.kernel_name(64, L, 100, fl | P)
        assert e.value.code == code and "TRPL_FLAG_PREDICT" in str(e.value), (hex(fl), e.value.code, str(e.value))
        if code == A.ERR_UNSUPPORTED:                                        # the bundle itself is valid without the flag
            assert "predict" not in A.kernel_name(64, L, 100, fl)
    # bundle 1 (no bits) and every other flag combine with it
    assert "predict" in A.kernel_name(64, 128, 8000, P | A.FLAG_SNAP_RAW | A.FLAG_PL_F32 | A.FLAG_NORMALIZE | A.flag_bdf_order(2))


def test_pvsim_refuses_predict_with_bundles_before_any_device(trpl):
    S, L, T = 4, 128, 10
    pl = np.zeros((S, T + 1))
    mat = np.ones((S, 12))
    sim = (1000.0, 1.0, L, T, 1, None, 7, 100)
    with pytest.raises(ValueError) as e:
        trpl.model.pvSim(pl, None, None, None, mat, sim, np.zeros(L), None, None, 2, init_mode="points", predict=True)
    assert "predict" in str(e.value) and "max_sims_per_block" in str(e.value)
    gi = {"sims_per_gpu": 4, "num_gpus": 1, "predict": True, "max_sims_per_block": 2}
    with pytest.raises(ValueError) as e:
        trpl.driver.simulate(trpl.model.pvSim, [], np.zeros((0, S)), np.ones((S, 13)), None, None, 1, list(sim),
                             np.zeros((1, L)), {"log_pl": True, "self_normalize": False}, gi, 0, [0.0], [0.0], [0.0])
    assert "predict" in str(e.value) and "max_sims_per_block" in str(e.value)
