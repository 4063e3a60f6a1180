"""The gradient-buffer contract's census (no GPU): every tape node that writes a parameter gradient has a contract case.

iseg_amd/functional.py books parameter gradients itself (see its first lines), so each such Function.backward re-implements autograd's rules by
hand; tests/test_grad_contract_gpu.py checks those rules case by case from the table in tests/grad_contract_cases.py.  This file keeps the table
complete: a new tape node whose backward takes a parameter-gradient destination cannot be added without a case that names it."""
import importlib
import inspect
import re

import pytest
import torch

from tests import grad_contract_cases as T

MODULES = ["iseg_amd.functional", "iseg_amd.layers.nasfpn", "iseg_amd.layers.multihead_axial_attention"]
# a parameter-gradient destination: the gradient-buffer helpers of functional.py
_DESTINATION = re.compile(r"\b(_grad|_param_grad|_grad_out|_se_grads)\(")


def _functions():
    out = {}
    for name in MODULES:
        mod = importlib.import_module(name)
        for attr, obj in vars(mod).items():
            if inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function and obj.__module__ == name:
                out[attr] = obj
    return out


def _books_parameter_gradients(fn):
    """the backward body, and the static helpers of the class it calls, take a parameter-gradient destination"""
    src = inspect.getsource(fn)
    start = src.find("def backward")
    return start >= 0 and _DESTINATION.search(src[start:]) is not None


def test_census_finds_the_known_nodes():
    """the selection rule itself: it must see the nodes this table was written for, and must not see a node without parameters"""
    fns = _functions()
    booking = {n for n, f in fns.items() if _books_parameter_gradients(f)}
    for name in ("_DenseFn", "_Conv2dFn", "_LayerNormFn", "_ConvNeXtBlockFn", "_BnSwishSEFn", "_BatchNormGroupFn", "_JpuTailFn", "_EmbeddingFn",
                 "_DcnJointFn", "_AttentionFn"):
        assert name in booking, name
    for name in ("_CastFn", "_ActFn", "_ForkFn", "_FlashAttentionFn", "_Dcnv3Fn", "_NearestUpFn", "_ChannelPermuteFn"):
        assert name in fns and name not in booking, name


def test_every_parameter_gradient_node_has_a_contract_case():
    fns = _functions()
    booking = {n for n, f in fns.items() if _books_parameter_gradients(f)}
    covered = {n for c in T.CASES for n in c.covers}
    unknown = sorted(covered - set(fns))
    assert not unknown, f"covers= names no Function of {MODULES}: {unknown}"
    stray = sorted(covered - booking)
    assert not stray, f"covers= names Functions whose backward books no parameter gradient: {stray}"
    missing = sorted(booking - covered)
    assert not missing, f"tape nodes that write parameter gradients without a case in tests/grad_contract_cases.py: {missing}"


def test_case_table_is_well_formed():
    names = [c.name for c in T.CASES]
    assert len(names) == len(set(names))
    for c in T.CASES:
        assert c.covers and c.parity.startswith("tests/test_") and "::" in c.parity, c.name
        assert set(c.tol) - {"norm"} == {"param", "dx"} and all(0.0 <= c.tol[k] <= 4e-2 for k in ("param", "dx")), c.name
        assert c.tol.get("norm", "max") in ("max", "l2"), c.name
        assert c.dtype in (torch.float32, torch.bfloat16)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_oracle_gradients_lie_in_the_sentinel_range(case):
    """inputs and upstream gradients are chosen so that every parameter gradient of the fp64 oracle peaks in [2^-4, 2^4] -- for the seeded run
    and for the second batch of the shared run"""
    from iseg_amd import nn

    nn.set_device("cpu")
    built = case.build()
    for seed in (0, 1):
        grads, _, _ = T.oracle(case, built, seeds=(seed,))
        T.assert_oracle_gradient_range(case, grads, built.params)
