"""What the non-finite case table (tests/nonfinite_cases.py) must satisfy on its own, without a GPU: every case's reference footprint is
useful (non-empty, at most half of the output, so the finite remainder is still a parity check), has the obvious shape (a guard against a typo
in a reference), every ReLU site of csrc has a case, and DEVIATIONS holds pinned expectations for exactly the cases it names."""
import pytest
import torch

from tests import nonfinite_cases as NF

PARAMS, IDS = NF.params()


@pytest.mark.parametrize("case,dtype,payload", PARAMS, ids=IDS)
def test_reference_footprint_is_useful_and_has_the_obvious_shape(case, dtype, payload):
    b = case.build(dtype, payload)
    # inputs are values of their storage dtype, and the payload is in place
    held = 0
    for name, v in b.inputs.items():
        if torch.is_tensor(v) and v.is_floating_point():
            st = b.in_dtypes.get(name, dtype)
            assert torch.equal(torch.nan_to_num(v.to(st).double(), 7.0, 8.0, 9.0), torch.nan_to_num(v, 7.0, 8.0, 9.0)), f"{name} is not rounded to {st}"
            cls = NF.classes(v)
            held += int((cls != 0).sum())
            assert set(cls.unique().tolist()) <= {0, 1 + NF.ALL3.index(payload)}
    assert held >= 2, "a case holds its payload at two positions at least (first element, vector body, ragged part)"
    nonfinite = sum(int((NF.classes(w) != 0).sum()) for w in b.want.values())
    total = sum(w.numel() for w in b.want.values())
    # The footprint conditions hold PER CASE (all outputs together) and for the case's first output on its own; a secondary output may be
    # non-finite throughout where the mathematics says so (dgamma of a LayerNorm with a NaN row: every column sums that row's xhat).
    # (an infinity may legitimately come out finite -- relu(-Inf) = 0, a clip, exp(-Inf) = 0 -- and the device must then give that value;
    # a NaN payload always reaches the output, except through a mask that compares it: the cases marked empty_ok)
    if payload == "nan" and not case.empty_ok:
        assert nonfinite > 0, "the reference output holds no NaN: the case checks nothing"
    assert 2 * nonfinite <= total, f"{nonfinite} of {total} reference outputs are non-finite: too little is left for the parity check"
    first = next(iter(b.want.values()))
    assert 2 * int((NF.classes(first) != 0).sum()) <= first.numel()
    if payload == "nan":
        for name, mask in b.shape.items():
            got = torch.isnan(b.want[name])
            assert torch.equal(got, mask), (f"{name}: the reference's NaN footprint ({int(got.sum())} elements) is not the expected one "
                                            f"({int(mask.sum())} elements)")
    # a deviation replaces the reference's expectation for that case only, and says what it pins
    assert (b.pinned is not None) == (case.key in NF.DEVIATIONS)
    if b.pinned is not None:
        assert set(b.pinned) == set(b.want)
        reason, behaviour = NF.DEVIATIONS[case.key]
        assert reason and behaviour


def test_every_relu_site_has_a_case_and_its_wrapper_exists():
    from iseg_amd import kernels      # (imports without the shared library: nothing is called)

    for code, name in ((NF.ACT_RELU, "ACT_RELU"), (NF.ACT_GELU, "ACT_GELU"), (NF.ACT_GELU_GRAD, "ACT_GELU_GRAD"), (NF.ACT_RELU_GRAD, "ACT_RELU_GRAD"),
                       (NF.ACT_MUL_AUX, "ACT_MUL_AUX"), (NF.ACT_SIGMOID, "ACT_SIGMOID"), (NF.ACT_SWISH, "ACT_SWISH"), (NF.ACT_GELU_TANH, "ACT_GELU_TANH")):
        assert getattr(kernels, name) == code
    families = {}
    for c in NF.CASES:
        families.setdefault(c.family, []).append(c)
    for site, (wrapper, family) in NF.RELU_SITES.items():
        assert callable(getattr(kernels, wrapper, None)), f"{site}: iseg_amd.kernels has no {wrapper}"
        assert family in families, f"{site}: no case of family {family}"
        built = [(c, c.build(c.dtypes[0], "nan")) for c in families[family][:4]]      # (each case built once; four per family are enough)
        behind_relu = [(c, b) for c, b in built if b.relu]
        assert behind_relu, f"{site}: no case of {family} puts a NaN through the ReLU"
        for c, b in behind_relu:
            assert any(torch.isnan(w).any() for w in b.want.values()), f"{c.family}/{c.name}: the reference's ReLU swallowed the NaN"


def test_deviations_name_existing_cases():
    keys = {c.key for c in NF.CASES}
    for key in NF.DEVIATIONS:
        assert key in keys, f"DEVIATIONS names {key}, which is not a case"
