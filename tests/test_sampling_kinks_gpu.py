"""The sampling kernels at the cell borders: DCNv3, DCNv2's sampling half and deformable attention against their fp64 references, with every
element of the offset gradient judged by its class (tests/sampling_kinks.py):

    interior  the as-is reference, to the max-norm tolerance of the core tests (fp32: 5e-5 of scale)
    lattice   the same, with no either-side allowance: fp32 and fp64 compute the same coordinate, so the kernel must take the reference's side at an
              exact integer and its inclusive clip bounds
    border    the gradient of the + side or of the - side of the kink (|coord - kink| < TAU: fp32 may land on either)

and every element of the continuous outputs (forward, value / mask / attention gradients) against the as-is reference.  bf16 storage: a stored
element is the fp32 value rounded once, |got - ref| <= 2^-8 |ref| + the fp32 tolerance (sampling_kinks.allowance); the statistics of the stored
rounding are tests/test_rounding_budget_gpu.py's.  tests/test_sampling_kinks_host.py shows on the CPU that the rule is attainable (the restatement in
torch.float32 meets it) and that it bites (mutants of the restatement miss it).

Routes, selected by shape as in test_dcnv3_gpu.py / test_deformable_mhsa_gpu.py: DCNv3 pipelined forward + window backward (Cg 8 / 16), general forward
and backward (Cg 3, 4, 24, 32), each through the dense entry points and the joint [pixels, ld] layout; dcnv2_sample forward / backward; deformable
attention with 16-byte loads (Ch 8 / 16) and one channel per lane (Ch 3), and its backward.  Every line printed is
    KINKS <case> <dtype> <output> [<class>]: <elements>, worst err <of scale> ...
"""
import pytest
import torch

from tests import sampling_kinks as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _params(op):
    ps = [(c, dt) for c in S.CASES if c.op == op for dt in S.DTYPES]
    return pytest.mark.parametrize("case,dtype", ps, ids=[f"{c.kind}-{c.name}-{S._dt(dt)}" for c, dt in ps])


def _check(case, dtype, got):
    """got: {output: (device tensor, stored in bf16?)}"""
    ref, cls = S.reference(case, dtype), S.classes(case, dtype)
    sh = S.shares(cls)
    print(f"KINKS {case.id} {S._dt(dtype)} classes: {sh['n']} elements, lattice {int(cls.lattice.sum())} ({sh['on_bound']} on a clip bound), "
          f"border {int(cls.border.sum())} ({sh['border']:.5f}), interior {int(cls.interior.sum())}; TAU {cls.tau:.3e}")
    if case.kind in ("random", "budget"):
        assert sh["border"] <= S.MAX_BORDER_SHARE
    assert set(got) == set(ref.base)
    bad = []
    for name, (g, stored) in got.items():
        assert g.dtype == (dtype if stored or dtype != BF else torch.float32) and g.numel() == ref.base[name].numel(), (name, g.dtype, tuple(g.shape))
        if name == "doffset":
            lines, b = S.judge_offset_gradient(case, dtype, g, ref, cls)
            print("\n".join(lines))
            print(f"KINKS {case.id} {S._dt(dtype)} doffset rel l2 against the as-is reference {S.rel_l2(g, ref.base['doffset']):.3e}")
        else:
            line, b = S.judge_continuous(case, dtype, name, g, ref, stored)
            print(line)
        bad += b
    assert not bad, "\n".join(bad)


@_params("dcnv3")
@pytest.mark.parametrize("layout", ["dense", "joint"])
def test_dcnv3_offset_gradient_by_class(cuda, case, dtype, layout):
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    p = case.p
    (N, H, W, C), G, s = p["shape"], p["G"], p.get("s", 1.0)
    Cg, gp = C // G, G * 9
    d = {k: v.cuda() for k, v in S.operands(case, dtype).items()}
    window = _hip.lib().iseg_dcnv3_bwd_side_bytes(N, H, W, G, Cg, 3, 3, 1, 1, 1, s) > 0
    assert window == (Cg in (8, 16)), "the backward route is not the one this case was chosen for"
    bf = dtype == BF
    if layout == "dense":
        y = K.dcnv3_fwd(d["x"], d["offset"], d["mask"], G, Cg, 3, 3, 1, 1, 1, s)
        dx, doff, dmask = K.dcnv3_bwd(d["x"], d["offset"], d["mask"], d["dout"], G, Cg, 3, 3, 1, 1, 1, s)
        got = {"y": (y, bf), "dx": (dx, False), "dmask": (dmask, bf), "doffset": (doff, bf)}
    else:
        ld = (3 * gp + 7) // 8 * 8 + 8
        om = torch.full((N * H * W, ld), float("nan"), dtype=dtype, device="cuda")
        om[:, :2 * gp] = d["offset"].reshape(-1, 2 * gp)
        om[:, 2 * gp:3 * gp] = d["mask"].reshape(-1, gp)
        y = K.dcnv3_fwd_joint(d["x"], om, G, Cg, 3, 3, 1, 1, 1, s)
        dx, dom = K.dcnv3_bwd_joint(d["x"], om, d["dout"], G, Cg, 3, 3, 1, 1, 1, s)
        got = {"y": (y, bf), "dx": (dx, bf), "dmask": (dom[:, 2 * gp:3 * gp].contiguous(), bf), "doffset": (dom[:, :2 * gp].contiguous(), bf)}
    torch.cuda.synchronize()
    _check(case, dtype, got)


@_params("dcnv2")
def test_dcnv2_sample_offset_gradient_by_class(cuda, case, dtype):
    from iseg_amd import kernels as K

    d = {k: v.cuda() for k, v in S.operands(case, dtype).items()}
    col = K.dcnv2_sample_fwd(d["x"], d["offset"])
    dx, doff = K.dcnv2_sample_bwd(d["x"], d["offset"], d["dout"])
    torch.cuda.synchronize()
    bf = dtype == BF
    _check(case, dtype, {"col": (col, bf), "dx": (dx, False), "dlogit": (doff[..., 18:].contiguous(), bf), "doffset": (doff[..., :18].contiguous(), bf)})


@_params("defattn")
def test_deformable_attention_offset_gradient_by_class(cuda, case, dtype):
    from iseg_amd import kernels as K

    p = case.p
    d = {k: v.cuda() for k, v in S.operands(case, dtype).items()}
    out = K.defattn_fwd(d["value"], d["offset"], d["attn"], p["heads"], p["P"], p["orf"])
    dvalue, doff, dattn = K.defattn_bwd(d["value"], d["offset"], d["attn"], d["dout"], p["heads"], p["P"], p["orf"])
    torch.cuda.synchronize()
    bf = dtype == BF
    _check(case, dtype, {"out": (out, bf), "dvalue": (dvalue, bf), "dattn": (dattn, bf), "doffset": (doff, bf)})
