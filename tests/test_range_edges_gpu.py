"""The softmax, loss, activation and normalisation kernels at the edges of their range: logits shifted by 1e4, rows whose exp terms all but
underflow, confident pixels, all-ignored batches, scores of +-200 in front of the online softmax, sigmoid arguments past the overflow of exp,
inputs scaled by 2^+-20.  Inputs, fp64 references and fp32 restatements come from tests/range_edge_inputs.py; tests/test_range_edges_host.py shows
on the CPU that every regime is reached and that the bounds used here are attainable in fp32 arithmetic.

Every regime group is compared on its own scale with the tolerance of the project's existing test of the same kernel.  Only in the groups
where fp32 arithmetic cannot meet that tolerance (RESTATEMENT_CEILING in range_edge_inputs.py lists them with the measured figures, and the host
test pins each) the bound is 4 x the error of the fp32 CPU restatement against fp64 on the same inputs -- never anything taken from the
kernel's output."""
import os

import pytest
import torch

from oracle import tf_ops as O
from tests import mask_loss_ref as MR
from tests import range_edge_inputs as E
from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def K():
    from iseg_amd import kernels

    return kernels


def _finite(*ts):
    for t in ts:
        assert torch.isfinite(t).all(), "non-finite output"


# ---------------------------------------------------------------------------------------------------------------------------
# softmax_ce_ignore, plain and focal
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(E.CE_MODES))
@pytest.mark.parametrize("C", E.LOSS_C)
def test_softmax_ce_ignore_range_edges(cuda, C, mode):
    """per-pixel loss, its scaled sum and dlogits of every regime of ce_cases(C) against oracle.tf_ops in fp64, group by group at the tolerances
    of test_softmax_ce_ignore (1e-5) / test_softmax_focal_ce_ignore (2e-5, 5e-5 on the gradient).  Out of reach of fp32 only with the label on
    the top class: plain CE at gap 12 (restatement: 6.9e-7 on losses of ~1e-4, 930 x the tolerance; 27 x on the gradient) and the clipped focal
    loss at gaps 12 / 30 / 200 (4.8e-9 on 2.5e-8, 240 x); there the bound is 4 x the restatement's error.  The loss sum holds at 1e-5 / 2e-5."""
    k = K()
    focal, use_w = E.CE_MODES[mode]
    tol_px, tol_dz = E.CE_TOL[focal is not None]
    for regime, case in E.ce_cases(C).items():
        P = case["z"].shape[0]
        scale = 0.37 / P
        lo, dz = E.ce_reference(case, C, focal, use_w, scale)
        lo32, dz32 = E.ce_restatement_fp32(case, C, focal, use_w, scale)
        px, sm, dl = k.softmax_ce_ignore(case["z"].float().cuda(), case["y"].cuda(), E.IGNORE, class_w=case["cw"].cuda() if use_w else None,
                                         want_px=True, want_sum=True, sum_scale=1.0 / P, want_grad=True, grad_scale=scale, focal=focal)
        _finite(px, sm, dl)
        what = f"C={C} {regime} {mode}"
        fam = E.ce_family(focal)
        E.check_groups(px, lo, case["groups"], tol_px, what + " loss", E.restatement_allowance(fam, "loss", lo32, lo, case["groups"]))
        E.check_groups(dl, dz, case["groups"], tol_dz, what + " dlogits", E.restatement_allowance(fam, "dlogits", dz32, dz, case["groups"]))
        mean = lo.mean().item()
        assert abs(sm.item() - mean) <= tol_px * max(1.0, abs(mean)), (what, sm.item(), mean)
        ignored = case["y"] == E.IGNORE
        assert (px.cpu()[ignored] == 0).all() and (dl.cpu()[ignored] == 0).all(), what + ": ignored pixels are exactly zero"
        if regime == "all_ignored":
            assert sm.item() == 0.0 and (px == 0).all() and (dl == 0).all()
        if regime == "zero_weight" and use_w:
            idx = case["groups"]["weight0"]
            assert (px.cpu()[idx] == 0).all() and (dl.cpu()[idx] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# upsample_ce
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upsample_ce_range_edges(cuda, dtype):
    """the regimes on the low-resolution logits (x8 bilinear, 2 x 32 x 32 output pixels): shifted, wide, confident, and the degenerate batches
    (all labels ignored, one valid pixel, a zero class weight on the labelled class, identical logits).  Loss sum and dz against the oracle's
    resize + CE in fp64 as in tests/test_upsample_ce_gpu.py (2e-5 on the loss; 2e-5 / 1e-2 on dz, per sample).  Interpolating fp32 logits of
    1e4 costs the restatement 2.8 x the dz tolerance in that sample; there, and nowhere else, the bound is 4 x the restatement's error."""
    k = K()
    N, Hi, Wi, C, s = E.UP_N, E.UP_HI, E.UP_WI, E.UP_C, E.UP_S
    Ho, Wo = Hi * s, Wi * s
    assert k.upsample_ce_supported(Hi, Wi, Ho, Wo, C)
    P = N * Ho * Wo
    tol_sum, tol_dz = E.UP_TOL[dtype]
    fam = "upsample_ce/" + IDS[DTYPES.index(dtype)]
    for case in E.upsample_ce_launches(dtype):
        name = case["name"]
        loss, grad = E.upsample_ce_reference(case)
        _, g32 = E.upsample_ce_reference(case, torch.float32)
        if dtype == torch.bfloat16:
            g32 = E.rq(g32, dtype)
        sm, dz = k.upsample_ce(case["z"].to(dtype).cuda(), case["y"].cuda(), Ho, Wo, E.IGNORE,
                               class_w=None if case["cw"] is None else case["cw"].cuda(), sum_scale=1.0 / P, grad_scale=1.0 / P)
        _finite(sm, dz)
        assert abs(sm.item() - loss.item()) <= tol_sum * max(1.0, abs(loss.item())), (name, sm.item(), loss.item())
        E.check_groups(dz, grad, case["groups"], tol_dz, f"upsample_ce {name} dz", E.restatement_allowance(fam, "dz", g32, grad, case["groups"]))
        if name == "all_ignored":
            assert sm.item() == 0.0 and (dz == 0).all(), "an all-ignored batch has an exactly zero loss and gradient"
        if name == "zero_weight":
            assert loss.item() > 0.1      # (the other labels still count)


# ---------------------------------------------------------------------------------------------------------------------------
# softmax_rows_fwd / softmax_rows_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", E.ALL_SOFTMAX_COLS)
def test_softmax_rows_range_edges(cuda, cols, dtype):
    """iseg_softmax_rows_fwd on both lane groupings of softmax_fwd_reg_kernel (cols 9: 16 lanes per row; 49 .. 197: a wave per row, 2 or 8
    elements per lane; 1021: 32 elements per lane) and, at cols 2053, on the one-wave-per-row softmax_fwd_kernel behind ld > 2048: shifted and wide rows, bias, the 0 / -100
    shift mask, a mask with one open column, the probability clip.  close()'s tolerances (2e-5 / 1.2e-2) per group; pad columns [cols, ld) hold
    NaN on input and must come back as exact zeros; unclipped rows sum to one."""
    k = K()
    ld = E.round_up8(cols)
    tol = E.SOFTMAX_TOL[dtype]
    for regime, case in E.softmax_rows_cases(cols, dtype).items():
        s = case["s"]
        problems, tq, _ = s.shape
        buf = torch.full((problems, tq, ld), float("nan"), dtype=dtype)
        buf[..., :cols] = s.to(dtype)
        out = torch.full((problems, tq, ld), float("nan"), dtype=dtype, device="cuda")
        bias, mask = case["bias"], case["mask"]
        k.softmax_rows_fwd(buf.cuda(), problems, tq, cols, ld, bias=None if bias is None else bias.float().cuda(), heads=E.SM_HEADS,
                           mask=None if mask is None else mask.float().cuda(), windows=E.SM_WINDOWS, clip=case["clip"], out=out)
        got = out.cpu().double().reshape(-1, ld)
        _finite(got)
        assert (got[:, cols:] == 0).all(), f"{regime}: pad columns are not zero"
        want = E.softmax_rows_reference(case)
        E.check_groups(got[:, :cols], want, case["groups"], tol, f"softmax_rows cols={cols} {regime}")
        if case["clip"] is None:
            rowsum_tol = 1e-5 if dtype == torch.float32 else 2.0 ** -8 * 2      # bf16: every stored probability is rounded to 2^-9 relative
            assert (got[:, :cols].sum(-1) - 1).abs().max() <= rowsum_tol, regime
        if regime == "one_open":
            idx = case["groups"]["one_open"]
            oc = case["open_col"][(torch.arange(problems) // E.SM_HEADS) % E.SM_WINDOWS].reshape(-1)
            onehot = torch.zeros(problems * tq, cols, dtype=torch.float64)
            onehot[torch.arange(problems * tq), oc] = 1.0
            assert (got[idx, :cols] - onehot[idx]).abs().max() <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols", E.ALL_SOFTMAX_COLS)
def test_softmax_rows_backward_cancels_a_common_offset(cuda, cols, dtype):
    """dS = P (g - sum g P) with dP = randn +- 100 per row, with and without the clip mask, on stored probabilities.  close()'s tolerances; in
    fp32 the dot product of ~100 carries 1e-5 of rounding (restatement: up to 3.1 x the tolerance on ordinary rows, 16 x on one-hot rows whose
    gradients are ~0.03), so the fp32 bound is 4 x the restatement's error; bf16 holds at close()'s tolerance."""
    k = K()
    ld = E.round_up8(cols)
    p, dp, groups = E.softmax_bwd_case(cols, dtype)
    rows = p.shape[0]
    for clip in (None, (0.02, 0.7)):
        pb = torch.full((rows, ld), float("nan"), dtype=dtype)
        db = torch.full((rows, ld), float("nan"), dtype=dtype)
        pb[:, :cols], db[:, :cols] = p.to(dtype), dp.to(dtype)
        out = torch.full((rows, ld), float("nan"), dtype=dtype, device="cuda")
        k.softmax_rows_bwd(pb.cuda(), db.cuda(), rows, cols, ld, clip=clip, out=out)
        got = out.cpu().double()
        _finite(got)
        assert (got[:, cols:] == 0).all()
        want = E.softmax_bwd_reference(p, dp, clip)
        w32 = E.softmax_bwd_reference(p, dp, clip, torch.float32)
        allow = E.restatement_allowance("softmax_bwd/fp32", "ds", w32, want, groups) if dtype == torch.float32 else None
        E.check_groups(got[:, :cols], want, groups, E.SOFTMAX_TOL[dtype], f"softmax_rows_bwd cols={cols} clip={clip}", allow)


# ---------------------------------------------------------------------------------------------------------------------------
# attention_packed: flash route, fused window route, and the materialised route behind both switches
# ---------------------------------------------------------------------------------------------------------------------------
def _attention_run(switch, mode, qkv, dy, heads, C, d, **kw):
    from iseg_amd import functional as F

    os.environ[switch] = mode
    qg = qkv.to(torch.bfloat16).cuda().requires_grad_(True)
    y = F.attention_packed(qg, heads, C, C, d ** -0.5, **kw)
    y.backward(dy.to(torch.bfloat16).cuda())
    return y.detach().cpu().double(), qg.grad.cpu().double()


def _attention_check(name, y, g, yr, gr, C):
    _finite(y, g)
    assert (y - yr).norm() / yr.norm() < 1.5e-2, name
    assert (g - gr).norm() / gr.norm() < 3e-2, name
    for k3, part in enumerate(("dq", "dk", "dv")):
        a, r = g[..., k3 * C:(k3 + 1) * C], gr[..., k3 * C:(k3 + 1) * C]
        assert (a - r).norm() <= 3e-2 * max(r.norm(), 1e-3 * gr.norm()), (name, part)


@pytest.mark.parametrize("T,positions", [(65, (0, 63, 64)), (130, (5, 127, 129))])
def test_flash_attention_with_a_late_dominant_key(cuda, T, positions):
    """csrc/flashattn.hip and the GEMM + softmax route (ISEG_FLASHATTN 1 / 0), bf16, head_dim 64, forward and backward: scores up to ~200, the
    dominant key of sample b in the first key tile, the last full tile and the ragged tail, so the running maximum arrives early, late and
    last.  The norm-relative bounds of tests/test_attention_gpu.py (1.5e-2 forward, 3e-2 backward, per dq / dk / dv slice)."""
    from iseg_amd import nn
    from tests.test_attention_gpu import _ref_attention

    heads, d, B = 3, 64, 3
    C = heads * d
    qkv, _ = E.attention_case(B, T, heads, d, positions, 21)
    dy = E.rq(E.rnd((B, T, C), 22), torch.bfloat16)
    qr = qkv.clone().requires_grad_(True)
    yr = _ref_attention(qr, heads, C, d ** -0.5)
    yr.backward(dy)
    nn.set_compute_dtype(torch.bfloat16)
    try:
        for mode in ("1", "0"):
            y, g = _attention_run("ISEG_FLASHATTN", mode, qkv, dy, heads, C, d)
            _attention_check(f"ISEG_FLASHATTN={mode} T={T}", y, g, yr.detach(), qr.grad, C)
    finally:
        os.environ.pop("ISEG_FLASHATTN", None)
        nn.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("ws", [7, 8])
def test_window_attention_with_a_dominant_key(cuda, ws):
    """csrc/winattn.hip and the materialised route (ISEG_WINATTN 1 / 0), bf16, head_dim 32, T = ws^2 with the relative-position bias: scores
    up to ~200, the dominant key first, last and in the middle.  Bounds as in test_fused_window_attention_matches_materialised_route_and_oracle."""
    from iseg_amd import nn
    from iseg_amd.backbones.swin import relative_position_index
    from tests.test_attention_gpu import _ref_attention

    heads, d, B, T = 3, 32, 3, ws * ws
    C = heads * d
    qkv, _ = E.attention_case(B, T, heads, d, (0, T - 1, T // 2), 31 + ws)
    dy = E.rq(E.rnd((B, T, C), 32), torch.bfloat16)
    index = torch.from_numpy(relative_position_index((ws, ws)).reshape(-1))
    table0 = (E.rnd(((2 * ws - 1) ** 2, heads), 33) * 0.5).float()
    qr = qkv.clone().requires_grad_(True)
    tr = table0.double().requires_grad_(True)
    yr = _ref_attention(qr, heads, C, d ** -0.5, tr[index.long()].reshape(T, T, heads).permute(2, 0, 1))
    yr.backward(dy)
    nn.set_compute_dtype(torch.bfloat16)
    try:
        for mode in ("1", "0"):
            table = torch.nn.Parameter(table0.clone().cuda())
            y, g = _attention_run("ISEG_WINATTN", mode, qkv, dy, heads, C, d, bias_table=table, bias_index=index.cuda(), bias_window=ws)
            _attention_check(f"ISEG_WINATTN={mode} ws={ws}", y, g, yr.detach(), qr.grad, C)
            gt = table.grad.cpu().double()
            _finite(gt)
            assert (gt - tr.grad).norm() <= 3e-2 * max(tr.grad.norm(), 1e-3 * qr.grad.norm()), mode      # one-hot rows: the bias gradient is ~0
    finally:
        os.environ.pop("ISEG_WINATTN", None)
        nn.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# MaskLoss
# ---------------------------------------------------------------------------------------------------------------------------
MASK_FLAGS = {"defaults": {}, "focal_ce": dict(apply_focal_ce_loss=True), "plain_sigmoid": dict(apply_focal_sigmoid_loss=False),
              "dice_only": dict(use_sigmoid_loss=False, use_ce_loss=False), "ce_only": dict(use_sigmoid_loss=False, use_dice_loss=False)}


@pytest.mark.parametrize("flags", list(MASK_FLAGS))
@pytest.mark.parametrize("mag", [80.0, 1e3])
def test_mask_loss_range_edges(cuda, mag, flags):
    """csrc/mask_loss.hip through MaskLoss: logits of +-80 / +-1e3 mixed with ordinary ones, a sample whose label mask is empty, one where it
    is full, an all-ignored sample.  tests/test_mask_loss_gpu.py's bound (2e-5 x max(1, scale) on values, 2e-5 x scale on gradients) per group of
    pixels -- extreme and ordinary -- against tests/mask_loss_ref.py."""
    from iseg_amd.losses.mask_loss import MaskLoss

    kw = MASK_FLAGS[flags]
    y, z, groups = E.mask_loss_case(mag)
    C = z.shape[-1]
    zr = z.double().requires_grad_(True)
    want_s = MR.mask_loss(y, zr, num_class=C, **kw)
    (want_ds,) = torch.autograd.grad(want_s, zr)
    want_px = MR.mask_loss(y, zr, reduction=True, num_class=C, **kw)
    up = torch.rand(want_px.shape, generator=E.gen(11), dtype=torch.float64) + 0.5
    (want_dpx,) = torch.autograd.grad((want_px * up).sum(), zr)
    zc = z.cuda().requires_grad_(True)
    got_s = MaskLoss(num_class=C, **kw)(y.cuda(), zc)
    (got_ds,) = torch.autograd.grad(got_s, zc)
    got_px = MaskLoss(num_class=C, reduction=True, **kw)(y.cuda(), zc)
    (got_dpx,) = torch.autograd.grad((got_px * up.float().cuda()).sum(), zc)
    _finite(got_s, got_ds, got_px, got_dpx)
    assert abs(float(got_s) - float(want_s)) <= 2e-5 * max(1.0, abs(float(want_s)))
    gp, wp = got_px.detach().cpu().double().reshape(-1), want_px.detach().reshape(-1)
    for name, idx in groups.items():
        err, scale = E.group_error(gp[idx], wp[idx])
        assert err <= 2e-5 * max(1.0, scale), (name, "per-pixel", err, scale)
        for what, got, want in (("dlogits(scalar)", got_ds, want_ds), ("dlogits(per-pixel)", got_dpx, want_dpx)):
            err, scale = E.group_error(got.detach().cpu().double().reshape(-1, C)[idx], want.reshape(-1, C)[idx])
            assert err <= 2e-5 * scale, (name, what, err, scale)
    assert float(got_px[3].abs().max()) == 0.0 and float(got_ds[3].abs().max()) == 0.0 and float(got_dpx[3].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# act_fwd / act_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "swish"])
def test_activation_grid(cuda, act, dtype):
    """+-0, +-{1e-30, 1, 10, 20, 87, 89, 104, 1e4} and the largest finite bf16 through iseg_act_fwd / iseg_act_bwd: finite, and element by element
    within close()'s relative tolerance (2e-5 / 1.2e-2) of fp64 above the floor 104 x FLT_MIN (denormal sigmoid factors).  GELU keeps the bounds
    of test_gelu_approximations_on_a_dense_grid: fp32 2e-6 absolute on top; bf16 1e-3 / 2e-3 absolute for |x| <= 8 and 2^-8 |x| on the tails."""
    k = K()
    code = {"relu": k.ACT_RELU, "gelu": k.ACT_GELU, "sigmoid": k.ACT_SIGMOID, "swish": k.ACT_SWISH}[act]
    x = E.act_grid(dtype)
    want, dwant = E.act_reference(x, act)
    xd = x.to(dtype).cuda()
    dyv = 1.5
    y = k.act_fwd(xd, code).cpu().double()
    dx = k.act_bwd(torch.full_like(xd, dyv), xd, code).cpu().double()
    _finite(y, dx)
    rel = 2e-5 if dtype == torch.float32 else 1.2e-2
    tail = x.abs() > 8
    if act == "gelu" and dtype == torch.float32:
        by, bd = rel * want.abs() + 2e-6, rel * dwant.abs() + 2e-6
    elif act == "gelu":
        by = torch.where(tail, 2.0 ** -8 * x.abs(), 1e-3 + 2.0 ** -8 * want.abs())
        bd = 2e-3 + 2.0 ** -8 * dwant.abs()
    else:
        by, bd = rel * want.abs() + E.ACT_FLOOR, rel * dwant.abs() + E.ACT_FLOOR
    bad = (y - want).abs() > by
    assert not bad.any(), (act, "value", x[bad].tolist(), y[bad].tolist(), want[bad].tolist())
    bad = (dx - dyv * dwant).abs() > dyv * bd
    assert not bad.any(), (act, "gradient", x[bad].tolist(), dx[bad].tolist(), (dyv * dwant[bad]).tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# DCNv3 mask softmax, deformable attention core
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dcn_mask_softmax_range_edges(cuda, dtype):
    """iseg_dcn_mask_softmax_fwd / _bwd (G = 4 groups of P = 9 logits in columns [72, 108) of a [pixels, 112] matrix) on shifted and wide rows,
    against torch.softmax in fp64 and its backward formula as tests/test_dcnv3_gpu.py builds its masks; close()'s tolerances per group; the
    offset columns stay untouched, the gradient's pad columns come back zero.  The backward gets dm = randn + 100; fp32 arithmetic misses
    the tolerance on the one-hot (wide) rows only (restatement: 13 x and 17 x), where the bound is 4 x the restatement's error."""
    k = K()
    G, P = E.DCN_G, E.DCN_P
    ld, col0 = 112, 2 * G * P
    tol = E.SOFTMAX_TOL[dtype]
    rows, groups, p, dm = E.dcn_mask_case(dtype)
    pixels = rows.shape[0] // G
    om = E.rq(E.rnd((pixels, ld), 830), dtype)
    om[:, col0:col0 + G * P] = rows.reshape(pixels, G * P)
    before = om.clone()
    omd = om.to(dtype).cuda()
    k.dcn_mask_softmax_fwd(omd, G, P)
    got = omd.cpu().double()
    _finite(got)
    assert torch.equal(got[:, :col0], before[:, :col0]) and torch.equal(got[:, col0 + G * P:], before[:, col0 + G * P:])
    E.check_groups(got[:, col0:col0 + G * P].reshape(-1, P), torch.softmax(rows, -1), groups, tol, "dcn mask softmax fwd")
    # backward on the reference's probabilities rounded to the storage dtype (the same inputs as the host test), dm = randn + 100
    om[:, col0:col0 + G * P] = p.reshape(pixels, G * P)
    dom = E.rq(E.rnd((pixels, ld), 832), dtype)
    dom[:, col0:col0 + G * P] = dm.reshape(pixels, G * P)
    domd = dom.to(dtype).cuda()
    k.dcn_mask_softmax_bwd(om.to(dtype).cuda(), domd, G, P)
    gd = domd.cpu().double()
    _finite(gd)
    assert torch.equal(gd[:, :col0], dom[:, :col0]) and (gd[:, col0 + G * P:] == 0).all()
    wantb = E.softmax_bwd_reference(p, dm)
    w32 = E.softmax_bwd_reference(p, dm, dtype=torch.float32)
    allow = E.restatement_allowance("dcn_bwd/fp32", "ds", w32, wantb, groups) if dtype == torch.float32 else None
    E.check_groups(gd[:, col0:col0 + G * P].reshape(-1, P), wantb, groups, tol, "dcn mask softmax bwd", allow)


@pytest.mark.parametrize("regime", ["shifted", "wide"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_deformable_attention_core_with_extreme_point_logits(cuda, dtype, regime):
    """F.deformable_attention_core (csrc/defattn.hip) with the attention logits of every (pixel, head) shifted by +-1e4 (fp32) / the bf16 offset,
    or with one point leading by 250: against tests/deformable_mhsa_ref.py at the bounds of tests/test_deformable_mhsa_gpu.py."""
    from iseg_amd import functional as F
    from iseg_amd import nn
    from tests import deformable_mhsa_ref as R

    shape, heads, P, orf = (2, 9, 7, 32), 2, 4, 2.0
    N, H, W, C = shape
    items = N * H * W * heads
    if regime == "shifted":
        a, _, _ = E.shifted_rows(P, dtype, 840, items // 4 + 1)
        a = a[torch.randperm(a.shape[0], generator=E.gen(841))][:items]
    else:
        a, _ = E.wide_rows(P, 842, items // 2 + 1)
        a = a[torch.randperm(a.shape[0], generator=E.gen(843))][:items]
    host = [E.rnd(shape, 1).to(dtype), (E.rnd((N, H, W, heads * P * 2), 2) * 1.5).to(dtype), a.reshape(N, H, W, heads * P).to(dtype),
            E.rnd(shape, 4).to(dtype)]
    v, o, al = (t.double().requires_grad_(True) for t in host[:3])
    want = R.core(v, o, al, heads, P, orf, scrub=False)
    want.backward(host[3].double())
    _finite(want.detach(), v.grad, o.grad, al.grad)
    nn.set_compute_dtype(dtype)
    try:
        vd, od, ad, dout = (t.cuda() for t in host)
        for t in (vd, od, ad):
            t.requires_grad_(True)
        out = F.deformable_attention_core(vd, od, ad, heads, P, orf)
        out.backward(dout)
        _finite(out, vd.grad, od.grad, ad.grad)
        close(out, want.detach(), dtype, "defattn fwd", f32_tol=1e-5, bf16_tol=1.5e-2)
        close(vd.grad, v.grad, dtype, "defattn dvalue", f32_tol=2e-5, bf16_tol=2e-2)
        close(ad.grad, al.grad, dtype, "defattn dattn", f32_tol=2e-5, bf16_tol=2e-2)
        if dtype == torch.float32:
            close(od.grad, o.grad, dtype, "defattn doffset", f32_tol=5e-5)
        else:
            assert (od.grad.cpu().double() - o.grad).norm().item() / o.grad.norm().item() < 5e-2
    finally:
        nn.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm, RMSNorm, GroupNorm, GRN at 2^20 and 2^-20
# ---------------------------------------------------------------------------------------------------------------------------
def _q(t, dtype):
    s = t.to(dtype)
    return s.cuda(), s.to(torch.float64)


@pytest.mark.parametrize("scale", list(E.NORM_SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,C", [(129, 96), (77, 263)])
def test_layernorm_scaled_inputs(cuda, dtype, rows, C, scale):
    """test_layernorm_fwd_bwd's inputs times 2^20 (squares ~1e12) and 2^-20 (eps = 1e-6 dominates the variance), its oracle and tolerances"""
    k = K()
    x, xr = _q((E.rnd((rows, C), 1) * 2 + 0.3) * E.NORM_SCALES[scale], dtype)
    g, b = (E.rnd((C,), 2) * 0.3 + 1).float(), (E.rnd((C,), 3) * 0.2).float()
    y, mean, rstd = k.layernorm_fwd(x, g.cuda(), b.cuda(), 1e-6)
    xx = xr.clone().requires_grad_(True)
    gg, bb = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yo = O.layer_norm(xx, gg, bb, 1e-6)
    _finite(y, mean, rstd)
    close(y, yo, dtype, "ln fwd")
    close(mean, xr.mean(-1), torch.float32, "ln mean", f32_tol=1e-5)
    dy, dyr = _q(E.rnd((rows, C), 4), dtype)
    yo.backward(dyr)
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = k.layernorm_bwd(dy, x, g.cuda(), mean, rstd, dgam, dbet)
    _finite(dx, dgam, dbet)
    close(dx, xx.grad, dtype, "ln dx", f32_tol=1e-4, bf16_tol=2e-2)
    close(dgam, gg.grad, torch.float32, "ln dgamma", f32_tol=2e-4 if dtype == torch.float32 else 2e-2)
    close(dbet, bb.grad, torch.float32, "ln dbeta", f32_tol=2e-4)


@pytest.mark.parametrize("scale", list(E.NORM_SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,C", [(37, 96), (5, 100)])
def test_rmsnorm_scaled_inputs(cuda, dtype, rows, C, scale):
    """test_rmsnorm's inputs times 2^+-20, its oracle and tolerances"""
    k = K()
    x, xr = _q(E.rnd((rows, C), 1) * E.NORM_SCALES[scale], dtype)
    sc = (E.rnd((C,), 2) * 0.3).float()
    dy, dyr = _q(E.rnd((rows, C), 3), dtype)
    y, rstd = k.rmsnorm_fwd(x, sc.cuda(), 1e-6)
    xr.requires_grad_(True)
    sr = sc.double().requires_grad_(True)
    yr = O.rms_norm(xr, sr, 1e-6)
    _finite(y, rstd)
    close(y, yr, dtype, "rmsnorm fwd")
    yr.backward(dyr)
    ds = torch.zeros(C, device="cuda")
    dx = k.rmsnorm_bwd(dy, x, sc.cuda(), rstd, ds, accumulate=False)
    _finite(dx, ds)
    close(dx, xr.grad, dtype, "rmsnorm dx", f32_tol=5e-5, bf16_tol=2e-2)
    close(ds, sr.grad, dtype, "rmsnorm dscale", f32_tol=5e-5, bf16_tol=2e-2)


@pytest.mark.parametrize("scale", list(E.NORM_SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,groups", [((3, 5, 7, 96), 2), ((2, 3, 3, 32), 32)])
def test_groupnorm_scaled_inputs(cuda, dtype, shape, groups, scale):
    """test_groupnorm's inputs times 2^+-20, its oracle and tolerances"""
    k = K()
    N, H, W, C = shape
    x, xr = _q((E.rnd(shape, 1) * 2 + 0.5) * E.NORM_SCALES[scale], dtype)
    gamma, beta = (E.rnd((C,), 2) * 0.2 + 1).float(), (E.rnd((C,), 3) * 0.1).float()
    dy, dyr = _q(E.rnd(shape, 4), dtype)
    y, mean, rstd = k.groupnorm_fwd(x.reshape(N, H * W, C), gamma.cuda(), beta.cuda(), groups, 1e-3)
    xr.requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = O.group_norm(xr, gr, br, groups, 1e-3)
    _finite(y, mean, rstd)
    close(y.reshape(shape), yr, dtype, "groupnorm fwd", f32_tol=2e-5, bf16_tol=1.2e-2)
    yr.backward(dyr)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = k.groupnorm_bwd(dy.reshape(N, H * W, C), x.reshape(N, H * W, C), gamma.cuda(), mean, rstd, groups, dg, db, accumulate=False)
    _finite(dx, dg, db)
    close(dx.reshape(shape), xr.grad, dtype, "groupnorm dx", f32_tol=5e-5, bf16_tol=2e-2)
    close(dg, gr.grad, dtype, "groupnorm dgamma", f32_tol=5e-5, bf16_tol=2e-2)
    close(db, br.grad, dtype, "groupnorm dbeta", f32_tol=5e-5, bf16_tol=2e-2)


@pytest.mark.parametrize("scale", list(E.NORM_SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 320), (17, 3, 3, 8)])
def test_grn_scaled_inputs(cuda, dtype, shape, scale):
    """test_grn_forward_backward_match_oracle's inputs times 2^+-20, its oracle and tolerances"""
    k = K()
    N, H, W, C = shape
    g = E.gen(sum(shape))
    x = (torch.randn(shape, generator=g) * E.NORM_SCALES[scale]).to(dtype)
    dy = torch.randn(shape, generator=g).to(dtype)
    gamma, beta = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    xc, dyc = x.cuda().reshape(N, H * W, C), dy.cuda().reshape(N, H * W, C)
    y, nx, gx = k.grn_fwd(xc, gamma.cuda(), beta.cuda(), 1e-6)
    dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")      # (a start of 1.0 would swallow gradients of 1e-5)
    dx = k.grn_bwd(dyc, xc, gamma.cuda(), nx, gx, dgamma, dbeta, 1e-6)
    _finite(y, nx, gx, dx, dgamma, dbeta)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = O.grn(xr, gr, br, 1e-6)
    yr.backward(dy.double())

    def rel(a, b):
        return (a.detach().cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-8)

    gxr = torch.sqrt((x.double() ** 2).sum(dim=(1, 2)) + 1e-6)
    assert rel(gx, gxr) < 1e-5
    assert rel(nx, gxr / (gxr.mean(dim=-1, keepdim=True) + 1e-6)) < 1e-5
    lo = dtype == torch.bfloat16
    assert rel(y.reshape(shape), yr.detach()) < (1e-2 if lo else 2e-6)
    assert rel(dx.reshape(shape), xr.grad) < (1e-2 if lo else 1e-5)
    assert rel(dgamma, gr.grad) < 2e-5 + (1e-6 if not lo else 0)
    assert rel(dbeta, br.grad) < 2e-5
