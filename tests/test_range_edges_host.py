"""The range-edge builders of tests/range_edge_inputs.py on the host: every regime is reached, the fp64 reference is finite everywhere, and a plain
fp32 restatement of the same formula meets the bound the device test will use -- so a device failure cannot be blamed on an unattainable
tolerance.  Where fp32 arithmetic cannot meet the existing tolerance the measured ratio is pinned by RESTATEMENT_CEILING, per kernel family,
quantity and group; every group that is not listed there meets the existing tolerance."""
import math

import pytest
import torch

from oracle import tf_ops as O
from tests import mask_loss_ref as MR
from tests import range_edge_inputs as E
from tests.test_attention_gpu import _ref_attention
from tests.test_kernels_gpu import close

DTYPES = [torch.float32, torch.bfloat16]


def _ratio_ok(err, scale, tol, key, what):
    """key = (family, quantity, group): 1 x the tolerance unless RESTATEMENT_CEILING lists the key"""
    ceiling = E.RESTATEMENT_CEILING.get(key, 1.0)
    assert err <= ceiling * tol * scale, f"{what} {key}: fp32 restatement error {err:.3e} > {ceiling:g} x {tol:.0e} x {scale:.3e}"


def test_every_listed_ceiling_is_needed():
    """a group is listed only where the fp32 restatement misses the existing tolerance (measured ratio > 1), and the ceiling stays within
    1.5 x of that measurement"""
    worst = {}

    def note(key, err, scale, tol):
        if key in E.RESTATEMENT_CEILING:
            worst[key] = max(worst.get(key, 0.0), err / (tol * scale))

    for C in E.LOSS_C:
        for mode, (focal, use_w) in E.CE_MODES.items():
            tol_px, tol_dz = E.CE_TOL[focal is not None]
            case = E.ce_cases(C)["confident"]
            P = case["z"].shape[0]
            lo, dz = E.ce_reference(case, C, focal, use_w, 0.37 / P)
            lo32, dz32 = E.ce_restatement_fp32(case, C, focal, use_w, 0.37 / P)
            for name, idx in case["groups"].items():
                note((E.ce_family(focal), "loss", name), *E.group_error(lo32[idx], lo[idx]), tol_px)
                note((E.ce_family(focal), "dlogits", name), *E.group_error(dz32[idx], dz[idx]), tol_dz)
    for cols in E.ALL_SOFTMAX_COLS:
        p, dp, groups = E.softmax_bwd_case(cols, torch.float32)
        for clip in (None, (0.02, 0.7)):
            ds, ds32 = E.softmax_bwd_reference(p, dp, clip), E.softmax_bwd_reference(p, dp, clip, torch.float32)
            for name, idx in groups.items():
                note(("softmax_bwd/fp32", "ds", name), *E.group_error(ds32[idx], ds[idx]), E.SOFTMAX_TOL[torch.float32])
    _, groups, p, dm = E.dcn_mask_case(torch.float32)
    w, w32 = E.softmax_bwd_reference(p, dm), E.softmax_bwd_reference(p, dm, dtype=torch.float32)
    for name, idx in groups.items():
        note(("dcn_bwd/fp32", "ds", name), *E.group_error(w32[idx], w[idx]), E.SOFTMAX_TOL[torch.float32])
    for case in E.upsample_ce_launches(torch.float32):
        _, g = E.upsample_ce_reference(case)
        _, g32 = E.upsample_ce_reference(case, torch.float32)
        for name, idx in case["groups"].items():
            note(("upsample_ce/fp32", "dz", name), *E.group_error(g32[idx], g[idx]), E.UP_TOL[torch.float32][1])
    assert set(worst) == set(E.RESTATEMENT_CEILING)
    for key, ceiling in E.RESTATEMENT_CEILING.items():
        assert 1.0 < worst[key] <= ceiling <= 1.5 * worst[key], (key, worst[key], ceiling)


@pytest.mark.parametrize("C", E.LOSS_C)
def test_ce_regimes_are_reached(C):
    cases = E.ce_cases(C)
    z, g = cases["shifted"]["z"], cases["shifted"]["groups"]
    for s in E.FP32_SHIFTS:
        rows = z[g[f"shift{s:+g}"]]
        assert (rows.mean(-1) - s).abs().max() < 12 and (rows.max(-1).values - rows.min(-1).values).min() > 0.5
    z, g = cases["wide"]["z"], cases["wide"]["groups"]
    wide = torch.cat([idx for name, idx in g.items() if name != "control"])
    assert len(wide) == len(E.peak_columns(C)) * E.ROWS
    d = z[wide] - z[wide].max(-1, keepdim=True).values
    assert (d.min(-1).values <= -200).all()
    under = torch.exp(d.float()) == 0
    assert under.any(-1).float().mean().item() == 1.0 and (under.sum(-1) == C - 2).all()      # 100 % of the rows; all but peak and runner-up
    for pc in E.peak_columns(C):
        assert (z[torch.cat([g[f"peak@{pc}/near"], g[f"peak@{pc}/far"]])].argmax(-1) == pc).all()
    assert max(E.peak_columns(C)) >= 64 or C <= 64
    c = cases["confident"]
    p = E.label_probability(c)[torch.cat([idx for name, idx in c["groups"].items() if name != "control"])]
    pv = p[~torch.isnan(p)]
    for b in (E.CLIP_LO, 1 - E.CLIP_HI):      # no labelled probability within a factor 2 of a clip bound, from either side
        for v in (pv, 1 - pv):
            assert not ((v > b / 2) & (v < 2 * b)).any()
    for gap in E.GAPS:
        hit, miss = c["groups"][f"gap{gap:g}/hit"], c["groups"][f"gap{gap:g}/miss"]
        zz = c["z"]
        top2 = zz.topk(2, -1).values
        assert ((top2[:, 0] - top2[:, 1])[torch.cat([hit, miss])] - gap).abs().max() < 1e-4 * max(1.0, gap)
        lab = c["y"][hit].long()
        ok = lab != E.IGNORE
        assert (zz[hit].argmax(-1)[ok] == lab[ok]).all()
        lab = c["y"][miss].long()
        ok = lab != E.IGNORE
        assert (zz[miss].argmax(-1)[ok] != lab[ok]).all() and ok.sum() > 10
    assert (cases["all_ignored"]["y"] == E.IGNORE).all()
    assert (cases["one_valid"]["y"] != E.IGNORE).sum() == 1
    zw = cases["zero_weight"]
    assert zw["cw"][1] == 0 and (zw["y"][zw["groups"]["weight0"]] == 1).all() and len(zw["groups"]["weight0"]) >= 100
    zi = cases["identical"]["z"][cases["identical"]["groups"]["identical"]]
    assert (zi == zi[:, :1]).all()


@pytest.mark.parametrize("C", E.LOSS_C)
@pytest.mark.parametrize("mode", list(E.CE_MODES))
def test_ce_reference_is_finite_and_fp32_restatement_meets_the_device_bound(C, mode):
    focal, use_w = E.CE_MODES[mode]
    tol_px, tol_dz = E.CE_TOL[focal is not None]
    for regime, case in E.ce_cases(C).items():
        P = case["z"].shape[0]
        lo, dz = E.ce_reference(case, C, focal, use_w, 0.37 / P)
        lo32, dz32 = E.ce_restatement_fp32(case, C, focal, use_w, 0.37 / P)
        assert torch.isfinite(lo).all() and torch.isfinite(dz).all() and torch.isfinite(lo32).all() and torch.isfinite(dz32).all()
        assert (lo[case["y"] == E.IGNORE] == 0).all() and (dz[case["y"] == E.IGNORE] == 0).all()
        for name, idx in case["groups"].items():
            if len(idx) == 0:
                continue
            _ratio_ok(*E.group_error(lo32[idx], lo[idx]), tol_px, (E.ce_family(focal), "loss", name), f"{regime} {mode}")
            _ratio_ok(*E.group_error(dz32[idx], dz[idx]), tol_dz, (E.ce_family(focal), "dlogits", name), f"{regime} {mode}")
        mean = lo.mean().item()      # the loss sum holds at the existing tolerance in every launch
        assert abs(lo32.mean().item() - mean) <= tol_px * max(1.0, abs(mean)), (regime, mode)
        if regime == "identical" and focal is None and not use_w:
            idx = case["groups"]["identical"]
            ok = case["y"][idx] != E.IGNORE
            assert (lo[idx][ok] - math.log(C)).abs().max() < 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cols", E.ALL_SOFTMAX_COLS)
def test_softmax_rows_builders(cols, dtype):
    tol = E.SOFTMAX_TOL[dtype]
    cases = E.softmax_rows_cases(cols, dtype)
    for regime, case in cases.items():
        assert torch.equal(case["s"], E.rq(case["s"], dtype))
        p = E.softmax_rows_reference(case)
        p32 = E.softmax_rows_reference(case, torch.float32)
        if dtype == torch.bfloat16:
            p32 = E.rq(p32, dtype)
        assert torch.isfinite(p).all()
        for name, idx in case["groups"].items():
            _ratio_ok(*E.group_error(p32[idx], p[idx]), tol, ("softmax_fwd", "p", name), f"softmax {regime}")
    s = cases["shifted"]
    rows = s["s"].reshape(-1, cols)
    for name, idx in s["groups"].items():
        if name == "control":
            continue
        off = float(name[5:])
        assert abs(off) >= (1e2 if dtype == torch.float32 else 16)
        assert min(len(torch.unique(r)) for r in rows[idx]) >= 3
        assert (rows[idx].mean(-1) - off).abs().max() < max(12.0, abs(off) / 64)
    if dtype == torch.float32:
        assert {float(n[5:]) for n in s["groups"] if n != "control"} == set(E.FP32_SHIFTS)
    w = cases["wide"]
    rows = w["s"].reshape(-1, cols)
    idx = torch.cat([i for n, i in w["groups"].items() if n != "control"])
    d = rows[idx] - rows[idx].max(-1, keepdim=True).values
    assert (d.min(-1).values <= -200).all() and ((torch.exp(d.float()) == 0).sum(-1) == cols - 2).all()
    # one open column: exactly one-hot in fp64 to well within the tolerance
    o = cases["one_open"]
    p = E.softmax_rows_reference(o)[o["groups"]["one_open"]]
    assert (p.max(-1).values >= 1 - 1e-12).all()
    a = E.softmax_rows_total(o).reshape(-1, cols)[o["groups"]["one_open"]]
    assert ((a > -50).sum(-1) == 1).all()
    # clip: no probability within 10 % of a bound (bf16 rounding is 0.4 %), and all three outcomes occur
    c = cases["clip"]
    lo, hi = c["clip"]
    pr = torch.softmax(E.softmax_rows_total(c), -1).reshape(-1, cols)[c["groups"]["clipped"]]
    assert ((pr / lo - 1).abs() > 0.1).all() and ((pr / hi - 1).abs() > 0.1).all()
    assert (pr > hi).any() and (pr < lo).any() and ((pr > lo) & (pr < hi)).any()
    # backward
    p, dp, groups = E.softmax_bwd_case(cols, dtype)
    assert (dp.mean(-1).abs() > 90).all()
    fam = "softmax_bwd/" + ("fp32" if dtype == torch.float32 else "bf16")
    for clip in (None, (0.02, 0.7)):
        ds = E.softmax_bwd_reference(p, dp, clip)
        ds32 = E.softmax_bwd_reference(p, dp, clip, torch.float32)
        if dtype == torch.bfloat16:
            ds32 = E.rq(ds32, dtype)
        assert torch.isfinite(ds).all()
        for name, idx in groups.items():
            _ratio_ok(*E.group_error(ds32[idx], ds[idx]), tol, (fam, "ds", name), "softmax bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_upsample_ce_launches(dtype):
    tag = "fp32" if dtype == torch.float32 else "bf16"
    tol_sum, tol_dz = E.UP_TOL[dtype]
    cases = {c["name"]: c for c in E.upsample_ce_launches(dtype)}
    assert {"all_ignored", "one_valid", "zero_weight", "identical", "gap5", "gap200"} <= set(cases) and len(cases) == 14
    if dtype == torch.float32:
        assert {"shift+10000", "shift-10000", "shift+100", "shift-100"} <= set(cases)
    for name, case in cases.items():
        assert torch.equal(case["z"], E.rq(case["z"], dtype))
        loss, g = E.upsample_ce_reference(case)
        l32, g32 = E.upsample_ce_reference(case, torch.float32)
        if dtype == torch.bfloat16:
            g32 = E.rq(g32, dtype)
        assert torch.isfinite(loss) and torch.isfinite(g).all() and torch.isfinite(l32) and torch.isfinite(g32).all()
        assert abs(l32.item() - loss.item()) <= tol_sum * max(1.0, abs(loss.item())), name
        for gname, idx in case["groups"].items():
            _ratio_ok(*E.group_error(g32[idx], g[idx]), tol_dz, ("upsample_ce/" + tag, "dz", gname), "upsample_ce")
    assert (cases["all_ignored"]["y"] == E.IGNORE).all()
    loss, g = E.upsample_ce_reference(cases["all_ignored"])
    assert loss.item() == 0.0 and (g == 0).all()
    assert (cases["one_valid"]["y"] != E.IGNORE).sum() == 1 and E.upsample_ce_reference(cases["one_valid"])[0].item() > 0
    zw = cases["zero_weight"]
    assert zw["cw"][1] == 0 and (zw["y"] == 1).float().mean() > 0.3
    zi = cases["identical"]["z"][0]
    assert (zi == zi[..., :1]).all()
    wide = O.resize_bilinear(cases["wide peak@0"]["z"], (32, 32))[0]
    assert ((wide.max(-1).values - wide.min(-1).values) >= 200).all()      # the upsampled pixels of the regime's sample stay wide


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_dcn_mask_case(dtype):
    tag = "fp32" if dtype == torch.float32 else "bf16"
    tol = E.SOFTMAX_TOL[dtype]
    rows, groups, p, dm = E.dcn_mask_case(dtype)
    assert rows.shape[0] % E.DCN_G == 0 and torch.equal(rows, E.rq(rows, dtype)) and (dm.mean(-1) > 90).all()
    want = torch.softmax(rows, -1)
    p32 = torch.softmax(rows.float(), -1).double()
    ds, ds32 = E.softmax_bwd_reference(p, dm), E.softmax_bwd_reference(p, dm, dtype=torch.float32)
    if dtype == torch.bfloat16:
        p32, ds32 = E.rq(p32, dtype), E.rq(ds32, dtype)
    assert torch.isfinite(want).all() and torch.isfinite(ds).all()
    for name, idx in groups.items():
        _ratio_ok(*E.group_error(p32[idx], want[idx]), tol, ("dcn_fwd/" + tag, "p", name), "dcn mask softmax")
        _ratio_ok(*E.group_error(ds32[idx], ds[idx]), tol, ("dcn_bwd/" + tag, "ds", name), "dcn mask softmax backward")
        if name.startswith("wide"):
            d = rows[idx] - rows[idx].max(-1, keepdim=True).values
            assert ((torch.exp(d.float()) == 0).sum(-1) == E.DCN_P - 2).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", ["relu", "gelu", "sigmoid", "swish"])
def test_act_grid(act, dtype):
    x = E.act_grid(dtype)
    assert len(x) == 25 and torch.isfinite(x).all() and x.abs().max().item() == E.BF16_MAX
    for m in (1e-30, 87.0, 89.0, 104.0, 1e4):
        assert ((x.abs() / m - 1).abs() < 2.0 ** -8).any()
    assert (x == 0).sum() >= 2 and torch.signbit(x[x == 0]).any()
    y, d = E.act_reference(x, act)
    assert torch.isfinite(y).all() and torch.isfinite(d).all()
    y32, d32 = E.act_reference(x, act, torch.float32)
    assert torch.isfinite(y32).all() and torch.isfinite(d32).all()
    rel = 2e-5
    assert ((y32 - y).abs() <= rel * y.abs() + E.ACT_FLOOR).all() and ((d32 - d).abs() <= rel * d.abs() + E.ACT_FLOOR).all()
    # against autograd of the textbook form where that form does not overflow
    xs = x[x.abs() <= 20].clone().requires_grad_(True)
    f = {"relu": torch.relu, "gelu": lambda t: 0.5 * t * (1 + torch.erf(t * math.sqrt(0.5))), "sigmoid": torch.sigmoid,
         "swish": lambda t: t * torch.sigmoid(t)}[act]
    out = f(xs)
    (g,) = torch.autograd.grad(out.sum(), xs)
    assert (out.detach() - y[x.abs() <= 20]).abs().max() < 1e-12 and (g - d[x.abs() <= 20]).abs().max() < 1e-12


@pytest.mark.parametrize("T,d,positions", [(65, 64, (0, 63, 64)), (130, 64, (5, 127, 129)), (49, 32, (0, 48, 24)), (64, 32, (0, 63, 31))])
def test_attention_case_is_one_hot_at_scores_of_200(T, d, positions):
    heads, B = 3, 3
    qkv, star = E.attention_case(B, T, heads, d, positions, 7)
    assert torch.equal(qkv, E.rq(qkv, torch.bfloat16)) and star == list(positions)
    a = E.attention_scores(qkv, heads, d)
    assert torch.isfinite(a).all()
    top = a.max(-1).values
    assert top.max() > 150 and top.min() > 20
    assert torch.exp(a.float().max()) == float("inf")      # an un-subtracted exp overflows fp32
    p = torch.softmax(a, -1)
    for b in range(B):
        assert (a[b].argmax(-1) == star[b]).all()
        assert (p[b, :, :, star[b]] > 1 - 1e-6).all()
    lead = top - a.topk(2, -1).values[..., 1]
    assert lead.min() > 15
    # the formula in fp32 on the bf16 inputs, output and gradients rounded to bf16, at the bounds of the device test
    C = heads * d
    dy = E.rq(E.rnd((B, T, C), 22), torch.bfloat16)
    qr = qkv.clone().requires_grad_(True)
    yr = _ref_attention(qr, heads, C, d ** -0.5)
    yr.backward(dy)
    q32 = qkv.float().requires_grad_(True)
    y32 = _ref_attention(q32, heads, C, d ** -0.5)
    y32.backward(dy.float())
    y32, g32, gr = E.rq(y32.detach().double(), torch.bfloat16), E.rq(q32.grad.double(), torch.bfloat16), qr.grad
    assert torch.isfinite(yr).all() and torch.isfinite(gr).all()
    assert (y32 - yr.detach()).norm() / yr.norm() < 1.5e-2 and (g32 - gr).norm() / gr.norm() < 3e-2
    for k3 in range(3):
        a_, r_ = g32[..., k3 * C:(k3 + 1) * C], gr[..., k3 * C:(k3 + 1) * C]
        assert (a_ - r_).norm() <= 3e-2 * max(r_.norm(), 1e-3 * gr.norm()), k3


@pytest.mark.parametrize("mag", [80.0, 1e3])
def test_mask_loss_case(mag):
    y, z, groups = E.mask_loss_case(mag)
    assert (z.abs() == mag).any() and len(groups["extreme"]) > 50 and len(groups["ordinary"]) > 50
    assert (z.reshape(-1, z.shape[-1])[groups["extreme"]].abs() == mag).all(-1).sum() >= len(groups["extreme"]) - 99      # (sample 2 keeps its class)
    assert (y[1] == 254).all() and (y[2] == 2).all() and (y[3] == E.IGNORE).all()
    for kw in ({}, dict(apply_focal_ce_loss=True), dict(apply_focal_sigmoid_loss=False), dict(use_sigmoid_loss=False, use_ce_loss=False),
               dict(use_sigmoid_loss=False, use_dice_loss=False)):
        zr = z.double().requires_grad_(True)
        px = MR.mask_loss(y, zr, reduction=True, num_class=5, **kw)
        (g,) = torch.autograd.grad(px.sum(), zr)
        z32 = z.clone().requires_grad_(True)
        px32 = MR.mask_loss(y, z32, reduction=True, num_class=5, **kw)
        (g32,) = torch.autograd.grad(px32.sum(), z32)
        assert torch.isfinite(px).all() and torch.isfinite(g).all() and torch.isfinite(px32).all() and torch.isfinite(g32).all()
        assert (px[3] == 0).all() and (g[3] == 0).all()
        pf, p32f = px.reshape(-1), px32.double().reshape(-1)
        gf, g32f = g.reshape(-1, 5), g32.double().reshape(-1, 5)
        for name, idx in groups.items():
            err, scale = E.group_error(p32f[idx], pf[idx])
            assert err <= 2e-5 * max(1.0, scale), (name, err, scale)
            err, scale = E.group_error(g32f[idx], gf[idx])
            assert err <= 2e-5 * scale, (name, err, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_power_of_two_scales_commute_with_storage_rounding(dtype):
    x = E.rnd((64, 96), 1) * 2 + 0.3
    for s in E.NORM_SCALES.values():
        assert torch.equal(E.rq(x * s, dtype), E.rq(x, dtype) * s)
    # at 2^-20 eps = 1e-6 dominates the variance (4 * 2^-40 ~ 4e-12); at 2^20 the squares are ~ 1e12
    assert (E.rq(x, dtype) * 2.0 ** -20).var(-1).max() < 1e-10 and ((E.rq(x, dtype) * 2.0 ** 20) ** 2).max() > 1e12


@pytest.mark.parametrize("scale", list(E.NORM_SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_norm_references_are_finite_and_fp32_meets_the_device_tolerances(dtype, scale):
    """the oracle calls of the four device tests in fp32 (outputs rounded to the storage dtype) against fp64, at those tests' tolerances"""
    sc = E.NORM_SCALES[scale]

    def both(fn, *ts):
        outs = []
        for dt in (torch.float64, torch.float32):
            leaves = [t.to(dt).clone().requires_grad_(True) for t in ts[:-1]]
            y = fn(*leaves)
            y.backward(ts[-1].to(dt))
            res = [y.detach().double()] + [t.grad.double() for t in leaves]
            outs.append(res if dt == torch.float64 else [E.rq(r, dtype) if i < 2 else r for i, r in enumerate(res)])
        for r in outs[0]:
            assert torch.isfinite(r).all()
        return outs

    x, dy = E.rq((E.rnd((77, 263), 1) * 2 + 0.3) * sc, dtype), E.rq(E.rnd((77, 263), 4), dtype)
    g, b = (E.rnd((263,), 2) * 0.3 + 1).float().double(), (E.rnd((263,), 3) * 0.2).float().double()
    w, r = both(lambda a, c, e: O.layer_norm(a, c, e, 1e-6), x, g, b, dy)
    close(r[0], w[0], dtype, "ln fwd")
    close(r[1], w[1], dtype, "ln dx", f32_tol=1e-4, bf16_tol=2e-2)
    close(r[2], w[2], torch.float32, "ln dgamma", f32_tol=2e-4)
    close(r[3], w[3], torch.float32, "ln dbeta", f32_tol=2e-4)
    x, dy = E.rq(E.rnd((37, 96), 1) * sc, dtype), E.rq(E.rnd((37, 96), 3), dtype)
    w, r = both(lambda a, c: O.rms_norm(a, c, 1e-6), x, (E.rnd((96,), 2) * 0.3).float().double(), dy)
    close(r[0], w[0], dtype, "rmsnorm fwd")
    close(r[1], w[1], dtype, "rmsnorm dx", f32_tol=5e-5, bf16_tol=2e-2)
    close(r[2], w[2], torch.float32, "rmsnorm dscale", f32_tol=5e-5)
    shape = (3, 5, 7, 96)
    x, dy = E.rq((E.rnd(shape, 1) * 2 + 0.5) * sc, dtype), E.rq(E.rnd(shape, 4), dtype)
    g, b = (E.rnd((96,), 2) * 0.2 + 1).float().double(), (E.rnd((96,), 3) * 0.1).float().double()
    w, r = both(lambda a, c, e: O.group_norm(a, c, e, 2, 1e-3), x, g, b, dy)
    close(r[0], w[0], dtype, "groupnorm fwd")
    close(r[1], w[1], dtype, "groupnorm dx", f32_tol=5e-5, bf16_tol=2e-2)
    close(r[2], w[2], torch.float32, "groupnorm dgamma", f32_tol=5e-5)
    close(r[3], w[3], torch.float32, "groupnorm dbeta", f32_tol=5e-5)
    shape = (2, 5, 7, 320)
    x, dy = E.rq(E.rnd(shape, 1) * sc, dtype), E.rq(E.rnd(shape, 4), dtype)
    w, r = both(lambda a, c, e: O.grn(a, c, e, 1e-6), x, (E.rnd((320,), 2) * 0.5).float().double(), (E.rnd((320,), 3) * 0.1).float().double(), dy)
    close(r[0], w[0], dtype, "grn fwd", f32_tol=2e-6, bf16_tol=1e-2)
    close(r[1], w[1], dtype, "grn dx", f32_tol=1e-5, bf16_tol=1e-2)
    close(r[2], w[2], torch.float32, "grn dgamma", f32_tol=2e-5)
    close(r[3], w[3], torch.float32, "grn dbeta", f32_tol=2e-5)
