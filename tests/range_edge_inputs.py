"""Seeded CPU builders of range-edge inputs for the kernels that hold an exp, a log, a running maximum or an rsqrt, with the fp64 references
and plain fp32 restatements that tests/test_range_edges_host.py (CPU) and tests/test_range_edges_gpu.py (device) share.  Test infrastructure only.

Every builder rounds its values to the storage dtype BEFORE the fp64 reference sees them (the q() convention of tests/test_kernels_gpu.py) and
returns its rows grouped by regime: a launch holds the regime's rows with ordinary randn * 3 rows alongside as a control, and every group is
compared on its own scale (close() scales its allowance by the largest element of the tensor it is given, so one row with a loss of 1e4 would
otherwise give every other row an absolute allowance of 0.1).

Regimes of a row of logits / scores:
    shifted    an ordinary row plus a per-row constant: +-1e2, +-1e4 in fp32; in bf16 the largest power of two at which every row keeps at least
               three distinct values after rounding (bf16_shift)
    wide       the maximum leads the runner-up by 5 and everything else by >= 200 (all other exp terms underflow fp32); the maximum sits at
               column 0, at the last column, and at a column >= 64 where the row is that long
    confident  the top logit leads the rest by 5, 12, 30 or 200; the label is the top class (loss -> 0) or another one (loss ~ gap)
    degenerate all labels ignored; exactly one valid pixel; a class weight of exactly 0 on the labelled class; rows of identical logits
"""
import math

import torch

LOSS_C = (3, 21, 64, 65, 150)
SOFTMAX_COLS = (9, 49, 64, 65, 197)
LONG_COLS = 1021          # ld 1024: the 32-elements-per-lane variant of the register kernels (ld 513 .. 2048), 3 x 2 rows
FALLBACK_COLS = 2053      # ld 2056 > 2048: the only way onto the one-wave-per-row softmax_fwd_kernel / softmax_bwd_kernel (3 x 2 rows)
ALL_SOFTMAX_COLS = SOFTMAX_COLS + (LONG_COLS, FALLBACK_COLS)
GAPS = (5.0, 12.0, 30.0, 200.0)
FP32_SHIFTS = (1e2, -1e2, 1e4, -1e4)
IGNORE = 255
CLIP_LO, CLIP_HI = 1e-7, 1.0 - 1e-7      # keras.backend.epsilon() clip of the focal cross-entropy
FLT_MIN = 1.17549435e-38
BF16_MAX = 3.3895313892515355e38
# sigmoid(x) is an fp32 denormal for x in [-104, -87.4] (flushed to zero or kept with a few bits): x * sigmoid(x) and the derivatives built on it
# are then wrong by up to 104 * FLT_MIN in absolute terms, which is the floor under the relative bound of the activation grid
ACT_FLOOR = 104 * FLT_MIN
ROWS = 96                                # rows per sub-group: a launch holds a few hundred rows (several workgroups of 4 waves)


# (alpha, gamma) | None, class weights
CE_MODES = {"plain": (None, False), "plain_w": (None, True), "focal_g0": ((0.25, 0.0), False), "focal_g2": ((0.25, 2.0), False),
            "focal_g2_w": ((1.0, 2.0), True)}
# the tolerances of test_softmax_ce_ignore / test_softmax_focal_ce_ignore (tests/test_kernels_gpu.py): (loss px, dlogits), relative to the scale
CE_TOL = {False: (1e-5, 1e-5), True: (2e-5, 5e-5)}
SOFTMAX_TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}      # the defaults of close()
# Groups whose existing tolerance is out of reach of fp32 arithmetic: (kernel family, quantity, group) -> ceiling on the ratio
# (fp32 restatement error) / (tolerance x scale), set just above the worst ratio measured over every C / cols of this file (the measured figure
# is in the comment).  tests/test_range_edges_host.py pins them, and shows that every group NOT listed here meets the existing tolerance in
# fp32; the device tests allow 4 x the restatement's error in the listed groups only, and the existing tolerance everywhere else.
#   plain CE, label on the top class: the loss is ln(1 + ~e^-gap) and the sum 1 + e^-gap is rounded to fp32 (6e-8)
#   focal CE, label on the top class, gap >= 12: 1 - 1e-7 is not an fp32 number (the clip lands on 1 - 1.19e-7)
#   softmax backward, fp32, dP offset by +-100: the dot product ~100 carries 1e-5 of rounding
#   upsample_ce, fp32 logits shifted by +-1e4: interpolating them in fp32 costs ~1e-3 per logit
RESTATEMENT_CEILING = {
    ("ce_plain", "loss", "gap12/hit"): 1200.0,          # 930: 6.9e-7 on losses of ~1e-4
    ("ce_plain", "dlogits", "gap12/hit"): 35.0,         # 27: ~1e-10 absolute
    ("ce_focal", "loss", "gap12/hit"): 300.0,           # 226
    ("ce_focal", "loss", "gap30/hit"): 300.0,           # 240: 4.8e-9 on the clipped loss of 2.5e-8
    ("ce_focal", "loss", "gap200/hit"): 300.0,          # 240
    ("softmax_bwd/fp32", "ds", "ordinary"): 4.0,        # 3.1
    ("softmax_bwd/fp32", "ds", "wide"): 20.0,           # 16: one-hot rows, whose gradients are ~0.03
    ("dcn_bwd/fp32", "ds", "wide peak@0"): 16.0,        # 13
    ("dcn_bwd/fp32", "ds", "wide peak@8"): 20.0,        # 17
    ("upsample_ce/fp32", "dz", "shift+10000/regime"): 3.5,      # 2.8
    ("upsample_ce/fp32", "dz", "shift-10000/regime"): 3.5,      # 2.8
}



def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed), dtype=torch.float64) * scale


def rq(t, dtype):
    """round to the storage dtype, back in fp64"""
    return t.to(dtype).to(torch.float64)


def bf16_shift(rows):
    """largest power-of-two offset at which every row of `rows` [R, C] keeps >= 3 distinct bf16 values (added with either sign)"""
    for e in range(14, 0, -1):
        ok = True
        for sign in (1.0, -1.0):
            v = rq(rows + sign * 2.0 ** e, torch.bfloat16)
            ok = ok and min(len(torch.unique(r)) for r in v) >= 3
        if ok:
            return 2.0 ** e
    raise AssertionError("no bf16 offset keeps three distinct values")


def peak_columns(C):
    cols = [0, C - 1]
    if C > 65:
        cols.append(64 + (C - 65) // 2)
    return cols      # (C = 65: the last column is the one behind the first 64 lanes)


# ---------------------------------------------------------------------------------------------------------------------------
# rows of logits / scores
# ---------------------------------------------------------------------------------------------------------------------------
def control_rows(C, seed, rows=ROWS):
    return rnd((rows, C), seed, 3.0)


def shifted_rows(C, dtype, seed, rows=ROWS):
    """-> (values [n * rows, C] (not yet rounded), {group: row indices}, offsets used)"""
    base = rnd((rows, C), seed, 3.0)
    if dtype == torch.bfloat16:
        s = bf16_shift(base)
        shifts = (s, -s, s / 2, -s / 2)
    else:
        shifts = FP32_SHIFTS
    z = torch.cat([base + s for s in shifts])
    groups = {f"shift{s:+g}": torch.arange(i * rows, (i + 1) * rows) for i, s in enumerate(shifts)}
    return z, groups, shifts


def wide_rows(C, seed, rows=ROWS):
    """the peak at 250 + noise, the runner-up 5 below it, every other column around 0 +- 9: max - min >= 200"""
    out, groups = [], {}
    for i, pc in enumerate(peak_columns(C)):
        z = rnd((rows, C), seed + i, 3.0).clamp(-12, 12)
        peak = 250.0 + rnd((rows,), seed + 10 + i, 2.0)
        z[:, (pc + 1) % C] = peak - 5.0
        z[:, pc] = peak
        groups[f"peak@{pc}"] = torch.arange(i * rows, (i + 1) * rows)
        out.append(z)
    return torch.cat(out), groups


def confident_rows(C, seed, rows=ROWS):
    """-> (z, top column per row, {gapG: rows}): the rest of the row is noise in [-1, 1], the top logit = max(rest) + gap"""
    out, tops, groups = [], [], {}
    for i, gap in enumerate(GAPS):
        z = rnd((rows, C), seed + i, 0.5).clamp(-1, 1)
        top = torch.randint(0, C, (rows,), generator=gen(seed + 20 + i))
        z[torch.arange(rows), top] = -10.0
        z[torch.arange(rows), top] = z.max(-1).values + gap
        groups[f"gap{gap:g}"] = torch.arange(i * rows, (i + 1) * rows)
        out.append(z)
        tops.append(top)
    return torch.cat(out), torch.cat(tops), groups


def random_labels(n, C, seed, ignore_share=0.1):
    g = gen(seed)
    y = torch.randint(0, C, (n,), generator=g, dtype=torch.int32)
    y[torch.rand(n, generator=g) < ignore_share] = IGNORE
    return y


def ce_cases(C):
    """fp32 logits for softmax_ce_ignore / the focal variant.  -> {regime: dict(z fp64 [P, C] of fp32 values, y int32 [P], cw fp32 [C],
    groups {name: row indices})}; every launch ends with a 'control' group of ordinary rows"""
    cases = {}
    cw = (torch.rand(C, generator=gen(77)) + 0.5).float()

    def pack(z, y, groups, cw_=cw):
        ctrl = control_rows(C, 900 + C)
        n = z.shape[0]
        groups = dict(groups)
        groups["control"] = torch.arange(n, n + ctrl.shape[0])
        return dict(z=rq(torch.cat([z, ctrl]), torch.float32), y=torch.cat([y, random_labels(ctrl.shape[0], C, 901 + C)]), cw=cw_, groups=groups)

    z, groups, _ = shifted_rows(C, torch.float32, 100 + C)
    cases["shifted"] = pack(z, random_labels(z.shape[0], C, 101 + C), groups)

    z, groups = wide_rows(C, 200 + C)
    y = random_labels(z.shape[0], C, 201 + C)
    g2 = {}
    for name, idx in groups.items():      # a third of the rows labelled with the peak, a third with the runner-up, the rest anywhere
        pc = int(name.split("@")[1])
        y[idx[0::3]] = pc
        y[idx[1::3]] = (pc + 1) % C
        hit = (y[idx] == pc) | (y[idx] == (pc + 1) % C)
        g2[name + "/near"] = idx[hit]          # loss <= 5.01: label on the peak or the runner-up
        g2[name + "/far"] = idx[~hit]          # loss ~ 250 (or 0: ignored)
    cases["wide"] = pack(z, y, g2)

    z, top, groups = confident_rows(C, 300 + C)
    y = top.to(torch.int32).clone()
    other = (top + 1 + torch.randint(0, C - 1, top.shape, generator=gen(301 + C))) % C
    miss = torch.arange(z.shape[0]) % 2 == 1
    y[miss] = other[miss].to(torch.int32)
    y[torch.arange(z.shape[0]) % 16 == 7] = IGNORE
    g2 = {}
    for name, idx in groups.items():
        g2[name + "/hit"] = idx[~miss[idx]]
        g2[name + "/miss"] = idx[miss[idx]]
    cases["confident"] = pack(z, y, g2)

    # degenerate batches: each is a launch of its own (no control rows: the batch itself is the case)
    z = rq(control_rows(C, 400 + C, 4 * ROWS), torch.float32)
    n = z.shape[0]
    allrows = {"all": torch.arange(n)}
    cases["all_ignored"] = dict(z=z, y=torch.full((n,), IGNORE, dtype=torch.int32), cw=cw, groups=allrows)
    y = torch.full((n,), IGNORE, dtype=torch.int32)
    y[n // 2 + 3] = C - 1
    cases["one_valid"] = dict(z=z, y=y, cw=cw, groups={"valid": torch.tensor([n // 2 + 3]), "ignored": torch.arange(n)[y == IGNORE]})
    y = random_labels(n, C, 402 + C)
    cw0 = cw.clone()
    cw0[1] = 0.0
    y[0::3] = 1
    cases["zero_weight"] = dict(z=z, y=y, cw=cw0, groups={"weight0": torch.arange(n)[y == 1], "others": torch.arange(n)[y != 1]})
    zi = z.clone()
    zi[0::2] = zi[0::2, :1].expand(-1, C)          # rows of identical logits: loss = ln C, gradient 1/C - onehot
    zi[0::4] = 0.0
    cases["identical"] = dict(z=zi, y=random_labels(n, C, 403 + C), cw=cw, groups={"identical": torch.arange(0, n, 2), "control": torch.arange(1, n, 2)})
    return cases


def ce_reference(case, C, focal=None, use_w=False, grad_scale=1.0, dtype=torch.float64):
    """the project's oracle in `dtype` (fp64: the reference; fp32: the plain restatement).  -> (loss_px, dlogits)"""
    from oracle import tf_ops as O

    z = case["z"].to(dtype).clone().requires_grad_(True)
    cw = case["cw"].to(dtype) if use_w else None
    if focal is None:
        lo = O.softmax_ce_ignore(case["y"], z, C, IGNORE, cw)
    else:
        lo = O.softmax_focal_ce_ignore(case["y"], z, C, IGNORE, cw, focal[0], focal[1])
    (lo.sum() * grad_scale).backward()
    return lo.detach().double(), z.grad.double()


def ce_restatement_fp32(case, C, focal=None, use_w=False, grad_scale=1.0):
    """the same formulas in plain fp32 torch: -log_softmax(z)[y] * w (torch's log_softmax subtracts the row maximum first, as the kernel does;
    the oracle's z - logsumexp(z) loses the loss to the rounding of z itself once |z| ~ 1e4); the focal form is the oracle's, in fp32"""
    if focal is not None:
        return ce_reference(case, C, focal, use_w, grad_scale, torch.float32)
    z = case["z"].float().clone().requires_grad_(True)
    y = case["y"].long()
    valid = y != IGNORE
    yc = y.clamp(0, C - 1)
    w = valid.float()
    if use_w:
        w = w * case["cw"].float()[yc]
    lo = -torch.log_softmax(z, -1)[torch.arange(len(y)), yc] * w
    (lo.sum() * grad_scale).backward()
    return lo.detach().double(), z.grad.double()


def restatement_allowance(family, quantity, ref32, ref64, groups):
    """{group: 4 x the fp32 restatement's max error against fp64} for the groups that RESTATEMENT_CEILING lists under (family, quantity) -- those
    whose existing tolerance is out of reach of fp32 arithmetic -- and for no other: everywhere else the existing tolerance holds.  The margin
    covers the accumulation order and the fast exp / log of the device"""
    return {name: 4.0 * group_error(ref32[idx], ref64[idx])[0] for name, idx in groups.items()
            if len(idx) and (family, quantity, name) in RESTATEMENT_CEILING}


def ce_family(focal):
    return "ce_plain" if focal is None else "ce_focal"


def label_probability(case):
    """fp64 softmax probability of the labelled class, NaN at ignored rows"""
    p = torch.softmax(case["z"], -1)
    y = case["y"].long()
    out = p[torch.arange(len(y)), y.clamp(0, p.shape[1] - 1)]
    return torch.where(y == IGNORE, torch.full_like(out, float("nan")), out)


# ---------------------------------------------------------------------------------------------------------------------------
# upsample_ce: the regimes on the low-resolution logits of a 2 x 4 x 4 x 21 map, x8 bilinear to 2 x 32 x 32 pixels
# ---------------------------------------------------------------------------------------------------------------------------
UP_N, UP_HI, UP_WI, UP_C, UP_S = 2, 4, 4, 21, 8
UP_TOL = {torch.float32: (2e-5, 2e-5), torch.bfloat16: (2e-5, 1e-2)}      # tests/test_upsample_ce_gpu.py: (loss sum, dz)


def upsample_ce_launches(dtype):
    """-> [dict(name, z fp64 [2, 4, 4, 21] of dtype values, y int32 [2, 32, 32], cw fp32 [21] | None, groups {name: sample indices})].  Sample 0
    carries the regime's 16 rows and sample 1 ordinary logits; half of the valid labels are the top class of the upsampled pixel.  The
    degenerate batches (all labels ignored, one valid pixel, a zero class weight on the labelled class, identical logits) fill both samples."""
    N, Hi, Wi, C, s = UP_N, UP_HI, UP_WI, UP_C, UP_S
    Ho, Wo = Hi * s, Wi * s
    P = N * Ho * Wo
    from oracle import tf_ops as O

    def labels(zq):
        y = random_labels(P, C, 731).reshape(N, Ho, Wo)
        top = O.resize_bilinear(zq, (Ho, Wo)).argmax(-1).to(torch.int32)
        half = torch.rand(N, Ho, Wo, generator=gen(732)) < 0.5
        return torch.where(half & (y != IGNORE), top, y)

    named = []
    z, groups, _ = shifted_rows(C, dtype, 700, 16)
    named += [(n, z[i]) for n, i in groups.items()]
    z, groups = wide_rows(C, 710, 16)
    named += [("wide " + n, z[i]) for n, i in groups.items()]
    z, _, groups = confident_rows(C, 720, 16)
    named += [(n, z[i]) for n, i in groups.items()]
    ctrl = control_rows(C, 730, 16)
    def two(name):
        return {name + "/regime": torch.tensor([0]), name + "/control": torch.tensor([1])}

    out = []
    for name, rows in named:
        zq = rq(torch.stack([rows, ctrl]).reshape(N, Hi, Wi, C), dtype)
        out.append(dict(name=name, z=zq, y=labels(zq), cw=None, groups=two(name)))
    both = {"batch": torch.arange(N)}
    zq = rq(control_rows(C, 740, 32).reshape(N, Hi, Wi, C), dtype)
    out.append(dict(name="all_ignored", z=zq, y=torch.full((N, Ho, Wo), IGNORE, dtype=torch.int32), cw=None, groups=both))
    y = torch.full((N, Ho, Wo), IGNORE, dtype=torch.int32)
    y[1, 13, 21] = C - 1
    out.append(dict(name="one_valid", z=zq, y=y, cw=None, groups=both))
    cw0 = (torch.rand(C, generator=gen(77)) + 0.5).float()
    cw0[1] = 0.0
    y = labels(zq).reshape(-1)
    y[0::3] = 1
    out.append(dict(name="zero_weight", z=zq, y=y.reshape(N, Ho, Wo), cw=cw0, groups=both))
    zi = zq.clone()
    zi[0] = zi[0, ..., :1].expand(-1, -1, C)      # sample 0: every low-resolution pixel holds one value in all classes, so does every upsampled one
    zi[0, 0] = 0.0
    out.append(dict(name="identical", z=zi, y=random_labels(P, C, 733).reshape(N, Ho, Wo), cw=None, groups=two("identical")))
    return out


def upsample_ce_reference(case, dtype=torch.float64):
    """mean loss and its gradient on the low-resolution logits.  fp64: the oracle's resize + softmax_ce_ignore, as tests/test_upsample_ce_gpu.py;
    fp32: the same resize in fp32 and -log_softmax(z)[y] * w"""
    from oracle import tf_ops as O

    C = UP_C
    N, Ho, Wo = case["y"].shape
    z = case["z"].to(dtype).clone().requires_grad_(True)
    up = O.resize_bilinear(z, (Ho, Wo))
    if dtype == torch.float64:
        loss = O.softmax_ce_ignore(case["y"], up, C, IGNORE, None if case["cw"] is None else case["cw"].double()).mean()
    else:
        y = case["y"].reshape(-1).long()
        yc = y.clamp(0, C - 1)
        w = (y != IGNORE).to(dtype)
        if case["cw"] is not None:
            w = w * case["cw"].to(dtype)[yc]
        loss = (-torch.log_softmax(up.reshape(-1, C), -1)[torch.arange(len(y)), yc] * w).mean()
    loss.backward()
    return loss.detach().double(), z.grad.double()


# ---------------------------------------------------------------------------------------------------------------------------
# DCNv3 mask softmax: G = 4 groups of P = 9 logits per pixel
# ---------------------------------------------------------------------------------------------------------------------------
DCN_G, DCN_P = 4, 9


def dcn_mask_case(dtype):
    """-> (logit rows [(4 + 2 + 1) * 64, 9] of dtype values, one (pixel, group) each; {group: row indices}; the probabilities rounded to dtype,
    which feed the backward; dm = randn + 100 of dtype values)"""
    z1, g1, _ = shifted_rows(DCN_P, dtype, 800, 64)
    z2, g2 = wide_rows(DCN_P, 810, 64)
    ctrl = control_rows(DCN_P, 820, 64)
    rows = rq(torch.cat([z1, z2, ctrl]), dtype)
    n1 = z1.shape[0]
    groups = dict(g1)
    groups.update({"wide " + n: i + n1 for n, i in g2.items()})
    groups["control"] = torch.arange(n1 + z2.shape[0], rows.shape[0])
    p = rq(torch.softmax(rows, -1), dtype)
    dm = rq(rnd((rows.shape[0], DCN_P), 831) + 100.0, dtype)
    return rows, groups, p, dm


# ---------------------------------------------------------------------------------------------------------------------------
# group-wise comparison
# ---------------------------------------------------------------------------------------------------------------------------
def group_error(got, want):
    """(max abs error, close()'s scale) of one group"""
    got, want = got.detach().cpu().double(), want.detach().double()
    return (got - want).abs().max().item(), max(want.abs().max().item(), 1e-6)


def check_groups(got, want, groups, tol, what, overrides=None):
    """every group on its own scale: max err <= tol * max(|want| over the group, 1e-6), the rule of close() applied per group.  overrides
    {group: absolute bound} replace the bound where the rule is unattainable in fp32 arithmetic (4 x the measured fp32-restatement error)"""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    for name, idx in groups.items():
        if len(idx) == 0:
            continue
        err, scale = group_error(got[idx], want[idx])
        bound = tol * scale
        if overrides and name in overrides:
            bound = max(bound, overrides[name])
        assert err <= bound, f"{what} [{name}]: max err {err:.3e} > bound {bound:.3e} (scale {scale:.3e})"


# ---------------------------------------------------------------------------------------------------------------------------
# softmax_rows: scores [problems, Tq, ld] with cols valid columns, bias [heads, Tq, cols], mask [windows, Tq, cols]
# ---------------------------------------------------------------------------------------------------------------------------
SM_HEADS, SM_WINDOWS, SM_B, SM_TQ = 3, 2, 4, 8      # 12 problems x 8 query rows = 96 rows per group


def round_up8(n):
    return (n + 7) // 8 * 8


def softmax_rows_cases(cols, dtype):
    """-> {regime: dict(s fp64 [problems, Tq, cols] of dtype values, groups {name: flat row indices}, bias, mask, clip)}; a launch is
    the regime's problems followed by 12 control problems"""
    tq = SM_TQ if cols < 1000 else 1      # the long rows: one query row per problem, 6 rows per group
    rows = (SM_B if cols < 1000 else SM_WINDOWS) * SM_HEADS * tq
    cases = {}

    def pack(z, groups, **kw):
        ctrl = control_rows(cols, 950 + cols, rows)
        n = z.shape[0]
        groups = dict(groups)
        groups["control"] = torch.arange(n, n + rows)
        s = rq(torch.cat([z, ctrl]), dtype)
        return dict(s=s.reshape(-1, tq, cols), groups=groups, bias=None, mask=None, clip=None, **kw)

    cases["control"] = pack(control_rows(cols, 500 + cols, rows), {"plain": torch.arange(rows)})
    z, groups, _ = shifted_rows(cols, dtype, 510 + cols, rows)
    cases["shifted"] = pack(z, groups)
    z, groups = wide_rows(cols, 520 + cols, rows)
    cases["wide"] = pack(z, groups)
    # bias + Swin-style shift mask of 0 / -100
    c = pack(control_rows(cols, 530 + cols, rows), {"masked": torch.arange(rows)})
    c["bias"] = rnd((SM_HEADS, tq, cols), 531 + cols, 0.5).float()
    m = torch.where(rnd((SM_WINDOWS, tq, cols), 532 + cols) > 0.3, -100.0, 0.0)
    m[:, :, 0] = 0.0      # every row keeps an open column, as a shifted window keeps its own region
    c["mask"] = m.float()
    cases["swin_mask"] = c
    # a mask that leaves one column open: the row is one-hot
    c = pack(control_rows(cols, 540 + cols, rows), {"one_open": torch.arange(rows)})
    m = torch.full((SM_WINDOWS, tq, cols), -100.0)
    open_col = torch.randint(0, cols, (SM_WINDOWS, tq), generator=gen(541 + cols))
    open_col[0, 0], open_col[-1, -1] = 0, cols - 1
    m.scatter_(2, open_col[..., None], 0.0)
    c["mask"], c["open_col"] = m, open_col
    cases["one_open"] = c
    # clip away from its bounds: top ~ 0.87 (clipped to hi), runner-up ~ 0.12 (passes), the rest <= 3e-3 (clipped to lo)
    z = rnd((rows, cols), 550 + cols, 0.5).clamp(-1, 1)
    top = torch.randint(0, cols, (rows,), generator=gen(551 + cols))
    z[torch.arange(rows), top] = 6.0 + math.log(cols)
    z[torch.arange(rows), (top + 1) % cols] = 4.0 + math.log(cols)
    c = pack(z, {"clipped": torch.arange(rows)})
    c["clip"] = (0.02, 0.7)
    cases["clip"] = c
    return cases


def softmax_rows_total(case):
    """scores + bias + mask as the kernel indexes them: problem z uses bias[z % heads] and mask[(z / heads) % windows]"""
    s = case["s"]
    z = torch.arange(s.shape[0])
    a = s.clone()
    if case["bias"] is not None:
        a = a + case["bias"].double()[z % SM_HEADS]
    if case["mask"] is not None:
        a = a + case["mask"].double()[(z // SM_HEADS) % SM_WINDOWS]
    return a


def softmax_rows_reference(case, dtype=torch.float64):
    a = softmax_rows_total(case).to(dtype)
    p = torch.softmax(a, -1)
    if case["clip"] is not None:
        p = p.clamp(case["clip"][0], case["clip"][1])
    return p.reshape(-1, p.shape[-1]).double()


def softmax_bwd_case(cols, dtype, offset=100.0):
    """probabilities of the control / wide rows (rounded to dtype) and dP = randn + a common offset of +-100 per row: dS = P (g - sum g P),
    where the offset cancels against itself to the extent that the rounded probabilities sum to one"""
    rows = 96 if cols < 1000 else 6
    z = torch.cat([control_rows(cols, 560 + cols, rows), wide_rows(cols, 561 + cols, rows)[0][:rows]])
    p = rq(torch.softmax(z, -1), dtype)
    sign = torch.where(torch.arange(2 * rows) % 2 == 0, 1.0, -1.0).double()
    dp = rq(rnd((2 * rows, cols), 562 + cols) + (offset * sign)[:, None], dtype)
    groups = {"ordinary": torch.arange(rows), "wide": torch.arange(rows, 2 * rows)}
    return p, dp, groups


def softmax_bwd_reference(p, dp, clip=None, dtype=torch.float64):
    p, g = p.to(dtype), dp.to(dtype)
    if clip is not None:
        g = torch.where((p > clip[0]) & (p < clip[1]), g, torch.zeros((), dtype=dtype))
    return (p * (g - (g * p).sum(-1, keepdim=True))).double()


# ---------------------------------------------------------------------------------------------------------------------------
# activations: a fixed grid
# ---------------------------------------------------------------------------------------------------------------------------
def act_grid(dtype):
    mags = [1e-30, 1.0, 10.0, 20.0, 87.0, 89.0, 104.0, 1e4, BF16_MAX]
    v = [0.0, -0.0] + [s * m for m in mags for s in (1.0, -1.0)]
    x = torch.tensor(v, dtype=torch.float64)
    x = torch.cat([x, x[:5]])      # 25 values: three 8-wide vectors and a scalar tail
    return rq(x, dtype)


def act_reference(x, act, dtype=torch.float64):
    """-> (value, derivative) of relu / gelu (exact erf) / sigmoid / swish in `dtype`, written so that no intermediate overflows"""
    x = x.to(dtype)
    s = torch.sigmoid(x)
    if act == "relu":
        return torch.relu(x).double(), (x > 0).double()
    if act == "sigmoid":
        return s.double(), (s * torch.sigmoid(-x)).double()
    if act == "swish":
        return (x * s).double(), (s + (x * s) * torch.sigmoid(-x)).double()
    cdf = 0.5 * torch.erfc(-x * math.sqrt(0.5))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    xp = torch.where(pdf == 0, torch.zeros_like(x), x * pdf)
    y = torch.where(cdf == 0, torch.zeros_like(x), x * cdf)
    return y.double(), (cdf + xp).double()


# ---------------------------------------------------------------------------------------------------------------------------
# attention: a dominant key per query, scores up to ~ +-200
# ---------------------------------------------------------------------------------------------------------------------------
def attention_case(B, T, heads, d, positions, seed):
    """bf16 qkv [B, T, 3C] (fp64 copy of the rounded values).  u = +-1 vector per head; key j* of sample b (positions[b % len]) is 2 u, the other
    keys randn; query i is s_i (u + 0.3 n_i) with s_i in [4, 12.5] x sqrt(64 / d): score(i, j*) = s_i (2 sqrt(d) + 0.6 N(0,1)), up to ~200 at
    either head_dim, and the other scores s_i N(0, 1.09): the attention is one-hot to ~e^-30 and the running maximum arrives with key j*"""
    C = heads * d
    g = gen(seed)
    u = torch.where(torch.rand(heads, d, generator=g) < 0.5, -1.0, 1.0).double()
    s = (4.0 + 8.5 * torch.rand(B, T, heads, 1, generator=g, dtype=torch.float64)) * math.sqrt(64.0 / d)
    qh = s * (u + 0.3 * torch.randn(B, T, heads, d, generator=g, dtype=torch.float64))
    kh = torch.randn(B, T, heads, d, generator=g, dtype=torch.float64)
    star = [positions[b % len(positions)] for b in range(B)]
    for b in range(B):
        kh[b, star[b]] = 2.0 * u
    vh = torch.randn(B, T, heads, d, generator=g, dtype=torch.float64) * 1.5
    qkv = torch.cat([t.reshape(B, T, C) for t in (qh, kh, vh)], -1)
    return rq(qkv, torch.bfloat16), star


def attention_scores(qkv, heads, d):
    B, T, _ = qkv.shape
    C = heads * d
    qh, kh = [qkv[..., i * C:(i + 1) * C].reshape(B, T, heads, d).permute(0, 2, 1, 3) for i in range(2)]
    return d ** -0.5 * (qh @ kh.transpose(-1, -2))


# ---------------------------------------------------------------------------------------------------------------------------
# MaskLoss: logits of +-80 / +-1e3 mixed with ordinary ones; an empty, a full and an all-ignored sample
# ---------------------------------------------------------------------------------------------------------------------------
def mask_loss_case(mag, seed=0, B=4, H=9, W=11, C=5):
    """-> (labels int32 [B, H, W], logits fp32 [B, H, W, C], {group: flat pixel indices}).  Samples: 0 mixed labels, 1 every label out of range
    (254: a valid all-negative row -- the label mask is empty), 2 one class everywhere with matching confident logits (the mask is full),
    3 all ignored.  A third of the pixels of every sample carry logits of +-mag, the others randn * 4 clamped to +-12."""
    g = gen(seed)
    z = (torch.randn(B, H, W, C, generator=g) * 4).clamp(-12, 12)
    y = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int32)
    y[torch.rand(B, H, W, generator=g) < 0.15] = IGNORE
    extreme = torch.rand(B, H, W, generator=g) < 0.33
    sign = torch.where(torch.rand(B, H, W, C, generator=g) < 0.5, -1.0, 1.0)
    z = torch.where(extreme[..., None], sign * mag, z)
    y[1] = 254
    y[2] = 2
    z[2, ..., 2] = torch.where(extreme[2], torch.full((), float(mag)), z[2, ..., 2].abs())
    y[3] = IGNORE
    flat = extreme.reshape(-1)
    idx = torch.arange(B * H * W)
    return y, z.float(), {"extreme": idx[flat], "ordinary": idx[~flat]}


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation layers: the project's usual inputs times 2^20 and 2^-20
# ---------------------------------------------------------------------------------------------------------------------------
NORM_SCALES = {"2^20": 2.0 ** 20, "2^-20": 2.0 ** -20}
