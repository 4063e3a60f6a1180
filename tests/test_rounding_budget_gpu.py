"""bf16 outputs of the HIP kernels must be THE once-rounded result: the rounding-budget statistic of tests/rounding_budget.py on the device.

close() of tests/test_kernels_gpu.py allows every element 1.5 to 4 bf16 ulps of the LARGEST element; a store that truncates, slab sums kept in
bf16 and an intermediate rounded to bf16 all fit inside it (tests/test_rounding_budget_host.py shows that they do, and that they miss the
conditions below).  Here every output of every case is compared element by element with the fp64 reference rounded once:

    1. share of elements equal to bf16(want64)  >=  1 - 8 (1 - BUDGET[family]), never below 0.95
    2. max |e|  <=  0.5 + 8 (the fp32 restatement's max |e| - 0.5), never above 0.75          (e in ulps of the output; the restatement's
       figure is the family's, family_max_e; no cap where a rounded intermediate never leaves the CU, UNSTORED_MAX_E)
    3. |mean(e sign(want))| and |mean(e)|  <=  6 x 0.2887 / sqrt(n) + (1 - share)              (n: independent errors, Case.independent)
    4. cast fp32 -> bf16: share == 1.0 (BUDGET 1.0), exact ties included

The kernels run through iseg_amd.kernels, the entry points of the parity tests.  Tier-2 families (gelu_approx*, mlp_fused*, dwconv_mfma, attention_*) are compared with the fp64
reference that holds the approximation their kernel comment declares.  Every line printed by a test is
    ROUNDING <family>/<case>:<output> n share max|e| bias_mag bias | floor budget
"""
import ctypes as Ct

import pytest
import torch

from tests import rounding_budget as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def K():
    from iseg_amd import kernels

    return kernels


def plan(k, A, B, D, M, N, Kd, a_kcontig, b_kcontig, ldd):
    """(main loop, reduction splits) the planner answers for this product -- the query of tests/test_gemm_plan_gpu.py"""
    from iseg_amd import _hip

    g = _hip.GemmArgs()
    g.A, g.lda, g.a_kcontig = A.data_ptr(), A.stride(0), a_kcontig
    g.B, g.ldb, g.b_kcontig = B.data_ptr(), B.stride(0), b_kcontig
    g.D, g.ldd = D.data_ptr(), ldd
    g.M, g.N, g.K, g.in_dtype, g.out_dtype, g.batch, g.batch_inner, g.alpha = M, N, Kd, 1, 1, 1, 1, 1.0
    L = _hip.lib()
    return int(L.iseg_gemm_variant(Ct.byref(g))), int(L.iseg_gemm_splits(Ct.byref(g)))


def _epilogue(d, p, M, N):
    kw = {"act": p.get("act", 0)}
    if "bias" in d:
        kw["bias"] = d["bias"]
    if "cs" in d:
        kw.update(colscale=d["cs"], rowscale=d["rs"], rows_per_group=p["rpg"], residual=d["res"])
    if p.get("pre_out"):
        kw["pre_out"] = torch.empty((M, N), dtype=BF, device="cuda")
        kw["pre_deriv"] = bool(p.get("pre_deriv"))
    return kw


def run_dense_fwd(k, d, p):
    M, N, Kd = p["M"], p["N"], p["Kd"]
    kw = _epilogue(d, p, M, N)
    out = {}
    if "concat" in p:
        ld, off = p["concat"]
        cat = torch.zeros((M, ld), dtype=BF, device="cuda")
        y = cat[:, off:off + N]
        k.dense_fwd(d["x"], d["w"], out=y, ldd=ld, **kw)
        assert cat[:, :off].abs().max().item() == 0 and cat[:, off + N:].abs().max().item() == 0, "wrote outside the slice"
    else:
        y = k.dense_fwd(d["x"], d["w"], **kw)
    variant, splits = plan(k, d["x"], d["w"], y, M, N, Kd, 1, 0, y.stride(0))
    assert variant == 0, f"dense_fwd planned onto main loop {variant}, not the register-staged one"
    assert not p.get("split") or splits > 1, f"K = {Kd} was not split"
    out["y"] = y.contiguous()
    if "pre_out" in kw:
        out["pre"] = kw["pre_out"]
    return out


def run_dense_fwd_t(k, d, p):
    M, N, Kd = p["M"], p["N"], p["Kd"]
    wt = d["w"].t().contiguous()
    kw = _epilogue(d, p, M, N)
    y = k.dense_fwd_t(d["x"], wt, kw.pop("bias", None), **kw)
    variant, splits = plan(k, d["x"], wt, y, M, N, Kd, 1, 1, N)
    assert variant != 0, "dense_fwd_t planned onto the register-staged main loop, not the LDS-DMA pipeline"
    assert not p.get("split") or splits > 1, f"K = {Kd} was not split"
    out = {"y": y}
    if "pre_out" in kw:
        out["pre"] = kw["pre_out"]
    return out


def run_dense_dgrad(k, d, p):
    W = d["w"].t().contiguous()      # [N, Kd]: the Keras kernel of the layer whose input gradient this is
    y = k.dense_dgrad(d["x"], W, act=p.get("act", 0), aux=d.get("aux"))
    variant, _ = plan(k, d["x"], W, y, p["M"], p["N"], p["Kd"], 1, 1, p["N"])
    assert variant != 0, "dense_dgrad planned onto the register-staged main loop"
    return {"y": y}


def _zeros(C, n=2):
    return [torch.zeros(C, device="cuda") for _ in range(n)]


def run_layernorm(k, d, p):
    y, _, _ = k.layernorm_fwd(d["x"], d["gamma"], d["beta"], p["eps"])
    dx = k.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], *_zeros(p["C"]), dx_add=d["add"])
    return {"y": y, "dx": dx}


def run_layernorm_post(k, d, p):
    rpg = p["rows"] // 4
    y, _, _ = k.layernorm_post_fwd(d["x"], d["gamma"], d["beta"], p["eps"], colscale=d["cs"], rowscale=d["rs"], rows_per_group=rpg, residual=d["res"])
    dgam, dbet, dcs = _zeros(p["C"], 3)
    dx = k.layernorm_post_bwd(d["dy"], d["x"], d["gamma"], d["beta"], d["mean"], d["rstd"], dgam, dbet, colscale=d["cs"], dcolscale=dcs,
                              rowscale=d["rs"], rows_per_group=rpg)
    return {"y": y, "dx": dx}


def run_layernorm_gather(k, d, p):
    y, _, _ = k.layernorm_gather_fwd(d["x"], d["fwd"], d["gamma"], d["beta"], p["eps"])
    dx = k.layernorm_gather_bwd(d["dy"], d["inv"], d["x"], d["gamma"], d["mean"], d["rstd"], *_zeros(p["C"]), dx_add=d["add"])
    return {"y": y, "dx": dx}


def run_batchnorm(k, d, p):
    rows, C, relu = p["rows"], p["C"], p["relu"]
    y = torch.empty_like(d["x"])
    k.bn_apply_fwd(d["x"], C, d["mean"], d["rstd"], d["gamma"], d["beta"], y, C, rows, C, relu)
    dx = torch.empty_like(d["x"])
    k.bn_bwd_apply(d["dy"], C, d["x"], C, d["yfwd"], C, d["mean"], d["rstd"], d["gamma"], d["sums"], 1.0 / rows, dx, C, rows, C, relu)
    return {"y": y, "dx": dx}


def _x3d(x):
    return x.reshape(x.shape[0], -1, x.shape[-1])


def run_dwconv(k, d, p):
    K_, C = p["K"], p["shape"][3]
    w = d["w"].reshape(K_ * K_, C).contiguous()
    pad = (K_ - 1) // 2
    y = k.dwconv2d(d["x"], w, d["bias"], K_, 1, pad, pad)
    dx = k.dwconv2d(d["dy"], w, None, K_, 1, pad, pad, flip=True, add=d["res"])
    return {"y": y, "dx": dx}


def run_dwconv_strided(k, d, p):
    K_, (_, H, W, C) = p["K"], p["shape"]
    w = d["w"].reshape(K_ * K_, C).contiguous()
    return {"y": k.dwconv2d_strided(d["x"], w, d["bias"], K_, p["stride"], 1),
            "dx": k.dwconv2d_strided_bwd_data(d["dy"], w, K_, p["stride"], 1, H, W)}


def _geom(k, p):
    N, H, W, C = p["shape"]
    Ho, pt = k.same_pad(H, p["K"], p["stride"], p["dil"])
    Wo, pl = k.same_pad(W, p["K"], p["stride"], p["dil"])
    return k.conv_geom(N, H, W, C, p["Cout"], p["K"], p["K"], p["stride"], p["stride"], p["dil"], p["dil"], pt, pl, Ho, Wo, 1)


def run_conv_igemm(k, d, p):
    geom = _geom(k, p)
    assert k.conv2d_igemm_supported(geom, BF)
    out = {"y": k.conv2d_igemm_fwd(d["x"], d["w"], d["bias"], geom), "dx": k.conv2d_igemm_bwd_data(d["dy"], d["w"], geom)}
    if p["kt"]:
        assert k.conv2d_igemm_fwd_kt_supported(geom, BF), "the forward pass has no LDS-DMA form at this shape"
        out["y@kt"] = k.conv2d_igemm_fwd_kt(d["x"], d["w"].reshape(-1, p["Cout"]).t().contiguous(), d["bias"], geom)
    return out


def run_conv_patch(k, d, p):
    geom = _geom(k, p)
    assert k.conv2d_patch_supported(geom, BF, k.PATCH_FWD) and k.conv2d_patch_supported(geom, BF, k.PATCH_BWD_DATA)
    return {"y": k.conv2d_patch_fwd(d["x"], d["w"].reshape(-1, p["Cout"]).t().contiguous(), d["bias"], geom),
            "dx": k.conv2d_patch_bwd_data(d["dy"], d["w"], geom)}


def run_conv_branches(k, d, p):
    N, H, W, C = p["shape"]
    Cout, nb = p["Cout"], len(R.BRANCH_TAPS)

    def table():
        return k.conv_branches(N, H, W, C, Cout, [(kk, kk, dil, dil) for kk, dil in R.BRANCH_TAPS])

    assert k.conv2d_branches_supported(table(), BF)
    ys = k.conv2d_branches_fwd(d["x"], [d[f"w{b}"].reshape(-1, Cout).t().contiguous() for b in range(nb)], table())
    dx = k.conv2d_branches_bwd_data([d[f"dy{b}"].reshape(-1, Cout) for b in range(nb)], [Cout] * nb, [d[f"w{b}"] for b in range(nb)], table())
    return dict({f"y{b}": y for b, y in enumerate(ys)}, dx=dx)


def run_dwconv_mfma(k, d, p):
    w = d["w"].reshape(49, p["shape"][3]).contiguous()
    return {"y": k.dwconv2d7_mfma(d["x"], w, d["bias"], 3, 3), "dx": k.dwconv2d7_mfma(d["dy"], w, None, 3, 3, flip=True, add=d["res"])}


def run_mlp_fused_chain(k, d, p):
    assert k.convnext_mlp_supported(p["C"], BF)
    _, bw = k.convnext_mlp_prep(d["W1"], d["W2"], d["gamma"], backward=True)
    g, dh, dy2 = k.convnext_mlp_bwd(d["y2"], d["dbr"], bw, d["b1"])
    return dict({"g": g} if p.get("with_g") else {}, dh=dh, dy2=dy2)


def run_mlp_fused_fwd(k, d, p):
    assert k.convnext_mlp_supported(p["C"], BF)
    fw, _ = k.convnext_mlp_prep(d["W1"], d["W2"], None, backward=False)
    return {"out": k.convnext_mlp_fwd(d["y2"], fw, d["b1"], d["b2"], d["gamma"], d["rs"], p["M"] // 4, d["res"])}


def run_mlp_fused_bwd_data(k, d, p):
    _, bw = k.convnext_mlp_prep(d["W1"], d["W2"], d["gamma"], backward=True)
    return {"dy2": k.convnext_mlp_bwd_data(d["y2"], d["dbr"], bw, d["b1"])}


def run_attention_flash(k, d, p):
    assert k.attention_fwd_supported(64, BF)
    return {"out": k.attention_fwd(d["qkv"], p["heads"], p["scale"])}


def run_attention_flash_bwd(k, d, p):
    from iseg_amd import _hip

    assert d["lse"].numel() == int(_hip.lib().iseg_attention_lse_elems(p["B"], p["T"], p["heads"]))
    C = p["heads"] * 64
    dqkv = k.attention_bwd(d["qkv"], d["out_fwd"], d["dout"], d["lse"].reshape(-1), p["heads"], p["scale"])
    return {"dq": dqkv[..., :C].contiguous(), "dk": dqkv[..., C:2 * C].contiguous(), "dv": dqkv[..., 2 * C:].contiguous()}


def run_attention_self(k, d, p):
    assert k.self_attention_supported(64, p["dv"], BF)
    return {"out": k.self_attention_fwd(d["q"], d["k"], d["v"], p["scale"], False)[0]}


def run_attention_self_bwd(k, d, p):
    from iseg_amd import _hip

    assert d["lse"].numel() == int(_hip.lib().iseg_self_attention_lse_elems(p["B"], p["T"]))
    dq, dk, dv = k.self_attention_bwd(d["q"], d["k"], d["v"], d["out_fwd"], d["dout"], d["lse"].reshape(-1), p["scale"])
    return {"dq": dq, "dk": dk, "dv": dv}


def run_attention_window(k, d, p):
    assert k.window_attention_supported(p["T"], 32, BF)
    C = p["heads"] * 32
    table = k.window_attention_table(d["bias"], None, p["heads"], p["T"])
    dqkv, _ = k.window_attention_bwd(d["qkv"], table, d["dout"], p["heads"], p["scale"])
    return {"out": k.window_attention_fwd(d["qkv"], table, p["heads"], p["scale"]), "dq": dqkv[..., :C].contiguous(),
            "dk": dqkv[..., C:2 * C].contiguous(), "dv": dqkv[..., 2 * C:].contiguous()}


def run_glu(k, d, p):
    dg, dx = torch.empty_like(d["g"]), torch.empty_like(d["g"])
    k.glu_bwd(d["dout"], d["g"], d["x"], dg, dx, R.ACT_GELU)
    return {"out": k.glu_fwd(d["g"], d["x"], R.ACT_GELU), "dg": dg, "dx": dx}


def run_upsample_ce(k, d, p):
    N, Hi, Wi, C = p["shape"]
    Ho, Wo = Hi * p["s"], Wi * p["s"]
    assert k.upsample_ce_supported(Hi, Wi, Ho, Wo, C)
    _, dz = k.upsample_ce(d["z"], d["y"], Ho, Wo, R.UP_IGNORE, sum_scale=1.0 / (N * Ho * Wo), grad_scale=1.0 / (N * Ho * Wo))
    return {"dz": dz}


def run_broadcast_rows(k, d, p):
    B, R = p["B"], p["R"]
    y = torch.zeros((B, R, 96), dtype=BF, device="cuda")
    k.broadcast_rows(d["v"], y, 96, R * 96, B, R, 96, scale=p["scale"])
    return {"y": y}


def _sampling(p):
    from tests import sampling_kinks as SK

    return next(c for c in SK.CASES if c.op == p["op"] and c.kind == "budget").p


def run_dcnv3(k, d, p):
    q = _sampling(p)
    G = q["G"]
    return {"y": k.dcnv3_fwd(d["x"], d["offset"], d["mask"], G, d["x"].shape[3] // G, 3, 3, 1, 1, 1, 1.0)}


def run_dcnv3_bwd(k, d, p):
    q = _sampling(p)
    G = q["G"]
    _, doff, dmask = k.dcnv3_bwd(d["x"], d["offset"], d["mask"], d["dout"], G, d["x"].shape[3] // G, 3, 3, 1, 1, 1, 1.0)      # (dx: fp32, not a case)
    return {"dmask": dmask, "doffset": doff}


def run_defattn(k, d, p):
    q = _sampling(p)
    return {"out": k.defattn_fwd(d["value"], d["offset"], d["attn"], q["heads"], q["P"], q["orf"])}


def run_defattn_bwd(k, d, p):
    q = _sampling(p)
    dvalue, doff, dattn = k.defattn_bwd(d["value"], d["offset"], d["attn"], d["dout"], q["heads"], q["P"], q["orf"])
    return {"dvalue": dvalue, "dattn": dattn, "doffset": doff}


RUN = {
    "dcnv3": run_dcnv3,
    "dcnv3_bwd": run_dcnv3_bwd,
    "dcnv2_sample": lambda k, d, p: {"col": k.dcnv2_sample_fwd(d["x"], d["offset"])},
    "dcnv2_sample_bwd": lambda k, d, p: {"doff": k.dcnv2_sample_bwd(d["x"], d["offset"], d["dout"])[1]},
    "defattn": run_defattn,
    "defattn_bwd": run_defattn_bwd,
    "cast": lambda k, d, p: {"y": k.cast(d["x"], BF)},
    "axpby": lambda k, d, p: {"y": k.axpby(d["a"], d["b"], p["alpha"], p["beta"])},
    "add_relu": lambda k, d, p: {"y": k.add_relu(d["a"], d["b"])},
    "rowscale": lambda k, d, p: {"y": k.rowscale(d["x"], d["s"], p["rpg"])},
    "broadcast_rows": run_broadcast_rows,
    "act_fwd": lambda k, d, p: {"y": k.act_fwd(d["x"], p["act"])},
    "act_bwd": lambda k, d, p: {"dx": k.act_bwd(d["dy"], d["x"], p["act"])},
    "dense_fwd": run_dense_fwd,
    "dense_fwd_t": run_dense_fwd_t,
    "dense_dgrad": run_dense_dgrad,
    "layernorm": run_layernorm,
    "layernorm_post": run_layernorm_post,
    "layernorm_gather": run_layernorm_gather,
    "batchnorm": run_batchnorm,
    "groupnorm": lambda k, d, p: {"y": k.groupnorm_fwd(_x3d(d["x"]), d["gamma"], d["beta"], p["groups"], 1e-3)[0]},
    "rmsnorm": lambda k, d, p: {"y": k.rmsnorm_fwd(d["x"], d["scale"], 1e-6)[0]},
    "grn": lambda k, d, p: {"y": k.grn_fwd(_x3d(d["x"]), d["gamma"], d["beta"], 1e-6)[0]},
    "dwconv": run_dwconv,
    "dwconv_strided": run_dwconv_strided,
    "conv_igemm": run_conv_igemm,
    "conv_patch": run_conv_patch,
    "conv_branches": run_conv_branches,
    "dwconv_mfma": run_dwconv_mfma,
    "mlp_fused_chain": run_mlp_fused_chain,
    "mlp_fused_fwd": run_mlp_fused_fwd,
    "mlp_fused_bwd_data": run_mlp_fused_bwd_data,
    "attention_flash": run_attention_flash,
    "attention_flash_bwd": run_attention_flash_bwd,
    "attention_window": run_attention_window,
    "attention_self": run_attention_self,
    "attention_self_bwd": run_attention_self_bwd,
    "glu": run_glu,
    "upsample_ce": run_upsample_ce,
    "resize": lambda k, d, p: {"y": k.resize_bilinear(d["x"], *p["out"]), "dx": k.resize_bilinear_bwd(d["dy"], p["shape"][1], p["shape"][2], BF)},
}
assert {c.kind for c in R.CASES} <= set(RUN)


def check(c):
    k = K()
    d = {name: (v.cuda() if torch.is_tensor(v) else v) for name, v in c.inputs().items()}
    got = RUN[c.kind](k, d, c.p)
    torch.cuda.synchronize()
    got = c.selected(got)
    fed = c.fed(got)
    want = c.outputs(torch.float64, fed) if fed else {name: ref for name, (_, ref, _) in R.restated(c).items()}
    assert {name.split("@")[0] for name in got} == set(want)
    bad = []
    for name, g in got.items():
        ref = want[name.split("@")[0]]
        assert g.dtype == BF and g.numel() == ref.numel(), f"{c.id}:{name}: {g.dtype} {tuple(g.shape)}"
        g = g.detach().cpu()
        st = R.rounding_stats(g, ref)
        line = R.report(f"{c.id}:{name}", g, ref, st)
        print(f"ROUNDING {c.id}:{name} n {ref.numel()} share {st.share:.6f} max|e| {st.max_abs_e:.5f} bias_mag {st.bias_mag:+.5f} bias {st.bias:+.5f} "
              f"| floor {R.share_floor(c.family):.6f} budget {R.BUDGET[c.family]}")
        why = R.failures(st, ref.numel(), c.family, R.family_max_e(c.family), c.independent())
        if why:
            bad.append(line + "\n    -> " + "; ".join(why))
    assert not bad, "\n".join(bad)


def _family_test(family):
    @pytest.mark.parametrize("c", R.family_cases(family), ids=lambda c: c.name)
    def test(cuda, c):
        check(c)

    test.__doc__ = f"every bf16 output of the `{family}` kernels is the once-rounded value of its tier-{R.family_cases(family)[0].tier} reference"
    return test


for _family in R.FAMILIES:
    globals()[f"test_rounding_budget_{_family}"] = _family_test(_family)
del _family
