"""HIP kernels vs the fp64 reference on operands that already hold a NaN or an infinity (cases, references and the deviations table:
tests/nonfinite_cases.py; what the table must satisfy on its own: tests/test_nonfinite_host.py).

Per case: the CLASS MASK of every output (finite / NaN / +Inf / -Inf) equals the reference's exactly -- or the pinned expectation of a
DEVIATIONS entry -- and the finite elements meet the tolerance of the kernel's existing parity test, on the scale of the largest finite
reference element.  No tolerance is new.

On the kernels before the NaN-keeping ReLU / clip (fmaxf and fminf return the operand that is not NaN) 94 of the 621 cases fail: every relu case
of gemm_fwd and gemm_dma, act_fwd-relu, add_relu, bn_apply / bn_finalize_apply (relu: the NaN; linear: a NaN variance clamped to 0 under +-Inf),
bn_infer_apply, bn_relu_upsample_add-*-z, resblock_tail, relu_dwconv3, relu_dwconv3_bwd, clip_fwd, softmax_rows_fwd-*-clip,
softmax_ce-*-focal-valid (loss and gradient), mask_loss-ce-focal, gemm_dgrad-gelu_grad-aux and act_bwd-gelu*-aux in bf16 (the clamp of the polynomial
derivative), and, from 0 * NaN at a clamped address, resize_bilinear_bwd-18x22-to-9x11-hp and upsample_ce."""
import pytest
import torch

from tests import nonfinite_cases as NF

pytestmark = pytest.mark.gpu

PARAMS, IDS = NF.params()


def K():
    from iseg_amd import kernels

    return kernels


class Dev:
    """device copies of a built case's inputs in their storage dtypes"""

    def __init__(self, b):
        self.b = b

    def __getitem__(self, name):
        v = self.b.inputs[name]
        return v.to(self.b.in_dtypes.get(name, self.b.dtype)).cuda() if torch.is_tensor(v) else v


# ---------------------------------------------------------------------------------------------------------------------------
# runners: family -> (kernels module, device inputs, built case) -> {output name: device tensor}
# ---------------------------------------------------------------------------------------------------------------------------
def run_gemm_fwd(k, d, b):
    epi = d["epi"]
    if epi == "none":
        return {"y": k.dense_fwd(d["x"], d["w"], d["bias"])}
    if epi == "relu":
        return {"y": k.dense_fwd(d["x"], d["w"], d["bias"], act=k.ACT_RELU)}
    if epi == "gelu_pre":
        x = d["x"]
        pre = torch.empty((x.shape[0], d["w"].shape[1]), dtype=x.dtype, device="cuda")
        return {"y": k.dense_fwd(x, d["w"], d["bias"], act=k.ACT_GELU, pre_out=pre), "pre": pre}
    return {"y": k.dense_fwd(d["x"], d["w"], d["bias"], colscale=d["cs"], rowscale=d["rs"], rows_per_group=d["G"], residual=d["res"])}


def run_gemm_dgrad(k, d, b):
    return {"dx": k.dense_dgrad(d["dy"], d["w"], act=d["act"], aux=d["aux"])}


def run_gemm_wgrad(k, d, b):
    x, dy = d["x"], d["dy"]
    M, Kd = x.shape
    N = dy.shape[1]
    dW = torch.full((Kd, N), 0.5, dtype=torch.float32, device="cuda")
    if d["bias_grad"]:
        db = torch.full((N,), -1.0, dtype=torch.float32, device="cuda")
        k.dense_wgrad(x, dy, dW, bias_grad=db)
        return {"dW": dW, "db": db}
    k.gemm(x, dy, dW, Kd, N, M, lda=x.stride(0), ldb=dy.stride(0), ldd=N, a_kcontig=0, b_kcontig=0, accumulate=True, split_k=3)
    return {"dW": dW}


def run_gemm_dma(k, d, b):
    import ctypes as C

    from iseg_amd import _hip

    x, wt, bias = d["x"], d["wt"], d["bias"]
    (M, Kd), N = x.shape, wt.shape[0]
    out = torch.empty((M, N), dtype=x.dtype, device="cuda")
    g = k._gemm_args(x, wt, out, M, N, Kd, lda=Kd, ldb=Kd, ldd=N, a_kcontig=1, b_kcontig=1, bias=bias, act=k.ACT_RELU)
    assert _hip.lib().iseg_gemm_variant(C.byref(g)) == d["form"], "the problem no longer takes the LDS-DMA form it is listed under"
    return {"y": k.dense_fwd_t(x, wt, bias, act=k.ACT_RELU, out=out)}


def run_layernorm(k, d, b):
    x, g = d["x"], d["gamma"]
    y, mean, rstd = k.layernorm_fwd(x, g, d["beta"], 1e-6)
    dgam, dbet = torch.zeros_like(g), torch.zeros_like(g)
    dx = k.layernorm_bwd(d["dy"], x, g, mean, rstd, dgam, dbet)
    return {"y": y, "dx": dx, "dgamma": dgam, "dbeta": dbet}


def run_layernorm_post(k, d, b):
    y, _, _ = k.layernorm_post_fwd(d["x"], d["gamma"], d["beta"], 1e-6, colscale=d["cs"], rowscale=d["rs"], rows_per_group=d["rpg"], residual=d["res"])
    return {"y": y}


def run_rmsnorm(k, d, b):
    x, sc = d["x"], d["scale"]
    y, rstd = k.rmsnorm_fwd(x, sc, 1e-6)
    ds = torch.zeros_like(sc)
    dx = k.rmsnorm_bwd(d["dy"], x, sc, rstd, ds, accumulate=False)
    return {"y": y, "dx": dx, "dscale": ds}


def run_groupnorm(k, d, b):
    x = d["x"]
    N, H, W, C = x.shape
    y, _, _ = k.groupnorm_fwd(x.reshape(N, H * W, C), d["gamma"], d["beta"], d["groups"], 1e-3)
    return {"y": y.reshape(N, H, W, C)}


def run_grn(k, d, b):
    x = d["x"]
    N, H, W, C = x.shape
    y, nx, gx = k.grn_fwd(x.reshape(N, H * W, C), d["gamma"], d["beta"], 1e-6)
    return {"y": y.reshape(N, H, W, C), "nx": nx, "gx": gx}


def run_bn_apply(k, d, b):
    x = d["x"]
    rows, C = x.shape
    mean, rstd = k.bn_finalize(k.bn_stats(x, C, rows, C), C, 1e-3, 0.9, None, None)
    y = torch.empty_like(x)
    k.bn_apply_fwd(x, C, mean, rstd, d["gamma"], d["beta"], y, C, rows, C, d["relu"])
    return {"y": y}


def run_bn_finalize_apply(k, d, b):
    x = d["x"]
    rows, C = x.shape
    y = torch.empty_like(x)
    k.bn_finalize_apply(k.bn_stats(x, C, rows, C), x, C, d["gamma"], d["beta"], y, C, rows, C, 1e-3, 0.9, None, None, d["relu"])
    return {"y": y}


def run_bn_infer_apply(k, d, b):
    x = d["x"]
    rows, C = x.shape
    y = torch.empty_like(x)
    k.bn_apply_fwd(x, C, d["mean"], d["rstd"], d["gamma"], d["beta"], y, C, rows, C, True)
    return {"y": y}


def run_softmax_fwd(k, d, b):
    s, cols, ld = d["s"], d["cols"], d["ld"]
    rows = s.shape[0]
    buf = torch.zeros((1, rows, ld), dtype=s.dtype, device="cuda")
    buf[0, :, :cols] = s
    out = torch.full((1, rows, ld), NF.NAN, dtype=s.dtype, device="cuda")
    k.softmax_rows_fwd(buf, 1, rows, cols, ld, clip=(1e-7, 1.0 - 1e-7) if d["clip"] else None, out=out)
    assert (out[0, :, cols:] == 0).all(), "pad columns are not zero"
    return {"p": out[0, :, :cols]}


def run_softmax_bwd(k, d, b):
    p, dp, cols, ld = d["p"], d["dp"], d["cols"], d["ld"]
    rows = p.shape[0]
    pb, db = torch.zeros((rows, ld), dtype=p.dtype, device="cuda"), torch.zeros((rows, ld), dtype=p.dtype, device="cuda")
    pb[:, :cols], db[:, :cols] = p, dp
    out = torch.full((rows, ld), NF.NAN, dtype=p.dtype, device="cuda")
    k.softmax_rows_bwd(pb, db, rows, cols, ld, out=out)
    return {"ds": out[:, :cols]}


def run_softmax_ce(k, d, b):
    z = d["z"]
    grad = "dz" in b.want
    px, sm, dz = k.softmax_ce_ignore(z, d["y"], NF.IGNORE, want_px=True, want_sum=True, sum_scale=1.0 / z.shape[0], want_grad=grad,
                                     grad_scale=1.0 / z.shape[0], focal=d["focal"])
    return {"px": px, "sum": sm, "dz": dz} if grad else {"px": px, "sum": sm}


def run_resblock_tail(k, d, b):
    assert k.resblock_tail_supported(d["z2"].shape[-1], d["stride"], b.dtype)
    bn0 = (d["mean0"], d["rstd0"], d["gamma0"], d["beta0"]) if d["bn0"] else None
    return {"out": k.resblock_tail_fwd(d["z2"], d["mean2"], d["rstd2"], d["gamma2"], d["beta2"], d["sc"], d["stride"], bn0=bn0)}


def run_relu_dwconv3(k, d, b):
    x = d["x"]
    assert k.sepconv_supported(*x.shape, d["stride"], 1, b.dtype)
    z, _ = k.relu_dwconv3_stats(x, d["w"], d["stride"], 1, stats=True)
    return {"z": z}


def run_relu_dwconv3_bwd(k, d, b):
    x = d["x"]
    C = x.shape[-1]
    assert k.sepconv_supported(*x.shape, d["stride"], 1, b.dtype)
    dw = torch.zeros((9, C), dtype=torch.float32, device="cuda")
    sums = torch.zeros(2 * C, dtype=torch.float32, device="cuda")
    dx = k.bnfold_dwconv3_relu_bwd(d["D"], d["z"], x, d["w"], d["mean"], d["rstd"], d["gamma"], sums, 0.0, False, dw, d["stride"], 1)
    return {"dx": dx, "dw": dw}


def run_mask_loss(k, d, b):
    px, mean, _ = k.mask_loss(d["z"], d["y"], NF.IGNORE, d["flags"], (0.0, 0.0, 1.0), want_px=True, want_mean=True)
    return {"px": px, "mean": mean}


def run_conv_igemm(k, d, b):
    x, w = d["x"], d["w"]
    N, H, W, Cin = x.shape
    kk, Cout = w.shape[0], w.shape[3]
    geom = k.conv_geom(N, H, W, Cin, Cout, kk, kk, 1, 1, 1, 1, kk // 2, kk // 2, H, W, 1)
    assert k.conv2d_igemm_supported(geom, b.dtype)
    if d["which"] == "fwd":
        return {"y": k.conv2d_igemm_fwd(x, w, d["bias"], geom)}
    return {"dx": k.conv2d_igemm_bwd_data(d["dy"], w, geom)}


def run_upsample_ce(k, d, b):
    z = d["z"]
    N, Hi, Wi, C = z.shape
    Ho, Wo = d["Ho"], d["Wo"]
    assert k.upsample_ce_supported(Hi, Wi, Ho, Wo, C)
    P = N * Ho * Wo
    s, dz = k.upsample_ce(z, d["y"], Ho, Wo, NF.IGNORE, sum_scale=1.0 / P, grad_scale=1.0 / P)
    return {"dz": dz, "sum": s}


def run_window_attention(k, d, b):
    qkv = d["qkv"]
    T, heads = qkv.shape[1], d["heads"]
    assert k.window_attention_supported(T, qkv.shape[2] // 3 // heads, b.dtype)
    table = k.window_attention_table(d["bias"], d["shift"], heads, T)
    return {"out": k.window_attention_fwd(qkv, table, heads, d["scale"])}


def run_gemma_attention(k, d, b):
    assert k.gemma_attention_supported(d["nq"], d["nkv"], d["h"], b.dtype)
    return {"out": k.gemma_attention_fwd(d["qkv"], d["pad"], d["nq"], d["nkv"], d["h"], d["scale"], False)[0]}


def run_conv_patch(k, d, b):
    x, w, kk = d["x"], d["w"], d["k"]
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    geom = k.conv_geom(N, H, W, Cin, Cout, kk, kk, kk, kk, 1, 1, 0, 0, H // kk, W // kk, 1)
    assert k.conv2d_patch_supported(geom, b.dtype, k.PATCH_FWD)
    return {"y": k.conv2d_patch_fwd(x, w.reshape(-1, Cout).t().contiguous(), d["bias"], geom)}


def run_conv_branches(k, d, b):
    x, taps = d["x"], d["taps"]
    ws = [d[f"w{i}"] for i in range(len(taps))]
    table = k.conv_branches(*x.shape, ws[0].shape[3], [(kk, kk, dil, dil) for kk, dil in taps])
    assert k.conv2d_branches_supported(table, b.dtype)
    ys = k.conv2d_branches_fwd(x, [w.reshape(-1, w.shape[3]).t().contiguous() for w in ws], table)
    return {f"y{i}": y for i, y in enumerate(ys)}


def run_jpu(k, d, b):
    x = d["x"]
    assert k.jpu_supported(*x.shape, b.dtype)
    z, _ = k.jpu_dwconv3x4_stats(x, d["w"], d["bias"], stats=True)
    return {"z": z}


def run_bn_swish_se(k, d, b):
    x = d["x"]
    N, H, W, C = x.shape
    assert k.mbconv_supported(N, H * W, C, d["W1"].shape[1])
    return {"out": k.bn_swish_se_fwd(x, d["mean"], d["rstd"], d["gamma"], d["beta"], d["W1"], d["b1"], d["W2"], d["b2"])[0]}


def run_pool(k, d, b):
    mode = k.POOL_AVG if d["mode"] == "avg" else k.POOL_MAX
    return {"y": k.pool2d_fwd(d["x"], d["k"], d["k"], d["s"], d["s"], d["pt"], d["pl"], d["Ho"], d["Wo"], mode)}


RUN = {
    "resblock_tail": run_resblock_tail,
    "relu_dwconv3": run_relu_dwconv3,
    "dwconv2d": lambda k, d, b: {"y": k.dwconv2d(d["x"], d["w"], d["bias"], d["K"], d["dil"], d["pad"], d["pad"])},
    "dwconv2d_strided": lambda k, d, b: {"y": k.dwconv2d_strided(d["x"], d["w"], d["bias"], d["K"], d["stride"], 1)},
    "resize_bilinear": lambda k, d, b: {"y": k.resize_bilinear(d["x"], d["Ho"], d["Wo"], out_dtype=torch.float32, align_corners=d["align"])},
    "pool2d_fwd": run_pool,
    "dwconv2d7_mfma": lambda k, d, b: {"y": k.dwconv2d7_mfma(d["x"], d["w"], d["bias"])},
    "jpu_dwconv3x4_stats": run_jpu,
    "bn_swish_se_fwd": run_bn_swish_se,
    "conv2d_patch_fwd": run_conv_patch,
    "conv2d_branches_fwd": run_conv_branches,
    "window_attention_fwd": run_window_attention,
    "gemma_attention_fwd": run_gemma_attention,
    "conv2d_igemm": run_conv_igemm,
    "upsample_ce": run_upsample_ce,
    "relu_dwconv3_bwd": run_relu_dwconv3_bwd,
    "mask_loss": run_mask_loss,
    "resize_bilinear_bwd": lambda k, d, b: {"dx": k.resize_bilinear_bwd(d["dy"], d["H"], d["W"], b.dtype, align_corners=d["align"])},
    "attention_fwd": lambda k, d, b: {"out": k.attention_fwd(d["qkv"], d["heads"], d["scale"])},
    "self_attention_fwd": lambda k, d, b: {"out": k.self_attention_fwd(d["q"], d["k"], d["v"], d["scale"], False)[0]},
    "gemm_fwd": run_gemm_fwd,
    "gemm_dgrad": run_gemm_dgrad,
    "gemm_wgrad": run_gemm_wgrad,
    "gemm_dma": run_gemm_dma,
    "act_fwd": lambda k, d, b: {"y": k.act_fwd(d["x"], d["act"])},
    "act_bwd": lambda k, d, b: {"dx": k.act_bwd(d["dy"], d["aux"], d["act"])},
    "add_relu": lambda k, d, b: {"y": k.add_relu(d["a"], d["b"])},
    "clip_fwd": lambda k, d, b: {"y": k.clip_fwd(d["x"], *NF.CLIP)},
    "clip_bwd": lambda k, d, b: {"dx": k.clip_bwd(d["x"], d["dy"], *NF.CLIP)},
    "glu_fwd": lambda k, d, b: {"out": k.glu_fwd(d["gate"], d["x"], d["act"])},
    "layernorm": run_layernorm,
    "layernorm_post": run_layernorm_post,
    "rmsnorm": run_rmsnorm,
    "groupnorm_fwd": run_groupnorm,
    "grn_fwd": run_grn,
    "bn_apply": run_bn_apply,
    "bn_finalize_apply": run_bn_finalize_apply,
    "bn_infer_apply": run_bn_infer_apply,
    "bn_relu_upsample_add": lambda k, d, b: {"y": k.bn_relu_upsample_add(d["z"], d["mean"], d["rstd"], d["gamma"], d["beta"], d["xc"])},
    "softmax_rows_fwd": run_softmax_fwd,
    "softmax_rows_bwd": run_softmax_bwd,
    "softmax_ce": run_softmax_ce,
}


def check(got, want, tol, what, elementwise=None):
    g = got.detach().to("cpu", torch.float64)
    w = want.to(torch.float64)
    assert tuple(g.shape) == tuple(w.shape), f"{what}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
    cg, cw = NF.classes(g), NF.classes(w)
    bad = cg != cw
    if bad.any():
        first = tuple(int(i) for i in bad.nonzero()[0])
        names = ("finite", "NaN", "+Inf", "-Inf")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements are in the wrong class, the first at {first}: "
                             f"{names[int(cg[first])]} ({g[first].item()}), the reference has {names[int(cw[first])]} ({w[first].item()})")
    fin = cw == 0
    if fin.any():
        scale = max(w[fin].abs().max().item(), 1e-6)
        err = (g[fin] - w[fin]).abs().max().item()
        print(f"{what}: {int((~fin).sum())} non-finite of {fin.numel()}, max err on the rest {err:.3e} (allowed {tol * scale:.3e})")
        if elementwise is not None:
            rel, floor = elementwise
            over = (g[fin] - w[fin]).abs() - (rel * w[fin].abs() + floor)
            assert over.max().item() <= 0, f"{what}: {int((over > 0).sum())} finite elements miss |err| <= {rel:.2e} |want| + {floor:.0e}"
            return
        assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.1e} * scale {scale:.3e} over the finite elements"


@pytest.mark.parametrize("case,dtype,payload", PARAMS, ids=IDS)
def test_nonfinite_class_mask_and_finite_parity(cuda, case, dtype, payload):
    k = K()
    b = case.build(dtype, payload)
    got = RUN[case.family](k, Dev(b), b)
    want = b.expected(case.key in NF.DEVIATIONS)
    assert set(got) == set(want)
    for name in want:
        out_dtype = b.out_dtypes.get(name, dtype)
        tol = b.tol.get(name, NF.DEFAULT_TOL)[0 if out_dtype == torch.float32 else 1]
        check(got[name], want[name], tol, f"{case.family}/{case.name}/{payload} {name}", b.elementwise.get(name))
