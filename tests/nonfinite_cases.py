"""Seeded CPU builders of inputs that already HOLD a NaN or an infinity, with the fp64 references that tests/test_nonfinite_host.py (CPU) and
tests/test_nonfinite_gpu.py (device) share.  Test infrastructure only.

The other suites feed finite operands (NaN appears only as poison AROUND buffers and as gradients into AdamW's scrub).  Here a few named
elements of ONE operand are overwritten with a payload -- NaN everywhere; +Inf / -Inf only where the answer does not hang on an approximation
(ReLU and clip, GEMM operands, the norms, softmax and cross-entropy logits; never the polynomial / tanh / erf GELU forms, sigmoid or swish) -- and
the kernel must put NaN, +Inf, -Inf and finite values exactly where the fp64 reference of the same operation puts them (the CLASS MASK of the
output), and meet the tolerance of its existing parity test on the finite remainder.

Every builder rounds its values to the storage dtype BEFORE the reference sees them (the q() convention of tests/test_kernels_gpu.py) and puts
the payload at three kinds of position: the first element, the 16-byte vector body, and the ragged part (last row, last column, scalar tail).
The reference is oracle.tf_ops or the fp64 restatement the kernel's parity test already uses, evaluated on the SAME poisoned input.

DEVIATIONS lists the cases whose expected mask is NOT the reference's: (family, case) -> (reason, exact expected behaviour).  An entry is
allowed only where the kernel never READS data that the reference multiplies by an exact zero (the kernel line is cited), for max pooling and
first-max ties (today's behaviour pinned), and for behaviour a docstring already declares.  A kernel that turns NaN into a finite number by
arithmetic is a bug, not a deviation.  The builder of such a case returns the pinned expectation next to the reference's (Built.pinned).
"""

import torch

from oracle import tf_ops as O

NAN, INF = float("nan"), float("inf")
PAYLOADS = {"nan": NAN, "+inf": INF, "-inf": -INF}
ALL3 = ("nan", "+inf", "-inf")
NAN_ONLY = ("nan",)
F32, BF16 = torch.float32, torch.bfloat16
BOTH = (F32, BF16)
DEFAULT_TOL = (2e-5, 1.2e-2)      # the defaults of close() in tests/test_kernels_gpu.py: (fp32 storage, bf16 storage)
IGNORE = 255

# ISEG_ACT_* codes of include/iseg_hip.h (iseg_amd/_hip.py; tests/test_nonfinite_host.py checks them against iseg_amd.kernels)
ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_GRAD, ACT_RELU_GRAD, ACT_MUL_AUX, ACT_SIGMOID, ACT_SWISH, ACT_GELU_TANH = range(9)
ACT_NAMES = {ACT_RELU: "relu", ACT_GELU: "gelu", ACT_SIGMOID: "sigmoid", ACT_SWISH: "swish", ACT_GELU_TANH: "gelu_tanh"}

# Every place in iseg_amd/csrc that applies ReLU to DATA (collected by hand; the backward masks `aux > 0 ? dy : 0` are not ReLUs of data):
# csrc site -> (the iseg_amd.kernels wrapper that reaches it, the family of this table that drives it).  tests/test_nonfinite_host.py checks
# that every wrapper exists and that every family named here has a case whose reference output holds a NaN behind a ReLU.
RELU_SITES = {
    "gemm_impl.h epi_apply (scalar epilogue)": ("dense_fwd", "gemm_fwd"),
    "gemm_impl.h epi_apply8 / epi_finish8 (vector epilogues)": ("dense_fwd", "gemm_fwd"),
    "gemm_dma.h epilogue through epi_finish8 (LDS-DMA forms)": ("dense_fwd_t", "gemm_dma"),
    "elementwise.hip act_value": ("act_fwd", "act_fwd"),
    "misc.hip add_relu_kernel": ("add_relu", "add_relu"),
    "norm.hip bn_apply_kernel": ("bn_apply_fwd", "bn_apply"),
    "norm.hip bn_apply_packed_kernel": ("bn_finalize_apply", "bn_finalize_apply"),
    "resize.hip bn_relu_upsample_add_kernel": ("bn_relu_upsample_add", "bn_relu_upsample_add"),
    "resblock.hip rb_fwd_kernel": ("resblock_tail_fwd", "resblock_tail"),
    "sepconv.hip relu_dwconv3 prologue": ("relu_dwconv3_stats", "relu_dwconv3"),
    "sepconv.hip bnfold_dwconv3_relu_bwd (recomputed ReLU of x)": ("bnfold_dwconv3_relu_bwd", "relu_dwconv3_bwd"),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed), dtype=torch.float64) * scale


def rq(t, dtype):
    """round to the storage dtype, back in fp64"""
    return t.to(dtype).to(torch.float64)


def poison(t, positions, payload):
    """a copy of `t` with the payload at every index tuple of `positions`"""
    t = t.clone()
    for p in positions:
        t[p] = PAYLOADS[payload]
    return t


def classes(t):
    """class mask of a tensor: 0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    t = t.detach().to("cpu", torch.float64)
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isnan(t)] = 1
    c[t == INF] = 2
    c[t == -INF] = 3
    return c


class Built:
    """one built case: `inputs` name -> fp64 CPU tensor (rounded to its storage dtype, payload in place) or a plain parameter; `in_dtypes` the
    storage dtype of the inputs that do not use the case's (fp32 parameter vectors, int32 labels); `want` name -> fp64 reference output;
    `tol` name -> (fp32, bf16) tolerance of the existing parity test and `out_dtypes` the dtype that picks between the two;
    `shape` name -> the bool mask the NaN footprint obviously has (host check, NaN payload only); `pinned` the expectation of a DEVIATIONS case"""

    def __init__(self, dtype, inputs, want, in_dtypes=None, tol=None, out_dtypes=None, shape=None, pinned=None, relu=False, elementwise=None):
        self.dtype, self.inputs, self.want = dtype, inputs, {k: v.detach() for k, v in want.items()}
        self.elementwise = elementwise or {}      # name -> (rel, abs): |err| <= rel * |want| + abs per element, where the parity test bounds it so
        self.in_dtypes, self.tol, self.out_dtypes = in_dtypes or {}, tol or {}, out_dtypes or {}
        self.shape, self.pinned, self.relu = shape or {}, pinned, relu

    def expected(self, deviation):
        return {k: v.detach() for k, v in self.pinned.items()} if deviation else self.want


class Case:
    def __init__(self, family, name, build, dtypes=BOTH, payloads=ALL3, empty_ok=False):
        self.family, self.name, self.build, self.dtypes, self.payloads, self.empty_ok = family, name, build, dtypes, payloads, empty_ok

    @property
    def key(self):
        return (self.family, self.name)


def params():
    """(case, dtype, payload) of every case, with readable ids"""
    out, ids = [], []
    for c in CASES:
        for d in c.dtypes:
            for p in c.payloads:
                out.append((c, d, p))
                ids.append(f"{c.family}-{c.name}-{'f32' if d == F32 else 'bf16'}-{p}")
    return out, ids


def rows_mask(shape, rows):
    m = torch.zeros(shape, dtype=torch.bool)
    m[list(rows)] = True
    return m


def cols_mask(shape, cols):
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., list(cols)] = True
    return m


def elems_mask(shape, positions):
    m = torch.zeros(shape, dtype=torch.bool)
    for p in positions:
        m[p] = True
    return m


CASES = []


def case(family, name, **kw):
    def deco(fn):
        CASES.append(Case(family, name, fn, **kw))
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM family
# ---------------------------------------------------------------------------------------------------------------------------
GEMM_FWD_SHAPES = ((77, 21, 256), (130, 96, 384))      # ragged M and N (scalar epilogue) / whole 8-column vectors with a ragged last row tile
WGRAD_TOL = {F32: 5e-5, BF16: 2e-4}                    # test_gemm_wgrad_splitk / test_wgrad_with_fused_bias_gradient (fp32 outputs)


def gemm_positions(operand, M, N, Kd):
    """payload positions per operand and the output rows / columns / elements a NaN there reaches"""
    if operand == "A":
        pos = [(0, 0), (M // 2, 8 + 3), (M - 1, Kd - 1)]
        return pos, ("rows", [p[0] for p in pos])
    if operand == "W":
        pos = [(0, 0), (Kd // 2, 8 + 3), (Kd - 1, N - 1)]
        return pos, ("cols", [p[1] for p in pos])
    if operand == "bias":
        pos = [(0,), (8 + 3,), (N - 1,)]
        return pos, ("cols", [p[0] for p in pos])
    pos = [(0, 0), (M // 2, 8 + 3), (M - 1, N - 1)]      # residual
    return pos, ("elems", pos)


def footprint(kind, shape):
    what, idx = kind
    return {"rows": rows_mask, "cols": cols_mask, "elems": elems_mask}[what](shape, idx)


def build_gemm_fwd(M, N, Kd, epi, operand):
    def build(dtype, payload):
        x, w = rq(rnd((M, Kd), 1), dtype), rq(rnd((Kd, N), 2, Kd ** -0.5), dtype)
        b = rq(rnd((N,), 3), F32)
        res = rq(rnd((M, N), 4), dtype)
        cs = rq(rnd((N,), 5) * 0.5 + 1, F32)
        rs = torch.tensor([0.0, 1.25, 1.25], dtype=torch.float64)
        G = -(-M // 3)
        pos, kind = gemm_positions(operand, M, N, Kd)
        ops = {"A": x, "W": w, "bias": b, "residual": res}
        ops[operand] = poison(ops[operand], pos, payload)
        x, w, b, res = ops["A"], ops["W"], ops["bias"], ops["residual"]
        h = x @ w + b
        want = {}
        if epi == "none":
            want["y"] = h
        elif epi == "relu":
            want["y"] = torch.relu(h)
        elif epi == "gelu_pre":
            want["y"], want["pre"] = O.gelu(h), h
        else:      # colscale * rowscale (one group scaled by exactly 0: 0 * NaN is NaN on both sides) + residual
            want["y"] = res + h * cs * rs.repeat_interleave(G)[:M].unsqueeze(1)
        inputs = {"x": x, "w": w, "bias": b, "res": res, "cs": cs, "rs": rs, "G": G, "epi": epi}
        return Built(dtype, inputs, want, in_dtypes={"bias": F32, "cs": F32, "rs": F32},
                     shape={k: footprint(kind, (M, N)) for k in want}, relu=epi == "relu")
    return build


for (_M, _N, _K) in GEMM_FWD_SHAPES:
    for _epi, _pl in (("none", ALL3), ("relu", ALL3), ("gelu_pre", NAN_ONLY), ("scale_res", ALL3)):
        for _op in ("A", "W", "bias") + (("residual",) if _epi == "scale_res" else ()):
            CASES.append(Case("gemm_fwd", f"{_M}x{_N}x{_K}-{_epi}-{_op}", build_gemm_fwd(_M, _N, _K, _epi, _op), payloads=_pl))


def build_gemm_dgrad(act, operand):
    M, N, Kd = 70, 21, 256

    def build(dtype, payload):
        dy, w = rq(rnd((M, N), 1), dtype), rq(rnd((Kd, N), 2, N ** -0.5), dtype)
        aux = rq(rnd((M, Kd), 3), dtype)
        if operand == "dy":
            pos = [(0, 0), (M // 2, 8 + 3), (M - 1, N - 1)]
            dy = poison(dy, pos, payload)
            mask = rows_mask((M, Kd), [p[0] for p in pos]) & ((aux > 0) | (act != ACT_RELU_GRAD))
        else:
            pos = [(0, 0), (M // 2, 96 + 3), (M - 1, Kd - 1)]
            aux = poison(aux, pos, payload)
            # the ReLU mask (aux > 0) is false for NaN: the reference's gradient there is an exact 0, and so must the kernel's be
            mask = torch.zeros((M, Kd), dtype=torch.bool) if act == ACT_RELU_GRAD else elems_mask((M, Kd), pos)
        g = dy @ w.T
        if act == ACT_RELU_GRAD:      # the select that `* (aux > 0)` of test_gemm_dgrad_and_gelu_grad stands for on finite values: no gradient where the mask is false
            want = torch.where(aux > 0, g, torch.zeros_like(g))
        elif act == ACT_MUL_AUX:
            want = g * aux
        else:
            a = aux.clone().requires_grad_(True)
            O.gelu(a).backward(torch.ones_like(a))
            want = g * a.grad
        return Built(dtype, {"dy": dy, "w": w, "aux": aux, "act": act}, {"dx": want}, shape={"dx": mask})
    return build


for _act, _nm, _pl in ((ACT_RELU_GRAD, "relu_grad", ALL3), (ACT_GELU_GRAD, "gelu_grad", NAN_ONLY), (ACT_MUL_AUX, "mul_aux", ALL3)):
    for _op in ("dy", "aux"):
        CASES.append(Case("gemm_dgrad", f"{_nm}-{_op}", build_gemm_dgrad(_act, _op), payloads=_pl,
                          empty_ok=(_act == ACT_RELU_GRAD and _op == "aux")))


def build_gemm_wgrad(operand, bias_grad):
    M, N, Kd = 1030, 21, 256

    def build(dtype, payload):
        x, dy = rq(rnd((M, Kd), 1), dtype), rq(rnd((M, N), 2), dtype)
        if operand == "x":      # one element x[m, k] reaches row k of dW = X^T dY (a whole NaN ROW of x would reach every element)
            pos = [(0, 0), (M // 2, 96 + 3), (M - 1, Kd - 1)]
            x = poison(x, pos, payload)
            mask, bmask = rows_mask((Kd, N), [p[1] for p in pos]), torch.zeros(N, dtype=torch.bool)
        else:
            pos = [(0, 0), (M // 2, 8 + 3), (M - 1, N - 1)]
            dy = poison(dy, pos, payload)
            mask, bmask = cols_mask((Kd, N), [p[1] for p in pos]), cols_mask((N,), [p[1] for p in pos])
        want, shape = {"dW": x.T @ dy + 0.5}, {"dW": mask}
        if bias_grad:
            want["db"], shape["db"] = dy.sum(0) - 1.0, bmask
        t = (WGRAD_TOL[dtype], WGRAD_TOL[dtype])
        return Built(dtype, {"x": x, "dy": dy, "bias_grad": bias_grad}, want, tol={"dW": t, "db": t}, out_dtypes={"dW": F32, "db": F32}, shape=shape)
    return build


for _op in ("x", "dy"):
    for _bg in (False, True):
        CASES.append(Case("gemm_wgrad", f"split3-{_op}" + ("-bias_grad" if _bg else ""), build_gemm_wgrad(_op, _bg)))


# the LDS-DMA forms (bf16, both operands K-contiguous: dense_fwd_t) with the ReLU epilogue, each at the smallest un-split `nt/` problem that
# tests/gemm_plan_cases.py / tests/golden/gemm_plans.json list for the form: form -> (M, N, K)
GEMM_DMA_SHAPES = {1: (300, 64, 72), 4: (1000, 136, 96), 9: (7000, 384, 192), 2: (16384, 512, 128), 6: (4096, 3072, 768), 8: (16384, 384, 1536)}


def build_gemm_dma(form, operand):
    M, N, Kd = GEMM_DMA_SHAPES[form]

    def build(dtype, payload):
        x, wt = rq(rnd((M, Kd), 1), dtype), rq(rnd((N, Kd), 2, Kd ** -0.5), dtype)
        b = rq(rnd((N,), 3), F32)
        pos, kind = gemm_positions(operand, M, N, Kd)
        if operand == "A":
            x = poison(x, pos, payload)
        else:
            b = poison(b, pos, payload)
        y = torch.relu(x @ wt.T + b)
        return Built(dtype, {"x": x, "wt": wt, "bias": b, "form": form}, {"y": y}, in_dtypes={"bias": F32}, shape={"y": footprint(kind, (M, N))},
                     relu=True)
    return build


for _form in GEMM_DMA_SHAPES:
    for _op in ("A", "bias"):
        CASES.append(Case("gemm_dma", f"form{_form}-relu-{_op}", build_gemm_dma(_form, _op), dtypes=(BF16,),
                          payloads=ALL3 if _form in (1, 4) else NAN_ONLY))


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise activations: n = 1027 = 128 vectors of 8 and a scalar tail of 3
# ---------------------------------------------------------------------------------------------------------------------------
EW_N = 1027
EW_POS = [(0,), (8 * 40 + 5,), (EW_N - 1,)]


def act_ref(v, act):
    return {ACT_RELU: torch.relu, ACT_GELU: O.gelu, ACT_SIGMOID: torch.sigmoid, ACT_SWISH: lambda t: t * torch.sigmoid(t),
            ACT_GELU_TANH: lambda t: torch.nn.functional.gelu(t, approximate="tanh")}[act](v)


def build_act_fwd(act):
    def build(dtype, payload):
        x = poison(rq(rnd((EW_N,), 1) * 1.5, dtype), EW_POS, payload)
        return Built(dtype, {"x": x, "act": act}, {"y": act_ref(x, act)}, shape={"y": elems_mask((EW_N,), EW_POS)}, relu=act == ACT_RELU)
    return build


def build_act_bwd(act, operand):
    def build(dtype, payload):
        dy, aux = rq(rnd((EW_N,), 2), dtype), rq(rnd((EW_N,), 1) * 1.5, dtype)
        if operand == "dy":
            dy = poison(dy, EW_POS, payload)
        else:
            aux = poison(aux, EW_POS, payload)
        if act == ACT_RELU:      # (the select, as in build_gemm_dgrad)
            want = torch.where(aux > 0, dy, torch.zeros_like(dy))
        else:
            a = aux.clone().requires_grad_(True)
            act_ref(a, act).backward(torch.ones_like(a))
            want = dy * a.grad
        mask = elems_mask((EW_N,), EW_POS)
        if act == ACT_RELU:
            mask = torch.zeros(EW_N, dtype=torch.bool) if operand == "aux" else mask & (aux > 0)
        return Built(dtype, {"dy": dy, "aux": aux, "act": act}, {"dx": want}, shape={"dx": mask})
    return build


for _act, _nm in ACT_NAMES.items():
    _pl = ALL3 if _act == ACT_RELU else NAN_ONLY
    CASES.append(Case("act_fwd", _nm, build_act_fwd(_act), payloads=_pl))
    for _op in ("dy", "aux"):
        CASES.append(Case("act_bwd", f"{_nm}-{_op}", build_act_bwd(_act, _op), payloads=_pl, empty_ok=(_act == ACT_RELU and _op == "aux")))


@case("add_relu", "n1032")      # (iseg_add_relu takes whole 16-byte vectors only: the ragged part is the last vector)
def build_add_relu(dtype, payload):
    n = 1032
    pos = [(0,), (8 * 40 + 5,), (n - 1,)]
    a, b = poison(rq(rnd((n,), 1), dtype), pos[:2], payload), poison(rq(rnd((n,), 2), dtype), pos[2:], payload)
    return Built(dtype, {"a": a, "b": b}, {"y": torch.relu(a + b)}, shape={"y": elems_mask((n,), pos)}, relu=True)


CLIP = (-0.5, 0.75)


@case("clip_fwd", "n1027")
def build_clip_fwd(dtype, payload):
    x = poison(rq(rnd((EW_N,), 1), dtype), EW_POS, payload)
    return Built(dtype, {"x": x}, {"y": torch.clamp(x, *CLIP)}, shape={"y": elems_mask((EW_N,), EW_POS)})


def build_clip_bwd(operand):
    def build(dtype, payload):
        x, dy = rq(rnd((EW_N,), 1), dtype), rq(rnd((EW_N,), 2), dtype)
        if operand == "x":
            x = poison(x, EW_POS, payload)      # tf.clip_by_value passes the gradient where lo <= x <= hi: false for NaN, an exact 0
            mask = torch.zeros(EW_N, dtype=torch.bool)
        else:
            dy = poison(dy, EW_POS, payload)
            mask = elems_mask((EW_N,), EW_POS) & (x >= CLIP[0]) & (x <= CLIP[1])
        want = torch.where((x >= CLIP[0]) & (x <= CLIP[1]), dy, torch.zeros_like(dy))
        return Built(dtype, {"x": x, "dy": dy}, {"dx": want}, shape={"dx": mask})
    return build


CASES.append(Case("clip_bwd", "n1027-x", build_clip_bwd("x"), empty_ok=True))
CASES.append(Case("clip_bwd", "n1027-dy", build_clip_bwd("dy"), empty_ok=True))


def build_glu(act, operand, cols):
    rows = 13

    def build(dtype, payload):
        g, x = rq(rnd((rows, cols), 1) * 1.5, dtype), rq(rnd((rows, cols), 2), dtype)
        pos = [(0, 0), (rows // 2, 8 + 3), (rows - 1, cols - 1)]
        if operand == "gate":
            g = poison(g, pos, payload)
        else:
            x = poison(x, pos, payload)
        return Built(dtype, {"gate": g, "x": x, "act": act}, {"out": act_ref(g, act) * x}, shape={"out": elems_mask((rows, cols), pos)},
                     relu=act == ACT_RELU and operand == "gate")
    return build


for _cols in (80, 79):      # the 16-byte form and the one-element-per-lane form
    for _act in (ACT_GELU, ACT_SWISH, ACT_GELU_TANH):      # (iseg_glu_fwd takes no ReLU gate)
        for _op in ("gate", "x"):
            CASES.append(Case("glu_fwd", f"{ACT_NAMES[_act]}-cols{_cols}-{_op}", build_glu(_act, _op, _cols), payloads=NAN_ONLY))


# ---------------------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------------------
LN_ROWS = 37
LN_TOL = {"y": DEFAULT_TOL, "dx": (1e-4, 2e-2), "dbeta": (2e-4, 2e-4)}      # test_layernorm_fwd_bwd


def norm_positions(rows, C):
    return [(0, 0), (rows // 2, min(8 + 3, C - 2)), (rows - 1, C - 1)]


def build_layernorm(C, operand):
    rows = LN_ROWS

    def build(dtype, payload):
        x = rq(rnd((rows, C), 1) * 2 + 0.3, dtype)
        g, b = rq(rnd((C,), 2) * 0.3 + 1, F32), rq(rnd((C,), 3) * 0.2, F32)
        dy = rq(rnd((rows, C), 4), dtype)
        pos = norm_positions(rows, C)
        if operand == "x":
            x = poison(x, pos, payload)
        else:
            dy = poison(dy, pos, payload)
        xx, gg, bb = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yo = O.layer_norm(xx, gg, bb, 1e-6)
        yo.backward(dy)
        prow = rows_mask((rows, C), [p[0] for p in pos])
        want = {"y": yo, "dx": xx.grad, "dgamma": gg.grad, "dbeta": bb.grad}
        if operand == "x":      # xhat of a poisoned row is NaN in every column, so dgamma = sum_rows dy * xhat is NaN in every column; dbeta = sum dy is not
            shape = {"y": prow, "dx": prow, "dgamma": torch.ones(C, dtype=torch.bool), "dbeta": torch.zeros(C, dtype=torch.bool)}
        else:
            pc = cols_mask((C,), [p[1] for p in pos])
            shape = {"y": torch.zeros((rows, C), dtype=torch.bool), "dx": prow, "dgamma": pc, "dbeta": pc}
        tol = dict(LN_TOL, dgamma=(2e-4, 2e-4) if dtype == F32 else (2e-2, 2e-2))
        return Built(dtype, {"x": x, "gamma": g, "beta": b, "dy": dy}, want, in_dtypes={"gamma": F32, "beta": F32}, tol=tol,
                     out_dtypes={"dgamma": F32, "dbeta": F32}, shape=shape)
    return build


for _C in (96, 8, 5):
    for _op in ("x", "dy"):
        # An infinite gradient makes both row means of the backward pass infinite, and an element of dx is then -Inf - (+-Inf): NaN or an
        # infinity according to the order in which the closed form is associated (autograd says NaN, the kernel's one-pass form -Inf for some
        # elements).  Neither is an approximation error and neither is finite, so the class is not the operation's to define: dy takes NaN only.
        CASES.append(Case("layernorm", f"C{_C}-{_op}", build_layernorm(_C, _op), payloads=ALL3 if _op == "x" else NAN_ONLY))


def build_layernorm_post(operand):
    rows, C, groups = 39, 96, 3

    def build(dtype, payload):
        x = rq(rnd((rows, C), 1) * 2 + 0.3, dtype)
        g, b = rq(rnd((C,), 2) * 0.3 + 1, F32), rq(rnd((C,), 3) * 0.2, F32)
        cs = rq(rnd((C,), 6) * 0.4 + 1, F32)
        rs = torch.tensor([0.0, 1.25, 2.5], dtype=torch.float64)
        res = rq(rnd((rows, C), 7), dtype)
        pos = norm_positions(rows, C)
        if operand == "x":
            x = poison(x, pos, payload)
            mask = rows_mask((rows, C), [p[0] for p in pos])
        else:
            res = poison(res, pos, payload)
            mask = elems_mask((rows, C), pos)
        rpg = rows // groups
        yo = O.layer_norm(x, g, b, 1e-6) * cs * rs[torch.arange(rows) // rpg][:, None] + res      # (row 0 lies in the group scaled by an exact 0)
        return Built(dtype, {"x": x, "gamma": g, "beta": b, "cs": cs, "rs": rs, "rpg": rpg, "res": res}, {"y": yo},
                     in_dtypes={"gamma": F32, "beta": F32, "cs": F32, "rs": F32}, shape={"y": mask})
    return build


for _op in ("x", "residual"):
    CASES.append(Case("layernorm_post", f"rows39-C96-{_op}", build_layernorm_post(_op)))


def build_rmsnorm(C, operand):
    rows = LN_ROWS

    def build(dtype, payload):
        x, sc, dy = rq(rnd((rows, C), 1), dtype), rq(rnd((C,), 2) * 0.3, F32), rq(rnd((rows, C), 3), dtype)
        pos = norm_positions(rows, C)
        if operand == "x":
            x = poison(x, pos, payload)
        else:
            dy = poison(dy, pos, payload)
        xx, ss = x.clone().requires_grad_(True), sc.clone().requires_grad_(True)
        yo = O.rms_norm(xx, ss, 1e-6)
        yo.backward(dy)
        prow = rows_mask((rows, C), [p[0] for p in pos])
        if operand == "x":
            shape = {"y": prow, "dx": prow, "dscale": torch.ones(C, dtype=torch.bool)}
        else:
            shape = {"y": torch.zeros((rows, C), dtype=torch.bool), "dx": prow, "dscale": cols_mask((C,), [p[1] for p in pos])}
        return Built(dtype, {"x": x, "scale": sc, "dy": dy}, {"y": yo, "dx": xx.grad, "dscale": ss.grad}, in_dtypes={"scale": F32},
                     tol={"dx": (5e-5, 2e-2), "dscale": (5e-5, 2e-2)}, shape=shape)      # test_rmsnorm (tests/test_misc_gpu.py)
    return build


for _C in (96, 100):
    for _op in ("x", "dy"):
        CASES.append(Case("rmsnorm", f"C{_C}-{_op}", build_rmsnorm(_C, _op)))


@case("groupnorm_fwd", "3x5x7x96-g2")
def build_groupnorm(dtype, payload):
    N, H, W, C, groups = 3, 5, 7, 96, 2
    x = rq(rnd((N, H, W, C), 1) * 2 + 0.5, dtype)
    g, b = rq(rnd((C,), 2) * 0.2 + 1, F32), rq(rnd((C,), 3) * 0.1, F32)
    pos = [(0, 0, 0, 0), (1, 2, 3, 8 + 3)]      # (sample 0, group 0), (sample 1, group 0): two of the six (sample, group) sets
    x = poison(x, pos, payload)
    mask = torch.zeros((N, H, W, C), dtype=torch.bool)
    mask[0, :, :, :C // groups] = True
    mask[1, :, :, :C // groups] = True
    return Built(dtype, {"x": x, "gamma": g, "beta": b, "groups": groups}, {"y": O.group_norm(x, g, b, groups, 1e-3)},
                 in_dtypes={"gamma": F32, "beta": F32}, shape={"y": mask})


@case("groupnorm_fwd", "2x3x3x32-g32-last")
def build_groupnorm_last(dtype, payload):
    N, H, W, C, groups = 2, 3, 3, 32, 32
    x = rq(rnd((N, H, W, C), 1) * 2 + 0.5, dtype)
    g, b = rq(rnd((C,), 2) * 0.2 + 1, F32), rq(rnd((C,), 3) * 0.1, F32)
    pos = [(0, 0, 0, 0), (N - 1, H - 1, W - 1, C - 1)]
    x = poison(x, pos, payload)
    mask = torch.zeros((N, H, W, C), dtype=torch.bool)
    mask[0, :, :, 0] = True
    mask[N - 1, :, :, C - 1] = True
    return Built(dtype, {"x": x, "gamma": g, "beta": b, "groups": groups}, {"y": O.group_norm(x, g, b, groups, 1e-3)},
                 in_dtypes={"gamma": F32, "beta": F32}, shape={"y": mask})


@case("grn_fwd", "4x5x7x24")
def build_grn(dtype, payload):
    # a NaN at (sample n, channel c) makes gx[n, c] NaN, the channel mean of gx NaN, and so nx[n, :] and the whole sample NaN: one of four samples
    N, H, W, C = 4, 5, 7, 24
    x = rq(rnd((N, H, W, C), 1), dtype)
    g, b = rq(rnd((C,), 2) * 0.3, F32), rq(rnd((C,), 3) * 0.1, F32)
    pos = [(0, 0, 0, 0), (0, 2, 3, 8 + 3), (0, H - 1, W - 1, C - 1)]
    x = poison(x, pos, payload)
    mask = torch.zeros((N, H, W, C), dtype=torch.bool)
    mask[0] = True
    gx = torch.pow((x * x).sum(dim=(1, 2)) + 1e-6, 0.5)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    smask = rows_mask((N, C), [0])
    return Built(dtype, {"x": x, "gamma": g, "beta": b}, {"y": O.grn(x, g, b, 1e-6), "nx": nx, "gx": gx},
                 in_dtypes={"gamma": F32, "beta": F32}, out_dtypes={"nx": F32, "gx": F32},
                 tol={"y": (2e-6, 1e-2), "nx": (1e-5, 1e-5), "gx": (1e-5, 1e-5)},      # test_grn_forward_backward_match_oracle
                 shape={"y": mask, "nx": smask, "gx": elems_mask((N, C), [(0, 0), (0, 8 + 3), (0, C - 1)])})


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm: rows = 3 * 5 * 7, C = 24
# ---------------------------------------------------------------------------------------------------------------------------
BN_ROWS, BN_C = 3 * 5 * 7, 24
BN_POS = [(0, 0), (BN_ROWS // 2, 8 + 3), (BN_ROWS - 1, BN_C - 1)]


def build_bn(relu):
    def build(dtype, payload):
        x = poison(rq(rnd((BN_ROWS, BN_C), 1) * 1.5 + 0.2, dtype), BN_POS, payload)
        g, b = rq(rnd((BN_C,), 2) * 0.3 + 1, F32), rq(rnd((BN_C,), 3) * 0.2, F32)
        yo, _, _ = O.batch_norm_train(x, g, b, 1e-3)
        if relu:
            yo = torch.relu(yo)
        return Built(dtype, {"x": x, "gamma": g, "beta": b, "relu": relu}, {"y": yo}, in_dtypes={"gamma": F32, "beta": F32},
                     tol={"y": (1e-4, 1.2e-2)}, shape={"y": cols_mask((BN_ROWS, BN_C), [p[1] for p in BN_POS])}, relu=relu)      # test_batchnorm_train
    return build


for _fam in ("bn_apply", "bn_finalize_apply"):      # bn_stats -> bn_finalize -> bn_apply_fwd, and bn_stats -> the one-launch bn_finalize_apply
    for _relu in (False, True):
        CASES.append(Case(_fam, "relu" if _relu else "linear", build_bn(_relu)))


@case("bn_infer_apply", "relu-element")
def build_bn_infer(dtype, payload):
    # inference statistics (finite mean / rstd handed to bn_apply_fwd): the poisoned element alone
    x = poison(rq(rnd((BN_ROWS, BN_C), 1) * 1.5 + 0.2, dtype), BN_POS, payload)
    g, b = rq(rnd((BN_C,), 2) * 0.3 + 1, F32), rq(rnd((BN_C,), 3) * 0.2, F32)
    mm, mv = rq(rnd((BN_C,), 4) * 0.3, F32), rq(rnd((BN_C,), 5).abs() + 0.5, F32)
    rstd = rq(torch.rsqrt(mv + 1e-3), F32)
    yo = torch.relu((x - mm) * rstd * g + b)
    return Built(dtype, {"x": x, "gamma": g, "beta": b, "mean": mm, "rstd": rstd}, {"y": yo},
                 in_dtypes={"gamma": F32, "beta": F32, "mean": F32, "rstd": F32}, tol={"y": (1e-4, 1.2e-2)},
                 shape={"y": elems_mask((BN_ROWS, BN_C), BN_POS)}, relu=True)


def build_bn_relu_upsample_add(operand):
    N, H, W, C, Hc, Wc = 2, 10, 14, 32, 5, 7

    def build(dtype, payload):
        z, xc = rq(rnd((N, H, W, C), 1) * 1.5 + 0.2, dtype), rq(rnd((N, Hc, Wc, C), 2), dtype)
        g, b = rq(rnd((C,), 3) * 0.3 + 1, F32), rq(rnd((C,), 4) * 0.2, F32)
        mean, rstd = rq(rnd((C,), 5) * 0.3 + 0.2, F32), rq(rnd((C,), 6).abs() * 0.2 + 0.6, F32)      # given statistics (finite): the element-wise part
        if operand == "z":
            pos = [(0, 0, 0, 0), (0, 4, 5, 8 + 3), (N - 1, H - 1, W - 1, C - 1)]
            z = poison(z, pos, payload)
        else:
            pos = [(0, 0, 0, 0), (N - 1, 2, 3, 8 + 3)]
            xc = poison(xc, pos, payload)
        yo = torch.relu((z - mean) * rstd * g + b) + O.resize_bilinear(xc, (H, W))
        return Built(dtype, {"z": z, "xc": xc, "gamma": g, "beta": b, "mean": mean, "rstd": rstd}, {"y": yo},
                     in_dtypes={"gamma": F32, "beta": F32, "mean": F32, "rstd": F32}, tol={"y": (1e-4, 2e-2)},
                     shape={"y": elems_mask((N, H, W, C), pos) if operand == "z" else resize_fwd_mask((N, H, W, C), Hc, Wc, pos, False)},
                     relu=operand == "z")
    return build


for _op in ("z", "x"):
    CASES.append(Case("bn_relu_upsample_add", f"2x10x14x32-{_op}", build_bn_relu_upsample_add(_op)))


# ---------------------------------------------------------------------------------------------------------------------------
# softmax rows (register kernels: ld 16 and ld 72) and the losses
# ---------------------------------------------------------------------------------------------------------------------------
def build_softmax(cols, clip):
    rows = 41

    def build(dtype, payload):
        ld = (cols + 7) // 8 * 8
        s = rq(rnd((rows, cols), 1) * 3, dtype)
        pos = [(0, 0), (rows // 2, min(8 + 3, cols - 2)), (rows - 1, cols - 1)]
        s = poison(s, pos, payload)
        p = torch.softmax(s, dim=-1)
        if clip:
            p = torch.clamp(p, 1e-7, 1.0 - 1e-7)      # (layers/multihead_self_attention.py: the clip of the probabilities; clamp hands a NaN on)
        return Built(dtype, {"s": s, "cols": cols, "ld": ld, "clip": clip}, {"p": p}, shape={"p": rows_mask((rows, cols), [q[0] for q in pos])})
    return build


for _cols in (9, 65, 2053):      # ld 16 and 72: the register kernels; ld 2056 > 2048: the one-wave-per-row softmax_fwd_kernel
    for _clip in (False, True):
        CASES.append(Case("softmax_rows_fwd", f"cols{_cols}" + ("-clip" if _clip else ""), build_softmax(_cols, _clip)))


def build_softmax_bwd(cols, operand):
    rows = 41

    def build(dtype, payload):
        ld = (cols + 7) // 8 * 8
        p = rq(torch.softmax(rnd((rows, cols), 1) * 3, dim=-1), dtype)
        dp = rq(rnd((rows, cols), 2), dtype)
        pos = [(0, 0), (rows // 2, min(8 + 3, cols - 2)), (rows - 1, cols - 1)]
        if operand == "p":
            p = poison(p, pos, payload)
        else:
            dp = poison(dp, pos, payload)
        ds = p * (dp - (dp * p).sum(-1, keepdim=True))      # the restatement of test_softmax_rows (tests/test_attention_gpu.py)
        return Built(dtype, {"p": p, "dp": dp, "cols": cols, "ld": ld}, {"ds": ds}, shape={"ds": rows_mask((rows, cols), [q[0] for q in pos])})
    return build


for _cols in (9, 65):
    for _op in ("p", "dp"):
        CASES.append(Case("softmax_rows_bwd", f"cols{_cols}-{_op}", build_softmax_bwd(_cols, _op), payloads=NAN_ONLY))


CE_P = 3 * 7 * 13      # 273 pixels: more than one 256-pixel tile at C = 21
CE_FOCAL = (0.25, 2.0)


def build_ce(C, focal, where):
    P = CE_P

    def build(dtype, payload):
        z = rq(rnd((P, C), 1) * 3, F32)
        y = torch.randint(0, C, (P,), generator=gen(5), dtype=torch.int32)
        y[torch.rand(P, generator=gen(6)) < 0.1] = IGNORE
        px_pos = [0, P // 2, P - 1]
        y[px_pos] = IGNORE if where == "ignored" else torch.tensor([0, 3, C - 1], dtype=torch.int32)
        pos = [(0, 0), (P // 2, min(8 + 3, C - 1)), (P - 1, C - 1)]
        zp = poison(z, pos, payload)

        def ref(zz):
            if focal:
                return O.softmax_focal_ce_ignore(y, zz, C, IGNORE, None, *CE_FOCAL)
            return O.softmax_ce_ignore(y, zz, C, IGNORE, None)
        zg = zp.clone().requires_grad_(True)
        lo = ref(zg)
        want = {"px": lo, "sum": lo.mean().reshape(1)}
        if focal and where == "valid":      # the gradient path of the clamp: d(mean loss) / d(logits), NaN over the poisoned pixel's row
            (want["dz"],) = torch.autograd.grad(lo.sum() / P, zg)
        pinned = None
        if where == "valid" and not focal:      # DEVIATIONS: the kernel reads the label's logit alone; the reference multiplies every log p_c by the one-hot row
            w = (y != IGNORE).to(z.dtype)
            gathered = (torch.logsumexp(zp, -1) - zp[torch.arange(P), y.long().clamp(0, C - 1)]) * w
            gathered[torch.isnan(zp).any(-1) | (zp == INF).any(-1)] = NAN      # (here the reference is NaN as well: Inf - Inf in log p)
            pinned = {"px": gathered, "sum": gathered.mean().reshape(1)}
        if where == "ignored":      # DEVIATIONS: the kernel never reads the logits of an ignored pixel into its loss: 0 there, and the sum stays finite
            clean = ref(z)
            pinned = {"px": clean, "sum": clean.mean().reshape(1)}
        t = (2e-5, 2e-5) if focal else (1e-5, 1e-5)      # test_softmax_ce_ignore / test_softmax_focal_ce_ignore
        return Built(dtype, {"z": zp, "y": y, "C": C, "focal": CE_FOCAL if focal else None}, want, in_dtypes={"z": F32, "y": torch.int32},
                     tol={"px": t, "sum": t, "dz": (5e-5, 5e-5)}, out_dtypes={"px": F32, "sum": F32, "dz": F32}, pinned=pinned,
                     shape={"px": elems_mask((P,), [(i,) for i in px_pos]), "sum": torch.ones(1, dtype=torch.bool)})
    return build


for _C in (21, 65):
    for _focal in (False, True):
        for _where in ("valid", "ignored"):
            CASES.append(Case("softmax_ce", f"C{_C}-{'focal' if _focal else 'plain'}-{_where}", build_ce(_C, _focal, _where), dtypes=(F32,),
                              empty_ok=_where == "ignored"))


# ---------------------------------------------------------------------------------------------------------------------------
# fused tails that hold a ReLU: the smallest shapes of tests/test_resblock_fused_gpu.py / tests/test_sepconv_fused_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
def build_resblock_tail(stride, bn0, operand):
    N, H, W, C = 2, 9, 11, 32

    def build(dtype, payload):
        Ho, Wo = -(-H // stride), -(-W // stride)
        z2, sc = rq(rnd((N, Ho, Wo, C), 1), dtype), rq(rnd((N, H, W, C), 2), dtype)
        st = {}
        for i in (2, 0):      # given statistics (finite): the element-wise tail
            st[f"mean{i}"], st[f"rstd{i}"] = rq(rnd((C,), 10 + i) * 0.2, F32), rq(rnd((C,), 20 + i).abs() * 0.2 + 0.7, F32)
            st[f"gamma{i}"], st[f"beta{i}"] = rq(rnd((C,), 30 + i).abs() + 0.5, F32), rq(rnd((C,), 40 + i) * 0.3, F32)
        if operand == "z2":
            pos = [(0, 0, 0, 0), (0, Ho // 2, Wo // 2, 8 + 3), (N - 1, Ho - 1, Wo - 1, C - 1)]
            z2 = poison(z2, pos, payload)
            mask = elems_mask((N, Ho, Wo, C), pos)
        else:      # an interior pixel and a corner of the shortcut: each reaches the one output pixel whose pooling window holds it
            pos = [(0, 0, 0, 0), (0, 4, 5, 8 + 3), (N - 1, H - 1, W - 1, C - 1)]
            sc = poison(sc, pos, payload)
            mask = elems_mask((N, Ho, Wo, C), [(n, h // stride, w // stride, c) for n, h, w, c in pos])
        x = (sc - st["mean0"]) * st["rstd0"] * st["gamma0"] + st["beta0"] if bn0 else sc
        if stride > 1:
            x = O.avg_pool_same(x, stride, stride)
        out = torch.relu((z2 - st["mean2"]) * st["rstd2"] * st["gamma2"] + st["beta2"] + x)
        return Built(dtype, dict(st, z2=z2, sc=sc, stride=stride, bn0=bn0), {"out": out}, in_dtypes={k: F32 for k in st},
                     tol={"out": (1e-3, 1.2e-2)}, shape={"out": mask}, relu=True)      # test_tail_fp32_against_fp64; bf16: the default of close()
    return build


for _s, _bn0 in ((1, False), (2, True)):
    for _op in ("z2", "sc"):
        CASES.append(Case("resblock_tail", f"s{_s}{'-bn0' if _bn0 else ''}-{_op}", build_resblock_tail(_s, _bn0, _op)))


def dw_reach(shape_out, pos, K, dil, stride, pad_t, pad_l):
    """output pixels whose K x K (dilated, strided) window holds one of the input pixels `pos`, same channel"""
    N, Ho, Wo, C = shape_out
    m = torch.zeros(shape_out, dtype=torch.bool)
    for n, h, w, c in pos:
        for i in range(K):
            for j in range(K):
                oh, ow = h + pad_t - i * dil, w + pad_l - j * dil
                if oh % stride == 0 and ow % stride == 0 and 0 <= oh // stride < Ho and 0 <= ow // stride < Wo:
                    m[n, oh // stride, ow // stride, c] = True
    return m


SPATIAL_POS = lambda N, H, W, C: [(0, 0, 0, 0), (0, H // 2, W // 2, 8 + 3), (N - 1, H - 1, W - 1, C - 1)]      # a corner, the interior, the last corner


def build_relu_dwconv3(stride):
    N, H, W, C = 3, 9, 11, 64      # test_stats_message

    def build(dtype, payload):
        x, w = rq(rnd((N, H, W, C), 1), dtype), rq(rnd((9, C), 2) / 3, F32)
        pos = SPATIAL_POS(N, H, W, C)
        x = poison(x, pos, payload)
        z = O.depthwise_conv2d(torch.relu(x), w.reshape(3, 3, C, 1), None, stride, 1, "same")
        _, pt, _ = O.same_pad(H, 3, stride, 1)
        _, pl, _ = O.same_pad(W, 3, stride, 1)
        return Built(dtype, {"x": x, "w": w, "stride": stride}, {"z": z}, in_dtypes={"w": F32}, tol={"z": (1e-5, 8e-3)},
                     shape={"z": dw_reach(tuple(z.shape), pos, 3, 1, stride, pt, pl)}, relu=True)
    return build


for _s in (1, 2):
    CASES.append(Case("relu_dwconv3", f"3x9x11x64-s{_s}", build_relu_dwconv3(_s)))


def build_relu_dwconv3_bwd(stride):
    N, H, W, C = 3, 9, 11, 64

    def build(dtype, payload):
        x, w = rq(rnd((N, H, W, C), 1), dtype), rq(rnd((9, C), 2) / 3, F32)
        pos = SPATIAL_POS(N, H, W, C)
        x = poison(x, pos, payload)
        rx = torch.relu(x).detach().requires_grad_(True)
        ww = w.reshape(3, 3, C, 1).clone().requires_grad_(True)
        z = O.depthwise_conv2d(rx, ww, None, stride, 1, "same")
        D = rq(rnd(tuple(z.shape), 3), dtype)
        z.backward(D)
        # inference statistics (train = 0): dz = D.  dx = [x > 0] dw^T(dz) -- the select: an exact 0 at a NaN x --, dw = sum relu(x) dz: NaN
        # in the taps of the poisoned channels that pair the NaN with a gradient inside the image
        dx = torch.where(x > 0, rx.grad, torch.zeros_like(x))
        st = {"mean": rq(rnd((C,), 4) * 0.2, F32), "rstd": rq(rnd((C,), 5).abs() * 0.2 + 0.7, F32), "gamma": rq(rnd((C,), 6).abs() + 0.5, F32)}
        return Built(dtype, dict(st, x=x, w=w, D=D, z=rq(z.detach().nan_to_num(0.0), dtype), stride=stride), {"dx": dx, "dw": ww.grad.reshape(9, C)},
                     in_dtypes={"w": F32, "mean": F32, "rstd": F32, "gamma": F32}, tol={"dx": (1e-4, 1.2e-2), "dw": (1e-4, 1.2e-2)},
                     shape={"dx": torch.zeros((N, H, W, C), dtype=torch.bool)}, relu=True)      # fp32: test_fused_matches_fp64 of test_sepconv_fused_gpu.py
    return build


for _s in (1, 2):      # NaN only: relu(-Inf) = 0 and 0 * dz leaves nothing to see, relu(+Inf) * dz sums +Inf and -Inf in an order-dependent way
    CASES.append(Case("relu_dwconv3_bwd", f"3x9x11x64-s{_s}", build_relu_dwconv3_bwd(_s), payloads=NAN_ONLY))


MASKLOSS_CE, MASKLOSS_FOCAL_CE = 4, 16      # ISEG_MASKLOSS_* of include/iseg_hip.h


def build_mask_loss(focal):
    B, H, W, C = 2, 9, 11, 21

    def build(dtype, payload):
        from tests import mask_loss_ref as MR

        z = rq((rnd((B, H * W, C), 1) * 4).clamp(-12, 12), F32)
        y = torch.randint(0, C, (B, H * W), generator=gen(5), dtype=torch.int32)
        y[torch.rand(B, H * W, generator=gen(6)) < 0.15] = IGNORE
        px = [(0, 0), (0, H * W // 2), (B - 1, H * W - 1)]
        for (b_, p_), lab in zip(px, (0, 3, C - 1)):
            y[b_, p_] = lab
        z = poison(z, [(0, 0, 0), (0, H * W // 2, 8 + 3), (B - 1, H * W - 1, C - 1)], payload)
        _, valid, t = MR.preprocess(y.reshape(B, H, W), z.reshape(B, H, W, C), C, IGNORE)
        ce = MR.ce_term(z, t, focal)
        ce = torch.where(torch.isnan(ce), torch.zeros_like(ce), ce)      # losses/mask_loss.py:148 of the reference: replace_nan_or_inf(ce_loss, 0.0)
        loss = ce * valid
        want = {"px": loss.reshape(-1), "mean": (loss.sum() / (valid.sum() + MR.EPS)).reshape(1)}
        return Built(dtype, {"z": z, "y": y, "flags": MASKLOSS_CE | (MASKLOSS_FOCAL_CE if focal else 0)}, want, in_dtypes={"z": F32, "y": torch.int32},
                     tol={"px": (2e-5, 2e-5), "mean": (2e-5, 2e-5)}, out_dtypes={"px": F32, "mean": F32})      # REL of tests/test_mask_loss_gpu.py
    return build


# The reference scrubs a NaN term itself (declared: csrc/mask_loss.hip `if (!(v == v)) v = 0.f`), so the expected footprint is EMPTY and the
# poisoned pixels report an exact 0 -- not the finite alpha * (1 - 1e-7)^2 * 16.1 that a clamp which swallows NaN made of them.
for _focal in (False, True):
    CASES.append(Case("mask_loss", f"ce-{'focal' if _focal else 'plain'}", build_mask_loss(_focal), dtypes=(F32,), payloads=NAN_ONLY, empty_ok=True))


# ---------------------------------------------------------------------------------------------------------------------------
# spatial kernels: N = 2, 9 x 11, one payload pixel in a corner, one in the interior, one in the last corner
# ---------------------------------------------------------------------------------------------------------------------------
def build_dwconv(Kk, dil, C):
    N, H, W = 2, 9, 11

    def build(dtype, payload):
        x = rq(rnd((N, H, W, C), 1), dtype)
        w, b = rq(rnd((Kk, Kk, C, 1), 2) / Kk, F32), rq(rnd((C,), 3) * 0.1, F32)
        pos = SPATIAL_POS(N, H, W, C)
        x = poison(x, pos, payload)
        pad = (Kk - 1) * dil // 2
        y = O.depthwise_conv2d(x, w, b, 1, dil)
        return Built(dtype, {"x": x, "w": w.reshape(Kk * Kk, C), "bias": b, "K": Kk, "dil": dil, "pad": pad}, {"y": y},
                     in_dtypes={"w": F32, "bias": F32}, shape={"y": dw_reach((N, H, W, C), pos, Kk, dil, 1, pad, pad)})
    return build


def mfma7_band_mask(shape, pos):
    """what csrc/dwconv_mfma.hip makes non-finite around the pixels `pos` (its header, lines 9-12): a unit is a 16-row output tile over a raw tile
    whose row rho is image row 16 th - 3 + rho (rho 0 .. 21 hold data); output row block j (4 rows) multiplies the row chunks j .. j + 2 of the raw
    tile with the banded weight operand, zeros included, so a pixel in chunk rho // 4 reaches the row blocks rho // 4 - 2 .. rho // 4 of every tile
    whose raw tile holds it -- clipped to the tile and the image -- in the columns w - 3 .. w + 3 of its channel"""
    N, H, W, C = shape
    m = torch.zeros(shape, dtype=torch.bool)
    for n, h, w, c in pos:
        for th in range(-(-H // 16)):
            rho = h - 16 * th + 3
            if not 0 <= rho <= 21:
                continue
            for j in range(max(rho // 4 - 2, 0), min(rho // 4, 3) + 1):
                r0 = 16 * th + 4 * j
                m[n, r0:min(r0 + 4, H), max(w - 3, 0):min(w + 4, W), c] = True
    return m


@case("dwconv2d7_mfma", "2x20x19x32", dtypes=(BF16,))      # two row tiles (rows 0 .. 15, 16 .. 19); the interior pixel's window crosses them
def build_dwconv7_mfma(dtype, payload):
    N, H, W, C = 2, 20, 19, 32
    x = rq(rnd((N, H, W, C), 1), dtype)
    w, b = rq(rnd((7, 7, C, 1), 2) / 7, BF16), rq(rnd((C,), 3) * 0.3, F32)      # bf16-representable weights, as tests/test_dwconv_mfma_gpu.py
    pos = [(0, 0, 0, 0), (0, 14, 9, 8 + 3), (N - 1, H - 1, W - 1, C - 1)]
    x = poison(x, pos, payload)
    y = O.depthwise_conv2d(x, w, b, 1, 1, "same")
    window, band = dw_reach((N, H, W, C), pos, 7, 1, 1, 3, 3), mfma7_band_mask((N, H, W, C), pos)
    assert not (window & ~band).any() and int((band & ~window).sum()) == 7 * 5      # rows 8 .. 10 and 18, 19 of the interior pixel's 7 columns
    pinned = y.clone()
    pinned[band & ~window] = NAN      # the payload times a zero of the band
    return Built(dtype, {"x": x, "w": w.reshape(49, C), "bias": b}, {"y": y}, in_dtypes={"w": F32, "bias": F32}, shape={"y": window},
                 pinned={"y": pinned}, elementwise={"y": (2.0 ** -8, 1e-5)})      # test_dwconv7_mfma_forward_matches_oracle


CASES.append(Case("dwconv2d", "k7-C32", build_dwconv(7, 1, 32)))
CASES.append(Case("dwconv2d", "k3-dil2-C112", build_dwconv(3, 2, 112)))


@case("dwconv2d_strided", "k3-s2-C16")
def build_dwconv_strided(dtype, payload):
    N, H, W, C, Kk, s = 2, 9, 11, 16, 3, 2
    x = rq(rnd((N, H, W, C), 1), dtype)
    w, b = rq(rnd((Kk, Kk, C, 1), 2) / Kk, F32), rq(rnd((C,), 3) * 0.1, F32)
    pos = SPATIAL_POS(N, H, W, C)
    x = poison(x, pos, payload)
    y = O.depthwise_conv2d(x, w, b, s, 1)
    _, pt, _ = O.same_pad(H, Kk, s, 1)
    _, pl, _ = O.same_pad(W, Kk, s, 1)
    return Built(dtype, {"x": x, "w": w.reshape(Kk * Kk, C), "bias": b, "K": Kk, "stride": s}, {"y": y}, in_dtypes={"w": F32, "bias": F32},
                 tol={"y": (1e-5, 2e-2)},      # test_strided_depthwise_conv_matches_oracle
                 shape={"y": dw_reach(tuple(y.shape), pos, Kk, 1, s, pt, pl)})


def resize_taps(out_size, in_size, align):
    """per output index the set of source indices the interpolation reads (both taps, whatever their weight: 0 * NaN is NaN in the reference)"""
    lo, hi, _ = O._interp_weights(out_size, in_size, torch.float64, align)
    return [{int(a), int(b)} for a, b in zip(lo, hi)]


def resize_fwd_mask(shape_out, Hi, Wi, pos, align):
    """outputs that read one of the source elements `pos`: the at most 2 x 2 neighbourhood scaled by the ratio"""
    N, Ho, Wo, C = shape_out
    ty, tx = resize_taps(Ho, Hi, align), resize_taps(Wo, Wi, align)
    m = torch.zeros(shape_out, dtype=torch.bool)
    for n, h, w, c in pos:
        for oy in range(Ho):
            for ox in range(Wo):
                if h in ty[oy] and w in tx[ox]:
                    m[n, oy, ox, c] = True
    return m


def resize_bwd_mask(shape_in, Ho, Wo, pos, align):
    """source elements that a poisoned gradient element of `pos` flows back to"""
    N, Hi, Wi, C = shape_in
    ty, tx = resize_taps(Ho, Hi, align), resize_taps(Wo, Wi, align)
    m = torch.zeros(shape_in, dtype=torch.bool)
    for n, oy, ox, c in pos:
        for h in ty[oy]:
            for w in tx[ox]:
                m[n, h, w, c] = True
    return m


def build_resize(align, Ho, Wo):
    N, H, W, C = 2, 9, 11, 8

    def build(dtype, payload):
        x = rq(rnd((N, H, W, C), 1), dtype)
        pos = [(0, 0, 0, 0), (0, H // 2, W // 2, 3), (N - 1, H - 1, W - 1, C - 1)]
        x = poison(x, pos, payload)
        y = O.resize_bilinear(x, (Ho, Wo), align_corners=align)
        return Built(dtype, {"x": x, "Ho": Ho, "Wo": Wo, "align": align}, {"y": y}, tol={"y": (1e-5, 1e-5)}, out_dtypes={"y": F32},
                     shape={"y": resize_fwd_mask((N, Ho, Wo, C), H, W, pos, align)})      # test_resize_bilinear_fwd_bwd (fp32 output)
    return build


for _align in (False, True):
    CASES.append(Case("resize_bilinear", f"9x11-to-18x22-{'ac' if _align else 'hp'}", build_resize(_align, 18, 22)))
    CASES.append(Case("resize_bilinear", f"9x11-to-13x17-{'ac' if _align else 'hp'}", build_resize(_align, 13, 17)))


def build_pool(mode):
    N, H, W, C, kk, s = 2, 9, 11, 8, 3, 2

    def build(dtype, payload):
        x = rq(rnd((N, H, W, C), 1), dtype)
        pos = [(0, 0, 0, 0), (0, H // 2, W // 2, 3), (N - 1, H - 1, W - 1, C - 1)]
        x = poison(x, pos, payload)
        Ho, pt, _ = O.same_pad(H, kk, s)
        Wo, pl, _ = O.same_pad(W, kk, s)
        y = (O.avg_pool_same if mode == "avg" else O.max_pool_same)(x, kk, s)
        pinned = None
        if mode == "max":      # DEVIATIONS: fmaxf skips a NaN -- the maximum of the window's other cells
            hole = torch.where(torch.isnan(x), torch.full_like(x, -INF), x)
            pinned = {"y": O.max_pool_same(hole, kk, s)}
        return Built(dtype, {"x": x, "k": kk, "s": s, "pt": pt, "pl": pl, "Ho": Ho, "Wo": Wo, "mode": mode}, {"y": y},
                     tol={"y": (1e-6, 8e-3)}, shape={"y": dw_reach(tuple(y.shape), pos, kk, 1, s, pt, pl)}, pinned=pinned)      # test_pool_same
    return build


CASES.append(Case("pool2d_fwd", "avg-k3-s2", build_pool("avg")))
CASES.append(Case("pool2d_fwd", "max-k3-s2", build_pool("max")))


def build_resize_bwd(align, Ho, Wo):
    N, H, W, C = 2, 9, 11, 8

    def build(dtype, payload):
        dy = rq(rnd((N, Ho, Wo, C), 2), F32)
        pos = [(0, 0, 0, 0), (0, Ho // 2, Wo // 2, 3), (N - 1, Ho - 1, Wo - 1, C - 1)]
        dy = poison(dy, pos, payload)
        xx = torch.zeros((N, H, W, C), dtype=torch.float64, requires_grad=True)
        O.resize_bilinear(xx, (Ho, Wo), align_corners=align).backward(dy)
        return Built(dtype, {"dy": dy, "H": H, "W": W, "align": align}, {"dx": xx.grad}, in_dtypes={"dy": F32}, tol={"dx": (2e-5, 1.2e-2)},
                     shape={"dx": resize_bwd_mask((N, H, W, C), Ho, Wo, pos, align)})
    return build


for _align in (False, True):
    CASES.append(Case("resize_bilinear_bwd", f"18x22-to-9x11-{'ac' if _align else 'hp'}", build_resize_bwd(_align, 18, 22), payloads=NAN_ONLY))
    CASES.append(Case("resize_bilinear_bwd", f"13x17-to-9x11-{'ac' if _align else 'hp'}", build_resize_bwd(_align, 13, 17), payloads=NAN_ONLY))


# ---------------------------------------------------------------------------------------------------------------------------
# attention forward (bf16, head_dim 64, T = 65: one whole 64-key tile and a ragged one): NaN only
# ---------------------------------------------------------------------------------------------------------------------------
ATT_TOL = (1.5e-2, 1.5e-2)      # tests/test_self_attention_gpu.py (the packed kernel is bit-identical per head: tests/test_attention_core_gpu.py)


def attention_ref(q, k, v, scale):
    return torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1) @ v


def build_attention(operand):
    B, T, heads, d = 2, 65, 2, 64
    C = heads * d

    def build(dtype, payload):
        qkv = rq(rnd((B, T, 3 * C), 1), dtype)
        mask = torch.zeros((B, T, C), dtype=torch.bool)
        if operand == "q":      # a query row of one head: that output row of that head
            pos = [(0, 0, 0), (0, T // 2, 8 + 3), (B - 1, T - 1, C - 1)]
            mask[0, 0, :d] = mask[0, T // 2, :d] = mask[B - 1, T - 1, d:] = True
        elif operand == "k":      # a key row: every query of that (batch, head)
            pos = [(0, 0, C), (B - 1, T - 1, 2 * C - 1)]
            mask[0, :, :d] = mask[B - 1, :, d:] = True
        else:      # a value element: its column, for every query of that batch
            pos = [(0, 0, 2 * C), (0, T // 2, 2 * C + 8 + 3), (B - 1, T - 1, 3 * C - 1)]
            mask[0, :, 0] = mask[0, :, 8 + 3] = mask[B - 1, :, C - 1] = True
        qkv = poison(qkv, pos, payload)
        qh, kh, vh = [qkv[..., i * C:(i + 1) * C].reshape(B, T, heads, d).permute(0, 2, 1, 3) for i in range(3)]
        out = attention_ref(qh, kh, vh, d ** -0.5).permute(0, 2, 1, 3).reshape(B, T, C)
        return Built(dtype, {"qkv": qkv, "heads": heads, "scale": d ** -0.5}, {"out": out}, tol={"out": ATT_TOL}, shape={"out": mask})
    return build


def build_self_attention(operand):
    B, T, dk, dv = 2, 65, 64, 64

    def build(dtype, payload):
        q, k, v = rq(rnd((B, T, dk), 1), dtype), rq(rnd((B, T, dk), 2), dtype), rq(rnd((B, T, dv), 3), dtype)
        mask = torch.zeros((B, T, dv), dtype=torch.bool)
        if operand == "q":
            pos = [(0, 0, 0), (0, T // 2, 8 + 3), (B - 1, T - 1, dk - 1)]
            q = poison(q, pos, payload)
            mask[0, 0] = mask[0, T // 2] = mask[B - 1, T - 1] = True
        elif operand == "k":
            pos = [(0, 0, 0), (0, T - 1, dk - 1)]
            k = poison(k, pos, payload)
            mask[0] = True
        else:
            pos = [(0, 0, 0), (0, T // 2, 8 + 3), (B - 1, T - 1, dv - 1)]
            v = poison(v, pos, payload)
            mask[0, :, 0] = mask[0, :, 8 + 3] = mask[B - 1, :, dv - 1] = True
        return Built(dtype, {"q": q, "k": k, "v": v, "scale": dk ** -0.5}, {"out": attention_ref(q, k, v, dk ** -0.5)}, tol={"out": ATT_TOL},
                     shape={"out": mask})
    return build


for _op in ("q", "k", "v"):
    CASES.append(Case("attention_fwd", f"T65-d64-{_op}", build_attention(_op), dtypes=(BF16,), payloads=NAN_ONLY))
    CASES.append(Case("self_attention_fwd", f"T65-dv64-{_op}", build_self_attention(_op), dtypes=(BF16,), payloads=NAN_ONLY))


# ---------------------------------------------------------------------------------------------------------------------------
# dense convolution on the implicit GEMM (bf16): NaN / Inf in one input element reaches its receptive field in every output channel
# ---------------------------------------------------------------------------------------------------------------------------
CONV = dict(N=2, H=9, W=11, Cin=16, Cout=16, k=3)


def pixels_mask(shape, per_channel_mask):
    return per_channel_mask.any(-1, keepdim=True).expand(shape).clone()


def build_conv_igemm(which):
    N, H, W, Cin, Cout, kk = (CONV[k] for k in ("N", "H", "W", "Cin", "Cout", "k"))

    def build(dtype, payload):
        x = rq(rnd((N, H, W, Cin), 1), dtype)
        w = rq(rnd((kk, kk, Cin, Cout), 2, (kk * kk * Cin) ** -0.5), dtype)
        b = rq(rnd((Cout,), 3), F32)
        dy = rq(rnd((N, H, W, Cout), 4), dtype)
        pos = SPATIAL_POS(N, H, W, Cin)
        if which == "fwd":
            x = poison(x, pos, payload)
            want = {"y": O.conv2d(x, w, b, 1, 1)}
            shape = {"y": pixels_mask((N, H, W, Cout), dw_reach((N, H, W, Cin), pos, kk, 1, 1, 1, 1))}
            tol = {}
        else:      # data gradient: the transposed footprint (symmetric for an odd kernel at stride 1)
            dy = poison(dy, pos, payload)
            xx = torch.zeros((N, H, W, Cin), dtype=torch.float64, requires_grad=True)
            O.conv2d(xx, w, None, 1, 1).backward(dy)
            want = {"dx": xx.grad}
            shape = {"dx": pixels_mask((N, H, W, Cin), dw_reach((N, H, W, Cout), pos, kk, 1, 1, 1, 1))}
            tol = {"dx": (2e-5, 1.5e-2)}      # test_conv_igemm_three_passes
        return Built(dtype, {"x": x, "w": w, "bias": b, "dy": dy, "which": which}, want, in_dtypes={"bias": F32}, tol=tol, shape=shape)
    return build


CASES.append(Case("conv2d_igemm", "fwd-2x9x11x16-k3", build_conv_igemm("fwd"), dtypes=(BF16,)))
CASES.append(Case("conv2d_igemm", "bwd_data-2x9x11x16-k3", build_conv_igemm("bwd_data"), dtypes=(BF16,)))


@case("conv2d_patch_fwd", "1x16x16x16-k4", dtypes=(BF16,))      # the smallest shape of tests/test_conv_patchify_gpu.py: kernel == stride
def build_conv_patch(dtype, payload):
    N, H, W, Cin, Cout, kk = 1, 16, 16, 16, 32, 4
    x = rq(rnd((N, H, W, Cin), 1), dtype)
    w = rq(rnd((kk, kk, Cin, Cout), 2, (kk * kk * Cin) ** -0.5), dtype)
    b = rq(rnd((Cout,), 3), F32)
    pos = [(0, 0, 0, 0), (0, H // 2 + 1, W // 2 + 2, 8 + 3), (0, H - 1, W - 1, Cin - 1)]
    x = poison(x, pos, payload)
    mask = torch.zeros((N, H // kk, W // kk, Cout), dtype=torch.bool)
    for n, h, w_, _ in pos:      # a patch belongs to exactly one output pixel
        mask[n, h // kk, w_ // kk] = True
    return Built(dtype, {"x": x, "w": w, "bias": b, "k": kk}, {"y": O.conv2d(x, w, b, kk, 1)}, in_dtypes={"bias": F32}, shape={"y": mask})


@case("conv2d_branches_fwd", "2x8x8x64-k1-k3d3", dtypes=(BF16,))      # tests/test_conv_branches_gpu.py, its smallest map
def build_conv_branches(dtype, payload):
    N, H, W, Cin, Cout = 2, 8, 8, 64, 64
    taps = [(1, 1), (3, 3)]
    x = rq(rnd((N, H, W, Cin), 1), dtype)
    pos = SPATIAL_POS(N, H, W, Cin)
    x = poison(x, pos, payload)
    inputs, want, shape = {"x": x, "taps": taps}, {}, {}
    for i, (kk, d) in enumerate(taps):
        w = rq(rnd((kk, kk, Cin, Cout), 10 + i, (kk * kk * Cin) ** -0.5), dtype)
        inputs[f"w{i}"] = w
        want[f"y{i}"] = O.conv2d(x, w, None, 1, d)
        pad = (kk - 1) * d // 2
        shape[f"y{i}"] = pixels_mask((N, H, W, Cout), dw_reach((N, H, W, Cin), pos, kk, d, 1, pad, pad))
    return Built(dtype, inputs, want, shape=shape)


@case("jpu_dwconv3x4_stats", "2x9x11x24")      # tests/test_jpu_fused_gpu.py test_stats_message
def build_jpu(dtype, payload):
    N, H, W, C = 2, 9, 11, 24
    x = rq(rnd((N, H, W, C), 1), dtype)
    w, b = rq(rnd((4, 9, C), 2) / 3, F32), rq(rnd((4, C), 3) * 0.5, F32)
    pos = SPATIAL_POS(N, H, W, C)
    x = poison(x, pos, payload)
    z = torch.stack([O.depthwise_conv2d(x, w[i].reshape(3, 3, C, 1), b[i], 1, r, "same") for i, r in enumerate((1, 2, 4, 8))])
    mask = torch.stack([dw_reach((N, H, W, C), pos, 3, r, 1, r, r) for r in (1, 2, 4, 8)])
    return Built(dtype, {"x": x, "w": w, "bias": b}, {"z": z}, in_dtypes={"w": F32, "bias": F32}, tol={"z": (1e-5, 8e-3)}, shape={"z": mask})


@case("bn_swish_se_fwd", "4x5x7x24-se4", payloads=NAN_ONLY)      # tests/test_mbconv_fused_gpu.py; swish: NaN only
def build_bn_swish_se(dtype, payload):
    # a NaN at (sample n, channel c) makes the squeezed mean m[n, c] NaN, through the excite product every gate of sample n, and so the sample
    N, H, W, C, Cse = 4, 5, 7, 24, 4
    x = rq(rnd((N, H, W, C), 1), dtype)
    st = {"mean": rq(rnd((C,), 4) * 0.2, F32), "rstd": rq(rnd((C,), 5).abs() * 0.2 + 0.7, F32), "gamma": rq(rnd((C,), 6).abs() + 0.5, F32),
          "beta": rq(rnd((C,), 7) * 0.3, F32), "W1": rq(rnd((C, Cse), 8) * C ** -0.5, F32), "b1": rq(rnd((Cse,), 9) * 0.1, F32),
          "W2": rq(rnd((Cse, C), 10) * Cse ** -0.5, F32), "b2": rq(rnd((C,), 11) * 0.1, F32)}
    pos = [(0, 0, 0, 0), (0, H // 2, W // 2, 8 + 3), (0, H - 1, W - 1, C - 1)]
    x = poison(x, pos, payload)
    swish = lambda t: t * torch.sigmoid(t)
    a = swish((x - st["mean"]) * st["rstd"] * st["gamma"] + st["beta"])
    g = torch.sigmoid(swish(a.mean(dim=(1, 2)) @ st["W1"] + st["b1"]) @ st["W2"] + st["b2"])
    mask = torch.zeros((N, H, W, C), dtype=torch.bool)
    mask[0] = True
    return Built(dtype, dict(st, x=x), {"out": a * g[:, None, None, :]}, in_dtypes={k: F32 for k in st}, tol={"out": (1e-5, 1e-2)}, shape={"out": mask})


# ---------------------------------------------------------------------------------------------------------------------------
# upsample_ce: the fused logits tail.  No ignored pixel: what an ignored pixel does with a NaN is the softmax_ce deviation above.
# ---------------------------------------------------------------------------------------------------------------------------
@case("upsample_ce", "2x3x4x21-x16", payloads=NAN_ONLY)
def build_upsample_ce(dtype, payload):
    N, Hi, Wi, C, sy, sx = 2, 3, 4, 21, 16, 16
    Ho, Wo = Hi * sy, Wi * sx
    z = rq(rnd((N, Hi, Wi, C), 1) * 2, dtype)
    y = torch.randint(0, C, (N, Ho, Wo), generator=gen(5), dtype=torch.int32)
    pos = [(0, 0, 0, 0), (N - 1, Hi - 1, Wi - 1, C - 1)]
    z = poison(z, pos, payload)
    zz = z.clone().requires_grad_(True)
    loss = O.softmax_ce_ignore(y, O.resize_bilinear(zz, (Ho, Wo)), C, IGNORE).mean()
    loss.backward()
    # the loss of every output pixel that reads the poisoned source pixel is NaN, and its gradient is NaN in every class of every source pixel
    # it reads: the source pixels that share an output pixel with the poisoned one
    reach = resize_fwd_mask((N, Ho, Wo, C), Hi, Wi, pos, False).any(-1)
    back = torch.zeros((N, Hi, Wi), dtype=torch.bool)
    ty, tx = resize_taps(Ho, Hi, False), resize_taps(Wo, Wi, False)
    for n, oy, ox in reach.nonzero().tolist():
        for h in ty[oy]:
            for w in tx[ox]:
                back[n, h, w] = True
    return Built(dtype, {"z": z, "y": y, "Ho": Ho, "Wo": Wo}, {"dz": zz.grad, "sum": loss.detach().reshape(1)}, in_dtypes={"y": torch.int32},
                 tol={"dz": (2e-5, 1e-2), "sum": (2e-5, 2e-5)}, out_dtypes={"sum": F32},      # test_upsample_ce_matches_oracle_and_separate_kernels
                 shape={"dz": back[..., None].expand(N, Hi, Wi, C).clone(), "sum": torch.ones(1, dtype=torch.bool)})


# ---------------------------------------------------------------------------------------------------------------------------
# window attention (ws 7, shift mask 0 / -100: every key stays visible) and Gemma's causal GQA attention (keys CAN be hidden): NaN only
# ---------------------------------------------------------------------------------------------------------------------------
def build_window_attention(operand):
    B, ws, heads, d, nW = 6, 7, 2, 32, 3
    T, C = ws * ws, heads * d

    def build(dtype, payload):
        from tests.test_attention_gpu import _ref_attention

        qkv = rq(rnd((B, T, 3 * C), 1), dtype)
        bias = rq(rnd((heads, T, T), 3) * 0.5, F32)
        shift = rq(torch.where(rnd((nW, T, T), 9) > 0.3, torch.tensor(-100.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)), F32)
        mask = torch.zeros((B, T, C), dtype=torch.bool)
        if operand == "q":
            pos = [(0, 0, 0), (1, T // 2, 8 + 3), (B - 1, T - 1, C - 1)]
            mask[0, 0, :d] = mask[1, T // 2, :d] = mask[B - 1, T - 1, d:] = True
        else:      # a key row: every query of that (window, head)
            pos = [(0, 0, C), (B - 1, T - 1, 2 * C - 1)]
            mask[0, :, :d] = mask[B - 1, :, d:] = True
        qkv = poison(qkv, pos, payload)
        out = _ref_attention(qkv, heads, C, d ** -0.5, bias, shift)
        return Built(dtype, {"qkv": qkv, "bias": bias, "shift": shift, "heads": heads, "scale": d ** -0.5}, {"out": out.reshape(B, T, C)},
                     in_dtypes={"bias": F32, "shift": F32}, tol={"out": ATT_TOL}, shape={"out": mask})      # test_fused_window_attention_matches_...: 1.5e-2
    return build


for _op in ("q", "k"):
    CASES.append(Case("window_attention_fwd", f"ws7-shift-{_op}", build_window_attention(_op), dtypes=(BF16,), payloads=NAN_ONLY))


GEMMA = dict(B=2, T=65, nq=4, nkv=2, h=64)


def build_gemma_attention(kind):
    B, T, nq, nkv, h = (GEMMA[k] for k in ("B", "T", "nq", "nkv", "h"))
    g = nq // nkv

    def build(dtype, payload):
        from tests import gemma_ref as GR

        qkv = rq(rnd((B, T, (nq + 2 * nkv) * h), 1), dtype)
        pad = torch.ones((B, T), dtype=torch.uint8)
        Cq = nq * h
        keys = [(0, 5, 0), (B - 1, T - 1, nkv - 1)]      # (batch, key, kv head): one in the first key tile, one in the ragged last tile
        pos = [(keys[0][0], keys[0][1], Cq + keys[0][2] * h), (keys[1][0], keys[1][1], Cq + keys[1][2] * h + h - 1)]
        if kind == "hidden":
            for b_, s_, _ in keys:
                pad[b_, s_] = 0

        def ref(t):
            q, k, v = t[..., :Cq].reshape(B, T, nq, h), t[..., Cq:Cq + nkv * h].reshape(B, T, nkv, h), t[..., Cq + nkv * h:].reshape(B, T, nkv, h)
            return GR.attention_core(q, k, v, pad, nq, nkv)
        clean = ref(qkv)
        want = ref(poison(qkv, pos, payload))
        # DEVIATIONS: a key that the padding or the causal mask hides from a query never enters that query's row (csrc/gemma.hip: `if (vis)` in
        # front of the maximum and the exponential); the reference ADDS -1e9 to the NaN score, so its whole (batch, kv head) group is NaN
        pinned = clean.clone()
        if kind == "visible":
            for b_, s_, kv in keys:
                pinned[b_, s_:, kv * g * h:(kv + 1) * g * h] = NAN      # the queries t >= s of the g query heads that share kv head `kv`
        return Built(dtype, {"qkv": poison(qkv, pos, payload), "pad": pad, "nq": nq, "nkv": nkv, "h": h, "scale": h ** -0.5}, {"out": want},
                     in_dtypes={"pad": torch.uint8}, tol={"out": ATT_TOL}, pinned={"out": pinned})      # test_core_both_routes_against_fp64: 1.5e-2
    return build


for _kind in ("hidden", "visible"):
    CASES.append(Case("gemma_attention_fwd", f"T65-key-{_kind}", build_gemma_attention(_kind), dtypes=(BF16,), payloads=NAN_ONLY))


# ---------------------------------------------------------------------------------------------------------------------------
# deviations: (family, case) -> (reason, exact expected behaviour).  DESIGN.md "Non-finite values" carries the same text.
# ---------------------------------------------------------------------------------------------------------------------------
_CE_IGNORED = ("skipped data: the loss of a pixel whose label is the ignore label is written as a literal 0 and its logits never enter it "
               "(csrc/loss.hip softmax_ce_kernel: `my_loss = in_range ? w * ... : 0.f`); the reference multiplies the NaN loss by a zero weight",
               "loss_px is exactly the reference's on the clean logits (0 at the ignored pixel) and the sum is finite")
_CE_GATHER = ("skipped data: the plain cross-entropy reads the label's logit alone (csrc/loss.hip softmax_ce_kernel: `w * (__logf(se) - (zy - mx))`); the "
              "reference sums onehot_c * log p_c over the classes, and 0 * log(0) is NaN for a -Inf logit of another class",
              "loss_px = logsumexp(z) - z[label]: finite for a -Inf logit of another class (its exp is 0), +Inf for a -Inf logit of the label, NaN for "
              "a NaN or a +Inf logit anywhere in the row, exactly as the reference in those three")
DEVIATIONS = {("softmax_ce", f"C{C}-{m}-ignored"): _CE_IGNORED for C in (21, 65) for m in ("plain", "focal")}
DEVIATIONS.update({("softmax_ce", f"C{C}-plain-valid"): _CE_GATHER for C in (21, 65)})
_GEMMA = ("skipped data: a key that the padding mask or the causal mask hides from a query never enters that query's row (csrc/gemma.hip "
          "gemma_attn_fwd_kernel: `if (vis) mx = fmaxf(mx, s)` and the masked probability is a literal 0); the reference adds -1e9 to the NaN score, "
          "which stays NaN in every row of that (batch, kv head)",
          "the queries that may see the poisoned key (t >= s, padding_mask[s] != 0) are NaN in the query heads of its kv head; every other output "
          "is the reference's on the clean input -- all of them when the padding mask hides the key")
DEVIATIONS[("gemma_attention_fwd", "T65-key-hidden")] = _GEMMA
DEVIATIONS[("gemma_attention_fwd", "T65-key-visible")] = _GEMMA
DEVIATIONS[("dwconv2d7_mfma", "2x20x19x32")] = (
    "declared behaviour (docstring of tests/test_dwconv_mfma_gpu.py::test_dwconv7_mfma_is_bit_reproducible_and_confines_non_finite_inputs): the "
    "matrix pipe multiplies a pixel by the zeros of the banded weight operand as well, and 0 * NaN = 0 * Inf = NaN",
    "the 49 outputs whose window holds the pixel are the reference's; NaN besides in the rest of the 4-row output blocks rho // 4 - 2 .. rho // 4 of "
    "each 16-row tile whose raw tile holds the pixel at row rho (at most 5 more rows), in the same 7 columns of that channel; nothing else")
DEVIATIONS[("pool2d_fwd", "max-k3-s2")] = (
    "max pooling: today's behaviour pinned (csrc/misc.hip pool2d_fwd_kernel: `acc = fmaxf(acc, v)` returns the operand that is not NaN); the "
    "reference's own source does not settle what tf.nn.max_pool does with a NaN",
    "a NaN cell is skipped: the output is the maximum of the window's other cells; +Inf and -Inf take part as values")

# behaviour that a docstring already declares -> (where it is declared, the case or test that pins it)
DECLARED = {
    "AdamW scrubs NaN gradients, SGD does not": ("iseg_amd/optimizers/modern.py _scrub_nan; csrc/optim.hip",
                                                 "tests/test_optimizer_gpu.py::test_sgd_does_not_scrub_nan_and_adamw_does"),
    "attention layers do not materialise the reference's replace_inf / replace_nan passes": (
        "docstring of iseg_amd/layers/multihead_self_attention.py", "softmax_rows_fwd-*-clip, attention_fwd-*, self_attention_fwd-*, window_attention_fwd-*"),
    "mask_loss scrubs a NaN term to 0, as the reference does": ("csrc/mask_loss.hip", "mask_loss-ce-plain, mask_loss-ce-focal"),
    "dwconv2d7_mfma spreads a non-finite pixel over the 4-row blocks of its band": ("tests/test_dwconv_mfma_gpu.py", "dwconv2d7_mfma-2x20x19x32"),
}

# kernels that turn a float into an index, an offset, a threshold or a loop bound: never fed a non-finite value on the device
NOT_COVERED = ("OHEM selection", "SOD / F-measure / confusion histograms", "connected-components labelling", "augment and projective transforms",
               "the sampling offsets of DCNv2, DCNv3 and deformable attention")
