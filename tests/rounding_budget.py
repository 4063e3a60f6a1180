"""The rounding budget of the bf16-storage kernels: is a bf16 output THE once-rounded result (fp32-accurate value, one round-to-nearest-even
store), or merely within a few ulps of the largest element, which is all close() of tests/test_kernels_gpu.py asks?  Test infrastructure only:
torch on the CPU, shared by tests/test_rounding_budget_host.py (CPU) and tests/test_rounding_budget_gpu.py (device).

    rounding_stats(got_bf16, want64) -> Stats(share, max_abs_e, bias_mag, bias)
        share      fraction of ALL elements with got == bf16(want64), compared as values (so +0 == -0); bf16(want64) is ONE nearest-even rounding
                   of the fp64 value (ideal_bf16: torch's own fp64 -> bf16 conversion goes through fp32 and double-rounds about 1 value in 1e5,
                   which is the size of the effect measured here)
        e          (got - want) / ulp, ulp = 2^(floor(log2(max(|want|, rms(want) / 16))) - 7): near-zero outputs count in the ulp of a typical
                   element (rms / 16), not in their own vanishing ulp
        max_abs_e  max |e|;  bias_mag = mean(e sign(want)) (a truncating store: -0.48);  bias = mean(e)
    mutants(y32)  the three precision defects that fit inside close() at 1.2e-2, applied to an fp32 result (host test only: they prove that the
                  statistic can fail)
    failures(...) the four conditions of the device test, as a list of messages (empty: met)

A Case holds seeded inputs (the rnd() Gaussians of tests/test_kernels_gpu.py, rounded to bf16 BEFORE either side sees them; per-channel parameters
and saved statistics are fp32, as the kernels take them) and ONE dtype-generic formula, `compute`.  Run in torch.float64 it is the reference
(oracle/tf_ops.py where the operation has an oracle); run in torch.float32 it is the restatement: the same arithmetic in fp32, whose reductions
run in another order (torch's blocked fp32 kernels; the GEMMs are summed over four slabs of K explicitly, see mm()).

Tier 1 (single rounding): the reference is the plain fp64 formula.  Tier 2 (restated): the kernel evaluates an approximation or rounds an
intermediate BY DESIGN, as a kernel comment states; the reference is fp64 with exactly that step inserted, and the inserted step cites the
comment as `# iseg_amd/csrc/<file>:<line>`.  DESIGN.md ("Rounding points") lists every family with its tier.

BUDGET[family] is the share the fp32 restatement reaches over the family's cases (pooled), measured once and written down;
test_every_budget_entry_is_backed_by_the_restatement keeps it honest.  The device floor is derived from it (share_floor).
"""
import functools
import inspect
import math
from typing import NamedTuple

import torch

from oracle import tf_ops as O
from tests import sampling_kinks as SK
from tests.test_kernels_gpu import rnd

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MIN_N = 40000            # every output has at least this many elements: 6 sigma of the mean of n once-rounded errors is then <= 0.009 ulp
SIGMA = 0.2887           # standard deviation of an error that is uniform in +-1/2 ulp
ACT_RELU, ACT_GELU, ACT_GELU_GRAD, ACT_RELU_GRAD, ACT_MUL_AUX, ACT_SIGMOID, ACT_SWISH = 1, 2, 3, 4, 5, 6, 7      # include/iseg_hip.h

# family -> share of the fp32 restatement (pooled over the family's cases), as measured on the CPU.  1.0: the fp32 value is exact or the output is
# an input value, so every element must be ideal.  Each entry is written with 1 - BUDGET = 1.25 x the measured 1 - share (the measured share is in the
# comment): the middle of what test_every_budget_entry_is_backed_by_the_restatement allows, so that the few elements another CPU's fp32 summation
# order moves do not tip it.
BUDGET = {
    "cast": 1.0,
    "elementwise_exact": 1.0,
    "elementwise": 0.9999955,     # 0.999996
    "gemm_fwd": 0.999909,         # 0.999927
    "gemm_dgrad": 0.999936,       # 0.999949
    "layernorm": 0.999964,        # 0.999971
    "batchnorm": 0.999979,        # 0.999983
    "norms": 0.99997,             # 0.999976
    "dwconv": 0.999914,           # 0.999931
    "conv": 0.99989,              # 0.999911
    "resize": 0.9992,             # 0.999362: the interpolation weights put many products next to a bf16 tie
    "resize_x2": 1.0,             # weights 1/4 and 3/4: every fp32 value is exact
    "upsample_ce": 0.999935,      # 0.999948
    "dwconv_mfma": 0.999965,      # 0.999972
    "mlp_fused": 0.999925,        # 0.999940
    "mlp_fused_fwd": 0.99959,     # 0.999672
    "mlp_fused_bwd_data": 0.99914,      # 0.999311
    "attention_flash": 0.99941,   # 0.999531
    "attention_flash_bwd": 0.99954,     # 0.999635
    "attention_window": 0.99972,  # 0.999779
    "attention_self": 0.99929,    # 0.999433
    "attention_self_bwd": 0.99895,      # 0.999163
    "gelu_approx": 0.9982,          # 0.998562: the degree-6 / degree-7 polynomials cancel, so their fp32 value depends on the evaluation order
    "gelu_approx_act": 0.999905,    # 0.999924
    "dcnv3": 0.99727,               # 0.997819: see FP32_COORDINATES
    "dcnv3_bwd": 0.99807,           # 0.998456 (mask gradient and the interior elements of the offset gradient)
    "dcnv2_sample": 0.999976,       # 0.999981 (the coordinate is one addition)
    "dcnv2_sample_bwd": 0.999952,   # 0.999961 (logit gradients and the interior elements of the offset gradients)
    "defattn": 0.99852,             # 0.998817
    "defattn_bwd": 0.99869,         # 0.998950 (value / attention gradients and the interior elements of the offset gradient)
}

# Tier-1 families whose fp32 restatement is NOT within 1e-3 ulp of a perfect store, and why: the sampling coordinate is computed in fp32 (as the
# kernels do: iseg_amd/csrc/dcnv3.hip:14-15, iseg_amd/csrc/defattn.hip:11-12) through a chain of 7 to 10 roundings at the magnitude of the image
# size, and a bilinear weight is that coordinate minus its floor: an absolute error of up to TAU / 4 ~ 1e-5 (tests/sampling_kinks.py) in a weight of
# order 1 is ~1e-5 of the output, 2.5e-3 of a bf16 ulp per tap and up to ~10 times that where the taps of an output cancel.  The restatement's
# measured max |e| (0.512 / 0.526 / 0.513 / 0.502 ulp) is held below the figure written here, and condition 2 of the device test scales its
# excess as everywhere.  DCNv2's coordinate is one addition: its families meet the 1e-3 of every other tier-1 family.
FP32_COORDINATES = {"dcnv3": 0.53, "dcnv3_bwd": 0.53, "defattn": 0.53, "defattn_bwd": 0.53}

# Families whose kernel rounds an intermediate to bf16 that never leaves the CU (the probabilities of the attention cores, G / dH of the fused MLP
# forward and data-gradient kernels).  One element of that intermediate which fp32 and fp64 round differently moves an output by the
# intermediate's ulp times one operand -- several ulps of a small output -- in ANY fp32 evaluation, the restatement included, so the 0.75 cap of
# condition 2 (faithful rounding) cannot hold there.  Conditions 1 and 3 are asserted as everywhere; condition 2 keeps its form,
# 0.5 + 8 x (restatement's max |e| - 0.5), with the restatement's figure written down here (measured value in the comment;
# test_unstored_max_e_is_backed_by_the_restatement holds it as BUDGET is held) and without the cap.
UNSTORED_MAX_E = {
    "mlp_fused_fwd": 2.6,           # 2.347
    "mlp_fused_bwd_data": 3.8,      # 3.374
    "attention_flash": 2.1,         # 1.865
    "attention_flash_bwd": 1.9,     # 1.738
    "attention_self": 3.9,          # 3.485
    "attention_self_bwd": 9.3,      # 8.345 (dQ: one dS next to a tie times a key of 3, against the ulp of a small dQ)
    "attention_window": 6.5,        # 5.774 (dK: a probability near 1 times a query of 3)
}

# mutants that have no meaning for a family (the host test skips them there and asserts nothing about them)
MUTANTS_SKIPPED = {
    "cast": {"bf16_partials": "no reduction", "double_rounding": "no intermediate: the input is the value to round"},
    "elementwise_exact": {"truncate": "the result is an input value or zero, which every store keeps", "bf16_partials": "no reduction",
                          "double_rounding": "nothing to round"},
    "elementwise": {"bf16_partials": "no reduction"},
    "resize": {"bf16_partials": "four-tap interpolation, no slabs"},
    "resize_x2": {"bf16_partials": "four-tap interpolation, no slabs"},
    "gelu_approx_act": {"bf16_partials": "no reduction"},
}


# ---------------------------------------------------------------------------------------------------------------------------
# the statistic
# ---------------------------------------------------------------------------------------------------------------------------
class Stats(NamedTuple):
    share: float
    max_abs_e: float
    bias_mag: float
    bias: float


def ideal_bf16(want64):
    """fp64 -> bf16 by ONE round-to-nearest-even (on the bit pattern: 45 mantissa bits go)"""
    bits = want64.to(F64).contiguous().view(torch.int64)
    lsb = (bits >> 45) & 1
    r = (bits + ((1 << 44) - 1) + lsb) & -(1 << 45)
    return r.view(F64).to(BF)      # exact: 8 significant bits


def errors_in_ulps(got, want64):
    want = want64.to(F64).reshape(-1)
    rms = want.pow(2).mean().sqrt().item()
    floor = max(rms / 16, 1e-30)
    _, ex = torch.frexp(want.abs().clamp(min=floor))      # |want| = m 2^ex, m in [0.5, 1): floor(log2 |want|) = ex - 1
    ulp = torch.exp2((ex - 1 - 7).to(F64))
    return (got.detach().cpu().reshape(-1).to(F64) - want) / ulp


def rounding_stats(got, want64):
    g = got.detach().cpu().reshape(-1)
    assert g.dtype == BF and g.numel() == want64.numel()
    want = want64.to(F64).reshape(-1)
    same = g.to(F64) == ideal_bf16(want).to(F64)
    e = errors_in_ulps(g, want)
    return Stats(same.double().mean().item(), e.abs().max().item(), (e * torch.sign(want)).mean().item(), e.mean().item())


def worst_elements(got, want64, k=10):
    g = got.detach().cpu().reshape(-1)
    want = want64.to(F64).reshape(-1)
    ideal = ideal_bf16(want)
    e = errors_in_ulps(g, want).abs()
    e = torch.where(g.to(F64) == ideal.to(F64), torch.zeros_like(e), e + 1e-9)      # wrong elements first, worst first
    idx = torch.topk(e, min(k, e.numel())).indices.tolist()
    return [(i, g[i].item(), want[i].item(), ideal[i].item()) for i in idx if e[i] > 0]


def share_floor(family):
    """1 - BUDGET is what fp32 accumulation in SOME order costs; 8 x is the margin for the matrix cores' order and adder tree; never below 0.95"""
    return max(0.95, 1.0 - 8.0 * (1.0 - BUDGET[family]))


def max_e_bound(restated_max, family=None):
    """faithful rounding: 8 x the restatement's excess over the 1/2 ulp of a perfect store, never above 0.75 (UNSTORED_MAX_E families: no cap)"""
    bound = 0.5 + 8.0 * max(restated_max - 0.5, 0.0)
    return bound if family in UNSTORED_MAX_E else min(0.75, bound)


def bias_bound(n, share):
    """an unbiased store: 6 sigma of the mean of n uniform errors, plus 1 ulp for each element that is not the ideal one"""
    return 6.0 * SIGMA / math.sqrt(n) + (1.0 - share)


def independent_n(values):
    """how many independent rounding errors a one-operand kernel's output holds: equal inputs give equal errors, so the mean error is a mean over
    the DISTINCT input values weighted by their counts, and its variance is sigma^2 sum(w^2): n_eff = 1 / sum(w^2).  (A Gaussian in bf16 has a
    few thousand distinct values however many elements are drawn.)"""
    _, counts = torch.unique(values.reshape(-1).to(F32), return_counts=True)
    w = counts.to(F64) / counts.sum()
    return int(1.0 / (w * w).sum().item())


def failures(st, n, family, restated_max, n_indep=None):
    """restated_max: family_max_e(family).  n_indep: the number of independent errors where it is below n (one-operand kernels: Case.independent); the bias bounds use it"""
    bad = []
    nb = n if n_indep is None else min(n, n_indep)
    if n < MIN_N:
        bad.append(f"only {n} elements (< {MIN_N})")
    if not st.share >= share_floor(family):
        bad.append(f"share {st.share:.6f} < {share_floor(family):.6f} (BUDGET {BUDGET[family]})")
    if not st.max_abs_e <= max_e_bound(restated_max, family):
        bad.append(f"max |e| {st.max_abs_e:.4f} ulp > {max_e_bound(restated_max, family):.4f} (restatement: {restated_max:.4f})")
    if not abs(st.bias_mag) <= bias_bound(nb, st.share):
        bad.append(f"|bias_mag| {abs(st.bias_mag):.4f} ulp > {bias_bound(nb, st.share):.4f}")
    if not abs(st.bias) <= bias_bound(nb, st.share):
        bad.append(f"|bias| {abs(st.bias):.4f} ulp > {bias_bound(nb, st.share):.4f}")
    return bad


def report(what, got, want64, st):
    rows = "\n".join(f"    [{i}] got {g!r} want64 {w!r} ideal {d!r}" for i, g, w, d in worst_elements(got, want64))
    return f"{what}: share {st.share:.6f} max|e| {st.max_abs_e:.4f} bias_mag {st.bias_mag:+.5f} bias {st.bias:+.5f}\n{rows}"


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants
# ---------------------------------------------------------------------------------------------------------------------------
PARTIAL_WEIGHTS = (1.25, -0.75, 0.75, -0.25)      # four slabs that sum to the result, with the cancellation a real reduction has


def mutants(y32):
    """-> {name: bf16 tensor}: what three defective kernels would store for the fp32 result y32
    truncate         the store drops the low 16 bits instead of rounding to nearest-even
    bf16_partials    the result reaches the epilogue as four slab sums kept in bf16 and added in bf16
    double_rounding  an intermediate (the value before a final multiply by a per-layer scale) is rounded to bf16 first"""
    y = y32.to(F32).contiguous()
    trunc = (y.view(torch.int32) & -65536).view(F32).to(BF)
    acc = torch.zeros_like(y, dtype=BF)
    for w in PARTIAL_WEIGHTS:
        acc = (acc.to(F32) + (y * w).to(BF).to(F32)).to(BF)
    twice = ((y * 1.3125).to(BF).to(F32) / 1.3125).to(BF)
    return {"truncate": trunc, "bf16_partials": acc, "double_rounding": twice}


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def bq(shape, seed, scale=1.0, shift=0.0):
    """a storage operand: seeded Gaussian, rounded to bf16"""
    return (rnd(shape, seed, scale) + shift).to(BF)


def par(shape, seed, scale=1.0, shift=0.0):
    """a per-channel parameter or saved statistic: fp32"""
    return (rnd(shape, seed, scale) + shift).to(F32)


def f32c(v):
    """a scalar argument as the C ABI receives it (float)"""
    return torch.tensor(v, dtype=F32).item()


def mm(a, b):
    """a [M, K] @ b [K, N]; in fp32 as four slabs of K added one after the other (a summation order of its own)"""
    if a.dtype != F32:
        return a @ b
    K = a.shape[1]
    step = -(-K // 4)
    acc = None
    for k0 in range(0, K, step):
        part = a[:, k0:k0 + step] @ b[k0:k0 + step]
        acc = part if acc is None else acc + part
    return acc


def _call(fn, *args, **p):
    """fn(*args, **the entries of p that fn names)"""
    names = inspect.signature(fn).parameters
    if any(v.kind == v.VAR_KEYWORD for v in names.values()):
        return fn(*args, **p)
    return fn(*args, **{k: v for k, v in p.items() if k in names})


def rb(x):
    """a value handed on in bf16 (an MFMA operand, a weight image): rounded once, back in the dtype of the computation"""
    return (ideal_bf16(x) if x.dtype == F64 else x.to(BF)).to(x.dtype)


class Case:
    def __init__(self, family, name, kind, make, compute, tier=1, **p):
        self.family, self.name, self.kind, self.make, self.compute, self.tier, self.p = family, name, kind, make, compute, tier, p
        self._inputs = None

    @property
    def id(self):
        return f"{self.family}/{self.name}"

    def inputs(self):
        if self._inputs is None:
            self._inputs = _call(self.make, **self.p)
        return self._inputs

    def independent(self):
        """None, or the number of independent rounding errors of a kernel whose every output is a function of ONE input element (`one=` names it)"""
        return independent_n(self.inputs()[self.p["one"]]) if "one" in self.p else None

    def fed(self, outputs):
        """{input name: bf16 tensor} for the cases with `feed={input: output}`: an intermediate that the kernel rounds to bf16 AND stores is handed
        to the reference as the side under test stored it (the device's on the device, the restatement's on the host).  Otherwise one element
        of the intermediate that fp32 and fp64 round differently moves an output behind it by several of its ulps, in the restatement too."""
        return {inp: outputs[out].detach().cpu().to(BF) for inp, out in self.p.get("feed", {}).items()}

    def selected(self, outputs):
        """the cases with `select=` (a function -> {output: boolean mask}) enter with the masked elements of those outputs only, as flat CPU
        tensors: the offset gradients of the sampling kernels are discontinuous at cell borders, where fp32 and fp64 may stand on different
        sides, and only their interior elements are a statement about rounding (the others: tests/test_sampling_kinks_gpu.py)"""
        if "select" not in self.p:
            return outputs
        masks = self.p["select"]()
        return {k: (v.detach().cpu()[masks[k]] if k in masks else v) for k, v in outputs.items()}

    def outputs(self, dtype, fed=None):
        """{output name: tensor in `dtype`}: torch.float64 = the reference, torch.float32 = the restatement"""
        i = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in dict(self.inputs(), **(fed or {})).items()}
        with torch.enable_grad():
            return {k: v.detach() for k, v in _call(self.compute, i, **self.p).items()}


CASES = []


def case(family, name, kind, make, compute, tier=1, **p):
    CASES.append(Case(family, name, kind, make, compute, tier, **p))


# ---- cast: the purest probe of the store's rounding mode -------------------------------------------------------------------
def make_cast():
    g = torch.Generator().manual_seed(71)
    x = torch.randn(49152, generator=g, dtype=F32) * torch.exp2(torch.randint(-2, 3, (49152,), generator=g).to(F32))
    b = bq((16384,), 72, 3.0).to(F32)
    _, ex = torch.frexp(b.abs().clamp(min=1e-30))
    ties = b + torch.exp2((ex - 1 - 8).to(F32))      # bf16 + 1/2 ulp, exact in fp32: nearest-even must pick the even neighbour
    return {"x": torch.cat([x, ties])}


case("cast", "fp32_to_bf16_with_ties", "cast", make_cast, lambda i: {"y": i["x"]})


# ---- elementwise ------------------------------------------------------------------------------------------------------------
EW = (4096, 96)      # large enough that the handful of elements an fp32 evaluation order moves is a stable share, not a count of 0 to 3


def make_pair():
    return {"a": bq(EW, 1), "b": bq(EW, 2)}


# scalars with a few bits: every product is exact in fp32, so the fp32 value is the fp64 value and the store alone decides the result (a scalar
# like 0.7f puts one product in ~200 within 1e-8 of a bf16 tie, which fp32 arithmetic itself then rounds twice)
ALPHA, BETA, BSCALE = 0.75, -1.375, 0.375
case("elementwise", "axpby", "axpby", make_pair, lambda i, alpha, beta: {"y": alpha * i["a"] + beta * i["b"]}, alpha=ALPHA, beta=BETA)
case("elementwise", "add", "axpby", make_pair, lambda i, alpha, beta: {"y": i["a"] + i["b"]}, alpha=1.0, beta=1.0)
case("elementwise", "add_relu", "add_relu", make_pair, lambda i: {"y": torch.relu(i["a"] + i["b"])})
case("elementwise", "rowscale", "rowscale", lambda rpg, **_: {"x": bq(EW, 3), "s": torch.tensor([0.0, 1.25, 0.75, 1.375], dtype=F32)},
     lambda i, rpg: {"y": i["x"] * i["s"].repeat_interleave(rpg)[:, None]}, rpg=1024)
case("elementwise", "broadcast_rows", "broadcast_rows", lambda B, R, scale: {"v": bq((B, 96), 4)},
     lambda i, B, R, scale: {"y": (scale * i["v"])[:, None, :].expand(B, R, 96).contiguous()}, B=512, R=4, scale=BSCALE, one="v")


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def act_value(x, act):
    return {ACT_RELU: torch.relu, ACT_SIGMOID: sigmoid, ACT_SWISH: lambda v: v * sigmoid(v)}[act](x)


def act_deriv(a, act):
    if act == ACT_RELU:
        return (a > 0).to(a.dtype)
    s = sigmoid(a)
    return s * (1 - s) if act == ACT_SIGMOID else s * (1 + a * (1 - s))


def make_act(seed=5, away_from_zero=False, **_):
    """away_from_zero (sigmoid): x = +-(1.5 + N(0, 0.5)).  sigmoid' is flat at 0, so dy * sigmoid'(x) lies just inside dy / 4 -- a bf16 value
    times a power of two -- for every |x| < 0.09 and always rounds outward: 7% of a unit Gaussian would put +0.007 ulp on bias_mag by themselves"""
    x = rnd(EW, seed)
    if away_from_zero:
        x = (1.5 + 0.5 * x) * torch.sign(rnd(EW, seed + 2))
    return {"x": x.to(BF), "dy": bq(EW, seed + 1)}


for _name, _act in (("sigmoid", ACT_SIGMOID), ("swish", ACT_SWISH)):
    case("elementwise", f"act_fwd_{_name}", "act_fwd", make_act, lambda i, act: {"y": act_value(i["x"], act)}, act=_act, one="x",
         away_from_zero=_act == ACT_SIGMOID)
    case("elementwise", f"act_bwd_{_name}", "act_bwd", make_act, lambda i, act: {"dx": i["dy"] * act_deriv(i["x"], act)}, act=_act,
         away_from_zero=_act == ACT_SIGMOID)
case("elementwise_exact", "act_fwd_relu", "act_fwd", make_act, lambda i, act: {"y": act_value(i["x"], act)}, act=ACT_RELU)
case("elementwise_exact", "act_bwd_relu", "act_bwd", make_act, lambda i, act: {"dx": i["dy"] * act_deriv(i["x"], act)}, act=ACT_RELU)


# ---- dense GEMM forward and data gradient -------------------------------------------------------------------------------------
def make_gemm(M, N, Kd, bias=False, epi=False, aux=False, wscale=1.0, bscale=1.0, **_):
    i = {"x": bq((M, Kd), 1), "w": bq((Kd, N), 2, wscale * Kd ** -0.5)}
    if bias:
        i["bias"] = par((N,), 3, bscale)
    if epi:
        i["cs"] = par((N,), 5, 0.5, 1.0)
        i["rs"] = torch.tensor([0.0, 1.25, 1.25, 0.7], dtype=F32)
        i["res"] = bq((M, N), 4)
    if aux:
        i["aux"] = bq((M, N), 6)
    return i


def gelu_poly(x):
    """gelu_poly of iseg_amd/csrc/common.h restated: Phi(x) ~ 1/2 + w q(w^2), w = clamp(x, -3.75, 3.75) / 7.5"""
    w = (x / 7.5 + 0.5).clamp(0.0, 1.0) - 0.5
    t = w * w
    q = 6617.0283203125 * t - 7851.36572265625
    for c in (3995.16552734375, -1156.386962890625, 214.41412353515625, -27.49638557434082, 2.987506628036499):
        q = q * t + c
    return x * (w * q + 0.5)


def gelu_poly_grad(x):
    """gelu_poly_grad of iseg_amd/csrc/common.h restated: gelu'(x) ~ 1/2 + w r(w^2), w = clamp(x, -4, 4) / 8"""
    w = (x * 0.125 + 0.5).clamp(0.0, 1.0) - 0.5
    t = w * w
    r = -375307.59375 * t + 481274.125
    for c in (-262435.875, 79767.0, -14897.58984375, 1771.6455078125, -132.86141967773438, 6.365922927856445):
        r = r * t + c
    return w * r + 0.5


def gelu_sig_both(x):
    """gelu_sig_both of iseg_amd/csrc/common.h restated: s = sigmoid(x (a0 + a1 x^2)); gelu ~ x s, gelu' ~ s + x s (1 - s)(a0 + 3 a1 x^2)"""
    a0, a1 = 1.600313485784997, 0.06940208738399849
    x2 = x * x
    s = 1.0 / (1.0 + torch.exp(-x * (a0 + a1 * x2)))
    y = x * s
    return y, s + y * (a0 + 3 * a1 * x2) * (1 - s)


def gemm_compute(i, act=0, pre_out=False, pre_deriv=False, rpg=0, **_):
    """the epilogue in the order of epi_apply (iseg_amd/csrc/gemm_impl.h): bias, pre_out, activation, colscale, rowscale, residual"""
    v = mm(i["x"], i["w"])
    out = {}
    if "bias" in i:
        v = v + i["bias"]
    if pre_out and not pre_deriv:
        out["pre"] = v
    if act == ACT_RELU:
        v = torch.relu(v)
    elif act == ACT_GELU and pre_deriv:
        v, out["pre"] = gelu_sig_both(v)      # iseg_amd/csrc/common.h:288 (sigmoid form where the epilogue needs gelu and gelu' of one value)
    elif act == ACT_GELU:
        v = gelu_poly(v)                      # iseg_amd/csrc/common.h:313 (transcendental-free GELU of the bf16 kernels); iseg_amd/csrc/gemm_impl.h:83
    elif act == ACT_GELU_GRAD:
        v = v * gelu_poly_grad(i["aux"])      # iseg_amd/csrc/common.h:313; iseg_amd/csrc/gemm_impl.h:83
    elif act == ACT_RELU_GRAD:
        v = torch.where(i["aux"] > 0, v, torch.zeros_like(v))
    elif act == ACT_MUL_AUX:
        v = v * i["aux"]
    if "cs" in i:
        v = v * i["cs"] * i["rs"].repeat_interleave(rpg)[:, None]
    if "res" in i:
        v = v + i["res"]
    out["y"] = v
    return out


# dense_fwd (the Keras kernel as stored) plans onto the register-staged main loop, dense_fwd_t / dense_dgrad (both operands K-contiguous) onto the
# LDS-DMA pipeline; the device test checks both with the planner's own answer (iseg_gemm_variant / iseg_gemm_splits)
case("gemm_fwd", "nn_bias_k384", "dense_fwd", make_gemm, gemm_compute, M=512, N=96, Kd=384, bias=True)
case("gemm_fwd", "nn_relu_pre_out_k96", "dense_fwd", make_gemm, gemm_compute, M=512, N=96, Kd=96, bias=True, act=ACT_RELU, pre_out=True)
case("gemm_fwd", "nn_scales_residual", "dense_fwd", make_gemm, gemm_compute, M=512, N=96, Kd=384, bias=True, epi=True, rpg=128)
case("gemm_fwd", "nn_split_k3072", "dense_fwd", make_gemm, gemm_compute, M=512, N=96, Kd=3072, split=True)
case("gemm_fwd", "nn_concat_slice", "dense_fwd", make_gemm, gemm_compute, M=512, N=96, Kd=384, concat=(320, 128))
case("gemm_fwd", "nt_bias_k384", "dense_fwd_t", make_gemm, gemm_compute, M=512, N=384, Kd=384, bias=True)
case("gemm_fwd", "nt_tail_k112_relu_pre_out", "dense_fwd_t", make_gemm, gemm_compute, M=512, N=96, Kd=112, bias=True, act=ACT_RELU, pre_out=True)
case("gemm_fwd", "nt_scales_residual", "dense_fwd_t", make_gemm, gemm_compute, M=512, N=96, Kd=384, bias=True, epi=True, rpg=128)
case("gemm_fwd", "nt_split_k3072", "dense_fwd_t", make_gemm, gemm_compute, M=512, N=96, Kd=3072, split=True)
# dX [M, N] = dY [M, Kd] @ W^T: in the terms of make_gemm x = dY, w = W^T (the runner hands the kernel W = w^T as stored)
case("gemm_dgrad", "plain", "dense_dgrad", make_gemm, gemm_compute, M=2048, N=96, Kd=384)
case("gemm_dgrad", "relu_grad", "dense_dgrad", make_gemm, gemm_compute, M=512, N=384, Kd=96, act=ACT_RELU_GRAD, aux=True)
case("gemm_dgrad", "mul_aux", "dense_dgrad", make_gemm, gemm_compute, M=512, N=384, Kd=96, act=ACT_MUL_AUX, aux=True)
# tier 2: the polynomial / sigmoid-form GELU of the bf16 epilogues
case("gelu_approx", "nn_gelu_pre_out", "dense_fwd", make_gemm, gemm_compute, 2, M=512, N=96, Kd=384, bias=True, act=ACT_GELU, pre_out=True)
case("gelu_approx", "nt_gelu", "dense_fwd_t", make_gemm, gemm_compute, 2, M=512, N=384, Kd=96, bias=True, act=ACT_GELU)
case("gelu_approx", "nt_gelu_pre_deriv", "dense_fwd_t", make_gemm, gemm_compute, 2, M=512, N=384, Kd=96, bias=True, act=ACT_GELU, pre_out=True,
     pre_deriv=True, wscale=0.4, bscale=0.2)
# (pre-activations of N(0, 0.45): gelu' is flat at its extrema, x = +-1.41, and saturates at 1 from x = 2.5 on; there every value rounds the same
# way, which a Gaussian of unit width shows as -0.01 ulp of bias in the fp32 restatement itself)
case("gelu_approx", "dgrad_gelu_grad", "dense_dgrad", make_gemm, gemm_compute, 2, M=512, N=384, Kd=96, act=ACT_GELU_GRAD, aux=True)
case("gelu_approx_act", "act_fwd_gelu", "act_fwd", make_act, lambda i, act: {"y": gelu_poly(i["x"])}, 2, act=ACT_GELU, one="x")      # iseg_amd/csrc/elementwise.hip:332
case("gelu_approx_act", "act_bwd_gelu", "act_bwd", make_act, lambda i, act: {"dx": i["dy"] * gelu_poly_grad(i["x"])}, 2, act=ACT_GELU)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
def row_stats(x, eps):
    """the saved statistics of a LayerNorm forward, as fp32 (what the backward kernels are handed)"""
    x = x.to(F64)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean.to(F32), torch.rsqrt(var + eps).to(F32)


def gather_tables(rows, pad_every):
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(11))
    fwd = []                                  # output row -> source row, with padding rows (-1) sprinkled in
    for n, src in enumerate(perm.tolist()):
        if n % pad_every == 0:
            fwd.append(-1)
        fwd.append(src)
    fwd = torch.tensor(fwd, dtype=torch.int32)
    inv = torch.empty(rows, dtype=torch.int32)
    inv[fwd[fwd >= 0].long()] = torch.nonzero(fwd >= 0).flatten().int()
    return fwd, inv


def make_ln(rows, C, eps, post=False, gather=False, **_):
    x = bq((rows, C), 1, 2.0, 0.3)
    i = {"x": x, "gamma": par((C,), 2, 0.3, 1.0), "beta": par((C,), 3, 0.2), "add": bq((rows, C), 5)}
    mean, rstd = row_stats(x, eps)
    if post:
        i["cs"] = par((C,), 6, 0.4, 1.0)
        i["rs"] = torch.tensor([0.0, 1.25, 1.25, 2.5], dtype=F32)
        i["res"] = bq((rows, C), 7)
    if gather:
        i["fwd"], i["inv"] = gather_tables(rows, 7)
        i["dy"] = bq((i["fwd"].numel(), C), 4)
        src = i["fwd"].clamp(min=0).long()
        mean, rstd = mean[src], rstd[src]      # per OUTPUT row
    else:
        i["dy"] = bq((rows, C), 4)
    i["mean"], i["rstd"] = mean, rstd
    return i


def ln_dx(g, x, mean, rstd):
    """dx of y = xhat * gamma (+ beta) for g = dy * gamma, from the saved statistics"""
    xhat = (x - mean[:, None]) * rstd[:, None]
    return rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def ln_compute(i, rows, C, eps, post=False, gather=False, **_):
    y = O.layer_norm(i["x"], i["gamma"], i["beta"], eps)
    if post:
        scale = i["cs"][None, :] * i["rs"].repeat_interleave(rows // 4)[:, None]
        return {"y": i["res"] + y * scale, "dx": ln_dx(i["dy"] * scale * i["gamma"], i["x"], i["mean"], i["rstd"])}
    if gather:
        pad = (i["fwd"] < 0)[:, None]
        yg = torch.where(pad, torch.zeros_like(y[:1]), y[i["fwd"].clamp(min=0).long()])
        inv = i["inv"].long()
        return {"y": yg, "dx": ln_dx(i["dy"][inv] * i["gamma"], i["x"], i["mean"][inv], i["rstd"][inv]) + i["add"]}
    return {"y": y, "dx": ln_dx(i["dy"] * i["gamma"], i["x"], i["mean"], i["rstd"]) + i["add"]}


case("layernorm", "plain_c96", "layernorm", make_ln, ln_compute, rows=4096, C=96, eps=1e-6)
case("layernorm", "plain_c384", "layernorm", make_ln, ln_compute, rows=1024, C=384, eps=1e-6)
case("layernorm", "post_norm_tail", "layernorm_post", make_ln, ln_compute, rows=4096, C=96, eps=1e-6, post=True)
case("layernorm", "row_tables", "layernorm_gather", make_ln, ln_compute, rows=4095, C=96, eps=1e-5, gather=True)


# ---- BatchNorm apply, GroupNorm / RMSNorm / GRN forward ------------------------------------------------------------------------------
def make_bn(rows, C, eps, relu):
    x = bq((rows, C), 1, 1.5, 0.2)
    dy = bq((rows, C), 4)
    gamma, beta = par((C,), 2, 0.3, 1.0), par((C,), 3, 0.2)
    x64 = x.to(F64)
    mean = x64.mean(0)
    rstd = torch.rsqrt((x64 * x64).mean(0) - mean * mean + eps)
    mean, rstd = mean.to(F32), rstd.to(F32)
    y64 = (x64 - mean.to(F64)) * rstd.to(F64) * gamma.to(F64) + beta.to(F64)
    y = ideal_bf16(torch.relu(y64) if relu else y64)      # the forward output the backward kernel reads its ReLU mask from
    dm = dy.to(F64) * (y.to(F64) > 0) if relu else dy.to(F64)
    xhat = (x64 - mean.to(F64)) * rstd.to(F64)
    sums = torch.cat([dm.sum(0), (dm * xhat).sum(0)]).to(F32)      # (dbeta, dgamma): what bn_bwd_reduce hands to bn_bwd_apply
    return {"x": x, "dy": dy, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "yfwd": y, "sums": sums}


def bn_compute(i, rows, C, eps, relu):
    xhat = (i["x"] - i["mean"]) * i["rstd"]
    y = xhat * i["gamma"] + i["beta"]
    dm = i["dy"] * (i["yfwd"] > 0) if relu else i["dy"]
    inv_n = 1.0 / rows
    dx = i["gamma"] * i["rstd"] * (dm - i["sums"][:C] * inv_n - xhat * i["sums"][C:] * inv_n)      # bn_bwd_apply_kernel, iseg_amd/csrc/norm.hip
    return {"y": torch.relu(y) if relu else y, "dx": dx}


case("batchnorm", "apply", "batchnorm", make_bn, bn_compute, rows=4096, C=96, eps=1e-3, relu=False)
case("batchnorm", "apply_relu", "batchnorm", make_bn, bn_compute, rows=4096, C=96, eps=1e-3, relu=True)

NORM_SHAPE = (8, 16, 16, 96)
case("norms", "groupnorm_fwd", "groupnorm", lambda groups: {"x": bq(NORM_SHAPE, 1, 1.5, 0.2), "gamma": par((96,), 2, 0.3, 1.0), "beta": par((96,), 3, 0.2)},
     lambda i, groups: {"y": O.group_norm(i["x"], i["gamma"], i["beta"], groups, 1e-3)}, groups=4)
case("norms", "rmsnorm_fwd", "rmsnorm", lambda: {"x": bq(EW, 1, 1.5, 0.2), "scale": par((96,), 2, 0.3)},
     lambda i: {"y": O.rms_norm(i["x"], i["scale"], 1e-6)})
case("norms", "grn_fwd", "grn", lambda: {"x": bq(NORM_SHAPE, 1), "gamma": par((96,), 2, 0.3), "beta": par((96,), 3, 0.2)},
     lambda i: {"y": O.grn(i["x"], i["gamma"], i["beta"], 1e-6)})


# ---- depthwise convolutions on the vector pipe (iseg_amd/csrc/dwconv.hip) -------------------------------------------------------------------
def make_dw(shape, K, stride):
    N, H, W, C = shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    return {"x": bq(shape, 1), "w": par((K, K, C, 1), 2, 1.0 / K), "bias": par((C,), 3, 0.1), "dy": bq((N, Ho, Wo, C), 4), "res": bq(shape, 5)}


def dw_taps_fp32(x, w, K, flip):
    """stride-1 depthwise convolution as the plain chain it is: one fp32 multiply-add per tap, tap after tap (torch's own fp32 convolution
    blocks its sums and is an order of magnitude closer to fp64 than any such chain, which would leave condition 2 nothing to multiply)"""
    N, H, W, C = x.shape
    pad = (K - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    acc = torch.zeros_like(x)
    for ky in range(K):
        for kx in range(K):
            tap = w[K - 1 - ky, K - 1 - kx, :, 0] if flip else w[ky, kx, :, 0]
            acc = acc + xp[:, ky:ky + H, kx:kx + W, :] * tap
    return acc


def dw_compute(i, shape, K, stride):
    if stride == 1 and i["x"].dtype == F32:
        return {"y": dw_taps_fp32(i["x"], i["w"], K, False) + i["bias"], "dx": dw_taps_fp32(i["dy"], i["w"], K, True) + i["res"]}
    x = i["x"].clone().requires_grad_(True)
    y = O.depthwise_conv2d(x, i["w"], i["bias"], stride, 1)
    dx, = torch.autograd.grad(y, x, i["dy"])
    return {"y": y, "dx": dx + i["res"] if stride == 1 else dx}


# 8 x 16 x 16 x 96 (24 tiles) is far below the plane size from which the 7 x 7 goes to the matrix cores (iseg_amd/csrc/dwconv_mfma.hip: 2048 tiles)
case("dwconv", "7x7", "dwconv", make_dw, dw_compute, shape=(8, 16, 16, 96), K=7, stride=1)
case("dwconv", "3x3_stride2", "dwconv_strided", make_dw, dw_compute, shape=(2, 32, 32, 96), K=3, stride=2)


# ---- implicit-GEMM and patchify convolutions ---------------------------------------------------------------------------------------
def make_conv(shape, K, stride, dil, Cout, **_):
    N, H, W, C = shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    return {"x": bq(shape, 1), "w": bq((K, K, C, Cout), 2, (K * K * C) ** -0.5), "bias": par((Cout,), 3, 0.3), "dy": bq((N, Ho, Wo, Cout), 4)}


def conv_compute(i, shape, K, stride, dil, Cout, **_):
    x = i["x"].clone().requires_grad_(True)
    y = O.conv2d(x, i["w"], i["bias"], stride, dil)
    dx, = torch.autograd.grad(y, x, i["dy"])
    return {"y": y, "dx": dx}


case("conv", "igemm_3x3_dilated", "conv_igemm", make_conv, conv_compute, shape=(2, 16, 16, 128), K=3, stride=1, dil=3, Cout=96, kt=True)      # (Cin % 64 == 0: the forward pass also has its LDS-DMA form)
case("conv", "igemm_3x3_stride2", "conv_igemm", make_conv, conv_compute, shape=(2, 32, 32, 96), K=3, stride=2, dil=1, Cout=96, kt=False)
case("conv", "patchify_2x2", "conv_patch", make_conv, conv_compute, shape=(2, 32, 32, 96), K=2, stride=2, dil=1, Cout=192)


# several convolutions of one input in one launch; their data gradients are one product over (branch, tap, channel): summed in fp32 in the
# accumulators and rounded once (iseg_amd/functional.py, conv_branches), so the reference is the plain sum of the branch gradients
BRANCH_TAPS = ((1, 1), (3, 2), (3, 5))


def make_branches(shape, Cout):
    N, H, W, C = shape
    i = {"x": bq(shape, 1)}
    for b, (kk, _) in enumerate(BRANCH_TAPS):
        i[f"w{b}"] = bq((kk, kk, C, Cout), 10 + b, (kk * kk * C) ** -0.5)
        i[f"dy{b}"] = bq((N, H, W, Cout), 20 + b)
    return i


def branches_compute(i, shape, Cout):
    x = i["x"].clone().requires_grad_(True)
    ys = [O.conv2d(x, i[f"w{b}"], None, 1, d) for b, (_, d) in enumerate(BRANCH_TAPS)]
    dx, = torch.autograd.grad(ys, x, [i[f"dy{b}"] for b in range(len(BRANCH_TAPS))])
    return dict({f"y{b}": y for b, y in enumerate(ys)}, dx=dx)


case("conv", "branches", "conv_branches", make_branches, branches_compute, shape=(2, 16, 16, 128), Cout=128)      # (Cin and Cout multiples of 64)


# ---- tier 2: the depthwise 7 x 7 on the matrix cores ------------------------------------------------------------------------------------
def dw_mfma_compute(i, shape, K, stride):
    i = dict(i, w=rb(i["w"]))      # iseg_amd/csrc/dwconv_mfma.hip:24 (weights are rounded to bf16; products and sums are fp32 in the matrix pipe)
    return dw_compute(i, shape, K, stride)


case("dwconv_mfma", "7x7", "dwconv_mfma", make_dw, dw_mfma_compute, 2, shape=(8, 16, 16, 96), K=7, stride=1)


# ---- tier 2: the fused ConvNeXt MLP (iseg_amd/csrc/mlp_fused.hip), forward and data-gradient chain ------------------------------------------------------
def make_mlp(M, C, b1_shift=0.0, y_scale=1.0, **_):
    """the fp32 master kernels hold bf16 values (the prep kernel rounds them itself), gamma too, so that W2 * gamma is exact in fp32 and its
    bf16 image is rounded once"""
    return {"y2": bq((M, C), 1, y_scale), "res": bq((M, C), 2), "dbr": bq((M, C), 3), "W1": bq((C, 4 * C), 4, C ** -0.5).to(F32),
            "W2": bq((4 * C, C), 5, (4 * C) ** -0.5).to(F32), "b1": par((4 * C,), 6, 0.2, b1_shift), "b2": par((C,), 7, 0.2),
            "gamma": bq((C,), 8, 0.3, 1.0).to(F32), "rs": torch.tensor([0.5, 0.75, 1.0, 1.25], dtype=F32)}


def mlp_fwd_compute(i, M, C):
    h = mm(i["y2"], i["W1"]) + i["b1"]
    G = rb(gelu_poly(h))                              # iseg_amd/csrc/mlp_fused.hip:11 (G^T = gelu(H^T + b1) in registers, rounded to bf16); the polynomial: iseg_amd/csrc/common.h:313
    z = (mm(G, i["W2"]) + i["b2"]) * i["gamma"]
    return {"out": z * i["rs"].repeat_interleave(M // 4)[:, None] + i["res"]}


def mlp_bwd_data_compute(i, M, C):
    h = mm(i["y2"], i["W1"]) + i["b1"]
    dG = mm(i["dbr"], rb(i["W2"] * i["gamma"]).t())   # iseg_amd/csrc/mlp_fused.hip:27
    dH = rb(dG * gelu_poly_grad(h))                   # iseg_amd/csrc/mlp_fused.hip:251; the chain alone takes the polynomial derivative, iseg_amd/csrc/common.h:313
    return {"dy2": mm(dH, i["W1"].t())}


def mlp_compute(i, M, C, with_g=False):
    h = mm(i["y2"], i["W1"]) + i["b1"]
    W2e = rb(i["W2"] * i["gamma"])                    # iseg_amd/csrc/mlp_fused.hip:27 (image A3: W2[hid][c] * gamma[c], bf16)
    dG = mm(i["dbr"], W2e.t())
    g, gd = gelu_sig_both(h)                          # iseg_amd/csrc/common.h:288 (the kernel that stores G and dH needs gelu and gelu' of one value)
    dH = dG * gd
    # iseg_amd/csrc/mlp_fused.hip:251 (dH^T in registers, rounded to bf16 = B operand of the next product); iseg_amd/csrc/mlp_fused.hip:253: the same bf16 dH leaves
    # the CU, so the reference multiplies the dH that was stored (Case.fed)
    dy2 = mm(i["dh_stored"] if "dh_stored" in i else rb(dH), i["W1"].t())
    return dict({"g": g} if with_g else {}, dh=dH, dy2=dy2)


# (iseg_convnext_mlp_bwd_data keeps its dH, formed with gelu_poly_grad, on the CU: nothing to hand to the reference, so its dy2 is left to the
# parity tests of tests/test_mlp_fused_gpu.py)
case("mlp_fused", "chain_c96", "mlp_fused_chain", make_mlp, mlp_compute, 2, M=2048, C=96, feed={"dh_stored": "dh"})
# the chain kernel also stores G = gelu(h).  gelu has a flat minimum at x = -0.75: a cluster of outputs sits at one place between two bf16 values
# and rounds one way (-0.0036 ulp of bias in the restatement with pre-activations of N(0, 1)), so this case draws them as N(1.5, 0.5)
case("mlp_fused", "chain_stored_g", "mlp_fused_chain", make_mlp, mlp_compute, 2, M=2048, C=96, feed={"dh_stored": "dh"}, b1_shift=1.5, y_scale=0.5,
     with_g=True)
# forward and data-gradient-only kernels: G / dH stay on the CU (UNSTORED_MAX_E)
case("mlp_fused_fwd", "c96", "mlp_fused_fwd", make_mlp, mlp_fwd_compute, 2, M=4096, C=96)
case("mlp_fused_bwd_data", "c96", "mlp_fused_bwd_data", make_mlp, mlp_bwd_data_compute, 2, M=4096, C=96)


# ---- tier 2: the GLU gate with GELU (iseg_amd/csrc/eva.hip:65: the polynomial forms of common.h in bf16) ---------------------------------------------------
def glu_compute(i):
    a, da = gelu_sig_both(i["g"])                     # iseg_amd/csrc/eva.hip:65; iseg_amd/csrc/common.h:288
    return {"out": i["x"] * a, "dg": i["dout"] * i["x"] * da, "dx": i["dout"] * a}


case("gelu_approx_act", "glu_gelu", "glu", lambda: {"g": bq(EW, 1), "x": bq(EW, 2), "dout": bq(EW, 3)}, glu_compute, 2)


# ---- softmax cross-entropy behind a x2 bilinear upsampling: the gradient on the low-resolution bf16 logits (iseg_amd/csrc/loss.hip) -----------------------
UP_IGNORE = 255


def make_upsample_ce(shape, s):
    N, Hi, Wi, C = shape
    g = torch.Generator().manual_seed(91)
    y = torch.randint(0, C, (N, Hi * s, Wi * s), generator=g, dtype=torch.int32)
    y[torch.rand(y.shape, generator=g) < 0.1] = UP_IGNORE
    return {"z": bq(shape, 1, 3.0), "y": y}


def upsample_ce_compute(i, shape, s):
    """d(sum of the pixel losses / pixels)/dz: 1 / pixels is a power of two, so the scale costs no rounding"""
    N, Hi, Wi, C = shape
    z = i["z"].clone().requires_grad_(True)
    up = O.resize_bilinear(z, (Hi * s, Wi * s))
    if z.dtype == F64:
        loss = O.softmax_ce_ignore(i["y"], up, C, UP_IGNORE, None).sum()
    else:
        y = i["y"].reshape(-1).long()
        loss = (-torch.log_softmax(up.reshape(-1, C), -1)[torch.arange(len(y)), y.clamp(0, C - 1)] * (y != UP_IGNORE).to(z.dtype)).sum()
    dz, = torch.autograd.grad(loss / (N * Hi * Wi * s * s), z)
    return {"dz": dz}


case("upsample_ce", "x2_dlogits", "upsample_ce", make_upsample_ce, upsample_ce_compute, shape=(16, 32, 32, 21), s=2)


# ---- tier 2: attention cores.  The probabilities (and dS) are bf16 MFMA operands that stay in registers / LDS: UNSTORED_MAX_E ------------------------
ATT_KEY_TILE = 64      # iseg_amd/csrc/attn_tile.h:9 (attn_fwd_tile: 64 queries, key tiles of 64, the online-softmax recurrence), AK at :30
LN2 = math.log(2.0)


def _heads(t, B, T, heads):
    return t.reshape(B, T, heads, -1).permute(0, 2, 1, 3)


def _unheads(t):
    B, h, T, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, h * d)


def flash_fwd(qkv, B, T, heads, scale):
    """the recurrence of flash_attn_fwd_kernel: per key tile the running row maximum m, p = exp(scale (s - m)), the row sum l of the UNROUNDED
    p, the accumulator rescaled by exp(scale (m_old - m)); out = o / l"""
    C = qkv.shape[-1] // 3
    return _unheads(online_softmax_pv(*[_heads(qkv[..., n * C:(n + 1) * C], B, T, heads) for n in range(3)], scale))


def online_softmax_pv(q, k, v, scale):
    T = q.shape[-2]
    s = q @ k.transpose(-1, -2)
    m = torch.full_like(s[..., :1], -float("inf"))
    l = torch.zeros_like(m)
    o = torch.zeros_like(v)
    for k0 in range(0, T, ATT_KEY_TILE):
        st = s[..., k0:k0 + ATT_KEY_TILE]
        mnew = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.exp((m - mnew) * scale)
        p = torch.exp((st - mnew) * scale)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + rb(p) @ v[..., k0:k0 + ATT_KEY_TILE, :]      # iseg_amd/csrc/attn_tile.h:11-13 (the probabilities are the bf16 B operand of O^T = V^T P^T on v_mfma_f32_16x16x32_bf16)
        m = mnew
    return o / l


def make_flash(B, T, heads, scale):
    """qkv, dout; for the backward kernels also what the training forward hands them: its bf16 output and L = log2 sum_j exp2(c s_ij) per row
    (fp32, rows padded to a multiple of 64: iseg_attention_lse_elems)"""
    qkv = bq((B, T, 3 * heads * 64), 1)
    q64 = qkv.to(F64)
    C = heads * 64
    q, k = _heads(q64[..., :C], B, T, heads), _heads(q64[..., C:2 * C], B, T, heads)
    L = torch.logsumexp(q @ k.transpose(-1, -2) * scale, -1) / LN2
    Tp = -(-T // 64) * 64
    lse = torch.zeros((B * heads, Tp), dtype=F32)
    lse[:, :T] = L.reshape(B * heads, T).to(F32)
    return {"qkv": qkv, "dout": bq((B, T, C), 2), "out_fwd": ideal_bf16(flash_fwd(q64, B, T, heads, scale)), "lse": lse}


def flash_bwd_compute(i, B, T, heads, scale):
    """flash_attn_dq_kernel / flash_attn_dkdv_kernel: p = exp2(c s - L) from the saved L (no running maximum), D = sum_d dO O,
    dS = p (dP - D) scale; P and dS are rounded to bf16 as the operands of dV = P^T dO, dK = dS^T Q, dQ = dS K"""
    C = heads * 64
    q, k, v = [_heads(i["qkv"][..., n * C:(n + 1) * C], B, T, heads) for n in range(3)]
    do, o = _heads(i["dout"], B, T, heads), _heads(i["out_fwd"], B, T, heads)
    dq, dk, dv = recomputed_p_bwd(q, k, v, do, o, i["lse"].reshape(B, heads, -1)[..., :T, None], scale)
    return {"dq": _unheads(dq), "dk": _unheads(dk), "dv": _unheads(dv)}


def recomputed_p_bwd(q, k, v, do, o, L, scale):
    p = torch.exp(q @ k.transpose(-1, -2) * scale - L * LN2)
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)) * scale
    pb, dsb = rb(p), rb(ds)                            # iseg_amd/csrc/attn_tile.h:16-17 (P and dS are the B operands of dV^T = dO^T P and dK^T = Q^T dS); iseg_amd/csrc/flashattn.hip:9-10 (dS of dQ)
    return dsb @ k, dsb.transpose(-1, -2) @ q, pb.transpose(-1, -2) @ do


FLASH = dict(B=2, T=150, heads=3, scale=0.125)      # three key tiles, the last one ragged
case("attention_flash", "t150_h3", "attention_flash", make_flash, lambda i, B, T, heads, scale: {"out": flash_fwd(i["qkv"], B, T, heads, scale)},
     2, **FLASH)
case("attention_flash_bwd", "t150_h3", "attention_flash_bwd", make_flash, flash_bwd_compute, 2, **FLASH)


# the single-head core of the non-local block (iseg_amd/csrc/selfattn.hip:4-6: the tile bodies of attn_tile.h over value slabs, so P stays in registers
# as the B operand of O^T = V^T P^T, iseg_amd/csrc/attn_tile.h:11-13; iseg_amd/csrc/selfattn.hip:8-10 for the backward pass), 64-wide q / k and a wide value
def make_self(B, T, dv, scale):
    q, k, v = bq((B, T, 64), 1), bq((B, T, 64), 2), bq((B, T, dv), 3)
    q64, k64 = q.to(F64), k.to(F64)
    Tp = -(-T // 64) * 64
    lse = torch.zeros((B, Tp), dtype=F32)
    lse[:, :T] = (torch.logsumexp(q64 @ k64.transpose(-1, -2) * scale, -1) / LN2).to(F32)
    return {"q": q, "k": k, "v": v, "dout": bq((B, T, dv), 4), "out_fwd": ideal_bf16(online_softmax_pv(q64, k64, v.to(F64), scale)), "lse": lse}


def self_bwd_compute(i, B, T, dv, scale):
    dq, dk, dvv = recomputed_p_bwd(i["q"], i["k"], i["v"], i["dout"], i["out_fwd"], i["lse"][:, :T, None], scale)
    return {"dq": dq, "dk": dk, "dv": dvv}


SELF = dict(B=6, T=150, dv=192, scale=0.125)
case("attention_self", "t150_dv192", "attention_self", make_self,
     lambda i, B, T, dv, scale: {"out": online_softmax_pv(i["q"], i["k"], i["v"], scale)}, 2, **SELF)
case("attention_self_bwd", "t150_dv192", "attention_self_bwd", make_self, self_bwd_compute, 2, **SELF)


def window_compute(i, B, T, heads, scale):
    """win_attn_fwd_kernel / win_attn_bwd_kernel (iseg_amd/csrc/winattn.hip:2-8): P = softmax(scale Q K^T + bias) normalised in fp32, rounded to bf16 as the
    operand of P V and of dV = P^T dO; dS = P (dP - rowsum(dP P)) from the fp32 P; scale dS rounded to bf16 as the operand of dQ and dK"""
    C = heads * 32
    q, k, v = [_heads(i["qkv"][..., n * C:(n + 1) * C], B, T, heads) for n in range(3)]
    do = _heads(i["dout"], B, T, heads)
    p = torch.softmax(q @ k.transpose(-1, -2) * scale + i["bias"][None], -1)
    pb = rb(p)                                         # iseg_amd/csrc/winattn.hip:5 (P goes through a wave-private LDS image to become the A operand of P V)
    dp = do @ v.transpose(-1, -2)
    dsb = rb(p * (dp - (dp * p).sum(-1, keepdim=True)) * scale)      # iseg_amd/csrc/winattn.hip:298 (scale * dS (bf16) replaces P)
    return {"out": _unheads(pb @ v), "dq": _unheads(dsb @ k), "dk": _unheads(dsb.transpose(-1, -2) @ q), "dv": _unheads(pb.transpose(-1, -2) @ do)}


case("attention_window", "w32_t49_h3", "attention_window",
     lambda B, T, heads, **_: {"qkv": bq((B, T, 3 * heads * 32), 1), "dout": bq((B, T, heads * 32), 2), "bias": par((heads, T, T), 3, 0.5)},
     window_compute, 2, B=32, T=49, heads=3, scale=32 ** -0.5)


# ---- bilinear resize ------------------------------------------------------------------------------------------------------------------
def make_resize(shape, out):
    N, Hi, Wi, C = shape
    return {"x": bq(shape, 1), "dy": bq((N, out[0], out[1], C), 2)}


def resize_compute(i, shape, out):
    x = i["x"].clone().requires_grad_(True)
    y = O.resize_bilinear(x, out)
    dx, = torch.autograd.grad(y, x, i["dy"])
    return {"y": y, "dx": dx}


case("resize", "up_12_to_20", "resize", make_resize, resize_compute, shape=(2, 12, 12, 160), out=(20, 20))
case("resize_x2", "exact_x2", "resize", make_resize, resize_compute, shape=(2, 16, 16, 96), out=(32, 32))


# ---- the sampling kernels: DCNv3, DCNv2's sampling half, deformable attention ---------------------------------------------------------
# The operands are the `budget` cases of tests/sampling_kinks.py (the recipes of the core tests at 2 x 40 x 36 x 32), the formula is the oracle itself
# (oracle/tf_ops.dcnv3_op, oracle/tf_ops.dcnv2 with identity products, tests/deformable_mhsa_ref.core): fp64 is the reference, torch.float32 the
# restatement.  Only bf16-STORED outputs are cases: the fp32 input gradients of iseg_dcnv3_bwd / iseg_dcnv2_sample_bwd keep their parity tolerance.
def _kink_case(op):
    return next(c for c in SK.CASES if c.op == op and c.kind == "budget")


def make_sampling(op):
    return dict(SK.operands(_kink_case(op), BF))


def sampling_compute(i, op, keep):
    out = SK.OPS[op].run(i, _kink_case(op).p, dtype=i["offset"].dtype)
    if op == "dcnv2":      # the kernel writes ONE [N, H, W, 27] gradient: 18 offsets, 9 modulation logits
        out["doff"] = torch.cat([out["doffset"], out["dlogit"]], dim=-1)
    return {k: out[k] for k in keep}


def sampling_interior(op):
    """-> {name of the offset gradient: its interior elements} (DCNv2: and every logit element)"""
    cls = SK.classes(_kink_case(op), BF)
    if op == "dcnv2":
        return {"doff": torch.cat([cls.interior, torch.ones(cls.interior.shape[:3] + (9,), dtype=torch.bool)], dim=-1)}
    return {"doffset": cls.interior}


for _op, _fwd, _bwd in (("dcnv3", ("y",), ("dmask", "doffset")), ("dcnv2", ("col",), ("doff",)), ("defattn", ("out",), ("dvalue", "dattn", "doffset"))):
    _fam = "dcnv2_sample" if _op == "dcnv2" else _op
    case(_fam, "40x36", _fam, make_sampling, sampling_compute, op=_op, keep=_fwd)
    case(_fam + "_bwd", "40x36", _fam + "_bwd", make_sampling, sampling_compute, op=_op, keep=_bwd, select=functools.partial(sampling_interior, _op))
del _op, _fwd, _bwd, _fam


FAMILIES = sorted({c.family for c in CASES})
assert set(FAMILIES) == set(BUDGET), (FAMILIES, sorted(BUDGET))


def family_cases(family):
    return [c for c in CASES if c.family == family]


_RESTATED, _FAMILY_MAX_E = {}, {}


def restated(c):
    """-> {output: (bf16 of the fp32 restatement, fp64 reference, fp32 restatement)}; computed once per case and shared, never modified"""
    if c.id not in _RESTATED:
        r32 = c.outputs(F32)
        ref = c.selected(c.outputs(F64, c.fed(r32)))
        r32 = c.selected(r32)
        _RESTATED[c.id] = {k: (r32[k].to(F32).to(BF), ref[k], r32[k].to(F32)) for k in ref}
    return _RESTATED[c.id]


def family_max_e(family):
    """the restatement's max |e| over every output of the family's cases: the figure condition 2 multiplies.  Per family, like BUDGET: the excess
    over 1/2 ulp is set by the handful of elements that sit next to a tie, so the maximum of ONE output is an extreme value of a few samples (0.50000
    to 0.50013 among the dense GEMM cases), while the family's is what fp32 accumulation costs at these shapes"""
    if family in UNSTORED_MAX_E:
        return UNSTORED_MAX_E[family]
    if family not in _FAMILY_MAX_E:
        _FAMILY_MAX_E[family] = measured_max_e(family)
    return _FAMILY_MAX_E[family]


def measured_max_e(family):
    if True:
        return max(rounding_stats(b16, ref).max_abs_e for c in family_cases(family) for b16, ref, _ in restated(c).values())
