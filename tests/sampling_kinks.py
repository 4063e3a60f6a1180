"""Cell borders of the three sampling kernels -- DCNv3 (dcn_tap, iseg_amd/csrc/dcnv3.hip:41), DCNv2's sampling half (dcn2_tap, :1086) and deformable
attention (da_tap, iseg_amd/csrc/defattn.hip:40) -- for tests/test_sampling_kinks_host.py (CPU) and tests/test_sampling_kinks_gpu.py (device).  Test
infrastructure only: torch on the CPU.

The gradient with respect to an offset is the one output of these operations that is NOT continuous: it jumps where a sampling coordinate crosses
an integer (the slope of the next cell takes over) and where it crosses a bound of a clipped coordinate (tf.clip_by_value passes the gradient inside
the bounds, bounds included, and nothing outside).  The kernels compute the coordinate in fp32, the references in fp64, so next to such a kink the
two may stand on different sides.  Every offset element (one tap, one axis) is therefore put into one of three classes from the fp64 coordinate of
the operands AS STORED (rounded to the storage dtype before either side sees them):

    lattice   delta == 0 exactly AND every step of the coordinate chain gives the same number in fp32 as in fp64 (Op.exact): the coordinate IS the
              kink for the kernel too, which has no excuse: it must take the reference's side and its inclusive bounds.
    border    delta < TAU, not lattice: fp32 may land on either side; the kernel must match the gradient of one side.  (This includes the few
              coordinates that are an integer in fp64 only because fp64 rounded them there, after a division by Hin = 7, say.)
    interior  everything else: the kernel must match the reference.

    delta = |coord - kink|, kink = the nearest integer (every clip bound -- 0 and H - 1 / W - 1 for deformable attention, 0 and H + 1 / W + 1 for
    DCNv2, none for DCNv3, which clips only indices -- is an integer)
    TAU   = 4 x R x 2^-23 x max(1, largest |coord| of the case), R = the fp32 roundings of the kernel's coordinate chain, counted below

One-sided references: the reference's gradients as they are and with the border elements' coordinates moved by +2 TAU and by -2 TAU.  The move is
made ONE AXIS AT A TIME (five evaluations, not three): the y gradient of a tap is linear in x inside a cell and continuous in x across a kink, so with
x left alone the moved evaluation is the exact one-sided limit in y; moving both axes of a tap at once would put an O(TAU) error of the size of the
tolerance into it.  DCNv3 / DCNv2: the move goes through the offset operand (additive; d coord / d offset is a constant).  Deformable attention: it
is added to the coordinate behind tanh, so the factor (1 - tanh^2) of the gradient is the one of the stored logit.
"""
import functools
from typing import NamedTuple

import torch

from oracle import tf_ops as O
from tests import deformable_mhsa_ref as R
from tests.test_kernels_gpu import rnd

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
ULP = 2.0 ** -23

# R, the number of fp32 roundings between the stored offset and the coordinate that floorf() / the bound comparisons see (a fused multiply-add only
# removes one).  An error of k ulp of a library function counts as 2 k roundings of half an ulp.
R_DCNV3 = 10       # dcn_tap, dcnv3.hip:41 -- :44 / Hin (1); :46 / Win (1); :48 gx * s (1), off0 * s (1), / Win (1), two additions (2); :50 - 1 (1), + 1 (1),
#                    * (Win - 2) (1); 2 * and 0.5 * are exact
R_DCNV2 = 1        # dcn2_tap, dcnv3.hip:1086 -- :1088 (float)(h + p / 3) + oy (1); the integer part is exact
TANHF_ULP = 2      # tanhf: the bound of the HIP math API's accuracy table (ROCm device library) as we recall it, 2 ulp at the most; a larger figure only
#                    moves elements from `interior` to `border`, and the 1 % cap on the border share keeps that honest
R_DEFATTN = 2 * TANHF_ULP + 3      # da_tap, defattn.hip:40 -- :41 tanhf (2 x 2); sy = H / offset_range_factor on the host (1); :42 ty * sy (1), (float)h + (1)

TOL = {      # fp32 storage, max-norm relative to the reference's largest element: the tolerances of test_dcnv3_gpu.py / test_deformable_mhsa_gpu.py
    "dcnv3": {"y": 1e-5, "dx": 2e-5, "dmask": 2e-5, "doffset": 5e-5},
    "dcnv2": {"col": 1e-5, "dx": 2e-5, "dlogit": 2e-5, "doffset": 5e-5},
    "defattn": {"out": 1e-5, "dvalue": 2e-5, "dattn": 2e-5, "doffset": 5e-5},
}
# bf16 storage.  A bf16-stored output is the fp32 value rounded once: |got - ref| <= 2^-8 |ref| (half an ulp of an 8-bit significand) + the fp32
# tolerance.  The input gradient of DCNv3 is the exception: its window route accumulates bf16 cases in 32-bit LDS cells (dcnv3.hip:894-896) and is
# held, as in test_dcnv3_gpu.py, to 2e-2 of scale.
BF16_FIXED_POINT = {("dcnv3", "dx"): 2e-2}
LIPSCHITZ = 64.0      # a continuous output moves by at most this x TAU x its scale between the one-sided evaluations (a jump would be ~ 1 / TAU times more)
MAX_BORDER_SHARE = 0.01
MIN_LATTICE = 1000
MIN_ON_BOUND = 50
MIN_NEAR = 200
SEPARATION = 100.0      # near-lattice cases: the two one-sided gradients differ by more than this x the interior tolerance on >= 90 % of the border elements


class Classes(NamedTuple):
    coord: torch.Tensor
    kink: torch.Tensor
    delta: torch.Tensor
    tau: float
    lattice: torch.Tensor
    border: torch.Tensor
    interior: torch.Tensor
    on_bound: torch.Tensor


def tau_of(rounds, coord):
    return 4.0 * rounds * ULP * max(1.0, coord.abs().max().item())


def per_axis(pair, like):
    """(value for axis 0, value for axis 1) -> tensor broadcastable against an offset-shaped tensor whose last dimension alternates the two axes"""
    return torch.tensor(pair, dtype=like.dtype).repeat(like.shape[-1] // 2)


def classify(coord, tau, hi=None, exact=None):
    """coord: fp64, in the layout of the offset operand (last dimension = taps x 2 axes).  hi: the upper clip bounds per axis, or None.  exact: where
    every step of the coordinate chain gives the same value in fp32 as in fp64.  An element whose fp64 coordinate is an integer only because fp64
    rounded it there (a division by Hin = 7, say) is not on the lattice for the kernel: it is a border element"""
    assert coord.dtype == F64
    kink = torch.round(coord)
    delta = (coord - kink).abs()
    lattice = (delta == 0) if exact is None else (delta == 0) & exact
    border = (delta < tau) & ~lattice
    on_bound = torch.zeros_like(lattice) if hi is None else lattice & ((kink == 0) | (kink == per_axis(hi, coord)))
    return Classes(coord, kink, delta, tau, lattice, border, ~(lattice | border), on_bound)


def _floor(t, mut):
    if mut == "trunc":
        return torch.trunc(t)
    if mut == "ceil_minus_1":
        return torch.ceil(t) - 1.0
    return torch.floor(t)


def _clip(t, lo, hi, mut):
    """tf.clip_by_value: the gradient passes inside [lo, hi], bounds included (torch.clamp does the same); mutant: only strictly inside"""
    c = torch.clamp(t, lo, hi)
    if mut == "strict_clip":
        return torch.where((t > lo) & (t < hi), c, c.detach())
    return c


MUTANTS = ("trunc", "ceil_minus_1", "strict_clip", "swap_corner")      # swap_corner: weights from the unclipped corner where the reference clips it / the converse


# ---------------------------------------------------------------------------------------------------------------------------
# DCNv3 (oracle/tf_ops.dcnv3_op; kernel 3 x 3, stride 1, dilation 1, padding 1: the geometry of every DCNv3 layer of the models)
# ---------------------------------------------------------------------------------------------------------------------------
def dcnv3_coordinates(off, H, W, G, s=1.0, steps=False):
    """the coordinate lines of oracle/tf_ops.dcnv3_op (:498-525) in off.dtype -> [N, H, W, G * 9 * 2]: element 2 k is px (row reference, Win),
    element 2 k + 1 is py -- the reference's [y, x] / [x, y] quirk.  steps=True: every intermediate, each broadcastable to [N, H, W, G * 9, 2]"""
    dt = off.dtype
    N = off.shape[0]
    Hin, Win = H + 2, W + 2
    ys = (torch.arange(H, dtype=dt) + 1.5) / Hin
    xs = (torch.arange(W, dtype=dt) + 1.5) / Win
    ref = torch.stack([ys.reshape(H, 1).expand(H, W), xs.reshape(1, W).expand(H, W)], dim=-1).reshape(1, H, W, 1, 2)
    lin = torch.arange(3, dtype=dt) - 1.0
    gx, gy = torch.meshgrid(lin, lin, indexing="ij")
    grid = torch.stack([gx / Win, gy / Hin], dim=-1).reshape(1, 1, 1, 9, 2).repeat(1, 1, 1, G, 1)
    norm = torch.tensor([Win, Hin], dtype=dt)
    o5 = off.reshape(N, H, W, G * 9, 2)
    loc = (ref + grid * s) + o5 * s / norm
    grids = 2 * loc - 1
    coord = 0.5 * ((grids + 1.0) * torch.tensor([Win - 2, Hin - 2], dtype=dt))
    if steps:
        return [ref, grid, grid * s, o5 * s, o5 * s / norm, ref + grid * s, loc, grids, grids + 1.0, coord]
    return coord.reshape(N, H, W, G * 18)


def dcnv3_restated(x, off, mask, G, s=1.0, mut=None, shift=None):
    """dcnv3_op from dcnv3_coordinates on, with the mutants; shift: added to the coordinates"""
    N, H, W, C = x.shape
    Cg = C // G
    Hin, Win = H + 2, W + 2
    coord = dcnv3_coordinates(off, H, W, G, s)
    if shift is not None:
        coord = coord + shift
    c = coord.reshape(N, H, W, G, 9, 2)
    px, py = c[..., 0], c[..., 1]
    fx, fy = _floor(px, mut).detach(), _floor(py, mut).detach()
    x0, x1 = fx.long().clamp(0, Win - 1), (fx.long() + 1).clamp(0, Win - 1)
    y0, y1 = fy.long().clamp(0, Hin - 1), (fy.long() + 1).clamp(0, Hin - 1)
    if mut == "swap_corner":
        dx0, dx1, dy0, dy1 = px - fx, fx + 1 - px, py - fy, fy + 1 - py
    else:
        dx0, dx1, dy0, dy1 = px - x0.to(px.dtype), x1.to(px.dtype) - px, py - y0.to(px.dtype), y1.to(px.dtype) - py
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1)).reshape(N, Hin, Win, G, Cg)
    n_i = torch.arange(N).reshape(N, 1, 1, 1, 1)
    g_i = torch.arange(G).reshape(1, 1, 1, G, 1)
    out = 0
    for yy, xx, ww in ((y0, x0, dx1 * dy1), (y1, x0, dx1 * dy0), (y0, x1, dx0 * dy1), (y1, x1, dx0 * dy0)):
        out = out + xp[n_i, yy, xx, g_i] * ww.unsqueeze(-1)
    out = (out * mask.reshape(N, H, W, G, 9, 1)).sum(dim=4)
    return out.reshape(N, H, W, C)


# ---------------------------------------------------------------------------------------------------------------------------
# DCNv2, the sampling half (oracle/tf_ops.dcnv2 with identity offset and output products)
# ---------------------------------------------------------------------------------------------------------------------------
def dcnv2_coordinates(off, H, W, steps=False):
    """off [N, H, W, >= 18] -> the unclipped padded coordinates g of oracle/tf_ops.dcnv2 (:604-608), [N, H, W, 18]: (h + ky + dy, w + kx + dx)"""
    dt = off.dtype
    N = off.shape[0]
    ys, xs = torch.arange(H, dtype=dt), torch.arange(W, dtype=dt)
    grid = torch.stack(torch.meshgrid(ys, xs, indexing="ij"), dim=-1).reshape(1, H, W, 1, 2)
    k = torch.arange(3, dtype=dt)
    patch = torch.stack(torch.meshgrid(k, k, indexing="ij"), dim=-1).reshape(9, 2)      # (1 + (ky - 1), 1 + (kx - 1)): pad + patch of :606-608
    g = grid + patch + off[..., :18].reshape(N, H, W, 9, 2)      # (grid + patch: integers, exact)
    return [g] if steps else g.reshape(N, H, W, 18)


def dcnv2_restated(x, off, mut=None, shift=None):
    """-> col [N, H, W, 9, C] (dcnv2 :609-623), with the mutants"""
    N, H, W, C = x.shape
    g = dcnv2_coordinates(off, H, W)
    if shift is not None:
        g = g + shift
    g = g.reshape(N, H, W, 9, 2)
    hi = torch.tensor([H + 1, W + 1], dtype=x.dtype)
    lo = torch.zeros(2, dtype=x.dtype)
    f = _floor(g, mut).detach()
    i1, i0 = torch.clamp(f + 1, lo, hi), torch.clamp(f, lo, hi)
    gc = _clip(g, lo, hi, mut)
    d0, d1 = (gc - f, f + 1 - gc) if mut == "swap_corner" else (gc - i0, i1 - gc)
    wts = (d0[..., 0] * d0[..., 1], d0[..., 0] * d1[..., 1], d1[..., 0] * d0[..., 1], d1[..., 0] * d1[..., 1])
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    n_i = torch.arange(N).reshape(N, 1, 1, 1)
    col = 0
    for wt, (cy, cx) in zip(wts, ((i1[..., 0], i1[..., 1]), (i1[..., 0], i0[..., 1]), (i0[..., 0], i1[..., 1]), (i0[..., 0], i0[..., 1]))):
        col = col + wt.unsqueeze(-1) * xp[n_i, cy.long(), cx.long()]
    return col * torch.sigmoid(off[..., 18:]).unsqueeze(-1)


def dcnv2_oracle_col(x, off):
    """oracle/tf_ops.dcnv2 itself as the sampling half: a 1 x 1 identity offset convolution and an identity [9 C, 9 C] kernel (exact in fp64)"""
    N, H, W, C = x.shape
    eye_o = torch.eye(27, dtype=x.dtype).reshape(1, 1, 27, 27)
    eye_k = torch.eye(9 * C, dtype=x.dtype).reshape(3, 3, C, 9 * C)
    return O.dcnv2(x, off, eye_k, None, eye_o, torch.zeros(27, dtype=x.dtype)).reshape(N, H, W, 9, C)


# ---------------------------------------------------------------------------------------------------------------------------
# deformable attention (tests/deformable_mhsa_ref.py)
# ---------------------------------------------------------------------------------------------------------------------------
def defattn_coordinates(o, H, W, heads, P, orf, steps=False):
    """the unclipped coordinates of deformable_mhsa_ref.sampling_coordinates (:27-36) in the layout of the offset logits [N, H, W, heads * P * 2]:
    (y, x) per point"""
    N = o.shape[0]
    scale = torch.tensor([H / orf, W / orf], dtype=o.dtype)
    base = torch.stack([torch.arange(H, dtype=o.dtype).reshape(H, 1).expand(H, W), torch.arange(W, dtype=o.dtype).reshape(1, W).expand(H, W)], dim=-1)
    t = torch.tanh(o.reshape(N, H, W, heads * P, 2))
    d = t * scale
    c = base.reshape(1, H, W, 1, 2) + d
    return [t, d, c] if steps else c.reshape(o.shape)


def defattn_restated(v, o, a, heads, P, orf, mut=None, shift=None):
    """deformable_mhsa_ref.core(scrub=False) with a shift added to the unclipped coordinates, and the mutants"""
    N, H, W, Cv = v.shape
    c = defattn_coordinates(o, H, W, heads, P, orf)
    if shift is not None:
        c = c + shift
    c = c.reshape(N, H, W, heads, P, 2)
    y, x = _clip(c[..., 0], 0.0, float(H - 1), mut), _clip(c[..., 1], 0.0, float(W - 1), mut)
    attn = torch.softmax(a.reshape(N, H, W, heads, P), dim=-1)
    value = v.reshape(N, H, W, heads, Cv // heads)
    if mut is None:
        sampled = R.bilinear_sample(value, y, x)
    else:
        y0, x0 = _floor(y, mut).detach(), _floor(x, mut).detach()
        y0c, y1c = y0.long().clamp(0, H - 1), (y0.long() + 1).clamp(0, H - 1)
        x0c, x1c = x0.long().clamp(0, W - 1), (x0.long() + 1).clamp(0, W - 1)
        wy1, wx1 = (y - y0c.to(y.dtype), x - x0c.to(y.dtype)) if mut == "swap_corner" else (y - y0, x - x0)
        wy0, wx0 = 1.0 - wy1, 1.0 - wx1
        n_i = torch.arange(N).reshape(N, 1, 1, 1, 1)
        h_i = torch.arange(heads).reshape(1, 1, 1, heads, 1)
        sampled = 0
        for yy, xx, ww in ((y0c, x0c, wy0 * wx0), (y0c, x1c, wy0 * wx1), (y1c, x0c, wy1 * wx0), (y1c, x1c, wy1 * wx1)):
            sampled = sampled + value[n_i, yy, xx, h_i] * ww.unsqueeze(-1)
    return (sampled * attn.unsqueeze(-1)).sum(dim=-2).reshape(N, H, W, Cv)


# ---------------------------------------------------------------------------------------------------------------------------
# the three operations behind one interface
# ---------------------------------------------------------------------------------------------------------------------------
class Op:
    """operands: dict of host tensors in the storage dtype; `offset` is the operand whose gradient has the kinks, `dout` the arriving gradient"""
    name = rounds = None

    def coords(self, ops, p, dtype=F64, steps=False):
        raise NotImplementedError

    def hi(self, ops, p):
        return None

    def exact(self, ops, p):
        """where every step of the coordinate chain is the same number in fp32 and in fp64"""
        s32, s64 = self.coords(ops, p, F32, steps=True), self.coords(ops, p, F64, steps=True)
        ok = torch.ones(s64[-1].shape, dtype=torch.bool)
        for a, b in zip(s32, s64):
            ok = ok & (a.to(F64) == b)
        return ok.reshape(ops["offset"].shape[:3] + (-1,))

    def dcoord(self, ops, p):
        """d coord / d offset per axis (DCN), or None where the move goes through the coordinate"""
        return None

    def forward(self, t, p, mut, shift, oracle):
        raise NotImplementedError

    def run(self, ops, p, mut=None, shift=None, oracle=True, dtype=F64):
        """forward and gradients in `dtype` -> {output: tensor}; oracle=True: through oracle/tf_ops or deformable_mhsa_ref itself (no mutants)"""
        t = {k: v.to(dtype) for k, v in ops.items()}
        if shift is not None and self.dcoord(ops, p) is not None:
            t["offset"] = self._shifted(t["offset"], shift / per_axis(self.dcoord(ops, p), shift))
            shift = None
        leaves = {k: t[k].clone().requires_grad_(True) for k in self.leaves}
        out = self.forward(dict(t, **leaves), p, mut, shift, oracle and mut is None and shift is None)
        grads = torch.autograd.grad(out, [leaves[k] for k in self.leaves], t["dout"].reshape(out.shape))
        return self.name_outputs(out.detach(), dict(zip(self.leaves, grads)))

    def _shifted(self, off, d):
        return off + d


class DcnV3(Op):
    name, rounds, leaves = "dcnv3", R_DCNV3, ("x", "offset", "mask")

    def coords(self, ops, p, dtype=F64, steps=False):
        _, H, W, _ = ops["x"].shape
        return dcnv3_coordinates(ops["offset"].to(dtype), H, W, p["G"], p.get("s", 1.0), steps)

    def dcoord(self, ops, p):
        _, H, W, _ = ops["x"].shape
        s = p.get("s", 1.0)
        return (s * W / (W + 2), s * H / (H + 2))

    def forward(self, t, p, mut, shift, oracle):
        G, s = p["G"], p.get("s", 1.0)
        if oracle:
            return O.dcnv3_op(t["x"], t["offset"], t["mask"], (3, 3), (1, 1), "SAME", (1, 1), G, t["x"].shape[3] // G, s)
        return dcnv3_restated(t["x"], t["offset"], t["mask"], G, s, mut, shift)

    def name_outputs(self, out, g):
        return {"y": out, "dx": g["x"], "dmask": g["mask"], "doffset": g["offset"]}


class DcnV2(Op):
    name, rounds, leaves = "dcnv2", R_DCNV2, ("x", "offset")

    def coords(self, ops, p, dtype=F64, steps=False):
        _, H, W, _ = ops["x"].shape
        return dcnv2_coordinates(ops["offset"].to(dtype), H, W, steps)

    def hi(self, ops, p):
        _, H, W, _ = ops["x"].shape
        return (H + 1, W + 1)

    def dcoord(self, ops, p):
        return (1.0, 1.0)

    def _shifted(self, off, d):
        return torch.cat([off[..., :18] + d, off[..., 18:]], dim=-1)

    def forward(self, t, p, mut, shift, oracle):
        return dcnv2_oracle_col(t["x"], t["offset"]) if oracle else dcnv2_restated(t["x"], t["offset"], mut, shift)

    def name_outputs(self, out, g):
        return {"col": out, "dx": g["x"], "dlogit": g["offset"][..., 18:], "doffset": g["offset"][..., :18]}


class DefAttn(Op):
    name, rounds, leaves = "defattn", R_DEFATTN, ("value", "offset", "attn")

    def coords(self, ops, p, dtype=F64, steps=False):
        _, H, W, _ = ops["value"].shape
        return defattn_coordinates(ops["offset"].to(dtype), H, W, p["heads"], p["P"], p["orf"], steps)

    def hi(self, ops, p):
        _, H, W, _ = ops["value"].shape
        return (H - 1, W - 1)

    def forward(self, t, p, mut, shift, oracle):
        if oracle:
            return R.core(t["value"], t["offset"], t["attn"], p["heads"], p["P"], p["orf"], scrub=False)
        return defattn_restated(t["value"], t["offset"], t["attn"], p["heads"], p["P"], p["orf"], mut, shift)

    def name_outputs(self, out, g):
        return {"out": out, "dvalue": g["value"], "dattn": g["attn"], "doffset": g["offset"]}


OPS = {"dcnv3": DcnV3(), "dcnv2": DcnV2(), "defattn": DefAttn()}


# ---------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------
def _random_operands(op, p, dtype):
    """the recipes of the core tests (test_dcnv3_gpu.py, test_deformable_mhsa_gpu.py): seeded Gaussians rounded to the storage dtype"""
    shape, seed = p["shape"], p.get("seed", 0)
    N, H, W, C = shape
    if op == "dcnv3":
        G = p["G"]
        d = {"x": rnd(shape, seed + 1), "offset": rnd((N, H, W, G * 18), seed + 2) * p.get("spread", 1.5),
             "mask": torch.softmax(rnd((N, H, W, G, 9), seed + 3), -1).reshape(N, H, W, G * 9), "dout": rnd(shape, seed + 4)}
    elif op == "dcnv2":
        off = rnd((N, H, W, 27), seed + 2)
        off[..., :18] *= p.get("spread", 1.5)
        d = {"x": rnd(shape, seed + 1), "offset": off, "dout": rnd((N, H, W, 9, C), seed + 4)}
    else:
        heads, P = p["heads"], p["P"]
        d = {"value": rnd(shape, seed + 1), "offset": rnd((N, H, W, heads * P * 2), seed + 2) * 1.5, "attn": rnd((N, H, W, heads * P), seed + 3) * 1.5,
             "dout": rnd(shape, seed + 4)}
    return {k: v.to(dtype) for k, v in d.items()}


def _choice(values, shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


DCN_LATTICE_OFFSETS = [k * 0.5 for k in range(-8, 9)]      # the host-side search runs over these storage-dtype offsets (exact in bf16)


def _lattice_operands(op, p, dtype):
    """offsets that put the coordinates ON the kinks.  DCNv2: small integers (0 on the edge pixels is the clip bound itself) and negative
    half-integers.  DCNv3: per element, a seeded pick among the multiples of 1/2 whose fp64 coordinate is an exact integer (W = 2, Win = 4: the +-1/2
    family; other widths: whatever the search finds), a non-lattice pick where there is none; a quarter of the taps that can reach it sit at -1/2 instead.  Deformable attention: logits 0 (every tap on its own
    pixel, the edge pixels on a clip bound) and +-20, where tanh is exactly +-1 in fp32 and fp64 and the offset is the integer H / factor."""
    d = _random_operands(op, p, F64)
    seed = p.get("seed", 0)
    shape = d["offset"].shape
    if op == "dcnv2":
        d["offset"][..., :18] = _choice([-3.0, -2.0, -1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0, -0.5, -1.5, -2.5], shape[:3] + (18,), seed + 7)
    elif op == "defattn":
        d["offset"] = _choice([0.0, 0.0, 0.0, 20.0, -20.0], shape, seed + 7)
    else:
        o = OPS[op]
        pick = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 7), dtype=F64)
        best = torch.full(shape, 0.25, dtype=F64)
        score = torch.full(shape, -1.0, dtype=F64)
        for k, cand in enumerate(DCN_LATTICE_OFFSETS):
            c = o.coords(dict(d, offset=torch.full(shape, cand, dtype=F64)), p)
            s = torch.where(c == torch.round(c), torch.frac(pick * (k + 3) * 7.31), torch.full_like(pick, -1.0))      # a seeded pick among the hits
            s = torch.where((c == -0.5) & (pick < 0.25), 2.0 + s.abs(), s)      # a quarter of the taps that can: a coordinate of -1/2, where truncation is not floor
            best = torch.where(s > score, torch.full_like(best, cand), best)
            score = torch.maximum(score, s)
        d["offset"] = best
    return {k: v.to(dtype) for k, v in d.items()}


def _near_operands(op, p, dtype):
    """the coordinate map inverted in fp64 for (nearest integer inside the image) +- k fp32 ulps, k in {0, 1, 2}; rounded to the storage dtype.
    So that the two sides of a kink differ by much more than the tolerance (the either-side rule proves nothing where they do not), the modulation
    / attention weights are nearly even, tanh stays below 0.8, and the DCN targets stay off the zero ring, where both one-sided gradients of the
    OTHER axis vanish, but for a sixteenth of them, which are put on the first or last row / column of the padded image (DCNv2: its clip bounds)"""
    o = OPS[op]
    d = _random_operands(op, p, F64)
    seed = p.get("seed", 0)
    c = o.coords(d, p)
    ref = d["x" if "x" in d else "value"]
    N, H, W, _ = ref.shape
    g = torch.Generator().manual_seed(seed + 9)
    if op == "dcnv3":
        d["mask"] = torch.softmax(rnd((N, H, W, p["G"], 9), seed + 3) * 0.25, -1).reshape(N, H, W, -1)
    elif op == "defattn":
        d["attn"] = d["attn"] * 0.25
    top = {"dcnv3": (W + 1, H + 1), "dcnv2": (H + 1, W + 1), "defattn": (H - 1, W - 1)}[op]
    if op == "defattn":
        T = torch.minimum(torch.round(c).clamp(min=0.0), per_axis(top, c))
    else:
        T = torch.minimum(torch.round(c).clamp(min=1.0), per_axis(top, c) - 1.0)
        edge = torch.randint(0, 32, c.shape, generator=g)
        T = torch.where(edge == 0, torch.zeros_like(T), torch.where(edge == 1, per_axis(top, c).expand_as(T), T))
    k = torch.randint(-2, 3, c.shape, generator=g).to(F64)
    target = T + k * ULP * torch.exp2(torch.floor(torch.log2(T.clamp(min=1.0))))
    if op == "defattn":
        scale = per_axis((H / p["orf"], W / p["orf"]), c)
        base = c - torch.tanh(d["offset"]) * scale
        ratio = (target - base) / scale
        ok = ratio.abs() < 0.8
        d["offset"] = torch.where(ok, torch.atanh(ratio.clamp(-0.8, 0.8)), d["offset"])
    else:
        new = d["offset"][..., :c.shape[-1]] + (target - c) / per_axis(o.dcoord(d, p), c)
        d["offset"] = torch.cat([new, d["offset"][..., c.shape[-1]:]], dim=-1)
    return {k_: v.to(dtype) for k_, v in d.items()}


BUILD = {"random": _random_operands, "budget": _random_operands, "lattice": _lattice_operands, "near": _near_operands}


class Case(NamedTuple):
    op: str
    name: str
    kind: str
    params: tuple      # sorted (key, value) pairs

    @property
    def p(self):
        return dict(self.params)

    @property
    def id(self):
        return f"{self.op}-{self.kind}-{self.name}"


def _case(op, name, kind, **p):
    return Case(op, name, kind, tuple(sorted(p.items())))


# One shape per route.  DCNv3 forward: pipelined at Cg 8 / 16, general (8-wide loads at Cg 24, scalar otherwise); backward: the window route at Cg 8 /
# 16 (20 x 18: more than one 16 x 16 tile), a lane per channel at Cg 4 / 32, the general kernel 8-wide at Cg 24 and scalar at Cg 3.  DCNv2: C = 8 (one
# chunk), 72 (more chunks than lanes per point).  Deformable attention: the shapes of test_deformable_mhsa_gpu.py (Ch 16 / 8: 16-byte loads; Ch 3:
# one channel per lane).
CASES = [
    _case("dcnv3", "cg16", "random", shape=(2, 9, 7, 32), G=2),
    _case("dcnv3", "cg8_tiles", "random", shape=(1, 20, 18, 16), G=2),
    _case("dcnv3", "cg4_s2", "random", shape=(2, 5, 8, 12), G=3, s=2.0),
    _case("dcnv3", "cg3", "random", shape=(1, 6, 6, 12), G=4),
    _case("dcnv3", "cg24", "random", shape=(1, 7, 9, 24), G=1),
    _case("dcnv3", "cg32", "random", shape=(1, 6, 5, 64), G=2),
    _case("dcnv3", "w2_cg8", "lattice", shape=(8, 2, 2, 16), G=2),
    _case("dcnv3", "w6_cg8", "lattice", shape=(4, 6, 6, 8), G=1),
    _case("dcnv3", "h2w6_cg4", "lattice", shape=(4, 2, 6, 8), G=2),
    _case("dcnv3", "w6_cg3", "lattice", shape=(2, 6, 6, 6), G=2),
    _case("dcnv3", "cg8", "near", shape=(2, 9, 7, 16), G=2),
    _case("dcnv3", "cg4", "near", shape=(2, 5, 8, 12), G=3),
    _case("dcnv3", "40x36", "budget", shape=(2, 40, 36, 32), G=2),
    _case("dcnv2", "c16", "random", shape=(2, 9, 7, 16)),
    _case("dcnv2", "c72", "random", shape=(1, 6, 5, 72)),
    _case("dcnv2", "c8", "lattice", shape=(3, 6, 5, 8)),
    _case("dcnv2", "c72", "lattice", shape=(1, 4, 7, 72)),
    _case("dcnv2", "c16", "near", shape=(2, 9, 7, 16)),
    _case("dcnv2", "40x36", "budget", shape=(2, 40, 36, 32)),
    _case("defattn", "ch16", "random", shape=(2, 9, 7, 32), heads=2, P=4, orf=2.0, seed=0),
    _case("defattn", "ch16_orf8", "random", shape=(1, 12, 12, 64), heads=4, P=4, orf=8.0),
    _case("defattn", "ch3", "random", shape=(2, 5, 8, 9), heads=3, P=3, orf=2.0),
    _case("defattn", "one_point", "random", shape=(1, 6, 6, 12), heads=4, P=1, orf=4.0),
    _case("defattn", "33x30", "random", shape=(1, 33, 30, 32), heads=2, P=4, orf=1.0),
    _case("defattn", "ch16", "lattice", shape=(2, 8, 6, 32), heads=2, P=4, orf=2.0),
    _case("defattn", "ch3", "lattice", shape=(2, 8, 6, 9), heads=3, P=3, orf=2.0),
    _case("defattn", "ch16", "near", shape=(2, 9, 7, 32), heads=2, P=4, orf=2.0),
    _case("defattn", "ch3", "near", shape=(2, 5, 8, 9), heads=3, P=3, orf=2.0),
    _case("defattn", "40x36", "budget", shape=(2, 40, 36, 32), heads=4, P=4, orf=2.0),      # 4 heads: the attention gradient has >= 40 000 elements too
]
DTYPES = (F32, BF)


@functools.lru_cache(maxsize=None)
def operands(case, dtype):
    return BUILD[case.kind](case.op, case.p, dtype)


@functools.lru_cache(maxsize=None)
def classes(case, dtype):
    op, ops, p = OPS[case.op], operands(case, dtype), case.p
    coord = op.coords(ops, p)
    return classify(coord, tau_of(op.rounds, coord), op.hi(ops, p), op.exact(ops, p))


class Reference(NamedTuple):
    base: dict          # {output: fp64 tensor}: the reference as it is
    plus: torch.Tensor      # the offset gradient with every border element on the + side of its kink
    minus: torch.Tensor
    moved: dict         # {continuous output: largest move between the evaluations / (TAU x scale)}


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """the as-is reference and the two one-sided offset gradients; computed once per (case, dtype), shared, never modified"""
    op, ops, p, cls = OPS[case.op], operands(case, dtype), case.p, classes(case, dtype)
    base = op.run(ops, p)
    plus, minus = base["doffset"].clone(), base["doffset"].clone()
    moved = {k: 0.0 for k in base if k != "doffset"}
    axis = torch.arange(cls.coord.shape[-1]) % 2
    for ax in (0, 1):
        sel = cls.border & (axis == ax)
        if not sel.any():
            continue
        for sign, dst in ((1.0, plus), (-1.0, minus)):
            out = op.run(ops, p, shift=sign * 2.0 * cls.tau * sel.to(F64))
            dst[sel] = out["doffset"][sel]
            for k in moved:
                moved[k] = max(moved[k], (out[k] - base[k]).abs().max().item() / (cls.tau * max(base[k].abs().max().item(), 1e-30)))
    return Reference(base, plus, minus, moved)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------
def allowance(op, name, ref, scale, dtype, stored_bf16):
    """fp32 storage: TOL x scale.  bf16 storage: the same for the fp32 arithmetic behind the store (1 % more: the rounding boundary itself moves
    with it), plus 2^-8 |ref| where the output is stored in bf16"""
    if dtype == BF and (op, name) in BF16_FIXED_POINT:
        return torch.full_like(ref, BF16_FIXED_POINT[(op, name)] * scale)
    tol = TOL[op][name] * scale
    if dtype == F32:
        return torch.full_like(ref, tol)
    return 1.01 * tol + (2.0 ** -8 * ref.abs() if stored_bf16 else 0.0)


def judge_offset_gradient(case, dtype, got, ref, cls):
    """-> (lines, failures).  interior and lattice: the as-is reference; border: the + side or the - side.  No element is left out"""
    got = got.detach().cpu().to(F64).reshape(ref.base["doffset"].shape)
    base = ref.base["doffset"]
    scale = max(base.abs().max().item(), 1e-30)

    def excess(r):
        return (got - r).abs() - allowance(case.op, "doffset", r, scale, dtype, dtype == BF)

    ex = torch.where(cls.border, torch.minimum(excess(ref.plus), excess(ref.minus)), excess(base))
    err = torch.where(cls.border, torch.minimum((got - ref.plus).abs(), (got - ref.minus).abs()), (got - base).abs())
    lines, bad = [], []
    for name, sel in (("interior", cls.interior), ("lattice", cls.lattice), ("border", cls.border)):
        n = int(sel.sum())
        if n == 0:
            lines.append(f"KINKS {case.id} {_dt(dtype)} doffset {name}: 0 elements")
            continue
        e = torch.where(sel, err, torch.full_like(err, -1.0)).reshape(-1)
        i = int(e.argmax())
        lines.append(f"KINKS {case.id} {_dt(dtype)} doffset {name}: {n} elements, worst err {e[i].item() / scale:.3e} of scale at [{i}] coord "
                     f"{cls.coord.reshape(-1)[i].item():.9g} got {got.reshape(-1)[i].item():.6g} ref {base.reshape(-1)[i].item():.6g} "
                     f"+ {ref.plus.reshape(-1)[i].item():.6g} - {ref.minus.reshape(-1)[i].item():.6g}")
        nbad = int((sel & (ex > 0)).sum())
        if nbad:
            j = int(torch.where(sel, ex, torch.full_like(ex, -1.0)).reshape(-1).argmax())
            bad.append(f"{case.id} {_dt(dtype)} doffset: {nbad} of {n} {name} elements outside the rule; worst at [{j}]: coord "
                       f"{cls.coord.reshape(-1)[j].item():.9g} got {got.reshape(-1)[j].item():.6g} ref {base.reshape(-1)[j].item():.6g} "
                       f"+ {ref.plus.reshape(-1)[j].item():.6g} - {ref.minus.reshape(-1)[j].item():.6g} (scale {scale:.3e})")
    return lines, bad


def judge_continuous(case, dtype, name, got, ref, stored_bf16):
    want = ref.base[name]
    g = got.detach().cpu().to(F64).reshape(want.shape)
    scale = max(want.abs().max().item(), 1e-30)
    ex = (g - want).abs() - allowance(case.op, name, want, scale, dtype, stored_bf16)
    err = (g - want).abs().max().item() / scale
    line = f"KINKS {case.id} {_dt(dtype)} {name}: {want.numel()} elements, worst err {err:.3e} of scale"
    nbad = int((ex > 0).sum())
    return line, ([f"{case.id} {_dt(dtype)} {name}: {nbad} of {want.numel()} elements off, worst {err:.3e} of scale {scale:.3e}"] if nbad else [])


def _dt(dtype):
    return "bf16" if dtype == BF else "fp32"


def rel_l2(got, want):
    return (got.detach().cpu().to(F64).reshape(want.shape) - want).norm().item() / max(want.norm().item(), 1e-300)


def shares(cls):
    n = cls.coord.numel()
    return {"n": n, "lattice": int(cls.lattice.sum()) / n, "border": int(cls.border.sum()) / n, "on_bound": int(cls.on_bound.sum())}

