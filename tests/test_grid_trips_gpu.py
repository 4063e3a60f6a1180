"""Every capped-grid launcher of iseg_amd/csrc driven through two full trips of its grid-strided loop and a ragged third (the case
table and the launcher arithmetic: tests/grid_trips.py), against a float64 reference of seeded inputs that were rounded to the storage
type first.  Every output element is compared; outputs (and the shared workspace) are NaN before the call, so a trip that was skipped
leaves NaN behind; accumulating entry points start from seeded destinations, so an item handled twice shows; and the ragged last trip is
asserted on its own after the whole tensor, so a failure names the trip.

Tolerances are the project's (`close()` of test_kernels_gpu.py and the per-kernel values of the existing tests).  Column sums over 10^5 ..
10^6 rows use `reduction_tol`: the error of a plain float32 np.sum of the same terms (column by column) against float64, times 8 for the different summation
order, or the project tolerance, whichever is larger; the measured float32-sum errors are recorded next to each case."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import tf_ops as O
from tests import grid_trips as GT
from tests.test_kernels_gpu import close, q, rnd

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def K():
    from iseg_amd import kernels

    return kernels


def storage(name):
    return pytest.mark.parametrize("d", list(GT.BY_NAME[name].shapes))


def shape_of(name, d):
    return dict(GT.BY_NAME[name].shapes[d])


def last_of(name, d, which=0):
    """first item of the ragged last trip of the `which`-th kernel of the entry"""
    c = GT.BY_NAME[name]
    return GT.first_of_last_trip(c.launcher(d, **c.shapes[d])[which])


def nan_like(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


@contextlib.contextmanager
def nan_outputs():
    """what the wrappers allocate (torch.empty / empty_like) is NaN (integers: the most negative value) while the call runs, and the cached
    workspace is all-ones bytes (NaN as floats): an output or a partial-sum slot that no trip wrote stays visible"""
    k = K()
    for buf in k._WS.values():
        buf.fill_(255)
    empty, empty_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_floating_point():
            t.fill_(NAN)
        elif t.dtype == torch.uint8:
            t.fill_(255)
        elif t.dtype == torch.int32:
            t.fill_(-2 ** 31)
        return t

    torch.empty = lambda *a, **kw: poison(empty(*a, **kw))
    torch.empty_like = lambda *a, **kw: poison(empty_like(*a, **kw))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def check(got, want, dtype, what, last, per_item=1, exact=False, **tol):
    """every element, then the ragged last trip (items >= `last`, `per_item` consecutive output elements each) on its own"""
    g = got.detach().reshape(-1).cpu().double()
    w = want.detach().reshape(-1).double()
    assert g.numel() == w.numel(), f"{what}: {g.numel()} outputs, {w.numel()} expected"
    lost = torch.isnan(g) & ~torch.isnan(w)
    if lost.any():
        first = int(lost.nonzero()[0])
        raise AssertionError(f"{what}: {int(lost.sum())} outputs were never written, the first at element {first} = item {first // per_item} "
                             f"(the last trip starts at item {last})")
    assert 0 < last * per_item < g.numel()
    for where, sl in (("all trips", slice(None)), (f"last trip, from item {last}", slice(last * per_item, None))):
        if exact:
            ne = g[sl] != w[sl]
            assert not ne.any(), f"{what} [{where}]: {int(ne.sum())} elements differ, the first at {int(ne.nonzero()[0]) + (sl.start or 0)}"
        else:
            close(g[sl], w[sl], dtype, f"{what} [{where}]", **tol)


def reduction_tol(terms, want, project_tol):
    """absolute tolerance of a long column sum: `terms` [rows, ...] float64 are the addends, `want` their float64 sum over rows.  Eight times
    the error of a plain float32 np.sum of the same addends (the kernel sums in another order), or the project's tolerance times the
    scale of the result, whichever is larger.  Returns (tolerance, measured float32-sum error)."""
    # (every column as a contiguous vector: np.sum then adds in pairwise blocks, as it does for any 1-D array; over axis 0 of a [rows, k]
    # array it would add row after row and its error -- 350 on the 1.4e6 of bn_stats -- would hide a lost workgroup quantum)
    t32 = np.ascontiguousarray(terms.reshape(terms.shape[0], -1).numpy().astype(np.float32).T)
    f32_err = float(np.abs(np.sum(t32, axis=1, dtype=np.float32).astype(np.float64) - want.reshape(-1).numpy()).max())
    return max(8.0 * f32_err, project_tol * max(float(want.abs().max()), 1e-6)), f32_err


def check_sum(got, want, tol, what):
    err = (got.detach().cpu().double().reshape(-1) - want.reshape(-1)).abs().max().item()
    print(f"{what}: max err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"      # (NaN fails too)


def check_sum_with_last_trip(run, rows, last, terms, pre, project_tol, what):
    """`run(n)` returns the kernel's column sums over the first n rows (the grid is at its cap either way); `terms` [rows, ...] are the float64
    addends, `pre` what the destination held.  The whole sum, then the ragged last trip on its own: the difference of the sums over all rows and
    over the rows before the last trip against the float64 sum of the last trip's rows -- each of the two results carries at most the
    tolerance, so their difference carries at most twice that."""
    want = terms.sum(0)
    tol, f32_err = reduction_tol(terms, want, project_tol)
    print(f"{what}: float32 np.sum error {f32_err:.3e}")
    full = run(rows).detach().cpu().double()
    check_sum(full, want + pre, tol, f"{what} [all trips]")
    head = run(last).detach().cpu().double()
    check_sum(full - head, terms[last:].sum(0), 2 * tol, f"{what} [last trip, rows {last}..]")


# ======================================================================================================================================
# elementwise.hip
# ======================================================================================================================================
@storage("cast")
def test_cast(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("cast", d)["n"]
    last = last_of("cast", d)
    src32 = rnd((n,), 1).float()
    out = k.cast(src32.cuda(), dtype, out=nan_like((n,), dtype))            # f32 -> storage type (round to nearest even)
    check(out, src32.to(dtype), dtype, "cast f32 -> storage", last, 8, exact=True)
    back = k.cast(out, torch.float32, out=nan_like((n,), torch.float32))      # storage type -> f32 (exact)
    check(back, src32.to(dtype).float(), torch.float32, "cast storage -> f32", last, 8, exact=True)
    same = k.cast(out, dtype, out=nan_like((n,), dtype))
    check(same, src32.to(dtype), dtype, "cast storage -> storage", last, 8, exact=True)


@storage("scale_cols_cast")
def test_scale_cols_cast(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("scale_cols_cast", d)
    src = rnd((s["rows"], s["cols"]), 1).float()
    cs = (rnd((s["cols"],), 2) * 0.5 + 1).float()
    with nan_outputs():
        out = k.scale_cols_cast(src.cuda(), cs.cuda(), dtype)
    check(out, src.double() * cs.double(), dtype, "scale_cols_cast", last_of("scale_cols_cast", d))


def _patches(xr, K_):
    N, H, W, C = xr.shape
    Ho, Wo = H // K_, W // K_
    return xr[:, :Ho * K_, :Wo * K_].reshape(N, Ho, K_, Wo, K_, C).permute(0, 1, 3, 2, 4, 5).reshape(N * Ho * Wo, K_ * K_ * C)


def _im2col_case(name, d):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    N, H, W, C, K_, st, ldc = (s[x] for x in ("N", "H", "W", "C", "K", "s", "ldc"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    with nan_outputs():
        col = k.im2col(x, K_, K_, st, st, 1, 1, 0, 0, H // st, W // st, dtype, ldc=ldc)
    Kd = K_ * K_ * C
    want = torch.zeros((col.shape[0], ldc), dtype=torch.float64)
    want[:, :Kd] = _patches(xr, K_)
    trips = GT.BY_NAME[name].launcher(d, **s)
    # the copy kernel's items are (pixel, tap, channel chunk) in the order of the patch columns: item i writes elements [i V, (i + 1) V) of the
    # patch matrix without its padding columns (V = 8, 4 for the contiguous-run form, or 1)
    V = col.shape[0] * Kd // trips[0].items
    check(col[:, :Kd], want[:, :Kd], dtype, f"{name} patches", GT.first_of_last_trip(trips[0]), V, exact=True)
    if ldc > Kd:
        check(col[:, Kd:], want[:, Kd:], dtype, f"{name} zero padding columns", GT.first_of_last_trip(trips[1]), exact=True)


@storage("im2col_vec")
def test_im2col_vec(cuda, d):
    _im2col_case("im2col_vec", d)


@storage("im2col_scalar_and_pad")
def test_im2col_scalar_and_pad(cuda, d):
    _im2col_case("im2col_scalar_and_pad", d)


@storage("im2col_runs")
def test_im2col_runs(cuda, d):
    _im2col_case("im2col_runs", d)


def _col2im_case(name, d):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    N, H, W, C, K_, st, ldc = (s[x] for x in ("N", "H", "W", "C", "K", "s", "ldc"))
    Ho, Wo = H // st, W // st
    Kd = K_ * K_ * C
    dcol, dcr = q(rnd((N * Ho * Wo, ldc), 1), dtype)
    with nan_outputs():
        dx = k.col2im(dcol, N, H, W, C, K_, K_, st, st, 1, 1, 0, 0, Ho, Wo)
    # non-overlapping taps: every input pixel is read by exactly one (output pixel, tap)
    want = dcr[:, :Kd].reshape(N, Ho, Wo, K_, K_, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
    V = 8 if C % 8 == 0 else 1
    check(dx, want, dtype, name, last_of(name, d), V, exact=True)


@storage("col2im_vec")
def test_col2im_vec(cuda, d):
    _col2im_case("col2im_vec", d)


@storage("col2im_scalar")
def test_col2im_scalar(cuda, d):
    _col2im_case("col2im_scalar", d)


def _colsum_case(name, d, seed):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    B, rows, C = s["batch"], s["rows"], s["C"]
    x, xr = q(rnd((B, rows, C), seed), dtype)
    pre = rnd((B, C), seed + 1).float()
    last = last_of(name, d)

    def run(n):
        out = pre.clone().cuda()
        with nan_outputs():
            k.colsum(x, C, rows * C, B, n, C, out, scale=1.0, accumulate=True)      # (the sample stride stays: the first n rows of every sample)
        return out

    check_sum_with_last_trip(run, rows, last, xr.permute(1, 0, 2).contiguous(), pre.double(), 1e-4 if d == "f32" else 1e-3, name)


# float32 np.sum error of the addends (N(0, 1), 1 058 053 rows x 8 columns), measured: fp32 storage 4.4e-04, bf16 storage 3.3e-04
@storage("colsum_vec")
def test_colsum_vec(cuda, d):
    _colsum_case("colsum_vec", d, 1)


# float32 np.sum error of the addends (N(0, 1), 2 x 351 310 rows x 3 columns), measured: fp32 storage 1.8e-04, bf16 storage 1.2e-04
@storage("colsum_scalar_batched")
def test_colsum_scalar_batched(cuda, d):
    _colsum_case("colsum_scalar_batched", d, 3)


@storage("broadcast_rows")
def test_broadcast_rows(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("broadcast_rows", d)
    B, R, C = s["B"], s["R"], s["C"]
    last = last_of("broadcast_rows", d)
    v, vr = q(rnd((B, C), 1), dtype)
    want = 0.5 * vr[:, None, :].expand(B, R, C)
    y = nan_like((B, R, C), dtype)
    k.broadcast_rows(v, y, C, R * C, B, R, C, scale=0.5)
    check(y, want, dtype, "broadcast_rows (store)", last, 8)
    y0, y0r = q(rnd((B, R, C), 2), dtype)
    k.broadcast_rows(v, y0, C, R * C, B, R, C, scale=0.5, accumulate=True)
    check(y0, y0r + want, dtype, "broadcast_rows (accumulate)", last, 8)


@storage("axpby")
def test_axpby(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("axpby", d)["n"]
    a, ar = q(rnd((n,), 1), dtype)
    b, br = q(rnd((n,), 2), dtype)
    y = k.axpby(a, b, 2.0, -1.0, out=nan_like((n,), dtype))
    check(y, 2 * ar - br, dtype, "axpby", last_of("axpby", d), 8)
    y = k.axpby(a, None, 0.5, 0.0, out=nan_like((n,), dtype))
    check(y, 0.5 * ar, dtype, "axpby (b = None)", last_of("axpby", d), 8)


@storage("scale_dev")
def test_scale_dev(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("scale_dev", d)["n"]
    x, xr = q(rnd((n,), 1), dtype)
    with nan_outputs():
        y = k.scale_dev(x, torch.tensor([1.75], device="cuda"))
    check(y, 1.75 * xr, dtype, "scale_dev", last_of("scale_dev", d), 8)


@storage("rowscale")
def test_rowscale(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("rowscale", d)
    rows, C, rpg = s["rows"], s["C"], s["rpg"]
    x, xr = q(rnd((rows, C), 1), dtype)
    f = torch.tensor([1.25, 0.0, 2.0], dtype=torch.float32)
    assert (rows - 1) // rpg == 2
    with nan_outputs():
        y = k.rowscale(x, f.cuda(), rpg)
    check(y, xr * f.double()[torch.arange(rows) // rpg][:, None], dtype, "rowscale", last_of("rowscale", d), 8)


def _uniform01(seed, n):
    """uniform01 of csrc/elementwise.hip: splitmix64 of (seed, element index), the top 24 bits as a float in [0, 1)"""
    idx = np.arange(1, n + 1, dtype=np.uint64)
    z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * idx
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


@storage("dropout")
def test_dropout(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("dropout", d)["n"]
    rate, seed = 0.25, 1234
    x, xr = q(rnd((n,), 1) + 3.0, dtype)      # (no zeros among the inputs: a zero output is a dropped element)
    with nan_outputs():
        y = k.dropout(x, rate, seed)
    keep = torch.from_numpy(_uniform01(seed, n) >= np.float32(rate))
    check(y, torch.where(keep, xr / (1.0 - rate), torch.zeros((), dtype=torch.float64)), dtype, "dropout", last_of("dropout", d), 8)
    assert torch.equal(y.cpu() != 0, keep), "the mask is a pure function of (seed, element index)"


@storage("fill_f32")
def test_fill_f32(cuda, d):
    k = K()
    n = shape_of("fill_f32", d)["n"]
    t = k.fill_f32(nan_like((n,), torch.float32), 1.5)
    check(t, torch.full((n,), 1.5), torch.float32, "fill_f32", last_of("fill_f32", d), exact=True)


def _act(v, act, k):
    return {k.ACT_RELU: torch.relu, k.ACT_GELU: O.gelu, k.ACT_SIGMOID: torch.sigmoid, k.ACT_SWISH: lambda t: t * torch.sigmoid(t)}[act](v)


@storage("act_fwd")
def test_act_fwd(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("act_fwd", d)["n"]
    x, xr = q(rnd((n,), 1) * 1.5, dtype)
    for act in (k.ACT_GELU, k.ACT_SWISH):
        with nan_outputs():
            y = k.act_fwd(x, act)
        check(y, _act(xr, act, k), dtype, f"act_fwd({act})", last_of("act_fwd", d), 8)


@storage("act_bwd")
def test_act_bwd(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("act_bwd", d)["n"]
    a, ar = q(rnd((n,), 1) * 1.5, dtype)
    dy, dyr = q(rnd((n,), 2), dtype)
    for act in (k.ACT_GELU, k.ACT_SIGMOID):
        with nan_outputs():
            dx = k.act_bwd(dy, a, act)
        aa = ar.clone().requires_grad_(True)
        _act(aa, act, k).backward(dyr)
        # bf16 storage evaluates gelu' with the polynomial of common.h (|error| <= 5.2e-4): inside the bf16 output tolerance
        check(dx, aa.grad, dtype, f"act_bwd({act})", last_of("act_bwd", d), 8)


@storage("copy2d")
def test_copy2d(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("copy2d", d)
    rows, cols, lds, ldd = s["rows"], s["cols"], s["lds"], s["ldd"]
    src, srcr = q(rnd((rows, lds), 1), dtype)
    dst = k.copy2d(src[:, lds - cols:], lds, nan_like((rows, ldd), dtype), ldd, rows, cols)
    check(dst, srcr[:, lds - cols:], dtype, "copy2d", last_of("copy2d", d), 8, exact=True)


@storage("add2d_f32")
def test_add2d_f32(cuda, d):
    k = K()
    s = shape_of("add2d_f32", d)
    rows, cols, lds, ldd = s["rows"], s["cols"], s["lds"], s["ldd"]
    src = rnd((rows, lds), 1).float()
    dst0 = rnd((rows, ldd), 2).float()
    dst = dst0.clone().cuda()
    k.add2d(src.cuda(), lds, dst, ldd, rows, cols)
    check(dst[:, :cols], dst0[:, :cols].double() + src[:, :cols].double(), torch.float32, "add2d_f32", last_of("add2d_f32", d) // cols, cols)
    assert torch.equal(dst[:, cols:].cpu(), dst0[:, cols:]), "columns past `cols` are not touched"


@storage("scale_rows_f32")
def test_scale_rows_f32(cuda, d):
    k = K()
    s = shape_of("scale_rows_f32", d)
    x = rnd((s["rows"], s["C"]), 1).float()
    f = (rnd((s["rows"],), 2) * 0.5 + 1).float()
    with nan_outputs():
        y = k.scale_rows(x.cuda(), f.cuda())
    check(y, x.double() * f.double()[:, None], torch.float32, "scale_rows_f32", last_of("scale_rows_f32", d))


# ======================================================================================================================================
# misc.hip
# ======================================================================================================================================
def _dirty(n, dtype, last_lane):
    """seeded values with NaN and +-inf in every trip; the largest finite value sits in the ragged last trip of the 16-byte body, the smallest
    in the scalar tail"""
    x = rnd((n,), 1).float()
    for i in (3, n // 3 + 1, 8 * last_lane + 9):
        x[i] = NAN
    x[17], x[n // 2 + 5], x[8 * last_lane + 70] = float("inf"), float("-inf"), float("inf")
    x[8 * last_lane + 11] = 50.0
    x[n - 2] = -60.0
    return x.to(dtype)


@storage("replace_nan_or_inf")
def test_replace_nan_or_inf(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("replace_nan_or_inf", d)["n"]
    last = last_of("replace_nan_or_inf", d, 1)
    assert last >= last_of("replace_nan_or_inf", d, 0)      # the apply pass's last trip lies inside the min / max pass's last trip
    xs = _dirty(n, dtype, last)
    with nan_outputs():
        y = k.replace_nan_or_inf(xs.cuda(), 0.25)
    want = O.replace_nan_or_inf(xs.double(), 0.25)
    assert want.max().item() == 50.0 and want.min().item() == -60.0
    check(y, want, dtype, "replace_nan_or_inf", last, 8, exact=True)


@storage("replace_nan_or_inf_bwd")
def test_replace_nan_or_inf_bwd(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("replace_nan_or_inf_bwd", d)["n"]
    last = last_of("replace_nan_or_inf_bwd", d)
    xs = _dirty(n, dtype, last)
    dy = rnd((n,), 2).to(dtype)
    with nan_outputs():
        dx = k.replace_nan_or_inf_bwd(xs.cuda(), dy.cuda())
    check(dx, torch.where(torch.isfinite(xs), dy, torch.zeros_like(dy)), dtype, "replace_nan_or_inf_bwd", last, 8, exact=True)


# float32 np.sum error of the dscale addends dy * xhat (32 805 rows x 8 columns), measured: fp32 storage 3.6e-05, bf16 storage 5.6e-05
@storage("rmsnorm")
def test_rmsnorm(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("rmsnorm", d)
    rows, C = s["rows"], s["C"]
    last = last_of("rmsnorm", d)
    x, xr = q(rnd((rows, C), 1), dtype)
    scale = (rnd((C,), 2) * 0.3).float()
    dy, dyr = q(rnd((rows, C), 3), dtype)
    with nan_outputs():
        y, rstd = k.rmsnorm_fwd(x, scale.cuda(), 1e-6)
    xx = xr.clone().requires_grad_(True)
    sr = scale.double().requires_grad_(True)
    yr = O.rms_norm(xx, sr, 1e-6)
    check(y, yr, dtype, "rmsnorm fwd", last, C)
    rr = 1.0 / torch.sqrt((xr * xr).mean(-1) + 1e-6)
    check(rstd, rr, torch.float32, "rmsnorm rstd", last)
    yr.backward(dyr)
    pre = rnd((C,), 4).float()
    dxs = {}

    def run(n):
        ds = pre.clone().cuda()
        with nan_outputs():
            dxs[n] = k.rmsnorm_bwd(dy[:n], x[:n], scale.cuda(), rstd[:n], ds, accumulate=True)
        return ds

    check_sum_with_last_trip(run, rows, last, dyr * xr * rr[:, None], pre.double(), 5e-5 if d == "f32" else 2e-2, "rmsnorm dscale")
    check(dxs[rows], xx.grad, dtype, "rmsnorm dx", last, C, f32_tol=5e-5, bf16_tol=2e-2)


@storage("pool2d_fwd")
def test_pool2d_fwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("pool2d_fwd", d)
    N, H, W, C, k_, st = (s[x] for x in ("N", "H", "W", "C", "k", "s"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    (Ho, pt), (Wo, pl) = k.same_pad(H, k_, st, 1), k.same_pad(W, k_, st, 1)
    last = last_of("pool2d_fwd", d)
    with nan_outputs():
        y = k.pool2d_fwd(x, k_, k_, st, st, pt, pl, Ho, Wo, k.POOL_MAX)
    check(y, O.max_pool_same(xr, k_, st), dtype, "max pool fwd", last, exact=True)
    with nan_outputs():
        y = k.pool2d_fwd(x, k_, k_, st, st, pt, pl, Ho, Wo, k.POOL_AVG)
    check(y, O.avg_pool_same(xr, k_, st), dtype, "avg pool fwd", last, f32_tol=1e-6, bf16_tol=8e-3)


@storage("pool2d_bwd_scalar")
def test_pool2d_bwd_scalar(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("pool2d_bwd_scalar", d)
    N, H, W, C, k_, st = (s[x] for x in ("N", "H", "W", "C", "k", "s"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    (Ho, pt), (Wo, pl) = k.same_pad(H, k_, st, 1), k.same_pad(W, k_, st, 1)
    dy, dyr = q(rnd((N, Ho, Wo, C), 2), dtype)
    with nan_outputs():
        dx = k.pool2d_bwd(x, dy, k_, k_, st, st, pt, pl, k.POOL_AVG)
    xx = xr.clone().requires_grad_(True)
    O.avg_pool_same(xx, k_, st).backward(dyr)
    check(dx, xx.grad, dtype, "avg pool bwd", last_of("pool2d_bwd_scalar", d), f32_tol=1e-6, bf16_tol=1.2e-2)


@storage("add_relu")
def test_add_relu(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("add_relu", d)["n"]
    a, ar = q(rnd((n,), 1), dtype)
    b, br = q(rnd((n,), 2), dtype)
    with nan_outputs():
        y = k.add_relu(a, b)
    check(y, torch.relu(ar + br), dtype, "add_relu", last_of("add_relu", d), 8)


# ======================================================================================================================================
# norm.hip: LayerNorm
# ======================================================================================================================================
def _ln_inputs(rows, C, dtype):
    x, xr = q(rnd((rows, C), 1) * 2 + 0.3, dtype)
    g = (rnd((C,), 2) * 0.3 + 1).float()
    b = (rnd((C,), 3) * 0.2).float()
    return x, xr, g, b


def _ln_stats(xr, eps):
    """per-row mean / rstd of the rounded input, as fp32 (what the backward kernels are handed) and as the float64 of that fp32"""
    mu = xr.mean(-1)
    rs = torch.rsqrt(((xr - mu[:, None]) ** 2).mean(-1) + eps)
    return mu.float(), rs.float()


def _ln_bwd_ref(gd, xr, mu, rs):
    """dx = rstd (gd - mean_c gd - xhat mean_c(gd xhat)) for gd = dy * gamma (times whatever scales the branch); also returns xhat"""
    xh = (xr - mu[:, None]) * rs[:, None]
    s1 = gd.mean(-1, keepdim=True)
    s2 = (gd * xh).mean(-1, keepdim=True)
    return rs[:, None] * (gd - s1 - xh * s2), xh


def _ln_fwd_case(name, d):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    last = last_of(name, d)
    x, xr, g, b = _ln_inputs(rows, C, dtype)
    with nan_outputs():
        y, mean, rstd = k.layernorm_fwd(x, g.cuda(), b.cuda(), 1e-6)
    check(y, O.layer_norm(xr, g.double(), b.double(), 1e-6), dtype, f"{name} y", last, C)
    mu, rs = _ln_stats(xr, 1e-6)
    check(mean, mu, torch.float32, f"{name} mean", last, f32_tol=1e-5)
    check(rstd, rs, torch.float32, f"{name} rstd", last, f32_tol=1e-5)


def _ln_bwd_case(name, d, with_add):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    last = last_of(name, d)
    x, xr, g, _ = _ln_inputs(rows, C, dtype)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    add, addr = q(rnd((rows, C), 5), dtype) if with_add else (None, 0.0)
    mean, rstd = _ln_stats(xr, 1e-6)
    dxr, xh = _ln_bwd_ref(dyr * g.double(), xr, mean.double(), rstd.double())
    mean, rstd = mean.cuda(), rstd.cuda()
    pre_g, pre_b = rnd((C,), 6).float(), rnd((C,), 7).float()
    out = {}

    def run(n):
        dg, db = pre_g.clone().cuda(), pre_b.clone().cuda()
        with nan_outputs():
            out[n] = k.layernorm_bwd(dy[:n], x[:n], g.cuda(), mean[:n], rstd[:n], dg, db, dx_add=None if add is None else add[:n], accumulate=True)
        return torch.cat([dg, db])

    terms = torch.cat([dyr * xh, dyr], dim=1)      # [rows, 2 C]: dgamma | dbeta
    del xh
    tol = 2e-4 if d == "f32" else 2e-2
    check_sum_with_last_trip(run, rows, last, terms, torch.cat([pre_g, pre_b]).double(), tol, f"{name} dgamma | dbeta")
    check(out[rows], dxr + addr, dtype, f"{name} dx", last, C, f32_tol=1e-4, bf16_tol=2e-2)


# float32 np.sum error of the addends, dgamma | dbeta columns, measured (the tests print it):
#   C = 96: fp32 storage (65 573 rows) 1.1e-04, bf16 storage (262 181 rows) 2.7e-04
#   C = 8 (1 048 613 rows): fp32 5.4e-04, bf16 4.3e-04;   C = 5 (16 421 rows): fp32 2.6e-05, bf16 2.3e-05
@storage("layernorm_fwd_c96")
def test_layernorm_fwd_c96(cuda, d):
    _ln_fwd_case("layernorm_fwd_c96", d)


@storage("layernorm_bwd_c96")
def test_layernorm_bwd_c96(cuda, d):
    _ln_bwd_case("layernorm_bwd_c96", d, with_add=False)


@storage("layernorm_fwd_c8")
def test_layernorm_fwd_c8(cuda, d):
    _ln_fwd_case("layernorm_fwd_c8", d)


@storage("layernorm_bwd_c8")
def test_layernorm_bwd_c8(cuda, d):
    _ln_bwd_case("layernorm_bwd_c8", d, with_add=True)


@storage("layernorm_fwd_any_c5")
def test_layernorm_fwd_any_c5(cuda, d):
    _ln_fwd_case("layernorm_fwd_any_c5", d)


@storage("layernorm_bwd_any_c5")
def test_layernorm_bwd_any_c5(cuda, d):
    _ln_bwd_case("layernorm_bwd_any_c5", d, with_add=True)


def _post_scales(rows, C):
    cs = (rnd((C,), 6) * 0.4 + 1).float()
    rs = torch.tensor([1.25, 0.0, 2.0], dtype=torch.float32)
    rpg = -(-rows // 3)
    return cs, rs, rpg, rs.double()[torch.arange(rows) // rpg][:, None]


@storage("layernorm_post_fwd")
def test_layernorm_post_fwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("layernorm_post_fwd", d)
    rows, C = s["rows"], s["C"]
    x, xr, g, b = _ln_inputs(rows, C, dtype)
    cs, rs, rpg, rowf = _post_scales(rows, C)
    res, resr = q(rnd((rows, C), 7), dtype)
    with nan_outputs():
        y, mean, rstd = k.layernorm_post_fwd(x, g.cuda(), b.cuda(), 1e-6, colscale=cs.cuda(), rowscale=rs.cuda(), rows_per_group=rpg, residual=res)
    want = resr + rowf * cs.double() * O.layer_norm(xr, g.double(), b.double(), 1e-6)
    check(y, want, dtype, "layernorm_post_fwd y", last_of("layernorm_post_fwd", d), C)
    check(mean, _ln_stats(xr, 1e-6)[0], torch.float32, "layernorm_post_fwd mean", last_of("layernorm_post_fwd", d), f32_tol=1e-5)


# float32 np.sum error of the addends, dgamma | dbeta | dcolscale columns, measured: fp32 storage (65 573 rows) 1.3e-04, bf16 storage (262 181 rows) 3.9e-04
@storage("layernorm_post_bwd")
def test_layernorm_post_bwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("layernorm_post_bwd", d)
    rows, C = s["rows"], s["C"]
    last = last_of("layernorm_post_bwd", d)
    x, xr, g, b = _ln_inputs(rows, C, dtype)
    cs, rs, rpg, rowf = _post_scales(rows, C)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    mean, rstd = _ln_stats(xr, 1e-6)
    rdy = dyr * rowf                                    # the gradient that reaches colscale * LN(x)
    dxr, xh = _ln_bwd_ref(rdy * (cs.double() * g.double()), xr, mean.double(), rstd.double())
    A, B = rdy * xh, rdy                                # column sums A, B: dgamma += cs A, dbeta += cs B, dcolscale += gamma A + beta B
    del xh
    terms = torch.cat([cs.double() * A, cs.double() * B, g.double() * A + b.double() * B], dim=1)
    del A, B
    mean, rstd = mean.cuda(), rstd.cuda()
    pre = rnd((3 * C,), 8).float()
    out = {}

    def run(n):
        dg, db, dc = (pre[i * C:(i + 1) * C].clone().cuda() for i in range(3))
        with nan_outputs():
            out[n] = k.layernorm_post_bwd(dy[:n], x[:n], g.cuda(), b.cuda(), mean[:n], rstd[:n], dg, db, colscale=cs.cuda(), dcolscale=dc,
                                          rowscale=rs.cuda(), rows_per_group=rpg)
        return torch.cat([dg, db, dc])

    check_sum_with_last_trip(run, rows, last, terms, pre.double(), 2e-4 if d == "f32" else 2e-2, "layernorm_post_bwd dgamma | dbeta | dcolscale")
    check(out[rows], dxr, dtype, "layernorm_post_bwd dx", last, C, f32_tol=1e-4, bf16_tol=2e-2)


def _gather_table(rows_out, seed):
    """output row -> source row with a padding row (-1) at every 17th output position, and the inverse table"""
    gen = torch.Generator().manual_seed(seed)
    keep = torch.ones(rows_out, dtype=torch.bool)
    keep[::17] = False
    n_in = int(keep.sum())
    fwd = torch.full((rows_out,), -1, dtype=torch.int32)
    fwd[keep] = torch.randperm(n_in, generator=gen).int()
    inv = torch.empty(n_in, dtype=torch.int32)
    inv[fwd[keep].long()] = torch.nonzero(keep).flatten().int()
    return fwd, inv, n_in


@storage("layernorm_gather_fwd")
def test_layernorm_gather_fwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("layernorm_gather_fwd", d)
    rows, C = s["rows"], s["C"]
    last = last_of("layernorm_gather_fwd", d)
    fwd, _, n_in = _gather_table(rows, 11)
    x, xr, g, b = _ln_inputs(n_in, C, dtype)
    with nan_outputs():
        y, mean, rstd = k.layernorm_gather_fwd(x, fwd.cuda(), g.cuda(), b.cuda(), 1e-5)
    pad = (fwd < 0)[:, None]
    src = fwd.clamp(min=0).long()
    zero = torch.zeros((), dtype=torch.float64)
    check(y, torch.where(pad, zero, O.layer_norm(xr, g.double(), b.double(), 1e-5)[src]), dtype, "layernorm_gather_fwd y", last, C)
    mu, rs = _ln_stats(xr, 1e-5)
    check(mean, torch.where(pad[:, 0], zero, mu.double()[src]), torch.float32, "layernorm_gather_fwd mean", last, f32_tol=1e-5)
    check(rstd, torch.where(pad[:, 0], zero, rs.double()[src]), torch.float32, "layernorm_gather_fwd rstd", last, f32_tol=1e-5)


# float32 np.sum error of the addends, dgamma | dbeta columns, measured: fp32 storage (65 573 rows) 9.7e-05, bf16 storage (262 181 rows) 2.3e-04
@storage("layernorm_gather_bwd")
def test_layernorm_gather_bwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("layernorm_gather_bwd", d)
    rows, C = s["rows"], s["C"]                       # SOURCE rows: the loop of the backward kernel
    last = last_of("layernorm_gather_bwd", d)
    rows_out = rows + -(-rows // 16)                  # one padding row per 16 source rows
    fwd, inv, n_in = _gather_table(rows_out, 12)
    assert n_in == rows
    inv[::11] = -1                                    # source rows whose gradient never arrives: dx = dx_add (none here), no parameter gradient
    x, xr, g, _ = _ln_inputs(rows, C, dtype)
    dy, dyr = q(rnd((rows_out, C), 4), dtype)
    mu, rs = _ln_stats(xr, 1e-5)
    has = (inv >= 0)
    src = inv.clamp(min=0).long()
    mean_out, rstd_out = torch.zeros(rows_out), torch.zeros(rows_out)      # statistics live per OUTPUT row
    mean_out[src[has]], rstd_out[src[has]] = mu[has], rs[has]
    d_src = torch.where(has[:, None], dyr[src], torch.zeros((), dtype=torch.float64))
    dxr, xh = _ln_bwd_ref(d_src * g.double(), xr, mu.double(), torch.where(has, rs.double(), torch.zeros((), dtype=torch.float64)))
    terms = torch.cat([d_src * (xr - mu.double()[:, None]) * rs.double()[:, None], d_src], dim=1)
    del xh
    mean_out, rstd_out, inv_d = mean_out.cuda(), rstd_out.cuda(), inv.cuda()
    pre = rnd((2 * C,), 6).float()
    out = {}

    def run(n):
        dg, db = pre[:C].clone().cuda(), pre[C:].clone().cuda()
        with nan_outputs():
            out[n] = k.layernorm_gather_bwd(dy, inv_d[:n], x[:n], g.cuda(), mean_out, rstd_out, dg, db, accumulate=True)
        return torch.cat([dg, db])

    check_sum_with_last_trip(run, rows, last, terms, pre.double(), 2e-4 if d == "f32" else 2e-2, "layernorm_gather_bwd dgamma | dbeta")
    check(out[rows], dxr, dtype, "layernorm_gather_bwd dx", last, C, f32_tol=1e-4, bf16_tol=2e-2)


# ======================================================================================================================================
# norm.hip: BatchNorm
# ======================================================================================================================================
def _bn_vectors(C):
    mean = (rnd((C,), 11) * 0.3 + 0.2).float()
    rstd = (rnd((C,), 12).abs() * 0.2 + 0.6).float()
    g = (rnd((C,), 13) * 0.3 + 1).float()
    b = (rnd((C,), 14) * 0.2).float()
    return mean, rstd, g, b


def _bn_pre(xr, mean, rstd, g, b):
    return (xr - mean.double()) * rstd.double() * g.double() + b.double()


def _away_from_relu_edge(x, xr, vec, dtype):
    """the kernels that re-derive the ReLU mask evaluate (x - mean) rstd gamma + beta in fp32: inputs whose pre-activation is within 1e-3 of zero are
    moved (by 1 / 16: exact in both storage types at this magnitude) so that the two sides cannot disagree on a mask bit"""
    near = _bn_pre(xr, *vec).abs() < 1e-3
    xr = torch.where(near, (xr + 0.0625).to(dtype).double(), xr)
    assert (_bn_pre(xr, *vec).abs() >= 1e-3).all()
    return xr.to(dtype).cuda(), xr


# float32 np.sum error of the addends x | x^2 (599 301 rows x 8 columns), measured: fp32 storage 5.1e-01, bf16 storage 3.8e-01 on sums of 1.4e6
@storage("bn_stats")
def test_bn_stats(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("bn_stats", d)
    rows, C = s["rows"], s["C"]
    x, xr = q(rnd((rows, C), 1) * 1.5 + 0.2, dtype)
    counts = {}

    def run(n):
        with nan_outputs():
            packed = k.bn_stats(x[:n], C, n, C)
        counts[n] = packed[2 * C].item()
        return packed[:2 * C]

    check_sum_with_last_trip(run, rows, last_of("bn_stats", d), torch.cat([xr, xr * xr], dim=1), torch.zeros(2 * C, dtype=torch.float64), 1e-4,
                             "bn_stats sum | sumsq")
    assert counts[rows] == rows


def _bn_apply_case(name, d, packed_form):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    x, xr = q(rnd((rows, C), 1) * 1.5 + 0.2, dtype)
    mean, rstd, g, b = _bn_vectors(C)
    y = nan_like((rows, C), dtype)
    if packed_form:
        packed = torch.cat([xr.sum(0), (xr * xr).sum(0), torch.tensor([float(rows)], dtype=torch.float64)]).float()
        mm, mv = rnd((C,), 6).float(), (rnd((C,), 7).abs() + 0.5).float()
        mm_d, mv_d = mm.clone().cuda(), mv.clone().cuda()
        with nan_outputs():
            mean_d, rstd_d = k.bn_finalize_apply(packed.cuda(), x, C, g.cuda(), b.cuda(), y, C, rows, C, 1e-3, 0.9, mm_d, mv_d, True)
        m = packed[:C].double() / rows
        var = packed[C:2 * C].double() / rows - m * m
        close(mean_d, m, torch.float32, f"{name} mean", f32_tol=1e-5)
        close(rstd_d, torch.rsqrt(var + 1e-3), torch.float32, f"{name} rstd", f32_tol=1e-5)
        close(mm_d, O.moving_update(mm.double(), m, 0.9), torch.float32, f"{name} moving mean", f32_tol=1e-5)
        close(mv_d, O.moving_update(mv.double(), var, 0.9), torch.float32, f"{name} moving var", f32_tol=1e-5)
        mean, rstd = mean_d.cpu(), rstd_d.cpu()      # the activations are held to the statistics the launch itself published
    else:
        k.bn_apply_fwd(x, C, mean.cuda(), rstd.cuda(), g.cuda(), b.cuda(), y, C, rows, C, True)
    check(y, torch.relu(_bn_pre(xr, mean, rstd, g, b)), dtype, f"{name} y", last_of(name, d), C, f32_tol=1e-4)


@storage("bn_apply_fwd")
def test_bn_apply_fwd(cuda, d):
    _bn_apply_case("bn_apply_fwd", d, False)


@storage("bn_apply_fwd_packed")
def test_bn_apply_fwd_packed(cuda, d):
    _bn_apply_case("bn_apply_fwd_packed", d, True)


# float32 np.sum error of the addends dz | dz xhat (1 320 197 rows x 8 columns), measured: fp32 storage 6.9e-04, bf16 storage 1.0e-03
@storage("bn_bwd_reduce")
def test_bn_bwd_reduce(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("bn_bwd_reduce", d)
    rows, C = s["rows"], s["C"]
    x, xr = q(rnd((rows, C), 1) * 1.5 + 0.2, dtype)
    vec = _bn_vectors(C)
    mean, rstd, g, b = vec
    y, yr = q(torch.relu(_bn_pre(xr, *vec)), dtype)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    dz = dyr * (yr > 0)
    del yr
    terms = torch.cat([dz, dz * (xr - mean.double()) * rstd.double()], dim=1)

    def run(n):
        with nan_outputs():
            return k.bn_bwd_reduce(dy[:n], C, x[:n], C, y[:n], C, mean.cuda(), rstd.cuda(), n, C, True)

    check_sum_with_last_trip(run, rows, last_of("bn_bwd_reduce", d), terms, torch.zeros(2 * C, dtype=torch.float64), 3e-4 if d == "f32" else 3e-2,
                             "bn_bwd_reduce dbeta | dgamma")


# float32 np.sum error of the addends dz | dz xhat (1 320 197 rows x 8 columns), measured: fp32 storage 4.3e-04, bf16 storage 2.8e-04
@storage("bn_bwd_reduce_remask")
def test_bn_bwd_reduce_remask(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("bn_bwd_reduce_remask", d)
    rows, C = s["rows"], s["C"]
    vec = _bn_vectors(C)
    mean, rstd, g, b = vec
    x, xr = _away_from_relu_edge(*q(rnd((rows, C), 1) * 1.5 + 0.2, DT[d]), vec, dtype)
    dy, dyr = q(rnd((rows, C), 4), dtype)
    dz = dyr * (_bn_pre(xr, *vec) > 0)
    terms = torch.cat([dz, dz * (xr - mean.double()) * rstd.double()], dim=1)

    def run(n):
        with nan_outputs():
            return k.bn_bwd_reduce_remask(dy[:n], C, x[:n], C, mean.cuda(), rstd.cuda(), g.cuda(), b.cuda(), n, C)

    check_sum_with_last_trip(run, rows, last_of("bn_bwd_reduce_remask", d), terms, torch.zeros(2 * C, dtype=torch.float64),
                             3e-4 if d == "f32" else 3e-2, "bn_bwd_reduce_remask dbeta | dgamma")


def _bn_bwd_apply_case(name, d, remask):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    vec = _bn_vectors(C)
    mean, rstd, g, b = vec
    x, xr = q(rnd((rows, C), 1) * 1.5 + 0.2, dtype)
    if remask:
        x, xr = _away_from_relu_edge(x, xr, vec, dtype)
        mask = _bn_pre(xr, *vec) > 0
    else:
        y, yr = q(torch.relu(_bn_pre(xr, *vec)), dtype)
        mask = yr > 0
        del yr
    dy, dyr = q(rnd((rows, C), 4), dtype)
    sums = (rnd((2 * C,), 5) * rows ** 0.5).float()      # any vector serves: the launch applies the sums it is handed (all-reduced in training)
    pre_g, pre_b = rnd((C,), 6).float(), rnd((C,), 7).float()
    dg, db = pre_g.clone().cuda(), pre_b.clone().cuda()
    dx = nan_like((rows, C), dtype)
    if remask:
        k.bn_bwd_apply_remask(dy, C, x, C, mean.cuda(), rstd.cuda(), g.cuda(), b.cuda(), sums.cuda(), 1.0 / rows, dx, C, rows, C, dgamma=dg, dbeta=db)
    else:
        k.bn_bwd_apply(dy, C, x, C, y, C, mean.cuda(), rstd.cuda(), g.cuda(), sums.cuda(), 1.0 / rows, dx, C, rows, C, True, dgamma=dg, dbeta=db)
    xh = (xr - mean.double()) * rstd.double()
    want = g.double() * rstd.double() * (dyr * mask - sums[:C].double() / rows - xh * sums[C:].double() / rows)
    check(dx, want, dtype, f"{name} dx", last_of(name, d), C, f32_tol=3e-4, bf16_tol=3e-2)
    # booked once, by one lane: a second booking (the lane of another trip) would double the addend
    close(db, pre_b.double() + sums[:C].double(), torch.float32, f"{name} dbeta += sums[:C]", f32_tol=1e-6)
    close(dg, pre_g.double() + sums[C:].double(), torch.float32, f"{name} dgamma += sums[C:]", f32_tol=1e-6)


@storage("bn_bwd_apply")
def test_bn_bwd_apply(cuda, d):
    _bn_bwd_apply_case("bn_bwd_apply", d, False)


@storage("bn_bwd_apply_remask")
def test_bn_bwd_apply_remask(cuda, d):
    _bn_bwd_apply_case("bn_bwd_apply_remask", d, True)


# ======================================================================================================================================
# resize.hip
# ======================================================================================================================================
def _resize_bwd_ref(dyr, Hi, Wi, align_corners=False):
    """transpose of O.resize_bilinear in float64: the same float32 lerp tables, scattered one axis at a time"""
    N, Ho, Wo, C = dyr.shape
    ylo, yhi, ty = O._interp_weights(Ho, Hi, torch.float64, align_corners)
    xlo, xhi, tx = O._interp_weights(Wo, Wi, torch.float64, align_corners)
    ty, tx = ty.view(1, Ho, 1, 1), tx.view(1, 1, Wo, 1)
    t = torch.zeros((N, Hi, Wo, C), dtype=torch.float64)
    t.index_add_(1, ylo, dyr * (1 - ty))
    t.index_add_(1, yhi, dyr * ty)
    out = torch.zeros((N, Hi, Wi, C), dtype=torch.float64)
    out.index_add_(2, xlo, t * (1 - tx))
    out.index_add_(2, xhi, t * tx)
    return out


# Source widths stay small in these cases on purpose.  The kernels form src = (dst + 0.5) * scale - 0.5 in fp32 with one fused multiply-add, the
# restatement (and TensorFlow) with two roundings: near src = 1000 the two differ by an ulp of 1.2e-4, which moves the lerp weights by as much --
# 2.6e-5 of the largest gradient at Wi = 1171, outside the 2e-5 these tests hold the narrow maps to.  test_resize_bwd_x_scalar_wide keeps a wide
# source with the tolerance that coordinate error gives.
def _resize_fwd_case(name, d, out_dtype=None, align_corners=False):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    N, Hi, Wi, Ho, Wo, C = (s[x] for x in ("N", "Hi", "Wi", "Ho", "Wo", "C"))
    x, xr = q(rnd((N, Hi, Wi, C), 1), dtype)
    with nan_outputs():
        y = k.resize_bilinear(x, Ho, Wo, out_dtype=out_dtype or dtype, align_corners=align_corners)
    t = GT.BY_NAME[name].launcher(d, **s)[0]
    check(y, O.resize_bilinear(xr, (Ho, Wo), align_corners), out_dtype or dtype, name, GT.first_of_last_trip(t), N * Ho * Wo * C // t.items, f32_tol=1e-5)


@storage("resize_fwd_rows")
def test_resize_fwd_rows(cuda, d):
    _resize_fwd_case("resize_fwd_rows", d, torch.float32)


@storage("resize_fwd_lds_rows")
def test_resize_fwd_lds_rows(cuda, d):
    _resize_fwd_case("resize_fwd_lds_rows", d, torch.float32)


@storage("resize_fwd_vec")
def test_resize_fwd_vec(cuda, d):
    _resize_fwd_case("resize_fwd_vec", d)


@storage("resize_ac_fwd_rows")
def test_resize_ac_fwd_rows(cuda, d):
    _resize_fwd_case("resize_ac_fwd_rows", d, torch.float32, align_corners=True)


def _resize_bwd_case(name, d, last_elem, dy_dtype=None, with_add=True, align_corners=False):
    """`last_elem(shape)`: first element of dx that the ragged last trip of the crossed pass feeds"""
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    N, Hi, Wi, Ho, Wo, C = (s[x] for x in ("N", "Hi", "Wi", "Ho", "Wo", "C"))
    dy, dyr = q(rnd((N, Ho, Wo, C), 2), dy_dtype or dtype)
    add, addr = q(rnd((N, Hi, Wi, C), 3), dtype) if with_add else (None, 0.0)
    with nan_outputs():
        dx = k.resize_bilinear_bwd(dy, Hi, Wi, dtype, dx_add=add, align_corners=align_corners)
    check(dx, _resize_bwd_ref(dyr, Hi, Wi, align_corners) + addr, dtype, name, last_elem, f32_tol=2e-5, bf16_tol=1.2e-2)


def _last_dx_row(s):
    return (s["N"] * s["Hi"] - 1) * s["Wi"] * s["C"]      # the X pass's last gradient rows (sample N - 1, oy near Ho - 1) feed the last row of dx


@storage("resize_bwd_x_lds_rows")
def test_resize_bwd_x_lds_rows(cuda, d):
    _resize_bwd_case("resize_bwd_x_lds_rows", d, _last_dx_row(shape_of("resize_bwd_x_lds_rows", d)), dy_dtype=torch.float32)


@storage("resize_bwd_x_scalar")
def test_resize_bwd_x_scalar(cuda, d):
    # Hi = Ho: the intermediate of the X pass has the layout of dx, so the X pass's last trip is the tail of dx (and no long vertical sum rides along)
    _resize_bwd_case("resize_bwd_x_scalar", d, last_of("resize_bwd_x_scalar", d))


@storage("resize_bwd_x_scalar_wide")
def test_resize_bwd_x_scalar_wide(cuda, d):
    """a source 1171 pixels wide (real maps are): on top of the project's 2e-5, one ulp of the fp32 source coordinate (2^-13 below 2048) on each
    of the at most 2 ceil(Wo / Wi) + 3 destinations that feed a source pixel, times the largest gradient"""
    k = K()
    s = shape_of("resize_bwd_x_scalar_wide", d)
    N, Hi, Wi, Ho, Wo, C = (s[x] for x in ("N", "Hi", "Wi", "Ho", "Wo", "C"))
    dy, dyr = q(rnd((N, Ho, Wo, C), 2), torch.float32)
    with nan_outputs():
        dx = k.resize_bilinear_bwd(dy, Hi, Wi, torch.float32)
    want = _resize_bwd_ref(dyr, Hi, Wi).reshape(-1)
    got = dx.cpu().double().reshape(-1)
    assert not torch.isnan(got).any()
    last = last_of("resize_bwd_x_scalar_wide", d)
    tol = 2e-5 * want.abs().max().item() + (2 * -(-Wo // Wi) + 3) * 2.0 ** -13 * dyr.abs().max().item()
    for where, sl in (("all trips", slice(None)), (f"last trip, from element {last}", slice(last, None))):
        err = (got[sl] - want[sl]).abs().max().item()
        print(f"resize_bwd_x_scalar_wide [{where}]: max err {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, f"resize_bwd_x_scalar_wide [{where}]: {err:.3e} > {tol:.3e}"


@storage("resize_bwd_x_vec")
def test_resize_bwd_x_vec(cuda, d):
    _resize_bwd_case("resize_bwd_x_vec", d, 8 * last_of("resize_bwd_x_vec", d))


@storage("resize_bwd_y_scalar")
def test_resize_bwd_y_scalar(cuda, d):
    _resize_bwd_case("resize_bwd_y_scalar", d, last_of("resize_bwd_y_scalar", d))


@storage("resize_bwd_y_vec")
def test_resize_bwd_y_vec(cuda, d):
    _resize_bwd_case("resize_bwd_y_vec", d, 8 * last_of("resize_bwd_y_vec", d))


@storage("resize_bwd_x2")
def test_resize_bwd_x2(cuda, d):
    _resize_bwd_case("resize_bwd_x2", d, 8 * last_of("resize_bwd_x2", d), with_add=False)


@storage("resize_ac_bwd")
def test_resize_ac_bwd(cuda, d):
    _resize_bwd_case("resize_ac_bwd", d, last_of("resize_ac_bwd", d, 1), align_corners=True)


@storage("resize_nearest_i32")
def test_resize_nearest_i32(cuda, d):
    k = K()
    s = shape_of("resize_nearest_i32", d)
    N, Hi, Wi, Ho, Wo, C = (s[x] for x in ("N", "Hi", "Wi", "Ho", "Wo", "C"))
    lab = torch.randint(0, 21, (N, Hi, Wi, C), dtype=torch.int32, generator=torch.Generator().manual_seed(1))
    with nan_outputs():
        y = k.resize_nearest_i32(lab.cuda(), Ho, Wo)
    check(y, O.resize_nearest(lab, (Ho, Wo)), torch.float32, "resize_nearest_i32", last_of("resize_nearest_i32", d), exact=True)


@storage("bn_relu_upsample_add")
def test_bn_relu_upsample_add(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("bn_relu_upsample_add", d)
    N, Hi, Wi, Ho, Wo, C = (s[x] for x in ("N", "Hi", "Wi", "Ho", "Wo", "C"))
    z, zr = q(rnd((N, Ho, Wo, C), 1) * 1.5 + 0.2, dtype)
    xc, xcr = q(rnd((N, Hi, Wi, C), 2), dtype)
    vec = _bn_vectors(C)
    with nan_outputs():
        out = k.bn_relu_upsample_add(z, *(v.cuda() for v in vec), xc)
    want = torch.relu(_bn_pre(zr, *vec)) + O.resize_bilinear(xcr, (Ho, Wo))
    check(out, want, dtype, "bn_relu_upsample_add", last_of("bn_relu_upsample_add", d), C, f32_tol=1e-4, bf16_tol=2e-2)


# ======================================================================================================================================
# attention.hip
# ======================================================================================================================================
@storage("clip_fwd_bwd")
def test_clip_fwd_bwd(cuda, d):
    k, dtype = K(), DT[d]
    n = shape_of("clip_fwd_bwd", d)["n"]
    last = last_of("clip_fwd_bwd", d)
    x, xr = q(rnd((n,), 1), dtype)
    dy, dyr = q(rnd((n,), 2), dtype)
    lo, hi = -0.5, 0.75                      # exact in both storage types: the pass test x >= lo && x <= hi has no rounding on either side
    with nan_outputs():
        y = k.clip_fwd(x, lo, hi)
    check(y, xr.clamp(lo, hi), dtype, "clip_fwd", last, exact=True)
    with nan_outputs():
        dx = k.clip_bwd(x, dy, lo, hi)
    check(dx, torch.where((xr >= lo) & (xr <= hi), dyr, torch.zeros((), dtype=torch.float64)), dtype, "clip_bwd", last, exact=True)


def _gather_case(name, d):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    fwd, _, n_in = _gather_table(rows, 21)
    x, xr = q(rnd((n_in, C), 1), dtype)
    with nan_outputs():
        y = k.gather_rows(x, fwd.cuda(), rows)
    want = torch.where((fwd < 0)[:, None], torch.zeros((), dtype=torch.float64), xr[fwd.clamp(min=0).long()])
    t = GT.BY_NAME[name].launcher(d, **s)[0]
    check(y, want, dtype, name, GT.first_of_last_trip(t), rows * C // t.items, exact=True)


@storage("gather_rows_vec")
def test_gather_rows_vec(cuda, d):
    _gather_case("gather_rows_vec", d)


@storage("gather_rows_scalar")
def test_gather_rows_scalar(cuda, d):
    _gather_case("gather_rows_scalar", d)


@storage("gather_rows_fma")
def test_gather_rows_fma(cuda, d):
    """window reverse + roll back + crop + drop path + skip connection of a Swin block (out[m] = res[m] + f[m // rpg] * w[inv[m]]), and its gradient
    towards the window rows (by the forward table, with the factor of the SOURCE row's sample)"""
    k, dtype = K(), DT[d]
    s = shape_of("gather_rows_fma", d)
    rows, C, use_res = s["rows"], s["C"], s["res"]
    last = last_of("gather_rows_fma", d)
    fwd, inv, n_in = _gather_table(rows, 22)         # fwd: window row -> token (or padding); inv: token -> window row
    rpg = -(-n_in // 3)
    f = torch.tensor([1.25, 0.0, 2.0], dtype=torch.float32)
    fo = f.double()[torch.arange(n_in) // rpg][:, None]
    zero = torch.zeros((), dtype=torch.float64)
    # the gradient form: rows = window rows (the capped loop), source = token rows, the factor of the source row's group, no residual
    dtok, dtokr = q(rnd((n_in, C), 1), dtype)
    with nan_outputs():
        dw = k.gather_rows_fma(dtok, fwd.cuda(), f.cuda(), rpg, True, None)
    check(dw, torch.where((fwd < 0)[:, None], zero, (fo * dtokr)[fwd.clamp(min=0).long()]), dtype, "gather_rows_fma (by source row)", last, C)
    del dtok, dtokr
    # the forward form over as many output rows: every output row reads a source row, the factor of the OUTPUT row's group, with the residual
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(23)).int()
    w, wr = q(rnd((rows, C), 2), dtype)
    res, resr = q(rnd((rows, C), 3), dtype) if use_res else (None, 0.0)
    rpg2 = -(-rows // 3)
    fo2 = f.double()[torch.arange(rows) // rpg2][:, None]
    with nan_outputs():
        out = k.gather_rows_fma(w, perm.cuda(), f.cuda(), rpg2, False, res)
    check(out, resr + fo2 * wr[perm.long()], dtype, "gather_rows_fma (by output row)", last, C)


def _softmax_case(name, d, inplace=False):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    problems, Tq, cols, ld = s["problems"], s["Tq"], s["cols"], s["ld"]
    rows = problems * Tq
    last = last_of(name, d)
    heads, nW = 3, 4
    sc, scr = q(rnd((rows, ld), 1) * 2, dtype)
    bias = rnd((heads, Tq, cols), 2).float()
    mask = torch.where(rnd((nW, Tq, cols), 3) > 1.0, -100.0, 0.0).float()
    probs = sc if inplace else nan_like((rows, ld), dtype)      # (in place: the widest form has room for two tensors only)
    k.softmax_rows_fwd(sc, problems, Tq, cols, ld, bias=bias.cuda(), heads=heads, mask=mask.cuda(), windows=nW, out=probs)
    z = torch.arange(problems)
    logits = scr[:, :cols].reshape(problems, Tq, cols) + bias.double()[z % heads] + mask.double()[(z // heads) % nW]
    want = torch.zeros((rows, ld), dtype=torch.float64)
    want[:, :cols] = torch.softmax(logits, -1).reshape(rows, cols)
    check(probs, want, dtype, f"{name} fwd (padding columns are zeros)", last, ld, f32_tol=2e-5, bf16_tol=1.2e-2)
    del sc, probs, logits
    p, pr = q(want, dtype)
    dp, dpr = q(rnd((rows, ld), 4), dtype)
    ds = dp if inplace else nan_like((rows, ld), dtype)
    k.softmax_rows_bwd(p, dp, rows, cols, ld, out=ds)
    wd = torch.zeros((rows, ld), dtype=torch.float64)
    pc, gc = pr[:, :cols], dpr[:, :cols]
    wd[:, :cols] = pc * (gc - (gc * pc).sum(-1, keepdim=True))
    check(ds, wd, dtype, f"{name} bwd", last, ld, f32_tol=2e-5, bf16_tol=1.2e-2)


@storage("softmax_rows_16")
def test_softmax_rows_16(cuda, d):
    _softmax_case("softmax_rows_16", d)


@storage("softmax_rows_64x2")
def test_softmax_rows_64x2(cuda, d):
    _softmax_case("softmax_rows_64x2", d)


@storage("softmax_rows_64x8")
def test_softmax_rows_64x8(cuda, d):
    _softmax_case("softmax_rows_64x8", d)


@storage("softmax_rows_64x32")
def test_softmax_rows_64x32(cuda, d):
    _softmax_case("softmax_rows_64x32", d, inplace=True)


# ======================================================================================================================================
# optim.hip, through the public optimizer classes
# ======================================================================================================================================
def _opt_params(name, seed):
    s = shape_of(name, "f32")
    sizes = GT.opt_variables(s["total"], s["big"], s["count"])
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, n in enumerate(sizes):
        p = torch.nn.Parameter(torch.randn(n, generator=g).cuda())
        p.iseg_name = f"v{i}/{'bias' if i % 2 else 'kernel'}"
        ps.append(p)
    ps[1].lr_multiplier = 10.0
    return s, sizes, ps


def _opt_grads(sizes, step, seed, nan):
    g = torch.Generator().manual_seed(1000 * seed + step)
    gs = [torch.randn(n, generator=g) * (3.0 if i == 0 else 0.3) * 1e-2 for i, n in enumerate(sizes)]
    if nan:
        gs[0][5] = NAN
        gs[-1][sizes[-1] - 1] = NAN      # the last element of the last variable: the ragged last trip
    return gs


def _seg_tail(store, nblocks_first):
    """(segment index, element offset inside it) of the first parameter the ragged last trip of the update kernel owns"""
    for i, (p, o, n) in enumerate(store.segments):
        if o + n > nblocks_first * 256:
            return i, max(0, nblocks_first * 256 - o)
    raise AssertionError("the last trip lies past the last variable")


@storage("adamw_clipnorm")
def test_adamw_clipnorm(cuda, d):
    from iseg_amd.optimizers.modern import AdamW
    from iseg_amd.param_store import ParamStore

    s, sizes, ps = _opt_params("adamw_clipnorm", 0)
    store = ParamStore(ps)
    trips = GT.BY_NAME["adamw_clipnorm"].launcher("f32", **s)
    assert store.nblocks == trips[0].items
    clip = dict(clipnorm=0.05)      # below every variable's gradient norm: each variable is scaled by its own factor
    opt = AdamW(learning_rate=1e-2, weight_decay=0.05, **clip)
    opt.exclude_from_weight_decay(var_names=["bias"])
    opt.build(store)
    w = [p.data.detach().cpu().double() for p in ps]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    seg, off = _seg_tail(store, GT.first_of_last_trip(trips[0]))
    for step in range(2):
        gs = _opt_grads(sizes, step, 3, nan=True)
        for p, g in zip(ps, gs):
            p.grad.copy_(g.cuda())
        opt.apply_gradients()
        gd = O.clip_gradients([O.scrub_nan(g.double()) for g in gs], **clip)
        for i, p in enumerate(ps):
            w[i], m[i], v[i] = O.adamw_step(w[i], gd[i], m[i], v[i], step + 1, 1e-2, float(getattr(p, "lr_multiplier", 1.0)), 0.0 if i % 2 else 0.05)
        for i, (p, o, n) in enumerate(store.segments):
            got = p.data.cpu().double()
            tol = 2e-6 + 2e-4 * 1e-2 * float(getattr(p, "lr_multiplier", 1.0))
            for where, sl in (("all trips", slice(None)),) + ((("last trip", slice(off, None)),) if i == seg else ()):
                assert torch.isfinite(got[sl]).all(), (step, i, where)
                err = (got[sl] - w[i][sl]).abs().max().item()
                assert err <= tol, f"step {step} variable {i} [{where}]: w err {err:.3e} > {tol:.3e}"
                assert (opt.m[o:o + n].cpu().double()[sl] - m[i][sl]).abs().max().item() <= 1e-6 * max(1.0, m[i].abs().max().item()), (step, i, where)
                assert (opt.v[o:o + n].cpu().double()[sl] - v[i][sl]).abs().max().item() <= 1e-6 * max(1.0, v[i].abs().max().item()), (step, i, where)
            assert torch.equal(p.iseg_compute.cpu(), p.data.cpu().to(torch.bfloat16)), f"step {step} variable {i}: the bf16 shadow is the rounded master"


@storage("sgd_global_clipnorm")
def test_sgd_global_clipnorm(cuda, d):
    from iseg_amd.optimizers.modern import SGD
    from iseg_amd.param_store import ParamStore

    s, sizes, ps = _opt_params("sgd_global_clipnorm", 1)
    ps[0].l2_regularizer = 1e-2
    store = ParamStore(ps)
    trips = GT.BY_NAME["sgd_global_clipnorm"].launcher("f32", **s)
    assert store.nblocks == trips[0].items
    clip = dict(global_clipnorm=0.5)      # below the global gradient norm
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, **clip)
    opt.build(store)
    w = [p.data.detach().cpu().double() for p in ps]
    m = [torch.zeros_like(x) for x in w]
    seg, off = _seg_tail(store, GT.first_of_last_trip(trips[0]))
    for step in range(2):
        gs = _opt_grads(sizes, step, 5, nan=False)
        for p, g in zip(ps, gs):
            p.grad.copy_(g.cuda())
        opt.apply_gradients()
        l2 = [float(getattr(p, "l2_regularizer", 0.0)) for p in ps]
        gd = O.clip_gradients([g.double() + 2.0 * l2[i] * w[i] for i, g in enumerate(gs)], **clip)
        for i, p in enumerate(ps):
            w[i], m[i] = O.sgd_step(w[i], gd[i], m[i], 0.05, float(getattr(p, "lr_multiplier", 1.0)), 0.9, 0.0, True)
        for i, (p, o, n) in enumerate(store.segments):
            got, gm = p.data.cpu().double(), opt.m[o:o + n].cpu().double()
            # every variable whole; then the parameters the ragged last trip of sgd_kernel owns, on their own: the tail of variable `seg` and
            # every variable behind it
            slices = (("all trips", slice(None)),) + ((("last trip", slice(off if i == seg else 0, None)),) if i >= seg else ())
            for where, sl in slices:
                assert torch.isfinite(got[sl]).all(), (step, i, where)
                err = (got[sl] - w[i][sl]).abs().max().item()
                assert err <= 3e-6 * max(1.0, w[i][sl].abs().max().item()), f"step {step} variable {i} [{where}]: w err {err:.3e}"
                err = (gm[sl] - m[i][sl]).abs().max().item()
                assert err <= 3e-6 * max(1.0, m[i][sl].abs().max().item()), f"step {step} variable {i} [{where}]: m err {err:.3e}"
            assert torch.equal(p.iseg_compute.cpu(), p.data.cpu().to(torch.bfloat16)), (step, i)


# ======================================================================================================================================
# eva.hip
# ======================================================================================================================================
@storage("qkv_rope")
def test_qkv_rope(cuda, d):
    """bias [q_bias | 0 | v_bias] and the rotary embedding on q, k of the tokens behind the prefix, in place on the packed rows"""
    k, dtype = K(), DT[d]
    s = shape_of("qkv_rope", d)
    B, Tn, prefix, C, hd = s["B"], s["tokens"], s["prefix"], s["C"], s["hd"]
    rows = B * Tn
    qkv, xr = q(rnd((rows, 3 * C), 1), dtype)
    qb, vb = (rnd((C,), 2) * 0.3).float(), (rnd((C,), 3) * 0.3).float()
    ang = rnd((Tn - prefix, hd // 2), 4).repeat_interleave(2, dim=1)      # every band twice, as the reference's table holds it
    emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).float()
    got = k.qkv_rope(qkv, qb.cuda(), vb.cuda(), emb.cuda(), Tn, prefix, C, hd)
    xr[:, :C] += qb.double()
    xr[:, 2 * C:] += vb.double()
    t = torch.arange(rows) % Tn
    e = emb.double()[(t - prefix).clamp(min=0)]
    sn, cs = e[:, None, :hd], e[:, None, hd:]
    for part in range(2):
        blk = xr[:, part * C:(part + 1) * C].reshape(rows, C // hd, hd)
        rot = torch.stack([-blk[..., 1::2], blk[..., 0::2]], dim=-1).reshape(rows, C // hd, hd)
        xr[:, part * C:(part + 1) * C] = torch.where((t >= prefix)[:, None, None], blk * cs + rot * sn, blk).reshape(rows, C)
    check(got, xr, dtype, "qkv_rope", last_of("qkv_rope", d), 8, f32_tol=1e-5, bf16_tol=2.0 ** -7)


@storage("glu_fwd_scalar")
def test_glu_fwd_scalar(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("glu_fwd_scalar", d)
    g, gr = q(rnd((s["rows"], s["cols"]), 1), dtype)
    x, xr = q(rnd((s["rows"], s["cols"]), 2), dtype)
    for act in (k.ACT_SWISH, k.ACT_GELU):
        with nan_outputs():
            y = k.glu_fwd(g, x, act)
        check(y, _act(gr, act, k) * xr, dtype, f"glu_fwd({act})", last_of("glu_fwd_scalar", d), f32_tol=2e-6, bf16_tol=1.2e-2)


@storage("glu_bwd_scalar")
def test_glu_bwd_scalar(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("glu_bwd_scalar", d)
    last = last_of("glu_bwd_scalar", d)
    g, gr = q(rnd((s["rows"], s["cols"]), 1), dtype)
    x, xr = q(rnd((s["rows"], s["cols"]), 2), dtype)
    do, dor = q(rnd((s["rows"], s["cols"]), 3), dtype)
    dg, dx = nan_like(g.shape, dtype), nan_like(g.shape, dtype)
    k.glu_bwd(do, g, x, dg, dx, k.ACT_SWISH)
    gg = gr.clone().requires_grad_(True)
    a = _act(gg, k.ACT_SWISH, k)
    a.backward(dor * xr)
    check(dg, gg.grad, dtype, "glu_bwd dgate", last, f32_tol=2e-6, bf16_tol=1.2e-2)
    check(dx, dor * a.detach(), dtype, "glu_bwd dx", last, f32_tol=2e-6, bf16_tol=1.2e-2)


# ======================================================================================================================================
# dcnv3.hip
# ======================================================================================================================================
def _mul_colsum_case(name, d):
    k, dtype = K(), DT[d]
    s = shape_of(name, d)
    rows, C = s["rows"], s["C"]
    a, ar = q(rnd((rows, C), 1), dtype)
    b, br = q(rnd((rows, C), 2), dtype)
    pre = rnd((C,), 3).float()

    def run(n):
        out = pre.clone().cuda()
        with nan_outputs():
            k.mul_colsum(a[:n], b[:n], out, accumulate=True)
        return out

    check_sum_with_last_trip(run, rows, last_of(name, d), ar * br, pre.double(), 1e-4 if d == "f32" else 1e-3, name)


# float32 np.sum error of the addends a * b (337 157 rows x 8 columns), measured: fp32 storage 7.8e-05, bf16 storage 8.4e-05
@storage("mul_colsum_vec")
def test_mul_colsum_vec(cuda, d):
    _mul_colsum_case("mul_colsum_vec", d)


# float32 np.sum error of the addends a * b (65 573 rows x 3 columns), measured: fp32 storage 5.9e-05, bf16 storage 5.0e-05
@storage("mul_colsum_scalar")
def test_mul_colsum_scalar(cuda, d):
    _mul_colsum_case("mul_colsum_scalar", d)


@storage("scale_cols_scalar")
def test_scale_cols_scalar(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("scale_cols_scalar", d)
    x, xr = q(rnd((s["rows"], s["C"]), 1), dtype)
    cs = (rnd((s["C"],), 2) * 0.5 + 1).float()
    with nan_outputs():
        y = k.scale_cols(x, cs.cuda())
    check(y, xr * cs.double(), dtype, "scale_cols", last_of("scale_cols_scalar", d))


@storage("split_cols_accumulate")
def test_split_cols_accumulate(cuda, d):
    k = K()
    s = shape_of("split_cols_accumulate", d)
    rows, n0, n1, ld = s["rows"], s["n0"], s["n1"], s["ld"]
    src = rnd((rows, ld), 1).float()
    d0, d1 = rnd((rows, n0), 2).float(), rnd((rows, n1), 3).float()
    g0, g1 = d0.clone().cuda(), d1.clone().cuda()
    k.split_cols_accumulate(src.cuda(), g0, n0, g1, n1)
    row = last_of("split_cols_accumulate", d) // (n0 + n1)      # items are (row, column of the n0 + n1): the last trip is the tail of the rows
    check(g0, d0.double() + src[:, :n0].double(), torch.float32, "split_cols_accumulate dst0", row, n0)
    check(g1, d1.double() + src[:, n0:n0 + n1].double(), torch.float32, "split_cols_accumulate dst1", row, n1)


@storage("dcn_mask_softmax_fwd")
def test_dcn_mask_softmax_fwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("dcn_mask_softmax_fwd", d)
    pixels, G, P, ld = s["pixels"], s["G"], s["P"], s["ld"]
    om, omr = q(rnd((pixels, ld), 1) * 2, dtype)
    k.dcn_mask_softmax_fwd(om, G, P)
    c0, c1 = 2 * G * P, 3 * G * P
    want = omr.clone()
    want[:, c0:c1] = torch.softmax(omr[:, c0:c1].reshape(pixels, G, P), -1).reshape(pixels, G * P)
    row = last_of("dcn_mask_softmax_fwd", d) // G
    check(om[:, c0:c1], want[:, c0:c1], dtype, "dcn_mask_softmax_fwd", row, G * P)
    got = om.cpu().double()
    assert torch.equal(got[:, :c0], omr[:, :c0]) and torch.equal(got[:, c1:], omr[:, c1:]), "offset and padding columns are not touched"


@storage("dcn_mask_softmax_bwd")
def test_dcn_mask_softmax_bwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("dcn_mask_softmax_bwd", d)
    pixels, G, P, ld = s["pixels"], s["G"], s["P"], s["ld"]
    c0, c1 = 2 * G * P, 3 * G * P
    om, omr = q(torch.rand((pixels, ld), generator=torch.Generator().manual_seed(1), dtype=torch.float64), dtype)      # any y serves the formula y (d - <y, d>)
    dom, domr = q(rnd((pixels, ld), 2), dtype)
    k.dcn_mask_softmax_bwd(om, dom, G, P)
    y, g = omr[:, c0:c1].reshape(pixels, G, P), domr[:, c0:c1].reshape(pixels, G, P)
    want = (y * (g - (y * g).sum(-1, keepdim=True))).reshape(pixels, G * P)
    row = last_of("dcn_mask_softmax_bwd", d) // G
    check(dom[:, c0:c1], want, dtype, "dcn_mask_softmax_bwd", row, G * P)
    got = dom.cpu().double()
    assert torch.equal(got[:, :c0], domr[:, :c0]), "the offset columns of the gradient are not touched"
    assert (got[:, c1:] == 0).all(), "the padding columns of the gradient come back zero, in every trip"


# ======================================================================================================================================
# loss.hip / mask_loss.hip
# ======================================================================================================================================
def _labels(shape, C, seed, ignore=255):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, shape, generator=g, dtype=torch.int32)
    y[torch.rand(shape, generator=g) < 0.1] = ignore
    return y


@storage("softmax_ce_confusion")
def test_softmax_ce_confusion(cuda, d):
    k = K()
    s = shape_of("softmax_ce_confusion", d)
    P, C = s["P"], s["C"]
    first_px = last_of("softmax_ce_confusion", d) * 256      # tiles of 256 pixels at C = 3
    z = (rnd((P, C), 1) * 3).float()
    y = _labels((P,), C, 5)
    zz = z.double().requires_grad_(True)
    lo = O.softmax_ce_ignore(y, zz, C, 255, None)
    scale = 0.37 / P
    (lo.sum() * scale).backward()
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    with nan_outputs():
        px, sm, dz = k.softmax_ce_ignore(z.cuda(), y.cuda(), 255, want_px=True, want_sum=True, sum_scale=1.0 / P, want_grad=True, grad_scale=scale, cm=cm)
    check(px, lo, torch.float32, "loss px", first_px, f32_tol=1e-5)
    check(dz, zz.grad, torch.float32, "dlogits", first_px, C, f32_tol=1e-5)
    assert abs(sm.item() - lo.mean().item()) <= 1e-5 * max(1.0, abs(lo.mean().item()))
    want_cm = O.confusion_matrix(y, O.argmax_first(z), C, 255)
    assert torch.equal(cm.cpu().reshape(C, C).double(), want_cm), "every workgroup flushes its histogram once, whatever the number of tiles it walked"


@storage("argmax_confusion")
def test_argmax_confusion(cuda, d):
    k = K()
    s = shape_of("argmax_confusion", d)
    P, C = s["P"], s["C"]
    z = rnd((P, C), 1).float()
    y = _labels((P,), C, 2)
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    with nan_outputs():
        pred = k.argmax_confusion(z.cuda(), y.cuda(), 255, cm=cm, want_pred=True)
    want = O.argmax_first(z)
    check(pred, want, torch.float32, "argmax", last_of("argmax_confusion", d) * 256, exact=True)
    assert torch.equal(cm.cpu().reshape(C, C).double(), O.confusion_matrix(y, want, C, 255))


@storage("upsample_ce_gather")
def test_upsample_ce_gather(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("upsample_ce_gather", d)
    N, Hi, Wi, C, f = s["N"], s["Hi"], s["Wi"], s["C"], s["s"]
    Ho, Wo = Hi * f, Wi * f
    assert k.upsample_ce_supported(Hi, Wi, Ho, Wo, C)
    z, zr = q(rnd((N, Hi, Wi, C), 1) * 2, dtype)
    y = _labels((N, Ho, Wo), C, 3)
    P = N * Ho * Wo
    with nan_outputs():
        sm, dz = k.upsample_ce(z, y.cuda(), Ho, Wo, 255, sum_scale=1.0 / P, grad_scale=1.0 / P)
    zz = zr.clone().requires_grad_(True)
    loss = O.softmax_ce_ignore(y, O.resize_bilinear(zz, (Ho, Wo)), C, 255).mean()
    loss.backward()
    assert abs(sm.item() - loss.item()) <= 2e-5 * max(1.0, abs(loss.item()))
    check(dz, zz.grad, dtype, "upsample_ce dz", last_of("upsample_ce_gather", d), f32_tol=2e-5, bf16_tol=1e-2)


@storage("mask_loss_px_dice")
def test_mask_loss_px_dice(cuda, d):
    """the per-pixel route of MaskLoss: the dice value of the image joins every valid pixel of it in a second, capped pass"""
    from tests import mask_loss_ref as MR

    k = K()
    s = shape_of("mask_loss_px_dice", d)
    B, H, W, C = s["B"], s["H"], s["W"], s["C"]
    z = (rnd((B, H, W, C), 1) * 4).clamp(-12, 12).float()
    y = _labels((B, H, W), C, 2)
    flags = k.MASKLOSS_SIGMOID | k.MASKLOSS_DICE | k.MASKLOSS_CE | k.MASKLOSS_FOCAL_SIGMOID
    with nan_outputs():
        px, _, _ = k.mask_loss(z.cuda().reshape(B, H * W, C), y.cuda().reshape(B, H * W), 255, flags, (20.0, 1.0, 1.0), want_px=True)
    want = MR.mask_loss(y, z.double(), reduction=True, num_class=C).reshape(-1)
    g, w = px.cpu().double(), want
    last = last_of("mask_loss_px_dice", d)
    for where, sl in (("all trips", slice(None)), (f"last trip, from pixel {last}", slice(last, None))):
        err = (g[sl] - w[sl]).abs().max().item()
        assert err <= 2e-5 * max(1.0, w[sl].abs().max().item()), f"mask_loss per pixel [{where}]: {err:.3e}"      # (the bound of test_mask_loss_gpu.py)


# ======================================================================================================================================
# gemm.hip:132
# ======================================================================================================================================
@storage("gemm_splitk_reduce")
def test_gemm_splitk_reduce(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("gemm_splitk_reduce", d)
    M, N, Kd, split = s["M"], s["N"], s["K"], s["split"]
    x, xr = q(rnd((M, Kd), 1), dtype)
    w, wr = q(rnd((Kd, N), 2) * Kd ** -0.5, dtype)
    b = rnd((N,), 3).float()
    out = nan_like((M, N), dtype)
    k.gemm(x, w, out, M, N, Kd, lda=Kd, ldb=N, ldd=N, a_kcontig=1, b_kcontig=0, bias=b.cuda(), split_k=split)      # (a bias: not the plain slab sum)
    check(out, xr @ wr + b.double(), dtype, "split-K reduce with an epilogue", last_of("gemm_splitk_reduce", d))


# ======================================================================================================================================
# grn.hip
# ======================================================================================================================================
def _grn_nx(gx):
    return gx / (gx.mean(-1, keepdim=True) + 1e-6)


# float32 np.sum error of the addends (2 x 337 157 rows x 8 columns), measured: sum x^2 fp32 storage 4.8e-02, bf16 9.1e-02 (on sums of 3.4e5);
# dgamma | dbeta fp32 6.4e-04, bf16 4.4e-04
@storage("grn_strips")
def test_grn_strips(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("grn_strips", d)
    N, HW, C = s["N"], s["HW"], s["C"]
    last = last_of("grn_strips", d)
    x, xr = q(rnd((N, HW, C), 1), dtype)
    dy, dyr = q(rnd((N, HW, C), 2), dtype)
    gamma, beta = (rnd((C,), 3) * 0.5).float(), (rnd((C,), 4) * 0.1).float()
    outs = {}

    def run_fwd(n):
        with nan_outputs():
            outs[n] = k.grn_fwd(x[:, :n].contiguous(), gamma.cuda(), beta.cuda(), 1e-6)
        return outs[n][2].double() ** 2      # gx^2 = sum_hw x^2 + eps, [N, C]

    check_sum_with_last_trip(run_fwd, HW, last, (xr * xr).permute(1, 0, 2).contiguous(), torch.full((N, C), 1e-6, dtype=torch.float64), 2e-5, "grn sum x^2")
    y, nx, gx = outs[HW]
    close(nx, _grn_nx(gx.cpu().double()), torch.float32, "grn nx from the launch's own gx", f32_tol=1e-5)
    nxd = nx.cpu().double()[:, None, :]
    check(y, gamma.double() * (xr * nxd) + beta.double() + xr, dtype, "grn y", last * C, f32_tol=2e-6, bf16_tol=1e-2)      # (element index inside sample 0)
    # backward: dgamma = sum dy x nx, dbeta = sum dy (nx, gx are inputs: the truncated call takes the full problem's)
    pre = rnd((2 * C,), 5).float()
    dxs = {}

    def run_bwd(n):
        dg, db = pre[:C].clone().cuda(), pre[C:].clone().cuda()
        with nan_outputs():
            dxs[n] = k.grn_bwd(dy[:, :n].contiguous(), x[:, :n].contiguous(), gamma.cuda(), nx, gx, dg, db, 1e-6, accumulate=True)
        return torch.cat([dg, db])

    terms = torch.cat([(dyr * xr * nxd).sum(0), dyr.sum(0)], dim=1)      # [HW, 2 C], summed over the samples
    check_sum_with_last_trip(run_bwd, HW, last, terms, pre.double(), 2e-5, "grn dgamma | dbeta")
    xx = xr.clone().requires_grad_(True)
    O.grn(xx.reshape(N, HW, 1, C), gamma.double(), beta.double(), 1e-6).backward(dyr.reshape(N, HW, 1, C))
    check(dxs[HW], xx.grad, dtype, "grn dx", last * C, f32_tol=1e-5, bf16_tol=1e-2)


@storage("grn_apply_fwd")
def test_grn_apply_fwd(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("grn_apply_fwd", d)
    N, HW, C = s["N"], s["HW"], s["C"]
    x, xr = q(rnd((N, HW, C), 1), dtype)
    gamma, beta = (rnd((C,), 3) * 0.5).float(), (rnd((C,), 4) * 0.1).float()
    with nan_outputs():
        y, nx, gx = k.grn_fwd(x, gamma.cuda(), beta.cuda(), 1e-6)
    gxr = torch.sqrt((xr * xr).sum(1) + 1e-6)
    close(gx, gxr, torch.float32, "grn gx", f32_tol=1e-5)
    close(nx, _grn_nx(gxr), torch.float32, "grn nx", f32_tol=1e-5)
    want = gamma.double() * (xr * nx.cpu().double()[:, None, :]) + beta.double() + xr
    check(y, want, dtype, "grn y", last_of("grn_apply_fwd", d, 1), 8, f32_tol=2e-6, bf16_tol=1e-2)


@storage("grn_fold_weights")
def test_grn_fold_weights(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("grn_fold_weights", d)
    N, Cout, C4 = s["N"], s["Cout"], s["C4"]
    wt, wtr = q(rnd((Cout, C4), 1), dtype)
    gamma = (rnd((C4,), 2) * 0.5).float()
    nx = (rnd((N, C4), 3).abs() + 0.5).float()
    with nan_outputs():
        out = k.grn_fold_weights(wt, gamma.cuda(), nx.cuda())
    want = wtr[None] * (gamma.double() * nx.double() + 1.0)[:, None, :]
    check(out, want, dtype, "grn_fold_weights", last_of("grn_fold_weights", d), 8)


# ======================================================================================================================================
# dwconv.hip / dwconv_strided.hip
# ======================================================================================================================================
@storage("dwconv_fwd_tiles")
def test_dwconv_fwd_tiles(cuda, d):
    """the tile-strided depthwise kernel (the route of dilations whose halo does not fit the LDS-tile kernel): forward with a bias, and the data
    gradient form (flipped taps)"""
    k, dtype = K(), DT[d]
    s = shape_of("dwconv_fwd_tiles", d)
    N, H, W, C, Kk, dil = (s[x] for x in ("N", "H", "W", "C", "K", "dil"))
    last = last_of("dwconv_fwd_tiles", d)
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    w = (rnd((Kk, Kk, C, 1), 2) / Kk).float()
    b = (rnd((C,), 3) * 0.1).float()
    pad = (Kk - 1) * dil // 2
    with nan_outputs():
        y = k.dwconv2d(x, w.reshape(Kk * Kk, C).cuda(), b.cuda(), Kk, dil, pad, pad)
    per_tile = H * W * C * N // GT.BY_NAME["dwconv_fwd_tiles"].launcher(d, **s)[0].items      # one tile per image row at W <= 4
    check(y, O.depthwise_conv2d(xr, w.double(), b.double(), 1, dil), dtype, "dw fwd", last, per_tile)
    with nan_outputs():
        dx = k.dwconv2d(x, w.reshape(Kk * Kk, C).cuda(), None, Kk, dil, (Kk - 1) * dil - pad, (Kk - 1) * dil - pad, flip=True)
    wf = w.reshape(Kk * Kk, C).flip(0).reshape(Kk, Kk, C, 1)
    check(dx, O.depthwise_conv2d(xr, wf.double(), None, 1, dil), dtype, "dw data gradient (flip)", last, per_tile)


@storage("dwconv_strided_bwd_weight")
def test_dwconv_strided_bwd_weight(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("dwconv_strided_bwd_weight", d)
    N, H, W, C, Kk, st = (s[x] for x in ("N", "H", "W", "C", "K", "s"))
    last = last_of("dwconv_strided_bwd_weight", d)
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    w = (rnd((Kk, Kk, C, 1), 2) / Kk)
    Ho, Wo = -(-H // st), -(-W // st)
    dy, dyr = q(rnd((N, Ho, Wo, C), 3), dtype)
    tail = (torch.arange(N * Ho * Wo) >= last).reshape(N, Ho, Wo, 1)      # the pixels of the ragged last trip
    pre_w, pre_b = rnd((Kk * Kk, C), 4).float(), rnd((C,), 5).float()
    tol = 2 * (1e-5 if d == "f32" else 2e-2)      # (test_strided_depthwise_conv_matches_oracle)
    for what, dyd, dyq in (("all trips", dy, dyr), ("last trip alone: the gradient rows before it zeroed", dy * tail.cuda(), dyr * tail)):
        dw, db = pre_w.clone().cuda(), pre_b.clone().cuda()
        with nan_outputs():
            k.dwconv2d_strided_bwd_weight(x, dyd, dw, db, Kk, st, 1, accumulate=True)
        ww, bb = w.clone().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
        O.depthwise_conv2d(xr, ww, bb, st, 1, "same").backward(dyq)
        for got, want, p, nm in ((dw, ww.grad.reshape(Kk * Kk, C), pre_w, "dW"), (db, bb.grad, pre_b, "db")):
            err = (got.cpu().double() - p.double() - want).abs().max().item()
            bound = tol * max(want.abs().max().item(), 1e-8)
            assert err <= bound, f"strided depthwise {nm} [{what}]: {err:.3e} > {bound:.3e}"


# ======================================================================================================================================
# augment.hip / projective.hip
# ======================================================================================================================================
@storage("normalize_image")
def test_normalize_image(cuda, d):
    k = K()
    pixels = shape_of("normalize_image", d)["pixels"]
    x = (rnd((pixels, 3), 1) * 60 + 120).float()
    a, b = [1 / 58.0, 1 / 57.0, 1 / 57.5], [-2.1, -2.0, -1.8]
    with nan_outputs():
        y = k.normalize_image(x.cuda(), a, b)
    want = x.double() * torch.tensor(a, dtype=torch.float32).double() + torch.tensor(b, dtype=torch.float32).double()
    check(y, want, torch.float32, "normalize_image", last_of("normalize_image", d))


@storage("augment_crop")
def test_augment_crop(cuda, d):
    from tests.test_input_pipeline_gpu import _reference

    k = K()
    s = shape_of("augment_crop", d)
    B, Hs, Ws, ch, cw = s["B"], s["Hs"], s["Ws"], s["ch"], s["cw"]
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (B, Hs, Ws, 3)).astype(np.float32)
    labs = rng.integers(0, 21, (B, Hs, Ws)).astype(np.int32)
    params = np.zeros((B, k.augment_params_ints()), dtype=np.int32)
    params[0, :8] = [Hs, Ws, 2 * Hs, 2 * Ws, 5, 9, 0, 0]                      # x2, cropped inside the scaled image
    params[1, :8] = [Hs - 30, Ws - 11, 2 * Hs - 60, 2 * Ws - 22, 0, 0, 1, 0]    # smaller than the crop: padded with the mean pixel, then flipped
    mean, scale, shift = [123.0, 117.0, 104.0], [1 / 58.0, 1 / 57.0, 1 / 57.5], [-2.1, -2.0, -1.8]
    with nan_outputs():
        out, lab = k.augment_crop_batch(torch.from_numpy(imgs).cuda(), torch.from_numpy(labs).cuda(), torch.from_numpy(params).cuda(), mean, scale, shift,
                                        255, ch, cw, 7)
    want, want_lab = [], []
    for b in range(B):
        xr, yr, _ = _reference(imgs[b], labs[b], params[b], mean, 255, ch, cw, scale, shift)
        want.append(xr)
        want_lab.append(yr)
    want, want_lab = torch.stack(want), torch.stack(want_lab)
    last = last_of("augment_crop", d)
    check(lab, want_lab, torch.float32, "augment_crop labels", last, exact=True)
    g, w = out.cpu().double().reshape(-1), want.reshape(-1)
    assert not torch.isnan(g).any()
    for where, sl in (("all trips", slice(None)), (f"last trip, from pixel {last}", slice(3 * last, None))):
        err = (g[sl] - w[sl]).abs().max().item()
        assert err <= 2e-4 * max(1.0, w[sl].abs().max().item()), f"augment_crop [{where}]: {err:.3e}"      # (the bound of test_input_pipeline_gpu.py)


# float32 np.sum error of the pixel sums (190 x 181 integer pixels x 3 channels), measured: 0 (every partial sum is an integer below 2^24)
@storage("augment_channel_means")
def test_augment_channel_means(cuda, d):
    k = K()
    s = shape_of("augment_channel_means", d)
    B, H, W = s["B"], s["H"], s["W"]
    last = last_of("augment_channel_means", d)
    imgs = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (B, H, W, 3)).astype(np.float32))
    params = np.zeros((B, k.augment_params_ints()), dtype=np.int32)
    params[:, :4] = [H, W, H, W]      # identity scale: the scaled pixel is the source pixel, the mean is the plain mean
    tailmask = (torch.arange(H * W) >= last).reshape(1, H, W, 1)
    for what, im in (("all trips", imgs), ("last trip alone: the pixels before it zeroed", imgs * tailmask)):
        fp = torch.full((B, k.augment_params_floats()), NAN)
        fp[:, 0], fp[:, 1] = 0.0, 1.5
        fpd = fp.cuda()
        with nan_outputs():
            k.augment_channel_means(im.cuda(), torch.from_numpy(params).cuda(), fpd)
        terms = im.double().reshape(B, H * W, 3).permute(1, 0, 2).contiguous()
        want = terms.sum(0)
        tol, f32_err = reduction_tol(terms, want, 1e-5)
        print(f"augment_channel_means [{what}]: float32 np.sum error {f32_err:.3e}")
        check_sum(fpd[:, 2:5].cpu().double() * (H * W), want, tol + 1e-6 * float(want.abs().max()), f"augment_channel_means [{what}]")      # (+ the fp32 division by H W)


@storage("projective_tiles")
def test_projective_tiles(cuda, d):
    """a pure translation by (2.25, -3.25): the bilinear taps and the nearest label of every output pixel are plain shifts of the source"""
    k = K()
    s = shape_of("projective_tiles", d)
    B, Hs, Ws, C = s["B"], s["Hs"], s["Ws"], s["C"]
    img = rnd((B, Hs, Ws, C), 1).float()
    lab = torch.randint(0, 21, (B, Hs, Ws), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    sizes = torch.tensor([[Hs, Ws], [Hs - 50, Ws - 9]], dtype=torch.int32)
    tf = torch.tensor([[1, 0, 2.25, 0, 1, -3.25, 0, 0]] * B, dtype=torch.float32)
    fill, lfill = 0.5, 255
    with nan_outputs():
        out, olab = k.projective_transform_batch(img.cuda(), lab.cuda(), tf.cuda(), sizes=sizes.cuda(), interpolation="bilinear", image_fill=fill, label_fill=lfill)
    want = torch.full((B, Hs, Ws, C), fill, dtype=torch.float64)
    wlab = torch.full((B, Hs, Ws), lfill, dtype=torch.int32)
    for b in range(B):
        H, W = int(sizes[b, 0]), int(sizes[b, 1])
        P = torch.full((H + 8, W + 8, C), fill, dtype=torch.float64)
        P[4:4 + H, 4:4 + W] = img[b, :H, :W].double()
        L = torch.full((H + 8, W + 8), lfill, dtype=torch.int32)
        L[4:4 + H, 4:4 + W] = lab[b, :H, :W]

        def tap(src, oy, ox):      # src[y + oy, x + ox] for every output pixel of the sample, the fill outside it
            return src[4 + oy:4 + oy + H, 4 + ox:4 + ox + W]

        top = 0.75 * tap(P, -4, 2) + 0.25 * tap(P, -4, 3)      # floor(x + 2.25) = x + 2, weights 0.75 | 0.25; floor(y - 3.25) = y - 4, weights 0.25 | 0.75
        bot = 0.75 * tap(P, -3, 2) + 0.25 * tap(P, -3, 3)
        want[b, :H, :W] = 0.25 * top + 0.75 * bot
        wlab[b, :H, :W] = tap(L, -3, 2)                        # round(y - 3.25) = y - 3, round(x + 2.25) = x + 2
    t = GT.BY_NAME["projective_tiles"].launcher(d, **s)[0]
    tiles_x, tiles_y = -(-Ws // 32), -(-Hs // 8)
    first = GT.first_of_last_trip(t)
    bl, yl = first // (tiles_x * tiles_y), (first % (tiles_x * tiles_y)) // tiles_x * 8      # the tile row band in which the last trip starts
    last_px = (bl * Hs + yl) * Ws
    check(out, want, torch.float32, "projective image", last_px, C, f32_tol=2e-6)
    check(olab, wlab, torch.float32, "projective labels", last_px, exact=True)


# ======================================================================================================================================
# defattn.hip (and dcn_zero / dcn_unfix of dcn_fixed.h behind its backward)
# ======================================================================================================================================
@storage("defattn")
def test_defattn(cuda, d):
    """one head of four channels and one point per pixel (the narrowest form: the scalar forward, the 4-lane backward): the forward lanes, the
    backward's (pixel, head) items and the fixed-point read-out of dvalue each take two full trips and a ragged third.  With one point the
    attention weight is 1 and its gradient exactly 0."""
    from tests import deformable_mhsa_ref as DR

    k, dtype = K(), DT[d]
    s = shape_of("defattn", d)
    N, H, W, heads, P, Ch = (s[x] for x in ("N", "H", "W", "heads", "P", "Ch"))
    trips = GT.BY_NAME["defattn"].launcher(d, **s)
    v, vr = q(rnd((N, H, W, heads * Ch), 1), dtype)
    o, orr = q(rnd((N, H, W, heads * P * 2), 2) * 1.5, dtype)
    a, ar = q(rnd((N, H, W, heads * P), 3) * 1.5, dtype)
    do, dor = q(rnd((N, H, W, heads * Ch), 4), dtype)
    with nan_outputs():
        out = k.defattn_fwd(v, o, a, heads, P, 4.0)
    vv, oo, aa = (t.requires_grad_(True) for t in (vr, orr, ar))
    want = DR.core(vv, oo, aa, heads, P, 4.0, scrub=False)
    check(out, want, dtype, "defattn fwd", GT.first_of_last_trip(trips[0]), f32_tol=1e-5, bf16_tol=1.5e-2)
    want.backward(dor)
    with nan_outputs():
        dv, doff, da = k.defattn_bwd(v, o, a, do, heads, P, 4.0)
    item = GT.first_of_last_trip(trips[1])
    check(dv, vv.grad, dtype, "defattn dvalue", GT.first_of_last_trip(trips[2]), f32_tol=2e-5, bf16_tol=2e-2)
    check(da, aa.grad, dtype, "defattn dattn", item, P, f32_tol=2e-5, bf16_tol=2e-2)
    g, w = doff.cpu().double().reshape(-1), oo.grad.reshape(-1)
    assert not torch.isnan(g).any()
    for where, sl in (("all trips", slice(None)), (f"last trip, from item {item}", slice(item * 2 * P, None))):
        # (bf16 logits put some coordinates at a cell border, where floor() in fp32 and fp64 differ: relative L2, as test_deformable_mhsa_gpu.py)
        assert (g[sl] - w[sl]).norm().item() / w[sl].norm().item() < 5e-2, f"defattn doffset [{where}]"


# ======================================================================================================================================
# misc.hip: max-pool gradient, the two 16-byte passes
# ======================================================================================================================================
@storage("pool2d_bwd_max_vec")
def test_pool2d_bwd_max_vec(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("pool2d_bwd_max_vec", d)
    N, H, W, C, k_, st = (s[x] for x in ("N", "H", "W", "C", "k", "s"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    (Ho, pt), (Wo, pl) = k.same_pad(H, k_, st, 1), k.same_pad(W, k_, st, 1)
    dy, dyr = q(rnd((N, Ho, Wo, C), 2), dtype)
    with nan_outputs():
        dx = k.pool2d_bwd(x, dy, k_, k_, st, st, pt, pl, k.POOL_MAX)
    xx = xr.clone().requires_grad_(True)
    O.max_pool_same(xx, k_, st).backward(dyr)
    check(dx, xx.grad, dtype, "max pool bwd (arg-max pass + gather pass)", last_of("pool2d_bwd_max_vec", d), 8, f32_tol=1e-6, bf16_tol=1.2e-2)


# ======================================================================================================================================
# elementwise.hip: layer-scale bookkeeping
# ======================================================================================================================================
@storage("layerscale_grads")
def test_layerscale_grads(cuda, d):
    """dW2 = Z gamma, dgamma = sum_k W2 Z + b2 S, db2 = gamma S, from Z and S (64 strips of 4 rows) and from the split-K slabs of [Z ; S] (128
    strips of 16 rows); K = 4179 rows: sixteen / two full passes over the strips and a ragged one"""
    k = K()
    s = shape_of("layerscale_grads", d)
    Kd, Nd, ns = s["K"], s["N"], s["nslabs"]
    slabs = (rnd((ns, Kd + 1, Nd), 1) * 0.5).float()
    ZS = slabs.double().sum(0)
    W2, b2, gamma = rnd((Kd, Nd), 2).float(), rnd((Nd,), 3).float(), (rnd((Nd,), 4) * 0.5 + 1).float()
    pre = [rnd((Kd, Nd), 5).float(), rnd((Nd,), 6).float(), rnd((Nd,), 7).float()]
    trips = GT.BY_NAME["layerscale_grads"].launcher(d, **s)

    def want(zs):
        Z, S = zs[:Kd], zs[Kd]
        return Z * gamma.double(), (W2.double() * Z).sum(0) + b2.double() * S, gamma.double() * S

    for form, t in (("tensors", trips[0]), ("slabs", trips[1])):
        first = GT.first_of_last_trip(t)
        keep = (torch.arange(Kd + 1) >= first).double()[:, None]      # the rows of the ragged last pass (and S) alone
        for where, sl, scale in (("all trips", slabs, 1.0), ("last trip alone: the rows before it zeroed", slabs * keep.float(), keep)):
            dW, dg, db = (t_.clone().cuda() for t_ in pre)
            if form == "tensors":
                zs = sl.sum(0)      # (fp32, in slab order)
                k.layerscale_grads(zs[:Kd].contiguous().cuda(), W2.cuda(), b2.cuda(), gamma.cuda(), zs[Kd].contiguous().cuda(), dW, dg, db, accumulate=True)
                ref = want(zs.double())
            else:
                k.layerscale_grads_slabs(sl.contiguous().cuda(), ns, W2.cuda(), b2.cuda(), gamma.cuda(), dW, dg, db, accumulate=True)
                ref = want(ZS * scale)
            check(dW, pre[0].double() + ref[0], torch.float32, f"layerscale dW2 ({form}) [{where}]", first, Nd)
            close(dg, pre[1].double() + ref[1], torch.float32, f"layerscale dgamma ({form}) [{where}]", f32_tol=1e-4)
            close(db, pre[2].double() + ref[2], torch.float32, f"layerscale db2 ({form}) [{where}]", f32_tol=1e-5)


# ======================================================================================================================================
# winattn.hip:356
# ======================================================================================================================================
@storage("win_bias_table")
def test_win_bias_table(cuda, d):
    k = K()
    s = shape_of("win_bias_table", d)
    nW, heads, T = s["nW"], s["heads"], s["T"]
    bias, mask = rnd((heads, T, T), 1).float(), torch.where(rnd((nW, T, T), 2) > 1.0, -100.0, 0.0).float()
    with nan_outputs():
        tab = k.window_attention_table(bias.cuda(), mask.cuda(), heads, T)
    want = torch.full((nW, heads, 64, 64), -3.4028234663852886e38, dtype=torch.float64)      # -FLT_MAX outside T x T
    want[:, :, :T, :T] = bias.double()[None] + mask.double()[:, None]
    inside = torch.zeros((nW, heads, 64, 64), dtype=torch.bool)
    inside[:, :, :T, :T] = True
    g = tab.cpu().double()
    assert not torch.isnan(g).any(), "table entries never written"
    last = last_of("win_bias_table", d)
    for where, sl in (("all trips", slice(None)), (f"last trip, from entry {last}", slice(last, None))):
        gi, wi, m = g.reshape(-1)[sl], want.reshape(-1)[sl], inside.reshape(-1)[sl]
        assert torch.equal(gi[~m], wi[~m]), f"win_bias_table [{where}]: outside T x T"
        close(gi[m], wi[m], torch.float32, f"win_bias_table [{where}]", f32_tol=1e-6)


# ======================================================================================================================================
# dwconv.hip: persistent kernels
# ======================================================================================================================================
@storage("dwconv_fwd_dma_rounds")
def test_dwconv_fwd_dma_rounds(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("dwconv_fwd_dma_rounds", d)
    N, H, W, C = (s[x] for x in ("N", "H", "W", "C"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    w = (rnd((7, 7, C, 1), 2) / 7).float()
    b = (rnd((C,), 3) * 0.1).float()
    with nan_outputs():
        y = k.dwconv2d(x, w.reshape(49, C).cuda(), b.cuda(), 7, 1, 3, 3)
    unit = last_of("dwconv_fwd_dma_rounds", d)                   # units are (row band of 8, column band of 32), one channel slab at C = 32
    first_row = unit // -(-W // 32) * 8
    check(y, O.depthwise_conv2d(xr, w.double(), b.double(), 1, 1), dtype, "dw 7x7 fwd (persistent DMA kernel)", first_row * W * C)


@storage("dwconv_bwd_weight_lds")
def test_dwconv_bwd_weight_lds(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("dwconv_bwd_weight_lds", d)
    N, H, W, C = (s[x] for x in ("N", "H", "W", "C"))
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    dy, dyr = q(rnd((N, H, W, C), 2), dtype)
    tile = last_of("dwconv_bwd_weight_lds", d)                   # tiles are (sample, column band of 32) at H <= 36
    tw = -(-W // 32)
    tail = torch.zeros((N, 1, W, 1), dtype=torch.bool)
    tail[tile // tw, :, tile % tw * 32:] = True
    tail[tile // tw + 1:] = True
    pre_w, pre_b = rnd((49, C), 4).float(), rnd((C,), 5).float()
    for what, dyd, dyq in (("all trips", dy, dyr), ("last trip alone: the gradient before it zeroed", dy * tail.cuda(), dyr * tail)):
        dw, db = pre_w.clone().cuda(), pre_b.clone().cuda()
        with nan_outputs():
            k.dwconv2d_bwd_weight(x, dyd, dw, db, 7, 1, 3, 3, accumulate=True)
        ww = torch.zeros((7, 7, C, 1), dtype=torch.float64, requires_grad=True)
        bb = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        O.depthwise_conv2d(xr, ww, bb, 1, 1).backward(dyq)
        close(dw - pre_w.cuda(), ww.grad.reshape(49, C), torch.float32, f"dw dW [{what}]", f32_tol=1e-4)      # (test_dwconv_fwd_bwd's tolerance)
        close(db - pre_b.cuda(), bb.grad, torch.float32, f"dw db [{what}]", f32_tol=1e-4)


# ======================================================================================================================================
# Swin's window partition / reverse with the index tables the backbone builds
# ======================================================================================================================================
def _swin_tables(s):
    from iseg_amd import nn
    from iseg_amd.backbones.swin import window_index_tables

    nn.set_device("cuda:0")
    return window_index_tables(s["N"], s["H"], s["W"], s["ws"], s["shift"])


def _partition_ref(xr, ws, shift):
    """backbones/swin.py:246-262: zero-pad to a multiple of the window, roll by -shift, cut into windows"""
    N, H, W, C = xr.shape
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    xp = torch.zeros((N, Hp, Wp, C), dtype=xr.dtype)
    xp[:, :H, :W] = xr
    xp = torch.roll(xp, (-shift, -shift), (1, 2))
    return xp.reshape(N, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


@storage("window_partition")
def test_window_partition(cuda, d):
    k, dtype = K(), DT[d]
    s = shape_of("window_partition", d)
    N, H, W, ws, shift, C = (s[x] for x in ("N", "H", "W", "ws", "shift", "C"))
    part, _, Hp, Wp = _swin_tables(s)
    x, xr = q(rnd((N, H, W, C), 1), dtype)
    with nan_outputs():
        y = k.gather_rows(x.reshape(-1, C), part, N * Hp * Wp)
    t = GT.BY_NAME["window_partition"].launcher(d, **s)[0]
    check(y, _partition_ref(xr, ws, shift), dtype, "window partition", GT.first_of_last_trip(t), N * Hp * Wp * C // t.items, exact=True)


@storage("window_reverse")
def test_window_reverse(cuda, d):
    """window reverse + roll back + crop + drop path + skip connection: out[m] = res[m] + f[sample of m] * windows[reverse[m]]"""
    k, dtype = K(), DT[d]
    s = shape_of("window_reverse", d)
    N, H, W, ws, shift, C = (s[x] for x in ("N", "H", "W", "ws", "shift", "C"))
    _, rev, Hp, Wp = _swin_tables(s)
    wnd, wr = q(rnd((N * Hp * Wp, C), 1), dtype)
    res, resr = q(rnd((N * H * W, C), 2), dtype) if d == "bf16" else (None, 0.0)      # (fp32 storage: no room for the residual)
    f = torch.tensor([1.25] * N, dtype=torch.float32)
    with nan_outputs():
        out = k.gather_rows_fma(wnd, rev, f.cuda(), H * W, False, res)
    back = wr.reshape(N, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, C)
    back = torch.roll(back, (shift, shift), (1, 2))[:, :H, :W].reshape(-1, C)
    check(out, resr + 1.25 * back, dtype, "window reverse", last_of("window_reverse", d), 8)


# ======================================================================================================================================
# sod_metrics.hip:54
# ======================================================================================================================================
@storage("sod_minmax")
def test_sod_minmax(cuda, d):
    """normalize=True: the minimum and the maximum of the uint8 prediction, found by two workgroups in ten passes, exist only among the pixels
    of the ragged last pass; the MAE of the normalised image shows whether they were found"""
    from tests import sod_metrics_ref as SR

    k = K()
    s = shape_of("sod_minmax", d)
    B, H, W = s["B"], s["H"], s["W"]
    last = last_of("sod_minmax", d)
    rng = np.random.default_rng(3)
    pred = rng.integers(40, 201, (B, H * W)).astype(np.uint8)
    pred[:, last + 300], pred[:, H * W - 2] = 3, 250
    pred = pred.reshape(B, H, W)
    gt = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    state = torch.zeros(k.SOD_STATE_DOUBLES, dtype=torch.float64, device=cuda)
    count = torch.zeros(1, dtype=torch.int64, device=cuda)
    _, per, _, _ = k.sod_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), normalize=True, wfm=False, state=state, count=count,
                                 want_per_image=True)
    for b in range(B):
        p, g = SR.prepare_data(pred[b], gt[b])
        assert float(p.min()) == 0.0 and float(p.max()) == 1.0
        mae = float(np.mean(np.abs(p.astype(np.float64) - g.astype(np.float64))))
        assert abs(per[b, 0].item() - mae) <= 1e-6, (b, per[b, 0].item(), mae)
