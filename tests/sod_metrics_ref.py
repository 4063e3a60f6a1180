"""fp64 restatement of the reference's SOD metrics (metrics/sod/sod_metrics.py on metrics/sod/sod_metric_utils.py), NumPy only.

Everything is fp64 except what the reference's fp32 decides discretely, which is kept in fp32 so that the integers agree with the kernels:
the histogram bin int(p * 255.0) is an np.float32 product (sod_metrics.py:611, :863), the adaptive threshold is min(2 mean, 1) with the mean
formed in fp64 and then rounded to fp32 and compared in fp32 (sod_metric_utils.py:98-109), and prepare_data's mapminmax runs in fp32 in the
reference's operation order (sod_metric_utils.py:82-95).

Where the reference's formula is not finite (a centroid quadrant of N <= 1 pixels, sod_metrics.py:389-391 divides by N - 1): a quadrant
without pixels contributes nothing (its weight is 0), and a single pixel has variances 0, so the ladder of _ssim gives 1.

Distance transform: exact integer squared distances, the smallest row-major index among equidistant foreground pixels.
"""
import numpy as np

EPS = 2.220446049250313e-16      # sod_metric_utils.py:13


def prepare_data(pred_u8, gt_u8):
    """sod_metric_utils.py:67-95"""
    gt = gt_u8 > 128
    pred = pred_u8.astype(np.float32) / np.float32(255.0)
    mx, mn = pred.max(), pred.min()
    if mx != mn:
        pred = (pred - mn) / (mx - mn)
    assert pred.dtype == np.float32
    return pred, gt


def adaptive_threshold(pred):
    """sod_metric_utils.py:98-109; fp32 value"""
    return np.float32(min(2.0 * float(pred.astype(np.float64).mean()), 1.0))


def histograms(pred, gt):
    """sod_metrics.py:611-627: (fg, bg) histograms [256] of int(pred * 255.0), the product in fp32"""
    bins = (pred.astype(np.float32) * np.float32(255.0)).astype(np.int32)
    return (np.bincount(bins[gt], minlength=256).astype(np.int64), np.bincount(bins[~gt], minlength=256).astype(np.int64))


def mae(pred, gt):
    """sod_metrics.py:157-168"""
    return float(np.abs(pred.astype(np.float64) - gt.astype(np.float64)).mean())


# ---- S-measure (sod_metrics.py:244-415) ------------------------------------------------------------------------------------------------
def centroid(gt):
    """sod_metrics.py:328-350: (cy, cx), already + 1"""
    h, w = gt.shape
    if gt.sum() == 0:
        cy, cx = np.round(h / 2.0), np.round(w / 2.0)
    else:
        ys, xs = np.nonzero(gt)
        cy, cx = np.round(ys.astype(np.float64).mean()), np.round(xs.astype(np.float64).mean())      # half to even, as tf.round
    return int(cy) + 1, int(cx) + 1


def _s_object(x):
    m, s = x.mean(), x.std()
    return 2.0 * m / (m * m + 1.0 + s + EPS)


def ssim(pred, gt):
    """sod_metrics.py:373-415 on one quadrant (fp64 arrays); the N <= 1 rule of the module docstring"""
    N = pred.size
    if N == 0:
        return 0.0
    x, y = pred.mean(), gt.mean()
    if N == 1:
        sx = sy = sxy = 0.0
    else:
        sx = ((pred - x) ** 2).sum() / (N - 1.0)
        sy = ((gt - y) ** 2).sum() / (N - 1.0)
        sxy = ((pred - x) * (gt - y)).sum() / (N - 1.0)
    alpha = 4.0 * x * y * sxy
    beta = (x * x + y * y) * (sx + sy)
    if alpha != 0.0:
        return alpha / (beta + EPS)
    return 1.0 if beta == 0.0 else 0.0


def s_measure(pred, gt, alpha=0.5):
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    y = g.mean()
    if y == 0.0:
        return 1.0 - p.mean()
    if y == 1.0:
        return p.mean()
    obj = _s_object(p[gt]) * y + _s_object(1.0 - p[~gt]) * (1.0 - y)
    h, w = gt.shape
    cy, cx = centroid(gt)
    area = float(h * w)
    w_lt = cy * cx / area
    w_rt = cy * (w - cx) / area
    w_lb = (h - cy) * cx / area
    w_rb = 1.0 - w_lt - w_rt - w_lb
    region = (ssim(p[:cy, :cx], g[:cy, :cx]) * w_lt + ssim(p[:cy, cx:], g[:cy, cx:]) * w_rt + ssim(p[cy:, :cx], g[cy:, :cx]) * w_lb +
              ssim(p[cy:, cx:], g[cy:, cx:]) * w_rb)
    return max(0.0, obj * alpha + region * (1.0 - alpha))


# ---- E-measure (sod_metrics.py:514-713) ------------------------------------------------------------------------------------------------
def _em(ff, fb, nfg, size):
    """ff, fb: prediction-foreground pixels on the gt foreground / background (scalars or arrays over the thresholds)"""
    ff, fb = np.asarray(ff, np.float64), np.asarray(fb, np.float64)
    pfg = ff + fb
    pbg = size - pfg
    if nfg == 0:
        s = pbg
    elif nfg == size:
        s = pfg
    else:
        bf = nfg - ff
        bb = pbg - bf
        mp, mg = pfg / size, nfg / size
        dp, dg = (1.0 - mp, 0.0 - mp), (1.0 - mg, 0.0 - mg)
        s = np.zeros_like(pfg)
        for part, (a, c) in zip((ff, fb, bf, bb), ((dp[0], dg[0]), (dp[0], dg[1]), (dp[1], dg[0]), (dp[1], dg[1]))):
            al = 2.0 * (a * c) / (a * a + c * c + EPS)
            s = s + ((al + 1.0) ** 2 / 4.0) * part
    return s / (size - 1.0 + EPS)


def adaptive_counts(pred, gt):
    """(count of p >= thr, count of p >= thr on the foreground), compared in fp32"""
    b = pred.astype(np.float32) >= adaptive_threshold(pred)
    return int(b.sum()), int((b & gt).sum())


def e_measure(pred, gt):
    """(adaptive, curve [256]); curve index i is threshold 255 - i"""
    fg, bg = histograms(pred, gt)
    nfg, size = float(gt.sum()), float(gt.size)
    curve = _em(np.cumsum(fg[::-1]), np.cumsum(bg[::-1]), nfg, size)
    nge, ngefg = adaptive_counts(pred, gt)
    return float(_em(ngefg, nge - ngefg, nfg, size)), curve


# ---- F-measure (sod_metrics.py:821-904) ------------------------------------------------------------------------------------------------
def f_measure(pred, gt, beta=0.3):
    """(adaptive, precision [257], recall [257], F [257]); index i is threshold 256 - i; beta multiplies as the reference writes it (not squared)"""
    fg, bg = histograms(pred, gt)
    fg = np.concatenate([fg, [0]]).astype(np.float64)      # 257 bins: bin 256 is empty for p <= 1
    bg = np.concatenate([bg, [0]]).astype(np.float64)
    TPs = np.cumsum(fg[::-1])
    Ps = TPs + np.cumsum(bg[::-1])
    T = max(float(gt.sum()), 1.0)
    prec = np.where(Ps == 0.0, 0.0, TPs / np.where(Ps == 0.0, 1.0, Ps))
    rec = TPs / T
    num = (1.0 + beta) * prec * rec
    den = np.where(num == 0.0, 1.0, beta * prec + rec)
    nge, ngefg = adaptive_counts(pred, gt)
    adp = 0.0
    if ngefg != 0:
        pre, r = ngefg / float(nge), ngefg / float(gt.sum())
        adp = (1.0 + beta) * pre * r / (beta * pre + r)
    return adp, prec, rec, num / den


# ---- weighted F-measure (sod_metrics.py:998-1053) --------------------------------------------------------------------------------------
def edt(fg):
    """(squared distance to the nearest True pixel [H,W] int64, its row-major index [H,W] int64); the smallest index among equidistant ones.
    Column scan, then a per-row minimum over the columns of dx^2 + g(x')^2 on the lexicographic key (distance, index)."""
    H, W = fg.shape
    assert fg.any()
    rows = np.arange(H)[:, None]
    up = np.maximum.accumulate(np.where(fg, rows, -1), axis=0)                              # nearest foreground row above (or here), -1: none
    dn = np.minimum.accumulate(np.where(fg, rows, 4 * H)[::-1], axis=0)[::-1]               # nearest below (or here), 4 H: none
    du = np.where(up >= 0, rows - up, 4 * H)
    dd = np.where(dn < 4 * H, dn - rows, 4 * H)
    ny = np.where(du <= dd, up, dn)                                                          # the upper one of two at the same distance
    has = (up >= 0) | (dn < 4 * H)
    assert H <= 16384 and W <= 16384
    M = np.int64(1) << 32                                                                    # key = squared distance * M + index
    g2 = np.where(has, np.minimum(du, dd).astype(np.int64) ** 2, 1 << 30)                    # 1 << 30: beyond every real squared distance
    idx = np.where(has, ny.astype(np.int64) * W + np.arange(W)[None, :], M - 1)
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                                                     # [x, x']
    d2 = np.empty((H, W), np.int64)
    nn = np.empty((H, W), np.int64)
    step = max(1, (1 << 22) // (W * W))
    for r0 in range(0, H, step):
        r1 = min(H, r0 + step)
        key = (dx2[None, :, :] + g2[r0:r1, None, :]) * M + idx[r0:r1, None, :]              # [rows, x, x']
        k = key.min(axis=2)
        d2[r0:r1] = k // M
        nn[r0:r1] = k % M
    return d2, nn


def gaussian7(sigma=5.0):
    """sod_metric_utils.py:201-229 (no entry falls under EPS * max)"""
    r = np.arange(-3, 4, dtype=np.float64)
    h = np.exp(-(r[None, :] ** 2 + r[:, None] ** 2) / (2 * sigma * sigma))
    return h / h.sum()


def convolve7(a, k):
    """scipy.ndimage.convolve(a, k, mode='constant', cval=0): a true convolution, out[y,x] = sum k[i,j] a[y - (i - 3), x - (j - 3)]"""
    H, W = a.shape
    pad = np.zeros((H + 6, W + 6))
    pad[3:-3, 3:-3] = a
    out = np.zeros((H, W))
    for i in range(7):
        for j in range(7):
            out += k[i, j] * pad[6 - i:6 - i + H, 6 - j:6 - j + W]
    return out


def weighted_f(pred, gt, beta=1.0, dist=None):
    """0 for an all-background gt (sod_metrics.py:986-993).  dist = (d2, nearest) replaces edt() (the SciPy cross-check passes SciPy's)"""
    if not gt.any():
        return 0.0
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    d2, nn = edt(gt) if dist is None else dist
    E = np.abs(p - g)
    Et = np.where(gt, E, E.reshape(-1)[nn])
    EA = convolve7(Et, gaussian7())
    MIN = np.where(gt & (EA < E), EA, E)
    Bw = np.where(gt, 1.0, 2.0 - np.exp(np.log(0.5) / 5.0 * np.sqrt(d2.astype(np.float64))))
    Ew = MIN * Bw
    TPw = g.sum() - Ew[gt].sum()
    FPw = Ew[~gt].sum()
    R = 1.0 - Ew[gt].mean()
    P = TPw / (TPw + FPw + EPS)
    return (1.0 + beta) * R * P / (R + beta * P + EPS)


def all_metrics(pred, gt, alpha=0.5, beta_fm=0.3, beta_wfm=1.0, wfm=True):
    """every per-image quantity the kernels produce, for one image (pred fp32 [H,W] in [0,1], gt bool [H,W])"""
    fg, bg = histograms(pred, gt)
    em_adp, em_curve = e_measure(pred, gt)
    fm_adp, prec, rec, fm_curve = f_measure(pred, gt, beta_fm)
    nge, ngefg = adaptive_counts(pred, gt)
    out = dict(hist_fg=fg, hist_bg=bg, nfg=int(gt.sum()), nge=nge, ngefg=ngefg, centroid=centroid(gt), thr=adaptive_threshold(pred),
               mae=mae(pred, gt), sm=s_measure(pred, gt, alpha), em_adp=em_adp, em_curve=em_curve, fm_adp=fm_adp, precision=prec, recall=rec,
               fm_curve=fm_curve)
    if wfm:
        dist = edt(gt) if gt.any() else None
        out["wfm"] = weighted_f(pred, gt, beta_wfm, dist=dist)
        out["dist"] = dist
    return out
