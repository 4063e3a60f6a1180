"""metrics/sod/sod_metric_utils.py of the reference: the constants and helpers the SOD metrics share (:12-13 EPS, :17-55
validate_and_normalize_input, :67-95 prepare_data, :98-109 get_adaptive_threshold, :138-152 safe_divide, :201-229 tf_gaussian_kernel), and
`composed_record`: the five metrics of one image built from tensor ops (bincount, masked sums, a separable distance transform).  The composed
route is what ISEG_SODMETRICS_FUSED=0 selects: the A/B partner and timing baseline of csrc/sod_metrics.hip, not a fallback.

The helpers of the reference that only TFHumanCorrectionEffortMeasure uses (morphology, skeleton, contours, RDP, Lab colour) are not here.
"""
import math

import torch

EPS = 2.220446049250313e-16      # np.spacing(1); an fp32 value too (2^-52)
STATE_DOUBLES = 1032
S_MAE, S_SM, S_EM_ADP, S_FM_ADP, S_WFM, S_EM, S_FM, S_PREC, S_REC = 0, 1, 2, 3, 4, 5, 261, 518, 775


def validate_and_normalize_input(pred, gt, normalize=True):
    """pred fp32 in [0, 1] and gt bool; with normalize, pred uint8 -> mapminmax(im2double) in fp32 and gt > 128"""
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError("Shape mismatch between prediction and ground truth")
    if normalize:
        return prepare_data(pred, gt)
    return pred.to(torch.float32), gt.to(torch.bool)


def prepare_data(pred, gt):
    """one image [H,W] or a batch [B,H,W] normalised image by image"""
    gt = gt > 128
    pred = pred.to(torch.float32)
    pred = pred / torch.full_like(pred, 255.0)      # a tensor divisor: a true fp32 division (a scalar divisor may become a multiplication by 1 / 255)
    flat = pred.reshape(-1, pred.shape[-2] * pred.shape[-1]) if pred.dim() == 3 else pred.reshape(1, -1)
    mx = flat.max(dim=1).values.reshape(-1, 1, 1) if pred.dim() == 3 else flat.max()
    mn = flat.min(dim=1).values.reshape(-1, 1, 1) if pred.dim() == 3 else flat.min()
    den = mx - mn
    pred = torch.where(den != 0, (pred - mn) / torch.where(den != 0, den, torch.ones_like(den)), pred)
    return pred, gt


def get_adaptive_threshold(matrix, max_value=1.0):
    """min(2 * mean, max_value) as an fp32 scalar; the mean is formed in fp64 and then rounded"""
    return torch.clamp(2.0 * matrix.to(torch.float64).mean(), max=max_value).to(torch.float32)


def safe_divide(numerator, denominator):
    denominator = denominator.to(torch.float32)
    numerator = numerator.to(torch.float32)
    return torch.where(denominator == 0.0, torch.zeros_like(numerator), numerator / torch.where(denominator == 0.0, torch.ones_like(denominator),
                                                                                                 denominator))


def gaussian_kernel(shape=(7, 7), sigma=5.0, dtype=torch.float64, device=None):
    """MATLAB's fspecial('gaussian', shape, sigma)"""
    m, n = (shape[0] - 1) / 2, (shape[1] - 1) / 2
    y = torch.arange(-m, m + 1, dtype=dtype, device=device)[:, None]
    x = torch.arange(-n, n + 1, dtype=dtype, device=device)[None, :]
    h = torch.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h = torch.where(h < EPS * h.max(), torch.zeros_like(h), h)
    s = h.sum()
    return h / s if float(s) != 0 else h


# ---------------------------------------------------------------------------------------------------------
# the composed route
# ---------------------------------------------------------------------------------------------------------
def _em(ff, fb, nfg, size):
    pfg = ff + fb
    pbg = size - pfg
    bf = nfg - ff
    bb = pbg - bf
    mp, mg = pfg / size, nfg / size
    dp, dg = (1.0 - mp, 0.0 - mp), (1.0 - mg, 0.0 - mg)
    s = torch.zeros_like(pfg)
    for part, (a, c) in zip((ff, fb, bf, bb), ((dp[0], dg[0]), (dp[0], dg[1]), (dp[1], dg[0]), (dp[1], dg[1]))):
        al = 2.0 * (a * c) / (a * a + c * c + EPS)
        s = s + ((al + 1.0) ** 2 / 4.0) * part
    s = torch.where(nfg == 0, pbg, torch.where(nfg == size, pfg, s))
    return s / (size - 1.0 + EPS)


def _ssim(p, g, m):
    """_ssim over the pixels of mask m; N == 0 contributes 0 and N == 1 has variances 0 (sod_metrics.SodMetricSet documents the rule)"""
    N = m.sum().to(torch.float64)
    Ns = torch.clamp(N, min=1.0)
    x = (p * m).sum() / Ns
    y = (g * m).sum() / Ns
    d = torch.clamp(N - 1.0, min=1.0)
    sx = (((p - x) ** 2) * m).sum() / d
    sy = (((g - y) ** 2) * m).sum() / d
    sxy = ((p - x) * (g - y) * m).sum() / d
    one = N <= 1.0
    sx, sy, sxy = (torch.where(one, torch.zeros_like(v), v) for v in (sx, sy, sxy))
    alpha = 4.0 * x * y * sxy
    beta = (x * x + y * y) * (sx + sy)
    score = torch.where(alpha != 0, alpha / (beta + EPS), torch.where(beta == 0, torch.ones_like(beta), torch.zeros_like(beta)))
    return torch.where(N == 0, torch.zeros_like(score), score)


def _s_object(x, m):
    n = torch.clamp(m.sum().to(torch.float64), min=1.0)
    mean = (x * m).sum() / n
    std = torch.sqrt((((x - mean) ** 2) * m).sum() / n)
    return 2.0 * mean / (mean * mean + 1.0 + std + EPS)


def distance_transform(fg):
    """(squared distance to the nearest True pixel, its row-major index), exact int64; the smallest index among equidistant pixels.
    Column scan (cummax / cummin), then a minimum over the columns of dx^2 + g(x')^2 on the key (distance, index), rows in chunks."""
    H, W = fg.shape
    dev = fg.device
    rows = torch.arange(H, device=dev)[:, None].expand(H, W)
    none = 4 * H
    up = torch.cummax(torch.where(fg, rows, torch.full_like(rows, -1)), dim=0).values
    dn = torch.flip(torch.cummin(torch.flip(torch.where(fg, rows, torch.full_like(rows, none)), [0]), dim=0).values, [0])
    du = torch.where(up >= 0, rows - up, torch.full_like(rows, none))
    dd = torch.where(dn < none, dn - rows, torch.full_like(rows, none))
    ny = torch.where(du <= dd, up, dn)
    has = (up >= 0) | (dn < none)
    M = 1 << 32
    g2 = torch.where(has, torch.minimum(du, dd) ** 2, torch.full_like(rows, 1 << 30))
    idx = torch.where(has, ny * W + torch.arange(W, device=dev)[None, :], torch.full_like(rows, M - 1))
    x = torch.arange(W, device=dev)
    dx2 = (x[:, None] - x[None, :]) ** 2
    d2 = torch.empty(H, W, dtype=torch.int64, device=dev)
    nn_ = torch.empty(H, W, dtype=torch.int64, device=dev)
    step = max(1, (1 << 23) // (W * W))
    for r0 in range(0, H, step):
        r1 = min(H, r0 + step)
        k = ((dx2[None] + g2[r0:r1, None, :]) * M + idx[r0:r1, None, :]).min(dim=2).values
        d2[r0:r1] = k // M
        nn_[r0:r1] = k % M
    return d2, nn_


def _weighted_f(p, gt, g, beta):
    d2, nn_ = distance_transform(gt)
    E = (p - g).abs()
    Et = torch.where(gt, E, E.reshape(-1)[nn_.clamp(max=E.numel() - 1)])
    K = gaussian_kernel(dtype=torch.float64, device=p.device)
    EA = torch.nn.functional.conv2d(Et[None, None], torch.flip(K, [0, 1])[None, None], padding=3)[0, 0]      # a true convolution
    MIN = torch.where(gt & (EA < E), EA, E)
    Bw = torch.where(gt, torch.ones_like(E), 2.0 - torch.exp(math.log(0.5) / 5.0 * torch.sqrt(d2.to(torch.float64))))
    Ew = MIN * Bw
    nfg = g.sum()
    efg = (Ew * g).sum()
    TPw = nfg - efg
    FPw = (Ew * (1.0 - g)).sum()
    R = 1.0 - efg / torch.clamp(nfg, min=1.0)
    P = TPw / (TPw + FPw + EPS)
    Q = (1.0 + beta) * R * P / (R + beta * P + EPS)
    return torch.where(nfg == 0, torch.zeros_like(Q), Q)


def composed_record(pred, gt, alpha=0.5, beta_fm=0.3, beta_wfm=1.0, wfm=True):
    """the per-image record [STATE_DOUBLES] fp64 (layout: include/iseg_hip.h) of one image, pred fp32 [H,W] in [0,1] and gt bool [H,W]"""
    H, W = pred.shape
    dev = pred.device
    p, g = pred.to(torch.float64), gt.to(torch.float64)
    size = float(H * W)
    nfg = g.sum()
    out = torch.zeros(STATE_DOUBLES, dtype=torch.float64, device=dev)
    out[S_MAE] = (p - g).abs().mean()
    # S-measure
    rows = torch.arange(H, device=dev, dtype=torch.float64)[:, None]
    cols = torch.arange(W, device=dev, dtype=torch.float64)[None, :]
    ns = torch.clamp(nfg, min=1.0)
    cy = torch.where(nfg == 0, torch.round(torch.tensor(H / 2.0, dtype=torch.float64, device=dev)), torch.round((rows * g).sum() / ns)) + 1
    cx = torch.where(nfg == 0, torch.round(torch.tensor(W / 2.0, dtype=torch.float64, device=dev)), torch.round((cols * g).sum() / ns)) + 1
    top, left = (rows < cy).to(torch.float64), (cols < cx).to(torch.float64)
    w_lt, w_rt, w_lb = cy * cx / size, cy * (W - cx) / size, (H - cy) * cx / size
    w_rb = 1.0 - w_lt - w_rt - w_lb
    region = (_ssim(p, g, top * left) * w_lt + _ssim(p, g, top * (1 - left)) * w_rt + _ssim(p, g, (1 - top) * left) * w_lb +
              _ssim(p, g, (1 - top) * (1 - left)) * w_rb)
    gm = nfg / size
    obj = _s_object(p, g) * gm + _s_object(1.0 - p, 1.0 - g) * (1.0 - gm)
    mixed = torch.clamp(obj * alpha + region * (1.0 - alpha), min=0.0)
    out[S_SM] = torch.where(nfg == 0, 1.0 - p.mean(), torch.where(nfg == size, p.mean(), mixed))
    # histograms, curves
    bins = (pred * 255.0).to(torch.int64).clamp(0, 255)
    fg_hist = torch.bincount(bins[gt], minlength=256).to(torch.float64)
    bg_hist = torch.bincount(bins[~gt], minlength=256).to(torch.float64)
    ff, fb = torch.cumsum(torch.flip(fg_hist, [0]), 0), torch.cumsum(torch.flip(bg_hist, [0]), 0)
    out[S_EM:S_EM + 256] = _em(ff, fb, nfg, size)
    Ps = ff + fb
    prec = torch.where(Ps == 0, torch.zeros_like(Ps), ff / torch.where(Ps == 0, torch.ones_like(Ps), Ps))
    rec = ff / torch.clamp(nfg, min=1.0)
    num = (1.0 + beta_fm) * prec * rec
    den = torch.where(num == 0, torch.ones_like(num), beta_fm * prec + rec)
    out[S_PREC + 1:S_PREC + 257] = prec
    out[S_REC + 1:S_REC + 257] = rec
    out[S_FM + 1:S_FM + 257] = num / den
    # adaptive E and F
    ge = pred >= get_adaptive_threshold(pred)
    nge, ngefg = ge.sum().to(torch.float64), (ge & gt).sum().to(torch.float64)
    out[S_EM_ADP] = _em(ngefg, nge - ngefg, nfg, size)
    pre, r = ngefg / torch.clamp(nge, min=1.0), ngefg / torch.clamp(nfg, min=1.0)
    fa = (1.0 + beta_fm) * pre * r / torch.where(ngefg == 0, torch.ones_like(pre), beta_fm * pre + r)
    out[S_FM_ADP] = torch.where(ngefg == 0, torch.zeros_like(fa), fa)
    if wfm:
        out[S_WFM] = _weighted_f(p, gt, g, beta_wfm)
    return out
