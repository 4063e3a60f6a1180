"""numpy restatement of TensorFlow's ImageProjectiveTransformV3 in CONSTANT fill mode, written from the op's semantics (the reference
reaches it through augments/random_rotate_augment.py:20-115), and of RandomRotateAugment's use of it (:221-296).

A transform row a0 a1 a2 b0 b1 b2 c0 c1 maps the OUTPUT (x, y) to the INPUT point:
    k = (c0 x + c1 y) + 1          k == 0 -> the fill value
    x' = ((a0 x + a1 y) + a2) / k  y' = ((b0 x + b1 y) + b2) / k
in float32, every operation rounded on its own, in this order -- the coordinates are the contract (a nearest-neighbour read flips at a
rounding boundary).  The interpolation itself runs in float64 here.
    nearest:  the pixel at (lround(y'), lround(x')), half away from zero; outside [0, H) x [0, W) the fill value
    bilinear: xf = floor(x'), xc = xf + 1 (rows alike); top = (xc - x') R(yf, xf) + (x' - xf) R(yf, xc), bot alike on row yc,
              out = (yc - y') top + (y' - yf) bot; R reads the fill value outside the image
Host tests (test_augments_host.py) check this file on answers that need no trigonometry."""
import numpy as np

F = np.float32


def source_coords(t, H, W):
    """(x', y', valid) for every output pixel of an H x W image: float32 [H, W] each, valid = (k != 0)"""
    t = np.asarray(t, dtype=F).reshape(8)
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        k = (t[6] * x + t[7] * y) + F(1)
        sx = ((t[0] * x + t[1] * y) + t[2]) / k
        sy = ((t[3] * x + t[4] * y) + t[5]) / k
    assert k.dtype == F and sx.dtype == F and sy.dtype == F
    valid = np.broadcast_to(k != 0, (H, W))
    return np.broadcast_to(sx, (H, W)), np.broadcast_to(sy, (H, W)), valid


def round_half_away(v):
    """std::round on float32 values, computed exactly in float64"""
    v = np.asarray(v, dtype=np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def _read(img, yy, xx, fill):
    """img [H, W, C] at float index arrays (integral values, possibly huge / inf / nan): fill outside [0, H) x [0, W)"""
    H, W = img.shape[:2]
    with np.errstate(invalid="ignore"):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    yi = np.where(inside, yy, 0).astype(np.int64)
    xi = np.where(inside, xx, 0).astype(np.int64)
    out = img[yi, xi].astype(np.float64)
    out[~inside] = fill
    return out


def projective_transform(img, t, interpolation="bilinear", fill=0.0):
    """img [H, W, C] (any dtype) -> float64 [H, W, C]"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    sx, sy, valid = source_coords(t, H, W)
    sx64, sy64 = sx.astype(np.float64), sy.astype(np.float64)
    if interpolation == "nearest":
        out = _read(img, round_half_away(sy64), round_half_away(sx64), fill)
    else:
        with np.errstate(invalid="ignore"):
            xf, yf = np.floor(sx64), np.floor(sy64)
            xc, yc = xf + 1, yf + 1
            wx0, wx1, wy0, wy1 = (xc - sx64)[..., None], (sx64 - xf)[..., None], (yc - sy64)[..., None], (sy64 - yf)[..., None]
            top = wx0 * _read(img, yf, xf, fill) + wx1 * _read(img, yf, xc, fill)
            bot = wx0 * _read(img, yc, xf, fill) + wx1 * _read(img, yc, xc, fill)
            out = wy0 * top + wy1 * bot
        # no tap inside the image (huge / non-finite coordinates included): the fill value itself
        with np.errstate(invalid="ignore"):
            none = ~(((xf >= 0) & (xf < W)) | ((xc >= 0) & (xc < W))) | ~(((yf >= 0) & (yf < H)) | ((yc >= 0) & (yc < H)))
        out[none] = fill
    out[~valid] = fill
    return out


def rotation_matrix(angle, H, W):
    """get_rotation_matrix (:118-167) for one image, float32"""
    a = F(angle)
    c, s = F(np.cos(a)), F(np.sin(a))
    h1, w1 = F(H) - F(1), F(W) - F(1)
    x_off = (w1 - (c * w1 - s * h1)) / F(2)
    y_off = (h1 - (s * w1 + c * h1)) / F(2)
    return np.array([c, -s, x_off, s, c, y_off, 0, 0], dtype=F)


def rotate_sample(img, lab, t, fill_color, ignore_label):
    """RandomRotateAugment's two transforms on one sample: (image before the replace step, image after it, label)"""
    raw = projective_transform(img, t, "bilinear", -1.0)
    out = np.where(raw < -1e-6, np.asarray(fill_color, dtype=np.float64).reshape(1, 1, -1), raw)
    rl = None
    if lab is not None:
        rl = projective_transform(np.asarray(lab)[:, :, None], t, "nearest", float(ignore_label))[:, :, 0].astype(np.int64)
    return raw, out, rl
