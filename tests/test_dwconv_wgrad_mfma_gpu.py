"""Depthwise 7 x 7 weight gradient on the matrix cores (csrc/dwconv_wgrad_mfma.hip) against an fp64 evaluation of
    dW[ky][kx][c] = sum_{n,r,q} Xp[n][r + ky][q + kx][c] dY[n][r][q][c]        db[c] = sum dY[n][r][q][c]
on the bf16-rounded operands (Xp: x zero-padded by pad_t rows above and pad_l columns to the left).  The VALU kernel iseg_dwconv2d_bwd_weight picks
at these shapes and the matrix-core kernel both form exact bf16 products and sum them in fp32; only the summation order differs, so the new kernel's
band is twice the error the VALU kernel shows against the same fp64 values on the same inputs.  That error is one figure per launch, the maximum over
dW and db: both are fp32 sums of the same N H W terms of the same magnitude, and db taken alone is a sum the VALU kernel often gets EXACTLY right
(bf16 terms, a few hundred of them: 0.0 against fp64 at 16 x 16 x 32 and 20 x 24 x 32) -- twice zero is no band for an fp32 sum in another order
(one rounding step, 9.5e-7, at 20 x 24 x 32)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (20, 24), (9, 9), (33, 17)]      # one tile; partial tiles on both axes; smaller than a tile; three tiles by two


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


@functools.lru_cache(maxsize=None)
def _case(H, W, C, pad_t, pad_l):
    """bf16 operands, the initial gradients of the accumulate case and the fp64 value of the formula (computed once per shape)"""
    N = 2
    x = _rnd((N, H, W, C), 1).to(torch.bfloat16)
    dy = _rnd((N, H, W, C), 2).to(torch.bfloat16)
    dw0 = _rnd((49, C), 3).float()
    db0 = _rnd((C,), 4).float()
    xp = torch.zeros((N, H + 6, W + 6, C), dtype=torch.float64)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x.double()
    dyd = dy.double()
    dw = torch.stack([(xp[:, ky:ky + H, kx:kx + W] * dyd).sum(dim=(0, 1, 2)) for ky in range(7) for kx in range(7)])
    return x, dy, dw0, db0, dw, dyd.sum(dim=(0, 1, 2))


def _run(fn, x, dy, dw0, db0, accumulate):
    dw, db = dw0.cuda().clone(), db0.cuda().clone()
    fn(x.cuda(), dy.cuda(), dw, db, accumulate)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def _check(H, W, C, accumulate, pad_t, pad_l):
    from iseg_amd import kernels as K

    x, dy, dw0, db0, rdw, rdb = _case(H, W, C, pad_t, pad_l)
    if accumulate:
        rdw, rdb = rdw + dw0.double(), rdb + db0.double()
    pdw, pdb = _run(lambda a, b, w, c, acc: K.dwconv2d_bwd_weight(a, b, w, c, 7, 1, pad_t, pad_l, accumulate=acc), x, dy, dw0, db0, accumulate)
    mdw, mdb = _run(lambda a, b, w, c, acc: K.dwconv2d7_bwd_weight_mfma(a, b, w, c, pad_t, pad_l, accumulate=acc), x, dy, dw0, db0, accumulate)
    e_pdw, e_pdb = (pdw.double() - rdw).abs().max().item(), (pdb.double() - rdb).abs().max().item()
    e_mdw, e_mdb = (mdw.double() - rdw).abs().max().item(), (mdb.double() - rdb).abs().max().item()
    print(f"wgrad {H}x{W}x{C} acc={int(accumulate)} pad=({pad_t},{pad_l}): max|dW| {rdw.abs().max().item():.3f} err VALU {e_pdw:.3e} MFMA {e_mdw:.3e}; "
          f"max|db| {rdb.abs().max().item():.3f} err VALU {e_pdb:.3e} MFMA {e_mdb:.3e}")
    assert torch.isfinite(mdw).all() and torch.isfinite(mdb).all()
    band = 2 * max(e_pdw, e_pdb)
    assert e_mdw <= band, (e_mdw, band)
    assert e_mdb <= band, (e_mdb, band)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("H,W", SHAPES)
def test_wgrad_mfma_matches_fp64(cuda, H, W, C, accumulate):
    _check(H, W, C, accumulate, 3, 3)      # the ConvNeXt block: "same" padding of a 7 x 7, 3 above / left (and 3 below / right)


@pytest.mark.parametrize("pad_t,pad_l", [(2, 4), (0, 6)])
def test_wgrad_mfma_pad_offsets(cuda, pad_t, pad_l):
    _check(20, 24, 32, False, pad_t, pad_l)      # the window origin is a pair of free offsets: rows and columns must not be confused


def test_wgrad_mfma_bit_reproducible(cuda):
    from iseg_amd import kernels as K

    x, dy, dw0, db0, _, _ = _case(33, 17, 64, 3, 3)
    run = lambda: _run(lambda a, b, w, c, acc: K.dwconv2d7_bwd_weight_mfma(a, b, w, c, 3, 3, accumulate=acc), x, dy, dw0, db0, False)
    (dw1, db1), (dw2, db2) = run(), run()
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db1.view(torch.int32), db2.view(torch.int32))


def test_wgrad_mfma_rejects_unsupported(cuda):
    from iseg_amd import _hip, kernels as K

    with pytest.raises(_hip.HipCallError):      # C % 32 != 0: an error, never a silent other route
        K.dwconv2d7_bwd_weight_mfma(torch.zeros(1, 8, 8, 24, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 8, 8, 24, dtype=torch.bfloat16, device="cuda"),
                                    torch.zeros(49, 24, device="cuda"), torch.zeros(24, device="cuda"))
