"""The packed kernels of csrc/flashattn.hip and the wide-value kernels of csrc/selfattn.hip run one attention core
(csrc/attn_tile.h): at dv = 64, on the same storage, the two must give the same bits wherever both compute the same expression."""
import pytest
import torch

pytestmark = pytest.mark.gpu


# a single token, an exact tile, a ragged second tile, a third tile
@pytest.mark.parametrize("B,heads,T", [(2, 1, 1), (2, 3, 64), (1, 2, 65), (2, 3, 130)])
def test_packed_and_single_head_kernels_agree_on_the_same_storage(cuda, B, heads, T):
    """out, lse and dV are bitwise equal.  dQ and dK read D = rowsum(dO o O), which the two row-dot kernels sum in different orders
    (one lane per row against eight lanes and a butterfly), so these two meet the two-route bound of test_attention_gpu.py."""
    from iseg_amd import kernels as K

    d = 64
    C = heads * d
    scale = d ** -0.5
    gen = torch.Generator().manual_seed(1000 * T + heads)
    qkv = torch.randn((B, T, 3 * C), generator=gen).to(cuda, torch.bfloat16)
    dout = torch.randn((B, T, C), generator=gen).to(cuda, torch.bfloat16)

    out, lse = K.attention_fwd_train(qkv, heads, scale)
    dqkv = K.attention_bwd(qkv, out, dout, lse, heads, scale)
    Tp = lse.numel() // (B * heads)
    lse = lse.view(B, heads, Tp)

    for h in range(heads):
        qh, kh, vh = (qkv[..., part * C + h * d:part * C + (h + 1) * d] for part in range(3))
        doh = dout[..., h * d:(h + 1) * d]
        for view, pitch in ((qh, 3 * C), (kh, 3 * C), (vh, 3 * C), (doh, C)):      # the very same storage, no copy
            taken, ld = K._pitched(view)
            assert taken.data_ptr() == view.data_ptr() and ld == pitch
        oh, lh = K.self_attention_fwd(qh, kh, vh, scale, True)
        dq, dk, dv = K.self_attention_bwd(qh, kh, vh, oh, doh, lh, scale)
        torch.cuda.synchronize()
        assert torch.equal(oh, out[..., h * d:(h + 1) * d]), h
        assert torch.equal(lh.view(B, Tp), lse[:, h]), h
        assert torch.equal(dv, dqkv[..., 2 * C + h * d:2 * C + (h + 1) * d]), h
        for name, got, part, other in (("dq", dq, 0, kh), ("dk", dk, 1, qh)):
            ref = dqkv[..., part * C + h * d:part * C + (h + 1) * d].float()
            diff, bound = (got.float() - ref).abs().max().item(), 4e-2 * ref.abs().max().item()
            print(f"B={B} heads={heads} T={T} h={h} {name}: max abs difference {diff:.3e}, bound {bound:.3e}")
            if T > 1:
                assert diff < bound, (name, h)
                continue
            # One key: p = 1 and dP = D in exact arithmetic, so dQ = dK = 0 and a bound relative to them is empty.  What either
            # route may leave is the fp32 rounding of the two 64-term sums dP and D (each within 64 * 2^-24 of its sum of
            # magnitudes), times scale and the other operand, rounded once to bf16.
            resid = (2 * 64 * 2.0 ** -24 * (doh.float() * oh.float()).abs().sum(-1).max().item() * scale
                     * other.float().abs().max().item() * (1 + 2.0 ** -8))
            print(f"    exact result 0: |{name}| {got.float().abs().max().item():.3e} / {ref.abs().max().item():.3e}, residue bound {resid:.3e}")
            assert got.float().abs().max().item() <= resid and ref.abs().max().item() <= resid, (name, h)
