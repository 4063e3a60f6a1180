"""One-pass backward of the fused ConvNeXt MLP at C = 96 (csrc/mlp_bwd_onepass.hip): the data gradient through the LayerNorm and every
parameter gradient from ONE kernel that forms the hidden tile once.  Checked against the fp64 restatement on the bf16-rounded operands (the
inputs and reference of tests/test_mlp_fused_gpu.py), against the pair of kernels it replaces, for bit-reproducibility, for its workspace
contract, and through the ConvNeXt block's tape."""
import pytest
import torch

from tests import guarded_memory as GM
from tests.test_mlp_fused_gpu import _bwd_reference, _inputs

pytestmark = pytest.mark.gpu

C = 96
GRADS = (("dW1", (C, 4 * C)), ("db1", (4 * C,)), ("dW2", (4 * C, C)), ("db2", (C,)), ("dgamma", (C,)))
# (M, rows per drop-path group (0: no row factor), layer scale): less than one tile with masked rows; whole tiles; a ragged last tile; several
# chunks with a ragged tail, no row factor, no layer scale; five row groups over many chunks
CASES = [(33, 0, True), (256, 64, True), (1000 + 37, 512, True), (4096 + 37, 0, False), (64 * 300, 3840, True)]
_cache = {}


def _case(M, rpg, use_gamma):
    """operands on the device + the fp64 reference, built once per case and shared (read-only) by the tests"""
    key = (M, rpg, use_gamma)
    if key in _cache:
        return _cache[key]
    from iseg_amd import kernels as K

    y1, dout, W1, b1, W2, b2, gamma = _inputs(M, C, 4242 + M)
    if not use_gamma:
        gamma = None
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(19 + M)
    lng, lnb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    y1b, doutb = (y1 * 1.7 + 0.3).to(bf), dout.to(bf)
    groups = -(-M // rpg) if rpg else 0
    rs = (torch.arange(groups, dtype=torch.float32) * 0.5 + 0.25) if groups else None
    rs_rows = rs[torch.arange(M) // rpg] if groups else None
    dev = lambda t: None if t is None else t.cuda()
    y2, mean, rstd = K.layernorm_fwd(y1b.cuda(), lng.cuda(), lnb.cuda(), 1e-6)      # the rows the kernels re-form on load, and their statistics
    _, bw = K.convnext_mlp_prep(W1.cuda(), W2.cuda(), dev(gamma), backward=True)
    ref = _bwd_reference(y2.cpu(), doutb, rs_rows, W1, b1, W2, b2, gamma)
    # LayerNorm backward in fp64 on the reference's dy2 (keras LayerNormalization, saved fp32 statistics)
    d, x = ref["dy2"], y1b.double()
    xh = (x - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
    t = d * lng.double()
    ref["dy1"] = rstd.double().cpu()[:, None] * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
    ref["dln_gamma"], ref["dln_beta"] = (d * xh).sum(0), d.sum(0)
    ops = dict(y1=y1b.cuda(), dout=doutb.cuda(), bw=bw, b1=b1.cuda(), W2=W2.cuda(), b2=b2.cuda(), gamma=dev(gamma),
               ln=(mean, rstd, lng.cuda(), lnb.cuda()), rs=dev(rs), rpg=rpg)
    _cache[key] = (ops, ref)
    return _cache[key]


def _buffers():
    """live gradient buffers: the kernels accumulate into what is there"""
    grads = {k: torch.full(shape, 0.5, dtype=torch.float32, device="cuda") for k, shape in GRADS}
    grads["dln_gamma"] = torch.full((C,), 0.25, device="cuda")
    grads["dln_beta"] = torch.full((C,), -0.5, device="cuda")
    return grads


PREFILL = {"dW1": 0.5, "db1": 0.5, "dW2": 0.5, "db2": 0.5, "dgamma": 0.5, "dln_gamma": 0.25, "dln_beta": -0.5}


def _onepass(o):
    from iseg_amd import kernels as K

    g = _buffers()
    dy1 = K.convnext_mlp_bwd_onepass(o["y1"], o["dout"], o["bw"], o["b1"], o["W2"], o["b2"], o["gamma"], o["ln"], g["dln_gamma"], g["dln_beta"],
                                     g["dW1"], g["db1"], g["dW2"], g["db2"], g["dgamma"] if o["gamma"] is not None else None, o["rs"], o["rpg"])
    return dy1, g


def _pair(o):
    """the two kernels the one-pass kernel replaces"""
    from iseg_amd import kernels as K

    g = _buffers()
    dy1 = K.convnext_mlp_bwd_data_ln(o["y1"], o["dout"], o["bw"], o["b1"], o["ln"], g["dln_gamma"], g["dln_beta"], o["rs"], o["rpg"])
    K.convnext_mlp_wgrad(o["y1"], o["dout"], o["bw"], o["b1"], o["W2"], o["b2"], o["gamma"], g["dW1"], g["db1"], g["dW2"], g["db2"],
                         g["dgamma"] if o["gamma"] is not None else None, o["rs"], o["rpg"], ln=o["ln"])
    return dy1, g


def _names(o):
    return ("dW1", "db1", "dW2", "db2") + (("dgamma",) if o["gamma"] is not None else ())


def _check(dy1, grads, want_dy1, want, o, what):
    """the project's tolerances for these quantities; `want` holds fp64 values WITHOUT the buffers' prefill"""
    scale = max(1.0, want_dy1.abs().max().item())
    err = (dy1.double().cpu() - want_dy1).abs().max().item()
    rel = err / max(want_dy1.abs().max().item(), 1e-8)
    print(what, "dy1 abs", err, "rel", rel)
    assert err < 2e-2 * scale, (what, "dy1", err)
    assert rel < 1.5e-2, (what, "dy1 relative (the dy2-level bound)", rel)
    for k in _names(o):
        got = grads[k].double().cpu() - PREFILL[k]
        e = (got - want[k]).abs().max().item() / max(want[k].abs().max().item(), 1e-8)
        print(what, k, e)
        assert e < 6e-3, (what, k, e)
    for k in ("dln_gamma", "dln_beta"):
        got = grads[k].double().cpu() - PREFILL[k]
        e = (got - want[k]).abs().max().item()
        print(what, k, e, want[k].abs().max().item())
        assert e < 5e-3 * max(1.0, want[k].abs().max().item()), (what, k, e)


@pytest.mark.parametrize("M,rpg,use_gamma", CASES)
def test_onepass_matches_the_fp64_reference_and_is_bit_reproducible(cuda, M, rpg, use_gamma):
    o, ref = _case(M, rpg, use_gamma)
    dy1, grads = _onepass(o)
    _check(dy1, grads, ref["dy1"], ref, o, "fp64")
    dy1b, grads2 = _onepass(o)
    assert torch.equal(dy1, dy1b)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    if not use_gamma:
        assert torch.equal(grads["dgamma"], torch.full((C,), 0.5, device="cuda"))      # no layer scale: its buffer is not touched


@pytest.mark.parametrize("M,rpg,use_gamma", CASES)
def test_onepass_agrees_with_the_pair_it_replaces(cuda, M, rpg, use_gamma):
    o, _ = _case(M, rpg, use_gamma)
    dy1, grads = _onepass(o)
    dy1p, gp = _pair(o)
    want = {k: v.double().cpu() - PREFILL[k] for k, v in gp.items()}
    _check(dy1, grads, dy1p.double().cpu(), want, o, "pair")


def test_onepass_workspace_one_byte_short_is_refused_and_nothing_is_written(cuda):
    from iseg_amd import _hip

    o, _ = _case(1000 + 37, 512, True)
    arena = GM.Arena(cuda, nbytes=96 << 20)
    with GM.guarded(arena, short_workspace=1) as scope:
        grads = None
        with pytest.raises(_hip.HipCallError, match=r"status -4\b") as e:
            grads = _buffers()
            _onepass_into(o, grads)
        assert str(e.value).startswith("iseg_convnext_mlp_bwd_onepass failed with status"), str(e.value)
        arena.check()
        untouched, total = arena.untouched(role=None, since=scope.refused_from)
        assert total >= 2 and untouched == total      # dy1 and the short workspace are still poison
    for k, v in grads.items():
        assert torch.equal(v, torch.full_like(v, PREFILL[k])), k


def _onepass_into(o, g):
    from iseg_amd import kernels as K

    return K.convnext_mlp_bwd_onepass(o["y1"], o["dout"], o["bw"], o["b1"], o["W2"], o["b2"], o["gamma"], o["ln"], g["dln_gamma"], g["dln_beta"],
                                      g["dW1"], g["db1"], g["dW2"], g["db2"], g["dgamma"], o["rs"], o["rpg"])


@pytest.mark.parametrize("M,rpg,use_gamma", [(33, 0, True), (1000 + 37, 512, True)])
def test_onepass_at_the_exact_workspace_size_keeps_the_guard_bands(cuda, M, rpg, use_gamma):
    o, ref = _case(M, rpg, use_gamma)
    arena = GM.Arena(cuda, nbytes=96 << 20)
    with GM.guarded(arena):
        grads = _buffers()
        dy1 = _onepass_into(o, grads)
        arena.check()
        assert len(arena.records) >= 2
        _check(dy1, grads, ref["dy1"], ref, o, "guarded")      # (poison read from a band would be NaN here)


def test_convnext_block_tape_takes_the_onepass_route_and_matches_the_pair(cuda, monkeypatch):
    """one ConvNeXt block, forward + backward at 2 x 64 x 64 x 96 with a drop-path mask: the tape's one-pass route against the same tape on the
    pair of kernels (the route of the parent commit, still the route at C = 192)"""
    from iseg_amd import kernels as K, nn
    from iseg_amd.backbones.convnext import Block
    from iseg_amd.param_store import ParamStore
    from tests.util_models import randomize_parameters

    dtype, shape = torch.bfloat16, (2, 64, 64, C)
    nn.set_compute_dtype(dtype)
    nn.set_device("cuda:0")
    try:
        blk = Block(C, drop_path_prob=0.2, layer_scale_init_value=1.0, name="stages/0/0")
        with nn.dry_run_scope():
            blk(torch.empty(shape, dtype=dtype, device="cuda"))
        blk._iseg_store = ParamStore(list(blk.parameters()))
        randomize_parameters(blk, 3)
        g = torch.Generator().manual_seed(1)
        x, dy = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
        blk.drop_path_mask = torch.tensor([1.25, 0.75], device="cuda")
        calls = []
        real = K.convnext_mlp_bwd_onepass
        monkeypatch.setattr(K, "convnext_mlp_bwd_onepass", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

        def run():
            for p in blk.parameters():
                p.grad = None
            xg = x.cuda().requires_grad_(True)
            y = blk(xg, training=True)
            y.backward(dy.cuda())
            torch.cuda.synchronize()
            return {"y": y.detach().clone(), "dx": xg.grad.clone(), **{p.iseg_name: p.grad.clone() for p in blk.parameters()}}

        new = run()
        assert calls, "the block's backward did not take the one-pass route"
        monkeypatch.setattr(K, "convnext_mlp_bwd_onepass_supported", lambda C_, dt_: False)
        n = len(calls)
        old = run()
        assert len(calls) == n
        assert torch.equal(new["y"], old["y"])
        for k in old:
            a, b = new[k].double(), old[k].double()
            e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-8)
            print(k, e)
            # dx and the depthwise gradients sit behind dy1 (2e-2 of its range); the MLP's own gradients only change through nothing at all
            assert e < (2e-2 if k == "dx" or "dwconv" in k or "depthwise" in k else 6e-3), (k, e)
    finally:
        nn.set_compute_dtype(torch.float32)
