"""The SyncBN statistics exchange of functional.py (_bn_batch_stats forward, _bn_exchange_sums backward) under every tape node that carries a
BatchNorm: batch_norm, batch_norm_group, batch_norm_relu_upsample_add, bn_swish_se, sepconv_unit and resblock_tail, fp32, training mode,
synchronised.  Two ranks (both on cuda:0, gloo transport because one box has one GPU) with half the batch each must reproduce the fp64
full-batch restatement the node's own test module compares against: outputs and input gradients concatenated over the ranks, parameter
gradients summed over the ranks, moving statistics bit-identical on both ranks.  The same nodes run once more on the full batch in this process,
without a process group (the branch on which the apply kernels book the parameter gradients), against the same references."""
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models as OM
from oracle import tf_ops as O
from tests import test_mbconv_fused_gpu as MB
from tests import test_resblock_fused_gpu as RB
from tests import test_sepconv_fused_gpu as SC
from tests.test_dp_gpu import _free_port

pytestmark = pytest.mark.gpu

BATCH = 4      # 2 samples per rank
SEPCONV = (BATCH,) + SC.CASES[1][1:]      # the smallest stride-2 entry, (3, 10, 12, 64, 32, 2, 1), with the batch set to 4
# the bounds of each node's fp32-against-fp64 test, by key prefix; the plain nodes take test_kernels_gpu.py's (test_batchnorm_train,
# test_bn_relu_upsample_add_and_remask_backward): forward and moving mean 1e-4, moving variance 1e-3, gradients 3e-4
PLAIN_TOL = {"out": 1e-4, "dx": 3e-4, "g:": 3e-4, "mean:": 1e-4, "var:": 1e-3}


def _rel(got, want):
    return (torch.as_tensor(got).double() - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def _plain_layers(*channels):
    layers = {("bn" if len(channels) == 1 else f"bn{i}"): RB._bn(f"bn{i}", C, 40 + i) for i, C in enumerate(channels)}
    for b in layers.values():
        b.synchronized = True
    return layers


def _randn(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def _layer_results(layers):
    res = {}
    for n, b in layers.items():
        res.update({f"g:{n}/{k}": getattr(b, k).grad for k in ("gamma", "beta")})
        res.update({f"mean:{n}": b.moving_mean, f"var:{n}": b.moving_variance})
    return res


def _layer_reference(w, new_stats):
    res = {f"g:{k}": v.grad for k, v in w.items() if v.requires_grad}
    for k, v in new_stats.items():
        n, stat = k.split("/")
        res[("mean:" if stat == "moving_mean" else "var:") + n] = v
    return res


# ---- the six nodes: _case_* (full-batch inputs and fresh layers from fixed seeds), _run_* (the product on samples lo:hi), _ref_* (fp64) ------
def _case_batch_norm():
    x, dy = _randn(1, (BATCH, 5, 7, 16), (BATCH, 5, 7, 16))
    return x * 1.5 + 0.2, dy, _plain_layers(16)


def _run_batch_norm(F, lo, hi):
    x, dy, layers = _case_batch_norm()
    b = layers["bn"]
    xd = x[lo:hi].cuda().requires_grad_(True)
    out = F.batch_norm(xd, b.gamma, b.beta, b.moving_mean, b.moving_variance, b.epsilon, b.momentum, True, relu=True, sync=True)
    out.backward(dy[lo:hi].cuda())
    return dict(out=out, dx=xd.grad, **_layer_results(layers))


def _ref_batch_norm(got):
    x, dy, layers = _case_batch_norm()
    w, stats = RB._weights(layers), {}
    xr = x.double().requires_grad_(True)
    pre = OM._bn(w, "bn", xr, True, layers["bn"].epsilon, new_stats=stats)
    (pre * (got["out"] > 0).double()).backward(dy.double())      # the product's ReLU mask, as tests/test_resblock_fused_gpu.py _ref takes it
    return dict(out=torch.relu(pre).detach(), dx=xr.grad, **_layer_reference(w, stats))


GROUP_SHAPES = [(BATCH, 3, 5, 16), (BATCH, 3, 5, 40), (BATCH, 1, 1, 8)]      # channel counts differ: the slot offsets of the message matter


def _case_group():
    ts = _randn(2, *GROUP_SHAPES, *GROUP_SHAPES)
    return [t * 1.5 + 0.2 for t in ts[:3]], ts[3:], _plain_layers(*[s[-1] for s in GROUP_SHAPES])


def _run_group(F, lo, hi):
    xs, dys, layers = _case_group()
    xd = [x[lo:hi].cuda().requires_grad_(True) for x in xs]
    outs = F.batch_norm_group(xd, list(layers.values()), relu=True)
    torch.autograd.backward(outs, [dy[lo:hi].cuda() for dy in dys])
    res = _layer_results(layers)
    for i in range(3):
        res.update({f"out{i}": outs[i], f"dx{i}": xd[i].grad})
    return res


def _ref_group(got):
    xs, dys, layers = _case_group()
    w, stats = RB._weights(layers), {}
    res = {}
    for i, (n, b) in enumerate(layers.items()):
        xr = xs[i].double().requires_grad_(True)
        pre = OM._bn(w, n, xr, True, b.epsilon, new_stats=stats)
        (pre * (got[f"out{i}"] > 0).double()).backward(dys[i].double())
        res.update({f"out{i}": torch.relu(pre).detach(), f"dx{i}": xr.grad})
    res.update(_layer_reference(w, stats))
    return res


def _case_upsample_add():
    z, x, dout = _randn(3, (BATCH, 6, 10, 16), (BATCH, 3, 5, 16), (BATCH, 6, 10, 16))
    return z * 1.5 + 0.2, x, dout, _plain_layers(16)


def _run_upsample_add(F, lo, hi):
    z, x, dout, layers = _case_upsample_add()
    b = layers["bn"]
    zd, xd = z[lo:hi].cuda().requires_grad_(True), x[lo:hi].cuda().requires_grad_(True)
    out = F.batch_norm_relu_upsample_add(zd, xd, b.gamma, b.beta, b.moving_mean, b.moving_variance, b.epsilon, b.momentum, sync=True)
    out.backward(dout[lo:hi].cuda())
    return dict(out=out, dx0=zd.grad, dx1=xd.grad, **_layer_results(layers))


def _ref_upsample_add(got):
    z, x, dout, layers = _case_upsample_add()
    w, stats = RB._weights(layers), {}
    zr, xr = z.double().requires_grad_(True), x.double().requires_grad_(True)
    pre = OM._bn(w, "bn", zr, True, layers["bn"].epsilon, new_stats=stats)
    # the node's output is relu(bn(z)) + up(x), which does not show the product's mask; these inputs leave no pre-activation within 1e-5 of
    # zero (fp32 places them to about 1e-6), so the fp64 mask is the product's
    assert pre.abs().min().item() > 1e-5
    out = torch.relu(pre) + O.resize_bilinear(xr, tuple(z.shape[1:3]))
    out.backward(dout.double())
    return dict(out=out.detach(), dx0=zr.grad, dx1=xr.grad, **_layer_reference(w, stats))


SE_SHAPE = (BATCH, 7, 9, 32, 4)      # N, H, W, C, Cse
SE_PARAMS = ("gamma", "beta", "W1", "b1", "W2", "b2")


def _case_bn_swish_se():
    N, H, W, C, Cse = SE_SHAPE
    x, dO = _randn(4, (N, H, W, C), (N, H, W, C))
    return x * 1.5 + 0.3, dO, MB._params(C, Cse, 5)


def _run_bn_swish_se(F, lo, hi):
    x, dO, p = _case_bn_swish_se()
    prm = {k: torch.nn.Parameter(v.clone().cuda(), requires_grad=k in SE_PARAMS) for k, v in p.items()}
    mm, mv = prm["mm"].data, prm["mv"].data
    xd = x[lo:hi].cuda().requires_grad_(True)
    assert F.bn_swish_se_supported(xd, SE_SHAPE[4], prm["gamma"], prm["beta"], mm, mv)
    out = F.bn_swish_se(xd, prm["gamma"], prm["beta"], mm, mv, MB.EPS, MB.MOMENTUM, True, prm["W1"], prm["b1"], prm["W2"], prm["b2"], sync=True)
    out.backward(dO[lo:hi].cuda())
    res = {"out": out, "dx": xd.grad, "mean:": mm, "var:": mv}
    res.update({f"g:{k}": prm[k].grad for k in SE_PARAMS})
    return res


def _ref_bn_swish_se(got):
    x, dO, p = _case_bn_swish_se()
    out, grads, mean, var = MB._reference(x, p, True, dO)
    res = {"out": out, "dx": grads["x"], "mean:": O.moving_update(p["mm"].double(), mean, MB.MOMENTUM),
           "var:": O.moving_update(p["mv"].double(), var, MB.MOMENTUM)}
    res.update({f"g:{k}": grads[k] for k in SE_PARAMS})
    return res


SEPCONV_KEYS = dict(v="out", dx="dx", ddw="g:ddw", dpw="g:dpw", dgamma="g:dgamma", dbeta="g:dbeta", moving_mean="mean:",
                    moving_variance="var:")


def _case_sepconv():
    N, H, W, C, Cout, s, d = SEPCONV
    u = SC._unit(C, Cout, s, d, torch.float32, seed=sum(SEPCONV))
    u.depthwise_bn.synchronized = True
    return (u,) + SC._inputs(N, H, W, C, Cout, s, d, torch.float32, sum(SEPCONV))


def _run_sepconv(F, lo, hi):
    u, x, dv = _case_sepconv()
    s, d = SEPCONV[5:]
    dw, bn, pw = u.depthwise_conv, u.depthwise_bn, u.pointwise_conv
    u._iseg_store.zero_grad()
    xd = x[lo:hi].clone().requires_grad_(True)
    assert F.sepconv_fused_enabled() and F.sepconv_supported(xd, dw.depthwise_kernel, bn, pw.kernel, s, d)
    v = F.sepconv_unit(xd, dw.depthwise_kernel, bn, pw.kernel, True, strides=s, dilation=d)
    v.backward(dv[lo:hi].clone())
    got = dict(v=v, dx=xd.grad, ddw=dw.depthwise_kernel.grad, dpw=pw.kernel.grad, dgamma=bn.gamma.grad, dbeta=bn.beta.grad,
               moving_mean=bn.moving_mean, moving_variance=bn.moving_variance)
    return {SEPCONV_KEYS[k]: t for k, t in got.items()}


def _ref_sepconv(got):
    u, x, dv = _case_sepconv()
    ref = SC._reference(u, x, dv, True, *SEPCONV[5:])
    return {SEPCONV_KEYS[k]: ref[k] for k in SC.KEYS}


def _case_resblock():
    """BN0 shortcut, stride 2: both layers' statistics in one message each way"""
    z2, sc, dout, layers = RB._case(True, 2, 32, H=9, W=7, N=BATCH, seed=6)
    for b in layers.values():
        b.synchronized = True
    return z2, sc, dout, layers


def _run_resblock(F, lo, hi):
    z2, sc, dout, layers = _case_resblock()
    zd, xd = z2[lo:hi].cuda().requires_grad_(True), sc[lo:hi].cuda().requires_grad_(True)
    assert F.resblock_fused_enabled() and F.resblock_tail_supported(zd, xd, layers["t_2_bn"], layers["t_0_bn"], 2)
    out = F.resblock_tail(zd, layers["t_2_bn"], xd, layers["t_0_bn"], 2, True)
    out.backward(dout[lo:hi].cuda())
    return dict(out=out, dx0=zd.grad, dx1=xd.grad, **_layer_results(layers))


def _ref_resblock(got):
    z2, sc, dout, layers = _case_resblock()
    w = RB._weights(layers)
    out, dz2, dsc, grads, stats = RB._ref(z2, sc, dout, w, 2, True, True, mask=torch.as_tensor(got["out"] > 0).double())
    res = dict(out=out, dx0=dz2, dx1=dsc)
    res.update({f"g:{k}": v for k, v in grads.items()})
    res.update(_layer_reference({}, stats))
    return res


NODES = {      # name: (product run, fp64 reference, bound by key prefix)
    "batch_norm": (_run_batch_norm, _ref_batch_norm, PLAIN_TOL),
    "batch_norm_group": (_run_group, _ref_group, PLAIN_TOL),
    "batch_norm_relu_upsample_add": (_run_upsample_add, _ref_upsample_add, PLAIN_TOL),
    "bn_swish_se": (_run_bn_swish_se, _ref_bn_swish_se, {"": 1e-5}),      # test_mbconv_fused_gpu.py
    "sepconv_unit": (_run_sepconv, _ref_sepconv, {"": 1e-4}),               # test_sepconv_fused_gpu.py
    "resblock_tail": (_run_resblock, _ref_resblock, {"": 1e-3}),            # test_resblock_fused_gpu.py
}


def _run_nodes(lo, hi):
    """every node forward and backward on samples lo:hi of its batch; numpy arrays (pickled by value: torch tensors would travel through
    /dev/shm handles that die with the child)"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    res = {}
    for name, (run, _, _) in NODES.items():
        res[name] = {k: t.detach().cpu().numpy().copy() for k, t in run(F, lo, hi).items()}
    torch.cuda.synchronize()
    return res


def _rank(rank, world, port, q):
    import os

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      ISEG_DIST_BACKEND="gloo")
    os.environ.pop("ISEG_DIST_NATIVE", None)
    from iseg_amd import dist

    dist.init()
    assert dist.active() and dist.world_size() == world
    per = BATCH // world
    q.put((rank, _run_nodes(rank * per, (rank + 1) * per)))
    dist.barrier()
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def runs(cuda):
    """{"two ranks": [rank 0's results, rank 1's], "one rank": [this process's, full batch, no process group]}"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(120)
    assert all(p.exitcode == 0 for p in procs)
    from iseg_amd import dist, nn

    assert not dist.active()
    try:
        full = _run_nodes(0, BATCH)
    finally:
        nn.set_compute_dtype(torch.float32)
    return {"two ranks": [r[1] for r in sorted(res, key=lambda r: r[0])], "one rank": [full]}


def _merge(parts):
    """outputs and input gradients concatenated over the ranks, parameter gradients summed, moving statistics bit-identical on every rank"""
    got = {}
    for k in parts[0]:
        vals = [torch.from_numpy(p[k]) for p in parts]
        if k.startswith("g:"):
            got[k] = torch.stack([v.double() for v in vals]).sum(0)
        elif k.startswith(("mean:", "var:")):
            assert all(torch.equal(v, vals[0]) for v in vals), f"ranks diverged on {k}"
            got[k] = vals[0]
        else:
            got[k] = torch.cat(vals)
    return got


def _check(runs, node):
    _, ref, tols = NODES[node]
    bad = {}
    for label, parts in runs.items():
        got = _merge([p[node] for p in parts])
        want = ref(got)
        assert set(want) == set(got)
        for k, w in want.items():
            assert tuple(got[k].shape) == tuple(w.shape), (label, k)
            tol = tols[max((p for p in tols if k.startswith(p)), key=len)]
            err = _rel(got[k], w.detach())
            print(f"{node} {label} {k}: {err:.3e} (bound {tol:.0e})")
            if not err < tol:
                bad[label, k] = (err, tol)
    assert not bad, bad


def test_batch_norm(runs):
    _check(runs, "batch_norm")


def test_batch_norm_group(runs):
    _check(runs, "batch_norm_group")


def test_batch_norm_relu_upsample_add(runs):
    _check(runs, "batch_norm_relu_upsample_add")


def test_bn_swish_se(runs):
    _check(runs, "bn_swish_se")


def test_sepconv_unit(runs):
    _check(runs, "sepconv_unit")


def test_resblock_tail(runs):
    _check(runs, "resblock_tail")


def test_batch_norm_inference_backward_reads_the_statistics_of_its_own_call(cuda):
    """an inference-mode F.batch_norm with trainable gamma / beta, then a training-mode call that updates the moving statistics in place: the
    first call's backward still books dgamma with the mean it was evaluated with"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    x, dy, layers = _case_batch_norm()
    b = layers["bn"]
    w = RB._weights(layers)
    args = (b.gamma, b.beta, b.moving_mean, b.moving_variance, b.epsilon, b.momentum)
    xd = x.cuda().requires_grad_(True)
    out = F.batch_norm(xd, *args, False, relu=True, sync=False)
    with torch.no_grad():
        F.batch_norm(x.cuda() * 2.0 + 1.0, *args, True, sync=False)      # moves the moving statistics in place
    assert not torch.equal(b.moving_mean.cpu().double(), w["bn/moving_mean"])
    out.backward(dy.cuda())
    xr = x.double().requires_grad_(True)
    pre = OM._bn(w, "bn", xr, False, b.epsilon)
    (pre * (out.detach().cpu() > 0).double()).backward(dy.double())
    assert _rel(out.detach().cpu(), torch.relu(pre).detach()) < PLAIN_TOL["out"]
    assert _rel(xd.grad.cpu(), xr.grad) < PLAIN_TOL["dx"]
    for k in ("gamma", "beta"):
        assert _rel(getattr(b, k).grad.cpu(), w[f"bn/{k}"].grad) < PLAIN_TOL["g:"], k
