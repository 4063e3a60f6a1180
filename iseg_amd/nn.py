"""Minimal Keras-flavoured layer system on torch tensors (host-side bookkeeping only).

The reference builds everything from keras.Model / keras.layers.Layer objects that are called as
`layer(inputs, training=None)` and own named variables (utils/keras3_utils.py:25-62).  This module provides the
same surface: lazily built layers, slash-separated variable names (used by the no-weight-decay rules of
utils/train_utils.py:8-37), fp32 master parameters with an optional bf16 shadow copy for the MFMA kernels.
"""
import contextlib
import math
import os
import zlib

import torch

# ---------------------------------------------------------------------------------------------------------
# global policy  (utils/common.py:32-64 enable_mixed_precision -> mixed_bfloat16 on MI355X, always)
# ---------------------------------------------------------------------------------------------------------
_POLICY = {"compute_dtype": torch.float32, "device": None, "seed": 0}


def set_compute_dtype(dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be float32 or bfloat16")
    _POLICY["compute_dtype"] = dtype


def compute_dtype():
    return _POLICY["compute_dtype"]


def set_device(device):
    _POLICY["device"] = torch.device(device) if device is not None else None


def device():
    if _POLICY["device"] is not None:
        return _POLICY["device"]
    if torch.cuda.is_available():
        return torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    return torch.device("cpu")  # parameters can be laid out without a GPU; every kernel call will refuse to run


def set_seed(seed):
    _POLICY["seed"] = int(seed)


def seed():
    return _POLICY["seed"]


# ---------------------------------------------------------------------------------------------------------
# initializers (keras defaults: glorot_uniform kernels, zeros / ones elsewhere); seeded per variable name
# ---------------------------------------------------------------------------------------------------------
def _gen(name):
    g = torch.Generator()
    g.manual_seed((zlib.crc32(name.encode()) ^ (_POLICY["seed"] * 0x9E3779B1)) & 0x7FFFFFFF)
    return g


def _fans(shape):
    if len(shape) < 1:
        return 1, 1
    if len(shape) == 1:
        return shape[0], shape[0]
    if len(shape) == 2:
        return shape[0], shape[1]
    rf = 1
    for s in shape[:-2]:
        rf *= s
    return shape[-2] * rf, shape[-1] * rf


def init_tensor(initializer, shape, name):
    shape = tuple(int(s) for s in shape)
    if callable(initializer):
        return torch.as_tensor(initializer(shape), dtype=torch.float32).reshape(shape)
    if isinstance(initializer, (int, float)):
        return torch.full(shape, float(initializer))
    if initializer in ("zeros", None):
        return torch.zeros(shape)
    if initializer == "ones":
        return torch.ones(shape)
    if initializer == "glorot_uniform":
        fi, fo = _fans(shape)
        lim = math.sqrt(6.0 / (fi + fo))
        return (torch.rand(shape, generator=_gen(name)) * 2 - 1) * lim
    if initializer == "he_normal":
        fi, _ = _fans(shape)
        return torch.randn(shape, generator=_gen(name)) * math.sqrt(2.0 / fi)
    if initializer == "he_normal_fan_out":      # keras VarianceScaling(scale=2, mode="fan_out", distribution="untruncated_normal") (layers/nasfpn.py:283-302)
        _, fo = _fans(shape)
        return torch.randn(shape, generator=_gen(name)) * math.sqrt(2.0 / fo)
    if initializer == "he_truncated_normal_fan_out":      # keras VarianceScaling(scale=2, mode="fan_out", distribution="truncated_normal") (backbones/efficientnet.py:94-97)
        _, fo = _fans(shape)
        return torch.randn(shape, generator=_gen(name)).clamp_(-2, 2) * (math.sqrt(2.0 / fo) / 0.87962566103423978)
    if isinstance(initializer, tuple) and initializer[0] == "uniform":      # keras RandomUniform(-v, v)
        return (torch.rand(shape, generator=_gen(name)) * 2 - 1) * float(initializer[1])
    if isinstance(initializer, tuple) and initializer[0] == "truncated_normal":
        std = initializer[1]
        t = torch.randn(shape, generator=_gen(name)).clamp_(-2, 2) * std
        return t
    raise ValueError(f"unknown initializer {initializer!r}")


# ---------------------------------------------------------------------------------------------------------
# Layer
# ---------------------------------------------------------------------------------------------------------
def replace_slash(name):
    return name


class Layer(torch.nn.Module):
    """keras.layers.Layer / keras.Model look-alike: `layer(inputs, training=None)` -> `call`, lazy `build`."""

    _auto_names = {}

    def __init__(self, name=None, trainable=True, **kwargs):
        super().__init__()
        if name is None:
            base = type(self).__name__.lower()
            n = Layer._auto_names.get(base, 0)
            Layer._auto_names[base] = n + 1
            name = base if n == 0 else f"{base}_{n}"
        self.__dict__["name"] = name
        self.trainable = trainable
        self.built = False

    # -- variables ------------------------------------------------------------------------------------------
    def add_weight(self, name, shape, initializer="zeros", trainable=True):
        full = f"{self.name}/{name}"
        data = init_tensor(initializer, shape, full).to(device())
        p = torch.nn.Parameter(data, requires_grad=bool(trainable and self.trainable))
        p.iseg_name = full
        p.lr_multiplier = 1.0
        p.iseg_compute = None   # bf16 shadow view, installed by ParamStore
        attr = name.replace("/", "_").replace(".", "_")
        self.__dict__.pop(attr, None)      # a plain placeholder attribute (e.g. self.kernel = None) gives way
        self.register_parameter(attr, p)
        return p

    def add_state(self, name, shape, initializer="zeros"):
        """non-trainable variable (BN moving statistics)"""
        full = f"{self.name}/{name}"
        t = init_tensor(initializer, shape, full).to(device())
        t.iseg_name = full
        attr = name.replace("/", "_")
        self.__dict__.pop(attr, None)
        self.register_buffer(attr, t)
        return t

    # -- call protocol ---------------------------------------------------------------------------------------
    def build(self, input_shape):
        self.built = True

    def call(self, inputs, training=None):
        raise NotImplementedError

    @staticmethod
    def _shape_of(inputs):
        if isinstance(inputs, torch.Tensor):
            return tuple(inputs.shape)
        if isinstance(inputs, (list, tuple)):
            return [Layer._shape_of(i) for i in inputs]
        if isinstance(inputs, dict):
            return {k: Layer._shape_of(v) for k, v in inputs.items()}
        return None

    def forward(self, inputs, *args, training=None, **kwargs):
        if not self.built:
            self.build(self._shape_of(inputs))
            self.built = True
        if training is None:
            training = False
        return self.call(inputs, *args, training=training, **kwargs)

    # -- introspection used by train_utils / modelhelper -------------------------------------------------------
    def sublayers(self):
        return [m for m in self.modules() if isinstance(m, Layer)]

    @property
    def weights(self):
        return list(self.parameters()) + [b for b in self.buffers()]

    @property
    def trainable_weights(self):
        return [p for p in self.parameters() if p.requires_grad]


def w(param):
    """the tensor a kernel should read for `param`: bf16 shadow under mixed precision, else the fp32 master"""
    if compute_dtype() == torch.bfloat16:
        sh = getattr(param, "iseg_compute", None)
        if sh is None:
            raise RuntimeError(
                f"parameter {getattr(param, 'iseg_name', '?')} has no bf16 shadow: call ParamStore(model) / "
                "model_common_setup before running under mixed precision")
        return sh
    return param.data


# ---------------------------------------------------------------------------------------------------------
# K-contiguous copies of the 2-D compute kernels (forward GEMMs through the LDS-DMA pipeline)
# ---------------------------------------------------------------------------------------------------------
_WEIGHTS_VERSION = [0]
_WT = {"version": -1, "params": [], "index": {}, "buf": None, "views": [], "table": None, "base": 0, "max_tiles": 0, "ptrs": []}


# Generation of the DEVICE BUFFERS behind wt() / mlp_tiled() / w_colscaled(): bumped whenever one of them (or a pointer table) is re-allocated --
# a model was dropped or added, a parameter registered, a kernel view changed.  A captured HIP graph holds raw pointers into those buffers, so the
# graph runners (iseg_amd/graphs.py) remember the generation they captured under and capture again when it has moved; replaying across a
# re-allocation would read and write freed memory without any error.
_BUFFERS_GENERATION = [0]


def buffers_generation():
    return _BUFFERS_GENERATION[0]


def bump_buffers_generation():
    """a long-lived device buffer that captured graphs point into was re-allocated outside this module (kernels._dcn_side)"""
    _BUFFERS_GENERATION[0] += 1


def weights_changed():
    """the bf16 compute copies were rewritten (optimizer step, ParamStore.sync_shadow): transposed copies are stale"""
    _WEIGHTS_VERSION[0] += 1


def _wt_rebuild():
    # the registry must not keep dropped models alive (or re-transpose their kernels forever): entries are weak references, dead ones go here
    live = [r for r in _WT["params"] if r() is not None]
    _WT["params"] = live
    _WT["index"] = {id(r()): j for j, r in enumerate(live)}
    _BUFFERS_GENERATION[0] += 1
    shadows = [r().iseg_compute for r in live]
    if not shadows:
        _WT.update(buf=None, views=[], table=None, ptrs=[], max_tiles=0, version=-1)
        return
    dev = shadows[0].device
    base = min(sh.data_ptr() for sh in shadows)
    total, rows = 0, []
    for r, sh in zip(live, shadows):
        k, n = getattr(r(), "iseg_kshape", None) or sh.shape      # (kernels with more than two axes: the [K, N] view their GEMM uses)
        rows.append([(sh.data_ptr() - base) // 2, total, k, n])
        total += (k * n + 7) // 8 * 8
    buf = torch.empty(total, dtype=torch.bfloat16, device=dev)
    _WT.update(buf=buf, base=base, views=[buf[do:do + k * n].view(n, k) for (_, do, k, n) in rows],
               table=torch.tensor(rows, dtype=torch.int64).to(dev), ptrs=[sh.data_ptr() for sh in shadows],
               max_tiles=max(((k + 63) // 64) * ((n + 63) // 64) for (_, _, k, n) in rows), version=-1)


def register_wt(params):
    """register every eligible 2-D kernel of `params` at once (ParamStore build): one rebuild instead of one per first use"""
    import weakref

    added = False
    for p in params:
        sh = getattr(p, "iseg_compute", None)
        if sh is None or not sh.is_cuda or (sh.dim() != 2 and getattr(p, "iseg_kshape", None) is None):
            continue
        i = _WT["index"].get(id(p))
        if i is None or _WT["params"][i]() is not p:
            _WT["index"][id(p)] = len(_WT["params"])
            _WT["params"].append(weakref.ref(p))
            added = True
    if added:
        _wt_rebuild()


def refresh_wt():
    """bring every registered K-contiguous kernel copy up to date NOW (one launch) -- for callers that will not pass through wt() again
    before the copies are read, i.e. the replay of a captured graph (iseg_amd/graphs.py)"""
    if _WT["version"] != _WEIGHTS_VERSION[0]:
        for r in _WT["params"]:
            if r() is not None:
                wt(r())
                break


def refresh_prep():
    """the same for the per-update derivations of the ConvNeXt blocks (tiled MLP images, layer-scale-folded kernels): a replayed inference
    graph reads them without passing through mlp_tiled() / w_colscaled(), whose host-side version check is what refreshes them"""
    if _PREP["entries"] and _PREP["version"] != _WEIGHTS_VERSION[0]:
        _prep_refresh()


def weights_version():
    return _WEIGHTS_VERSION[0]


def wt(param, kshape=None):
    """[N][K] bf16 copy of the kernel `param` ([K][N]; `kshape` = the (K, N) view of a kernel with more axes: a 1x1 convolution's
    [1, 1, Cin, Cout], keras MultiHeadAttention's [C, heads, d] / [heads, d, C]) under mixed precision, or None (fp32 compute, no shadow, no 2-D
    view).  All registered kernels are re-transposed by ONE launch (iseg_transpose_batched) the first time any of them is asked for after a
    weight update."""
    if compute_dtype() != torch.bfloat16:
        return None
    sh = getattr(param, "iseg_compute", None)
    if sh is None or not sh.is_cuda:
        return None
    if sh.dim() != 2:
        kshape = kshape or getattr(param, "iseg_kshape", None)
        if kshape is None or kshape[0] * kshape[1] != sh.numel() or not sh.is_contiguous():
            return None
        if getattr(param, "iseg_kshape", None) != tuple(kshape):
            param.iseg_kshape = tuple(kshape)
            _WT["index"].pop(id(param), None)      # (registered under another view: rebuild)
    i = _WT["index"].get(id(param))
    if i is None or i >= len(_WT["params"]) or _WT["params"][i]() is not param:      # new, or an id recycled after its owner died
        register_wt([param])
        i = _WT["index"][id(param)]
    if _WT["version"] != _WEIGHTS_VERSION[0]:
        dead = any(r() is None for r in _WT["params"])
        if dead or any(r().iseg_compute.data_ptr() != q for r, q in zip(_WT["params"], _WT["ptrs"])):      # a dropped model / a new ParamStore re-homed the shadows
            _wt_rebuild()
            i = _WT["index"][id(param)]
        from . import _hip
        from . import kernels as K

        _hip.call("iseg_transpose_batched", _WT["base"], K.ptr(_WT["buf"]), K.ptr(_WT["table"]), len(_WT["params"]), _WT["max_tiles"], K.stream())
        _WT["version"] = _WEIGHTS_VERSION[0]
    return _WT["views"][i]


# ---------------------------------------------------------------------------------------------------------
# per-weight-update derivations of the ConvNeXt blocks (tiled MLP images, layer-scale-folded kernels): ONE launch per update for all blocks
# ---------------------------------------------------------------------------------------------------------
_PREP = {"version": -1, "entries": [], "index": {}, "table": None, "ptrs": None, "max": 0}


def _prep_key(kind, params):
    return (kind,) + tuple(id(p) for p in params)


def _prep_request(kind, params, make):
    """the derived buffers of (kind, params), refreshed by one batched launch the first time any of them is asked for after a weight update"""
    import weakref

    key = _prep_key(kind, params)
    i = _PREP["index"].get(key)
    if i is not None and any(r() is not p for r, p in zip(_PREP["entries"][i]["refs"], params)):
        i = None      # an id was recycled by another parameter
    if i is None:
        # drop the entries of models that are gone (the registry must not keep them alive or re-derive them forever)
        live = [e for e in _PREP["entries"] if all(r() is not None for r in e["refs"])]
        _PREP["entries"] = live
        _PREP["index"] = {e["key"]: j for j, e in enumerate(live)}
        bufs = make()
        _PREP["index"][key] = i = len(live)
        live.append({"key": key, "kind": kind, "refs": [weakref.ref(p) for p in params], "bufs": bufs})
        _BUFFERS_GENERATION[0] += 1
        _PREP["table"] = None
        _PREP["version"] = -1
    if _PREP["version"] != _WEIGHTS_VERSION[0]:
        _prep_refresh()
    return _PREP["entries"][i]["bufs"]


def _prep_rows(e):
    ps = [r() for r in e["refs"]]
    if e["kind"] == 1:
        w1, w2, gamma = ps[0], ps[1], (ps[2] if len(ps) > 2 else None)
        fw, bw = e["bufs"]
        Cc = w1.shape[0]
        return [1, w1.data.data_ptr(), w2.data.data_ptr(), gamma.data.data_ptr() if gamma is not None else 0, fw.data_ptr(),
                bw.data_ptr() if bw is not None else 0, Cc, 0], 5 * 4 * Cc * Cc
    if e["kind"] == 2:
        wa, wb = ps[0], ps[1]
        ba, bb = (ps[2], ps[3]) if len(ps) > 2 else (None, None)
        blob = e["bufs"][3]
        Cc, na, nb = wa.shape[0], wa.shape[1], wb.shape[1]
        ld = (na + nb + 7) // 8 * 8
        return [2, wa.data.data_ptr(), wb.data.data_ptr(), ba.data.data_ptr() if ba is not None else 0, blob.data_ptr(),
                bb.data.data_ptr() if bb is not None else 0, Cc, na | (nb << 20) | (ld << 40)], Cc * ld
    w2, gamma = ps
    (dst,) = e["bufs"]
    rows, cols = w2.shape
    return [0, w2.data.data_ptr(), 0, gamma.data.data_ptr(), dst.data_ptr(), 0, cols, rows], rows * cols


def _prep_refresh():
    from . import _hip
    from . import kernels as K

    rows, mx = [], 0
    for e in _PREP["entries"]:
        if any(r() is None for r in e["refs"]):
            continue
        r, n = _prep_rows(e)
        rows.append(r)
        mx = max(mx, n)
    if not rows:
        return
    if _PREP["table"] is None or _PREP["ptrs"] != rows:      # first use, a new block, or a re-homed parameter
        _BUFFERS_GENERATION[0] += 1
        dev = _PREP["entries"][0]["bufs"][0].device
        _PREP["table"] = torch.tensor(rows, dtype=torch.int64).to(dev)
        _PREP["ptrs"], _PREP["max"] = rows, mx
    _hip.call("iseg_convnext_weight_prep_batched", K.ptr(_PREP["table"]), len(rows), int(_PREP["max"]), K.stream())
    _PREP["version"] = _WEIGHTS_VERSION[0]


def mlp_tiled(w1, w2, gamma):
    """(fw_tiled, bw_tiled) of a fused ConvNeXt MLP (csrc/mlp_fused.hip images), valid for the current weights"""
    def make():
        from . import _hip

        L = _hip.lib()
        Cc = w1.shape[0]
        dev = w1.device
        return (torch.empty(L.iseg_convnext_mlp_tiled_bytes(Cc, 0) // 2, dtype=torch.bfloat16, device=dev),
                torch.empty(L.iseg_convnext_mlp_tiled_bytes(Cc, 1) // 2, dtype=torch.bfloat16, device=dev))

    return _prep_request(1, [w1, w2] + ([gamma] if gamma is not None else []), make)


def w_colscaled(w2, gamma):
    """bf16 copy of the 2-D kernel w2 with its columns scaled by gamma (layer scale folded into the data-gradient product)"""
    return _prep_request(0, [w2, gamma], lambda: (torch.empty(tuple(w2.shape), dtype=torch.bfloat16, device=w2.device),))[0]


def joint_kernels(wa, wb, ba=None, bb=None):
    """two 2-D kernels [C, Na], [C, Nb] on the same input (and their biases) as the operands of ONE product of width ld = Na + Nb rounded up to 8:
    (rowcat [C, ld] bf16 -- the data gradient's operand, transposed [ld, C] bf16 -- the forward product's K-contiguous operand, bias [ld] fp32),
    zero in the padding columns, valid for the current weights (re-derived with the other per-update images, csrc/mlp_fused.hip kind 2).  The
    DCNv3 layer's offset | mask projection (layers/dcn_v3/dcn_v3.py)."""
    Cc, na, nb = wa.shape[0], wa.shape[1], wb.shape[1]
    ld = (na + nb + 7) // 8 * 8

    def make():
        blob = torch.empty(2 * Cc * ld * 2 + ld * 4, dtype=torch.uint8, device=wa.device)
        rowcat = blob[:Cc * ld * 2].view(torch.bfloat16).view(Cc, ld)
        tr = blob[Cc * ld * 2:2 * Cc * ld * 2].view(torch.bfloat16).view(ld, Cc)
        bias = blob[2 * Cc * ld * 2:].view(torch.float32)
        return (rowcat, tr, bias, blob)

    params = [wa, wb] + ([ba, bb] if ba is not None and bb is not None else [])
    return _prep_request(2, params, make)[:3]


_DRY = [False]


def dry_run():
    """True while layers are being built by shape propagation only (no kernel is launched, outputs are uninitialised)"""
    return _DRY[0]


@contextlib.contextmanager
def dry_run_scope():
    prev = _DRY[0]
    _DRY[0] = True
    try:
        with torch.no_grad():
            yield
    finally:
        _DRY[0] = prev
