"""What every launcher checks before it touches the device: the storage dtype (common.h by_dtype) and the workspace (ISEG_NEED_WORKSPACE).

The calls pass small HOST buffers, so a launcher that wrongly got past its checks must never get the chance to hand them to a kernel: the module
skips itself where a GPU is present.  Without one the refusals under test come back before any launch.

(a) one entry point per launcher file that dispatches on a storage type, otherwise valid arguments, dtype = 2: status -1 (ISEG_STATUS_ARG) and
    a message that names the entry point and the dtype.  mask_loss.hip takes no storage dtype (fp32 logits only) and has no case.
(b) a null workspace with a sufficient byte count: status -4 (ISEG_STATUS_WORKSPACE) from the entry point itself.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to launchers: only where no kernel could ever receive them")

BAD = 2      # neither ISEG_F32 (0) nor ISEG_BF16 (1)
GELU = 2     # ISEG_ACT_GELU


@pytest.fixture(scope="module")
def hip():
    from iseg_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    _hip.lib()
    return _hip


class Buf:
    """a zeroed, 256-byte aligned host buffer"""

    def __init__(self, nbytes=4096):
        self.raw = C.create_string_buffer(nbytes + 256)
        self.ptr = (C.addressof(self.raw) + 255) // 256 * 256
        self.nbytes = nbytes


def _bufs(n):
    return [Buf() for _ in range(n)]


def _bad_dtype_calls():
    """name -> (lib) -> status; every geometry is the smallest the launcher accepts (C = 8, a few pixels)"""
    def cast(lib, b):
        return lib.iseg_cast(b[0].ptr, BAD, b[1].ptr, 0, 64, None)

    def add_relu(lib, b):
        return lib.iseg_add_relu(b[0].ptr, b[1].ptr, b[2].ptr, 64, BAD, None)

    def bn_apply_fwd(lib, b):
        return lib.iseg_bn_apply_fwd(b[0].ptr, 8, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, 8, 4, 8, 0, BAD, None)

    def clip_fwd(lib, b):
        return lib.iseg_clip_fwd(b[0].ptr, b[1].ptr, 64, 0.0, 1.0, BAD, None)

    def resize_bilinear_ac_fwd(lib, b):
        return lib.iseg_resize_bilinear_ac_fwd(b[0].ptr, BAD, b[1].ptr, 0, 1, 2, 2, 4, 4, 8, None)

    def scale_cols(lib, b):
        return lib.iseg_scale_cols(b[0].ptr, b[1].ptr, b[2].ptr, 4, 8, BAD, None)

    def defattn_fwd(lib, b):
        return lib.iseg_defattn_fwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, 1, 2, 2, 1, 4, 8, 2.0, BAD, None)

    def glu_fwd(lib, b):
        return lib.iseg_glu_fwd(b[0].ptr, 8, b[1].ptr, 8, b[2].ptr, 8, 4, 8, GELU, BAD, None)

    def grn_fwd(lib, b):
        need = lib.iseg_grn_workspace_bytes(1, 4, 8)
        ws = Buf(need)
        return lib.iseg_grn_fwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, 1, 4, 8, 1e-6, BAD, ws.ptr, need, None)

    def upsample_ce(lib, b):
        need = lib.iseg_upsample_ce_workspace_bytes(1, 2, 2, 4, 4, 8)
        ws = Buf(need)
        return lib.iseg_upsample_ce(b[0].ptr, BAD, b[1].ptr, None, 1, 2, 2, 4, 4, 8, 255, b[2].ptr, 1.0, None, 1.0, None, ws.ptr, need, None)

    def bn_swish_gate_fwd(lib, b):
        return lib.iseg_bn_swish_gate_fwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, b[6].ptr, 1, 4, 8, BAD, None)

    def relu_dwconv3_stats(lib, b):
        return lib.iseg_relu_dwconv3_stats(b[0].ptr, b[1].ptr, b[2].ptr, None, 1, 4, 4, 8, 1, 1, BAD, None, 0, None)

    def resblock_tail_fwd(lib, b):
        return lib.iseg_resblock_tail_fwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, None, None, None, None, b[6].ptr, 1, 4, 4, 8, 1,
                                          BAD, None)

    def dwconv2d_fwd(lib, b):
        return lib.iseg_dwconv2d_fwd(b[0].ptr, b[1].ptr, None, None, b[2].ptr, 1, 4, 4, 8, 3, 1, 1, 1, 0, BAD, None)

    def dwconv2d_strided_fwd(lib, b):
        return lib.iseg_dwconv2d_strided_fwd(b[0].ptr, b[1].ptr, None, b[2].ptr, 1, 4, 4, 8, 3, 2, 1, 0, 0, 2, 2, BAD, None)

    return {  # source file: (entry point, call)
        "elementwise.hip": ("iseg_cast", cast),
        "misc.hip": ("iseg_add_relu", add_relu),
        "norm.hip": ("iseg_bn_apply_fwd", bn_apply_fwd),
        "attention.hip": ("iseg_clip_fwd", clip_fwd),
        "resize.hip": ("iseg_resize_bilinear_ac_fwd", resize_bilinear_ac_fwd),
        "dcnv3.hip": ("iseg_scale_cols", scale_cols),
        "defattn.hip": ("iseg_defattn_fwd", defattn_fwd),
        "eva.hip": ("iseg_glu_fwd", glu_fwd),
        "grn.hip": ("iseg_grn_fwd", grn_fwd),
        "loss.hip": ("iseg_upsample_ce", upsample_ce),
        "mbconv.hip": ("iseg_bn_swish_gate_fwd", bn_swish_gate_fwd),
        "sepconv.hip": ("iseg_relu_dwconv3_stats", relu_dwconv3_stats),
        "resblock.hip": ("iseg_resblock_tail_fwd", resblock_tail_fwd),
        "dwconv.hip": ("iseg_dwconv2d_fwd", dwconv2d_fwd),
        "dwconv_strided.hip": ("iseg_dwconv2d_strided_fwd", dwconv2d_strided_fwd),
    }


@pytest.mark.parametrize("source", sorted(_bad_dtype_calls()))
def test_unknown_dtype_is_an_argument_error(hip, source):
    entry, call = _bad_dtype_calls()[source]
    status = call(hip.lib(), _bufs(8))
    message = hip.last_error()
    assert status == -1, (entry, status, message)
    assert message.startswith(entry + ":") and "dtype %d" % BAD in message, message


def _null_workspace_calls():
    def bnfold_dwconv3_relu_bwd(lib, b):
        need = lib.iseg_bnfold_dwconv3_relu_bwd_workspace_bytes(1, 4, 4, 8, 1, 1)
        assert need > 0
        return lib.iseg_bnfold_dwconv3_relu_bwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, None, None, None, None, 1.0, 0, b[4].ptr, b[5].ptr, 1, 4, 4, 8,
                                                1, 1, 0, None, need, None)

    def colsum(lib, b):
        return lib.iseg_colsum(b[0].ptr, 8, 0, 1, 4, 8, b[1].ptr, 1.0, 0, 0, None, 1 << 20, None)

    def rmsnorm_bwd(lib, b):
        return lib.iseg_rmsnorm_bwd(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, 0, 4, 8, 0, None, 1 << 20, None)

    return {"iseg_bnfold_dwconv3_relu_bwd": bnfold_dwconv3_relu_bwd, "iseg_colsum": colsum, "iseg_rmsnorm_bwd": rmsnorm_bwd}


@pytest.mark.parametrize("entry", sorted(_null_workspace_calls()))
def test_null_workspace_is_refused_whatever_its_size(hip, entry):
    status = _null_workspace_calls()[entry](hip.lib(), _bufs(8))
    message = hip.last_error()
    assert status == -4, (entry, status, message)
    assert message.startswith(entry + ":") and "workspace bytes" in message, message
