"""Connected-components labelling on the host: the restatement tests/ccl_ref.py on hand-written answers and against scipy, the C ABI entry
iseg_ccl_label (declared, exported, bound, no workspace function), and what the wrapper and the launcher refuse before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ccl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(rows):
    return np.array([[int(c != ".") for c in r] for r in rows], np.int32)


def test_u_shape_joined_only_through_the_bottom_row():
    """the first raster pixel (the left arm's top) reaches the right arm only through the last row; the pixel between the arms is met second"""
    got, n = R.label_image(_img(["#...#",
                                 "#.#.#",
                                 "#...#",
                                 "#####"]))
    want = np.array([[1, 0, 0, 0, 1],
                     [1, 0, 2, 0, 1],
                     [1, 0, 0, 0, 1],
                     [1, 1, 1, 1, 1]], np.int32)
    assert n == 2 and np.array_equal(got, want) and got.dtype == np.int32


def test_diagonal_line_is_one_component_per_pixel():
    got, n = R.label_image(np.eye(6, dtype=np.int32))
    assert n == 6 and np.array_equal(got, np.diag(np.arange(1, 7)).astype(np.int32))


def test_rows_do_not_wrap():
    img = np.zeros((4, 5), np.int32)
    img[:, 0] = img[:, -1] = 1
    got, n = R.label_image(img)
    want = np.zeros((4, 5), np.int32)
    want[:, 0], want[:, -1] = 1, 2
    assert n == 2 and np.array_equal(got, want)


def test_all_zeros_one_pixel_all_ones():
    z = np.zeros((3, 4), np.int32)
    got, n = R.label_image(z)
    assert n == 0 and np.array_equal(got, z)
    one = z.copy()
    one[2, 1] = 1
    got, n = R.label_image(one)
    assert n == 1 and np.array_equal(got, one)      # the reference's reduce_sum <= 1 shortcut returns the input: the same thing
    got, n = R.label_image(np.ones((3, 4), np.int32))
    assert n == 1 and np.array_equal(got, np.ones((3, 4), np.int32))


def test_batch_and_nonzero_values():
    m = np.zeros((2, 2, 3), np.int32)
    m[0, 0, 0], m[0, 0, 2], m[1, 1, 1] = 2, -7, 255
    labels, counts = R.label_components(m)
    assert counts.tolist() == [2, 1] and labels[0].tolist() == [[1, 0, 2], [0, 0, 0]] and labels[1].tolist() == [[0, 0, 0], [0, 1, 0]]


@pytest.mark.parametrize("density", [0.3, 0.59, 0.9])
def test_restatement_agrees_with_scipy(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100))
    for H, W in ((1, 17), (23, 1), (19, 31), (40, 40)):
        for _ in range(5):
            m = (rng.random((H, W)) < density).astype(np.int32)
            want, n = ndimage.label(m)      # default structure: 4-connectivity, numbered in raster order of the first pixel
            got, k = R.label_image(m)
            assert k == n and np.array_equal(got, want)


def test_gpu_patterns_are_what_they_claim():
    """the generators of tests/test_ccl_gpu.py: one serpentine, one spiral, one comb; ceil(HW/2) squares; a corner pixel that is the only link"""
    from tests import test_ccl_gpu as T

    for H, W in ((33, 65), (97, 131)):
        for one in ("serpentine", "spiral", "comb"):
            assert T._case(one, H, W, 3)[2].tolist() == [1, 1, 1], one
        assert T._case("checkerboard", H, W, 1)[2].tolist() == [(H * W + 1) // 2]
        assert T._case("diagonal", H, W, 1)[2].tolist() == [min(H, W)]
        m = np.array(T._case("tile_corner", H, W, 1)[0][0])
        assert R.label_image(m)[1] == 1
        m[T.TILE_H, T.TILE_W - 1] = 0
        assert R.label_image(m)[1] == 2
    s = T._case("spiral", 37, 53, 1)[0][0]
    assert 0.3 * s.size < s.sum() < 0.7 * s.size


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "iseg_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def hip():
    from iseg_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    _hip.lib()
    return _hip


def test_entry_point_is_declared_exported_and_bound(hip):
    assert re.search(r"\bint\s+iseg_ccl_label\s*\(", _header())
    assert hasattr(C.CDLL(hip.LIB_PATH), "iseg_ccl_label")
    res, args = hip.SIGNATURES["iseg_ccl_label"]
    assert res is C.c_int and len(args) == 9
    from iseg_amd import build

    assert "ccl.hip" in build.SOURCES


def test_no_workspace_function(hip):
    """all memory is three typed, shape-sized buffers: nothing to add to the workspace ledger"""
    names = re.findall(r"\b(iseg_[a-z0-9_]+)\s*\(", _header()) + list(hip.SIGNATURES)
    assert not [n for n in names if "ccl" in n and n.endswith("_workspace_bytes")]
    assert [n for n in set(names) if "ccl" in n] == ["iseg_ccl_label"]


def test_ops_package_exports_ccl():
    import iseg_amd.ops as ops
    from iseg_amd.ops.ccl import label_components

    assert ops.ccl.label_components is label_components


def test_wrapper_refuses_host_tensors_other_dtypes_and_other_ranks(hip):
    from iseg_amd import kernels
    from iseg_amd.ops import ccl

    for f in (kernels.ccl_label, ccl.label_components):
        with pytest.raises(hip.HipCallError):
            f(torch.zeros(2, 4, 4, dtype=torch.int32))
        with pytest.raises(hip.HipCallError):
            f(torch.zeros(4, 4, dtype=torch.uint8))
        with pytest.raises(TypeError):
            f(torch.zeros(2, 4, 4))
        with pytest.raises(TypeError):
            f(torch.zeros(2, 4, 4, dtype=torch.int64))
        with pytest.raises(ValueError):
            f(torch.zeros(1, 2, 4, 4, dtype=torch.int32))
        with pytest.raises(ValueError):
            f(torch.zeros(4, dtype=torch.bool))


class Buf:
    """a zeroed, 256-byte aligned host buffer"""

    def __init__(self, nbytes=4096):
        self.raw = C.create_string_buffer(nbytes + 256)
        self.ptr = (C.addressof(self.raw) + 255) // 256 * 256


REFUSED = {
    "H=0": dict(H=0),
    "W=0": dict(W=0),
    "H=16385": dict(H=16385),
    "W=16385": dict(W=16385),
    "N=0": dict(N=0),
    "N=65536": dict(N=65536),
    "mask==labels": dict(alias=True),
    "null mask": dict(null="mask"),
    "null labels": dict(null="labels"),
    "null counts": dict(null="counts"),
    "null row_base": dict(null="row_base"),
}


@pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to the launcher: only where no kernel could ever receive them")
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_launcher_refuses_before_any_launch(hip, case):
    """ISEG_STATUS_ARG, with a message that names the entry point, for arguments outside the contract; both mask types"""
    kw = REFUSED[case]
    for u8 in (0, 1):
        p = dict(mask=Buf().ptr, labels=Buf().ptr, counts=Buf().ptr, row_base=Buf().ptr)
        if kw.get("alias"):
            p["mask"] = p["labels"]
        if kw.get("null"):
            p[kw["null"]] = None
        status = hip.lib().iseg_ccl_label(p["mask"], u8, kw.get("N", 1), kw.get("H", 4), kw.get("W", 4), p["labels"], p["counts"], p["row_base"], None)
        message = hip.last_error()
        assert status == -1, (case, status, message)
        assert message.startswith("iseg_ccl_label:"), message
