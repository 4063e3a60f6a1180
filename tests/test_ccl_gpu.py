"""Connected-components labelling through the HIP kernels (csrc/ccl.hip), by the C ABI wrapper and by ops.ccl.label_components, against the
restatement tests/ccl_ref.py.  The result is integers: every comparison is torch.equal on labels and counts, no tolerance anywhere.

Tiles are 64 x 16 pixels, so the shapes cross tile seams in both directions with ragged edges (33 x 65, 37 x 53, 97 x 131), hit them
exactly (64 x 64) or degenerate to a row or a column of tiles (1 x 300, 300 x 1).
"""
import functools

import numpy as np
import pytest
import torch

from tests import ccl_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (33, 65), (37, 53), (97, 131)]
TILE_W, TILE_H = 64, 16


# ---- patterns: (H, W, image index) -> [H, W] int32 in {0, 1} ------------------------------------------------------------------------------
def _random(density):
    def make(H, W, k):
        return (np.random.default_rng([int(density * 100), H, W, k]).random((H, W)) < density).astype(np.int32)
    return make


def serpentine(H, W, k):
    """full rows alternating with one connecting pixel at alternating ends: ONE component whose parent chain is as long as the image"""
    m = np.zeros((H, W), np.int32)
    m[0::2] = 1
    for j, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if (j + k) % 2 == 0 else 0] = 1
    return m


def spiral(H, W, k):
    """a rectangular spiral: a one-pixel path from a corner inwards that turns right whenever it would run into the border or into itself
    (it keeps one pixel of background between its windings); mirrored in every second image"""
    m = np.zeros((H, W), np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                break
            dy, dx = dx, -dy      # right -> down -> left -> up
        else:
            return m[:, ::-1].copy() if k % 2 else m
        y, x = ny, nx
        m[y, x] = 1


def comb(H, W, k):
    """vertical teeth joined only along the last row: the numbering is decided at the top, the merges happen at the bottom"""
    m = np.zeros((H, W), np.int32)
    m[:, 0::2] = 1
    m[H - 1] = 1
    return m


def checkerboard(H, W, k):
    return ((np.add.outer(np.arange(H), np.arange(W)) + k) % 2 == 0).astype(np.int32)


def diagonal(H, W, k):
    m = np.zeros((H, W), np.int32)
    n = min(H, W)
    m[np.arange(n), np.arange(n)] = 1
    return m


def ones(H, W, k):
    return np.ones((H, W), np.int32)


def zeros(H, W, k):
    return np.zeros((H, W), np.int32)


def one_pixel(H, W, k):
    m = np.zeros((H, W), np.int32)
    m[(H - 1) // (k + 1), (W - 1) // (k + 1)] = 1
    return m


def two_distant_pixels(H, W, k):
    m = np.zeros((H, W), np.int32)
    m[0, 0] = m[H - 1, W - 1] = 1
    return m


def tile_corner(H, W, k):
    """two blobs, upper-left and lower-right of a tile corner, joined by a single pixel placed exactly on that corner"""
    cy, cx = (TILE_H, TILE_W) if H > TILE_H and W > TILE_W else (H // 2, W // 2)
    m = np.zeros((H, W), np.int32)
    m[:cy, :cx] = 1                 # ends in the last row and column of the tile before the corner
    m[cy:, cx:] = 1                 # begins in the first row and column of the tile behind it: the two touch by a diagonal only
    if cx >= 1:
        m[cy, cx - 1] = 1           # the one pixel: below the first blob's last row, left of the second blob's first column
    return m


PATTERNS = {"random30": _random(0.3), "random59": _random(0.59), "random90": _random(0.9), "serpentine": serpentine, "spiral": spiral, "comb": comb,
            "checkerboard": checkerboard, "diagonal": diagonal, "ones": ones, "zeros": zeros, "one_pixel": one_pixel,
            "two_distant_pixels": two_distant_pixels, "tile_corner": tile_corner}


@functools.lru_cache(maxsize=None)
def _case(pattern, H, W, N):
    """(mask [N,H,W], labels, counts) as read-only numpy arrays; computed once per session"""
    m = np.stack([PATTERNS[pattern](H, W, k) for k in range(N)])
    labels, counts = R.label_components(m)
    for a in (m, labels, counts):
        a.setflags(write=False)
    return m, labels, counts


def _run(mask, dtype=torch.int32):
    from iseg_amd import kernels as K

    labels, counts = K.ccl_label(torch.from_numpy(np.array(mask)).to(dtype).cuda())
    torch.cuda.synchronize()
    return labels.cpu(), counts.cpu()


def _assert_equal(got, want, what):
    labels, counts = got
    wl, wc = torch.from_numpy(np.array(want[0])), torch.from_numpy(np.array(want[1]))
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    assert torch.equal(counts, wc), f"{what}: counts {counts.tolist()} != {wc.tolist()}"
    if not torch.equal(labels, wl):
        bad = torch.nonzero(labels != wl)
        n, y, x = bad[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} labels differ; first at image {n} ({y}, {x}): {int(labels[n, y, x])} != {int(wl[n, y, x])}")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_parity_with_the_restatement(cuda, pattern, shape, N):
    m, labels, counts = _case(pattern, *shape, N)
    _assert_equal(_run(m), (labels, counts), f"{pattern} {shape} N={N}")


def test_batch_isolation(cuda):
    """image n ends with a full row, image n + 1 begins with one; an empty image between full ones: counts are per image, no label leaks"""
    H, W = 37, 53
    m = np.zeros((5, H, W), np.int32)
    m[0, H - 1] = 1
    m[1, 0] = 1
    m[2] = 1
    m[4] = 1
    m[4, 5] = 0      # two components in the last image
    want = R.label_components(m)
    assert want[1].tolist() == [1, 1, 1, 0, 2]
    _assert_equal(_run(m), want, "batch isolation")


@pytest.mark.parametrize("shape", [(37, 53), (97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_byte_masks_and_nonzero_values(cuda, shape):
    m, labels, counts = _case("random59", *shape, 3)
    _assert_equal(_run(m * 255, torch.uint8), (labels, counts), "uint8 0/255")
    _assert_equal(_run(m, torch.bool), (labels, counts), "bool")
    odd = np.where(np.random.default_rng(3).random(m.shape) < 0.5, 2, -7).astype(np.int32) * m
    assert set(np.unique(odd)) == {0, 2, -7}
    _assert_equal(_run(odd), (labels, counts), "int32 {0, 2, -7}")


def test_ops_label_components(cuda):
    from iseg_amd import kernels as K
    from iseg_amd.ops import ccl

    m, labels, counts = _case("random59", 97, 131, 3)
    M = torch.from_numpy(np.array(m)).cuda()
    kl, kc = K.ccl_label(M)
    got = ccl.label_components(M)
    assert torch.equal(got, kl) and got.dtype == torch.int32 and got.shape == M.shape
    gl, gc = ccl.label_components(M, return_counts=True)
    assert torch.equal(gl, kl) and torch.equal(gc, kc) and torch.equal(gc, gl.amax((1, 2)))
    _assert_equal((gl.cpu(), gc.cpu()), (labels, counts), "ops.ccl.label_components")
    one = ccl.label_components(M[1])      # [H, W]: one image
    assert one.shape == M[1].shape and torch.equal(one, kl[1])
    # caller-owned outputs
    L, Cn = torch.empty_like(kl), torch.empty_like(kc)
    rl, rc = K.ccl_label(M, labels=L, counts=Cn)
    assert rl is L and rc is Cn and torch.equal(L, kl) and torch.equal(Cn, kc)


def test_two_calls_are_bit_identical(cuda):
    for pattern in ("random59", "serpentine"):
        m = _case(pattern, 97, 131, 3)[0]
        a, b = _run(m), _run(m)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_inside_guard_bands(cuda):
    """labels, counts and row_base at exact size between poison, at addresses = 16 (mod 512); row_base may hold anything afterwards"""
    from iseg_amd import kernels as K
    from tests import guarded_memory as GM

    m, labels, counts = _case("random59", 97, 131, 2)
    arena = GM.Arena(cuda, 16 << 20)
    M = arena.alloc(m.shape, torch.int32, "operand", name="mask")
    M.copy_(torch.from_numpy(np.array(m)))
    with GM.guarded(arena):
        gl, gc = K.ccl_label(M)
    arena.check()
    assert [r.shape for r in arena.records[1:]] == [(2, 97, 131), (2,), (2, 97)] and gl.data_ptr() % 512 == 16
    _assert_equal((gl.cpu(), gc.cpu()), (labels, counts), "guarded")


def test_graph_replay_follows_the_input_buffer(cuda):
    """a capture fails on any host read, copy or allocation inside the launcher; each replay labels what the static buffer then holds"""
    from iseg_amd import kernels as K

    first, second = _case("random59", 97, 131, 2), _case("comb", 97, 131, 2)
    buf = torch.zeros(2, 97, 131, dtype=torch.int32, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.ccl_label(buf)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        labels, counts = K.ccl_label(buf)
    for m, wl, wc in (first, second):
        buf.copy_(torch.from_numpy(np.array(m)))
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal((labels.cpu(), counts.cpu()), (wl, wc), "replay")


def test_one_larger_case(cuda):
    m = (np.random.default_rng(512).random((2, 512, 512)) < 0.59).astype(np.int32)
    try:
        from scipy import ndimage
    except ImportError:
        want = R.label_components(m)
    else:
        done = [ndimage.label(x) for x in m]      # default structure: 4-connectivity, raster order of the first pixel
        want = (np.stack([d[0] for d in done]).astype(np.int32), np.array([d[1] for d in done], np.int32))
    _assert_equal(_run(m), want, "2x512x512 at 0.59")
