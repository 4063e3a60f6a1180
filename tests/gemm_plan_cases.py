"""The problems whose host-side plan (reduction split, slab count, main loop, workspace) is pinned by tests/golden/gemm_plans.json, and the
recorder of that file.

The planner queries of include/iseg_hip.h are pure host functions of the argument block: they look at the operands' ADDRESSES (alignment) and
never at what lies behind them, so the problems here carry made-up addresses and nothing is allocated or launched.

    python -m tests.gemm_plan_cases --record no_device|mi355x [--lib path/to/libiseg_hip.so] [--commit HASH]

writes one section of the golden file from the library that is built (or the one given).  Two sections, because the plan depends on the device:
without one the weight-gradient LDS-DMA forms 7 / 8 are off (their dynamic-LDS limit cannot be raised) and the CU count defaults to 256.
tests/test_gemm_plan_host.py checks `no_device`, tests/test_gemm_plan_gpu.py checks `mi355x`.
"""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_MUL_AUX = 0, 2, 5

# made-up operand addresses, 4 KiB aligned and far apart
_ADDR = {"A": 1 << 32, "B": 2 << 32, "D": 3 << 32, "bias": 4 << 32, "colscale": 5 << 32, "rowscale": 6 << 32, "residual": 7 << 32, "aux": 8 << 32,
         "pre_out": 9 << 32, "colsum_out": 10 << 32}
_POINTERS = tuple(_ADDR)


def _gemm(name, M, N, K, ak, bk, *, dtype=BF16, out=None, off=None, **fields):
    """one iseg_gemm problem: (name, GemmArgs fields).  Pointer fields are given as True (the made-up address); `off` = {field: byte offset}.
    lda / ldb / ldd default to the dense ones of the orientation."""
    f = {"M": M, "N": N, "K": K, "a_kcontig": ak, "b_kcontig": bk, "in_dtype": dtype, "out_dtype": dtype if out is None else out, "alpha": 1.0,
         "batch": 1, "batch_inner": 1, "A": True, "B": True, "D": True}
    f["lda"] = K if ak else M
    f["ldb"] = K if bk else N
    f["ldd"] = N
    f.update(fields)
    for p in _POINTERS:
        if f.get(p):
            f[p] = _ADDR[p] + (off or {}).get(p, 0)
    for p, ld in (("residual", "ldr"), ("aux", "ldaux"), ("pre_out", "ldp")):
        if f.get(p):
            f.setdefault(ld, N)
    return name, f


def _nt(name, M, N, K, **kw):      # both operands K-contiguous: dense_fwd_t, dense_dgrad
    return _gemm(name, M, N, K, 1, 1, **kw)


def _nn(name, M, N, K, **kw):      # the Keras kernel as stored: dense_fwd
    return _gemm(name, M, N, K, 1, 0, **kw)


def _tn(name, rows, C_, N, *, bias=False, **kw):      # weight gradient dW[C, N] = X[rows, C]^T dY[rows, N], fp32 out
    kw.setdefault("out", F32)
    return _gemm(name, C_, N, rows, 0, 0, colsum_out=bias, colsum_accumulate=int(bias), accumulate=1, **kw)


def _with_splits(cases, splits=(0, 1, 3)):
    out = []
    for name, f in cases:
        for s in splits:
            out.append((f"{name}/split_k={s}", dict(f, split_k=s)))
    return out


def _gemm_cases():
    cases = []
    # the four ConvNeXt-T stages: pwconv1 [C -> 4C], pwconv2 [4C -> C] forward, data gradients, weight gradients with and without the bias gradient
    stage = []
    for rows, Cc in ((262144, 96), (65536, 192), (16384, 384), (4096, 768)):
        s = f"convnext/rows={rows},C={Cc}"
        stage += [
            _nt(f"{s}/pwconv1_fwd_t", rows, 4 * Cc, Cc, bias=True, act=ACT_GELU, pre_out=True, pre_deriv=1),
            _nn(f"{s}/pwconv1_fwd", rows, 4 * Cc, Cc, bias=True, act=ACT_GELU, pre_out=True),
            _nt(f"{s}/pwconv2_fwd_t", rows, Cc, 4 * Cc, bias=True, colscale=True, residual=True),
            _nn(f"{s}/pwconv2_fwd", rows, Cc, 4 * Cc, bias=True, colscale=True, residual=True),
            _nt(f"{s}/pwconv2_dgrad", rows, 4 * Cc, Cc, act=ACT_MUL_AUX, aux=True),
            _nt(f"{s}/pwconv1_dgrad", rows, Cc, 4 * Cc),
            _tn(f"{s}/pwconv1_wgrad", rows, Cc, 4 * Cc),
            _tn(f"{s}/pwconv1_wgrad+bias", rows, Cc, 4 * Cc, bias=True),
            _tn(f"{s}/pwconv2_wgrad", rows, 4 * Cc, Cc),
            _tn(f"{s}/pwconv2_wgrad+bias", rows, 4 * Cc, Cc, bias=True),
        ]
    cases += _with_splits(stage)
    # tests/test_kernels_gpu.py::test_gemm_wgrad_splitk (x [M, Kd], dy [M, N]), both storage types
    wg = []
    for M, N, Kd in ((4096, 384, 96), (5000, 96, 384), (1030, 21, 256), (640, 768, 3072), (9000, 256, 200)):
        for dtype, tag in ((BF16, "bf16"), (F32, "f32")):
            wg.append(_tn(f"wgrad_splitk/{tag}/rows={M},C={Kd},N={N}", M, Kd, N, dtype=dtype))
    cases += _with_splits(wg)
    # tests/test_kernels_gpu.py::test_wgrad_lds_dma_pipeline, 96 x 288 and the ragged 2049-row one among them
    dma_tn = []
    for rows, Cc, N in ((16384, 1536, 384), (16384, 384, 1536), (4096, 3072, 768), (4096, 768, 3072), (2048, 136, 200), (6144, 392, 128),
                        (2176, 128, 520), (17424, 384, 1536), (8200, 768, 2304), (2049, 128, 128), (4096, 96, 384), (4096, 384, 96),
                        (8192, 112, 336), (4096, 96, 288)):
        for bias in (False, True):
            dma_tn.append(_tn(f"wgrad_dma/rows={rows},C={Cc},N={N}{'+bias' if bias else ''}", rows, Cc, N, bias=bias))
    cases += _with_splits(dma_tn)
    # the LDS-DMA pipeline's own shapes (test_gemm_dma_pipeline_*): every tile form, ragged edges, K tails, a split inside the DMA kernel
    nt = [_nt(f"nt/M={M},N={N},K={K}", M, N, K) for M, N, K in
          ((300, 64, 256), (1000, 136, 128), (7000, 384, 192), (16384, 512, 128), (25000, 264, 320), (640, 128, 2048), (300, 64, 72),
           (1000, 136, 96), (7000, 384, 112), (131072, 112, 112), (16384, 512, 200), (25000, 264, 328), (640, 128, 2040),
           (4096, 384, 1536), (4096, 256, 1024), (4096, 384, 1000), (2048, 256, 4096), (512, 128, 8192), (16384, 384, 1536), (4096, 768, 3072),
           (4096, 3072, 768), (300, 32, 256), (300, 21, 256), (300, 48, 64), (63, 128, 256), (4096, 96, 24), (4096, 96, 32))]
    cases += _with_splits(nt)
    cases += _with_splits([_nt(f"nt_f32/M={M},N={N},K={K}", M, N, K, dtype=F32) for M, N, K in ((1000, 136, 128), (640, 128, 2048), (300, 21, 256))])
    cases += _with_splits([_nt("nt_f32_out/M=640,N=128,K=2048", 640, 128, 2048, out=F32, accumulate=1, alpha=0.5),
                           _nn("nn/M=640,N=128,K=4096", 640, 128, 4096), _nn("nn/M=300,N=21,K=256", 300, 21, 256)])
    # strided batches (attention products: T = 200 tokens, d = 128, 12 = 3 x 4 problems), aligned strides and one that is not
    T, d, ld = 200, 128, 1024
    batched = dict(lda=ld, ldb=ld, ldd=T, alpha=0.125, batch=12, batch_inner=4, sa_outer=T * ld, sa_inner=d, sb_outer=T * ld, sb_inner=d,
                   sd_outer=4 * T * T, sd_inner=T * T)
    cases += _with_splits([_nt("batch/qk", T, T, d, **batched), _nt("batch/qk_stride_off", T, T, d, **dict(batched, sa_inner=d + 4)),
                           _nt("batch/long_k", 128, 128, 4096, batch=4, sa_outer=128 * 4096, sb_outer=128 * 4096, sd_outer=128 * 128),
                           _tn("batch/wgrad", 4096, 128, 128, batch=2, sa_outer=4096 * 128, sb_outer=4096 * 128, sd_outer=128 * 128)])
    # B per row group (one kernel per sample): the LDS-DMA path only
    cases += _with_splits([_nt("b_group/M=4096,N=256,K=256", 4096, 256, 256, b_group_rows=256, b_group_stride=256 * 256),
                           _nt("b_group/M=1024,N=128,K=4096", 1024, 128, 4096, b_group_rows=512, b_group_stride=128 * 4096)])
    # an operand 2 bytes off its 16-byte alignment, a fused operand off, a row stride that is no multiple of 8
    M, N, K = 7000, 384, 192
    odd = [_nt(f"misaligned/{p}+{o}", M, N, K, bias=True, residual=True, off={p: o}) for p, o in
           (("A", 2), ("B", 2), ("D", 2), ("residual", 2), ("bias", 4))]
    odd += [_nt("pitch/lda=K+4", M, N, K, lda=K + 4), _nt("pitch/ldb=K+4", M, N, K, ldb=K + 4), _nt("pitch/ldd=N+4", M, N, K, ldd=N + 4),
            _nt("pitch/ldr=N+4", M, N, K, residual=True, ldr=N + 4), _nt("pitch/lda=K+8", M, N, K, lda=K + 8),
            _tn("misaligned/wgrad_A+2", 16384, 384, 1536, off={"A": 2}), _tn("pitch/wgrad_lda=C+4", 16384, 384, 1536, lda=388),
            _tn("pitch/wgrad_ldb=N+8", 16384, 384, 1536, ldb=1544)]
    cases += _with_splits(odd)
    return cases


def _pair_cases():
    """(name, first problem, second problem): the two weight gradients of an un-fused ConvNeXt block, Z = g^T dbr [4C, C] and dW1 = x^T dh [C, 4C]"""
    pairs = []
    for rows, Cc in ((262144, 96), (65536, 192), (16384, 384), (4096, 768), (2049, 128), (16384, 136)):
        z = _tn("z", rows, 4 * Cc, Cc, bias=True)[1]
        w1 = _tn("dW1", rows, Cc, 4 * Cc, bias=True)[1]
        pairs.append((f"pair/rows={rows},C={Cc}", z, w1))
    z = _tn("z", 16384, 1536, 384, bias=True)[1]
    pairs.append(("pair/other_rows", z, _tn("dW1", 8192, 384, 1536, bias=True)[1]))
    pairs.append(("pair/first_misaligned", _tn("z", 16384, 1536, 384, bias=True, off={"A": 2})[1], _tn("dW1", 16384, 384, 1536, bias=True)[1]))
    return pairs


def _same_pad(size, k, s, d):
    out = -(-size // s)
    total = max((out - 1) * s + (k - 1) * d + 1 - size, 0)
    return out, total // 2


def _geom(name, N, H, W, Cin, Cout, k, s, d=1, groups=1, same=True):
    Ho, pt = _same_pad(H, k, s, d) if same else (H // s, 0)
    Wo, pl = _same_pad(W, k, s, d) if same else (W // s, 0)
    return name, (N, H, W, Cin, Cout, k, k, s, s, d, d, pt, pl, Ho, Wo, groups)


def _conv_cases():
    return [
        # ConvNeXt's patchify layers: the 2 x 2 / stride-2 downsampling between the stages and the 4 x 4 / stride-4 stem
        _geom("convnext/down0", 16, 128, 128, 96, 192, 2, 2), _geom("convnext/down1", 16, 64, 64, 192, 384, 2, 2),
        _geom("convnext/down2", 16, 32, 32, 384, 768, 2, 2), _geom("convnext/down2_batch1", 1, 32, 32, 384, 768, 2, 2),
        _geom("convnext/stem", 16, 512, 512, 3, 96, 4, 4), _geom("convnext/stem_8ch", 4, 256, 256, 8, 96, 4, 4),
        _geom("convnext/down_narrow", 2, 16, 16, 96, 192, 2, 2), _geom("patch/3x3s3", 2, 48, 48, 64, 128, 3, 3),
        # ResNet's strided 3 x 3 at 64 x 64 x 128, an ASPP dilated 3 x 3 at 16 x 16, plain and small layers
        _geom("resnet/3x3s2", 2, 64, 64, 128, 128, 3, 2), _geom("resnet/3x3s2_batch16", 16, 64, 64, 128, 128, 3, 2),
        _geom("aspp/3x3d6", 16, 16, 16, 768, 256, 3, 1, 6), _geom("aspp/3x3d12_batch1", 1, 16, 16, 768, 256, 3, 1, 12),
        _geom("plain/3x3", 4, 32, 32, 64, 64, 3, 1), _geom("plain/3x3_wide", 2, 64, 64, 256, 256, 3, 1), _geom("plain/3x3_cout32", 2, 16, 16, 64, 32, 3, 1),
        _geom("grouped/3x3g4", 2, 32, 32, 128, 128, 3, 1, 1, 4), _geom("plain/1x7", 1, 8, 8, 512, 512, 7, 1),
    ]


GEMM_CASES = _gemm_cases()
PAIR_CASES = _pair_cases()
CONV_CASES = _conv_cases()


def gemm_args(hip, fields):
    g = hip.GemmArgs()
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def answers(hip, lib):
    """what the built library plans for every case: {"gemm": {name: row}, "pairs": {name: row}, "conv": {name: row}}"""
    out = {"gemm": {}, "pairs": {}, "conv": {}}
    for name, f in GEMM_CASES:
        g = C.byref(gemm_args(hip, f))
        out["gemm"][name] = {"splits": int(lib.iseg_gemm_splits(g)), "slabs": int(lib.iseg_gemm_slabs(g)), "variant": int(lib.iseg_gemm_variant(g)),
                             "workspace": int(lib.iseg_gemm_workspace_bytes(g))}
    for name, f0, f1 in PAIR_CASES:
        out["pairs"][name] = {"pair_splits": int(lib.iseg_gemm_tn_pair_splits(C.byref(gemm_args(hip, f0)), C.byref(gemm_args(hip, f1))))}
    for name, geom in CONV_CASES:
        g = C.byref(hip.ConvGeom(*geom))
        out["conv"][name] = {"workspace": [int(lib.iseg_conv2d_igemm_workspace_bytes(g, p)) for p in range(4)],
                             "patch_supported": [int(lib.iseg_conv2d_patch_supported(g, BF16, p)) for p in range(3)],
                             "fwd_kt_supported": int(lib.iseg_conv2d_igemm_fwd_kt_supported(g, BF16))}
    return out


def knobs_set():
    """the ISEG_GEMM_DMA_* variables in the environment: the library reads them once and plans differently under them"""
    return sorted(k for k in os.environ if k.startswith("ISEG_GEMM_DMA_"))


def golden(section):
    with open(GOLDEN) as f:
        return json.load(f)[section]


def mismatches(want, got):
    """every case must have a recorded row (a missing one is a failure, not a skip) and every recorded answer must be the planned one"""
    bad = []
    for kind, rows in got.items():
        for name, row in rows.items():
            rec = want.get(kind, {}).get(name)
            if rec is None:
                bad.append(f"{kind} {name}: no recorded row")
            elif rec != row:
                bad.append(f"{kind} {name}: recorded {rec}, planned {row}")
    return bad


def variants(section, orientation):
    """iseg_gemm_variant answers recorded for the bf16 problems of one orientation (a_kcontig, b_kcontig)"""
    fields = dict(GEMM_CASES)
    return {row["variant"] for name, row in section["gemm"].items()
            if (fields[name]["a_kcontig"], fields[name]["b_kcontig"]) == orientation and fields[name]["in_dtype"] == BF16}


def load_library(path=None):
    """(the _hip module, the CDLL): the library that is built, or another build of it at `path` (recording from an earlier commit)"""
    from iseg_amd import _hip

    if path is None:
        if not os.path.exists(_hip.LIB_PATH):
            from iseg_amd.build import build

            build(verbose=False)
        return _hip, _hip.lib()
    import torch  # noqa: F401  (one HIP runtime per process: see _hip.lib)

    dll = C.CDLL(path)
    for name, (res, args) in _hip.SIGNATURES.items():
        fn = getattr(dll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return _hip, dll


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", required=True, choices=["no_device", "mi355x"])
    ap.add_argument("--lib", default=None, help="record from this build of libiseg_hip.so instead of the one in the tree")
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built at")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args(argv)
    if knobs_set():
        raise SystemExit(f"unset {knobs_set()} first: the recorded plans are those of the defaults")
    import torch

    if (a.record == "mi355x") != torch.cuda.is_available():
        raise SystemExit(f"section {a.record} is recorded {'on the GPU machine' if a.record == 'mi355x' else 'where there is no GPU'}")
    hip, lib = load_library(a.lib)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.record] = answers(hip, lib)
    if a.commit:
        doc.setdefault("recorded_at_commit", {})[a.record] = a.commit
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.record}: {sum(len(v) for v in doc[a.record].values())} rows -> {a.out}")


if __name__ == "__main__":
    main()
