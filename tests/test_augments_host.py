"""Host side of data_process/augments/ and AugmentationsPipeLine (no GPU): constructor signatures against the reference's, the random
decisions' ranges, the rotation matrix, the pipeline's order -- and the numpy restatement of the projective transform (projective_ref.py)
on answers that need no trigonometry."""
import inspect

import numpy as np
import pytest

from tests import projective_ref as R

REQ = inspect.Parameter.empty
# augments/*.py of the reference: (parameter, default) in order; every class here adds seed=0 behind them
SIGNATURES = {
    "DataAugmentationBase": [("name", None)],
    "ResizeAugment": [("max_resize_height", REQ), ("max_resize_width", REQ), ("name", None)],
    "RandomScaleAugment": [("min_scale_factor", 0.5), ("max_scale_factor", 2.0), ("scale_factor_step_size", 0.1), ("break_aspect_ratio", False),
                           ("name", None)],
    "PadAugment": [("target_height", REQ), ("target_width", REQ), ("image_pad_value", [127.5, 127.5, 127.5]), ("label_pad_value", 255),
                   ("name", None)],
    "PadToOddAugment": [("image_pad_value", [127.5, 127.5, 127.5]), ("label_pad_value", 255), ("name", None)],
    "RandomCropAugment": [("crop_height", 513), ("crop_width", 513), ("name", None)],
    "RandomFlipAugment": [("prob_of_flip", 0.5), ("name", None)],
    "RandomErasingAugment": [("prob", 0.25), ("min_area_size", 0), ("max_area_size", 0.25), ("min_area_count", 1), ("max_area_count", 3),
                             ("fill_constant_color", [0, 0, 0]), ("use_fill_noise_color", False), ("ignore_label", 255), ("name", None)],
    "LambdaAugment": [("fn", REQ), ("name", None)],
    "RandomBrightnessAugment": [("max_delta", 32), ("execute_prob", 0.5), ("name", None)],
    "RandomContrastAugment": [("lower", 0.5), ("upper", 1.5), ("execute_prob", 0.5), ("name", None)],
    "RandomHueAugment": [("max_delta", 0.1), ("execute_prob", 0.5), ("name", None)],
    "RandomSaturationAugment": [("lower", 0.9), ("upper", 1.1), ("execute_prob", 0.5), ("name", None)],
    "RandomPhotoMetricDistortions": [("name", None)],
    "RandomNoisyEvalAugment": [("noise_level", 0), ("name", None)],
    "RandomJEPGQualityAugment": [("name", None)],
    "RandomRotateAugment": [("prob_of_rotate", 0.5), ("fill_constant_color", [0, 0, 0]), ("ignore_label", 255), ("name", None)],
}
# what `from iseg.data_process.augments import *` gives in the reference (augments/__init__.py)
REFERENCE_EXPORTS = ["ResizeAugment", "RandomScaleAugment", "PadAugment", "RandomCropAugment", "RandomFlipAugment", "RandomBrightnessAugment",
                     "RandomContrastAugment", "RandomHueAugment", "RandomSaturationAugment", "RandomPhotoMetricDistortions",
                     "RandomErasingAugment", "RandomJEPGQualityAugment", "RandomNoisyEvalAugment", "RandomRotateAugment"]


# ---- projective_ref.py itself ---------------------------------------------------------------------------------------------------------
def _image(H, W, C=3, seed=0):
    return np.random.default_rng(seed).uniform(0, 255, (H, W, C)).astype(np.float32)


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_ref_identity_returns_the_input_bit_for_bit(interpolation):
    img = _image(5, 7)
    out = R.projective_transform(img, [1, 0, 0, 0, 1, 0, 0, 0], interpolation, fill=-1.0)
    assert np.array_equal(out, img.astype(np.float64))


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_ref_integer_shift_leaves_a_fill_border(interpolation):
    img = _image(6, 8)
    out = R.projective_transform(img, [1, 0, 2, 0, 1, -1, 0, 0], interpolation, fill=-7.0)      # out(y, x) = img(y - 1, x + 2)
    want = np.full((6, 8, 3), -7.0)
    want[1:, :6] = img[:5, 2:]
    assert np.array_equal(out, want)


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_ref_quarter_turn_is_rot90(interpolation):
    W = 6
    img = _image(W, W)
    out = R.projective_transform(img, [0, -1, W - 1, 1, 0, 0, 0, 0], interpolation, fill=-1.0)  # out(y, x) = img(x, W - 1 - y)
    assert np.array_equal(out, np.rot90(img.astype(np.float64), k=1))       # rot90(m)[i, j] = m[j, W - 1 - i]: counterclockwise
    assert not np.array_equal(out, np.rot90(img.astype(np.float64), k=-1))


def test_ref_zero_projection_gives_the_fill_value():
    img = _image(4, 4)
    out = R.projective_transform(img, [1, 0, 0, 0, 1, 0, -0.5, 0], "bilinear", fill=-3.0)       # k = 1 - x / 2: 0 at x = 2
    assert np.all(out[:, 2] == -3.0) and np.array_equal(out[:, 0], img[:, 0].astype(np.float64))
    out = R.projective_transform(img, [1, 0, 0, 0, 1, 0, -0.5, 0], "nearest", fill=-3.0)
    assert np.all(out[:, 2] == -3.0)


def test_ref_nearest_rounds_half_away_from_zero():
    img = np.arange(6, dtype=np.float32).reshape(1, 6, 1)
    out = R.projective_transform(img, [1, 0, 2.5, 0, 1, 0, 0, 0], "nearest", fill=-1.0)          # x' = x + 2.5
    assert out[0, 0, 0] == 3.0 and out[0, 2, 0] == 5.0 and out[0, 3, 0] == -1.0                  # 2.5 -> 3 (not the even 2); 5.5 -> 6: outside
    out = R.projective_transform(img, [1, 0, -0.5, 0, 1, 0, 0, 0], "nearest", fill=-1.0)         # x' = x - 0.5
    assert out[0, 0, 0] == -1.0 and out[0, 1, 0] == 1.0                                          # -0.5 -> -1: outside; 0.5 -> 1
    assert np.array_equal(R.round_half_away(np.float32([0.49999997, -0.49999997, 1.5, -1.5])), [0.0, -0.0, 2.0, -2.0])


def test_ref_huge_and_non_finite_coordinates_are_outside():
    img = _image(3, 4)
    for t in ([1, 0, 1e9, 0, 1, 0, 0, 0], [1, 0, np.inf, 0, 1, 0, 0, 0], [1, 0, np.nan, 0, 1, 0, 0, 0]):
        for interpolation in ("nearest", "bilinear"):
            assert np.all(R.projective_transform(img, t, interpolation, fill=-2.0) == -2.0)


def test_ref_coordinates_are_float32_in_the_stated_order():
    t = np.float32([0.9553365, -0.29552022, 3.7, 0.29552022, 0.9553365, -1.3, 1e-3, -2e-3])
    sx, sy, valid = R.source_coords(t, 9, 11)
    assert sx.dtype == np.float32 and valid.all()
    x, y = np.float32(7), np.float32(5)
    k = np.float32(np.float32(np.float32(t[6] * x) + np.float32(t[7] * y)) + np.float32(1))
    want = np.float32(np.float32(np.float32(np.float32(t[0] * x) + np.float32(t[1] * y)) + t[2]) / k)
    assert sx[5, 7] == want


# ---- the package --------------------------------------------------------------------------------------------------------------------------
def test_constructor_signatures_equal_the_reference():
    from iseg_amd.data_process import augments as A

    for cls_name, want in SIGNATURES.items():
        params = list(inspect.signature(getattr(A, cls_name).__init__).parameters.values())[1:]
        got = [(p.name, p.default) for p in params]
        assert got == want + [("seed", 0)], (cls_name, got)
        assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params), cls_name
    for name in REFERENCE_EXPORTS + ["DataAugmentationBase"]:
        assert name in A.__all__ and inspect.isclass(getattr(A, name))
    scope = {}
    exec("from iseg_amd.data_process.augments import *", scope)
    assert all(name in scope for name in REFERENCE_EXPORTS)
    from iseg_amd.data_process import pipeline as P

    assert all(hasattr(P, name) for name in REFERENCE_EXPORTS)      # the reference's pipeline.py star-imports the augments
    sig = inspect.signature(P.AugmentationsPipeLine.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("target_height", None), ("target_width", None), ("augments", []), ("perform_post_process", True), ("name", None)]


def test_names_default_to_the_class_name_and_call_calls_call():
    from iseg_amd.data_process.augments import DataAugmentationBase, LambdaAugment, RandomFlipAugment, random_execute_helper

    assert DataAugmentationBase().name == "DataAugmentationBase" and RandomFlipAugment().name == "RandomFlipAugment"
    assert RandomFlipAugment(name="flip").name == "flip"
    assert LambdaAugment(lambda a, b: (b, a))(1, 2) == (2, 1)
    rng = np.random.default_rng(0)
    assert random_execute_helper(1.0, lambda: "a", lambda: "b", rng) == "a"
    assert random_execute_helper(0.0, lambda: "a", lambda: "b", rng) == "b"
    picks = [random_execute_helper(0.3, lambda: 1, lambda: 0, rng) for _ in range(2000)]
    assert 0.25 < np.mean(picks) < 0.35


def test_rotation_matrix_hand_values():
    from iseg_amd.data_process.augments.random_rotate_augment import get_rotation_matrix

    m = get_rotation_matrix(np.float32([0.0, 0.0]), 5, 7)
    assert m.dtype == np.float32 and m.shape == (2, 8)
    assert np.array_equal(m[0], np.float32([1, 0, 0, 0, 1, 0, 0, 0])) and np.array_equal(m[1], m[0])
    # a 5 x 7 image (h - 1 = 4, w - 1 = 6) at float32 pi / 2: sin = 1 exactly, cos = c = cos(float32(pi / 2)) ~ -4.37e-8
    a = np.float32(np.pi / 2)
    c = np.float32(np.cos(a))
    assert np.float32(np.sin(a)) == 1.0 and abs(c) < 1e-7
    f = np.float32
    x_off = (f(6) - (c * f(6) - f(1) * f(4))) / f(2)      # ~ (6 + 4) / 2 = 5
    y_off = (f(4) - (f(1) * f(6) + c * f(4))) / f(2)      # ~ (4 - 6) / 2 = -1
    m = get_rotation_matrix(np.float32([a]), 5, 7)[0]
    assert np.array_equal(m, np.float32([c, -1, x_off, 1, c, y_off, 0, 0]))
    assert abs(float(m[2]) - 5.0) < 1e-6 and abs(float(m[5]) + 1.0) < 1e-6
    assert np.array_equal(m, R.rotation_matrix(a, 5, 7))
    # one size per angle (a padded batch of different-sized samples)
    mb = get_rotation_matrix(np.float32([0.3, 2.5]), np.array([5, 20]), np.array([7, 3]))
    assert np.array_equal(mb[0], R.rotation_matrix(0.3, 5, 7)) and np.array_equal(mb[1], R.rotation_matrix(2.5, 20, 3))


def test_draws_stay_inside_the_documented_ranges():
    from iseg_amd.data_process import augments as A

    H, W, N = 40, 56, 1000
    grid = {round(float(v), 4) for v in np.linspace(np.float32(0.5), np.float32(2.0), 16, dtype=np.float32)}
    sc = A.RandomScaleAugment(seed=1)
    draws = [sc.draw(H, W) for _ in range(N)]
    assert all(h == w and round(h, 4) in grid for h, w in draws) and {round(h, 4) for h, _ in draws} == grid
    sb = A.RandomScaleAugment(0.5, 2.0, 0.25, break_aspect_ratio=True, seed=1)
    draws = [sb.draw(H, W) for _ in range(N)]
    assert all(0.5 <= h <= 2.0 and 0.5 <= w <= 2.0 for h, w in draws) and any(h != w for h, w in draws)
    assert A.RandomScaleAugment(1.0, 1.0).draw(H, W) == (1.0, 1.0)
    cont = A.RandomScaleAugment(0.5, 2.0, 0, seed=1)
    assert all(0.5 <= cont.draw(H, W)[0] < 2.0 for _ in range(N))
    cr = A.RandomCropAugment(33, 40, seed=2)
    offs = [cr.draw(H, W) for _ in range(N)]
    assert {o[0] for o in offs} == set(range(H - 33 + 1)) and {o[1] for o in offs} == set(range(W - 40 + 1))
    with pytest.raises(ValueError):
        cr.draw(32, W)
    fl = A.RandomFlipAugment(0.25, seed=3)
    assert 0.2 < np.mean([fl.draw(H, W) for _ in range(N)]) < 0.3
    assert all(A.RandomFlipAugment(1.0).draw(H, W) for _ in range(20)) and A.PadAugment(48, 48).draw(H, W) == (48, 56)
    assert A.PadToOddAugment().draw(40, 55) == (41, 55)
    er = A.RandomErasingAugment(prob=0.5, max_area_count=4, seed=4)
    decisions = [er.draw(H, W) for _ in range(N)]
    assert 0.45 < np.mean([d is not None for d in decisions]) < 0.55
    for d in decisions:
        if d is not None:
            assert 1 <= len(d["rects"]) <= 3
            for y, x, h, w in d["rects"]:
                assert 1 <= h <= max(H // 4, 1) and 1 <= w <= max(W // 4, 1) and 0 <= y <= H - h and 0 <= x <= W - w
    assert all(d is not None for d in [A.RandomErasingAugment(prob=1.0).draw(H, W) for _ in range(20)])
    for cls, lo, hi, kw in ((A.RandomBrightnessAugment, -32, 32, {}), (A.RandomContrastAugment, 0.5, 1.5, {}), (A.RandomHueAugment, -0.1, 0.1, {}),
                            (A.RandomSaturationAugment, 0.9, 1.1, {})):
        aug = cls(seed=5, **kw)
        vals = [aug.draw(H, W) for _ in range(N)]
        assert 0.45 < np.mean([v is not None for v in vals]) < 0.55
        assert all(lo <= v < hi for v in vals if v is not None)
        assert all(cls(execute_prob=1.0).draw(H, W) is not None for _ in range(5))
    pm = A.RandomPhotoMetricDistortions(seed=6)
    for _ in range(N):
        c, s, h = pm.draw(H, W)
        assert (c is None or 0.75 <= c < 1.25) and (s is None or 0.75 <= s < 1.25) and -0.1 <= h < 0.1
    assert A.RandomNoisyEvalAugment(0.0005).draw(H, W) is None and A.RandomNoisyEvalAugment(4.0).draw(H, W) is not None
    rt = A.RandomRotateAugment(prob_of_rotate=0.5, seed=7)
    angles = [rt.draw(H, W) for _ in range(N)]
    assert 0.45 < np.mean([a is not None for a in angles]) < 0.55
    assert all(a.dtype == np.float32 and 0.0 <= a <= np.float32(2 * np.pi) for a in angles if a is not None)
    assert A.RandomRotateAugment(prob_of_rotate=0.0).draw(H, W) is None
    assert A.ResizeAugment(24, 20).draw(48, 36) == (24, 18) and A.ResizeAugment(24, 20).draw(16, 12) == (16, 12)
    # the same seed draws the same decisions
    assert [A.RandomCropAugment(9, 9, seed=8).draw(H, W) for _ in range(3)] == [A.RandomCropAugment(9, 9, seed=8).draw(H, W) for _ in range(3)]


def test_pipeline_applies_the_augments_in_order(capsys):
    from iseg_amd.data_process import AugmentationsPipeLine
    from iseg_amd.data_process.augments import LambdaAugment

    trace = []

    def stage(tag):
        def fn(image, label):
            trace.append(tag)
            return image + [tag], label

        return LambdaAugment(fn, name=f"stage_{tag}")

    pipe = AugmentationsPipeLine(augments=[stage("a"), stage("b"), stage("c")], perform_post_process=False)
    assert pipe.name == "AugmentationsPipeLine" and pipe.target_height is None and pipe.target_width is None
    image, label = pipe.process([], "label")
    assert trace == ["a", "b", "c"] and image == ["a", "b", "c"] and label == "label"
    pipe.process([], None)
    assert capsys.readouterr().out.count("Processed augments = ['stage_a', 'stage_b', 'stage_c']") == 1      # printed once
    assert AugmentationsPipeLine(0, -1).target_height is None and AugmentationsPipeLine(5, 6).target_width == 6
    assert AugmentationsPipeLine()(None) is None


def test_post_process_casts_squeezes_and_checks_the_target_size():
    import torch

    from iseg_amd.data_process import AugmentationsPipeLine

    image, label = torch.zeros(4, 6, 3, dtype=torch.uint8), torch.ones(4, 6, 1, dtype=torch.int64)
    out, lab = AugmentationsPipeLine(4, 6).process(image, label)
    assert out.dtype == torch.float32 and lab.dtype == torch.int32 and tuple(lab.shape) == (4, 6)
    out, lab = AugmentationsPipeLine().process(image, None)
    assert lab is None and tuple(out.shape) == (4, 6, 3)
    with pytest.raises(ValueError):
        AugmentationsPipeLine(5, 6).process(image, label)


def test_transform_refuses_what_the_device_does_not_implement():
    import torch

    from iseg_amd.data_process.augments.random_rotate_augment import transform

    images = torch.zeros(1, 4, 4, 3)
    with pytest.raises(NotImplementedError):
        transform(images, np.float32([1, 0, 0, 0, 1, 0, 0, 0]))                                   # the default fill mode is "reflect"
    for mode in ("reflect", "wrap", "nearest"):
        with pytest.raises(NotImplementedError):
            transform(images, np.float32([1, 0, 0, 0, 1, 0, 0, 0]), fill_mode=mode)
    with pytest.raises(NotImplementedError):
        transform(images, np.float32([1, 0, 0, 0, 1, 0, 0, 0]), fill_mode="constant", output_shape=[8, 8])


def test_jpeg_quality_is_constructible_and_raises_on_call():
    from iseg_amd.data_process.augments import RandomJEPGQualityAugment

    aug = RandomJEPGQualityAugment()
    assert aug.name == "RandomJEPGQualityAugment"
    with pytest.raises(NotImplementedError, match="not part of the on-device pipeline"):
        aug(None, None)


def test_kernels_refuse_host_tensors():
    import torch

    from iseg_amd import _hip
    from iseg_amd import kernels as K

    with pytest.raises(_hip.HipCallError):
        K.projective_transform_batch(torch.zeros(1, 4, 4, 3), None, torch.zeros(1, 8))


def test_constructors_refuse_bad_arguments():
    import torch

    from iseg_amd.data_process.augments import RandomErasingAugment, RandomRotateAugment

    for lo, hi in ((-0.1, 0.5), (0.2, 1.5), (0.6, 0.5)):
        with pytest.raises(ValueError):
            RandomErasingAugment(min_area_size=lo, max_area_size=hi)
    with pytest.raises(ValueError):
        RandomErasingAugment(fill_constant_color=[1, 2])
    assert RandomErasingAugment(fill_constant_color=None)._fill_constant_color == [0.0, 0.0, 0.0]
    assert RandomErasingAugment(fill_constant_color=(1, 2, 3))._fill_constant_color == [1.0, 2.0, 3.0]
    assert RandomErasingAugment(fill_constant_color=9)._fill_constant_color == [9.0]
    with pytest.raises(ValueError, match="fill_constant_color"):      # checked before anything touches the device
        RandomRotateAugment().apply_batch(torch.zeros(2, 4, 4, 4), None, None, np.float32([0.1, 0.2]))
