"""CPU: the numpy oracle of the device-side crop / flip / RandAugment (tests/randaug_oracle.py)
against Pillow itself, bit for bit, and the host side of the feature: the sampler, the plan words
and the refusals (no kernel launches).

The mapping from a RandAugment (op, magnitude) to a Pillow call (``pil_op`` below) is restated
from torchvision's published v2 source; torchvision is not installed, so only the pixel arithmetic
is pinned here, against Pillow."""
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

import preprocess as pp
import randaug_oracle as ro
import sdpnet_hip as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_op(a: np.ndarray, name: str, m: float) -> np.ndarray:
    im = Image.fromarray(a)
    W, H = im.size
    if name == "Identity":
        r = im
    elif name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        r = im.transform((W, H), Image.Transform.AFFINE, ro.matrix(name, m, H, W), Image.Resampling.NEAREST)
    elif name == "Rotate":
        r = im.rotate(m)
    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
        r = getattr(ImageEnhance, name)(im).enhance(1.0 + m)
    elif name == "Posterize":
        r = ImageOps.posterize(im, int(m))
    elif name == "Solarize":
        r = ImageOps.solarize(im, m)
    elif name == "AutoContrast":
        r = ImageOps.autocontrast(im)
    elif name == "Equalize":
        r = ImageOps.equalize(im)
    else:
        raise ValueError(name)
    return np.asarray(r)


def special_images(H: int, W: int, seed: int = 0):
    """random | constant | a two-valued channel | a channel with hi == lo | grey with the L mean
    at (or, for an odd pixel count, as near as it gets to) x.5."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    rand = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    two = rand.copy()
    two[..., 1] = rng.choice(np.array([10, 200], np.uint8), (H, W))
    flat = rand.copy()
    flat[..., 2] = 99
    half = np.full(H * W, 100, np.uint8)
    half[:(H * W) // 2] = 101
    half = np.repeat(rng.permutation(half).reshape(H, W, 1), 3, axis=2)
    return {"random": rand, "constant": np.full((H, W, 3), 77, np.uint8), "two_valued": two, "flat_channel": flat,
            "half_mean": half}


def magnitudes(name: str, H: int, W: int):
    """Bin 9 (the default) and the extremes, bins 1 and 30, each with both signs where signed."""
    out = []
    for bin_ in (9, 1, 30):
        m = pp.ra_magnitude(name, H, W, bin_)
        out += [m, -m] if name in ro.SIGNED else [m]
    return list(dict.fromkeys(out))


SIZES = [(37, 53), (224, 224), (225, 224), (5, 7)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ro.OPS)
def test_oracle_equals_pillow(name, size):
    H, W = size
    imgs = special_images(H, W)
    if (H, W) != (37, 53):  # the special images once at a small and once at an even size; else random
        imgs = {k: v for k, v in imgs.items() if k in ("random", "half_mean") or (H, W) == (224, 224)}
    for key, a in imgs.items():
        for m in magnitudes(name, H, W):
            assert np.array_equal(ro.apply_op(a, name, m), pil_op(a, name, m)), (key, name, m)


def test_half_mean_image_is_at_the_rounding_point():
    L = ro.luma(special_images(224, 224)["half_mean"])
    assert abs(L.astype(np.int64).sum() / L.size - 100.5) < 1e-9


def test_equalize_step_zero_and_flat_channel_are_identity():
    tiny = special_images(5, 7)["random"]
    assert np.array_equal(ro.apply_op(tiny, "Equalize"), tiny)  # (35 - last) // 255 == 0
    flat = special_images(37, 53)["flat_channel"]
    assert np.array_equal(ro.apply_op(flat, "AutoContrast")[..., 2], flat[..., 2])
    assert np.array_equal(ro.apply_op(flat, "Equalize")[..., 2], flat[..., 2])


@pytest.mark.parametrize("f", [0.73, 1.27])
def test_blend_all_pairs(f):
    """Every (degenerate, source) byte pair through Image.blend, the call ImageEnhance makes."""
    d = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    s = np.ascontiguousarray(d.T)
    ref = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(s), f))
    assert np.array_equal(ro.blend(d, s, f), ref)


# ---- resized crop ----
def crop_cases(H, W, OH, OW):
    """(top, left, h, w): the whole image, a box in each corner, a 20 x 30 box (upscaled at 224),
    a large box (400 x 300 in the 500 x 375 source), and a box as wide as the output."""
    bh, bw = max(H // 2, 1), max(W // 3, 1)
    cases = {"whole": (0, 0, H, W), "top_left": (0, 0, bh, bw), "top_right": (0, W - bw, bh, bw),
             "bottom_left": (H - bh, 0, bh, bw), "bottom_right": (H - bh, W - bw, bh, bw)}
    if H >= 25 and W >= 35:
        cases["small_20x30"] = (3, 4, 20, 30)
    if H >= 400 and W >= 300:
        cases["large_400x300"] = (50, 40, 400, 300)
    if W >= OW and H >= 7 and H != OH:
        cases["same_width"] = (1, W - OW, min(H - 1, 2 * OH + 5), OW)  # horizontal pass skipped
    return cases


SOURCES = [(37, 53), (500, 375), (64, 64)]
OUTS = [(224, 224), (32, 40)]


@pytest.mark.parametrize("out_size", OUTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "x".join(map(str, s)))
def test_resized_crop_oracle_equals_pillow(src, out_size):
    H, W = src
    OH, OW = out_size
    a = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for key, (top, left, h, w) in crop_cases(H, W, OH, OW).items():
        ref = Image.fromarray(a).crop((left, top, left + w, top + h)).resize((OW, OH), Image.Resampling.BICUBIC)
        for flip in (False, True):
            want = np.asarray(ref.transpose(Image.Transpose.FLIP_LEFT_RIGHT) if flip else ref)
            assert np.array_equal(ro.resized_crop(a, (top, left, h, w), out_size, flip), want), (key, flip)


def test_crop_cases_cover_the_skipped_pass():
    assert "same_width" in crop_cases(500, 375, 224, 224) and "same_width" in crop_cases(64, 64, 32, 40)
    assert "large_400x300" in crop_cases(500, 375, 224, 224) and "small_20x30" in crop_cases(37, 53, 224, 224)


# ---- the sampler and the plan ----
SAMPLE_SIZES = [(500, 375), (37, 53), (64, 64), (10, 1000), (1000, 10), (333, 500)] * 8


def test_sampler_is_deterministic_and_inside():
    a = pp.CropAugPlan.sample(SAMPLE_SIZES, (224, 224), torch.Generator().manual_seed(5))
    b = pp.CropAugPlan.sample(SAMPLE_SIZES, (224, 224), torch.Generator().manual_seed(5))
    c = pp.CropAugPlan.sample(SAMPLE_SIZES, (224, 224), torch.Generator().manual_seed(6))
    assert np.array_equal(a.pack(), b.pack()) and a.ops == b.ops
    assert not np.array_equal(a.pack(), c.pack())
    for (H, W), (top, left, h, w) in zip(SAMPLE_SIZES, a.boxes.tolist()):
        assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= H and left + w <= W
    assert set(a.flip.tolist()) == {0, 1}
    names = {n for per in a.ops for n, _ in per}
    assert names <= set(sp.RA_OPS) and len(names) >= 10 and all(len(per) == 2 for per in a.ops)
    signs = {math.copysign(1.0, m) for per in a.ops for n, m in per if n in pp.RA_SIGNED}
    assert signs == {1.0, -1.0}


def test_sampler_fallback_branch():
    """No try fits a 10 x 1000 image (h >= sqrt(0.08 * 10000 * 3 / 4) > 10): the central crop of
    the whole height at the ratio bound, centred with // 2."""
    p = pp.CropAugPlan.sample([(10, 1000), (1000, 10)], (224, 224), torch.Generator().manual_seed(0))
    assert p.boxes.tolist() == [[0, (1000 - 13) // 2, 10, 13], [(1000 - 13) // 2, 0, 13, 10]]


def test_magnitude_table():
    lin = lambda hi: float(torch.linspace(0.0, hi, 31)[9])  # noqa: E731
    H, W = 224, 200
    want = {"Identity": 0.0, "ShearX": lin(0.3), "ShearY": lin(0.3), "TranslateX": lin(150.0 / 331.0 * W),
            "TranslateY": lin(150.0 / 331.0 * H), "Rotate": lin(30.0), "Brightness": lin(0.9), "Color": lin(0.9),
            "Contrast": lin(0.9), "Sharpness": lin(0.9), "Posterize": 7.0, "Solarize": 178.5, "AutoContrast": 0.0,
            "Equalize": 0.0}
    assert {n: pp.ra_magnitude(n, H, W) for n in sp.RA_OPS} == want
    assert 8 - round(9 / 7.5) == 7 and float(255.0 * torch.linspace(1.0, 0.0, 31)[9]) == 178.5
    assert int(pp.ra_magnitude("TranslateX", H, W)) == 27 and int(pp.ra_magnitude("TranslateY", H, W)) == 30


def test_plan_words():
    f32 = lambda v: int(np.array([v], np.float32).view(np.int32)[0])  # noqa: E731
    assert pp.ra_words("Identity", 0.0, 224, 224) == [0] * 8
    assert pp.ra_words("TranslateX", -30.45, 224, 224) == [3, 65536, 0, 30 * 65536 + 32768, 0, 65536, 32768, 0]
    assert pp.ra_words("ShearY", 0.5, 8, 8) == [2, 65536, 0, 32768, 32768, 65536, 16384 + 32768, 0]
    assert pp.ra_words("Color", 0.27, 224, 224) == [7, f32(1.27), 0, 0, 0, 0, 0, 0]
    assert pp.ra_words("Posterize", 7.0, 224, 224)[:2] == [10, 0xfe]
    assert pp.ra_words("Solarize", 178.5, 224, 224)[:2] == [11, 179]
    assert pp.ra_words("Solarize", 178.0, 224, 224)[:2] == [11, 178]
    m = ro.matrix("Rotate", 9.0, 37, 53)
    assert pp.ra_matrix("Rotate", 9.0, 37, 53) == m
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731
    assert pp.ra_words("Rotate", 9.0, 37, 53)[1:7] == [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                                                       fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    p = pp.CropAugPlan.from_bins([(64, 64), (37, 53)], (32, 40), [(1, 2, 30, 40), (0, 0, 37, 53)], [1, 0],
                                 [[("Rotate", -1), ("Equalize", 1)], [("Posterize", -1), ("Color", 1)]])
    w = p.pack()
    assert w.dtype == np.int32 and w.size == p.words() == 2 * 8 + 2 * 2 * 8
    assert w[:16].tolist() == [1, 2, 30, 40, 1, 0, 0, 0, 0, 0, 37, 53, 0, 0, 0, 0]
    assert w[16:].reshape(2, 2, 8)[:, :, 0].tolist() == [[5, 13], [10, 7]]
    assert p.ops[0][0] == ("Rotate", -9.0) and p.ops[1][0] == ("Posterize", 7.0)
    assert p.pack(row_origin=True)[:4].tolist() == [0, 2, 30, 40]


def test_refusals():
    one = [[("Identity", 0.0)]]
    with pytest.raises(NotImplementedError, match="taps"):  # 400 / 4 source pixels per output pixel
        pp.CropAugPlan([(500, 375)], (4, 4), [(0, 0, 400, 300)], [0], one)
    with pytest.raises(NotImplementedError, match="aspect"):
        pp.CropAugPlan([(500, 375)], (224, 224), [(0, 0, 404, 4)], [0], one)
    with pytest.raises(ValueError, match="outside"):
        pp.CropAugPlan([(37, 53)], (224, 224), [(30, 0, 8, 53)], [0], one)
    with pytest.raises(ValueError, match="outside"):
        pp.CropAugPlan([(37, 53)], (224, 224), [(0, 0, 0, 53)], [0], one)
    for size in ((2, 224), (224, 2)):
        with pytest.raises(NotImplementedError, match="SMOOTH"):
            pp.CropAugPlan([(37, 53)], size, [(0, 0, 37, 53)], [0], [[("Sharpness", 0.27)]])
        with pytest.raises(NotImplementedError):
            ro.smooth(np.zeros(size + (3,), np.uint8))
    with pytest.raises(NotImplementedError, match="fixed-point"):  # a corner maps beyond 32768
        pp.ra_words("ShearX", 200.0, 224, 224)
    with pytest.raises(NotImplementedError, match="fixed-point"):
        ro.affine_nearest(np.zeros((224, 224, 3), np.uint8), ro.matrix("ShearX", 200.0, 224, 224))
    with pytest.raises(ValueError, match="unknown"):
        pp.ra_words("Invert", 0.0, 224, 224)
    with pytest.raises(ValueError, match="same number"):
        pp.CropAugPlan([(37, 53)] * 2, (32, 40), [(0, 0, 37, 53)] * 2, [0, 0], [[("Identity", 0.0)], []])
    with pytest.raises(ValueError, match="num_ops"):
        pp.CropAugPlan.sample([(37, 53)], (32, 40), num_ops=5)


def test_wrappers_check_before_the_library():
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.randaugment(x, torch.zeros(32, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.resized_crop(torch.zeros(384, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                        torch.zeros(2, 2, dtype=torch.int32), torch.zeros(16, dtype=torch.int32), (8, 8), 5, 8, 8)
    L = sp.lib()  # null operands and bad sizes are refused before any launch
    assert L.sdp_randaugment(None, None, None, 1, 8, 8, 2, None, None) == 1
    assert L.sdp_randaugment(8, 8, 8, 1, 8, 8, 5, 8, None) == 1
    assert L.sdp_randaugment(8, 8, 8, 1, 8, 8, 0, 8, None) == 1
    assert L.sdp_randaugment(None, None, None, 0, 8, 8, 2, None, None) == 0
    assert L.sdp_resized_crop(None, None, None, None, 1, 8, 8, 5, None, None, 256, 8, None, None) == 1
    assert L.sdp_resized_crop(8, 8, 8, 8, 1, 8, 8, 161, 8, 8, 256, 8, 8, None) == 1
    assert L.sdp_resized_crop(8, 8, 8, 8, 1, 8, 8, 5, 8, 8, 16, 8, 8, None) == 1   # tmp below one row
    assert L.sdp_resized_crop(None, None, None, None, 0, 8, 8, 5, None, None, 256, 8, None, None) == 0


def test_new_exports_are_declared_and_bound():
    """tests/test_abi.py's rule for the two new entry points: declared in the header, exported by
    the library, bound in the wrapper module."""
    src = open(os.path.join(REPO, "include", "sdpnet_hip.h")).read()
    syms = set(re.findall(r"^(?:int64_t|int|const char\*)\s+(sdp_\w+)\s*\(", src, re.M))
    for name in ("sdp_resized_crop", "sdp_randaugment"):
        assert name in syms and name in sp.exported_symbols() and hasattr(sp.lib(), name)
