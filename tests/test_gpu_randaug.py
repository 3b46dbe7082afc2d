"""GPU: sdp_resized_crop, sdp_randaugment and TrainImageTransform against the numpy restatement of
Pillow (tests/randaug_oracle.py, itself pinned to Pillow in test_randaug_host.py), bit for bit.

uint8 pixels are compared with array_equal: both sides do the same integer / fp32 / double
operations in the same order, so there is no tolerance.  The end-to-end outputs are the batch
kernel's (tests/test_gpu_augment.py): at most three correctly rounded fp32 operations on table
entries, bf16 by the same round-to-nearest-even, compared with torch.equal."""
import numpy as np
import pytest
import torch
from PIL import Image

import augment_oracle as ao
import preprocess as pp
import randaug_oracle as ro
import sdpnet_hip as sp
from test_randaug_host import OUTS, SOURCES, crop_cases, special_images

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def guarded(shape):
    """A uint8 device tensor of ``shape`` inside a buffer with GUARD marked bytes on both sides."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all())


# ---- sdp_resized_crop ----
@pytest.mark.parametrize("out_size", OUTS, ids=lambda s: "x".join(map(str, s)))
def test_resized_crop_mixed_batch(out_size):
    """Every crop case of every source, flip off and on, as one batch of mixed sizes."""
    OH, OW = out_size
    imgs, items = [], []
    for H, W in SOURCES:
        a = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        for i, box in enumerate(crop_cases(H, W, OH, OW).values()):
            for flip in (0, 1):
                imgs.append(a)
                items.append((box, flip if i else 1 - flip))
    B = len(imgs)
    sizes = [a.shape[:2] for a in imgs]
    plan = pp.CropAugPlan(sizes, out_size, [b for b, _ in items], [f for _, f in items], [[("Identity", 0.0)]] * B)
    nbytes = np.array([a.size for a in imgs], np.int64)
    offs = np.zeros(B, np.int64)
    offs[1:] = np.cumsum(nbytes)[:-1]
    pix = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(DEV)
    hw = np.array(sizes, np.int32)
    words = torch.from_numpy(plan.pack()[:sp.CROP_PLAN_PER_IMAGE * B].copy()).to(DEV)
    buf, out = guarded((B, OH, OW, 3))
    max_h, max_w = int(plan.boxes[:, 2].max()), int(plan.boxes[:, 3].max())
    got = sp.resized_crop(pix, torch.from_numpy(offs).to(DEV), torch.from_numpy(hw).to(DEV), words, out_size,
                          plan.kmax(), max_h, max_w, out=out, host=(offs, hw, plan.boxes))
    assert got is out
    got = out.cpu().numpy()
    assert guards_intact(buf)
    for b, (a, (box, flip)) in enumerate(zip(imgs, items)):
        assert np.array_equal(got[b], ro.resized_crop(a, box, out_size, bool(flip))), (b, a.shape, box, flip)


def test_resized_crop_clamps_a_bad_plan_word():
    """Words the host would refuse (the wrapper is told nothing to check) stay inside the image:
    the launch completes and the guards around the output hold."""
    a = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    words = np.zeros((3, 8), np.int32)
    words[0, :4] = (-5, -7, 1000, 1000)
    words[1, :4] = (36, 52, 50, 50)
    words[2, :4] = (2 ** 31 - 1, 2 ** 31 - 1, -3, 0)
    pix = torch.from_numpy(np.concatenate([a.reshape(-1)] * 3)).to(DEV)
    offs = torch.arange(3, dtype=torch.int64, device=DEV) * a.size
    hw = torch.tensor([[37, 53]] * 3, dtype=torch.int32, device=DEV)
    buf, out = guarded((3, 32, 40, 3))
    sp.resized_crop(pix, offs, hw, torch.from_numpy(words.reshape(-1)).to(DEV), (32, 40), 9, 37, 53, out=out)
    got = out.cpu().numpy()
    assert guards_intact(buf)
    assert np.array_equal(got[0], ro.resized_crop(a, (0, 0, 37, 53), (32, 40)))  # clamped to the whole image
    assert np.array_equal(got[1], ro.resized_crop(a, (36, 52, 1, 1), (32, 40)))  # and to the last pixel


# ---- sdp_randaugment ----
def run_ops(images, ops):
    """images: list of equal-sized HWC arrays; ops: per image a list of (name, magnitude).
    Returns (device result as numpy, plan)."""
    H, W, _ = images[0].shape
    B = len(images)
    plan = pp.CropAugPlan([(H, W)] * B, (H, W), [(0, 0, H, W)] * B, [0] * B, ops)
    words = torch.from_numpy(plan.pack()[sp.CROP_PLAN_PER_IMAGE * B:].copy()).to(DEV)
    src = torch.from_numpy(np.stack(images)).to(DEV)
    buf, out = guarded((B, H, W, 3))
    sbuf, scratch = guarded((B * H * W * 3,))
    got = sp.randaugment(src, words, plan.num_ops, scratch=scratch, out=out)
    assert got is out
    res = out.cpu().numpy()
    assert guards_intact(buf) and guards_intact(sbuf)
    assert np.array_equal(src.cpu().numpy(), np.stack(images)), "the input batch was modified"
    return res


def single_op_cases(H, W):
    cases = []
    for name in ro.OPS:
        m = pp.ra_magnitude(name, H, W)
        cases += [(name, m), (name, -m)] if name in ro.SIGNED else [(name, m)]
    return cases


# LDS tier at its largest size, LDS tier small and odd, global tier, and the Equalize step == 0 size
@pytest.mark.parametrize("size", [(224, 224), (37, 53), (225, 224), (5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_every_op_alone(size):
    H, W = size
    specials = special_images(H, W)
    if (H, W) == (5, 7):
        specials = {"random": specials["random"]}
    images, ops, keys = [], [], []
    for key, a in specials.items():
        for case in single_op_cases(H, W):
            images.append(a)
            ops.append([case])
            keys.append((key, case))
    got = run_ops(images, ops)
    for b, (a, op) in enumerate(zip(images, ops)):
        assert np.array_equal(got[b], ro.apply_ops(a, op)), keys[b]


def test_all_ordered_pairs():
    """14 x 14 ops as one B = 196 launch: an op must read what its predecessor finished writing."""
    H, W = 40, 56
    rng = np.random.default_rng(11)
    signed = lambda n: (n, pp.ra_magnitude(n, H, W) * (rng.choice([-1.0, 1.0]) if n in ro.SIGNED else 1.0))  # noqa: E731
    ops = [[signed(a), signed(b)] for a in ro.OPS for b in ro.OPS]
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in ops]
    got = run_ops(images, ops)
    for b, (a, op) in enumerate(zip(images, ops)):
        assert np.array_equal(got[b], ro.apply_ops(a, op)), op


@pytest.mark.parametrize("size", [(40, 56), (225, 224)], ids=["lds", "global"])
def test_four_ops(size):
    H, W = size
    rng = np.random.default_rng(12)
    B = 28 if size == (40, 56) else 7
    ops = []
    for b in range(B):
        names = [ro.OPS[(2 * b + 5 * k) % 14] for k in range(4)]
        ops.append([(n, pp.ra_magnitude(n, H, W) * (-1.0 if (b + k) % 2 and n in ro.SIGNED else 1.0))
                    for k, n in enumerate(names)])
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in ops]
    got = run_ops(images, ops)
    for b, (a, op) in enumerate(zip(images, ops)):
        assert np.array_equal(got[b], ro.apply_ops(a, op)), op


def test_in_place_and_unknown_op_codes():
    """Op codes outside 0..13 act as Identity (the host never emits one); out = None works in place."""
    H, W = 37, 53
    a = np.random.default_rng(13).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    words = np.zeros((4, 2, 8), np.int32)
    words[0, :, 0] = (14, -1)
    words[1, :, 0] = (2 ** 31 - 1, -2 ** 31)
    words[1, :, 1:] = -1
    words[2, 0] = pp.ra_words("Posterize", 4.0, H, W)
    words[2, 1, 0] = 99
    words[3, 0, 0] = 1000
    words[3, 1] = pp.ra_words("Rotate", 30.0, H, W)
    x = torch.from_numpy(a).to(DEV)
    got = sp.randaugment(x, torch.from_numpy(words.reshape(-1)).to(DEV), 2)
    assert got is x
    got = got.cpu().numpy()
    assert np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1])
    assert np.array_equal(got[2], ro.apply_op(a[2], "Posterize", 4.0))
    assert np.array_equal(got[3], ro.apply_op(a[3], "Rotate", 30.0))


# ---- end to end ----
E2E_SIZES = [(500, 375), (37, 53), (64, 64), (300, 224), (224, 224), (131, 480)]


def e2e_inputs():
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in E2E_SIZES]
    boxes = [(50, 40, 400, 300), (3, 4, 20, 30), (0, 0, 64, 64), (10, 0, 250, 224), (0, 0, 224, 224), (100, 200, 31, 280)]
    ops = [[("Rotate", 1), ("Equalize", 1)], [("Sharpness", -1), ("ShearX", 1)], [("Color", 1), ("Identity", 1)],
           [("AutoContrast", 1), ("Contrast", -1)], [("TranslateY", -1), ("Solarize", 1)],
           [("Posterize", 1), ("Brightness", 1)]]
    crop = pp.CropAugPlan.from_bins(E2E_SIZES, (224, 224), boxes, [1, 0, 1, 0, 0, 1], ops)
    labels = torch.tensor([3, 1, 4, 1, 5, 9])
    return images, labels, crop


def e2e_plan(mode):
    plan = pp.AugPlan.identity(6, 224, 224)
    plan.erase[1] = (10, 20, 60, 90)
    plan.erase[5] = (150, 0, 74, 224)
    if mode == "mixup":
        plan.with_mixup(0.37)
    elif mode == "cutmix":
        plan.with_cutmix(0.45, 112, 150)
    return plan


_E2E_U8 = {}


def e2e_oracle_u8():
    """The two new oracles composed, once for all the end-to-end cases."""
    if not _E2E_U8:
        images, _, crop = e2e_inputs()
        _E2E_U8["u8"] = np.stack([ro.apply_ops(ro.resized_crop(a, box, (224, 224), bool(f)), ops)
                                  for a, box, f, ops in zip(images, crop.boxes, crop.flip, crop.ops)])
        _E2E_U8["u8"].setflags(write=False)
    return _E2E_U8["u8"]


@pytest.mark.parametrize("mode", ["none", "mixup", "cutmix"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_train_image_transform_pinned(dtype, mode):
    images, labels, crop = e2e_inputs()
    plan = e2e_plan(mode)
    ref, tref = ao.apply(torch.from_numpy(e2e_oracle_u8().copy()), labels, plan, 10, channels_last=True)
    t = pp.TrainImageTransform((224, 224), num_classes=10, device=DEV, dtype=dtype)
    pil = [Image.fromarray(images[0]), torch.from_numpy(images[1])] + images[2:]
    out, targets = t(pil, labels, crop_plan=crop, plan=plan)
    assert out.dtype == dtype and tuple(out.shape) == (6, 3, 224, 224)
    assert torch.equal(out.cpu(), ref.to(dtype))
    if mode == "none":
        assert targets.dtype == torch.int64 and torch.equal(targets.cpu(), labels)
    else:
        assert targets.dtype == torch.float32 and torch.equal(targets.cpu(), tref)


def test_train_image_transform_seeded_runs_agree():
    images, labels, _ = e2e_inputs()
    runs = []
    for _ in range(2):
        t = pp.train_transforms((224, 224), device=DEV, dtype=torch.bfloat16, num_classes=10,
                                generator=torch.Generator().manual_seed(77))
        outs = [t(images, labels) for _ in range(3)]  # three batches: both staging buffers, one reused
        runs.append([(o.cpu(), y.cpu()) for o, y in outs])
    for (o1, y1), (o2, y2) in zip(*runs):
        assert torch.equal(o1, o2) and torch.equal(y1, y2)
    assert not torch.equal(runs[0][0][0], runs[0][1][0])  # the generator moved on between batches


def test_device_aug_loader_over_lists():
    images, labels, _ = e2e_inputs()

    class Loader:
        sampler = None

        def __len__(self):
            return 2

        def __iter__(self):
            yield images[:4], labels[:4]
            yield images[4:], labels[4:].tolist()

    g = torch.Generator().manual_seed(5)
    t = pp.TrainImageTransform((32, 40), num_classes=10, device=DEV, mix=None, generator=g)
    batches = list(pp.DeviceAugLoader(Loader(), t))
    assert len(batches) == 2
    g2 = torch.Generator().manual_seed(5)
    for (out, y), lo, hi in zip(batches, (0, 4), (4, 6)):
        crop, plan = pp.TrainImageTransform((32, 40), num_classes=10, device=DEV, mix=None,
                                            generator=g2).sample(E2E_SIZES[lo:hi])
        u8 = np.stack([ro.apply_ops(ro.resized_crop(a, box, (32, 40), bool(f)), ops)
                       for a, box, f, ops in zip(images[lo:hi], crop.boxes, crop.flip, crop.ops)])
        ref, _ = ao.apply(torch.from_numpy(u8), labels[lo:hi], plan, 10, channels_last=True)
        assert torch.equal(out.cpu(), ref) and torch.equal(y.cpu(), labels[lo:hi])
