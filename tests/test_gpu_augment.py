"""GPU: sdp_train_batch_aug against the torch restatement of the reference's collate
(tests/augment_oracle.py), bit for bit.

Every output element is at most three correctly rounded fp32 operations on entries of the
normalisation table (two products and a sum for MixUp, a copy otherwise), and the table equals
torch's ToDtype + Normalize by construction, so fp32 images, fp32 targets and bf16 images
(against ``oracle.to(bfloat16)``, the same round-to-nearest-even) are compared with torch.equal."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import augment_oracle as ao
import preprocess as pp
import sdpnet_hip as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# the last two are extra: the smallest shapes on the 8-pixels-per-lane path (W % 8 == 0)
SHAPES = [(1, 8, 12), (3, 18, 30), (5, 17, 33), (2, 5, 3), (4, 224, 224), (3, 9, 16), (2, 7, 8)]


def batch(B, H, W, K, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + B * 131 + H * 17 + W)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, K, (B,), generator=g)
    return img, labels


def run(img, labels, plan, K, dtype, channels_last=False):
    """The kernel through the binding, on device copies of the operands."""
    src = img.permute(0, 2, 3, 1).contiguous() if channels_last else img
    lut = pp.normalize_lut().to(DEV)
    plan_d = torch.from_numpy(plan.pack()).to(DEV)
    return sp.train_batch_aug(src.to(DEV), labels.to(DEV), lut, plan_d, K, dtype, plan.mode != 0,
                              channels_last=channels_last, labels_host=labels)


def check(img, labels, plan, K, channels_last=False):
    src = img.permute(0, 2, 3, 1).contiguous() if channels_last else img
    ref, tref = ao.apply(src, labels, plan, K, channels_last=channels_last)
    for dtype in (torch.float32, BF):
        out, t = run(img, labels, plan, K, dtype, channels_last)
        assert out.dtype == dtype and out.shape == ref.shape
        assert torch.equal(out.cpu(), ref.to(dtype)), f"images {dtype} differ from the oracle"
        if plan.mode == 0:
            assert t is None
        else:
            assert t.dtype == torch.float32 and torch.equal(t.cpu(), tref), "targets differ from the oracle"


def hand_plan(B, H, W, mode):
    """Flip on image 0 only, an erase in a corner of image 0, one on the last image that no
    other image has (so B > 1 sees it on the partner side alone), and a mix whose CutMix box cuts
    through the last image's rectangle."""
    plan = pp.AugPlan.identity(B, H, W)
    plan.flip[0] = 1
    eh, ew = max(H // 3, 1), max(W // 3, 1)
    if eh < H and ew < W:
        plan.erase[0] = (0, 0, eh, ew)
        if B > 1:
            plan.erase[B - 1] = (H - eh - (H > eh + 1), W // 2 - ew // 2, eh, ew)
    if mode == 1:
        plan.with_mixup(0.37)
    elif mode == 2:
        plan.with_cutmix(0.45, W // 2, (2 * H) // 3)
    return plan


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_oracle(shape, K, channels_last, mode):
    B, H, W = shape
    img, labels = batch(B, H, W, K)
    check(img, labels, hand_plan(B, H, W, mode), K, channels_last)


# (x1, y1, x2, y2) at (H, W) = (18, W): each border, a corner, empty, the whole image, one pixel
def boxes(H, W):
    return {"left": (0, 5, 7, 11), "right": (W - 9, 2, W, 9), "top": (4, 0, 20, 6), "bottom": (3, H - 5, 17, H),
            "corner": (W - 3, H - 2, W, H), "empty": (11, 4, 11, 4), "empty_row": (2, 7, 19, 7),
            "full": (0, 0, W, H), "pixel": (13, 9, 14, 10), "unaligned": (7, 1, 9, 17)}


@pytest.mark.parametrize("W", [30, 32])
@pytest.mark.parametrize("name", list(boxes(18, 32)))
def test_cutmix_boxes(name, W):
    B, H, K = 3, 18, 10
    img, labels = batch(B, H, W, K, seed=1)
    plan = pp.AugPlan.identity(B, H, W)
    plan.flip[1] = 1
    plan.erase[2] = (6, 9, 7, 6)  # overlaps the edge of most boxes
    x1, y1, x2, y2 = boxes(H, W)[name]
    plan.mode, plan.box = pp.MODE_CUTMIX, (x1, y1, x2, y2)
    plan.lam = 1.0 - (x2 - x1) * (y2 - y1) / (W * H)
    plan.wa, plan.wp = pp.mix_weights(plan.lam)
    check(img, labels, plan, K)


@pytest.mark.parametrize("W", [30, 32])
@pytest.mark.parametrize("mode", [1, 2])
def test_erase_and_flip_cases(mode, W):
    B, H, K = 4, 18, 10
    img, labels = batch(B, H, W, K, seed=2)
    labels[2] = labels[1]                      # equal labels in a pair: one entry wa + wp
    plan = pp.AugPlan.identity(B, H, W)
    plan.flip[1] = 1                           # the pairs (1, 0) and (2, 1) flip one image each
    plan.erase[0] = (0, 0, 5, 9)               # top-left corner; image 0 is the partner of image 1
    plan.erase[2] = (H - 4, W - 7, 4, 7)       # bottom-right corner
    plan.erase[3] = (3, 0, 1, W - 1)           # one row, one pixel short of the width
    plan.erase[1] = (2, 5, 0, 6)               # h == 0: no erase
    plan = plan.with_mixup(0.8125) if mode == 1 else plan.with_cutmix(0.5, 10, 8)
    check(img, labels, plan, K)


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_mix_weight_extremes(lam):
    B, H, W, K = 3, 18, 32, 10
    img, labels = batch(B, H, W, K, seed=3)
    check(img, labels, hand_plan(B, H, W, 0).with_mixup(lam), K)
    check(img, labels, hand_plan(B, H, W, 0).with_cutmix(lam, 16, 9), K)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("W", [12, 16])
def test_single_image_is_its_own_partner(mode, W):
    img, labels = batch(1, 8, W, 10, seed=4)
    plan = hand_plan(1, 8, W, mode)
    check(img, labels, plan, 10)
    out, t = run(img, labels, plan, 10, torch.float32)
    assert t[0, labels[0]].item() == np.float32(np.float32(plan.wa) + np.float32(plan.wp))


@pytest.mark.parametrize("W", [30, 32])
@pytest.mark.parametrize("seed", range(20))
def test_sampled_plans(seed, W):
    B, H, K = 3, 18, 10
    img, labels = batch(B, H, W, K, seed=seed)
    g = torch.Generator().manual_seed(seed)
    check(img, labels, pp.AugPlan.sample(B, H, W, g, erase_p=0.6, flip_p=0.5), K)


def test_unaligned_operands_and_strided_targets():
    """Pixels that start one byte off an 8-byte boundary leave the wide path (W % 8 == 0 alone
    does not select it); target rows longer than K keep their tail."""
    B, H, W, K = 3, 9, 16, 10
    img, labels = batch(B, H, W, K, seed=5)
    plan = hand_plan(B, H, W, 1)
    ref, tref = ao.apply(img, labels, plan, K)
    raw = torch.zeros(img.numel() + 1, dtype=torch.uint8, device=DEV)
    raw[1:] = img.to(DEV).view(-1)
    t = torch.full((B, K + 6), -7.0, device=DEV)
    out, t2 = sp.train_batch_aug(raw[1:].view(B, 3, H, W), labels.to(DEV), pp.normalize_lut().to(DEV),
                                 torch.from_numpy(plan.pack()).to(DEV), K, torch.float32, True, targets=t)
    assert t2 is t and torch.equal(out.cpu(), ref)
    assert torch.equal(t[:, :K].cpu(), tref) and bool((t[:, K:] == -7.0).all())


def test_empty_batch_and_mode_none_targets():
    lut = pp.normalize_lut().to(DEV)
    plan = pp.AugPlan.identity(0, 8, 8)
    out, t = sp.train_batch_aug(torch.empty(0, 3, 8, 8, dtype=torch.uint8, device=DEV), None, lut,
                                torch.from_numpy(plan.pack()).to(DEV), 10, torch.float32, False)
    assert out.shape == (0, 3, 8, 8) and t is None


class _ListLoader(list):
    sampler = "the-sampler"


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_loader_matches_oracle_batch_for_batch(dtype):
    """Three host batches through DeviceAugLoader: the staging buffers alternate (the third batch
    reuses the first one's), and the plans come from the same seeded generator as the oracle's."""
    B, H, W, K = 4, 16, 24, 10
    data = _ListLoader(batch(B, H, W, K, seed=10 + i) for i in range(3))
    tf = pp.TrainBatchTransform(K, device=DEV, dtype=dtype, erase_p=0.7, flip_p=0.5,
                                generator=torch.Generator().manual_seed(99))
    loader = pp.DeviceAugLoader(data, tf)
    assert len(loader) == 3 and loader.sampler == "the-sampler"
    got = list(loader)  # all three in flight before any result is read
    g = torch.Generator().manual_seed(99)
    for (img, labels), (out, t) in zip(data, got):
        plan = pp.AugPlan.sample(B, H, W, g, erase_p=0.7, flip_p=0.5)
        ref, tref = ao.apply(img, labels, plan, K)
        assert out.is_cuda and out.dtype == dtype and torch.equal(out.cpu(), ref.to(dtype))
        assert t.is_cuda and t.dtype == torch.float32 and torch.equal(t.cpu(), tref)
    assert tf._staging[0].buf is not None and tf._staging[1].buf is not None


def test_transform_device_inputs_mode_none_and_label_check():
    B, H, W, K = 3, 8, 16, 10
    img, labels = batch(B, H, W, K, seed=20)
    tf = pp.TrainBatchTransform(K, device=DEV, mix=None, channels_last=True,
                                generator=torch.Generator().manual_seed(1))
    nhwc = img.permute(0, 2, 3, 1).contiguous()
    plan = hand_plan(B, H, W, 0)
    ref, _ = ao.apply(nhwc, labels, plan, K, channels_last=True)
    for src, lab in ((nhwc, labels), (nhwc.to(DEV), labels.to(DEV)), (nhwc.to(DEV), labels)):
        out, t = tf(src, lab, plan)
        assert torch.equal(out.cpu(), ref)
        assert t.is_cuda and t.dtype == torch.int64 and torch.equal(t.cpu(), labels)
    bad = labels.clone()
    bad[0] = K
    with pytest.raises(ValueError, match="label outside"):
        tf(nhwc, bad, plan)
    with pytest.raises(ValueError, match="plan is for"):
        tf(nhwc, labels, pp.AugPlan.identity(B, H, W + 1))


def test_targets_feed_the_soft_cross_entropy():
    """sdpnet_train.cross_entropy on the produced rows = nn.CrossEntropyLoss(label_smoothing=0.1)
    on the oracle's rows, to the 1e-5 (relative to the loss) of test_gpu_train_kernels.py's
    soft-target test."""
    import sdpnet_train as st
    B, H, W, K = 6, 8, 16, 1000
    img, labels = batch(B, H, W, K, seed=30)
    logits = 3 * torch.randn(B, K, generator=torch.Generator().manual_seed(31))
    for plan in (hand_plan(B, H, W, 1), hand_plan(B, H, W, 2)):
        _, t = run(img, labels, plan, K, torch.float32)
        _, tref = ao.apply(img, labels, plan, K)
        got = st.cross_entropy(logits.to(DEV), t, 0.1)
        ref = nn.CrossEntropyLoss(label_smoothing=0.1)(logits, tref)
        err = abs(got.item() - ref.item())
        assert err <= 1e-5 * max(1e-6, abs(ref.item())), (got.item(), ref.item())
