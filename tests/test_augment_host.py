"""CPU: the training-batch augmentation's host side -- the plan sampler (preprocess.AugPlan), the
torch restatement the GPU tests compare against (augment_oracle), and the argument checks of the
sdp_train_batch_aug wrapper (nothing is launched)."""
import math

import numpy as np
import pytest
import torch

import augment_oracle as ao
import preprocess as pp
import sdpnet_hip as sp


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------
def test_same_seed_same_plan():
    a = pp.AugPlan.sample(16, 32, 48, gen(7), flip_p=0.5)
    b = pp.AugPlan.sample(16, 32, 48, gen(7), flip_p=0.5)
    c = pp.AugPlan.sample(16, 32, 48, gen(8), flip_p=0.5)
    assert np.array_equal(a.pack(), b.pack())
    assert (a.mode, a.wa, a.wp, a.box) == (b.mode, b.wa, b.wp, b.box)
    assert not np.array_equal(a.pack(), c.pack())
    assert a.flip.sum() not in (0, 16)  # flip_p = 0.5 over 16 images


def test_flip_default_off_and_mix_none():
    p = pp.AugPlan.sample(64, 16, 16, gen(0), mix=None)
    assert p.mode == pp.MODE_NONE and not p.flip.any()
    with pytest.raises(ValueError):
        pp.AugPlan.sample(2, 8, 8, gen(0), mix="cutmix-only")


@pytest.mark.parametrize("H,W", [(32, 32), (17, 33), (224, 224), (5, 3)])
def test_erase_rectangles_inside_image(H, W):
    p = pp.AugPlan.sample(500, H, W, gen(H * 1000 + W), mix=None, erase_p=1.0)
    top, left, h, w = p.erase.T
    on = (h > 0) & (w > 0)
    assert on.any() or (H, W) == (5, 3)
    assert (h[on] < H).all() and (w[on] < W).all()
    assert (top >= 0).all() and (left >= 0).all()
    assert (top + h <= H).all() and (left + w <= W).all()
    # area and aspect inside torchvision's ranges, up to the rounding of h and w to integers
    if (H, W) == (224, 224):
        area = (h[on] * w[on]) / (H * W)
        assert area.min() > 0.02 * 0.9 and area.max() < 0.33 * 1.1
        ratio = h[on] / w[on]
        assert ratio.min() > 0.3 * 0.9 and ratio.max() < 3.3 * 1.1
        # the position is uniform over its range: both far ends are reached in 500 draws
        assert (top[on] + h[on]).max() > H - 16 and top[on].min() < 16


def test_erase_count_is_binomial():
    p = pp.AugPlan.sample(4000, 32, 32, gen(123), mix=None)
    n = int(((p.erase[:, 2] > 0) & (p.erase[:, 3] > 0)).sum())
    assert abs(n - 1000) <= 137, n  # 5 sigma of Binomial(4000, 0.25)


def test_cutmix_count_is_binomial():
    g = gen(321)
    modes = [pp.AugPlan.sample(1, 8, 8, g).mode for _ in range(2000)]
    assert set(modes) == {pp.MODE_MIXUP, pp.MODE_CUTMIX}
    n = modes.count(pp.MODE_CUTMIX)
    assert abs(n - 1000) <= 112, n  # 5 sigma of Binomial(2000, 0.5)


def _box_formula(lam, r_x, r_y, H, W):
    r = 0.5 * math.sqrt(1.0 - lam)
    hw, hh = int(r * W), int(r * H)
    return (max(r_x - hw, 0), max(r_y - hh, 0), min(r_x + hw, W), min(r_y + hh, H))


@pytest.mark.parametrize("lam,r_x,r_y", [(0.3, 10, 7), (0.9, 0, 0), (0.5, 29, 17), (0.0, 15, 9), (0.0, 0, 17),
                                         (1.0, 11, 4), (0.75, 29, 0)])
def test_cutmix_box_formula(lam, r_x, r_y):
    H, W = 18, 30
    box, lam_adj = pp.cutmix_box(lam, r_x, r_y, H, W)
    assert box == _box_formula(lam, r_x, r_y, H, W)
    x1, y1, x2, y2 = box
    assert 0 <= x1 <= x2 <= W and 0 <= y1 <= y2 <= H
    assert lam_adj == 1.0 - (x2 - x1) * (y2 - y1) / (W * H)
    plan = pp.AugPlan.identity(3, H, W).with_cutmix(lam, r_x, r_y)
    assert plan.mode == pp.MODE_CUTMIX and plan.box == box
    assert (plan.wa, plan.wp) == pp.mix_weights(lam_adj)
    if lam == 1.0:
        assert (x2 - x1) * (y2 - y1) == 0 and plan.wa == 1.0 and plan.wp == 0.0  # empty box
    if (lam, r_x, r_y) == (0.0, 15, 9):
        assert box == (0, 0, W, H) and plan.wa == 0.0 and plan.wp == 1.0  # centred: the whole image


def test_sampled_cutmix_follows_the_formula():
    g = gen(5)
    seen = 0
    for _ in range(200):
        p = pp.AugPlan.sample(2, 18, 30, g)
        x1, y1, x2, y2 = p.box
        if p.mode == pp.MODE_CUTMIX:
            seen += 1
            assert 0 <= x1 <= x2 <= 30 and 0 <= y1 <= y2 <= 18
            assert p.lam == 1.0 - (x2 - x1) * (y2 - y1) / (30 * 18)
        assert (p.wa, p.wp) == pp.mix_weights(p.lam)
    assert seen > 50


@pytest.mark.parametrize("lam", [0.0, 1.0, 0.5, 0.1, 0.8731234, 1e-9, 0.3333333333333333, 0.9999999])
def test_weights_sum_to_one_within_an_ulp(lam):
    wa, wp = pp.mix_weights(lam)
    assert wa == float(np.float32(lam)) and wp == float(np.float32(1.0 - lam))
    assert abs((wa + wp) - 1.0) <= 2.0 ** -23
    # and they are the values torch rounds the Python scalars to
    one = torch.ones(1)
    assert one.mul(lam).item() == wa and one.mul(1.0 - lam).item() == wp


def test_pack_layout():
    p = pp.AugPlan.identity(2, 8, 12).with_cutmix(0.5, 6, 4)
    p.flip[1] = 1
    p.erase[0] = (1, 2, 3, 4)
    w = p.pack()
    assert w.dtype == np.int32 and w.shape == (8 + 8 * 2,)
    assert w[0] == 2 and tuple(w[3:7]) == p.box and w[7] == 0
    assert tuple(w[1:3].view(np.float32)) == (np.float32(p.wa), np.float32(p.wp))
    assert tuple(w[8:16]) == (0, 1, 2, 3, 4, 0, 0, 0) and tuple(w[16:24]) == (1, 0, 0, 0, 0, 0, 0, 0)


def test_lut_is_the_eval_normalisation():
    lut = pp.normalize_lut()
    assert lut.dtype == torch.float32 and lut.shape == (3, 256)
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 256).expand(1, 3, 256).reshape(1, 3, 16, 16)
    x = u8.to(torch.float32) / 255.0
    m = torch.tensor(pp.IMAGENET_MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(pp.IMAGENET_STD, dtype=torch.float32)[:, None, None]
    assert torch.equal(lut.view(3, 16, 16), ((x - m) / s)[0])
    assert torch.equal(ao.per_image(u8.contiguous(), pp.AugPlan.identity(1, 16, 16))[0], lut.view(3, 16, 16))


# ---------------------------------------------------------------------------
# oracle against a 3-image example worked element by element
# ---------------------------------------------------------------------------
def _by_hand(img, labels, plan, K):
    """Every output element from its definition, in numpy fp32 scalars: no roll, no slicing."""
    B, _, H, W = img.shape
    f = np.float32
    mean, std = pp.IMAGENET_MEAN, pp.IMAGENET_STD

    def v(i, c, y, x):
        top, left, h, w = plan.erase[i]
        if top <= y < top + h and left <= x < left + w:
            return f(0)
        sx = W - 1 - x if plan.flip[i] else x
        return (f(img[i, c, y, sx]) / f(255.0) - f(mean[c])) / f(std[c])

    wa, wp = f(plan.wa), f(plan.wp)
    out = np.zeros((B, 3, H, W), np.float32)
    x1, y1, x2, y2 = plan.box
    for b in range(B):
        p = (b - 1 + B) % B
        for c in range(3):
            for y in range(H):
                for x in range(W):
                    if plan.mode == 1:
                        out[b, c, y, x] = f(v(p, c, y, x) * wp) + f(v(b, c, y, x) * wa)
                    elif plan.mode == 2 and y1 <= y < y2 and x1 <= x < x2:
                        out[b, c, y, x] = v(p, c, y, x)
                    else:
                        out[b, c, y, x] = v(b, c, y, x)
    t = np.zeros((B, K), np.float32)
    for b in range(B):
        p = (b - 1 + B) % B
        for k in range(K):
            t[b, k] = f(wp * f(k == labels[p])) + f(wa * f(k == labels[b]))
    return out, t


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("channels_last", [False, True])
def test_oracle_equals_worked_example(mode, channels_last):
    B, H, W, K = 3, 4, 6, 5
    img = torch.randint(0, 256, (B, 3, H, W), generator=gen(3), dtype=torch.uint8)
    labels = torch.tensor([4, 1, 1])
    plan = pp.AugPlan.identity(B, H, W)
    plan.flip[1] = 1
    plan.erase[0] = (0, 0, 2, 3)   # corner
    plan.erase[2] = (1, 2, 2, 3)   # overlaps the CutMix box edge below
    if mode == 1:
        plan.with_mixup(0.3)
    elif mode == 2:
        plan.with_cutmix(0.4, 3, 2)
        assert plan.box == (1, 1, 5, 3)
    src = img.permute(0, 2, 3, 1).contiguous() if channels_last else img
    out, t = ao.apply(src, labels, plan, K, channels_last=channels_last)
    ref, tref = _by_hand(img.numpy(), labels.numpy(), plan, K)
    assert out.dtype == torch.float32 and torch.equal(out, torch.from_numpy(ref))
    if mode == 0:
        assert torch.equal(t, labels)
    else:
        assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(tref))
        assert abs(float(t.sum(1).max()) - 1) < 1e-6
        assert t[2, 1] == np.float32(np.float32(plan.wa) + np.float32(plan.wp))  # equal labels in a pair


# ---------------------------------------------------------------------------
# wrapper argument checks (raised before anything touches a device)
# ---------------------------------------------------------------------------
def _args(B=2, H=8, W=8, K=10):
    img = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    labels = torch.zeros(B, dtype=torch.int64)
    lut = pp.normalize_lut()
    plan = torch.from_numpy(pp.AugPlan.identity(B, H, W).with_mixup(0.5).pack())
    return img, labels, lut, plan, K


def test_wrapper_rejects_cpu_tensors():
    img, labels, lut, plan, K = _args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.train_batch_aug(img, labels, lut, plan, K, torch.float32, True, labels_host=labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp.TrainBatchTransform(K, device="cpu")


def test_wrapper_rejects_wrong_dtypes_and_shapes():
    img, labels, lut, plan, K = _args()
    with pytest.raises(ValueError):
        sp.train_batch_aug(img.float(), labels, lut, plan, K, torch.float32, True)
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels.int(), lut, plan, K, torch.float32, True)
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels, lut.double(), plan, K, torch.float32, True)
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels, lut, plan.long(), K, torch.float32, True)
    with pytest.raises(TypeError):
        sp.train_batch_aug(img, labels, lut, plan, K, torch.float16, True)
    with pytest.raises(ValueError):
        sp.train_batch_aug(img[:, :2], labels, lut, plan, K, torch.float32, True)       # not RGB / not contiguous
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels[:1], lut, plan, K, torch.float32, True)          # labels are [B]
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels, lut, plan[:-1], K, torch.float32, True)         # plan too short
    with pytest.raises(ValueError):
        sp.train_batch_aug(img, labels, lut[:, :255], plan, K, torch.float32, True)


def test_wrapper_rejects_labels_out_of_range():
    img, labels, lut, plan, K = _args()
    for bad in (-1, K, 1 << 40):
        lab = labels.clone()
        lab[1] = bad
        with pytest.raises(ValueError, match="label outside"):
            sp.train_batch_aug(img, lab, lut, plan, K, torch.float32, True, labels_host=lab)


def test_wrapper_rejects_short_target_rows():
    img, labels, lut, plan, K = _args()
    with pytest.raises(ValueError, match="targets"):
        sp.train_batch_aug(img, labels, lut, plan, K, torch.float32, True, targets=torch.zeros(2, K - 1))
    overlapping = torch.zeros(2 * K).as_strided((2, K), (K - 1, 1))  # ldt < K
    with pytest.raises(ValueError, match="targets"):
        sp.train_batch_aug(img, labels, lut, plan, K, torch.float32, True, targets=overlapping)
    with pytest.raises(ValueError, match="targets"):
        sp.train_batch_aug(img, labels, lut, plan, K, torch.float32, False, targets=torch.zeros(2, K))


def test_entry_point_rejects_bad_arguments_before_launch():
    """The C entry point itself: nulls and inconsistent sizes are hipErrorInvalidValue (1), an
    empty batch is a no-op, and no device is touched."""
    L = sp.lib()
    f = L.sdp_train_batch_aug
    assert f(None, 0, None, None, None, 2, 8, 8, 0, None, None, 0, 0, None) == 1
    assert f(8, 0, 8, 8, 8, 2, 8, 8, 0, None, None, 0, 0, None) == 1       # out is null
    assert f(8, 0, 8, 8, 8, 2, 8, 8, 2, 8, None, 0, 0, None) == 1          # unknown output dtype
    assert f(8, 0, 8, 8, 8, 2, 0, 8, 0, 8, None, 0, 0, None) == 1          # H == 0
    assert f(8, 0, 8, 8, 8, -1, 8, 8, 0, 8, None, 0, 0, None) == 1         # B < 0
    assert f(8, 0, 8, 8, 8, 2, 8, 8, 0, 8, 8, 9, 10, None) == 1            # ldt < K
    assert f(8, 0, None, 8, 8, 2, 8, 8, 0, 8, 8, 10, 10, None) == 1        # targets without labels
    assert f(None, 0, None, None, None, 0, 8, 8, 0, None, None, 0, 0, None) == 0   # B == 0
