"""The tail of the reference's training input pipeline restated in torch CPU ops, given a plan
(helper of test_augment_host.py and test_gpu_augment.py; no test of its own).

Per image, as ``train_transforms`` ends (hf_dataset_generator.py:43-57):
    ToImage -> ToDtype(float32, scale=True) -> Normalize -> RandomErasing(value 0)
with the normalisation written as oracle/eval_oracle.py writes it.  Over the batch, as the collate
(hf_dataset_generator.py:325-336, dataset_generator.py:105-110) runs torchvision's CutMix / MixUp:
    MixUp:  x.roll(1, 0).mul(1 - lam).add_(x.mul(lam))
    CutMix: out = x.clone(); out[..., y1:y2, x1:x2] = x.roll(1, 0)[..., y1:y2, x1:x2]
    labels: one_hot(y, K).float(); t.roll(1, 0).mul_(1 - lam).add_(t.mul(lam))
The random decisions come from the plan (preprocess.AugPlan); its fp32 weights wa / wp are the
values torch rounds ``lam`` / ``1 - lam`` to when it multiplies an fp32 tensor by the scalar.
"""
import torch

from preprocess import IMAGENET_MEAN, IMAGENET_STD, MODE_CUTMIX, MODE_MIXUP, MODE_NONE


def per_image(images_u8: torch.Tensor, plan, mean=IMAGENET_MEAN, std=IMAGENET_STD,
              channels_last: bool = False) -> torch.Tensor:
    """uint8 batch -> fp32 [B, 3, H, W]: scale, normalise, flip, erase (each image on its own)."""
    x = images_u8.cpu()
    if channels_last:
        x = x.permute(0, 3, 1, 2)
    x = x.contiguous().to(torch.float32) / 255.0
    for c in range(3):
        x[:, c] = (x[:, c] - mean[c]) / std[c]
    out = []
    for b in range(x.shape[0]):
        img = x[b]
        if int(plan.flip[b]):
            img = img.flip(-1)
        img = img.clone()
        top, left, h, w = (int(v) for v in plan.erase[b])
        if h > 0 and w > 0:
            img[:, top:top + h, left:left + w] = 0.0
        out.append(img)
    return torch.stack(out) if out else x


def apply(images_u8: torch.Tensor, labels: torch.Tensor, plan, num_classes: int, mean=IMAGENET_MEAN,
          std=IMAGENET_STD, channels_last: bool = False):
    """(images fp32 [B, 3, H, W], targets): targets are fp32 [B, K] rows when the plan mixes,
    else the int64 labels."""
    x = per_image(images_u8, plan, mean, std, channels_last)
    labels = labels.cpu().to(torch.int64)
    if plan.mode == MODE_NONE:
        return x, labels
    wa, wp = torch.tensor(plan.wa, dtype=torch.float32), torch.tensor(plan.wp, dtype=torch.float32)
    if plan.mode == MODE_MIXUP:
        out = x.roll(1, 0).mul(wp).add_(x.mul(wa))
    elif plan.mode == MODE_CUTMIX:
        x1, y1, x2, y2 = plan.box
        out = x.clone()
        out[..., y1:y2, x1:x2] = x.roll(1, 0)[..., y1:y2, x1:x2]
    else:
        raise ValueError(plan.mode)
    t = torch.nn.functional.one_hot(labels, num_classes).float()
    t = t.roll(1, 0).mul_(wp).add_(t.mul(wa))
    return out, t
