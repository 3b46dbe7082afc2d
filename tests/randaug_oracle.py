"""RandomResizedCrop + flip and the 14 RandAugment ops restated in numpy (helper of
test_randaug_host.py and test_gpu_randaug.py; no test of its own).

The reference's ``train_transforms`` (hf_dataset_generator.py:43-57) runs these steps through
torchvision's v2 transforms on PIL images, i.e. through Pillow.  Every function here restates the
integer / fp32 arithmetic of Pillow 12.2.0 (Image.transform's 16.16 fixed-point nearest path,
ImageEnhance's blend, ImageFilter.SMOOTH, ImageOps.autocontrast / equalize / posterize / solarize)
and is pinned against Pillow itself, bit for bit, in test_randaug_host.py.  The mapping from a
RandAugment (op, magnitude) to a Pillow call is restated from torchvision's published v2 source;
torchvision is not installed here, so that mapping is not checked against torchvision.

An op takes and returns an HWC uint8 RGB array.  ``magnitude`` means what torchvision hands to its
functional: the shear tangent, the integer translation, the angle in degrees, m of the enhancers'
factor 1 + m, the bits Posterize keeps, Solarize's threshold.
"""
import math

import numpy as np

from eval_oracle import pil_resize_u8

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")


# ---- RandomResizedCrop + RandomHorizontalFlip ----
def resized_crop(img: np.ndarray, box, out_size, flip: bool = False) -> np.ndarray:
    """img.crop((left, top, left + w, top + h)).resize((OW, OH), BICUBIC), mirrored when ``flip``:
    the crop is an image of its own (taps clamp at the box)."""
    top, left, h, w = (int(v) for v in box)
    out = pil_resize_u8(np.ascontiguousarray(img[top:top + h, left:left + w]), out_size)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


# ---- geometric ops: Image.transform(size, AFFINE, m, NEAREST), fill 0 ----
def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def matrix(name: str, magnitude: float, H: int, W: int):
    """The six coefficients (output -> input) of a geometric op."""
    m = float(magnitude)
    if name == "ShearX":
        return (1.0, m, 0.0, 0.0, 1.0, 0.0)
    if name == "ShearY":
        return (1.0, 0.0, 0.0, m, 1.0, 0.0)
    if name == "TranslateX":
        return (1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0)
    if name == "TranslateY":
        return (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m)))
    if name == "Rotate":  # Image.rotate(m): about (w / 2, h / 2), entries rounded to 15 digits
        a = -math.radians(m % 360.0)
        mt = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        cx, cy = W / 2, H / 2
        mt[2] = mt[0] * -cx + mt[1] * -cy + mt[2]
        mt[5] = mt[3] * -cx + mt[4] * -cy + mt[5]
        mt[2] += cx
        mt[5] += cy
        return tuple(mt)
    raise ValueError(name)


def affine_nearest(img: np.ndarray, m) -> np.ndarray:
    H, W, _ = img.shape
    for x, y in ((0, 0), (W, 0), (0, H), (W, H)):  # Pillow leaves fixed point outside this range
        if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
            raise NotImplementedError("affine matrix outside the 16.16 fixed-point range")
    a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
    a2 = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (a2 + a0 * x + a1 * y) >> 16
    yin = (a5 + a3 * x + a4 * y) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


# ---- enhancers: blend(degenerate, img, f) ----
def blend(d: np.ndarray, s: np.ndarray, f: float) -> np.ndarray:
    """ImagingBlend in fp32: t = d + f * (s - d), one rounded product, one rounded sum."""
    f32 = np.float32(f)
    di, si = d.astype(np.int32), s.astype(np.int32)
    t = di.astype(np.float32) + (f32 * (si - di).astype(np.float32)).astype(np.float32)
    if 0.0 <= f32 <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.clip(t, 0.0, 255.0).astype(np.int32).astype(np.uint8)


def luma(img: np.ndarray) -> np.ndarray:
    p = img.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16).astype(np.uint8)


def smooth(img: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH: (1 1 1; 1 5 1; 1 1 1) / 13 inside, the one-pixel border copied."""
    H, W, _ = img.shape
    if H < 3 or W < 3:
        raise NotImplementedError("SMOOTH needs H >= 3 and W >= 3")
    p = img.astype(np.int64)
    s = 4 * p[1:-1, 1:-1]
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            s = s + p[dy:H - 2 + dy, dx:W - 2 + dx]
    out = img.copy()
    out[1:-1, 1:-1] = np.clip((2 * s + 13) // 26, 0, 255).astype(np.uint8)  # floor(s / 13 + 0.5)
    return out


def degenerate(name: str, img: np.ndarray) -> np.ndarray:
    if name == "Brightness":
        return np.zeros_like(img)
    if name == "Color":
        return np.repeat(luma(img)[..., None], 3, axis=2)
    if name == "Contrast":
        L = luma(img)
        mean = int(int(L.astype(np.int64).sum()) / L.size + 0.5)
        return np.full_like(img, mean)
    if name == "Sharpness":
        return smooth(img)
    raise ValueError(name)


# ---- histogram ops ----
def _hist(ch: np.ndarray):
    return np.bincount(ch.reshape(-1), minlength=256).tolist()


def autocontrast_lut(h):
    nz = [i for i, v in enumerate(h) if v]
    lo, hi = nz[0], nz[-1]
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(i * scale + offset))) for i in range(256)]


def equalize_lut(h):
    histo = [v for v in h if v]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))  # Image.point clips the table to uint8
        n += h[i]
    return lut


def _per_channel(img: np.ndarray, make_lut) -> np.ndarray:
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = np.asarray(make_lut(_hist(img[..., c])), np.uint8)[img[..., c]]
    return out


def apply_op(img: np.ndarray, name: str, magnitude: float = 0.0) -> np.ndarray:
    H, W, _ = img.shape
    if name == "Identity":
        return img.copy()
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        return affine_nearest(img, matrix(name, magnitude, H, W))
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return blend(degenerate(name, img), img, 1.0 + float(magnitude))
    if name == "Posterize":
        return img & np.uint8(~(2 ** (8 - int(magnitude)) - 1) & 0xff)
    if name == "Solarize":
        return np.where(img < magnitude, img, 255 - img).astype(np.uint8)
    if name == "AutoContrast":
        return _per_channel(img, autocontrast_lut)
    if name == "Equalize":
        return _per_channel(img, equalize_lut)
    raise ValueError(name)


def apply_ops(img: np.ndarray, ops) -> np.ndarray:
    """ops: a sequence of (name, magnitude), applied in order."""
    for name, mag in ops:
        img = apply_op(img, name, mag)
    return img
