"""On-device validation preprocessing.

Counterpart of the reference's ``val_transforms`` (hf_dataset_generator.py:27-41),
which ``model_test.py:50-52`` builds as ``val_transforms(image_size=(320, 320),
crop_size=(224, 224))``:

    RGB -> Resize(image_size, BICUBIC) -> CenterCrop(crop_size) -> ToImage
        -> ToDtype(float32, scale=True) -> Normalize(mean, std)

The reference applies it per PIL image on the dataloader's CPU workers.  Here a batch
of decoded images is packed into one pinned host buffer, copied once, and transformed
by ``sdp_val_preprocess`` (csrc/eval.hip) straight into the model's NCHW input, fp32 or
bf16.  The resize is Pillow's 8-bit resampler restated bit for bit (the crop's uint8
pixels equal PIL's), so images with an aspect ratio H / W above 100 -- where Pillow
changes its pass order -- are refused rather than approximated.

Training counterpart, for the batch-level tail of the reference's ``train_transforms`` and
collate (hf_dataset_generator.py:43-57, :325-336; dataset_generator.py:105-110):

    ToImage -> ToDtype(float32, scale=True) -> Normalize -> RandomErasing(p=0.25)
        -> RandomChoice([CutMix(), MixUp(alpha=0.8)]) -> [B, 1000] float targets

The loader's workers keep decode, RandomResizedCrop and RandAugment (they work on PIL images)
and hand over uint8 batches; ``TrainBatchTransform`` draws the random decisions on the host
(``AugPlan``), uploads pixels, labels and plan in one copy and runs ``sdp_train_batch_aug``
(csrc/augment.hip), which reproduces the reference's fp32 arithmetic bit for bit.

``TrainImageTransform`` moves the head of ``train_transforms`` onto the device as well:

    RGB -> RandomResizedCrop(224, BICUBIC) -> RandomHorizontalFlip -> RandAugment()

The workers then only decode.  ``CropAugPlan`` draws the crop boxes, flips and RandAugment ops on
the host; decoded images of any sizes, both plans and the labels go up in one copy, and
``sdp_resized_crop`` (csrc/eval.hip) -> ``sdp_randaugment`` (csrc/randaug.hip) ->
``sdp_train_batch_aug`` produce the model's input.  The uint8 pixels equal Pillow 12.2.0's bit for
bit (the library torchvision calls for PIL images).  The mapping from RandAugment's (op, magnitude
bin) to a Pillow call is restated from torchvision's published v2 source; torchvision is not
installed where this was written, so that mapping is unverified against torchvision itself.

Decode itself is hybrid (``JpegDecoder``): every transform above also takes encoded JPEGs (``bytes``
/ ``bytearray`` / ``memoryview`` items).  The serial Huffman decode runs on a host thread pool
(``sdp_jpeg_entropy_decode``, plain C++, the GIL released); the quantised coefficients go up in one
copy and ``sdp_jpeg_reconstruct`` (csrc/jpeg.hip) dequantises, inverts the DCT, upsamples the chroma
and converts the colours straight into the packed ``pix / offs / hw`` buffer the kernels above read:
the decoded pixels never exist on the host.  The pixels equal ``Image.open(f).convert("RGB")`` of
Pillow 12.2.0 bit for bit; a JPEG outside the subset (progressive, CMYK, ...) is decoded by Pillow
and placed into the same buffer; a malformed one raises.
"""
from __future__ import annotations

import functools
import io
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

import sdpnet_hip as sp

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # hf_dataset_generator.py:30-31
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_TAPS = 160


def _as_rgb_u8(img) -> np.ndarray:
    """transforms.RGB() + ToImage for one decoded image -> HWC uint8 (host)."""
    if hasattr(img, "convert") and hasattr(img, "mode"):  # PIL image
        if img.mode != "RGB":
            img = img.convert("RGB")
        return np.asarray(img, dtype=np.uint8)
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"val preprocessing takes decoded uint8 images, got {a.dtype}")
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, axis=2)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"expected an HWC RGB image, got shape {a.shape}")
    return a[:, :, :3]


def _taps(n_in: int, n_out: int) -> int:
    return int(math.ceil(2.0 * max(1.0, n_in / n_out))) * 2 + 1


def _is_encoded(img) -> bool:
    return isinstance(img, (bytes, bytearray, memoryview))


class JpegDecoder:
    """Hybrid JPEG decode of a batch: ``decode(items) -> (pix, offs, hw)`` on ``device``, the packed
    triple sdp_val_preprocess and sdp_resized_crop read (pix uint8 [sum 3 H W], offs int64 [B], hw
    int32 [B, 2]).

    Every encoded item is probed (markers only).  The supported ones are Huffman-decoded on a pool
    of ``num_threads`` host threads (at most 16) into one pinned buffer, which goes up in one copy
    together with the descriptors, and one ``sdp_jpeg_reconstruct`` call writes their pixels.  An
    unsupported item (progressive, CMYK, ...) is decoded by Pillow and travels as pixels in the same
    upload, as does an item that is already decoded (PIL image, ndarray, tensor), so the batch is
    always complete and in order.  A malformed item raises ``ValueError`` naming its index before
    anything is uploaded."""

    MAX_THREADS = 16

    def __init__(self, device="cuda", num_threads: int = 8):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("JpegDecoder runs sdp_jpeg_reconstruct; the HIP path has no CPU fallback")
        self.num_threads = max(1, min(int(num_threads), self.MAX_THREADS))
        self._pool = ThreadPoolExecutor(self.num_threads) if self.num_threads > 1 else None
        self._staging = (_Staging(), _Staging())
        self._turn = 0
        self.last_fallbacks: List[int] = []   # indices of the last batch that Pillow decoded

    @staticmethod
    def _pillow(data) -> np.ndarray:
        from PIL import Image
        return _as_rgb_u8(Image.open(io.BytesIO(bytes(data))))

    def decode(self, items: Sequence) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.decode_with_host(items)[:3]

    def decode_with_host(self, items: Sequence):
        """``decode`` plus the host copies of offs (int64 [B]) and hw (int64 [B, 2])."""
        B = len(items)
        if B == 0:
            z = torch.empty(0, dtype=torch.uint8, device=self.device)
            return (z, torch.empty(0, dtype=torch.int64, device=self.device),
                    torch.empty(0, 2, dtype=torch.int32, device=self.device), np.zeros(0, np.int64),
                    np.zeros((0, 2), np.int64))
        infos: List[Optional[np.ndarray]] = [None] * B
        arrs: List[Optional[np.ndarray]] = [None] * B
        self.last_fallbacks = []
        for i, it in enumerate(items):
            if not _is_encoded(it):
                arrs[i] = _as_rgb_u8(it)
                continue
            rc, info = sp.jpeg_probe(it)
            if rc < 0:
                raise ValueError(f"item {i}: malformed JPEG ({sp.JPEG_MALFORMED.get(rc, rc)})")
            if rc > 0:
                try:
                    arrs[i] = self._pillow(it)
                except Exception as e:
                    raise ValueError(f"item {i}: malformed JPEG ({e})") from e
                self.last_fallbacks.append(i)
            else:
                infos[i] = info
        hw = np.array([(a.shape[0], a.shape[1]) if a is not None else (int(f[1]), int(f[0]))
                       for a, f in zip(arrs, infos)], np.int64)
        if (hw <= 0).any():
            raise ValueError("empty image")
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offs = np.zeros(B, np.int64)
        offs[1:] = np.cumsum(nbytes)[:-1]
        n_pix = int(nbytes.sum())
        jpegs = [i for i in range(B) if infos[i] is not None]
        ncoef = np.array([_round_up(int(infos[i][10]), 64) for i in jpegs], np.int64)
        coef_off = np.zeros(len(jpegs), np.int64)
        coef_off[1:] = np.cumsum(ncoef)[:-1]
        n_coef = int(ncoef.sum())
        # one pinned buffer: descriptors | offs | hw | coefficients | pixels of the items decoded on the host
        W = sp.JPEG_DESC_WORDS
        n_desc = 4 * W * len(jpegs)
        o_offs = _round_up(n_desc, 16)
        o_hw = _round_up(o_offs + 8 * B, 16)
        o_coef = _round_up(o_hw + 8 * B, 16)
        o_raw = _round_up(o_coef + 2 * n_coef, 16)
        raw = [i for i in range(B) if arrs[i] is not None]
        raw_off = np.zeros(len(raw), np.int64)
        raw_off[1:] = np.cumsum(nbytes[raw])[:-1]
        total = o_raw + int(nbytes[raw].sum())
        st = self._staging[self._turn]
        self._turn ^= 1
        host = st.take(total)
        hv = host.numpy()
        desc = hv[:n_desc].view(np.int32)
        desc[:] = 0
        hv[o_offs:o_offs + 8 * B].view(np.int64)[:] = offs
        hv[o_hw:o_hw + 8 * B].view(np.int32)[:] = hw.astype(np.int32).reshape(-1)
        coef = hv[o_coef:o_coef + 2 * n_coef].view(np.int16)

        def job(k: int) -> int:
            i = jpegs[k]
            d = desc[k * W:(k + 1) * W]
            rc, info = sp.jpeg_entropy_decode(items[i], coef[coef_off[k]:coef_off[k] + ncoef[k]],
                                              d[sp.JPEG_DESC_QT:].view(np.uint8))
            if rc == 0:  # the planar samples of an image take as many bytes as it has coefficients
                sp.jpeg_fill_desc(d, info, coef_off[k], coef_off[k], offs[i])
            return rc

        codes = list(self._pool.map(job, range(len(jpegs)))) if self._pool is not None and len(jpegs) > 1 \
            else [job(k) for k in range(len(jpegs))]
        for k, rc in enumerate(codes):
            if rc < 0:
                raise ValueError(f"item {jpegs[k]}: malformed JPEG ({sp.JPEG_MALFORMED.get(rc, rc)})")
        late = [jpegs[k] for k, rc in enumerate(codes) if rc > 0]
        if late:  # unsupported only behind the scan (a second scan, DNL): Pillow takes them, the batch is redone
            items = list(items)
            for i in late:
                try:
                    items[i] = self._pillow(items[i])
                except Exception as e:
                    raise ValueError(f"item {i}: malformed JPEG ({e})") from e
            first = self.last_fallbacks
            out = self.decode_with_host(items)
            self.last_fallbacks = sorted(first + late)
            return out
        for i, o in zip(raw, raw_off.tolist()):
            hv[o_raw + o:o_raw + o + nbytes[i]] = np.ascontiguousarray(arrs[i]).reshape(-1)
        with torch.cuda.device(self.device):
            dev = host.to(self.device, non_blocking=True)
            st.event = torch.cuda.Event()
            st.event.record()
            offs_d = dev[o_offs:o_offs + 8 * B].view(torch.int64).clone()  # copies: the upload can then go
            hw_d = dev[o_hw:o_hw + 8 * B].view(torch.int32).view(B, 2).clone()
            if not jpegs:  # nothing to reconstruct: the uploaded pixels are the batch
                return dev[o_raw:o_raw + n_pix], offs_d, hw_d, offs, hw
            pix = torch.empty(n_pix, dtype=torch.uint8, device=self.device)
            ws = torch.empty(n_coef, dtype=torch.uint8, device=self.device)
            sp.jpeg_reconstruct(dev[o_coef:o_coef + 2 * n_coef].view(torch.int16), desc, dev[:n_desc].view(torch.int32),
                                len(jpegs), ws, pix)
            for i, o in zip(raw, raw_off.tolist()):
                pix[offs[i]:offs[i] + nbytes[i]] = dev[o_raw + o:o_raw + o + nbytes[i]]
        return pix, offs_d, hw_d, offs, hw


class ValTransform:
    """Batched ``val_transforms(image_size, crop_size, mean, std)``:
    ``__call__(images) -> Tensor[B, 3, crop_h, crop_w]`` on ``device``."""

    def __init__(self, image_size=(320, 320), crop_size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 device="cuda", dtype=torch.float32):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        if self.crop_size[0] > self.image_size[0] or self.crop_size[1] > self.image_size[1]:
            raise NotImplementedError("CenterCrop larger than the resized image (padding) is not supported")
        # torchvision center_crop origin: int(round((size - crop) / 2.0))
        self.top = int(round((self.image_size[0] - self.crop_size[0]) / 2.0))
        self.left = int(round((self.image_size[1] - self.crop_size[1]) / 2.0))
        self.mean, self.std = tuple(mean), tuple(std)
        self.device = torch.device(device)
        self.dtype = dtype
        self.jpeg_decoder: Optional[JpegDecoder] = None  # made on the first batch that holds encoded JPEGs

    def _jpeg(self) -> JpegDecoder:
        if self.jpeg_decoder is None:
            self.jpeg_decoder = JpegDecoder(self.device)
        return self.jpeg_decoder

    def _call_encoded(self, images: Sequence, return_u8: bool):
        """A batch with encoded JPEGs in it: decoded on the device into the packed triple."""
        pix, offs_d, hw_d, _, hw = self._jpeg().decode_with_host(images)
        RH, RW = self.image_size
        kmax = 1
        for H, W in hw.tolist():
            if H > 100 * W:
                raise NotImplementedError(f"image {H}x{W}: aspect ratio above 100 (Pillow reorders its passes there)")
            kmax = max(kmax, _taps(W, RW), _taps(H, RH))
        if kmax > MAX_TAPS:
            raise NotImplementedError(f"downscale factor too large ({kmax} taps > {MAX_TAPS})")
        tmp_stride = int(hw[:, 0].max()) * self.crop_size[1] * 4
        out, u8 = sp.val_preprocess(pix, offs_d, hw_d, self.image_size, self.crop_size, self.top, self.left, kmax,
                                    self.mean, self.std, tmp_stride, self.dtype, want_u8=return_u8,
                                    max_w=int(hw[:, 1].max()))
        return (out, u8) if return_u8 else out

    def __call__(self, images: Sequence, return_u8: bool = False):
        if any(_is_encoded(im) for im in images):
            return self._call_encoded(images, return_u8)
        arrs = [_as_rgb_u8(im) for im in images]
        B = len(arrs)
        RH, RW = self.image_size
        if B == 0:
            out = torch.empty(0, 3, *self.crop_size, dtype=self.dtype, device=self.device)
            u8 = torch.empty(0, *self.crop_size, 3, dtype=torch.uint8, device=self.device)
            return (out, u8) if return_u8 else out
        kmax, hmax, wmax = 1, 1, 1
        for a in arrs:
            H, W = a.shape[:2]
            if H == 0 or W == 0:
                raise ValueError("empty image")
            if H > 100 * W:
                raise NotImplementedError(f"image {H}x{W}: aspect ratio above 100 (Pillow reorders its passes there)")
            kmax = max(kmax, _taps(W, RW), _taps(H, RH))
            hmax = max(hmax, H)
            wmax = max(wmax, W)
        if kmax > MAX_TAPS:
            raise NotImplementedError(f"downscale factor too large ({kmax} taps > {MAX_TAPS})")
        sizes = [a.shape[0] * a.shape[1] * 3 for a in arrs]
        offs = np.zeros(B, dtype=np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        hv = host.numpy()
        for a, o, n in zip(arrs, offs, sizes):
            hv[o:o + n] = np.ascontiguousarray(a).reshape(-1)
        hw = torch.tensor([[a.shape[0], a.shape[1]] for a in arrs], dtype=torch.int32)
        pix = host.to(self.device, non_blocking=True)
        offs_d = torch.from_numpy(offs).to(self.device)
        hw_d = hw.to(self.device)
        tmp_stride = hmax * self.crop_size[1] * 4  # RGBX words of the horizontal pass
        out, u8 = sp.val_preprocess(pix, offs_d, hw_d, self.image_size, self.crop_size, self.top, self.left, kmax,
                                    self.mean, self.std, tmp_stride, self.dtype, want_u8=return_u8, max_w=wmax)
        return (out, u8) if return_u8 else out


def val_transforms(image_size=(320, 320), crop_size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                   device="cuda", dtype=torch.float32) -> ValTransform:
    """hf_dataset_generator.py:27-41 signature; returns the batched device transform."""
    return ValTransform(image_size, crop_size, mean, std, device=device, dtype=dtype)


def batches(dataset: Iterable, transform: ValTransform, batch_size: int = 256) -> Iterable[Tuple[torch.Tensor, torch.Tensor]]:
    """(images, labels) device batches from an iterable of (decoded image, int label)
    pairs -- the hf_dataset + DataLoader(batch_size=256, shuffle=False) of
    model_test.py:52-53 with the transform moved onto the GPU.  An image may also be an encoded
    JPEG (bytes / bytearray / memoryview): the transform then decodes the batch on the device."""
    imgs: List = []
    labels: List[int] = []
    for img, lab in dataset:
        imgs.append(img)
        labels.append(int(lab))
        if len(imgs) == batch_size:
            yield transform(imgs), torch.tensor(labels, dtype=torch.int64).to(transform.device)
            imgs, labels = [], []
    if imgs:
        yield transform(imgs), torch.tensor(labels, dtype=torch.int64).to(transform.device)


# ---------------------------------------------------------------------------
# training: RandomErasing + CutMix / MixUp + soft targets on the device
# ---------------------------------------------------------------------------
ERASE_SCALE = (0.02, 0.33)   # torchvision RandomErasing defaults (value 0)
ERASE_RATIO = (0.3, 3.3)
ERASE_ATTEMPTS = 10
MIXUP_ALPHA = 0.8            # hf_dataset_generator.py:325-336: RandomChoice([CutMix(), MixUp(alpha=0.8)])
CUTMIX_ALPHA = 1.0
MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


def normalize_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """fp32 [3, 256]: ToDtype(float32, scale=True) + Normalize of every uint8 value, with the
    expression of the evaluation oracle, so that table look-up equals the fp32 ops bit for bit."""
    u = torch.arange(256, dtype=torch.float32) / 255.0
    return torch.stack([(u - float(mean[c])) / float(std[c]) for c in range(3)]).contiguous()


def cutmix_box(lam: float, r_x: int, r_y: int, H: int, W: int) -> Tuple[Tuple[int, int, int, int], float]:
    """torchvision CutMix: ((x1, y1, x2, y2), lam_adjusted) of the box centred on (r_x, r_y)."""
    r = 0.5 * math.sqrt(1.0 - lam)
    r_w_half, r_h_half = int(r * W), int(r * H)
    x1, y1 = max(r_x - r_w_half, 0), max(r_y - r_h_half, 0)
    x2, y2 = min(r_x + r_w_half, W), min(r_y + r_h_half, H)
    return (x1, y1, x2, y2), float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))


def mix_weights(lam: float) -> Tuple[float, float]:
    """(wa, wp): the fp32 weights of an image and of its partner, as torch rounds the Python
    scalars of ``x.roll(1, 0).mul(1.0 - lam).add_(x.mul(lam))`` (the subtraction in double)."""
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return f32(lam), f32(1.0 - lam)


@dataclass
class AugPlan:
    """The random decisions of one training batch, as plain host data.

    flip [B] (0 / 1), erase [B, 4] (top, left, h, w in output coordinates; h == 0 or w == 0: no
    erase), mode (0 none, 1 MixUp, 2 CutMix), wa / wp (the weights of an image and of its partner
    ``(b - 1) mod B``, exact fp32 values), box (x1, y1, x2, y2)."""
    B: int
    H: int
    W: int
    flip: np.ndarray
    erase: np.ndarray
    mode: int = MODE_NONE
    lam: float = 1.0
    wa: float = 1.0
    wp: float = 0.0
    box: Tuple[int, int, int, int] = field(default=(0, 0, 0, 0))

    @staticmethod
    def identity(B: int, H: int, W: int) -> "AugPlan":
        return AugPlan(B, H, W, np.zeros(B, np.int32), np.zeros((B, 4), np.int32))

    @staticmethod
    def sample(B: int, H: int, W: int, generator: Optional[torch.Generator] = None, mix: Optional[str] = "reference",
               erase_p: float = 0.25, flip_p: float = 0.0) -> "AugPlan":
        """Draw a plan from torch's CPU generator; the same seed gives the same plan.

        Per image: flip with probability ``flip_p``; RandomErasing with probability ``erase_p``
        and torchvision's defaults: up to 10 attempts of area = H W U(0.02, 0.33), aspect =
        exp(U(log 0.3, log 3.3)), h = round(sqrt(area aspect)), w = round(sqrt(area / aspect)),
        the first with h < H and w < W taken, then top ~ U{0..H-h}, left ~ U{0..W-w}; no erase
        if none fits.  Per batch (``mix="reference"``): CutMix (alpha 1.0) or MixUp (alpha 0.8)
        with equal probability, lam ~ Beta(alpha, alpha) in fp32 as torchvision draws it.
        The draws of a batch are taken in bulk (a fixed number per image), so the stream is not
        torchvision's; the distribution and the formulas are."""
        if mix not in (None, "reference"):
            raise ValueError(f"mix must be 'reference' or None, got {mix!r}")
        g = generator
        per = torch.rand(B, 4 + 2 * ERASE_ATTEMPTS, generator=g, dtype=torch.float64).numpy()
        flip = (per[:, 0] < flip_p).astype(np.int32)
        erase = np.zeros((B, 4), np.int32)
        s0, s1 = ERASE_SCALE
        l0, l1 = math.log(ERASE_RATIO[0]), math.log(ERASE_RATIO[1])
        for b in np.nonzero(per[:, 1] < erase_p)[0]:
            for a in range(ERASE_ATTEMPTS):
                area = H * W * (s0 + (s1 - s0) * per[b, 4 + 2 * a])
                aspect = math.exp(l0 + (l1 - l0) * per[b, 5 + 2 * a])
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if not (h < H and w < W):
                    continue
                top = min(int(per[b, 2] * (H - h + 1)), H - h)
                left = min(int(per[b, 3] * (W - w + 1)), W - w)
                erase[b] = (top, left, h, w)
                break
        plan = AugPlan(B, H, W, flip, erase)
        if mix is None:
            return plan
        pick = torch.rand(1, generator=g).item()
        alpha = CUTMIX_ALPHA if pick < 0.5 else MIXUP_ALPHA
        lam = float(torch._sample_dirichlet(torch.tensor([alpha, alpha]), g)[0])
        if pick < 0.5:
            r_x = int(torch.randint(W, (1,), generator=g))
            r_y = int(torch.randint(H, (1,), generator=g))
            return plan.with_cutmix(lam, r_x, r_y)
        return plan.with_mixup(lam)

    def with_mixup(self, lam: float) -> "AugPlan":
        self.mode, self.lam, self.box = MODE_MIXUP, float(lam), (0, 0, 0, 0)
        self.wa, self.wp = mix_weights(lam)
        return self

    def with_cutmix(self, lam: float, r_x: int, r_y: int) -> "AugPlan":
        self.box, lam_adj = cutmix_box(lam, r_x, r_y, self.H, self.W)
        self.mode, self.lam = MODE_CUTMIX, lam_adj
        self.wa, self.wp = mix_weights(lam_adj)
        return self

    def words(self) -> int:
        return sp.AUG_PLAN_HEADER + sp.AUG_PLAN_PER_IMAGE * self.B

    def pack(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The int32 words sdp_train_batch_aug reads (layout: include/sdpnet_hip.h)."""
        if out is None:
            out = np.empty(self.words(), np.int32)
        out[:] = 0
        out[0] = self.mode
        out[1:3] = np.array([self.wa, self.wp], np.float32).view(np.int32)
        out[3:7] = self.box
        per = out[sp.AUG_PLAN_HEADER:].reshape(self.B, sp.AUG_PLAN_PER_IMAGE)
        per[:, 0] = self.flip
        per[:, 1:5] = self.erase
        return out


class _Staging:
    """One pinned upload buffer and the event recorded after its last copy."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.event: Optional[torch.cuda.Event] = None

    def take(self, nbytes: int) -> torch.Tensor:
        if self.event is not None:
            self.event.synchronize()  # the copy out of this buffer, two batches ago
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self.buf[:nbytes]


def _round_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class TrainBatchTransform:
    """The reference's training tail on a uint8 batch: ``__call__(images_u8, labels, plan=None)
    -> (images [B, 3, H, W] of ``dtype`` on ``device``, targets)``.  targets are the fp32
    [B, num_classes] probability rows, or the int64 labels when the plan does not mix.

    images_u8 ([B, 3, H, W], or [B, H, W, 3] with ``channels_last``) and labels may each live on
    the host or on the device.  Whatever is on the host is packed behind the plan into one of two
    alternating pinned buffers and uploaded with one copy; a buffer is reused only after the event
    recorded behind its copy, so the only host wait is on a copy from two batches earlier and
    nothing synchronises the device."""

    def __init__(self, num_classes: int = 1000, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda",
                 dtype=torch.float32, mix: Optional[str] = "reference", erase_p: float = 0.25, flip_p: float = 0.0,
                 channels_last: bool = False, generator: Optional[torch.Generator] = None):
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrainBatchTransform runs sdp_train_batch_aug; the HIP path has no CPU fallback")
        sp.dcode(dtype)
        self.dtype = dtype
        self.mix, self.erase_p, self.flip_p = mix, float(erase_p), float(flip_p)
        self.channels_last = bool(channels_last)
        self.generator = generator
        self.lut = normalize_lut(mean, std).to(self.device)
        self._staging = (_Staging(), _Staging())
        self._turn = 0

    def sample(self, B: int, H: int, W: int) -> AugPlan:
        return AugPlan.sample(B, H, W, self.generator, self.mix, self.erase_p, self.flip_p)

    def __call__(self, images_u8: torch.Tensor, labels: torch.Tensor, plan: Optional[AugPlan] = None):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise TypeError(f"training batches are uint8 [B, 3, H, W] / [B, H, W, 3], got {images_u8.dtype} "
                            f"{tuple(images_u8.shape)}")
        B = images_u8.shape[0]
        H, W = images_u8.shape[1:3] if self.channels_last else images_u8.shape[2:4]
        labels = labels.to(torch.int64)
        if labels.shape != (B,):
            raise ValueError(f"labels must be [B] = [{B}], got {tuple(labels.shape)}")
        if plan is None:
            plan = self.sample(B, H, W)
        if (plan.B, plan.H, plan.W) != (B, H, W):
            raise ValueError(f"plan is for {(plan.B, plan.H, plan.W)}, the batch is {(B, H, W)}")
        labels_host = None if labels.is_cuda else labels
        if labels_host is not None and B and not (0 <= int(labels_host.min()) and int(labels_host.max()) < self.num_classes):
            raise ValueError(f"label outside [0, {self.num_classes})")
        # one pinned buffer: plan words | host labels | host pixels (16-byte aligned sections)
        n_plan = 4 * plan.words()
        o_lab = _round_up(n_plan, 16)
        o_img = _round_up(o_lab + (0 if labels.is_cuda else 8 * B), 16)
        total = o_img + (0 if images_u8.is_cuda else images_u8.numel())
        st = self._staging[self._turn]
        self._turn ^= 1
        host = st.take(total)
        plan.pack(host[:n_plan].view(torch.int32).numpy())
        if not labels.is_cuda:
            host[o_lab:o_lab + 8 * B].view(torch.int64).copy_(labels)
        if not images_u8.is_cuda:
            host[o_img:].view(images_u8.shape).copy_(images_u8)
        with torch.cuda.device(self.device):
            dev = host.to(self.device, non_blocking=True)
            st.event = torch.cuda.Event()
            st.event.record()
        plan_d = dev[:n_plan].view(torch.int32)
        labels_d = labels if labels.is_cuda else dev[o_lab:o_lab + 8 * B].view(torch.int64)
        images_d = images_u8.contiguous() if images_u8.is_cuda else dev[o_img:].view(images_u8.shape)
        mixed = plan.mode != MODE_NONE
        out, targets = sp.train_batch_aug(images_d, labels_d, self.lut, plan_d, self.num_classes, self.dtype, mixed,
                                          channels_last=self.channels_last)
        if mixed:
            return out, targets
        # uploaded labels are a view of the upload; a copy lets the pixels' memory go
        return out, (labels_d if labels.is_cuda else labels_d.clone())


# ---------------------------------------------------------------------------
# training: RandomResizedCrop + flip + RandAugment on the device
# ---------------------------------------------------------------------------
RRC_SCALE = (0.08, 1.0)          # torchvision RandomResizedCrop defaults
RRC_RATIO = (3.0 / 4.0, 4.0 / 3.0)
RRC_ATTEMPTS = 10
RA_NUM_OPS, RA_MAGNITUDE, RA_BINS = 2, 9, 31   # torchvision RandAugment() defaults
RA_SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
_RA_AFFINE = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
_RA_ENHANCE = ("Brightness", "Color", "Contrast", "Sharpness")


@functools.lru_cache(maxsize=None)
def ra_magnitude(name: str, H: int, W: int, magnitude: int = RA_MAGNITUDE, num_bins: int = RA_BINS) -> float:
    """The unsigned magnitude torchvision's RandAugment hands to its functional for bin
    ``magnitude`` of ``num_bins`` on an H x W image (fp32 linspace, as torchvision computes it):
    the shear tangent, the translation in pixels (before int()), the angle in degrees, m of the
    enhancers' factor 1 + m, the bits Posterize keeps, Solarize's threshold."""
    lin = lambda hi: float(torch.linspace(0.0, hi, num_bins)[magnitude])  # noqa: E731
    if name in ("ShearX", "ShearY"):
        return lin(0.3)
    if name == "TranslateX":
        return lin(150.0 / 331.0 * W)
    if name == "TranslateY":
        return lin(150.0 / 331.0 * H)
    if name == "Rotate":
        return lin(30.0)
    if name in _RA_ENHANCE:
        return lin(0.9)
    if name == "Posterize":
        return float(int((8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int())[magnitude]))
    if name == "Solarize":
        return float(255.0 * torch.linspace(1.0, 0.0, num_bins)[magnitude])
    if name in ("Identity", "AutoContrast", "Equalize"):
        return 0.0
    raise ValueError(f"unknown RandAugment op {name!r}")


def ra_matrix(name: str, magnitude: float, H: int, W: int) -> Tuple[float, ...]:
    """The output -> input coefficients Pillow's Image.transform(AFFINE) receives for a geometric op."""
    m = float(magnitude)
    if name == "ShearX":
        return (1.0, m, 0.0, 0.0, 1.0, 0.0)
    if name == "ShearY":
        return (1.0, 0.0, 0.0, m, 1.0, 0.0)
    if name == "TranslateX":
        return (1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0)
    if name == "TranslateY":
        return (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m)))
    if name == "Rotate":  # Image.rotate: entries rounded to 15 digits, translated about (w / 2, h / 2)
        a = -math.radians(m % 360.0)
        c, sn = round(math.cos(a), 15), round(math.sin(a), 15)
        cx, cy = W / 2, H / 2
        return (c, sn, c * -cx + sn * -cy + 0.0 + cx, -sn, c, -sn * -cx + c * -cy + 0.0 + cy)
    raise ValueError(name)


def ra_words(name: str, magnitude: float, H: int, W: int) -> List[int]:
    """The eight plan words of one op (layout: include/sdpnet_hip.h), every double-precision step
    done here.  Raises NotImplementedError where Pillow itself would leave the restated path."""
    if name not in sp.RA_OPS:
        raise ValueError(f"unknown RandAugment op {name!r}")
    w = [sp.RA_OPS.index(name), 0, 0, 0, 0, 0, 0, 0]
    if name in _RA_AFFINE:
        m = ra_matrix(name, magnitude, H, W)
        for x, y in ((0, 0), (W, 0), (0, H), (W, H)):  # Geometry.c check_fixed
            if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
                raise NotImplementedError(f"{name}({magnitude}) on {H}x{W}: outside Pillow's 16.16 fixed-point range")
        fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731
        w[1:7] = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                  fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in w[1:7]):
            raise NotImplementedError(f"{name}({magnitude}) on {H}x{W}: outside Pillow's 16.16 fixed-point range")
    elif name in _RA_ENHANCE:
        if name == "Sharpness" and (H < 3 or W < 3):
            raise NotImplementedError(f"Sharpness on {H}x{W}: ImageFilter.SMOOTH needs H >= 3 and W >= 3")
        w[1] = int(np.array([1.0 + float(magnitude)], np.float32).view(np.int32)[0])
    elif name == "Posterize":
        bits = int(magnitude)
        if not 0 <= bits <= 8:
            raise ValueError(f"Posterize keeps 0..8 bits, got {bits}")
        w[1] = ~(2 ** (8 - bits) - 1) & 0xff
    elif name == "Solarize":
        w[1] = min(max(int(math.ceil(float(magnitude))), 0), 256)  # the first v with not (v < threshold)
    return w


@dataclass
class CropAugPlan:
    """The per-image random decisions of RandomResizedCrop, RandomHorizontalFlip and RandAugment
    for one batch of decoded images, as plain host data.

    sizes [B, 2] (H, W of every decoded image), out_size (OH, OW), boxes [B, 4] (top, left, h, w
    inside the image), flip [B] (0 / 1), ops: per image a list of (op name, magnitude) -- every
    image the same number (1..4) --, the magnitude signed and meaning what torchvision hands to its
    functional (``ra_magnitude``).  The ops act on the OH x OW crop."""
    sizes: np.ndarray
    out_size: Tuple[int, int]
    boxes: np.ndarray
    flip: np.ndarray
    ops: List[List[Tuple[str, float]]]

    def __post_init__(self):
        self.sizes = np.asarray(self.sizes, np.int64).reshape(-1, 2)
        self.boxes = np.asarray(self.boxes, np.int64).reshape(-1, 4)
        self.flip = np.asarray(self.flip, np.int64).reshape(-1)
        self.out_size = (int(self.out_size[0]), int(self.out_size[1]))
        self.ops = [[(str(n), float(m)) for n, m in per] for per in self.ops]
        self.validate()

    @property
    def B(self) -> int:
        return self.sizes.shape[0]

    @property
    def num_ops(self) -> int:
        return len(self.ops[0]) if self.ops else RA_NUM_OPS

    @staticmethod
    def identity(sizes, out_size) -> "CropAugPlan":
        """The whole image resized, no flip, one Identity op."""
        sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        boxes = np.concatenate([np.zeros_like(sizes), sizes], axis=1)
        return CropAugPlan(sizes, out_size, boxes, np.zeros(len(sizes), np.int64), [[("Identity", 0.0)] for _ in sizes])

    @staticmethod
    def from_bins(sizes, out_size, boxes, flip, ops, magnitude: int = RA_MAGNITUDE,
                  num_bins: int = RA_BINS) -> "CropAugPlan":
        """Every decision pinned; ops: per image a list of (op name, sign), sign +1 / -1 (ignored
        by the unsigned ops), the magnitude taken from bin ``magnitude`` of ``num_bins``."""
        OH, OW = int(out_size[0]), int(out_size[1])
        full = [[(n, (float(sg) if n in RA_SIGNED else 1.0) * ra_magnitude(n, OH, OW, magnitude, num_bins))
                 for n, sg in per] for per in ops]
        return CropAugPlan(sizes, out_size, boxes, flip, full)

    @staticmethod
    def sample(sizes, out_size, generator: Optional[torch.Generator] = None, num_ops: int = RA_NUM_OPS,
               magnitude: int = RA_MAGNITUDE, num_bins: int = RA_BINS, scale=RRC_SCALE, ratio=RRC_RATIO,
               flip_p: float = 0.5) -> "CropAugPlan":
        """Draw a plan from torch's CPU generator; the same seed gives the same plan.

        RandomResizedCrop (torchvision ``get_params``): up to 10 tries of area = H W U(scale),
        r = exp(U(log ratio)), w = round(sqrt(area r)), h = round(sqrt(area / r)), the first with
        0 < w <= W and 0 < h <= H taken with top ~ U{0..H-h}, left ~ U{0..W-w}; else the central
        crop of the whole width or height clamped to the ratio bounds.  Flip with probability
        ``flip_p``.  RandAugment (``num_ops`` ops, bin ``magnitude`` of ``num_bins``, NEAREST, fill
        None): every op uniform over the 14, a signed op negated with probability 0.5.

        The distributions and formulas are torchvision's as published (v2 transforms, restated
        without torchvision at hand: unverified against torchvision itself); the random stream is
        not -- the draws of a batch are taken in bulk, a fixed number per image."""
        sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        B = len(sizes)
        OH, OW = int(out_size[0]), int(out_size[1])
        if not 1 <= num_ops <= sp.RA_MAX_OPS:
            raise ValueError(f"num_ops must be 1..{sp.RA_MAX_OPS}, got {num_ops}")
        c_try, c_op = 3, 3 + 2 * RRC_ATTEMPTS
        u = torch.rand(B, c_op + 2 * num_ops, generator=generator, dtype=torch.float64).numpy()
        l0, l1 = math.log(ratio[0]), math.log(ratio[1])
        boxes = np.zeros((B, 4), np.int64)
        ops: List[List[Tuple[str, float]]] = []
        for b, (H, W) in enumerate(sizes.tolist()):
            area = H * W
            for a in range(RRC_ATTEMPTS):
                target = area * (scale[0] + (scale[1] - scale[0]) * u[b, c_try + 2 * a])
                r = math.exp(l0 + (l1 - l0) * u[b, c_try + 2 * a + 1])
                w, h = int(round(math.sqrt(target * r))), int(round(math.sqrt(target / r)))
                if 0 < w <= W and 0 < h <= H:
                    top = min(int(u[b, 1] * (H - h + 1)), H - h)
                    left = min(int(u[b, 2] * (W - w + 1)), W - w)
                    break
            else:  # central fallback
                in_ratio = float(W) / float(H)
                if in_ratio < min(ratio):
                    w = W
                    h = int(round(w / min(ratio)))
                elif in_ratio > max(ratio):
                    h = H
                    w = int(round(h * max(ratio)))
                else:
                    w, h = W, H
                top, left = (H - h) // 2, (W - w) // 2
            boxes[b] = (top, left, h, w)
            per = []
            for k in range(num_ops):
                name = sp.RA_OPS[min(int(u[b, c_op + 2 * k] * len(sp.RA_OPS)), len(sp.RA_OPS) - 1)]
                m = ra_magnitude(name, OH, OW, magnitude, num_bins)
                if name in RA_SIGNED and u[b, c_op + 2 * k + 1] <= 0.5:
                    m = -m
                per.append((name, m))
            ops.append(per)
        return CropAugPlan(sizes, (OH, OW), boxes, (u[:, 0] < flip_p).astype(np.int64), ops)

    def kmax(self) -> int:
        """The largest tap count of the batch's boxes."""
        OH, OW = self.out_size
        return max([1] + [max(_taps(int(w), OW), _taps(int(h), OH)) for _, _, h, w in self.boxes])

    def validate(self) -> None:
        """Everything the kernels rely on; raises before anything reaches the device."""
        B = self.B
        OH, OW = self.out_size
        if OH <= 0 or OW <= 0:
            raise ValueError(f"output size {self.out_size}")
        if self.boxes.shape[0] != B or self.flip.shape[0] != B or len(self.ops) != B:
            raise ValueError("sizes, boxes, flip and ops must describe the same number of images")
        if B and not (1 <= self.num_ops <= sp.RA_MAX_OPS and all(len(p) == self.num_ops for p in self.ops)):
            raise ValueError(f"every image takes the same number of ops, 1..{sp.RA_MAX_OPS}")
        if not np.isin(self.flip, (0, 1)).all():
            raise ValueError("flip bits are 0 / 1")
        for (H, W), (top, left, h, w) in zip(self.sizes.tolist(), self.boxes.tolist()):
            if H <= 0 or W <= 0:
                raise ValueError("empty image")
            if not (0 <= top and 1 <= h and top + h <= H and 0 <= left and 1 <= w and left + w <= W):
                raise ValueError(f"box {(top, left, h, w)} outside its {H}x{W} image")
            if h > 100 * w:
                raise NotImplementedError(f"box {h}x{w}: aspect ratio above 100 (Pillow reorders its passes there)")
            if w > sp.CROP_MAX_W:
                raise NotImplementedError(f"box {w} pixels wide (limit {sp.CROP_MAX_W})")
        if self.kmax() > MAX_TAPS:
            raise NotImplementedError(f"downscale factor too large ({self.kmax()} taps > {MAX_TAPS})")
        for per in self.ops:
            for name, m in per:
                ra_words(name, m, OH, OW)

    def words(self) -> int:
        return (sp.CROP_PLAN_PER_IMAGE + sp.RA_PLAN_PER_OP * self.num_ops) * self.B

    def pack(self, out: Optional[np.ndarray] = None, row_origin: bool = False) -> np.ndarray:
        """int32 words: [B][8] for sdp_resized_crop, then [B][num_ops][8] for sdp_randaugment
        (layouts: include/sdpnet_hip.h).  ``row_origin``: boxes for images that were cut to the
        box's rows before packing (top 0)."""
        if out is None:
            out = np.empty(self.words(), np.int32)
        out[:] = 0
        B, n = self.B, sp.CROP_PLAN_PER_IMAGE * self.B
        crop = out[:n].reshape(B, sp.CROP_PLAN_PER_IMAGE)
        crop[:, 0:4] = self.boxes
        if row_origin:
            crop[:, 0] = 0
        crop[:, 4] = self.flip
        OH, OW = self.out_size
        ra = out[n:].reshape(B, self.num_ops, sp.RA_PLAN_PER_OP) if B else out[n:]
        for b, per in enumerate(self.ops):
            for k, (name, m) in enumerate(per):
                ra[b, k] = np.array(ra_words(name, m, OH, OW), np.int64).astype(np.int32)
        return out


class TrainImageTransform:
    """The reference's whole ``train_transforms`` plus its collate on decoded images:
    ``__call__(images, labels, crop_plan=None, plan=None) -> (images [B, 3, OH, OW] of ``dtype`` on
    ``device``, targets)``.  targets as for ``TrainBatchTransform``.

    images: a sequence of decoded images (PIL, ndarray or uint8 tensor, HWC) of any sizes; labels:
    int64 [B] (a tensor on either side, or a sequence of ints).  The rows of every image that its
    crop box covers, both plans, the image table and the host labels are packed into one of two
    alternating pinned buffers and uploaded with one copy; the only host wait is on the copy out
    of that buffer two batches earlier.  Then sdp_resized_crop -> sdp_randaugment (in place) ->
    sdp_train_batch_aug.  The flip happens in the crop kernel (``flip_p``), so the ``AugPlan``
    drawn here has no flips."""

    def __init__(self, image_size=(224, 224), num_classes: int = 1000, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 device="cuda", dtype=torch.float32, mix: Optional[str] = "reference", erase_p: float = 0.25,
                 flip_p: float = 0.5, num_ops: int = RA_NUM_OPS, magnitude: int = RA_MAGNITUDE,
                 num_magnitude_bins: int = RA_BINS, scale=RRC_SCALE, ratio=RRC_RATIO,
                 generator: Optional[torch.Generator] = None):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrainImageTransform runs sdp_resized_crop / sdp_randaugment / sdp_train_batch_aug; "
                               "the HIP path has no CPU fallback")
        sp.dcode(dtype)
        self.dtype = dtype
        self.mix, self.erase_p, self.flip_p = mix, float(erase_p), float(flip_p)
        self.num_ops, self.magnitude, self.num_magnitude_bins = int(num_ops), int(magnitude), int(num_magnitude_bins)
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.generator = generator
        self.lut = normalize_lut(mean, std).to(self.device)
        self._staging = (_Staging(), _Staging())
        self._turn = 0
        self.jpeg_decoder: Optional[JpegDecoder] = None  # made on the first batch that holds encoded JPEGs

    def sample_crop(self, sizes) -> CropAugPlan:
        return CropAugPlan.sample(sizes, self.image_size, self.generator, self.num_ops, self.magnitude,
                                  self.num_magnitude_bins, self.scale, self.ratio, self.flip_p)

    def sample_batch(self, B: int) -> AugPlan:
        return AugPlan.sample(B, *self.image_size, self.generator, self.mix, self.erase_p, 0.0)

    def sample(self, sizes) -> Tuple[CropAugPlan, AugPlan]:
        """Both plans of one batch, drawn in the order ``__call__`` draws them."""
        crop = self.sample_crop(sizes)
        return crop, self.sample_batch(crop.B)

    def _call_encoded(self, images: Sequence, labels, crop_plan: Optional[CropAugPlan], plan: Optional[AugPlan]):
        """A batch with encoded JPEGs in it: the whole images are decoded on the device (one upload of
        coefficients), the plans and host labels follow in a second, small upload, and the same three
        kernels run with the boxes in whole-image coordinates."""
        B = len(images)
        OH, OW = self.image_size
        labels = torch.as_tensor(labels).to(torch.int64)
        if labels.shape != (B,):
            raise ValueError(f"labels must be [B] = [{B}], got {tuple(labels.shape)}")
        if self.jpeg_decoder is None:
            self.jpeg_decoder = JpegDecoder(self.device)
        pix_d, offs_d, hw_d, offs, sizes = self.jpeg_decoder.decode_with_host(images)
        if crop_plan is None:
            crop_plan = self.sample_crop(sizes)
        if crop_plan.out_size != self.image_size or not np.array_equal(crop_plan.sizes, sizes):
            raise ValueError("crop_plan was made for other image sizes or another output size")
        if plan is None:
            plan = self.sample_batch(B)
        if (plan.B, plan.H, plan.W) != (B, OH, OW):
            raise ValueError(f"plan is for {(plan.B, plan.H, plan.W)}, the batch is {(B, OH, OW)}")
        if not labels.is_cuda and not (0 <= int(labels.min()) and int(labels.max()) < self.num_classes):
            raise ValueError(f"label outside [0, {self.num_classes})")
        boxes = crop_plan.boxes
        # one pinned buffer: crop + RandAugment plan | batch plan | host labels
        n_crop, n_plan = 4 * crop_plan.words(), 4 * plan.words()
        o_plan = _round_up(n_crop, 16)
        o_lab = _round_up(o_plan + n_plan, 16)
        st = self._staging[self._turn]
        self._turn ^= 1
        host = st.take(o_lab + (0 if labels.is_cuda else 8 * B))
        hv = host.numpy()
        crop_plan.pack(hv[:n_crop].view(np.int32))
        plan.pack(hv[o_plan:o_plan + n_plan].view(np.int32))
        if not labels.is_cuda:
            hv[o_lab:o_lab + 8 * B].view(np.int64)[:] = labels.numpy()
        with torch.cuda.device(self.device):
            dev = host.to(self.device, non_blocking=True)
            st.event = torch.cuda.Event()
            st.event.record()
            n_box = 4 * sp.CROP_PLAN_PER_IMAGE * B
            crop_d = dev[:n_box].view(torch.int32)
            ra_d = dev[n_box:n_crop].view(torch.int32)
            plan_d = dev[o_plan:o_plan + n_plan].view(torch.int32)
            labels_d = labels if labels.is_cuda else dev[o_lab:o_lab + 8 * B].view(torch.int64)
            u8 = sp.resized_crop(pix_d, offs_d, hw_d, crop_d, self.image_size, crop_plan.kmax(), int(boxes[:, 2].max()),
                                 int(boxes[:, 3].max()), host=(offs, sizes, boxes))
            sp.randaugment(u8, ra_d, crop_plan.num_ops)
            mixed = plan.mode != MODE_NONE
            out, targets = sp.train_batch_aug(u8, labels_d, self.lut, plan_d, self.num_classes, self.dtype, mixed,
                                              channels_last=True)
        if mixed:
            return out, targets
        return out, (labels_d if labels.is_cuda else labels_d.clone())

    def __call__(self, images: Sequence, labels, crop_plan: Optional[CropAugPlan] = None,
                 plan: Optional[AugPlan] = None):
        if len(images) and any(_is_encoded(im) for im in images):
            return self._call_encoded(images, labels, crop_plan, plan)
        arrs = [_as_rgb_u8(im) for im in images]
        B = len(arrs)
        OH, OW = self.image_size
        labels = torch.as_tensor(labels).to(torch.int64)
        if labels.shape != (B,):
            raise ValueError(f"labels must be [B] = [{B}], got {tuple(labels.shape)}")
        if B == 0:
            return torch.empty(0, 3, OH, OW, dtype=self.dtype, device=self.device), labels.to(self.device)
        sizes = np.array([a.shape[:2] for a in arrs], np.int64)
        if crop_plan is None:
            crop_plan = self.sample_crop(sizes)
        if crop_plan.out_size != self.image_size or not np.array_equal(crop_plan.sizes, sizes):
            raise ValueError("crop_plan was made for other image sizes or another output size")
        if plan is None:
            plan = self.sample_batch(B)
        if (plan.B, plan.H, plan.W) != (B, OH, OW):
            raise ValueError(f"plan is for {(plan.B, plan.H, plan.W)}, the batch is {(B, OH, OW)}")
        if not labels.is_cuda and not (0 <= int(labels.min()) and int(labels.max()) < self.num_classes):
            raise ValueError(f"label outside [0, {self.num_classes})")
        # only the rows under a box travel: image b becomes its rows [top, top + h), full width
        boxes = crop_plan.boxes
        hw = np.stack([boxes[:, 2], sizes[:, 1]], axis=1)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offs = np.zeros(B, np.int64)
        offs[1:] = np.cumsum(nbytes)[:-1]
        # one pinned buffer: crop + RandAugment plan | batch plan | offs | hw | host labels | pixels
        n_crop, n_plan = 4 * crop_plan.words(), 4 * plan.words()
        o_plan = _round_up(n_crop, 16)
        o_offs = _round_up(o_plan + n_plan, 16)
        o_hw = _round_up(o_offs + 8 * B, 16)
        o_lab = _round_up(o_hw + 8 * B, 16)
        o_img = _round_up(o_lab + (0 if labels.is_cuda else 8 * B), 16)
        n_img = int(nbytes.sum())
        st = self._staging[self._turn]
        self._turn ^= 1
        host = st.take(o_img + n_img)
        hv = host.numpy()
        crop_plan.pack(hv[:n_crop].view(np.int32), row_origin=True)
        plan.pack(hv[o_plan:o_plan + n_plan].view(np.int32))
        hv[o_offs:o_offs + 8 * B].view(np.int64)[:] = offs
        hv[o_hw:o_hw + 8 * B].view(np.int32)[:] = hw.astype(np.int32).reshape(-1)
        if not labels.is_cuda:
            hv[o_lab:o_lab + 8 * B].view(np.int64)[:] = labels.numpy()
        for a, (top, _, h, _), o, n in zip(arrs, boxes.tolist(), offs.tolist(), nbytes.tolist()):
            hv[o_img + o:o_img + o + n].reshape(h, a.shape[1], 3)[:] = a[top:top + h]
        with torch.cuda.device(self.device):
            dev = host.to(self.device, non_blocking=True)
            st.event = torch.cuda.Event()
            st.event.record()
            n_box = 4 * sp.CROP_PLAN_PER_IMAGE * B
            crop_d = dev[:n_box].view(torch.int32)
            ra_d = dev[n_box:n_crop].view(torch.int32)
            plan_d = dev[o_plan:o_plan + n_plan].view(torch.int32)
            offs_d = dev[o_offs:o_offs + 8 * B].view(torch.int64)
            hw_d = dev[o_hw:o_hw + 8 * B].view(torch.int32).view(B, 2)
            labels_d = labels if labels.is_cuda else dev[o_lab:o_lab + 8 * B].view(torch.int64)
            pix_d = dev[o_img:o_img + n_img]
            max_h, max_w = int(boxes[:, 2].max()), int(boxes[:, 3].max())
            rows = np.concatenate([np.zeros((B, 1), np.int64), boxes[:, 1:]], axis=1)
            u8 = sp.resized_crop(pix_d, offs_d, hw_d, crop_d, self.image_size, crop_plan.kmax(), max_h, max_w,
                                 host=(offs, hw, rows))
            sp.randaugment(u8, ra_d, crop_plan.num_ops)
            mixed = plan.mode != MODE_NONE
            out, targets = sp.train_batch_aug(u8, labels_d, self.lut, plan_d, self.num_classes, self.dtype, mixed,
                                              channels_last=True)
        if mixed:
            return out, targets
        return out, (labels_d if labels.is_cuda else labels_d.clone())


def train_transforms(image_size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda",
                     dtype=torch.float32, **kw) -> TrainImageTransform:
    """hf_dataset_generator.py:43-57 signature; returns the batched device transform (which also
    does the collate's CutMix / MixUp; ``mix=None`` leaves the int64 labels)."""
    return TrainImageTransform(image_size, mean=mean, std=std, device=device, dtype=dtype, **kw)


class DeviceAugLoader:
    """Wraps a loader of (uint8 images, int labels) host batches into an iterable of
    (images, targets) device batches: drops into ``Trainer(train_data=...)`` (its ``.to(gpu_id)``
    on the batches is then a no-op; ``len()`` and ``.sampler`` are the loader's).  With a
    ``TrainImageTransform`` the loader yields (list of decoded images, labels) instead, i.e. its
    ``collate_fn`` returns lists."""

    def __init__(self, loader, transform):
        self.loader = loader
        self.transform = transform

    def __len__(self) -> int:
        return len(self.loader)

    @property
    def sampler(self):
        return self.loader.sampler

    def __iter__(self):
        for images, labels in self.loader:
            yield self.transform(images, labels)
