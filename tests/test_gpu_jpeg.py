"""GPU: the hybrid JPEG decoder -- sdp_jpeg_reconstruct on a heterogeneous batch against Pillow,
the Pillow fallback of JpegDecoder, the refusals, and the transforms fed with JPEG bytes against the
same transforms fed with the Pillow-decoded arrays.  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

import golden_util as gu
import jpeg_oracle as jo
import preprocess as pp
import sdpnet_hip as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5
GAP = 80          # sentinel bytes in front of, between and behind the images of pix
LARGE = (333, 301)  # several hundred pixels a side: interior MCU rows, many workgroups per image


@pytest.fixture(scope="module")
def grid():
    """[(name, jpeg bytes, Pillow's RGB pixels)] of the whole grid plus one large size."""
    return [(n, d, jo.pillow_rgb(d)) for n, d in jo.grid_cases(extra_sizes=[LARGE])]


def pack(files, gap=GAP):
    """Entropy-decode ``files`` on the host into the arrays sdp_jpeg_reconstruct takes:
    (coef int16, desc int32 [B * 64], pix offsets, pix bytes, ws bytes)."""
    W = sp.JPEG_DESC_WORDS
    desc = np.zeros(len(files) * W, np.int32)
    infos = []
    for d in files:
        rc, info = sp.jpeg_probe(d)
        assert rc == 0
        infos.append(info)
    n = np.array([int(i[10]) for i in infos], np.int64)
    coef_off = np.zeros(len(files), np.int64)
    coef_off[1:] = np.cumsum(n)[:-1]
    coef = np.zeros(int(n.sum()), np.int16)
    offs, at = [], gap
    for k, (d, info) in enumerate(zip(files, infos)):
        q = desc[k * W:(k + 1) * W]
        rc, _ = sp.jpeg_entropy_decode(d, coef[coef_off[k]:coef_off[k] + n[k]], q[sp.JPEG_DESC_QT:].view(np.uint8))
        assert rc == 0
        sp.jpeg_fill_desc(q, info, coef_off[k], coef_off[k], at)
        offs.append(at)
        at += int(info[0]) * int(info[1]) * 3 + gap
    return coef, desc, offs, at, int(n.sum())


def test_heterogeneous_batch_equals_pillow(grid):
    files = [d for _, d, _ in grid]
    assert len(files) == 396
    coef, desc, offs, n_pix, n_ws = pack(files)
    coef_d = torch.from_numpy(coef).to(DEV)
    desc_d = torch.from_numpy(desc).to(DEV)
    pix = torch.full((n_pix,), SENT, dtype=torch.uint8, device=DEV)
    ws = torch.full((n_ws + 4096,), SENT, dtype=torch.uint8, device=DEV)
    sp.jpeg_reconstruct(coef_d, desc, desc_d, len(files), ws, pix, ws_bytes=n_ws)   # one call
    torch.cuda.synchronize()
    got = pix.cpu().numpy()
    assert (ws[n_ws:] == SENT).all().item(), "workspace written beyond its stated size"
    bad, covered = [], np.zeros(n_pix, bool)
    for (name, _, want), o in zip(grid, offs):
        H, Wd = want.shape[:2]
        covered[o:o + H * Wd * 3] = True
        if not np.array_equal(got[o:o + H * Wd * 3].reshape(H, Wd, 3), want):
            bad.append(name)
    assert not bad, f"{len(bad)} of {len(grid)} images differ from Pillow: {bad[:10]}"
    assert (got[~covered] == SENT).all(), "pix written between or around the images"


def test_reconstruct_refuses_ranges_outside_the_buffers(grid):
    files = [d for n, d, _ in grid if n.startswith(("17x33-rgb-s2-q92", "9x17-l-s0-q50"))][:3]
    coef, desc, offs, n_pix, n_ws = pack(files)
    coef_d = torch.from_numpy(coef).to(DEV)
    W = sp.JPEG_DESC_WORDS

    def attempt(d, coef_t=coef_d, ws_bytes=n_ws, pix_bytes=n_pix):
        pix = torch.full((n_pix,), SENT, dtype=torch.uint8, device=DEV)
        ws = torch.full((n_ws,), SENT, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="leaves the buffers"):
            sp.jpeg_reconstruct(coef_t, d, torch.from_numpy(d).to(DEV), len(files), ws, pix, ws_bytes=ws_bytes,
                                pix_bytes=pix_bytes)
        torch.cuda.synchronize()
        assert (pix == SENT).all().item() and (ws == SENT).all().item(), "written before the refusal"

    last = (len(files) - 1) * W
    for word, value in ((6, coef.size - 8), (8, n_ws - 8), (10, n_pix - 8), (6, -8), (8, -8), (10, -1), (6, 4),
                        (0, 0), (1, 70000), (2, 2), (3, 3), (4, 1 << 20), (5, 0)):
        d = desc.copy()
        if word in (6, 8, 10):
            d[last + word:last + word + 2].view(np.int64)[:] = value
        else:
            d[last + word] = value
        attempt(d)
    attempt(desc.copy(), coef_t=coef_d[:-8])
    attempt(desc.copy(), ws_bytes=n_ws - 1)
    attempt(desc.copy(), pix_bytes=n_pix - GAP - 1)
    # and the unchanged descriptor passes
    pix = torch.full((n_pix,), SENT, dtype=torch.uint8, device=DEV)
    sp.jpeg_reconstruct(coef_d, desc, torch.from_numpy(desc).to(DEV), len(files), torch.empty(n_ws, dtype=torch.uint8,
                        device=DEV), pix)
    assert (pix[:GAP] == SENT).all().item() and not (pix[offs[0]:offs[0] + 64] == SENT).all().item()


def _unpack(pix, offs, hw):
    pix, offs, hw = pix.cpu().numpy(), offs.cpu().tolist(), hw.cpu().tolist()
    return [pix[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offs, hw)]


def test_decoder_falls_back_to_pillow_in_order(grid):
    ok = [d for n, d, _ in grid if n.startswith(("50x70-rgb-s2-q92-r1", "29x37-l-s1-q50-r0", "8x8-rgb-s1-q100-r0"))]
    assert len(ok) == 3
    items = [ok[0], jo.progressive_file(), ok[1], jo.cmyk_file(), jo.adobe_rgb_file(), ok[2],
             jo.grid_image(13, 11, True, 77)]
    dec = pp.JpegDecoder(DEV, num_threads=4)
    pix, offs, hw = dec.decode(items)
    assert pix.is_cuda and offs.dtype == torch.int64 and hw.dtype == torch.int32 and tuple(hw.shape) == (7, 2)
    assert dec.last_fallbacks == [1, 3, 4]
    want = [jo.pillow_rgb(it) if isinstance(it, bytes) else it for it in items]
    for k, (g, w) in enumerate(zip(_unpack(pix, offs, hw), want)):
        assert np.array_equal(g, w), k
    # types: bytearray and memoryview are encoded JPEGs too
    pix2, offs2, hw2 = dec.decode([bytearray(ok[0]), memoryview(ok[1])])
    for g, w in zip(_unpack(pix2, offs2, hw2), (want[0], want[2])):
        assert np.array_equal(g, w)
    assert pp.JpegDecoder(DEV, num_threads=999).num_threads == 16


def test_malformed_item_raises_with_its_index(grid):
    ok = [d for n, d, _ in grid if n.startswith("17x33-rgb-s2-q92")][:2]
    dec = pp.JpegDecoder(DEV, num_threads=2)
    for bad in (ok[0][:len(ok[0]) // 2], ok[0][:-2], jo.undefined_huffman_id_file(ok[0]), b"not a jpeg", b""):
        with pytest.raises(ValueError, match="item 2: malformed JPEG"):
            dec.decode([ok[0], ok[1], bad, ok[0]])
    # nothing of the failed batches is left behind: the next batch is complete and right
    pix, offs, hw = dec.decode(ok)
    for g, d in zip(_unpack(pix, offs, hw), ok):
        assert np.array_equal(g, jo.pillow_rgb(d))


@pytest.fixture(scope="module")
def photos():
    """Eight JPEGs of different sizes and modes, and Pillow's pixels of each."""
    spec = [(97, 80, True, 2, 0), (64, 64, True, 0, 0), (131, 75, True, 1, 3), (80, 120, False, 2, 0),
            (71, 93, True, 2, 2), (112, 112, True, 2, 0), (90, 61, True, 1, 0), (65, 129, False, 0, 1)]
    files = [jo.encode(jo.grid_image(w, h, c, 300 + k), 88, s, r) for k, (w, h, c, s, r) in enumerate(spec)]
    files[6] = jo.encode(jo.grid_image(90, 61, True, 306), 88, 1, progressive=True)   # one takes the fallback
    return files, [jo.pillow_rgb(d) for d in files]


def test_val_transform_on_jpeg_bytes(photos):
    files, arrays = photos
    for dtype in (torch.float32, torch.bfloat16):
        t = pp.ValTransform(image_size=(80, 80), crop_size=(64, 64), device=DEV, dtype=dtype)
        a, a8 = t(files, return_u8=True)
        b, b8 = t(arrays, return_u8=True)
        assert torch.equal(a8, b8) and torch.equal(a, b)
        mixed = t([files[0], arrays[1], files[2]] + arrays[3:])
        assert torch.equal(mixed, b)
    assert t.jpeg_decoder.last_fallbacks == []


def test_train_transform_on_jpeg_bytes(photos):
    files, arrays = photos
    B = len(files)
    labels = torch.arange(B) % 10
    for mix in ("reference", None):
        t = pp.TrainImageTransform(image_size=(56, 56), num_classes=10, device=DEV, mix=mix)
        g = torch.Generator().manual_seed(5)
        sizes = [a.shape[:2] for a in arrays]
        crop = pp.CropAugPlan.sample(sizes, (56, 56), g)
        plan = pp.AugPlan.sample(B, 56, 56, g, mix)
        xa, ta = t(files, labels, crop_plan=crop, plan=plan)
        xb, tb = t(arrays, labels, crop_plan=crop, plan=plan)
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert t.jpeg_decoder.last_fallbacks == [6]


def test_batches_over_a_bytes_dataset_gives_the_same_logits(photos):
    import model as ours
    files, arrays = photos
    meta, _ = gu.load_case("s_c256_h2")   # 112-px images
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    sd, _ = gu.build_inputs(meta, m)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    t = pp.ValTransform(image_size=(128, 128), crop_size=(112, 112), device=DEV)

    def run(images):
        out = []
        with torch.no_grad():
            for x, y in pp.batches(zip(images, range(len(images))), t, batch_size=3):
                out.append((m(x), y))
        return torch.cat([o for o, _ in out]), torch.cat([y for _, y in out])

    la, ya = run(files)
    lb, yb = run(arrays)
    assert la.shape[0] == len(files) and torch.equal(ya, yb)
    assert torch.isfinite(la).all().item() and torch.equal(la, lb)
