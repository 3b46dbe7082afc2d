"""numpy restatement of baseline JPEG decoding, as the hybrid decoder splits it.

``entropy_decode(data)`` is a pure-Python marker parser and Huffman decoder that yields what
``sdp_jpeg_entropy_decode`` yields: the quantised coefficients, component-major, blocks in raster
order over the padded MCU grid, 64 values per block in natural order, and the quantisation tables in
natural order.  ``reconstruct(...)`` is what ``sdp_jpeg_reconstruct`` computes: dequantisation, the
13-bit fixed-point Loeffler / Ligtenberg / Moschytz inverse DCT (columns first), "fancy" 2:1 chroma
upsampling with the edges of the component's true size, and the 16-bit fixed-point YCbCr -> RGB
conversion.  ``decode(data)`` chains the two into HWC uint8 RGB; tests pin it to Pillow's
``Image.open(...).convert("RGB")`` bit for bit.

It takes the streams the product takes (one scan, Huffman, 8-bit, grey or YCbCr at 1x1 / 2x1 / 2x2)
and raises ``Unsupported`` or ``Malformed`` elsewhere; it is written for clarity, not for speed.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], np.int64)

MODE_444, MODE_H2V1, MODE_H2V2 = 0, 1, 2


class Unsupported(Exception):
    """A well-formed JPEG outside the subset."""


class Malformed(Exception):
    """Not a decodable JPEG."""


@dataclass
class Coefficients:
    W: int
    H: int
    ncomp: int
    mode: int                       # MODE_444 (also grey), MODE_H2V1, MODE_H2V2
    grids: List[Tuple[int, int]]    # per component (blocks wide, blocks high) of the padded MCU raster
    restart_interval: int
    coef: np.ndarray                # int16 [sum of blocks * 64]
    qt: np.ndarray                  # uint8 [ncomp, 64], natural order

    @property
    def ncoef(self) -> int:
        return 64 * sum(w * h for w, h in self.grids)


def _huff_table(counts, symbols) -> Dict[Tuple[int, int], int]:
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, data: bytes, pos: int):
        self.d, self.pos, self.acc, self.n = data, pos, 0, 0

    def bit(self) -> int:
        if self.n == 0:
            d = self.d
            if self.pos >= len(d):
                raise Malformed("entropy data truncated")
            b = d[self.pos]
            if b == 0xFF:
                if self.pos + 1 >= len(d) or d[self.pos + 1] != 0:
                    raise Malformed("entropy data ends before the last MCU")
                self.pos += 2
            else:
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise Malformed("code not in the Huffman table")

    def align(self):
        self.n = 0


def _extend(v: int, s: int) -> int:
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def entropy_decode(data: bytes) -> Coefficients:
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Malformed("no SOI")
    pos = 2
    qts: Dict[int, np.ndarray] = {}
    dc: Dict[int, dict] = {}
    ac: Dict[int, dict] = {}
    frame = None
    ri = 0
    adobe_transform = None
    while True:
        if pos + 4 > len(d) or d[pos] != 0xFF:
            raise Malformed("marker expected")
        while pos < len(d) and d[pos] == 0xFF:
            pos += 1
        if pos + 2 >= len(d):
            raise Malformed("truncated")
        m = d[pos]
        pos += 1
        n = (d[pos] << 8) | d[pos + 1]
        seg = d[pos + 2:pos + n]
        if n < 2 or pos + n > len(d):
            raise Malformed("segment length")
        pos += n
        if m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Unsupported("sample precision")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if H == 0:
                raise Unsupported("DNL")
            if nc not in (1, 3):
                raise Unsupported("component count")
            frame = (W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i])
                            for i in range(nc)])
        elif m == 0xC2 or (0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8)):
            raise Unsupported(f"SOF{m - 0xC0}")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                syms = list(seg[q + 17:q + 17 + sum(counts)])
                (dc if tc == 0 else ac)[th] = _huff_table(counts, syms)
                q += 17 + sum(counts)
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise Unsupported("16-bit quantisation table")
                t = np.zeros(64, np.uint8)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qts[seg[q] & 15] = t
                q += 65
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe_transform = seg[11]
        elif m == 0xDA:
            break
        elif m == 0xDC:
            raise Unsupported("DNL")
    if frame is None:
        raise Malformed("SOS before SOF")
    W, H, comps = frame
    nc = len(comps)
    if seg[0] != nc:
        raise Unsupported("several scans")
    if nc == 3:
        if adobe_transform == 0 or bytes(c[0] for c in comps) == b"RGB":
            raise Unsupported("RGB colour transform")
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling")
        mode = {(1, 1): MODE_444, (2, 1): MODE_H2V1, (2, 2): MODE_H2V2}[(hs, vs)]
    else:
        hs = vs = 1  # a single-component scan is non-interleaved: one block per MCU
        mode = MODE_444
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    grids = [(mx * hs, my * vs)] + [(mx, my)] * (nc - 1)
    tabs = []
    for i in range(nc):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td not in dc or ta not in ac or comps[i][3] not in qts:
            raise Malformed("undefined table")
        tabs.append((dc[td], ac[ta]))
    base = np.cumsum([0] + [w * h for w, h in grids])
    coef = np.zeros(int(base[-1]) * 64, np.int16)
    br = _Bits(d, pos)
    pred = [0] * nc
    rst = 0
    for mcu in range(mx * my):
        if ri and mcu and mcu % ri == 0:
            br.align()
            p = br.pos
            while p + 1 < len(d) and d[p] == 0xFF and d[p + 1] == 0xFF:
                p += 1
            if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD0 + rst:
                raise Malformed("restart marker")
            br.pos = p + 2
            rst = (rst + 1) & 7
            pred = [0] * nc
        row, col = divmod(mcu, mx)
        for c in range(nc):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            for v in range(cv):
                for h in range(ch):
                    blk = int(base[c]) + (row * cv + v) * grids[c][0] + col * ch + h
                    out = coef[blk * 64:blk * 64 + 64]
                    s = br.symbol(tabs[c][0])
                    if s > 11:
                        raise Malformed("DC category")
                    pred[c] += _extend(br.bits(s), s) if s else 0
                    out[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.symbol(tabs[c][1])
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63 or s > 10:
                                raise Malformed("AC coefficient")
                            out[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            break
    p = br.pos
    while p + 1 < len(d) and d[p] == 0xFF and d[p + 1] == 0xFF:
        p += 1
    if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD9:
        raise Malformed("no EOI after the last MCU")
    qt = np.stack([qts[c[3]] for c in comps])
    return Coefficients(W, H, nc, mode, grids, ri, coef, qt)


# ---------------------------------------------------------------------------
# reconstruction
# ---------------------------------------------------------------------------
def _descale(x: np.ndarray, n: int) -> np.ndarray:
    return (x + (1 << (n - 1))) >> n


def _idct_1d(v: List[np.ndarray], shift: int) -> List[np.ndarray]:
    """One pass over eight int64 arrays (the same entry of every block)."""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    t2 = z1 - z3 * 15137
    t3 = z1 + z2 * 6270
    t0 = (v[0] + v[4]) << 13
    t1 = (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return [_descale(x, shift) for x in o]


def idct_blocks(coef: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """int16 [n, 64] quantised blocks, uint8 [64] table -> uint8 [n, 8, 8] samples."""
    x = coef.reshape(-1, 8, 8).astype(np.int64) * qt.reshape(8, 8).astype(np.int64)
    cols = _idct_1d([x[:, k, :] for k in range(8)], 11)          # down the columns: index k is the row
    ws = np.stack(cols, axis=1)
    rows = _idct_1d([ws[:, :, k] for k in range(8)], 18)
    return np.clip(np.stack(rows, axis=2) + 128, 0, 255).astype(np.uint8)


def plane(coef: np.ndarray, qt: np.ndarray, bw: int, bh: int) -> np.ndarray:
    s = idct_blocks(coef, qt).reshape(bh, bw, 8, 8)
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _up_h2v1(s: np.ndarray) -> np.ndarray:
    s = s.astype(np.int64)
    n = s.shape[1]
    out = np.empty((s.shape[0], 2 * n), np.int64)
    if n <= 2:
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def _up_h2v2(s: np.ndarray) -> np.ndarray:
    s = s.astype(np.int64)
    h, n = s.shape
    if n <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    above = np.concatenate([s[:1], s[:-1]], axis=0)
    below = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * h, 2 * n), np.int64)
    for k, nb in ((0, above), (1, below)):
        c = 3 * s + nb
        left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        o = np.empty((h, 2 * n), np.int64)
        o[:, 0::2] = (3 * c + left + 8) >> 4
        o[:, 1::2] = (3 * c + right + 7) >> 4
        o[:, 0] = (4 * c[:, 0] + 8) >> 4
        o[:, -1] = (4 * c[:, -1] + 7) >> 4
        out[k::2] = o
    return out


def reconstruct(c: Coefficients) -> np.ndarray:
    """HWC uint8 RGB of one image's coefficients."""
    W, H = c.W, c.H
    base = np.cumsum([0] + [w * h for w, h in c.grids]) * 64
    planes = [plane(c.coef[base[i]:base[i + 1]], c.qt[i], *c.grids[i]) for i in range(c.ncomp)]
    y = planes[0][:H, :W].astype(np.int64)
    if c.ncomp == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    if c.mode == MODE_444:
        cb, cr = (p[:H, :W].astype(np.int64) for p in planes[1:])
    else:
        cw = -(-W // 2)
        chh = -(-H // 2) if c.mode == MODE_H2V2 else H
        up = _up_h2v2 if c.mode == MODE_H2V2 else _up_h2v1
        cb, cr = (up(p[:chh, :cw])[:H, :W] for p in planes[1:])
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    return reconstruct(entropy_decode(data))


# ---------------------------------------------------------------------------
# the test grid
# ---------------------------------------------------------------------------
GRID_SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 33), (29, 37), (3, 64), (40, 3), (50, 70)]  # (W, H)
GRID_SUBSAMPLING = (0, 1, 2)
GRID_QUALITY = (50, 92, 100)


def grid_image(W: int, H: int, colour: bool, seed: int) -> np.ndarray:
    """A deterministic image with smooth gradients, an edge and noise: every coefficient band is used."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = []
    for k in range(3 if colour else 1):
        a = 127 + 90 * np.sin((xx * (0.11 + 0.05 * k) + yy * (0.07 + 0.03 * k)) + seed + k)
        a += 60 * ((xx + 2 * yy + 5 * k) % 23 < 9)
        a += rng.normal(0, 18, (H, W))
        ch.append(np.clip(a, 0, 255))
    a = np.stack(ch, axis=2).astype(np.uint8)
    return a if colour else a[:, :, 0]


def encode(arr: np.ndarray, quality: int = 90, subsampling: int = 2, restart: int = 0, **kw) -> bytes:
    import io

    from PIL import Image
    buf = io.BytesIO()
    if restart:
        kw["restart_marker_blocks"] = restart
    kw["subsampling"] = subsampling   # Pillow writes the factors into a greyscale frame header too
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def grid_cases(extra_sizes=()):
    """(name, jpeg bytes) over sizes x subsampling x colour / grey x restart on / off x quality.
    Greyscale takes the subsampling axis too: Pillow then writes 2x1 / 2x2 factors into the frame
    header of a single-component file, whose scan is not interleaved all the same."""
    out = []
    seed = 0
    for (W, H) in list(GRID_SIZES) + list(extra_sizes):
        for colour in (True, False):
            for sub in GRID_SUBSAMPLING:
                for q in GRID_QUALITY:
                    for rst in (0, 1):
                        seed += 1
                        img = grid_image(W, H, colour, seed)
                        out.append((f"{W}x{H}-{'rgb' if colour else 'l'}-s{sub}-q{q}-r{rst}",
                                    encode(img, q, sub, rst)))
    return out


def pillow_rgb(data: bytes) -> np.ndarray:
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


# ---------------------------------------------------------------------------
# files outside the subset, and damaged ones
# ---------------------------------------------------------------------------
def progressive_file(W: int = 40, H: int = 30) -> bytes:
    return encode(grid_image(W, H, True, 901), 85, 2, progressive=True)


def cmyk_file(W: int = 24, H: int = 18) -> bytes:
    import io

    from PIL import Image
    rgb = grid_image(W, H, True, 902)
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, "JPEG", quality=85)
    return buf.getvalue()


def _find(data: bytes, marker: int) -> int:
    """Offset of the FF of the first segment with this marker code (walking the segments)."""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        if data[pos + 1] == marker:
            return pos
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise ValueError(f"marker {marker:#x} not found")


def h1v2_file() -> bytes:
    """A 4:4:4 file whose frame header is patched to luma sampling 1x2."""
    d = bytearray(encode(grid_image(16, 16, True, 903), 85, 0))
    sof = _find(d, 0xC0)
    assert d[sof + 11] == 0x11
    d[sof + 11] = 0x12
    return bytes(d)


def adobe_rgb_file() -> bytes:
    """A three-component file with an Adobe APP14 segment that says transform 0 (RGB)."""
    d = encode(grid_image(16, 16, True, 904), 85, 0)
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    return d[:2] + app14 + d[2:]


def undefined_huffman_id_file(data: bytes) -> bytes:
    """``data`` with the first scan component's table selectors set to tables 3 / 3."""
    d = bytearray(data)
    d[_find(d, 0xDA) + 6] = 0x33
    return bytes(d)
