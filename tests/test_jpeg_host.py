"""CPU: the JPEG oracle against Pillow, and the host entropy decoder (sdp_jpeg_probe /
sdp_jpeg_entropy_decode through ctypes) against the oracle.

Grid: sizes 1x1, 7x5, 8x8, 9x17, 16x16, 17x33, 29x37, 3x64, 40x3, 50x70 x subsampling 0 / 1 / 2 x
quality 50 / 92 / 100 x RGB / L x restart markers on / off = 360 files.  Every host call writes
into a coefficient buffer that sits inside a sentinel-filled guard band, which must stay untouched."""
import numpy as np
import PIL
import pytest
import torch  # noqa: F401  (load torch's HIP runtime first, as the product does)

import jpeg_oracle as jo
import sdpnet_hip as sp

GUARD = 256
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def grid():
    return jo.grid_cases()


def host_decode(data, cap=None):
    """(code, info, coef or None, qt) with the guard band checked."""
    prc, pinfo = sp.jpeg_probe(data)
    n = int(pinfo[10]) if prc == 0 else 64
    cap = n if cap is None else cap
    buf = np.full(cap + 2 * GUARD, SENTINEL, np.int16)
    qt = np.zeros(192, np.uint8)
    rc, info = sp.jpeg_entropy_decode(data, buf[GUARD:GUARD + cap], qt)
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + cap:] == SENTINEL).all(), "guard band written"
    if prc != 0:
        assert rc == prc, (prc, rc)
    if rc == 0:
        assert np.array_equal(info, pinfo)
    return rc, info, (buf[GUARD:GUARD + n].copy() if rc == 0 else None), qt


def test_oracle_equals_pillow(grid):
    print(f"Pillow {PIL.__version__}")
    assert len(grid) == 360
    bad = [name for name, data in grid if not np.array_equal(jo.decode(data), jo.pillow_rgb(data))]
    assert not bad, f"oracle differs from Pillow {PIL.__version__} on {len(bad)} files: {bad[:8]}"


def test_host_decoder_equals_oracle(grid):
    restarts = 0
    for name, data in grid:
        o = jo.entropy_decode(data)
        rc, info, coef, qt = host_decode(data)
        assert rc == 0, (name, rc)
        grids = [g for g in o.grids] + [(0, 0)] * (3 - o.ncomp)
        mx, my = o.grids[-1] if o.ncomp == 3 else o.grids[0]
        want = [o.W, o.H, o.ncomp, o.mode, *[v for g in grids for v in g], o.ncoef, o.restart_interval, mx, my, 0, 0]
        assert info.tolist() == want, name
        assert np.array_equal(coef, o.coef), name
        assert np.array_equal(qt[:64 * o.ncomp].reshape(-1, 64), o.qt) and not qt[64 * o.ncomp:].any(), name
        restarts += o.restart_interval > 0
    assert restarts == len(grid) // 2


def test_grey_scan_is_not_interleaved():
    """Pillow writes greyscale files with 2x2 factors in the frame header; the scan has one block per MCU."""
    data = jo.encode(jo.grid_image(17, 33, False, 5), 90, 2)
    assert data[jo._find(data, 0xC0) + 11] == 0x22
    rc, info = sp.jpeg_probe(data)
    assert rc == 0 and info[:6].tolist() == [17, 33, 1, 0, 3, 5]


@pytest.mark.parametrize("make,code", [(jo.progressive_file, 1), (jo.cmyk_file, 4), (jo.h1v2_file, 5),
                                       (jo.adobe_rgb_file, 8)])
def test_unsupported_is_not_malformed(make, code):
    data = make()
    rc, _ = sp.jpeg_probe(data)
    assert rc == code
    assert host_decode(data)[0] == code
    if make is not jo.h1v2_file:
        with pytest.raises(jo.Unsupported):
            jo.entropy_decode(data)


@pytest.mark.parametrize("colour,restart", [(True, 1), (False, 0)])
def test_malformed_streams_are_refused(colour, restart):
    data = jo.encode(jo.grid_image(24, 17, colour, 7), 90, 2, restart)
    assert host_decode(data)[0] == 0
    for k in range(len(data)):
        assert host_decode(data[:k])[0] < 0, f"prefix of {k} bytes"
    assert data[-2:] == b"\xff\xd9"
    assert host_decode(data[:-2])[0] == -8
    assert host_decode(data[:-2] + b"\xff\xd0")[0] < 0
    bad_id = jo.undefined_huffman_id_file(data)
    assert sp.jpeg_probe(bad_id)[0] == -6 and host_decode(bad_id)[0] == -6
    if restart:
        d = bytearray(data)
        at = data.index(b"\xff\xd1", jo._find(data, 0xDA))
        d[at + 1] = 0xD3
        assert host_decode(bytes(d))[0] == -7
    n = int(sp.jpeg_probe(data)[1][10])
    for cap in (0, 63, n - 1):
        assert host_decode(data, cap)[0] == -9


def test_damaged_entropy_data_never_leaves_the_buffer():
    """Single-byte changes inside the scan: any outcome but a write outside the stated capacity
    (the guard band) or a crash."""
    data = jo.encode(jo.grid_image(29, 37, True, 11), 92, 2, 1)
    start = jo._find(data, 0xDA)
    rng = np.random.default_rng(0)
    outcomes = set()
    for k in range(start, len(data)):
        d = bytearray(data)
        d[k] ^= int(rng.integers(1, 256))
        outcomes.add(np.sign(host_decode(bytes(d))[0]))
    assert -1 in outcomes


def test_thread_pool_decodes_in_process(grid):
    """ctypes releases the GIL around the call and the decoder keeps no state: a pool gives the
    sequential results."""
    from concurrent.futures import ThreadPoolExecutor
    files = [d for _, d in grid[::9]]
    seq = [host_decode(d)[2] for d in files]
    with ThreadPoolExecutor(8) as pool:
        par = list(pool.map(lambda d: host_decode(d)[2], files * 4))
    for k, c in enumerate(par):
        assert np.array_equal(c, seq[k % len(files)])
