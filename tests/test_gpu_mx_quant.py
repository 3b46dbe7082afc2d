"""GPU: the MX quantiser (sdp_mx_quant_rows), bit-exact bytes and scales against tests/mx_oracle.py.

A scale one step too coarse is nearly invisible in a model's logits (rms error x 1.00 .. 1.02), a
truncating element rounding doubles it: only bit-exact checks catch the first, so everything here is
``torch.equal`` on the bytes."""
import pytest
import torch

import input_families as fam
import mx_oracle as mo
import sdpnet_hip as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def check(x_cpu, what, stats=None, rows=None, M=None):
    """Quantise x_cpu (bf16 / fp32 [M, K], or the rows ``rows`` of a buffer) on the GPU and compare
    with the oracle on the same values (with stats: the fp32 two-operation LayerNorm first)."""
    K = x_cpu.shape[-1]
    M = x_cpu.shape[0] if M is None else M
    v = x_cpu.float()
    if stats is not None:
        v = (v - stats[:, 0:1]) * stats[:, 1:2]          # exactly two fp32 operations, as the kernel
    want_q, want_s = mo.encode(v)
    G = 256
    qbig = torch.full((G + M * K + G,), 0xAB, dtype=torch.uint8, device=DEV)
    sbig = torch.full((G + M * (K // 32) + G,), 0xAB, dtype=torch.uint8, device=DEV)
    out = sp.MX(qbig[G:G + M * K].view(M, K), sbig[G:G + M * (K // 32)].view(M, K // 32))
    src = sp.dense(x_cpu.to(DEV)) if rows is None else rows
    sp.mx_quant_rows(src, M, K, stats=None if stats is None else stats.to(DEV).contiguous(), out=out)
    torch.cuda.synchronize()
    for b in (qbig, sbig):
        assert (b[:G] == 0xAB).all() and (b[-G:] == 0xAB).all(), f"{what}: guard bands"
    s, q = out.s.cpu(), out.q.cpu()
    assert torch.equal(s, want_s), f"{what}: {int((s != want_s).sum())} of {s.numel()} scales differ"
    assert torch.equal(q, want_q), f"{what}: {int((q != want_q).sum())} of {q.numel()} bytes differ"
    return q, s


def all_bf16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


def test_every_bf16_pattern_in_consecutive_blocks():
    """Blocks of 32 consecutive bit patterns (NaN and Inf patterns included: NaN blocks)."""
    q, s = check(all_bf16().view(512, 128), "consecutive patterns")
    assert (q == mo.NAN_BYTE).any() and (s == 0).any()


@pytest.mark.parametrize("big", [1.0, 1.875, 448.0, 3.0e38, 2.0 ** -100])
def test_every_bf16_pattern_next_to_a_large_neighbour(big):
    """Every finite pattern shares a block with one fixed large element, so that every value meets
    every e4m3 exponent, the subnormal grid and zero under a scale it does not set itself."""
    pat = all_bf16()
    pat = torch.where(torch.isfinite(pat.float()), pat, torch.zeros_like(pat))
    nblk = -(-65536 // 31)
    nblk += -nblk % 4
    body = torch.zeros(nblk * 31, dtype=BF)
    body[:65536] = pat
    x = torch.zeros(nblk, 32, dtype=BF)
    x[:, 0] = big
    x[:, 1:] = body.view(nblk, 31)
    check(x.view(-1, 128), f"neighbour {big}")


def test_fp32_inputs_around_the_1_75_threshold():
    t = torch.tensor(1.75)
    trio = torch.stack([torch.nextafter(t, torch.tensor(0.0)), t, torch.nextafter(t, torch.tensor(2.0))])
    g = torch.Generator().manual_seed(1)
    rows = []
    for ex in (-100, -20, 0, 7, 30, 100):
        x = torch.rand(3, 4, 32, generator=g) * 1.7          # the rest of each block stays below 1.75
        x[:, :, 5] = trio[:, None]
        rows.append((x * 2.0 ** ex).view(3, 128))
    q, s = check(torch.cat(rows), "fp32 threshold")
    assert (s[0::3] == s[1::3]).all() and (s[2::3].int() == s[1::3].int() + 1).all()


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_input_families_with_layernorm_statistics(dtype):
    """Rows whose offset is far above their spread, flat, tiny and huge rows: the quantiser must
    apply (x - mean) * rstd as those two fp32 operations, not x * rstd - mean * rstd."""
    C = 384
    M = 3 * len(fam.FAMILIES)
    x, names = fam.family_rows(M, C, dtype, seed=7)
    _, mean, rstd = fam.ln_ref64(x, None, None, 1e-5)
    stats = torch.cat([mean, rstd], 1).float()
    check(x, f"families {dtype}", stats=stats)


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_row_mapped_token_buffer_between_nan_bands(dtype):
    """The image rows of a [B, R + P, C] token buffer (grp = P, gstride = R + P, off = R); the
    register rows and the bands around the buffer are NaN: none of them may reach an output."""
    B, R, P, C, G = 3, 4, 49, 256, 4096
    Nt = R + P
    g = torch.Generator().manual_seed(3)
    big = torch.full((G + B * Nt * C + G,), float("nan"), dtype=dtype)
    tok = big[G:G + B * Nt * C].view(B, Nt, C)
    img = (torch.randn(B, P, C, generator=g) * torch.exp2(torch.randint(-8, 9, (B, P, 1), generator=g).float())).to(dtype)
    tok[:, R:] = img
    stats = torch.stack([torch.randn(B * P, generator=g) * 0.1, torch.rand(B * P, generator=g) + 0.5], 1)
    bigd = big.to(DEV)
    rows = sp.Rows(bigd[G:G + B * Nt * C].view(B * Nt, C), C, P, Nt, R)
    q, _ = check(img.reshape(B * P, C), f"rowmap {dtype}", rows=rows)
    assert not (q == mo.NAN_BYTE).any()
    check(img.reshape(B * P, C), f"rowmap + stats {dtype}", stats=stats, rows=rows)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 3, 65])
def test_small_shapes(M, K):
    g = torch.Generator().manual_seed(10 * M + K)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-30, 31, (M, 1), generator=g).float())
    check(x.to(BF), f"bf16 {M}x{K}")
    check(x, f"fp32 {M}x{K}")


def test_padded_row_strides():
    """Input, byte and scale rows wider than K."""
    M, K = 5, 128
    g = torch.Generator().manual_seed(2)
    xb = torch.full((M, K + 64), float("nan"), dtype=BF)
    xb[:, :K] = torch.randn(M, K, generator=g).to(BF)
    want_q, want_s = mo.encode(xb[:, :K].float())
    out = sp.MX(torch.full((M, K + 16), 0xAB, dtype=torch.uint8, device=DEV),
                torch.full((M, 8), 0xAB, dtype=torch.uint8, device=DEV))
    sp.mx_quant_rows(sp.Rows(xb.to(DEV), K + 64), M, K, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.q[:, :K].cpu(), want_q) and (out.q[:, K:] == 0xAB).all()
    assert torch.equal(out.s[:, :4].cpu(), want_s) and (out.s[:, 4:] == 0xAB).all()
