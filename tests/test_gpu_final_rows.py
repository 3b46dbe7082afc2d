"""GPU: the final encoder computed on the register rows only (logits from the registers).

Everything here is an equality: sdp_attention_rows runs the full kernel's per-tile code on the
rows it keeps, and the rows-limited final encoder runs the full call's GEMM kernels on the
gathered register rows, so the forced-full path (model.final_rows = False) is the reference
and torch.equal the bound.
"""
import pytest
import torch

import sdpnet_hip as sp
import synth

DEV = "cuda"
BF = torch.bfloat16


def test_attention_rows_rejects_bad_arguments_before_launch():
    L = sp.lib()
    args = (1, None, 8, None, 8, 1, 4, 1, 8, None, None, None, None, 1e-5, None, 0, 0)
    assert L.sdp_attention_rows(*args, 2, None) == 1      # null operands
    assert L.sdp_attention_rows(1, 8, 8, 8, 8, 1, 4, 1, 8, None, None, None, None, 1e-5, None, 0, 0, 0, None) == 1  # q_rows < 1


# ------------------------------------------------------------------ attention limit
_ATTN = {}


def _attn_case(N):
    """(qkv, norms, full-call output) for B = 3, H = 8, hd = 96; computed once per N."""
    if N not in _ATTN:
        B, H, hd = 3, 8, 96
        C = H * hd
        g = torch.Generator(device="cpu").manual_seed(700 + N)
        qkv = (2.0 * torch.randn(B * N, 3 * C, generator=g)).to(DEV).to(BF)
        qkn = tuple((0.1 * torch.randn(hd, generator=g) + (1.0 if i % 2 == 0 else 0.0)).to(DEV) for i in range(4))
        full = torch.full((B * N, C), 7.0, dtype=BF, device=DEV)
        sp.attention(qkv, full, B, N, H, hd, qk_norm=qkn, eps=1e-5)
        assert not (full == 7.0).all(dim=1).any(), "the full call left a row unwritten"
        _ATTN[N] = (qkv, qkn, full)
    return _ATTN[N]


@pytest.mark.gpu
@pytest.mark.parametrize("N,q_rows", [(200, 1), (200, 4), (200, 32), (200, 33), (200, 200),   # attn_fa4
                                      (260, 4), (260, 33),                                   # attn_fa6
                                      (40, 4)])                                              # padded last tile
def test_attention_leading_rows_equal_full_call(N, q_rows):
    B, H, hd = 3, 8, 96
    C = H * hd
    assert sp.attention_variant(BF, N, H, hd) == (3 if N > 256 else 4)
    qkv, qkn, full = _attn_case(N)
    out = torch.full((B * N, C), 7.0, dtype=BF, device=DEV)
    sp.attention(qkv, out, B, N, H, hd, qk_norm=qkn, eps=1e-5, q_rows=q_rows)
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, N, C)[:, :q_rows], full.view(B, N, C)[:, :q_rows])
    if q_rows >= N:
        assert torch.equal(out, full)
    else:
        # whole 32-row query tiles past the limit are skipped: their rows keep the fill
        t = -(-q_rows // 32) * 32
        assert (out.view(B, N, C)[:, t:] == 7.0).all()


# ------------------------------------------------------------------ model
_MODELS = {}


def _model(C, from_register=True, blocks=2):
    key = (C, from_register, blocks)
    if key not in _MODELS:
        import model as ours
        cfg = synth.canonical("XXS" if C == 128 else "M", num_blocks=blocks, head_output_from_register=from_register)
        assert cfg["embedding_dim"] == C and cfg["patch_size"] == 16
        torch.manual_seed(0)
        m = ours.MainModel(**cfg)
        m.load_state_dict(synth.synth_state_dict(m, 231424314))
        _MODELS[key] = m.to(DEV).eval()
    return _MODELS[key]


def _run(m, x, spy, full, streams, **kw):
    """Forward with the final encoder forced full or not; returns (outputs, q_rows of every
    attention call)."""
    m.final_rows = False if full else None
    m.num_streams = streams
    spy.clear()
    try:
        y = m(x, **kw)
        torch.cuda.synchronize()
    finally:
        m.final_rows = None
        m.num_streams = None
    return y, list(spy)


@pytest.fixture
def spy(monkeypatch):
    calls = []
    real = sp.attention

    def attention(*a, **kw):
        calls.append(kw.get("q_rows"))
        return real(*a, **kw)
    monkeypatch.setattr(sp, "attention", attention)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("num_registers,R", [(3, 4), (0, 1)])
@pytest.mark.parametrize("B,streams", [(3, 1), (130, 2), (131, 2)])   # 65 + 65 and a ragged 66 + 65
def test_register_row_logits_equal_full_path(spy, dtype, num_registers, R, B, streams):
    m = _model(128)
    x = synth_images_cached(B, 64).to(dtype)
    ref, qr = _run(m, x, spy, True, streams, num_registers=num_registers)
    assert qr == [None] * (3 * streams)
    y, qr = _run(m, x, spy, False, streams, num_registers=num_registers)
    per = [None, None, R]           # two blocks, then the final encoder
    assert qr == per * streams
    assert y.dtype == dtype and torch.isfinite(y.float()).all()
    assert torch.equal(y, ref)


_IMAGES = {}


def synth_images_cached(B, size):
    if (B, size) not in _IMAGES:
        _IMAGES[(B, size)] = synth.synth_images(3, B, size).to(DEV)
    return _IMAGES[(B, size)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_raw_outputs_keep_the_full_path(spy, dtype):
    m = _model(128)
    x = synth_images_cached(3, 64).to(dtype)
    ref, _ = _run(m, x, spy, True, 1, return_raw_outputs=True)
    out, qr = _run(m, x, spy, False, 1, return_raw_outputs=True)
    assert qr == [None] * 3
    assert len(out) == 3
    for a, b in zip(out, ref):      # logits, x, registers
        assert torch.equal(a, b)
    # and they are the logits of the rows-limited call
    y, qr = _run(m, x, spy, False, 1)
    assert qr[-1] == 4 and torch.equal(y, ref[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_pooled_head_keeps_the_full_path(spy, dtype):
    m = _model(128, from_register=False)
    x = synth_images_cached(3, 64).to(dtype)
    ref, _ = _run(m, x, spy, True, 1)
    y, qr = _run(m, x, spy, False, 1)
    assert qr == [None] * 3         # the head pools the image rows: nothing to skip
    assert torch.equal(y, ref)


@pytest.mark.gpu
def test_real_kernel_routes_at_c768(spy):
    """C = 768, 224 x 224, B = 2, bf16: attn_fa4 with the row limit, the fast GEMM on the
    register rows (8 rows, zero rows up to its smallest M) against the full 400-row calls."""
    m = _model(768, blocks=1)
    x = synth_images_cached(2, 224).to(BF)
    assert sp.attention_variant(BF, 200, 8, 96) == 4 and sp.gemm_variant(BF, 400, 768, 768) == 1
    ref, _ = _run(m, x, spy, True, 1)
    y, qr = _run(m, x, spy, False, 1)
    assert qr == [None, 4]
    assert torch.isfinite(y.float()).all() and torch.equal(y, ref)
