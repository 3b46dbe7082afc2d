"""CPU: the rounding-budget checks (tests/bf16_budget.py) can tell right from wrong.

Torch emulations only -- bf16 inputs, fp32 matmul, round-to-nearest-even -- of the fast GEMM and of
the flash attention (32-key online softmax, P rounded to bf16 for the numerator).  The correct
emulations pass both checks; each faulty variant that today's ``close()`` (1.2e-2 / 2e-2 of the
global maximum) lets through fails.  One variant is NOT caught and is recorded as a blind spot
(test_blind_spot_p_truncation_under_qk_norm)."""
import math

import pytest
import torch

import bf16_budget as bb

BF = torch.bfloat16
GEMM_SHAPES = [(300, 384, 768), (257, 264, 64)]
ATTN_SHAPES = [(200, 96), (53, 32)]
H = 2


def _trunc32(y32):
    """fp32 -> bf16 by truncation."""
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


_GEMM = {}


def gemm_case(M, N, K):
    if (M, N, K) not in _GEMM:
        g = torch.Generator().manual_seed(1000 + K)
        x = (torch.randn(M, K, generator=g).double() * bb.pow2((M, 1), -6, 6, 1)).to(BF)
        w = (torch.randn(N, K, generator=g).double() * 0.05 * bb.pow2((N, 1), -3, 3, 2)).to(BF)
        ref = x.double() @ w.double().t()
        sabs = x.double().abs() @ w.double().abs().t()
        e = 2.0 * K * 2.0 ** -24 * sabs  # K - 1 accumulations at 2^-23 each (products are exact)
        _GEMM[(M, N, K)] = (x, w, ref, sabs, e, x.float() @ w.float().t())
    return _GEMM[(M, N, K)]


def gemm_checks(y, M, N, K, what):
    x, w, ref, sabs, e, _ = gemm_case(M, N, K)
    bb.assert_elementwise(y, ref, e, what)
    bb.assert_rms_vs_model(y, bb.rne_bf16(ref), ref, bb.budget_scale(ref, sabs), 1.10, what)


def fails(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_correct_emulation_passes(M, N, K):
    acc = gemm_case(M, N, K)[5]
    gemm_checks(acc.to(BF), M, N, K, f"gemm emulation {M}x{N}x{K}")


def _acc_rounded_every_64(M, N, K):
    x, w = gemm_case(M, N, K)[:2]
    acc = torch.zeros(M, N)
    for k0 in range(0, K, 64):
        acc = (acc + x[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().t()).to(BF).float()
    return acc.to(BF)


def _small_rows_zeroed(M, N, K):
    x, _, _, _, _, acc = gemm_case(M, N, K)
    y = acc.to(BF)
    y[x.float().abs().amax(1) <= 2.0 ** -4] = 0
    return y


GEMM_FAULTS = {
    "truncated": lambda M, N, K: _trunc32(gemm_case(M, N, K)[5]),
    "scaled_1.003": lambda M, N, K: (gemm_case(M, N, K)[5] * 1.003).to(BF),
    "acc_bf16_every_64k": _acc_rounded_every_64,
    "small_rows_zeroed": _small_rows_zeroed,
}


@pytest.mark.parametrize("fault", list(GEMM_FAULTS))
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_faulty_variants_fail(fault, M, N, K):
    if fault == "acc_bf16_every_64k" and K == 64:
        return  # one 64-wide step: the variant is the correct kernel
    y = GEMM_FAULTS[fault](M, N, K)
    x, w, ref, sabs, e, _ = gemm_case(M, N, K)
    # today's check lets it through ...
    assert (y.double() - ref).abs().max() <= 1.2e-2 * ref.abs().max(), "the variant is meant to pass close()"
    # ... the budget does not: the RMS against the model catches every variant, the element bound
    # every one that is not a uniform sub-ulp bias
    D = bb.budget_scale(ref, sabs)
    assert fails(bb.assert_rms_vs_model, y, bb.rne_bf16(ref), ref, D, 1.10, f"{fault} {M}x{N}x{K}")
    assert fails(gemm_checks, y, M, N, K, fault)
    if fault == "small_rows_zeroed":
        assert fails(bb.assert_elementwise, y, ref, e, fault)


# ------------------------------------------------------------------ attention
def attn_inputs(N, hd, norm):
    g = torch.Generator().manual_seed(7 * N + hd)
    q, k, v = (torch.randn(H, N, hd, generator=g) for _ in range(3))
    v = v.double() * bb.pow2((hd,), -3, 3, 3)
    if norm:
        q, k = q * 2.0 + 0.3, k * 2.0 - 0.2
        gq, gk = (2.0 + 0.1 * torch.randn(hd, generator=g) for _ in range(2))
        bq, bk = (0.1 * torch.randn(hd, generator=g) for _ in range(2))
        nrm = (gq, bq, gk, bk)
    else:
        q, nrm = q * 4.0, None  # scores of std ~ 4: a scale or exponent error shows
    return q.to(BF), k.to(BF), v.to(BF), nrm


def attn_emulate(q, k, v, nrm, scale, eps=1e-5, unbiased=False, p_trunc=False):
    """fp32 flash attention as the kernels run it: q / k head-normalised and rounded to bf16, 32-key
    tiles, running max, P rounded to bf16 for P V only, fp32 accumulators, bf16 output."""
    qf, kf, vf = q.float(), k.float(), v.float()
    if nrm is not None:
        def ln(x, g_, b_):
            mu = x.mean(-1, keepdim=True)
            var = x.var(-1, unbiased=unbiased, keepdim=True)
            return ((x - mu) * torch.rsqrt(var + eps) * g_ + b_).to(BF).float()
        qf, kf = ln(qf, nrm[0], nrm[1]), ln(kf, nrm[2], nrm[3])
    N = qf.shape[-2]
    m = torch.full(qf.shape[:-1] + (1,), -math.inf)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(qf)
    for k0 in range(0, N, 32):
        s = qf @ kf[..., k0:k0 + 32, :].transpose(-1, -2) * scale
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        pb = _trunc32(p).float() if p_trunc else p.to(BF).float()
        acc = acc * alpha + pb @ vf[..., k0:k0 + 32, :]
        m = mn
    return (acc / l).to(BF)


def attn_ratio(N, hd, norm, **fault):
    q, k, v, nrm = attn_inputs(N, hd, norm)
    scale = fault.pop("scale_factor", 1.0) / math.sqrt(hd)
    y = attn_emulate(q, k, v, nrm, scale, **fault)
    ref, model, sabs, *_ = bb.attention_ref_model(q.double(), k.double(), v.double(), 1.0 / math.sqrt(hd), nrm)
    D = bb.budget_scale(ref, sabs)
    return y, ref, model, D


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("N,hd", ATTN_SHAPES)
def test_attention_correct_emulation_passes(N, hd, norm):
    y, ref, model, D = attn_ratio(N, hd, norm)
    bb.assert_rms_vs_model(y, model, ref, D, 1.25, f"attention emulation N={N} hd={hd} norm={norm}")
    if not norm:
        q, k, v, _ = attn_inputs(N, hd, False)
        sabs = bb.attention_ref_model(q.double(), k.double(), v.double(), 1.0 / math.sqrt(hd))[2]
        e = bb.attention_element_bound(q.double(), k.double(), sabs, 1.0 / math.sqrt(hd))
        bb.assert_elementwise(y, ref, e, f"attention emulation N={N} hd={hd}")


def test_p_rounding_worst_case_is_2_pow_minus_8():
    """Why the attention element bound takes the P rounding at 2^-8 and not at the 2^-9 that the
    budget scale D carries: a value just above a power of two rounds by almost 2^-8 of itself (half
    an ulp at the bottom of the binade); 2^-9 holds only at the top.  Where one key dominates a
    row, its P rounds like that and the output moves by as much: on the MI355X and in the emulation
    alike, 1 element of 18,496 at (N 289, hd 32) exceeded the bound built on 2^-9."""
    x = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    rel = float((bb.rne_bf16(x) - x).abs() / x)
    assert 2.0 ** -9 < rel <= 2.0 ** -8


@pytest.mark.parametrize("N,hd", ATTN_SHAPES)
def test_attention_softmax_scale_off_by_1pct_fails(N, hd):
    y, ref, model, D = attn_ratio(N, hd, False, scale_factor=1.01)
    assert (y.double() - ref).abs().max() <= 2e-2 * ref.abs().max(), "the variant is meant to pass close()"
    assert fails(bb.assert_rms_vs_model, y, model, ref, D, 1.25, f"scale x1.01 N={N} hd={hd}")


@pytest.mark.parametrize("N,hd", ATTN_SHAPES)
def test_attention_unbiased_head_ln_variance_fails(N, hd):
    y, ref, model, D = attn_ratio(N, hd, True, unbiased=True)
    if hd >= 96:  # (hd = 32: the variance is off by 3 %, which close() sees as well)
        assert (y.double() - ref).abs().max() <= 2e-2 * ref.abs().max(), "the variant is meant to pass close()"
    assert fails(bb.assert_rms_vs_model, y, model, ref, D, 1.25, f"unbiased variance N={N} hd={hd}")


@pytest.mark.parametrize("N,hd", ATTN_SHAPES)
def test_attention_p_truncation_shows_without_qk_norm(N, hd):
    """Without the q/k norm the P rounding is a visible share of the error: truncating P moves the
    metric by 1.23x (N 200, hd 96) and 1.27x (N 53, hd 32) here -- the output rounding, which the
    fault leaves alone, is the rest.  That straddles the 1.25 margin, so P truncation alone is a
    BORDERLINE catch: these cases bound a P-rounding fault, they do not promise to flag it."""
    y, ref, model, D = attn_ratio(N, hd, False, p_trunc=True)
    try:
        ratio = bb.assert_rms_vs_model(y, model, ref, D, 1.25, f"P truncated N={N} hd={hd}")[2]
    except AssertionError:
        return  # caught outright
    assert ratio > 1.15, ratio  # not caught, but far from the correct emulation's 0.96 .. 1.00


@pytest.mark.parametrize("N,hd", ATTN_SHAPES)
def test_blind_spot_p_truncation_under_qk_norm(N, hd):
    """KNOWN BLIND SPOT: with the q/k head LayerNorm on, the rounding of the normalised q and k
    dominates the error, and truncating P instead of rounding it moves the metric by a few per
    cent only -- inside the 1.25 margin.  P rounding is checked by the no-norm cases (above)."""
    y, ref, model, D = attn_ratio(N, hd, True, p_trunc=True)
    rk, rm, ratio = bb.assert_rms_vs_model(y, model, ref, D, 1.25, f"P truncated under q/k norm N={N} hd={hd}")
    assert ratio < 1.25


# ------------------------------------------------------------------ the helpers themselves
def test_ulp_and_rounding_helpers():
    a = torch.tensor([1.0, 1.5, 1.9999999, 2.0, 0.75, 3e-5, 0.0, -260.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -23, 2.0 ** -133, 2.0],
                        dtype=torch.float64)
    assert torch.equal(bb.ulp_bf16(a), want)
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 37.0
    x32 = x.float()  # fp32 -> bf16 is one rounding in torch
    assert torch.equal(bb.rne_bf16(x32.double()), x32.to(BF).double())
    assert torch.equal(bb.trunc_bf16(x32.double()), _trunc32(x32).double())
    # a value the double -> float -> bfloat16 casts round twice: just above a bf16 tie
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(bb.rne_bf16(t)) == 1.0 + 2.0 ** -7
    ref = torch.tensor([1.0, 100.0], dtype=torch.float64)
    bb.assert_elementwise(torch.tensor([1.0 + 2.0 ** -8, 100.25]), ref, 0.0, "half an ulp")
    assert fails(bb.assert_elementwise, torch.tensor([1.0 + 2.0 ** -7, 100.0]), ref, 0.0, "one ulp")
