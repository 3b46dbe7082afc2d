"""GPU: the small-M split-K GEMM (sdp_gemm_splitk) with explicit ``bm`` and ``splits``.

Judged by the scheme of tests/test_gpu_bf16_budget.py, whose data maker and rounding model are
imported, not restated: inputs in bf16, the reference in fp64 of those values, rows scaled by powers
of two, ``assert_elementwise`` with e = 2 (K + N_EPI) 2^-24 * terms (it holds for any summation
order, so for any number of K-slices) and ``assert_rms_vs_model`` at the GEMM margin 1.10 against
the single-rounding model of kernel 9: bf16(act(acc + b [+ R]) [+ R]).

Shapes are the smallest at which the kernel can go wrong: one row, fewer rows than an MFMA tile,
one short of / one past the 64-row tile, several tiles with a ragged last one (199, also ragged for
bm = 128); one, three and twelve column chunks; one K-tile (one slice only), K-tile counts that
split evenly and unevenly (K = 320: five tiles in two or three slices) and one tile per slice."""
import functools

import pytest
import torch

import bf16_budget as bb
import input_families as fam
import sdpnet_hip as sp
import test_gpu_bf16_budget as tb

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HIP_INVALID = 1  # hipErrorInvalidValue

MS = [1, 3, 63, 65, 199]
NS = [64, 192, 768]
KS = [64, 192, 320, 768]
BMS = [64, 128]


def splits_of(K):
    return sorted({s for s in (1, 2, 3, K // 64) if 1 <= s <= K // 64})


@functools.lru_cache(maxsize=None)
def ln_data(shape):
    """LN-fold operands of one shape (statistics of d["xl"] by parts, folded weight), made once."""
    M, N, K = tb.shape_of(shape)
    d = tb.gemm_data(shape)
    part = torch.empty(M, K // 64, 2, device=DEV)
    sp.row_partials(sp.dense(d["xl"]), M, K, part)
    st = torch.empty(M, 2, device=DEV)
    sp.ln_stats(part, sp.dense(d["xl"]), M, K, 1e-5, st)
    w, colsum, cvec = sp.fold_ln_weight(d["w32"], d["g"], d["be"], d["b"], BF)
    return st, colsum, cvec, w


def run_case(shape, epi, bm, splits, out, res, pbuf=None, ws=None):
    """One gemm_splitk call of epilogue ``epi`` into ``out``; returns gemm_expect's tuple."""
    M, N, K = tb.shape_of(shape)
    d = tb.gemm_data(shape)
    has_b, act, resid = tb.EPILOGUES[epi]
    x, w, bias, ln, lnx = d["x"], d["w"], d["b"] if has_b else None, None, None
    if epi == "ln_fold":
        st, colsum, bias, w = ln_data(shape)
        x, ln, lnx = d["xl"], (st, colsum), (st, colsum, bias)
    L = sp.lib()
    oldg = L.sdp_gemm_set_exact_gelu(1 if act == "gelu_erf" else 0)
    try:
        sp.gemm_splitk(sp.dense(x), w, out, M, N, K, bm, splits, bias=bias, resid=res if resid else None,
                       act=tb.ACT_CODE[act], resid_pre=resid == "pre", ln=ln, part=pbuf, ws=ws)
        torch.cuda.synchronize()
    finally:
        L.sdp_gemm_set_exact_gelu(oldg)
    return tb.gemm_expect(9, d, epi, K, "xl", lnx, w.double() if ln else None)


def chunk_stats64(y):
    """fp64 {mean, M2} of every 64-column chunk of the stored values y [M, N] -> [M, N/64] each."""
    c = y.double().view(y.shape[0], -1, 64)
    mean = c.mean(-1)
    return mean, ((c - mean[..., None]) ** 2).sum(-1), c.abs().amax(-1)


def assert_chunk_partials(pbuf, y, what):
    """part against the fp64 statistics of the stored bf16 chunk, with input_families' bounds for a
    64-term row: |d mean| <= C u max|x|; M2 is a variance sum, 4 C u relative (twice the 2 C u that
    stat_bounds allows rstd, which is its inverse square root), plus what the mean's own error adds
    to a sum of squared deviations, C (d mean)^2."""
    mean, m2, amax = chunk_stats64(y)
    mb = 64 * fam.U * amax
    got_mean, got_m2 = pbuf[..., 0].double(), pbuf[..., 1].double()
    assert torch.isfinite(pbuf).all(), what
    assert ((got_mean - mean).abs() <= mb).all(), f"{what}: chunk mean"
    assert ((got_m2 - m2).abs() <= 4 * 64 * fam.U * m2 + 64 * mb * mb).all(), f"{what}: chunk M2"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_splitk_budget(M, N, K):
    shape = (M, N, K)
    d = tb.gemm_data(shape)
    for epi in tb.EPILOGUES:
        for bm in BMS:
            for splits in splits_of(K):
                y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
                pbuf = torch.full((M, N // 64, 2), float("nan"), device=DEV) if epi == "resid_part" else None
                ref, model, e, terms = run_case(shape, epi, bm, splits, sp.dense(y), sp.dense(d["r"]), pbuf)
                what = f"splitk {shape} {epi} bm{bm} S{splits}"
                bb.assert_elementwise(y, ref, e, what)
                bb.assert_rms_vs_model(y, model, ref, bb.budget_scale(ref, terms), 1.10, what)
                if pbuf is not None:
                    assert_chunk_partials(pbuf, y, what)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("epi", ["plain", "resid_post", "resid_pre", "resid_pre_gelu", "resid_part", "ln_fold"])
def test_splitk_row_maps_inplace_residual_and_guard_bands(epi, bm, splits):
    """Output and in-place residual are the image rows of a [B, R + P, C] token buffer; the token
    buffer and the workspace (sized exactly by sdp_gemm_splitk_ws_bytes) lie between NaN bands."""
    M, N, K = tb.shape_of(tb.ROWMAP)
    d = tb.gemm_data(tb.ROWMAP)
    B, R, P = tb.RM_B, tb.RM_R, tb.RM_P
    Nt, G = R + P, 4096
    big = torch.full((G + B * Nt * N + G,), float("nan"), dtype=BF, device=DEV)
    tok = big[G:G + B * Nt * N].view(B * Nt, N)
    tok.copy_(tb.randn(B * Nt, N, seed=22).to(BF))
    tok.view(B, Nt, N)[:, R:] = d["r"].view(B, P, N)
    tok0 = tok.clone()
    need = sp.gemm_splitk_ws_bytes(M, N, bm, splits)
    assert need == (splits * M * N * 4 if splits > 1 else 0)
    wbig = torch.full((G + need // 4 + G,), float("nan"), device=DEV)
    ws = wbig[G:G + need // 4] if need else None
    pbuf = torch.full((B * Nt, N // 64, 2), float("nan"), device=DEV) if epi == "resid_part" else None
    out = sp.Rows(tok, N, P, Nt, R)
    ref, model, e, terms = run_case(tb.ROWMAP, epi, bm, splits, out, out, pbuf, ws)
    got = tok.view(B, Nt, N)[:, R:].reshape(M, N)
    assert torch.equal(tok.view(B, Nt, N)[:, :R], tok0.view(B, Nt, N)[:, :R])  # register rows: bit-unchanged
    assert torch.isnan(big[:G]).all() and torch.isnan(big[-G:]).all()
    assert torch.isnan(wbig[:G]).all() and torch.isnan(wbig[-G:]).all()
    what = f"splitk rowmap {epi} bm{bm} S{splits}"
    bb.assert_elementwise(got, ref, e, what)
    bb.assert_rms_vs_model(got, model, ref, bb.budget_scale(ref, terms), 1.10, what)
    if pbuf is not None:
        pv = pbuf.view(B, Nt, N // 64, 2)
        assert torch.isnan(pv[:, :R]).all()  # partials are written at the physical rows of the output only
        assert_chunk_partials(pv[:, R:].reshape(M, N // 64, 2), got, what)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("bm", BMS)
def test_splitk_partials_on_input_families(bm, splits):
    """{mean, M2} of rows whose offset is far above their spread (and the other LayerNorm
    families): a one-pass M2 = sum x^2 - 64 mean^2 fails here.  X . I^T stores the family rows
    exactly, so the stored values are known; the partials are judged per chunk and, combined by
    sdp_ln_stats as the model combines them, by input_families.assert_stats."""
    C = 192
    M = 5 * len(fam.FAMILIES)
    x, names = fam.family_rows(M, C, BF, seed=5)
    x = x.to(DEV)
    eye = torch.eye(C, dtype=BF, device=DEV)
    y = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    part = torch.full((M, C // 64, 2), float("nan"), device=DEV)
    sp.gemm_splitk(sp.dense(x), eye, sp.dense(y), M, C, C, bm, splits, part=part)
    torch.cuda.synchronize()
    assert torch.equal(y, x)
    assert_chunk_partials(part, y, f"families bm{bm} S{splits}")
    st = torch.empty(M, 2, device=DEV)
    sp.ln_stats(part, sp.dense(y), M, C, 1e-5, st)
    fam.assert_stats(st[:, 0], st[:, 1], y, 1e-5, names, f"splitk part + ln_stats bm{bm} S{splits}")


@pytest.mark.parametrize("M,N,K", [(199, 768, 768), (65, 192, 320), (3, 64, 192)])
def test_splitk_is_deterministic(M, N, K):
    d = tb.gemm_data((M, N, K))
    for bm in BMS:
        for splits in [s for s in splits_of(K) if s > 1]:
            outs = []
            for _ in range(5):
                y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
                sp.gemm_splitk(sp.dense(d["x"]), d["w"], sp.dense(y), M, N, K, bm, splits, bias=d["b"],
                               resid=sp.dense(d["r"]), act=1)
                outs.append(y)
            torch.cuda.synchronize()
            for y in outs[1:]:
                assert torch.equal(y, outs[0]), (M, N, K, bm, splits)


def _raw_call(x, w, y, M, N, K, bm, splits, ws, ws_bytes):
    st = torch.cuda.current_stream().cuda_stream
    return sp.lib().sdp_gemm_splitk(sp.BF16, x.data_ptr(), x.shape[1], 0, 0, 0, w.data_ptr(), w.shape[1], None,
                                    None, 0, 0, 0, 0, y.data_ptr(), y.shape[1], 0, 0, 0, M, N, K, 0, 0, None, None,
                                    None, bm, splits, ws.data_ptr() if ws is not None else None, ws_bytes, st)


@pytest.mark.parametrize("what,N,bm,splits,short", [
    ("bad bm", 128, 32, 1, False), ("bad bm", 128, 96, 2, False), ("splits 0", 128, 64, 0, False),
    ("splits > K/64", 128, 64, 4, False), ("short ws", 128, 64, 3, True), ("N 100", 100, 64, 1, False)])
def test_splitk_invalid_arguments_launch_nothing(what, N, bm, splits, short):
    M, K = 70, 192
    x = torch.ones(M, K, dtype=BF, device=DEV)
    w = torch.ones(128, K, dtype=BF, device=DEV)
    y = torch.full((M, 128), float("nan"), dtype=BF, device=DEV)
    wsn = max(splits, 1) * M * 128
    ws = torch.full((wsn,), float("nan"), device=DEV)
    ws_arg = ws[:wsn - 4] if short else ws
    # the C entry refuses before any launch
    assert _raw_call(x, w, y, M, N, K, bm, splits, ws, (wsn - 4) * 4 if short else wsn * 4) == HIP_INVALID
    # and so does the checked wrapper
    with pytest.raises((ValueError, RuntimeError)):
        sp.gemm_splitk(sp.Rows(x, K), w, sp.Rows(y, 128), M, N, K, bm, splits, ws=ws_arg)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(ws).all(), what
    if splits >= 1 and bm in BMS:
        assert sp.gemm_splitk_ws_bytes(M, 128, bm, splits) == (splits * M * 128 * 4 if splits > 1 else 0)
    else:
        assert sp.gemm_splitk_ws_bytes(M, 128, bm, splits) == -1
