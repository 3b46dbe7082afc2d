"""GPU: the block-scaled MXFP8 GEMM (sdp_gemm_mx).

Operands are *already quantised* by tests/mx_oracle.py on the CPU, so the reference is the fp64
product of the decoded values and only the fp32 accumulation (and the epilogue) separates kernel
and reference.  Judged by the scheme of tests/test_gpu_bf16_budget.py, whose data maker, epilogue
table and rounding model are imported: ``assert_elementwise`` with e = 2 (K + N_EPI) 2^-24 * terms
and ``assert_rms_vs_model`` at 1.10 against the single-rounding model bf16(act(acc + b [+ R]) [+ R]).
That e is derived for round-to-nearest fp32 sums in any order; see profiles/mx_fp8.md for what the
scaled MFMA's internal 128-term sum was found to meet.  ``ln_fold`` is left out of the epilogue
list: sdp_gemm_mx has no LN fold (the LayerNorm is applied by the quantiser).

The lane-map test comes first in the file: exact small integers, scales of mixed powers of two,
an identity-like X against an asymmetric W; the result must be bit-equal.

Shapes are the smallest that can go wrong: one row, fewer rows than an MFMA tile, one short of /
one past the 128-row tile, several tiles with a ragged last one; N of half a column tile, one and a
half, and six; one, two, three (odd) and six K-tiles."""
import functools

import pytest
import torch

import bf16_budget as bb
import input_families as fam
import mx_oracle as mo
import sdpnet_hip as sp
import test_gpu_bf16_budget as tb
from test_gpu_gemm_splitk import assert_chunk_partials

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HIP_INVALID = 1

MS = [1, 3, 127, 129, 300]
NS = [64, 192, 768]
KS = [128, 256, 384, 768]
EPIS = [e for e in tb.EPILOGUES if e != "ln_fold"]
MX_EPIS = [e for e in EPIS if tb.EPILOGUES[e][2] is None]  # MX output takes no residual


def dev(q, s):
    return sp.MX(q.to(DEV).contiguous(), s.to(DEV).contiguous())


# ------------------------------------------------------------------------------- lane map
def test_lane_map_exact_integers():
    """X[m][k] = [k == m] under per-(row, block) scales, W[n][k] = asymmetric small integers under
    per-(row, block) scales: Y[m][n] = W[n][m] 2^(sx[m][m/32] + sw[n][m/32]) exactly, so a wrong
    k pairing of the two operands, a scale taken from another lane or block, or swapped output
    indices each change the result.  Then a dense +-1 pattern against the same W (per-row scales)."""
    M = K = 256
    N = 64
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    xv = (k == m).double()
    wv = (((3 * n + 5 * k + (n * k) % 7) % 13) - 6).double()
    blk = torch.arange(K // 32)[None, :]
    xs = (127 + (m + 2 * blk) % 5 - 2).to(torch.uint8)
    ws = (127 + (3 * n + blk) % 7 - 3).to(torch.uint8)
    xq, wq = mo.e4m3_bytes(xv).to(torch.uint8), mo.e4m3_bytes(wv).to(torch.uint8)
    ref = mo.decode(xq, xs) @ mo.decode(wq, ws).t()
    assert torch.equal(ref, ref.to(BF).double()) and len(ref.unique()) > 50
    y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    sp.gemm_mx(dev(xq, xs), dev(wq, ws), M, N, K, y=sp.dense(y))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref), "identity X: operand / scale lane map"

    xv = torch.where((k + m) % 8 == 0, 1.0 - 2.0 * ((k // 8 + m) % 2), 0.0).double()
    xs = (127 + m % 5 - 2).expand(M, K // 32).to(torch.uint8)
    ws = (127 + n % 7 - 3).expand(N, K // 32).to(torch.uint8)
    xq = mo.e4m3_bytes(xv).to(torch.uint8)
    ref = mo.decode(xq, xs) @ mo.decode(wq, ws).t()
    assert torch.equal(ref, ref.to(BF).double())
    sp.gemm_mx(dev(xq, xs), dev(wq, ws), M, N, K, y=sp.dense(y))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref), "dense +-1 X: k pairing inside a lane"


# ------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def mx_data(shape):
    """tb.gemm_data's operands quantised by the oracle, and the fp64 references of the decoded
    values in gemm_data's layout (so tb.gemm_expect applies unchanged).  Made once, left unchanged."""
    d = tb.gemm_data(shape)
    xq, xs = mo.encode(d["x"].float().cpu())
    wq, ws = mo.encode(d["w"].float().cpu())
    x64, w64 = mo.decode(xq, xs).to(DEV), mo.decode(wq, ws).to(DEV)
    return {"X": dev(xq, xs), "W": dev(wq, ws), "b": d["b"], "r": d["r"], "acc": x64 @ w64.t(),
            "sabs": x64.abs() @ w64.abs().t(), "x64": x64}


def run_case(shape, epi, y=None, out_mx=None, res=None, pbuf=None):
    M, N, K = tb.shape_of(shape)
    d = mx_data(shape)
    has_b, act, resid = tb.EPILOGUES[epi]
    L = sp.lib()
    oldg = L.sdp_gemm_set_exact_gelu(1 if act == "gelu_erf" else 0)
    try:
        sp.gemm_mx(d["X"], d["W"], M, N, K, y=y, out_mx=out_mx, bias=d["b"] if has_b else None,
                   resid=res if resid else None, act=tb.ACT_CODE[act], resid_pre=resid == "pre", part=pbuf)
        torch.cuda.synchronize()
    finally:
        L.sdp_gemm_set_exact_gelu(oldg)
    return tb.gemm_expect(9, d, epi, K)


# ------------------------------------------------------------------------------- bf16 output
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_gemm_mx_bf16_budget(M, N, K):
    shape = (M, N, K)
    d = mx_data(shape)
    for epi in EPIS:
        y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        pbuf = torch.full((M, N // 64, 2), float("nan"), device=DEV) if epi == "resid_part" else None
        ref, model, e, terms = run_case(shape, epi, y=sp.dense(y), res=sp.dense(d["r"]), pbuf=pbuf)
        what = f"gemm_mx {shape} {epi}"
        bb.assert_elementwise(y, ref, e, what)
        bb.assert_rms_vs_model(y, model, ref, bb.budget_scale(ref, terms), 1.10, what)
        if pbuf is not None:
            assert_chunk_partials(pbuf, y, what)


# ------------------------------------------------------------------------------- MX output
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_gemm_mx_mx_output(M, N, K):
    """Scale byte = the oracle's scale of the reference block, either neighbour where the reference
    maximum is within e of a threshold; each element within e + half the e4m3 spacing at the stored
    scale; the rms in those units at most 1.10 x that of the oracle-quantised reference."""
    shape = (M, N, K)
    for epi in MX_EPIS:
        G = 64
        qbig = torch.full((G + M * N + G,), 0xAB, dtype=torch.uint8, device=DEV)
        sbig = torch.full((G + M * (N // 32) + G,), 0xAB, dtype=torch.uint8, device=DEV)
        out = sp.MX(qbig[G:G + M * N].view(M, N), sbig[G:G + M * (N // 32)].view(M, N // 32))
        ref, _, e, _ = run_case(shape, epi, out_mx=out)
        what = f"gemm_mx MX out {shape} {epi}"
        assert (qbig[:G] == 0xAB).all() and (qbig[-G:] == 0xAB).all() and (sbig[:G] == 0xAB).all() \
            and (sbig[-G:] == 0xAB).all(), what
        ref, e = ref.cpu(), e.cpu().expand_as(ref)
        q, s = out.q.cpu(), out.s.cpu()
        rb, eb = ref.abs().view(M, -1, 32), e.view(M, -1, 32)
        amax, emax = rb.amax(-1), eb.amax(-1)
        lo, hi = mo.codes_of_amax((amax - emax).clamp_min(0)), mo.codes_of_amax(amax + emax)
        assert ((s.long() >= lo) & (s.long() <= hi)).all(), f"{what}: scale bytes"
        got = mo.decode(q, s)
        assert torch.isfinite(got).all(), what
        D = e + 0.5 * mo.e4m3_spacing(ref.abs() + e, s)
        err = (got - ref).abs()
        print(f"MX {what}: worst element at {float((err / D).max()):.3f} of its bound")
        assert (err <= D).all(), f"{what}: {int((err > D).sum())} elements outside e + spacing / 2"
        model = mo.fake_quant(ref.float())
        rk = float(((got - ref) / D).pow(2).mean().sqrt())
        rm = float(((model - ref) / D).pow(2).mean().sqrt())
        print(f"MX {what}: kernel {rk:.4f} oracle-quantised {rm:.4f} ratio {rk / rm if rm else 0.0:.3f}")
        assert rk <= 1.10 * rm, f"{what}: rms {rk:.4f} > 1.10 x {rm:.4f}"


# ------------------------------------------------------------------------------- row maps
@pytest.mark.parametrize("epi", ["plain", "resid_post", "resid_pre", "resid_pre_gelu", "resid_part"])
def test_gemm_mx_row_maps_inplace_residual_and_guard_bands(epi):
    """Output and in-place residual are the image rows of a [B, R + P, C] token buffer that lies
    between NaN bands; the partials land at the physical rows of the output only."""
    M, N, K = tb.shape_of(tb.ROWMAP)
    d = mx_data(tb.ROWMAP)
    B, R, P = tb.RM_B, tb.RM_R, tb.RM_P
    Nt, G = R + P, 4096
    big = torch.full((G + B * Nt * N + G,), float("nan"), dtype=BF, device=DEV)
    tok = big[G:G + B * Nt * N].view(B * Nt, N)
    tok.copy_(tb.randn(B * Nt, N, seed=22).to(BF))
    tok.view(B, Nt, N)[:, R:] = d["r"].view(B, P, N)
    tok0 = tok.clone()
    pbuf = torch.full((B * Nt, N // 64, 2), float("nan"), device=DEV) if epi == "resid_part" else None
    out = sp.Rows(tok, N, P, Nt, R)
    ref, model, e, terms = run_case(tb.ROWMAP, epi, y=out, res=out, pbuf=pbuf)
    got = tok.view(B, Nt, N)[:, R:].reshape(M, N)
    assert torch.equal(tok.view(B, Nt, N)[:, :R], tok0.view(B, Nt, N)[:, :R])  # register rows: bit-unchanged
    assert torch.isnan(big[:G]).all() and torch.isnan(big[-G:]).all()
    what = f"gemm_mx rowmap {epi}"
    bb.assert_elementwise(got, ref, e, what)
    bb.assert_rms_vs_model(got, model, ref, bb.budget_scale(ref, terms), 1.10, what)
    if pbuf is not None:
        pv = pbuf.view(B, Nt, N // 64, 2)
        assert torch.isnan(pv[:, :R]).all()
        assert_chunk_partials(pv[:, R:].reshape(M, N // 64, 2), got, what)


def test_gemm_mx_partials_on_input_families():
    """{mean, M2} of rows whose offset is far above their spread (and the other LayerNorm
    families) through an identity weight: every output is a single product, so the stored values
    are exactly the decoded MX rows."""
    C = 256
    M = 5 * len(fam.FAMILIES)
    x, names = fam.family_rows(M, C, BF, seed=5)
    xq, xs = mo.encode(x.float())
    eq, es = mo.encode(torch.eye(C))
    want = mo.decode(xq, xs)
    assert torch.equal(want, want.to(BF).double())
    y = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    part = torch.full((M, C // 64, 2), float("nan"), device=DEV)
    sp.gemm_mx(dev(xq, xs), dev(eq, es), M, C, C, y=sp.dense(y), part=part)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), want)
    assert_chunk_partials(part, y, "gemm_mx families")
    st = torch.empty(M, 2, device=DEV)
    sp.ln_stats(part, sp.dense(y), M, C, 1e-5, st)
    fam.assert_stats(st[:, 0], st[:, 1], y, 1e-5, names, "gemm_mx part + ln_stats")


# ------------------------------------------------------------------------------- the rest
@pytest.mark.parametrize("M,N,K", [(300, 768, 768), (129, 192, 384), (3, 64, 128)])
def test_gemm_mx_is_deterministic_and_independent_of_m(M, N, K):
    d = mx_data((M, N, K))
    outs = []
    for _ in range(5):
        y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        sp.gemm_mx(d["X"], d["W"], M, N, K, y=sp.dense(y), bias=d["b"], resid=sp.dense(d["r"]), act=1)
        outs.append(y)
    torch.cuda.synchronize()
    for y in outs[1:]:
        assert torch.equal(y, outs[0]), (M, N, K)
    # the first rows alone give the same bits: a fixed K order, whatever M is
    m1 = min(M, 2)
    y = torch.full((m1, N), float("nan"), dtype=BF, device=DEV)
    sp.gemm_mx(d["X"], d["W"], m1, N, K, y=sp.dense(y), bias=d["b"], resid=sp.dense(d["r"]), act=1)
    torch.cuda.synchronize()
    assert torch.equal(y, outs[0][:m1])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_gemm_mx_nonfinite_block_poisons_exactly_its_row(bad):
    M, N, K = 131, 192, 256
    d = tb.gemm_data((M, N, K))
    c = mx_data((M, N, K))
    x = d["x"].float().cpu().clone()
    x[77, 150] = bad
    xq, xs = mo.encode(x)
    for mx_out in (False, True):
        if mx_out:
            clean, dirty = sp.mx_empty(M, N, DEV), sp.mx_empty(M, N, DEV)
            sp.gemm_mx(c["X"], c["W"], M, N, K, out_mx=clean, bias=d["b"])
            sp.gemm_mx(dev(xq, xs), c["W"], M, N, K, out_mx=dirty, bias=d["b"])
            torch.cuda.synchronize()
            a, b = mo.decode(clean.q.cpu(), clean.s.cpu()), mo.decode(dirty.q.cpu(), dirty.s.cpu())
            keep = torch.arange(M) != 77
            assert torch.equal(clean.q[keep.to(DEV)], dirty.q[keep.to(DEV)])
            assert torch.equal(clean.s[keep.to(DEV)], dirty.s[keep.to(DEV)])
        else:
            a = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
            b = a.clone()
            sp.gemm_mx(c["X"], c["W"], M, N, K, y=sp.dense(a), bias=d["b"])
            sp.gemm_mx(dev(xq, xs), c["W"], M, N, K, y=sp.dense(b), bias=d["b"])
            torch.cuda.synchronize()
            a, b = a.cpu().double(), b.cpu().double()
        keep = torch.arange(M) != 77
        assert torch.isfinite(a).all()
        assert torch.isnan(b[77]).all() and torch.equal(a[keep], b[keep]), f"mx_out {mx_out}"


@pytest.mark.parametrize("what", ["K % 128", "N % 32, MX out", "null scales", "MX out + residual", "both outputs"])
def test_gemm_mx_invalid_arguments_launch_nothing(what):
    M, N, K = 70, 64, 128
    if what == "K % 128":
        K = 192
    if what == "N % 32, MX out":
        N = 48
    X, W = sp.mx_empty(M, 256, DEV), sp.mx_empty(64, 256, DEV)
    for t in (X.q, X.s, W.q, W.s):
        t.fill_(0x38)
    y = torch.full((M, 64), float("nan"), dtype=BF, device=DEV)
    oq = torch.full((M, 64), 0xAB, dtype=torch.uint8, device=DEV)
    os_ = torch.full((M, 2), 0xAB, dtype=torch.uint8, device=DEV)
    r = torch.ones(M, 64, dtype=BF, device=DEV)
    mx_out = what in ("N % 32, MX out", "MX out + residual", "both outputs")
    st = torch.cuda.current_stream().cuda_stream
    rc = sp.lib().sdp_gemm_mx(X.q.data_ptr(), 256, None if what == "null scales" else X.s.data_ptr(), 8,
                              W.q.data_ptr(), 256, W.s.data_ptr(), 8, None,
                              r.data_ptr() if what == "MX out + residual" else None, 64, 0, 0, 0,
                              y.data_ptr() if (not mx_out or what == "both outputs") else None, 64, 0, 0, 0,
                              oq.data_ptr() if mx_out else None, 64, os_.data_ptr() if mx_out else None, 2,
                              M, N, K, 0, 0, None, st)
    assert rc == HIP_INVALID, what
    if what != "null scales":  # and so does the checked wrapper
        with pytest.raises((ValueError, RuntimeError)):
            sp.gemm_mx(X, W, M, N, K, y=sp.Rows(y, 64) if (not mx_out or what == "both outputs") else None,
                       out_mx=sp.MX(oq, os_) if mx_out else None,
                       resid=sp.Rows(r, 64) if what == "MX out + residual" else None)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and (oq == 0xAB).all() and (os_ == 0xAB).all(), what
