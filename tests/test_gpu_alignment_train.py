"""GPU: the training-side entry points (train.hip, attn_train.hip, wgrad.hip, the layout kernels of
misc.hip) and the GEMMs that have no slower form, on misaligned bases and odd row strides.

Same harness and contract as test_gpu_alignment.py.  Two kinds of entry point meet here:

* those with an element-wise twin (sdp_act_fwd / _bwd, sdp_rowscale_add, sdp_act_rowscale_add,
  sdp_seg_colsum, sdp_ln_apply, sdp_ln_bwd, sdp_softmax_*, sdp_gemm_flex, the layout kernels): every
  perturbation must return 0 and meet the aligned test's bound (bit-equality where the aligned suite
  already asserts vector path == element path);
* those that refuse what their one kernel cannot take (sdp_ln_fwd, sdp_add_ln_fwd,
  sdp_rowscale_add_dropout / _mixed, sdp_gemm_train_epi, sdp_gemm_splitk, sdp_attn_train_fwd /
  _bwd): a refusal must leave every output byte untouched, and ``alignment.TABLE`` pins which
  perturbations are refused.  Their Python callers fall back (sdpnet_hip / sdpnet_train).

The C entry points are called directly where the Python wrapper fixes a row stride."""
import math

import pytest
import torch
import torch.nn.functional as F

import alignment as al
import sdpnet_hip as sp
from test_gpu_alignment import BF, DEV, DT_ID, DTYPES, F32, Op, close, rnd, rows, sweep
from test_gpu_kernels import ACTS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _full_precision_references():
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield
    torch.set_float32_matmul_precision(old)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pl(v):
    """pointer, row stride"""
    return [v.data_ptr(), v.stride(0)]


def ra(v):
    """pointer, row stride, dense row map"""
    return [v.data_ptr(), v.stride(0), 0, 0, 0]


def ptr(t):
    return None if t is None else t.data_ptr()


NOROWS = [None, 0, 0, 0, 0]


def equal_to(name, want):
    def verify(v):
        assert torch.equal(v[name], want), f"{name} differs from the aligned run"
    return verify


def same_as(name, want, dtype, rel):
    """bf16: bit for bit; fp32: the aligned test's bound, and the same zeros (the dropout mask)."""
    def verify(v):
        if dtype == BF:
            assert torch.equal(v[name], want), f"{name} differs from the aligned run"
        else:
            assert torch.equal(v[name] == 0, want == 0), f"{name}: the zeros (dropout mask) moved"
            close(v[name], want.double(), dtype, rel=rel, what=name)
    return verify


# =========================================================================== activation, row scale
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_act_fwd_bwd(dtype, code, p):
    """The 8-wide kernels and the one-element kernels give the same bits, dropout mask included
    (test_act_vector_path_equals_elementwise_path): kept across every shift."""
    M, N, L, dc = 37, 64, sp.lib(), sp.dcode(dtype)
    z = (torch.linspace(-6, 6, M * N, device=DEV).view(M, N) + 0.013).to(dtype)
    dy = rnd(M, N, dtype=dtype, seed=11)
    y0, dz0 = torch.empty_like(z), torch.empty_like(z)
    sp.act_fwd(z, y0, M, N, code, p, 99)
    sp.act_bwd(z, dy, dz0, M, N, code, p, 99)
    if p == 0.0:
        close(y0, ACTS[code](z.double()), dtype, rel=2e-5 if dtype == F32 else 2e-2, what="act_fwd")
    what = f"{DT_ID[dtype]} act {code} p {p}"
    sweep("sdp_act_fwd", dict(Z=Op(z), Y=Op(z, "out")),
          lambda v: L.sdp_act_fwd(dc, *pl(v["Z"]), *pl(v["Y"]), M, N, code, p, 99, stream()) == 0,
          same_as("Y", y0, dtype, 2e-5), what)
    sweep("sdp_act_bwd", dict(Z=Op(z), DY=Op(dy), DZ=Op(z, "out")),
          lambda v: L.sdp_act_bwd(dc, *pl(v["Z"]), *pl(v["DY"]), *pl(v["DZ"]), M, N, code, p, 99, stream()) == 0,
          same_as("DZ", dz0, dtype, 2e-5), what)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rowscale_add(dtype, act):
    """sdp_rowscale_add / sdp_act_rowscale_add: y = round(act(x)) * scale[m] + r."""
    M, N, L, dc = 37, 64, sp.lib(), sp.dcode(dtype)
    x, r = rnd(M, N, dtype=dtype, seed=21, scale=2.0), rnd(M, N, dtype=dtype, seed=22)
    sc = rnd(M, seed=23).abs() + 0.5
    a = ACTS[act](x.double())
    ref = (a.to(dtype).double() if act else a) * sc.double()[:, None] + r.double()
    ops = dict(X=Op(x), R=Op(r), Y=Op(x, "out"), scale=Op(sc))

    def call(v):
        tail = [*ra(v["X"]), ptr(v["scale"]), 1, *ra(v["R"]), *ra(v["Y"]), M, N, stream()]
        return (L.sdp_act_rowscale_add(dc, act, *tail) if act else L.sdp_rowscale_add(dc, *tail)) == 0
    sweep("sdp_act_rowscale_add" if act else "sdp_rowscale_add", ops, call,
          lambda v: close(v["Y"], ref, dtype, what="rowscale_add"), f"{DT_ID[dtype]} act {act}")


@pytest.mark.parametrize("xdt,ydt", [(BF, BF), (F32, F32), (BF, F32)], ids=["bf16", "fp32", "bf16-fp32"])
def test_rowscale_add_dropout_and_mixed_refuse_cleanly(xdt, ydt):
    """The fused-dropout and mixed-dtype forms exist on the 8-wide kernel only: any operand off a
    16-B row is refused (hipErrorNotSupported / hipErrorInvalidValue) before a launch, and
    sdpnet_hip.rowscale_add then runs the two passes -- the same bits
    (test_rowscale_dropout_fused_is_bit_identical), here on operands one element into their storage."""
    M, N, L = 37, 64, sp.lib()
    x, r = rnd(M, N, dtype=xdt, seed=31, scale=2.0), rnd(M, N, dtype=ydt, seed=32)
    sc = rnd(M, seed=33).abs() + 0.5
    y0 = torch.empty(M, N, dtype=ydt, device=DEV)
    sp.rowscale_add(sp.dense(x), sp.dense(y0), M, N, scale=sc, resid=sp.dense(r), p=0.25, seed=5, dmode=1)
    ops = dict(X=Op(x), R=Op(r), Y=Op(r, "out"), scale=Op(sc))
    sweep("sdp_rowscale_add_dropout", ops,
          lambda v: L.sdp_rowscale_add_dropout(sp.dcode(xdt), sp.dcode(ydt), *ra(v["X"]), ptr(v["scale"]), 1, *ra(v["R"]),
                                               *ra(v["Y"]), M, N, 0.25, 5, 1, stream()) == 0,
          equal_to("Y", y0), f"{DT_ID[xdt]}->{DT_ID[ydt]}")
    if xdt != ydt:
        m0 = torch.empty(M, N, dtype=ydt, device=DEV)
        sp.rowscale_add(sp.dense(x), sp.dense(m0), M, N, scale=sc, resid=sp.dense(r))
        sweep("sdp_rowscale_add_mixed", ops,
              lambda v: L.sdp_rowscale_add_mixed(sp.dcode(xdt), sp.dcode(ydt), 0, *ra(v["X"]), ptr(v["scale"]), 1,
                                                 *ra(v["R"]), *ra(v["Y"]), M, N, stream()) == 0,
              equal_to("Y", m0), f"{DT_ID[xdt]}->{DT_ID[ydt]}")
    else:   # the wrapper's two-pass fallback on dense operands at a storage offset of one element
        xs, rs = al.place(x, al.BASE[0], ld=N), al.place(r, al.BASE[0], ld=N)
        ys = al.place(r, al.BASE[0], ld=N, out=True)
        sp.rowscale_add(sp.Rows(xs, N), sp.Rows(ys, N), M, N, scale=sc, resid=sp.Rows(rs, N), p=0.25, seed=5, dmode=1)
        torch.cuda.synchronize()
        assert not al.findings(ys) and torch.equal(ys == 0, y0 == 0)
        close(ys, y0.double(), ydt, what="two-pass fallback")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_seg_colsum(dtype):
    G, ln, C, L = 2, 37, 128, sp.lib()
    X = rnd(G * ln, C, dtype=dtype, seed=10)
    ref = X.double().view(G, ln, C).sum(1)
    sweep("sdp_seg_colsum", dict(X=Op(X), out=Op(torch.empty(G, C, device=DEV), "out")),
          lambda v: L.sdp_seg_colsum(sp.dcode(dtype), *pl(v["X"]), G, ln, ln, 1, C, *pl(v["out"]), 1.0, 0,
                                     stream()) == 0,
          lambda v: close(v["out"], ref, F32, rel=1e-5, what="seg_colsum"), DT_ID[dtype])


# =========================================================================== training LayerNorm
def ln_data(dtype, M, C, eps=1e-5):
    x = (rnd(M, C, seed=13, scale=1.5) + rnd(M, 1, seed=14, scale=2.0)).to(dtype)
    g, b = rnd(C, seed=15, scale=0.2, shift=1.0), rnd(C, seed=16, scale=0.2)
    x64 = x.double()
    mean, rstd = x64.mean(1), 1 / torch.sqrt(x64.var(1, unbiased=False) + eps)
    st = torch.stack([mean, rstd], 1).float().contiguous()
    return x, g, b, st, mean, rstd


@pytest.mark.parametrize("M,C", [(5, 64), (77, 96), (9, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_ln_apply_and_ln_fwd(dtype, M, C):
    """sdp_ln_apply is element-wise.  sdp_ln_fwd (ln_fwd_sm for C <= 128, ln_fwd_v8 above) has no
    element form: it refuses rows or parameters off 16 B and statistics off 8 B, and
    sdpnet_train._ln_fwd_rows then runs sdp_rowstats + sdp_ln_apply."""
    L, dc = sp.lib(), sp.dcode(dtype)
    x, g, b, st, mean, rstd = ln_data(dtype, M, C)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    ref_ap = (x.double() - st[:, 0:1].double()) * st[:, 1:2].double() * g.double() + b.double()
    what = f"{DT_ID[dtype]} {M}x{C}"
    sweep("sdp_ln_apply", dict(X=Op(x), Y=Op(x, "out"), stats=Op(st.view(-1)), gamma=Op(g), beta=Op(b)),
          lambda v: L.sdp_ln_apply(dc, *ra(v["X"]), ptr(v["stats"]), ptr(v["gamma"]), ptr(v["beta"]), *ra(v["Y"]), M, C,
                                   stream()) == 0,
          lambda v: close(v["Y"], ref_ap, dtype, what="ln_apply"), what)

    def verify(v):
        close(v["Y"], ref, dtype, what="ln_fwd")
        close(v["stats"][:, 0], mean, F32, rel=1e-5, what="mean")
        close(v["stats"][:, 1], rstd, F32, rel=1e-4, what="rstd")
    sweep("sdp_ln_fwd", dict(X=Op(x), Y=Op(x, "out"), gamma=Op(g), beta=Op(b), stats=Op(st, "out", ld=2)),
          lambda v: L.sdp_ln_fwd(dc, *ra(v["X"]), 1e-5, ptr(v["gamma"]), ptr(v["beta"]), ptr(v["stats"]), *ra(v["Y"]), M,
                                 C, stream()) == 0, verify, what)


@pytest.mark.parametrize("M,C", [(5, 64), (77, 96), (9, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_ln_bwd(dtype, M, C):
    """ln_bwd_sm / ln_bwd_v8 read X, DY, ADD, gamma and write DX by 16 B; anything else runs
    ln_bwd_k (one element per lane).  Bounds of test_layernorm_fwd_bwd (4 x the forward's)."""
    L, dc = sp.lib(), sp.dcode(dtype)
    x, g, b, st, _, _ = ln_data(dtype, M, C)
    dy, add = rnd(M, C, dtype=dtype, seed=17), rnd(M, C, dtype=dtype, seed=18)
    xr, gr, br = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(xr, (C,), gr, br, 1e-5), (xr, gr, br), dy.double())
    nb = L.sdp_ln_bwd_blocks(M)
    tol = 8e-5 if dtype == F32 else 8e-2

    def verify(v):
        close(v["DX"], gx + add.double(), dtype, rel=tol, what="ln dx")
        part = v["part"].view(nb, 2, C).double().sum(0)
        close(part[0], gg, F32, rel=tol, what="ln dgamma")
        close(part[1], gb, F32, rel=tol, what="ln dbeta")
    ops = dict(X=Op(x), DY=Op(dy), ADD=Op(add), DX=Op(x, "out"), stats=Op(st.view(-1)), gamma=Op(g),
               part=Op(torch.empty(nb, 2 * C, device=DEV), "out", ld=2 * C))
    sweep("sdp_ln_bwd", ops,
          lambda v: L.sdp_ln_bwd(dc, *ra(v["X"]), ptr(v["stats"]), ptr(v["gamma"]), *ra(v["DY"]), *ra(v["ADD"]),
                                 *ra(v["DX"]), M, C, ptr(v["part"]), stream()) == 0, verify, f"{DT_ID[dtype]} {M}x{C}")


@pytest.mark.parametrize("xdt,ydt", [(BF, BF), (F32, F32), (BF, F32)], ids=["bf16", "fp32", "bf16-fp32"])
def test_add_ln_fwd_refuses_cleanly(xdt, ydt):
    """y = x * scale + r and a = LN(y) in one pass (C = 1032): one kernel, 16-B rows and parameters,
    8-B statistics; otherwise hipErrorNotSupported before a launch (sp.add_ln_fwd returns False and
    sdpnet_train runs the two passes)."""
    M, C = 9, 1032
    x, r = rnd(M, C, dtype=xdt, seed=41), rnd(M, C, dtype=ydt, seed=42, scale=2.0)
    g, b = rnd(C, seed=43, scale=0.2, shift=1.0), rnd(C, seed=44, scale=0.2)
    sc = rnd(M, seed=45).abs() + 0.5
    y64 = x.double() * sc.double()[:, None] + r.double()
    a64 = F.layer_norm(y64.to(ydt).double(), (C,), g.double(), b.double(), 1e-5)

    def call(v):
        return sp.add_ln_fwd(rows(v["X"]), rows(v["Y"]), rows(v["A"]), M, C, rows(v["R"]), 1e-5, v["gamma"], v["beta"],
                             v["stats"], scale=v["scale"], sgrp=1)

    def verify(v):
        close(v["Y"], y64, ydt, what="add_ln y")
        close(v["A"], a64, xdt, what="add_ln a")
        assert torch.isfinite(v["stats"]).all()
    ops = dict(X=Op(x), R=Op(r), Y=Op(r, "out"), A=Op(x, "out"), gamma=Op(g), beta=Op(b), scale=Op(sc),
               stats=Op(torch.empty(M, 2, device=DEV), "out", ld=2))
    sweep("sdp_add_ln_fwd", ops, call, verify, f"{DT_ID[xdt]}->{DT_ID[ydt]}")


# =========================================================================== softmax rows
@pytest.mark.parametrize("mode", ["plain", "dropout", "mask"])
@pytest.mark.parametrize("N", [53, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_softmax_fwd_bwd(dtype, N, mode):
    """softmax_fwd_r / softmax_bwd_r (register rows, 16-B accesses) against softmax_*_k (one element
    per lane).  rows 24 (mask: one (batch, head) block of N rows), bounds of test_softmax_fwd_bwd."""
    L, dc = sp.lib(), sp.dcode(dtype)
    R, Npad, scale = (N if mode == "mask" else 24), (N + 3) // 4 * 4, 1 / math.sqrt(96)
    p = 0.2 if mode == "dropout" else 0.0
    S = rnd(R, Npad, seed=19, scale=4.0)
    mask = rnd(N * N, seed=20) if mode == "mask" else None
    z = S[:, :N].double() * scale + (mask.double().view(N, N) if mask is not None else 0)
    Pref = torch.softmax(z, -1)
    P0, Pd0 = torch.empty(R, Npad, dtype=dtype, device=DEV), torch.empty(R, Npad, dtype=dtype, device=DEV)
    sp.softmax_fwd(S, P0, Pd0, R, N, Npad, scale, p, 77, mask=(mask, 0, 0, 1) if mask is not None else None)
    tol = 2e-6 if dtype == F32 else 1e-2

    def fwd(v):
        head = [dc, *pl(v["S"]), ptr(v["P"]), ptr(v["Pd"]), v["P"].stride(0), R, N, Npad, scale, p, 77]
        if mask is None:
            return L.sdp_softmax_fwd(*head, stream()) == 0
        return L.sdp_softmax_fwd_mask(*head, ptr(v["mask"]), 0, 0, 1, stream()) == 0

    def vfwd(v):
        close(v["P"][:, :N], Pref, dtype, rel=tol, what="softmax")
        assert bool((v["P"][:, N:] == 0).all()) and bool((v["Pd"][:, N:] == 0).all())
        assert torch.equal(v["Pd"] != 0, Pd0 != 0), "the dropout mask moved with the address"
        close(v["Pd"], Pd0.double(), dtype, rel=tol, what="dropped softmax")
    what = f"{DT_ID[dtype]} N {N} {mode}"
    sweep("sdp_softmax_fwd", dict(S=Op(S), P=Op(P0, "out", ld=Npad), Pd=Op(P0, "out", ld=Npad), mask=Op(mask)), fwd,
          vfwd, what)
    if mode == "mask":
        return
    dP = rnd(R, Npad, dtype=dtype, seed=21)
    dS0 = torch.empty(R, Npad, dtype=dtype, device=DEV)
    sp.softmax_bwd(P0, dP, dS0, R, N, Npad, p, 77)
    keep = (Pd0[:, :N] != 0).double() / (1 - p) if p else 1.0
    P64 = P0[:, :N].double()
    dpm = dP[:, :N].double() * keep
    ref = P64 * (dpm - (dpm * P64).sum(-1, keepdim=True))

    def vbwd(v):
        close(v["DS"][:, :N], ref, dtype, rel=1e-5 if dtype == F32 else 2e-2, what="softmax bwd")
        assert bool((v["DS"][:, N:] == 0).all())
    sweep("sdp_softmax_bwd", dict(P=Op(P0), DPd=Op(dP), DS=Op(P0, "out")),
          lambda v: L.sdp_softmax_bwd(dc, *pl(v["P"]), *pl(v["DPd"]), *pl(v["DS"]), R, N, Npad, p, 77, stream()) == 0,
          vbwd, what)


# =========================================================================== layout kernels
@pytest.mark.parametrize("C", [128, 130])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_layout_kernels(dtype, C):
    """sdp_nchw_to_rows, sdp_rows_to_nchw, sdp_group_mean, sdp_nchw_add_table, sdp_transpose,
    sdp_unpatchify: one element per lane in every form, so every placement gives the same values."""
    B, H, W, L, dc = 2, 7, 9, sp.lib(), sp.dcode(dtype)
    HW = H * W
    x = rnd(B, C, H, W, dtype=dtype, seed=51)
    xm = x.view(B * C, HW)
    rw = x.permute(0, 2, 3, 1).reshape(B * HW, C).contiguous()
    what = f"{DT_ID[dtype]} C={C}"
    sweep("sdp_nchw_to_rows", dict(X=Op(xm, ld=HW), Y=Op(rw, "out")),
          lambda v: L.sdp_nchw_to_rows(dc, ptr(v["X"]), dc, *ra(v["Y"]), B, C, HW, stream()) == 0, equal_to("Y", rw), what)
    sweep("sdp_rows_to_nchw", dict(X=Op(rw), Y=Op(xm, "out", ld=HW)),
          lambda v: L.sdp_rows_to_nchw(dc, *ra(v["X"]), dc, ptr(v["Y"]), B, C, HW, stream()) == 0, equal_to("Y", xm), what)
    mref = rw.double().view(B, HW, C).mean(1)
    sweep("sdp_group_mean", dict(X=Op(rw), out=Op(rw[:B], "out")),
          lambda v: L.sdp_group_mean(dc, *ra(v["X"]), dc, *pl(v["out"]), B, HW, C, stream()) == 0,
          lambda v: close(v["out"], mref, dtype, rel=1e-5 if dtype == F32 else 8e-3, what="group_mean"), what)
    table = rnd(HW, C, seed=58)
    tref = (x.double() + table.double().t().reshape(1, C, H, W)).to(dtype).view(B * C, HW)
    sweep("sdp_nchw_add_table", dict(X=Op(xm, "inout", ld=HW), table=Op(table.view(-1))),
          lambda v: L.sdp_nchw_add_table(dc, ptr(v["X"]), ptr(v["table"]), B, C, HW, stream()) == 0,
          lambda v: close(v["X"], tref, dtype, rel=1e-6 if dtype == F32 else 8e-3, what="nchw_add_table"), what)
    tr = rw.t().contiguous()
    sweep("sdp_transpose", dict(X=Op(rw), Y=Op(tr, "out")),
          lambda v: L.sdp_transpose(dc, *pl(v["X"]), *pl(v["Y"]), B * HW, C, stream()) == 0, equal_to("Y", tr), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_unpatchify(dtype):
    p, img, Bn, L, dc = 8, 64, 2, sp.lib(), sp.dcode(dtype)
    kpad, n = 3 * p * p, (img // p) ** 2 * Bn
    rws = rnd(n, kpad, dtype=dtype, seed=52)
    ref = F.fold(rws.double().view(Bn, -1, kpad).transpose(1, 2), img, p, stride=p).to(dtype).view(Bn * 3 * img, img)
    sweep("sdp_unpatchify", dict(rows=Op(rws, ld=kpad), img=Op(ref, "out", ld=img)),
          lambda v: L.sdp_unpatchify(dc, ptr(v["rows"]), dc, ptr(v["img"]), Bn, img, img, p, kpad, stream()) == 0,
          equal_to("img", ref), DT_ID[dtype])


# =========================================================================== training GEMMs
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_gemm_flex(dtype, ta, tb):
    """gemm_flex_bf16 loads 8 elements where an operand's base and leading dimension allow (per
    operand), single elements otherwise; C is stored one element at a time; fp32 is all scalar."""
    M, N, K, L, dc = 128, 128, 32, sp.lib(), sp.dcode(dtype)
    A, B = rnd(*((K, M) if ta else (M, K)), dtype=dtype, seed=1), rnd(*((N, K) if tb else (K, N)), dtype=dtype, seed=2)
    ref = 0.5 * (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    sweep("sdp_gemm_flex", dict(A=Op(A), B=Op(B), C=Op(torch.empty(M, N, device=DEV), "out")),
          lambda v: L.sdp_gemm_flex(dc, 0, ta, tb, *pl(v["A"]), 0, 0, *pl(v["B"]), 0, 0, *pl(v["C"]), 0, 0, M, N, K, 1, 1,
                                    1, 0, 0.5, 0, stream()) == 0,
          lambda v: close(v["C"], ref, F32, rel=1e-5 if dtype == F32 else 2e-2, what="gemm_flex"),
          f"{DT_ID[dtype]} ta={ta} tb={tb}")


@pytest.mark.parametrize("mode", [1, 2])
def test_gemm_train_epi_refuses_cleanly(mode):
    """sdp_gemm_train_epi (bf16, the 256 x 256 kernel only): hipErrorNotSupported before a launch for
    any operand off 16 B or leading dimension off 8; the caller runs the GEMM and the activation
    kernel.  An accepted call equals the aligned one bit for bit."""
    M, N, K, L = 300, 256, 128, sp.lib()
    x, w, b = rnd(M, K, dtype=BF, seed=1), rnd(N, K, dtype=BF, seed=2, scale=0.05), rnd(N, seed=3, scale=0.1)
    zin = rnd(M, N, dtype=BF, seed=4, scale=1.5)
    y0, h0 = torch.empty(M, N, dtype=BF, device=DEV), torch.empty(M, N, dtype=BF, device=DEV)
    if mode == 1:
        assert sp.gemm_train_epi(1, x, w, y0, M, N, K, bias=b, y2=h0, act=1, p=0.2, seed=77)
        ops = dict(X=Op(x), W=Op(w), bias=Op(b), Y=Op(y0, "out"), Y2=Op(y0, "out"))
        z64 = x.double() @ w.double().t() + b.double()
        close(y0, z64, BF, what="train_epi mode 1")
    else:
        assert sp.gemm_train_epi(2, x, w, y0, M, N, K, z=zin, act=1, p=0.2, seed=78)
        ops = dict(X=Op(x), W=Op(w), Z=Op(zin), Y=Op(y0, "out"))

    def call(v):
        z, y2 = v.get("Z"), v.get("Y2")
        rc = L.sdp_gemm_train_epi(mode, *pl(v["X"]), *pl(v["W"]), ptr(v.get("bias")), ptr(z), z.stride(0) if z is not None
                                  else 0, *pl(v["Y"]), ptr(y2), y2.stride(0) if y2 is not None else 0, M, N, K, 1, 0.2,
                                  77 if mode == 1 else 78, stream())
        return rc == 0

    def verify(v):
        assert torch.equal(v["Y"], y0) and (mode == 2 or torch.equal(v["Y2"], h0))
    sweep("sdp_gemm_train_epi", ops, call, verify, f"mode {mode}")


def test_gemm_splitk_refuses_cleanly():
    """sdp_gemm_splitk: hipErrorInvalidValue before a launch for X, W off 16-B rows, Y, R off 8-B
    rows, bias or workspace off 16 B (sdpnet_hip.h); sdpnet_hip.gemm asks _splitk_aligned first and
    keeps the ordinary path.  An accepted call meets the GEMM bound."""
    M, N, K, bm, splits, L = 64, 128, 256, 64, 2, sp.lib()
    x, w, b = rnd(M, K, dtype=BF, seed=1), rnd(N, K, dtype=BF, seed=2, scale=0.05), rnd(N, seed=5)
    r = rnd(M, N, dtype=BF, seed=6)
    ref = x.double() @ w.double().t() + b.double() + r.double()
    need = sp.gemm_splitk_ws_bytes(M, N, bm, splits)
    ws = torch.full((need // 4,), 3.0, device=DEV)   # not the slabs' values: the reduce must read what was stored
    ops = dict(X=Op(x), W=Op(w), bias=Op(b), R=Op(r), Y=Op(r, "out"), ws=Op(ws, "inout"))

    def call(v):
        return L.sdp_gemm_splitk(1, *ra(v["X"]), *pl(v["W"]), ptr(v["bias"]), *ra(v["R"]), *ra(v["Y"]), M, N, K, 0, 0,
                                 None, None, None, bm, splits, ptr(v["ws"]), need, stream()) == 0
    sweep("sdp_gemm_splitk", ops, call, lambda v: close(v["Y"], ref, BF, what="gemm_splitk"), f"{M}x{N}x{K}")


# =========================================================================== flash training attention
@pytest.mark.parametrize("B,N,H,hd", [(2, 53, 4, 16), (1, 64, 2, 96)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attn_train_refuses_cleanly(B, N, H, hd, p):
    """sdp_attn_train_fwd / _bwd: bf16x8 loads of qkv / o / dO rows, 8-B stores of o, dq, dk, dv; no
    other kernel, so a misaligned operand is hipErrorInvalidValue before a launch (sdpnet_train
    allocates all of them itself).  An accepted call equals the aligned one bit for bit; the aligned
    one meets the bounds of test_flash_train_attention_vs_torch."""
    assert sp.attn_train_applies(BF, N, hd)
    C, T, L, scale, seed = H * hd, B * N, sp.lib(), 1.0 / math.sqrt(hd), 1234567 + N
    qkv, do = rnd(T, 3 * C, dtype=BF, seed=1, scale=1.5), rnd(T, C, dtype=BF, seed=2)
    o0, lse0 = torch.empty(T, C, dtype=BF, device=DEV), torch.empty(B * H * N, device=DEV)
    sp.attn_train_fwd(qkv, o0, lse0, B, N, H, hd, scale, p, seed)
    g0 = [torch.empty(T, C, dtype=BF, device=DEV) for _ in range(3)]
    delta0 = torch.empty(B * H * N, device=DEV)
    sp.attn_train_bwd(qkv, o0, do, lse0, delta0, (g0[0], 0), (g0[1], 0), (g0[2], 0), B, N, H, hd, scale, p, seed)
    q, k, v_ = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    keep = sp.attn_dropout_mask(B * H, N, p, seed, DEV).view(B, H, N, N).double() / (1 - p)
    oref = ((torch.softmax(q @ k.transpose(-1, -2) * scale, -1) * keep) @ v_).permute(0, 2, 1, 3).reshape(T, C)
    close(o0, oref, BF, rel=1e-2, what="train attention O")
    what = f"{(B, N, H, hd)} p {p}"

    def vf(v):
        assert torch.equal(v["o"], o0) and torch.equal(v["lse"], lse0)
    # lse / delta start as 7.0, not as the expected values: a dropped store shows
    sweep("sdp_attn_train_fwd", dict(qkv=Op(qkv), o=Op(o0, "out"), lse=Op(torch.full_like(lse0, 7.0), "inout")),
          lambda v: L.sdp_attn_train_fwd(1, *pl(v["qkv"]), *pl(v["o"]), ptr(v["lse"]), B, N, H, hd, scale, p, seed,
                                         stream()) == 0, vf, what)

    def vb(v):
        assert all(torch.equal(v[n], g) for n, g in zip(("dq", "dk", "dv"), g0)) and torch.equal(v["delta"], delta0)
    ops = dict(qkv=Op(qkv), o=Op(o0), dO=Op(do), lse=Op(lse0), delta=Op(torch.full_like(delta0, 7.0), "inout"),
               dq=Op(o0, "out"),
               dk=Op(o0, "out"), dv=Op(o0, "out"))
    sweep("sdp_attn_train_bwd", ops,
          lambda v: L.sdp_attn_train_bwd(1, *pl(v["qkv"]), *pl(v["o"]), *pl(v["dO"]), ptr(v["lse"]), ptr(v["delta"]),
                                         *pl(v["dq"]), *pl(v["dk"]), *pl(v["dv"]), B, N, H, hd, scale, p, seed,
                                         stream()) == 0, vb, what)


# =========================================================================== losses, metrics, dW
@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_losses_and_metrics(dtype, K):
    """sdp_ce_loss(_counted) / _soft, sdp_bce_loss / _soft, sdp_distill_loss and sdp_logits_metrics read
    logits, targets and teacher one element at a time and write dlogits the same way (B 6): under every
    shift and stride dlogits equal the aligned run's bit for bit and the loss agrees to 1e-5 (its sum
    over rows is accumulated atomically)."""
    Bn = 6
    lg = rnd(Bn, K, dtype=dtype, seed=61, scale=2.0)
    tg = torch.softmax(rnd(Bn, K, seed=62), -1).contiguous()
    te = rnd(Bn, K, dtype=dtype, seed=63, scale=2.0)
    lab = (torch.arange(Bn, device=DEV) * 3) % K
    forms = {
        "sdp_ce_loss": lambda v, loss: sp.ce_loss(v["logits"], lab, 0.1, 1.0, v["dlogits"], loss),
        "sdp_ce_loss_soft": lambda v, loss: sp.ce_loss_soft(v["logits"], v["targets"], 0.1, 1.0, v["dlogits"], loss),
        "sdp_bce_loss": lambda v, loss: sp.bce_loss(v["logits"], lab, 0.1, 1.0, v["dlogits"], loss),
        "sdp_bce_loss_soft": lambda v, loss: sp.bce_loss_soft(v["logits"], v["targets"], 0.1, 1.0, v["dlogits"], loss),
        "sdp_distill_loss": lambda v, loss: sp.distill_loss(v["logits"], v["teacher"], v["targets"], 0.1, 0.5, 2.0, 0, 1.0,
                                                            v["dlogits"], loss),
    }
    for entry, fn in forms.items():
        soft, kd = entry.endswith("soft") or entry == "sdp_distill_loss", entry == "sdp_distill_loss"
        d0, l0 = torch.empty(Bn, K, dtype=dtype, device=DEV), torch.zeros(1, device=DEV)
        fn(dict(logits=lg, targets=tg, teacher=te, dlogits=d0), l0)
        assert bool(torch.isfinite(d0.float()).all()) and bool(torch.isfinite(l0).all())
        got = {}

        def call(v, fn=fn, got=got):
            got["loss"] = torch.zeros(1, device=DEV)
            fn(v, got["loss"])

        def verify(v, d0=d0, l0=l0, got=got):
            assert torch.equal(v["dlogits"], d0), "dlogits differ from the aligned run"
            close(got["loss"], l0, F32, rel=1e-5, what="loss")
        sweep(entry, dict(logits=Op(lg), targets=Op(tg if soft else None), teacher=Op(te if kd else None),
                          dlogits=Op(d0, "out")), call, verify, f"{DT_ID[dtype]} K={K}")
    m0 = sp.logits_metrics(lg, lab, 0.1)
    got = {}

    def metrics(v):
        got["m"] = sp.logits_metrics(v["logits"], lab, 0.1)
    sweep("sdp_logits_metrics", dict(logits=Op(lg)), metrics, lambda v: close(got["m"], m0, F32, rel=1e-6, what="metrics"),
          f"{DT_ID[dtype]} K={K}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_dw_wgrad(dtype):
    """dw_wgrad_k chooses 16-B staging loads inside the kernel (bf16, A and DY % 16, lda, lddy % 8),
    element loads otherwise; the partial slabs are written one float at a time."""
    B, H, W, C, k, L, dc = 2, 7, 9, 96, 5, sp.lib(), sp.dcode(dtype)
    M = B * H * W
    a, dy = rnd(M, C, dtype=dtype, seed=71), rnd(M, C, dtype=dtype, seed=72)
    nch = L.sdp_dw_wgrad_chunks(B)
    ref = sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    xr = a.double().view(B, H, W, C).permute(0, 3, 1, 2)
    w = torch.zeros(C, 1, k, k, dtype=torch.float64, device=DEV, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(xr, w, padding="same", groups=C), w, dy.double().view(B, H, W, C).permute(0, 3, 1, 2))
    close(ref, gw.view(C, k * k), F32, rel=1e-5 if dtype == F32 else 2e-2, what="dw_wgrad")

    def verify(v):
        close(v["part"].double().sum(0).view(C, k * k), gw.view(C, k * k), F32, rel=1e-5 if dtype == F32 else 2e-2,
              what="dw_wgrad")
    sweep("sdp_dw_wgrad", dict(A=Op(a), DY=Op(dy), part=Op(torch.empty(nch, C * k * k, device=DEV), "out", ld=C * k * k)),
          lambda v: L.sdp_dw_wgrad(dc, *ra(v["A"]), *ra(v["DY"]), B, H, W, C, k, ptr(v["part"]), stream()) == 0, verify,
          DT_ID[dtype])


# =========================================================================== weight gradient, casts
def test_gemm_wgrad_refuses_cleanly():
    """sdp_gemm_wgrad (bf16, one 8-phase kernel): hipErrorNotSupported before a launch for dY / X off
    16-B rows or a slab buffer off 16 B / ldc % 4 (sdpnet_train._wgrad then takes sdp_gemm_flex);
    hipErrorInvalidValue for a slab stride that is no multiple of 4 floats (f32x4 slab stores)."""
    N, K, M, L = 256, 256, 64, sp.lib()
    dy, x = rnd(M, N, dtype=BF, seed=31, scale=0.5), rnd(M, K, dtype=BF, seed=32)
    ref = dy.double().t() @ x.double()
    sweep("sdp_gemm_wgrad", dict(A=Op(dy), B=Op(x), C=Op(torch.empty(N, K, device=DEV), "out")),
          lambda v: L.sdp_gemm_wgrad(*pl(v["A"]), *pl(v["B"]), *pl(v["C"]), N * v["C"].stride(0), N, K, M, 1, None,
                                     stream()) == 0,
          lambda v: close(v["C"], ref, F32, rel=1e-5, what="wgrad"), f"{N}x{K}x{M}")
    # two splits (M = 128, one K-tile each): the second slab starts split_stride floats after the first
    M2 = 128
    dy2, x2 = rnd(M2, N, dtype=BF, seed=33, scale=0.5), rnd(M2, K, dtype=BF, seed=34)
    for extra, ok in ((0, True), (4, True), (1, False), (2, False)):
        slabs = al.blank(1, 2 * N * K + 8, F32, DEV)[0]
        rc = L.sdp_gemm_wgrad(*pl(dy2), *pl(x2), slabs.data_ptr(), K, N * K + extra, N, K, M2, 1, None, stream())
        torch.cuda.synchronize()
        assert (rc == 0) == ok, f"split_stride N K + {extra}: rc {rc}"
        if not ok:
            assert al.untouched(slabs), "slabs written although the call was refused"
            continue
        for s_ in range(2):
            got = slabs[s_ * (N * K + extra): s_ * (N * K + extra) + N * K].view(N, K)
            close(got, dy2[64 * s_: 64 * s_ + 64].double().t() @ x2[64 * s_: 64 * s_ + 64].double(), F32, rel=1e-5,
                  what=f"wgrad slab {s_}")
        rest = torch.cat([slabs[N * K: N * K + extra], slabs[2 * N * K + extra:]])
        assert bool(torch.isnan(rest).all()), "floats between / after the slabs written"


@pytest.mark.parametrize("first", [4, 8, 12])
def test_mt_cast_transpose_flat_sources(first):
    """mt_cast_transpose_k takes float4 loads only for a 16-B aligned source and 8-B / 16-B stores
    only where the destination address allows: fp32 master weights that are views of one flat buffer
    at 4 / 8 / 12 B (mod 16), into destinations at 0 / 2 / 4 / 8 B, give the aligned run's bits."""
    from test_gpu_alignment import flat_views, pads_untouched
    shapes = [(64, 64), (100, 72), (3, 132), (256, 256), (70, 130)]
    views, ibuf, pad = flat_views([r * c for r, c in shapes], 40, first)
    srcs = [v.view(r, c) for v, (r, c) in zip(views, shapes)]
    assert all(t.data_ptr() % 16 for t in srcs) and all(t.is_contiguous() for t in srcs)
    aligned = [t.clone() for t in srcs]
    a_out = [(torch.zeros(r, c, dtype=BF, device=DEV), torch.zeros(c, r, dtype=BF, device=DEV)) for r, c in shapes]
    sp.mt_cast_transpose([(x, d, t) for x, (d, t) in zip(aligned, a_out)])
    for x, (d, t) in zip(aligned, a_out):
        assert torch.equal(d, x.to(BF)) and torch.equal(t, x.to(BF).t())
    for shift in (0, 2, 4, 8):
        outs = [(al.blank(r, c, BF, DEV, shift, c + 8), al.blank(c, r, BF, DEV, shift, r + 8)) for r, c in shapes]
        sp.mt_cast_transpose([(x, d, t) for x, (d, t) in zip(srcs, outs)])
        torch.cuda.synchronize()
        for (d, t), (d0, t0) in zip(outs, a_out):
            assert torch.equal(d, d0) and torch.equal(t, t0), f"destination shift {shift}: differs from the aligned run"
            assert not al.findings(d) and not al.findings(t), (shift, al.findings(d), al.findings(t))
    assert pads_untouched(ibuf, pad) and all(torch.equal(a, b) for a, b in zip(srcs, aligned))


@pytest.mark.parametrize("first", [4, 8, 12])
def test_grad_sumsq_on_flat_views(first):
    """The atomic sdp_grad_sumsq reads one float per lane: gradients that are views of a flat buffer
    give sum g^2 within fp32 summation error of fp64 (each partial chain is at most 16 fused adds, a
    256-lane tree and 5 atomic adds of positive terms: below 64 x 2^-24 = 4e-6 relative; bound 1e-5),
    the non-finite flag stays clear, and no pad float is written."""
    from test_gpu_alignment import SIZES, flat_views, pads_untouched
    gv, gbuf, gpad = flat_views(SIZES, 600, first)
    blocks, nb = sp.mt_block_table(SIZES, torch.device(DEV))
    sizes = torch.tensor(SIZES, dtype=torch.int64, device=DEV)
    ptrs = torch.tensor([t.data_ptr() for t in gv], dtype=torch.int64, device=DEV)
    state = torch.zeros(2, device=DEV)
    assert sp.lib().sdp_grad_sumsq(ptrs.data_ptr(), sizes.data_ptr(), blocks.data_ptr(), nb, state.data_ptr(),
                                   stream()) == 0
    torch.cuda.synchronize()
    ref = sum(float((t.double() ** 2).sum()) for t in gv)
    assert abs(float(state[0]) - ref) <= 1e-5 * ref, (float(state[0]), ref)
    assert int(state.view(torch.int32)[1]) == 0 and pads_untouched(gbuf, gpad)


# =========================================================================== mixed / fused LayerNorm forms
@pytest.mark.parametrize("M,C", [(5, 64), (77, 96), (9, 2048)])
def test_ln_mixed_forms(M, C):
    """sdp_ln_fwd_mixed (fp32 rows -> bf16) and sdp_ln_bwd_mixed (fp32 X / ADD / DX, bf16 DY) exist on
    the 8-wide kernels only: a misaligned row or gamma is hipErrorInvalidValue before a launch
    (sdpnet_train._ln_fwd_rows and its own activation buffers keep them aligned)."""
    L = sp.lib()
    x, g, b, st, mean, rstd = ln_data(F32, M, C)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)

    def vf(v):
        close(v["Y"], ref, BF, what="ln_fwd_mixed")
        close(v["stats"][:, 0], mean, F32, rel=1e-5, what="mean")
        close(v["stats"][:, 1], rstd, F32, rel=1e-4, what="rstd")
    sweep("sdp_ln_fwd_mixed", dict(X=Op(x), Y=Op(x.to(BF), "out"), gamma=Op(g), beta=Op(b), stats=Op(st, "out", ld=2)),
          lambda v: L.sdp_ln_fwd_mixed(0, 1, *ra(v["X"]), 1e-5, ptr(v["gamma"]), ptr(v["beta"]), ptr(v["stats"]),
                                       *ra(v["Y"]), M, C, stream()) == 0, vf, f"{M}x{C}")
    dy, add = rnd(M, C, dtype=BF, seed=17), rnd(M, C, seed=18)
    xr, gr, br = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(xr, (C,), gr, br, 1e-5), (xr, gr, br), dy.double())
    nb = L.sdp_ln_bwd_blocks(M)

    def vb(v):   # bounds of test_layernorm_fwd_bwd for a bf16 gradient
        close(v["DX"], gx + add.double(), BF, rel=8e-2, what="ln dx")
        part = v["part"].view(nb, 2, C).double().sum(0)
        close(part[0], gg, F32, rel=8e-2, what="ln dgamma")
        close(part[1], gb, F32, rel=8e-2, what="ln dbeta")
    ops = dict(X=Op(x), DY=Op(dy), ADD=Op(add), DX=Op(x, "out"), stats=Op(st.view(-1)), gamma=Op(g),
               part=Op(torch.empty(nb, 2 * C, device=DEV), "out", ld=2 * C))
    sweep("sdp_ln_bwd_mixed", ops,
          lambda v: L.sdp_ln_bwd_mixed(0, 1, *ra(v["X"]), ptr(v["stats"]), ptr(v["gamma"]), *ra(v["DY"]), *ra(v["ADD"]),
                                       *ra(v["DX"]), M, C, ptr(v["part"]), stream()) == 0, vb, f"{M}x{C}")


@pytest.mark.parametrize("xdt", [F32, BF], ids=["fp32-stream", "bf16"])
@pytest.mark.parametrize("M,C", [(77, 256), (9, 2048)])
def test_ln_bwd_fused_refuses_cleanly(xdt, M, C):
    """sdp_ln_bwd_fused with the branch-gradient output O2 = bf16(bf16(DX scale) gelu'(Z)): ln_bwd_v8
    only, so anything off a 16-B row (X, DY, ADD, DX, Z, O2) or gamma off 16 B is
    hipErrorNotSupported and sdpnet_hip.ln_bwd runs the separate passes.  An accepted call gives the
    aligned run's DX and O2 bit for bit; the aligned DX meets test_layernorm_fwd_bwd's bound."""
    L = sp.lib()
    x, g, b, st, _, _ = ln_data(xdt, M, C)
    dy, add = rnd(M, C, dtype=BF, seed=17), rnd(M, C, dtype=xdt, seed=18)
    z, sc = rnd(M, C, dtype=BF, seed=19, scale=1.5), rnd(M, seed=20).abs() + 0.5
    dx0, o20 = torch.empty_like(x), torch.empty(M, C, dtype=BF, device=DEV)
    sp.ln_bwd(sp.dense(x), st, g, sp.dense(dy), sp.dense(dx0), M, C, add=sp.dense(add),
              emit=dict(out=o20, scale=sc, sgrp=1, z=z, act=1))
    xr = x.double().requires_grad_(True)
    (gx,) = torch.autograd.grad(F.layer_norm(xr, (C,), g.double(), b.double(), 1e-5), xr, dy.double())
    close(dx0, gx + add.double(), xdt, rel=8e-5 if xdt == F32 else 8e-2, what="fused ln dx")
    nb = L.sdp_ln_bwd_blocks(M)

    def call(v):
        return L.sdp_ln_bwd_fused(sp.dcode(xdt), 1, *ra(v["X"]), ptr(v["stats"]), ptr(v["gamma"]), *ra(v["DY"]),
                                  *ra(v["ADD"]), *ra(v["DX"]), M, C, ptr(v["part"]), None, None, None, ptr(v["scale"]), 1,
                                  *pl(v["Z"]), 1, 0.0, 0, 0, *pl(v["O2"]), None, None, 0, 0, 0, stream()) == 0

    def verify(v):
        assert torch.equal(v["DX"], dx0) and torch.equal(v["O2"], o20), "DX / O2 differ from the aligned run"
        assert torch.isfinite(v["part"]).all()
    ops = dict(X=Op(x), DY=Op(dy), ADD=Op(add), DX=Op(x, "out"), Z=Op(z), O2=Op(o20, "out"), stats=Op(st.view(-1)),
               gamma=Op(g), scale=Op(sc), part=Op(torch.empty(nb, 2 * C, device=DEV), "out", ld=2 * C))
    sweep("sdp_ln_bwd_fused", ops, call, verify, f"{DT_ID[xdt]} {M}x{C}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_training_layernorm_falls_back_on_a_misaligned_parameter(dtype):
    """sdpnet_train._ln_fwd with gamma / beta / rows off a 16-B boundary: sdp_ln_fwd would refuse, so
    the two passes run (sdp_rowstats + sdp_ln_apply) and give the same LayerNorm and statistics."""
    import sdpnet_train as st_
    M, C = 77, 96
    x, g, b, _, mean, rstd = ln_data(dtype, M, C)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    for gs, bs, xs in ((al.place(g, al.BASE[0]), b, x), (g, al.place(b, al.BASE[2]), x),
                       (g, b, al.place(x, al.BASE[0], ld=C)), (g, b, x)):
        a, stt = st_._ln_fwd(sp.Rows(xs, C), M, C, gs, bs, 1e-5, dtype)
        torch.cuda.synchronize()
        close(a, ref, dtype, what="_ln_fwd")
        close(stt[:, 0], mean, F32, rel=1e-5, what="mean")
        close(stt[:, 1], rstd, F32, rel=1e-4, what="rstd")


# =========================================================================== MX pair
def _bytes(n, shift, fill=0xAB):
    """n bytes at ``shift`` (mod 16) inside a 0xAB-filled buffer with 64 guard bytes on both sides."""
    buf = torch.full((64 + 16 + n + 64,), fill, dtype=torch.uint8, device=DEV)
    off = 64 + (shift - buf.data_ptr() - 64) % 16
    return buf, buf[off:off + n]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_mx_quant_rows_refuses_cleanly(dtype):
    """sdp_mx_quant_rows reads 16-B input vectors and float2 statistics and writes 8-B byte groups and
    4-B scale words: X off 16 B (or ldx off 16 B), stats off 8 B, Q off 16 B or S off 4 B is
    hipErrorInvalidValue before a launch; an accepted call stays bit-exact against tests/mx_oracle.py."""
    import mx_oracle as mo
    M, K, L, dc = 5, 128, sp.lib(), sp.dcode(dtype)
    x = rnd(M, K, dtype=dtype, seed=81, scale=3.0)
    stats = torch.stack([rnd(M, seed=82, scale=0.1), rnd(M, seed=83).abs() + 0.5], 1).contiguous()
    want_q, want_s = mo.encode(((x.float() - stats[:, 0:1]) * stats[:, 1:2]).cpu())
    got = {}

    def call(v, qshift=0, sshift=0):
        got["qb"], q = _bytes(M * K, qshift)
        got["sb"], s_ = _bytes(M * (K // 32), sshift)
        rc = L.sdp_mx_quant_rows(dc, *ra(v["X"]), ptr(v["stats"]), q.data_ptr(), K, s_.data_ptr(), K // 32, M, K, stream())
        torch.cuda.synchronize()
        got["q"], got["s"] = q.view(M, K), s_.view(M, K // 32)
        if rc != 0:
            assert bool((got["qb"] == 0xAB).all()) and bool((got["sb"] == 0xAB).all()), "written although refused"
        return rc == 0

    def verify(v):
        assert torch.equal(got["q"].cpu(), want_q) and torch.equal(got["s"].cpu(), want_s), "not bit-exact"
        for buf, view in ((got["qb"], got["q"]), (got["sb"], got["s"])):
            lo = view.data_ptr() - buf.data_ptr()
            assert bool((buf[:lo] == 0xAB).all()) and bool((buf[lo + view.numel():] == 0xAB).all()), "guard bytes"
    entry = "sdp_mx_quant_rows" if dtype == BF else "sdp_mx_quant_rows[fp32]"
    sweep(entry, dict(X=Op(x), stats=Op(stats.view(-1))), call, verify, DT_ID[dtype])
    aligned = dict(X=x, stats=stats.view(-1))
    for qs, ss in ((4, 0), (8, 0), (0, 1), (0, 2)):
        assert call(aligned, qs, ss) is False, f"Q + {qs} B / S + {ss} B was not refused"
    assert call(aligned) is True
    verify(aligned)


def test_gemm_mx_refuses_cleanly():
    """sdp_gemm_mx: 16-B rows of the e4m3 operands, 4-B scale rows, 8-B rows of Y and R, a 16-B bias,
    8-B partials, else hipErrorInvalidValue before a launch (layers._mx_weights copies a parameter
    that is not 16-B aligned).  An accepted call gives the aligned run's rows bit for bit."""
    M, N, K, L = 37, 64, 128, sp.lib()
    xq = sp.mx_quant_rows(sp.dense(rnd(M, K, dtype=BF, seed=91)), M, K)
    wq = sp.mx_quant_rows(sp.dense(rnd(N, K, seed=92, scale=0.05)), N, K)
    b, r = rnd(N, seed=93), rnd(M, N, dtype=BF, seed=94)
    y0, p0 = torch.empty(M, N, dtype=BF, device=DEV), torch.empty(M, 2, device=DEV)
    sp.gemm_mx(xq, wq, M, N, K, y=sp.dense(y0), bias=b, resid=sp.dense(r), part=p0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y0.float()).all())

    def call(v, ops=None):
        o = ops or dict(xq=xq.q, xs=xq.s, wq=wq.q, ws=wq.s)
        return L.sdp_gemm_mx(*pl(o["xq"]), *pl(o["xs"]), *pl(o["wq"]), *pl(o["ws"]), ptr(v["bias"]), *ra(v["R"]),
                             *ra(v["Y"]), None, 0, None, 0, M, N, K, 0, 0, ptr(v["part"]), stream()) == 0

    def verify(v):
        assert torch.equal(v["Y"], y0) and torch.equal(v["part"], p0), "differs from the aligned run"
    ops = dict(bias=Op(b), R=Op(r), Y=Op(r, "out"), part=Op(p0, "out", ld=2))
    sweep("sdp_gemm_mx", ops, call, verify, f"{M}x{N}x{K}")
    # the byte operands: e4m3 rows 4 / 8 B and scale rows 1 / 2 B off their boundary
    for name, shifts in (("xq", (4, 8)), ("wq", (4, 8)), ("xs", (1, 2)), ("ws", (1, 2))):
        src = dict(xq=xq.q, xs=xq.s, wq=wq.q, ws=wq.s)
        for sh in shifts:
            t = src[name]
            _, flat = _bytes(t.numel(), sh)
            flat.copy_(t.reshape(-1))
            moved = dict(src, **{name: flat.view(t.shape)})
            y = al.blank(M, N, BF, DEV)
            part = al.blank(M, 2, F32, DEV)
            assert call(dict(bias=b, R=r, Y=y, part=part), moved) is False, f"{name} + {sh} B was not refused"
            torch.cuda.synchronize()
            assert al.untouched(y) and al.untouched(part), f"{name} + {sh} B: written although refused"
