"""GPU: every covered entry point on operands whose base address or row stride is off the
alignment its vector tier needs (tests/alignment.py), one operand at a time and all at once.

The shapes are ones the vector tier takes (asserted where the library can be asked), so only the
address sends a call elsewhere.  A call must return 0 with the result within the bound of the entry
point's existing aligned test (``close`` of test_gpu_kernels.py against an fp64 reference of the
same rounded inputs) and nothing but its logical output written, or be refused with no output byte
written; ``alignment.TABLE`` says which, per operand.  The aligned baseline runs first in every
test.  Every operand lies in its own guard-banded allocation, so no access leaves mapped memory."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import alignment as al
import sdpnet_hip as sp
from test_gpu_kernels import ACTS
from test_gpu_kernels import close as _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
DT_ID = {F32: "fp32", BF: "bf16"}


@pytest.fixture(autouse=True)
def _full_precision_references():
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield
    torch.set_float32_matmul_precision(old)


def rnd(*shape, dtype=F32, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).to(dtype).to(DEV)


_WORST = [0.0]


def close(got, ref, dtype, rel=None, what=""):
    """test_gpu_kernels.close, unchanged; the error as a share of its bound is kept for the report
    line of sweep() (profiles/alignment.md)."""
    tol = rel if rel is not None else (2e-5 if dtype == torch.float32 else 1.2e-2)
    err = (got.float() - ref.float()).abs().max().item()
    _WORST[0] = max(_WORST[0], err / (tol * (ref.float().abs().max().item() + 1e-6) + 1e-6))
    _close(got, ref, dtype, rel, what)


def rows(v: torch.Tensor) -> sp.Rows:
    return sp.Rows(v, v.stride(0))


# --------------------------------------------------------------------------- the driver
class Op:
    """One operand of a call: ``dense`` (its logical contents, or the shape donor of an output),
    ``role`` in / out / inout, ``ld`` the aligned row stride (matrices; default C + 8)."""

    def __init__(self, dense, role="in", ld=None):
        self.dense, self.role = dense, role
        self.ld = None if dense is None or dense.dim() == 1 else (ld if ld is not None else dense.shape[-1] + 8)


def case_ids(entry: str, ops):
    """The perturbations the table lists for the operands of this call (None: the aligned run)."""
    dtypes = {n: o.dense.dtype for n, o in ops.items() if o.dense is not None}
    return [(None, None)] + al.TABLE[entry].cases(dtypes)


def ident(pc):
    op, case = pc
    return "aligned" if op is None else "all+elem" if op == al.ALL else f"{op}:{case.id}"


def run(entry: str, ops, pc, call, verify, what=""):
    """Place every operand (the one named by ``pc`` perturbed, or all of them), make the call,
    hold it to the contract.  ``call(v)`` gets name -> view and returns False for a refusal it
    reports by value; an exception of the wrapper's error check is a refusal too."""
    op, case = pc
    E = al.TABLE[entry]
    v, expect = {}, al.RAN
    for name, o in ops.items():
        if o.dense is None:
            v[name] = None
            continue
        c = case if name == op else al.Case(shift="elem") if op == al.ALL else None
        if c is not None and c.delta and o.ld is None:
            c = None
        if c is not None and E.expect(name, c, o.dense.dtype) == al.REFUSED:
            expect = al.REFUSED
        v[name] = al.place(o.dense, c, o.ld, out=o.role == "out")
    before = {n: v[n].clone() for n, o in ops.items() if o.role == "inout"}
    try:
        refused = call(v) is False
    except RuntimeError as e:     # sdpnet_hip._check: the entry point returned non-zero
        assert "hip error code" in str(e), e
        refused = True
    torch.cuda.synchronize()
    label = f"{entry} {what} [{ident(pc)}]"
    return al.judge(label, refused,
                    {n: (v[n], o.dense) for n, o in ops.items() if o.role == "in" and o.dense is not None},
                    {n: v[n] for n, o in ops.items() if o.role == "out" and o.dense is not None}, lambda: verify(v),
                    expect,
                    {n: (v[n], before[n]) for n in before})


def sweep(entry, ops, call, verify, what=""):
    """The aligned baseline, then every perturbation of the table; one assertion message for all."""
    fails, seen = [], {}
    _WORST[0] = 0.0
    for pc in case_ids(entry, ops):
        try:
            seen[ident(pc)] = run(entry, ops, pc, call, verify, what)
        except AssertionError as e:
            if pc[0] is None:
                raise
            fails.append(str(e))
    assert seen.get("aligned") == al.RAN
    refused = sorted(k for k, o in seen.items() if o == al.REFUSED)
    print(f"ALIGN {entry} | {what} | {len(seen) - len(refused)} ran, {len(refused)} refused {refused} | "
          f"{len(fails)} failed | worst error {_WORST[0]:.3f} of the bound")
    assert not fails, f"{len(fails)} perturbation(s) failed: " + " || ".join(fails)
    return seen


# =========================================================================== LayerNorm family
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("M,C", [(5, 64), (77, 96), (9, 2048)])
def test_layernorm(dtype, M, C):
    """launch_ln's vector kernels (VPL 1 / 1 / 16) read gamma and beta as f32x4."""
    x = rnd(M, C, dtype=dtype, seed=20, scale=3.0, shift=1.5)
    g, b = rnd(C, seed=21, scale=0.1, shift=1.0), rnd(C, seed=22, scale=0.1)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    ops = dict(X=Op(x), Y=Op(x, "out"), gamma=Op(g), beta=Op(b))
    sweep("sdp_layernorm", ops,
          lambda v: sp.layernorm(rows(v["X"]), v["gamma"], v["beta"], 1e-5, rows(v["Y"]), M, C),
          lambda v: close(v["Y"], ref, dtype, what="layernorm"), f"{DT_ID[dtype]} {M}x{C}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("M,C", [(77, 128), (5, 64), (9, 2048)])
def test_rowstats_row_partials_ln_stats(dtype, M, C):
    x = rnd(M, C, dtype=dtype, seed=60, scale=1.5) + rnd(M, 1, dtype=dtype, seed=61, scale=3.0)
    x64, nch = x.double(), (C + 63) // 64
    mean, rstd = x64.mean(1), 1 / torch.sqrt(x64.var(1, unbiased=False) + 1e-6)
    blk = x64.view(M, nch, 64)
    pmean = blk.mean(2)
    part_ref = torch.stack([pmean, ((blk - pmean[..., None]) ** 2).sum(2)], 2).view(M, nch * 2)

    def stats_ok(st):
        close(st[:, 0], mean, F32, rel=1e-5, what="mean")
        close(st[:, 1], rstd, F32, rel=1e-4, what="rstd")

    def part_ok(p):
        p = p.view(M, nch, 2)
        close(p[..., 0], pmean, F32, rel=1e-5, what="chunk mean")
        close(p[..., 1], part_ref.view(M, nch, 2)[..., 1], F32, rel=1e-5, what="chunk M2")

    what = f"{DT_ID[dtype]} {M}x{C}"
    blank_st, blank_p = torch.empty(M, 2, device=DEV), torch.empty(M, nch * 2, device=DEV)
    sweep("sdp_rowstats", dict(X=Op(x), stats=Op(blank_st, "out", ld=2)),
          lambda v: sp.rowstats(rows(v["X"]), 1e-6, v["stats"], M, C), lambda v: stats_ok(v["stats"]), what)
    sweep("sdp_row_partials", dict(X=Op(x), part=Op(blank_p, "out", ld=nch * 2)),
          lambda v: sp.row_partials(rows(v["X"]), M, C, v["part"]), lambda v: part_ok(v["part"]), what)
    part = torch.empty(M, nch * 2, device=DEV)
    sp.row_partials(sp.dense(x), M, C, part)
    sweep("sdp_ln_stats", dict(part=Op(part, ld=nch * 2), stats=Op(blank_st, "out", ld=2)),
          lambda v: sp.ln_stats(v["part"], sp.Rows(v["part"], nch * 2), M, C, 1e-6, v["stats"]),
          lambda v: stats_ok(v["stats"]), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("H,hd", [(4, 16), (2, 128)])
def test_qk_headnorm(dtype, H, hd):
    T, C = 77, H * hd
    qkv = rnd(T, 3 * C, dtype=dtype, seed=24, scale=2.0)
    gq, bq, gk, bk = (rnd(hd, seed=s, scale=0.1, shift=1.0 if s % 2 == 0 else 0.0) for s in (25, 26, 27, 28))
    ref = qkv.double().clone()
    ref[:, :C] = F.layer_norm(ref[:, :C].view(T, H, hd), (hd,), gq.double(), bq.double()).view(T, C)
    ref[:, C:2 * C] = F.layer_norm(ref[:, C:2 * C].view(T, H, hd), (hd,), gk.double(), bk.double()).view(T, C)
    ops = dict(QKV=Op(qkv, "inout"), gq=Op(gq), bq=Op(bq), gk=Op(gk), bk=Op(bk))
    sweep("sdp_qk_headnorm", ops,
          lambda v: sp.qk_headnorm(v["QKV"], T, H, hd, v["gq"], v["bq"], v["gk"], v["bk"], 1e-5),
          lambda v: close(v["QKV"], ref, dtype, what="qk headnorm"), f"{DT_ID[dtype]} H={H} hd={hd}")


# =========================================================================== GEMM
GEMM_EPI = ["plain", "bias_gelu", "resid_part", "ln_fold"]


@functools.lru_cache(maxsize=None)
def gemm_data(dtype, M, N, K):
    """Inputs and fp64 references of one shape, made once and left unchanged."""
    d = dict(x=rnd(M, K, dtype=dtype, seed=1), w=rnd(N, K, dtype=dtype, seed=2, scale=0.05), b=rnd(N, seed=5),
             r=rnd(M, N, dtype=dtype, seed=6))
    z = d["x"].double() @ d["w"].double().t()
    d["plain"] = z
    d["bias_gelu"] = F.gelu(z + d["b"].double())
    d["resid_part"] = z + d["b"].double() + d["r"].double()
    # LN fold: rows with a mean; statistics by the library on the aligned rows, fp32 master weight
    xl = (rnd(M, K, seed=62, scale=1.3) + rnd(M, 1, seed=63, scale=2.0)).to(dtype)
    part = torch.empty(M, (K + 63) // 64, 2, device=DEV)
    sp.row_partials(sp.dense(xl), M, K, part)
    st = torch.empty(M, 2, device=DEV)
    sp.ln_stats(part, sp.dense(xl), M, K, 1e-5, st)
    wf, colsum, cvec = sp.fold_ln_weight(rnd(N, K, seed=64, scale=0.05), rnd(K, seed=65, scale=0.2, shift=1.0),
                                         rnd(K, seed=66, scale=0.2), d["b"], dtype)
    mean, rstd = st[:, 0:1].double(), st[:, 1:2].double()
    d.update(xl=xl, st=st, wf=wf, colsum=colsum, cvec=cvec)
    d["ln_fold"] = rstd * (xl.double() @ wf.double().t()) - rstd * mean * colsum.double() + cvec.double()
    return d


@pytest.mark.parametrize("epi", GEMM_EPI)
@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (90, 128, 256)])
@pytest.mark.parametrize("dtype,kern", [(F32, 0), (BF, 9), (BF, 14)], ids=["fp32", "bf16-k9", "bf16-k14"])
def test_gemm(dtype, kern, M, N, K, epi):
    """sdp_gemm / sdp_gemm_ln: plain, bias + GELU, residual + row partials, LN fold.  bf16 starts on
    the 256 x 256 MFMA kernel with epilogue 9 or 14; fp32 always runs the generic kernel."""
    d = gemm_data(dtype, M, N, K)
    if dtype == BF:   # M = 90 is below the fast kernel's smallest M: that shape starts on the generic kernel,
        assert sp.gemm_variant(BF, M, N, K) == (1 if M >= 128 else 0)   # whose 8-B accesses test the address
    nch = (N + 63) // 64
    ln, part = epi == "ln_fold", epi == "resid_part"
    ops = dict(X=Op(d["xl"] if ln else d["x"]), W=Op(d["wf"] if ln else d["w"]), Y=Op(d["r"], "out"),
               R=Op(d["r"] if part else None), bias=Op(None if epi == "plain" else d["cvec"] if ln else d["b"]),
               ln_stats=Op(d["st"].view(-1) if ln else None), ln_colsum=Op(d["colsum"] if ln else None),
               part=Op(torch.empty(M, nch * 2, device=DEV) if part else None, "out", ld=nch * 2))
    entry = "sdp_gemm" if epi in ("plain", "bias_gelu") else "sdp_gemm_ln"

    def call(v):   # the C entry points themselves: sp.gemm wants a contiguous weight (no ldw > K)
        L, ptr = sp.lib(), lambda t: None if t is None else t.data_ptr()   # noqa: E731
        head = [sp.dcode(dtype), *rows(v["X"]).args(), v["W"].data_ptr(), v["W"].stride(0), ptr(v["bias"]),
                *(rows(v["R"]).args() if part else [None, 0, 0, 0, 0]), *rows(v["Y"]).args(), M, N, K,
                1 if epi == "bias_gelu" else 0, 0]
        stream = torch.cuda.current_stream().cuda_stream
        if entry == "sdp_gemm":
            return L.sdp_gemm(*head, stream) == 0
        return L.sdp_gemm_ln(*head, ptr(v["ln_stats"]), ptr(v["ln_colsum"]), ptr(v["part"]), stream) == 0

    def verify(v):
        close(v["Y"], d[epi], dtype, rel=(2e-5 if dtype == F32 else 2e-2) if ln else None, what=f"gemm {epi}")
        if part:   # {mean, M2} of the stored rows' 64-column chunks (test_gemm_emits_row_partials)
            y = v["Y"].double()
            p = v["part"].view(M, nch, 2)
            for c in range(nch):
                blk = y[:, 64 * c: 64 * c + 64]
                mu = blk.mean(1)
                close(p[:, c, 0], mu, F32, rel=1e-5, what="emitted chunk mean")
                close(p[:, c, 1], ((blk - mu[:, None]) ** 2).sum(1), F32, rel=1e-4, what="emitted chunk M2")

    old = sp.lib().sdp_gemm_set_fast_kernel(kern) if kern else None
    try:
        sweep(entry, ops, call, verify, f"{DT_ID[dtype]} k{kern} {M}x{N}x{K} {epi}")
    finally:
        if kern:
            sp.lib().sdp_gemm_set_fast_kernel(old)


# =========================================================================== depthwise conv
def conv64(x, w, k):
    """x fp64 [B, H, W, C], w fp64 [C, k, k]: 'same' cross-correlation per channel, by shifts."""
    B, H, W, C = x.shape
    p = k // 2
    xp = torch.zeros(B, H + 2 * p, W + 2 * p, C, dtype=torch.float64, device=x.device)
    xp[:, p:p + H, p:p + W] = x
    out = torch.zeros_like(x)
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + H, kx:kx + W] * w[:, ky, kx]
    return out


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,H,W,C,k", [(1, 16, 16, 128, 7), (3, 7, 7, 64, 3)])
@pytest.mark.parametrize("dtype,kern", [(F32, 1), (F32, 2), (BF, 1), (BF, 2), (BF, 3)],
                         ids=["fp32-tier1", "fp32-tier2", "bf16-tier1", "bf16-tier2", "bf16-tier3"])
def test_dwconv(dtype, kern, B, H, W, C, k, ln):
    """Tier 3 (MFMA, bf16) and tier 2 need 16-B rows, float2 statistics and (tier 2) a 16-B bias;
    tier 1 takes anything, with element accesses where an operand is not aligned."""
    M = B * H * W
    x = rnd(M, C, dtype=dtype, seed=30, scale=2.0, shift=0.5)
    w, b = rnd(C, k * k, seed=31, scale=0.2), rnd(C, seed=32)
    xin = x.double()
    st = g = be = None
    if ln:
        g, be = rnd(C, seed=33, scale=0.1, shift=1.0), rnd(C, seed=34, scale=0.1)
        st = torch.empty(M, 2, device=DEV)
        sp.rowstats(sp.dense(x), 1e-6, st, M, C)
        xin = (xin - st[:, 0:1].double()) * st[:, 1:2].double() * g.double() + be.double()
    ref = (conv64(xin.view(B, H, W, C), w.double().view(C, k, k), k) + b.double()).view(M, C)
    ops = dict(X=Op(x), Y=Op(x, "out"), stats=Op(st.view(-1) if ln else None), ln_gamma=Op(g), ln_beta=Op(be),
               weight=Op(w.view(-1)), bias=Op(b))

    def call(v):
        sp.dwconv(rows(v["X"]), v["weight"].view(C, k * k), v["bias"], rows(v["Y"]), B, H, W, C, k, stats=v["stats"],
                  ln_gamma=v["ln_gamma"], ln_beta=v["ln_beta"])

    old = sp.lib().sdp_dwconv_set_kernel(kern)
    try:
        sweep("sdp_dwconv", ops, call, lambda v: close(v["Y"], ref, dtype, what="dwconv"),
              f"{DT_ID[dtype]} tier {kern} {(B, H, W, C, k)} {'ln' if ln else 'plain'}")
    finally:
        sp.lib().sdp_dwconv_set_kernel(old)


# =========================================================================== attention
def attn_ref(qkv64, B, N, H, hd, add=None):
    q, k, v = qkv64.view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if add is not None:
        s = s + add
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * N, H * hd)


try:
    ATTN_TIERS = [2, 3, 4, 5, 6] if sp.lib().sdp_build_info() != 0 else [3, 4, 5]
except Exception:  # library not loadable here (CPU collection without a build)
    ATTN_TIERS = [3, 4, 5]


@pytest.mark.parametrize("mode", ["plain", "qknorm", "mask", "rows"])
@pytest.mark.parametrize("B,N,H,hd", [(2, 53, 4, 16), (1, 77, 2, 64), (1, 260, 8, 96)])
@pytest.mark.parametrize("dtype,kern", [(F32, 0)] + [(BF, t) for t in ATTN_TIERS],
                         ids=["fp32"] + [f"bf16-tier{t}" for t in ATTN_TIERS])
def test_attention(dtype, kern, B, N, H, hd, mode):
    """sdp_attention / sdp_attention_rows.  The flash kernels load QKV rows by 16 B, store O by 8 B
    and read the q / k norm parameters as f32x4; anything else goes to the generic kernel (which
    applies the norms in place on the QKV rows, as the header says)."""
    C = H * hd
    qkv = rnd(B * N, 3 * C, dtype=dtype, seed=44, scale=2.0 if mode == "qknorm" else 1.0)
    nrm = [None] * 4
    ref_in = qkv.double().clone()
    if mode == "qknorm":
        nrm = [rnd(hd, seed=s, scale=0.1, shift=1.0 if s % 2 == 1 else 0.0) for s in (45, 46, 47, 48)]
        n64 = [t.double() for t in nrm]
        ref_in[:, :C] = F.layer_norm(ref_in[:, :C].view(-1, H, hd), (hd,), n64[0], n64[1]).view(-1, C)
        ref_in[:, C:2 * C] = F.layer_norm(ref_in[:, C:2 * C].view(-1, H, hd), (hd,), n64[2], n64[3]).view(-1, C)
        ref_in = ref_in.to(dtype).double()   # the normalised q and k are rounded to the storage type
    add = None
    if mode == "mask":
        add = torch.zeros(B, 1, N, N, device=DEV)
        add[0, 0, :, N - 10:] = float("-inf")
        add[B - 1] += rnd(1, N, N, seed=42)
    ref = attn_ref(ref_in, B, N, H, hd, None if add is None else add.double())
    q_rows = 5 if mode == "rows" else None
    # a mask sends every call to attn_generic (sdp_attention_variant is 0 with one): those sweeps start
    # in the element tier and hold the mask operand and the generic kernel to the contract
    if dtype == BF and mode != "mask":
        old = sp.lib().sdp_attention_set_kernel(kern)
        try:
            assert sp.attention_variant(BF, N, H, hd) >= 2, "the aligned call must start on a flash kernel"
        finally:
            sp.lib().sdp_attention_set_kernel(old)
    # rows mode: O starts as zeros, for rows past q_rows may stay unwritten
    o_op = Op(torch.zeros(B * N, C, dtype=dtype, device=DEV), "inout") if mode == "rows" else Op(qkv[:, :C], "out")
    ops = dict(QKV=Op(qkv, "inout" if mode == "qknorm" else "in"), O=o_op,
               q_gamma=Op(nrm[0]), q_beta=Op(nrm[1]), k_gamma=Op(nrm[2]), k_beta=Op(nrm[3]),
               mask=Op(add.view(-1) if add is not None else None))

    def call(v):
        m = v["mask"]
        sp.attention(v["QKV"], v["O"], B, N, H, hd, m, N * N if m is not None else 0, 0,
                     qk_norm=(v["q_gamma"], v["q_beta"], v["k_gamma"], v["k_beta"]) if mode == "qknorm" else None,
                     eps=1e-5, q_rows=q_rows)

    def verify(v):
        if mode == "qknorm" and not torch.equal(v["QKV"], qkv):
            # the generic path normalised q and k in place (header): then they are the normalised rows
            close(v["QKV"], ref_in, dtype, what="q / k normalised in place")
            assert torch.equal(v["QKV"][:, 2 * C:], qkv[:, 2 * C:]), "the v third was modified"
        got, want = v["O"], ref
        if q_rows is not None:   # rows at or past q_rows of an image may or may not be written
            keep = (torch.arange(B * N, device=DEV) % N) < q_rows
            got, want = got[keep], ref[keep]
            assert torch.isfinite(got).all()
        close(got, want, dtype, rel=(2e-5 if dtype == F32 else 2e-2) if mode == "qknorm" else None, what="attention")

    old = sp.lib().sdp_attention_set_kernel(kern) if kern else None
    try:
        entry = "sdp_attention_rows" if mode == "rows" else "sdp_attention"
        sweep(entry, ops, call, verify, f"{DT_ID[dtype]} tier {kern} {(B, N, H, hd)} {mode}")
    finally:
        if kern:
            sp.lib().sdp_attention_set_kernel(old)


# =========================================================================== element-wise entry points
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_act_and_cast(dtype):
    """sdp_act / sdp_cast walk a flat array one element per lane: a contiguous tensor at any storage
    offset gives the aligned run's result bit for bit."""
    M, N = 37, 64
    x = torch.linspace(-6, 6, M * N, device=DEV).view(M, N).to(dtype)
    other = BF if dtype == F32 else F32
    for code in ACTS:
        y0 = torch.empty_like(x)
        sp.act(x, y0, code)
        close(y0, ACTS[code](x.double()), dtype, rel=2e-6 if dtype == F32 else 8e-3, what=f"act {code}")

        def same(v, y0=y0):
            assert torch.equal(v["Y"], y0), "the result depends on the operand's address"
        sweep("sdp_act", dict(X=Op(x, ld=N), Y=Op(x, "out", ld=N)), lambda v, code=code: sp.act(v["X"], v["Y"], code),
              same, f"{DT_ID[dtype]} act {code}")
    c0 = sp.cast(x, other)
    assert torch.equal(c0, x.to(other))

    def cast(v):
        rc = sp.lib().sdp_cast(sp.dcode(dtype), v["X"].data_ptr(), sp.dcode(other), v["Y"].data_ptr(), M * N,
                               torch.cuda.current_stream().cuda_stream)
        return rc == 0

    def same_cast(v):
        assert torch.equal(v["Y"], c0)
    sweep("sdp_cast", dict(X=Op(x, ld=N), Y=Op(c0, "out", ld=N)), cast, same_cast, f"{DT_ID[dtype]} cast")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("C", [128, 130])   # 16-B row-copy kernel / element kernel
def test_copy_rows(dtype, C):
    B, R = 2, 5
    src = rnd(B * R, C, dtype=dtype, seed=55)

    def call(v):
        s, d = v["src"], v["dst"]
        sp.copy_rows(s, s.stride(0), R * s.stride(0), d, d.stride(0), R * d.stride(0), B, R, C)

    def same(v):
        assert torch.equal(v["dst"], src)
    sweep("sdp_copy_rows", dict(src=Op(src), dst=Op(src, "out")), call, same, f"{DT_ID[dtype]} C={C}")


@pytest.mark.parametrize("idt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_patchify(dtype, idt):
    """The strip kernel reads pixel pairs and writes column pairs; an image or an output one element
    off goes to the per-row kernel.  p = 8, img 64."""
    p, img, Bn = 8, 64, 2
    kpad = 3 * p * p
    x = rnd(Bn, 3, img, img, dtype=idt, seed=50)
    ref = F.unfold(x.double(), p, stride=p).transpose(1, 2).reshape(-1, kpad).to(dtype)
    n = (img // p) ** 2 * Bn

    def call(v):
        sp.patchify(v["img"].view(Bn, 3, img, img), v["out"], p, kpad)

    def same(v):
        assert torch.equal(v["out"], ref)
    sweep("sdp_patchify", dict(img=Op(x.view(Bn * 3 * img, img), ld=img), out=Op(ref.view(n, kpad), "out", ld=kpad)),
          call, same, f"{DT_ID[idt]}->{DT_ID[dtype]}")


# =========================================================================== multi-tensor kernels
SIZES = [1, 7, 4096, 4097]


def flat_views(numels, seed, first=4, fill=None):
    """Views of one flat fp32 buffer filled with the sentinel: the first starts ``first`` bytes past a
    16-B boundary, pads of 1, 2 and 3 floats cycle between the tensors (offsets 4, 8 and 12 mod 16
    all occur).  Returns (views, the buffer as int32, mask of the pad elements)."""
    _, sent = al.SENTINEL[F32]
    offs, o = [], 0
    for i, n in enumerate(numels):
        want = (first // 4 - 1 + i) % 3 + 1          # floats past a 16-B boundary: 1, 2, 3 in turn
        o += (want - o) % 4 or 4                      # a pad of 1..4 sentinel floats
        offs.append(o)
        o += n
    ibuf = torch.full((o + 4,), sent, dtype=torch.int32, device=DEV)
    assert ibuf.data_ptr() % 16 == 0
    buf = ibuf.view(F32)
    pad = torch.ones(o + 4, dtype=torch.bool, device=DEV)
    views = []
    for i, (n, off) in enumerate(zip(numels, offs)):
        t = buf[off:off + n]
        t.copy_(rnd(n, seed=seed + i) if fill is None else torch.full((n,), fill, device=DEV))
        pad[off:off + n] = False
        views.append(t)
    return views, ibuf, pad


def pads_untouched(ibuf, pad):
    _, sent = al.SENTINEL[F32]
    return bool((ibuf[pad] == sent).all())


@pytest.mark.parametrize("first", [4, 8, 12])
def test_adamw_and_grad_sumsq_parts_on_flat_views(first):
    """Parameters, gradients and both moments as views of flat buffers (every tensor of the pointer
    tables off a 16-B boundary): two fused steps with clipping are bit-equal to the same steps on
    ordinary tensors, and no pad element is written.  sdp_grad_sumsq_parts, sdp_sum_partials,
    sdp_adamw_dev and sdp_adamw_finish are element-wise; the deterministic norm makes the clip
    coefficient -- and so every parameter -- reproducible."""
    import sdpnet_train as st
    pv, pbuf, ppad = flat_views(SIZES, 100, first)
    gv, gbuf, gpad = flat_views(SIZES, 200, first)
    assert {t.data_ptr() % 16 for t in pv} == {4, 8, 12} and pv[0].data_ptr() % 16 == first
    flat = [torch.nn.Parameter(t) for t in pv]
    twin = [torch.nn.Parameter(t.clone()) for t in pv]
    assert all(t.data_ptr() % 16 == 0 for t in twin)
    oa, ob = st.AdamW(flat, lr=1e-2, weight_decay=0.1), st.AdamW(twin, lr=1e-2, weight_decay=0.1)
    mom = []
    for step in range(2):
        for i, (a, b) in enumerate(zip(flat, twin)):
            g = rnd(a.numel(), seed=300 + 10 * step + i, scale=3.0)
            gv[i].copy_(g)
            a.grad, b.grad = gv[i], g.clone()
        if step == 0:   # the moments of the flat run are views of flat buffers too
            oa.step(grad_scale=1.0, max_norm=0.0)   # creates the state
            ob.step(grad_scale=1.0, max_norm=0.0)
            for name in ("exp_avg", "exp_avg_sq"):
                mv, mbuf, mpad = flat_views(SIZES, 0, first, fill=0.0)
                for p, t in zip(flat, mv):
                    t.copy_(oa.state[p][name])
                    oa.state[p][name] = t
                mom.append((mbuf, mpad))
        else:
            oa.step(grad_scale=2.0, max_norm=1.0)
            ob.step(grad_scale=2.0, max_norm=1.0)
    torch.cuda.synchronize()
    for a, b in zip(flat, twin):
        assert torch.equal(a.detach(), b.detach()), "parameters differ from the run on ordinary tensors"
        for name in ("exp_avg", "exp_avg_sq"):
            assert oa.state[a][name].data_ptr() % 16 != 0
            assert torch.equal(oa.state[a][name], ob.state[b][name]), name
        assert float(oa.state[a]["step"]) == float(ob.state[b]["step"]) == 2.0
    assert pads_untouched(pbuf, ppad) and pads_untouched(gbuf, gpad)
    assert all(pads_untouched(b, m) for b, m in mom)


@pytest.mark.parametrize("first", [4, 8, 12])
def test_ema_update_on_flat_views(first):
    """ema_k takes its f32x4 path only when out, a and b are all 16-B aligned (a per-tensor test in
    the kernel); any other placement runs its element loop, bit-equal."""
    av, abuf, apad = flat_views(SIZES, 400, first)
    bv, bbuf, bpad = flat_views(SIZES, 500, first)
    a0, b0 = [t.clone() for t in av], [t.clone() for t in bv]
    ref = [t.clone() for t in a0]
    dev = torch.device(DEV)
    blocks, nb = sp.mt_block_table(SIZES, dev)
    sizes = torch.tensor(SIZES, dtype=torch.int64, device=DEV)
    ptr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)  # noqa: E731
    sp.ema_update(ptr(ref), ptr(ref), ptr(b0), sizes, blocks, nb, 0.9, 0.1)        # aligned run (in place on a)
    sp.ema_update(ptr(av), ptr(av), ptr(bv), sizes, blocks, nb, 0.9, 0.1)          # flat views
    torch.cuda.synchronize()
    for got, want, b, bb in zip(av, ref, bv, b0):
        assert torch.equal(got, want) and torch.equal(b, bb)
    assert pads_untouched(abuf, apad) and pads_untouched(bbuf, bpad)
