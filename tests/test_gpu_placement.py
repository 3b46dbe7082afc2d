"""GPU: the kernels on operands placed beyond 2^31 bytes, 2^32 bytes and 2^31 elements, inside
guard bands (placement.py).

Every case runs the same data twice -- all operands "near" (whole extent below 2^31 bytes) and
one operand "far" (groups of rows on both sides of each mark) -- and asserts
  * the far result bit-equal to the near one (same arithmetic on both sides of every dispatch
    guard; LN partials across the GEMM's `small` guard to the 1e-5 / 1e-4 of
    test_gemm_specialised_epilogue_bit_identical),
  * the near result against the fp32 reference with the tolerance of the kernel's own test,
  * every element outside the logical ones untouched (padding columns, rows between the groups,
    rows before / after the operand), no logical output row left unwritten, inputs unchanged.
The sentinel outside the logical elements is a NaN, so a read there poisons the result.

A test holds at most 16 GiB of device memory (one far operand per case: 4 GiB bf16, 8 GiB fp32)
and skips only when torch.cuda.mem_get_info() shows less free memory than it needs.
SDPNET_PLACEMENT_REPORT=<file> appends one JSON line per test (time, peak memory, marks crossed).
"""
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

import placement as pl
import sdpnet_hip as sp
from test_gpu_kernels import ACTS, attn_ref, close, rnd
from test_gpu_train_kernels import ACT_REF, close as tclose

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
DTYPES = [F32, BF]
GROUPS = 5          # bf16: marks at groups 2 and 4 (base 2^30); fp32: at groups 1, 2 and 4 (base 2^31)
GIB = 1 << 30
_CROSSED = []       # (operand, dtype, marks) of the far placements of the running test
_FAR_BLOCK = [0]    # bytes of the far block the caching allocator holds for the running test


@pytest.fixture(autouse=True)
def _measured(request):
    """Exact fp32 references (as test_gpu_kernels.py), memory released at exit, and the test's
    time / peak device memory for the report."""
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    del _CROSSED[:]
    _FAR_BLOCK[0] = 0
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak, held = torch.cuda.max_memory_allocated(), torch.cuda.max_memory_reserved()
    torch.cuda.empty_cache()
    torch.set_float32_matmul_precision(old)
    out = os.environ.get("SDPNET_PLACEMENT_REPORT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"test": request.node.name, "seconds": round(dt, 3), "peak_gib": round(peak / GIB, 3),
                                "reserved_gib": round(held / GIB, 3),
                                "crossed": sorted({f"{n}:{d}:{','.join(str(m) for m in mk)}"
                                                   for n, d, mk in _CROSSED})}) + "\n")


def need(nbytes: int):
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip(f"needs {nbytes / GIB:.1f} GiB of free device memory, torch.cuda.mem_get_info() shows "
                    f"{free / GIB:.1f} GiB")


def far_block(nbytes: int):
    """Before a far allocation: the freed far block of the previous run is reused when this one fits
    into it (a 4 - 8 GiB allocation from the driver now and then takes a second), and released
    first when it does not, so that a test never holds two of them."""
    if nbytes > _FAR_BLOCK[0]:
        torch.cuda.empty_cache()
        _FAR_BLOCK[0] = nbytes
    need(nbytes + GIB)


def place(name, C, dtype, far, grp=64, M=None, data=None, ld=None):
    if far:
        fm = pl.Placement.far_map(C, dtype, pl.marks_for(dtype), grp, 2 if dtype == BF else 1, M, ld)
        far_block(fm["total_rows"] * fm["ld"] * (2 if dtype == BF else 4))
        p = pl.Placement.far(C, dtype, pl.marks_for(dtype), DEV, grp=grp, sub=2 if dtype == BF else 1, M=M, ld=ld)
        assert p.groups == GROUPS and p.crossed() == list(p.marks)
        _CROSSED.append((name, str(dtype).split(".")[-1], tuple(p.marks)))
    else:
        p = pl.Placement.near(C, dtype, DEV, grp=grp, groups=GROUPS, M=M, ld=ld)
        assert p.nbytes < 1 << 31
    if data is not None:
        p.scatter(data)
    return p


def run_placements(spec, outs, call, configs, grp=64, M=None, cmp=None):
    """spec: name -> (C, dtype, dense data or None).  configs: far-operand name tuples; a name
    "a=b" makes operand a the very buffer of operand b (which then starts with a's data).  call(P)
    runs the kernel on the placements and may return extra placements to judge (name -> Placement).
    The first config is run all-near too, and is what every other result must equal (cmp[name]
    replaces torch.equal).  Returns the near results, for the comparison with the reference."""
    base = None
    for far in [None] + list(configs):
        names = set(far or ())
        alias = dict(n.split("=") for n in names if "=" in n)
        P = {}
        for name, (C, dtype, data) in spec.items():
            if name in alias:
                continue
            src = next((a for a, b in alias.items() if b == name), name)
            P[name] = place(name, C, dtype, name in names, grp, M, spec[src][2])
        for a, b in alias.items():
            P[a] = P[b]
        extra = call(P) or {}
        torch.cuda.synchronize()
        got = {}
        tag = f"far {sorted(names)}" if far else "near"
        for name, p in list(P.items()) + list(extra.items()):
            if name in alias:
                continue
            if isinstance(p, torch.Tensor):   # a dense result of the call (sums over all rows)
                got[name] = p
                continue
            written = name in outs or name in extra
            p.check(f"{name} [{tag}]", written=written)
            if written:
                got[name] = p.gather().clone()
            else:
                assert torch.equal(p.gather(), spec[name][2]), f"input {name} changed [{tag}]"
        if base is None:
            base = got
        else:
            for name, v in got.items():
                if cmp and name in cmp:
                    cmp[name](v, base[name], f"{name} [{tag}] vs near")
                else:
                    assert torch.equal(v, base[name]), f"{name} [{tag}] differs from the near placement"
        del P, extra, got, p
    return base


def fast_kernel(kern):
    class _K:
        def __enter__(self):
            self.old = sp.lib().sdp_gemm_set_fast_kernel(kern)

        def __exit__(self, *a):
            sp.lib().sdp_gemm_set_fast_kernel(self.old)
    return _K()


def part_cmp(got, near, what):
    close(got[:, 0::2], near[:, 0::2], F32, rel=1e-5, what=what + " partial mean")
    close(got[:, 1::2], near[:, 1::2], F32, rel=1e-4, what=what + " partial M2")


M_ROWS = GROUPS * 64 - 7   # ragged last group, ragged against the 256-row GEMM tile


# ------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("act,pre", [(1, False), (3, True)])
def test_gemm_fp32_generic(act, pre):
    M, N, K = M_ROWS, 130, 96
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
    assert sp.gemm_variant(F32, M, N, K) == 0

    def call(P):
        sp.gemm(P["x"].rows, w, P["y"].rows, M, N, K, bias=b, resid=P["r"].rows, act=act, resid_pre=pre)

    spec = {"x": (K, F32, x), "y": (N, F32, None), "r": (N, F32, r)}
    got = run_placements(spec, {"y"}, call, [("x",), ("y",), ("r",), ("r=y",), ("r=y", "y")], M=M)
    z = x @ w.t() + b
    close(got["y"], ACTS[act](z + r) if pre else ACTS[act](z) + r, F32, what="fp32 generic gemm")


GEMM_SHAPES = {"plain": (328, 768), "bias": (3072, 768), "ln_bias": (3072, 768), "resid_part": (768, 3072),
               "bias_resid_part": (768, 768)}   # N (328: ragged against the 64 / 256-column tiles), K


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("combo", list(GEMM_SHAPES))
@pytest.mark.parametrize("kern", [9, 14])
def test_gemm_bf16_fast(kern, combo, act):
    """The model's epilogue combinations across the `small` guard: near = the specialised
    (buffer-descriptor, 32-bit offset) epilogue at kernel 14, far = the run-time-flag one."""
    M = M_ROWS
    N, K = GEMM_SHAPES[combo]
    assert sp.gemm_variant(BF, M, N, K) == 1
    x = rnd(M, K, dtype=BF, seed=81)
    w = rnd(N, K, dtype=BF, seed=82, scale=0.05)
    b = rnd(N, seed=83) if "bias" in combo else None
    has_r = "resid" in combo
    r = rnd(M, N, dtype=BF, seed=84) if has_r else None
    ln = None
    if combo == "ln_bias":
        part_x = torch.empty(M, K // 64, 2, device=DEV)
        sp.row_partials(sp.dense(x), M, K, part_x)
        st = torch.empty(M, 2, device=DEV)
        sp.ln_stats(part_x, sp.dense(x), M, K, 1e-5, st)
        g, be = rnd(K, seed=85) * 0.2 + 1, rnd(K, seed=86) * 0.2
        w, colsum, b = sp.fold_ln_weight(w.float(), g, be, b, BF)
        ln = (st, colsum)
    nch = N // 64

    def call(P):
        part = P["y"].twin(2 * nch, F32) if has_r else None
        with fast_kernel(kern):
            sp.gemm(P["x"].rows, w, P["y"].rows, M, N, K, bias=b, resid=P["r"].rows if has_r else None, act=act,
                    ln=ln, part=part.t if has_r else None)
        return {"part": part} if has_r else None

    spec = {"x": (K, BF, x), "y": (N, BF, None)}
    configs = [("x",), ("y",)]
    if has_r:
        spec["r"] = (N, BF, r)
        configs += [("r",), ("r=y",), ("r=y", "y")]
    got = run_placements(spec, {"y"}, call, configs, M=M, cmp={"part": part_cmp})
    acc = x.float() @ w.float().t()
    if ln is not None:
        v = st[:, 1:2] * acc - (st[:, 1] * st[:, 0])[:, None] * colsum[None] + b
    else:
        v = acc + (b if b is not None else 0)
    v = ACTS[act](v)
    if has_r:
        v = v.to(BF).float() + r.float()
    close(got["y"], v, BF, what=f"kernel {kern} {combo}")
    if has_r:
        yc = got["y"].float().view(M, nch, 64)
        mu = yc.mean(-1)
        p = got["part"].view(M, nch, 2)
        close(p[..., 0], mu, F32, rel=1e-5, what="partial mean vs stored rows")
        close(p[..., 1], ((yc - mu[..., None]) ** 2).sum(-1), F32, rel=1e-4, what="partial M2 vs stored rows")


@pytest.mark.parametrize("act,pre,has_b", [(3, False, True), (0, True, False), (1, True, True)])
def test_gemm_bf16_other_epilogues(act, pre, has_b):
    """Another activation, and resid_pre (with an activation it leaves the whole-line epilogue)."""
    M, N, K = M_ROWS, 768, 768
    x, w = rnd(M, K, dtype=BF, seed=91), rnd(N, K, dtype=BF, seed=92, scale=0.05)
    b = rnd(N, seed=93) if has_b else None
    r = rnd(M, N, dtype=BF, seed=94)

    def call(P):
        sp.gemm(P["x"].rows, w, P["y"].rows, M, N, K, bias=b, resid=P["r"].rows, act=act, resid_pre=pre)

    spec = {"x": (K, BF, x), "y": (N, BF, None), "r": (N, BF, r)}
    got = run_placements(spec, {"y"}, call, [("x",), ("y",), ("r",), ("r=y", "y")], M=M)
    z = x.float() @ w.float().t() + (b if has_b else 0)
    close(got["y"], ACTS[act](z + r.float()) if pre else ACTS[act](z) + r.float(), BF, what=f"act {act} pre {pre}")


@pytest.mark.parametrize("combo", ["bias", "resid_part"])
def test_gemm_bf16_groups_of_four(combo):
    """grp < 8 is the other way out of `small`: the same rows in groups of 4 equal groups of 64."""
    M, N, K = M_ROWS, 768, 768
    x, w = rnd(M, K, dtype=BF, seed=95), rnd(N, K, dtype=BF, seed=96, scale=0.05)
    b = rnd(N, seed=97) if combo == "bias" else None
    r = rnd(M, N, dtype=BF, seed=98) if combo != "bias" else None
    res = []
    for grp in (64, 4):
        px = place("x", K, BF, False, grp, M, x)
        py = place("y", N, BF, False, grp, M, r)
        part = py.twin(2 * (N // 64), F32) if r is not None else None
        sp.gemm(px.rows, w, py.rows, M, N, K, bias=b, resid=py.rows if r is not None else None, act=1,
                part=None if part is None else part.t)
        torch.cuda.synchronize()
        px.assert_untouched("x")
        py.check(f"y grp {grp}", written=True)
        assert torch.equal(px.gather(), x)
        if part is not None:
            part.check(f"part grp {grp}", written=True)
        res.append((py.gather().clone(), None if part is None else part.gather().clone()))
    assert torch.equal(res[0][0], res[1][0]), "groups of 4 differ from groups of 64"
    if r is not None:
        part_cmp(res[1][1], res[0][1], "groups of 4")
    v = F.gelu(x.float() @ w.float().t() + (b if b is not None else 0))
    close(res[0][0], v.to(BF).float() + r.float() if r is not None else v, BF, what=combo)


# ---------------------------------------------------------------------- LayerNorm family
def _ln_data(M, C, dtype):
    x = (rnd(M, C, seed=20, scale=1.5) + rnd(M, 1, seed=21, scale=2.0)).to(dtype)
    return x, rnd(C, seed=22) * 0.1 + 1, rnd(C, seed=23) * 0.1


@pytest.mark.parametrize("C", [768, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_and_ln_apply(dtype, C):
    M = M_ROWS
    x, g, b = _ln_data(M, C, dtype)
    st = torch.full((M, 2), float("nan"), device=DEV)

    def call(P):
        sp.layernorm(P["x"].rows, g, b, 1e-6, P["y"].rows, M, C)
        st.fill_(float("nan"))
        sp.rowstats(P["x"].rows, 1e-6, st, M, C)
        sp.ln_apply(P["x"].rows, st, g, b, P["y2"].rows, M, C)
        P["st"].scatter(st)

    spec = {"x": (C, dtype, x), "y": (C, dtype, None), "y2": (C, dtype, None), "st": (2, F32, None)}
    got = run_placements(spec, {"y", "y2", "st"}, call, [("x",), ("y",), ("y2",)], M=M)
    xf = x.float()
    ref = F.layer_norm(xf, (C,), g, b, 1e-6)
    close(got["y"], ref, dtype, what="layernorm")
    tclose(got["y2"], ref, 2e-5 if dtype == F32 else 2e-2, "ln_apply")
    ref_st = torch.stack([xf.mean(1), 1 / torch.sqrt(xf.var(1, unbiased=False) + 1e-6)], 1)
    close(got["st"], ref_st, F32, rel=1e-5, what="rowstats")


@pytest.mark.parametrize("C", [768, 200])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_partials_ln_stats_ln_fwd(dtype, C):
    M = M_ROWS
    x, g, b = _ln_data(M, C, dtype)
    nch = (C + 63) // 64
    st, st2 = torch.empty(M, 2, device=DEV), torch.empty(M, 2, device=DEV)

    def call(P):
        part = P["x"].twin(2 * nch, F32)
        sp.row_partials(P["x"].rows, M, C, part.t)
        sp.ln_stats(part.t, P["x"].rows, M, C, 1e-6, st.fill_(float("nan")))
        sp.ln_fwd(P["x"].rows, 1e-5, g, b, st2.fill_(float("nan")), P["y"].rows, M, C)
        P["st"].scatter(st)
        P["st2"].scatter(st2)
        return {"part": part}

    spec = {"x": (C, dtype, x), "y": (C, dtype, None), "st": (2, F32, None), "st2": (2, F32, None)}
    got = run_placements(spec, {"y", "st", "st2"}, call, [("x",), ("y",)], M=M)
    xf = x.float()
    p = got["part"].view(M, nch, 2)
    for c in range(nch):
        blk = xf[:, 64 * c: 64 * c + 64]
        mu = blk.mean(1)
        close(p[:, c, 0], mu, F32, rel=1e-5, what="chunk mean")
        close(p[:, c, 1], ((blk - mu[:, None]) ** 2).sum(1), F32, rel=1e-5, what="chunk M2")
    close(got["st"][:, 0], xf.mean(1), F32, rel=1e-5, what="mean")
    close(got["st"][:, 1], 1 / torch.sqrt(xf.var(1, unbiased=False) + 1e-6), F32, rel=1e-4, what="rstd")
    tclose(got["st2"][:, 0], xf.mean(1), 1e-5, "ln_fwd mean")
    tclose(got["st2"][:, 1], 1 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5), 1e-4, "ln_fwd rstd")
    tclose(got["y"], F.layer_norm(xf, (C,), g, b, 1e-5), 2e-5 if dtype == F32 else 2e-2, "ln_fwd")


# ------------------------------------------------------------- row copies, means, rowscale
@pytest.mark.parametrize("C", [128, 130])   # 16-B / scalar row-copy kernels
@pytest.mark.parametrize("dtype", DTYPES)
def test_transposes_copies_group_mean(dtype, C):
    B, H, W = GROUPS, 8, 8
    M = B * H * W
    x = rnd(B, C, H, W, dtype=dtype, seed=51)
    rows = x.permute(0, 2, 3, 1).reshape(M, C).contiguous()
    back = torch.empty_like(x)
    mean = torch.empty(B, C, dtype=dtype, device=DEV)

    def call(P):
        sp.nchw_to_rows(x, P["y"].rows)
        sp.rows_to_nchw(P["x"].rows, back.fill_(float("nan")))
        sp.group_mean(P["x"].rows, mean.fill_(float("nan")), B, H * W, C)
        src, dst = P["x"], P["c"]
        sp.copy_rows(src.t, src.ld, src.gstride * src.ld, dst.t, dst.ld, dst.gstride * dst.ld, B, H * W, C,
                     src_offset_rows=src.off, dst_offset_rows=dst.off)
        P["back"].scatter(back.permute(0, 2, 3, 1).reshape(M, C))
        P["mean"].scatter(mean.repeat_interleave(H * W, 0))

    spec = {"x": (C, dtype, rows), "y": (C, dtype, None), "c": (C, dtype, None), "back": (C, dtype, None),
            "mean": (C, dtype, None)}
    got = run_placements(spec, {"y", "c", "back", "mean"}, call, [("x",), ("y",), ("c",)], M=M)
    assert torch.equal(got["y"], rows) and torch.equal(got["c"], rows) and torch.equal(got["back"], rows)
    close(got["mean"][::H * W], rows.float().view(B, H * W, C).mean(1), dtype, rel=1e-5 if dtype == F32 else 8e-3)


@pytest.mark.parametrize("xdt,ydt,act", [(F32, F32, 0), (BF, BF, 0), (BF, F32, 0), (BF, BF, 1), (F32, F32, 7)])
def test_rowscale_add(xdt, ydt, act):
    """sdp_rowscale_add, _mixed and sdp_act_rowscale_add: y = act(x) * scale[m / sgrp] + resid."""
    M, N, sgrp = M_ROWS, 768, 64
    x, r = rnd(M, N, seed=60, dtype=xdt), rnd(M, N, seed=61, dtype=ydt)
    sc = (torch.rand(GROUPS, generator=torch.Generator().manual_seed(2)) + 0.5).to(DEV)

    def call(P):
        sp.rowscale_add(P["x"].rows, P["y"].rows, M, N, scale=sc, sgrp=sgrp, resid=P["r"].rows, act=act)

    spec = {"x": (N, xdt, x), "y": (N, ydt, None), "r": (N, ydt, r)}
    got = run_placements(spec, {"y"}, call, [("x",), ("y",), ("r",), ("r=y", "y")], M=M)
    ref = ACT_REF[act](x.float()) * sc.repeat_interleave(sgrp)[:M, None] + r.float()
    tclose(got["y"], ref, 2e-5 if ydt == F32 and xdt == F32 else 2e-2, "rowscale_add")


@pytest.mark.parametrize("dmode", [1, 2])
def test_rowscale_add_dropout(dmode):
    """The fused dropout form is bit-identical to its two passes (as its own test asserts), far as near."""
    M, N, p, seed = M_ROWS, 768, 0.2, 12345
    x, r = rnd(M, N, seed=62, dtype=BF), rnd(M, N, seed=63, dtype=BF)

    def call(P):
        sp.rowscale_add(P["x"].rows, P["y"].rows, M, N, resid=P["r"].rows, p=p, seed=seed, dmode=dmode)

    spec = {"x": (N, BF, x), "y": (N, BF, None), "r": (N, BF, r)}
    got = run_placements(spec, {"y"}, call, [("x",), ("y",), ("r",)], M=M)
    ref = torch.empty(M, N, dtype=BF, device=DEV)
    if dmode == 1:
        tmp = torch.empty_like(x)
        sp.act_fwd(x, tmp, M, N, 0, p, seed)
        sp.rowscale_add(sp.dense(tmp), sp.dense(ref), M, N, resid=sp.dense(r))
    else:
        sp.rowscale_add(sp.dense(x), sp.dense(ref), M, N, resid=sp.dense(r))
        sp.act_bwd(ref, ref, ref, M, N, 0, p, seed)
    assert torch.equal(got["y"], ref)


# ------------------------------------------------------------------------- depthwise conv
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("kern", [1, 2, 3])
@pytest.mark.parametrize("dtype,C", [(F32, 64), (BF, 768), (BF, 40)])
def test_dwconv(dtype, C, kern, ln):
    B, H, W, k = GROUPS, 8, 8, 7
    M = B * H * W
    x = rnd(B, C, H, W, dtype=dtype, seed=30, scale=2.0) + 0.5
    w, b = rnd(C, 1, k, k, seed=31, scale=0.2), rnd(C, seed=32)
    rows = x.permute(0, 2, 3, 1).reshape(M, C).contiguous()
    xin, kw = x.float(), {}
    if ln:
        g, be = rnd(C, seed=33) * 0.1 + 1, rnd(C, seed=34) * 0.1
        stats = torch.empty(M, 2, device=DEV)
        sp.rowstats(sp.dense(rows), 1e-6, stats, M, C)
        kw = dict(stats=stats, ln_gamma=g, ln_beta=be)
        xin = F.layer_norm(rows.float(), (C,), g, be, 1e-6).view(B, H, W, C).permute(0, 3, 1, 2)

    def call(P):
        old = sp.lib().sdp_dwconv_set_kernel(kern)
        try:
            sp.dwconv(P["x"].rows, w.view(C, k * k).contiguous(), b, P["y"].rows, B, H, W, C, k, **kw)
        finally:
            sp.lib().sdp_dwconv_set_kernel(old)

    got = run_placements({"x": (C, dtype, rows), "y": (C, dtype, None)}, {"y"}, call, [("x",), ("y",)], M=M)
    ref = F.conv2d(xin, w, b, padding="same", groups=C).permute(0, 2, 3, 1).reshape(M, C)
    close(got["y"], ref, dtype, what="dwconv")


# -------------------------------------------------- strided kernels: a large ld, few rows
@pytest.mark.parametrize("code", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_fwd_bwd_large_ld(dtype, code):
    """act_fwd / act_bwd take (pointer, ld): five rows one group stride apart -- the last row of
    each group of a far placement, on both sides of every mark -- with z, dy, y and dz as column
    blocks of the same rows (act_bwd has one ld for its three operands)."""
    N, M = 264, GROUPS
    z = (torch.linspace(-6, 6, M * N, device=DEV).view(M, N) + 0.013).to(dtype)
    dy = rnd(M, N, seed=11, dtype=dtype)
    fm = pl.Placement.far_map(4 * N, dtype, pl.marks_for(dtype), 64, 2 if dtype == BF else 1)
    res = []
    for far in (False, True):
        if far:
            far_block(fm["total_rows"] * fm["ld"] * (2 if dtype == BF else 4))
            p = pl.Placement(M, 4 * N, dtype, DEV, 1, fm["gstride"], pl.OFF + 63, fm["ld"], fm["total_rows"],
                             pl.marks_for(dtype))
            assert p.crossed() == list(p.marks)
            _CROSSED.append(("z|dy|y|dz", str(dtype).split(".")[-1], p.marks))
        else:
            p = pl.Placement(M, 4 * N, dtype, DEV, 1, 69, pl.OFF + 63, fm["ld"], 4 * 69 + pl.OFF + 64 + pl.TAIL)
        p.t[p.prow, :N] = z
        p.t[p.prow, N:2 * N] = dy
        col = lambda k: p.t[p.off, k * N:]   # noqa: E731
        ld = p.gstride * p.ld
        sp.act_fwd(col(0), col(2), M, N, code, ldz=ld, ldy=ld)
        sp.act_bwd(col(0), col(1), col(3), M, N, code, ld=ld)
        torch.cuda.synchronize()
        p.check(f"act far={far}", written=True)
        g = p.gather().clone()
        assert torch.equal(g[:, :N], z) and torch.equal(g[:, N:2 * N], dy), "inputs changed"
        res.append(g[:, 2 * N:])
        del p
        torch.cuda.empty_cache()
    assert torch.equal(res[0], res[1])
    zr = z.float().clone().requires_grad_(True)
    yr = ACT_REF[code](zr)
    (gz,) = torch.autograd.grad(yr, zr, dy.float())
    tol = 2e-5 if dtype == F32 else 2e-2
    tclose(res[0][:, :N], yr.detach(), tol, f"act {code} fwd")
    tclose(res[0][:, N:], gz, tol, f"act {code} bwd")


# ------------------------------------------------------------------------------ attention
def _attn_far(dtype, N, kern, norm, mask=False):
    """A dense QKV tensor just over 4 GiB: the images across the 2^31- and 2^32-byte marks, their
    neighbours and the last one hold data, every other image the NaN sentinel (an image's output
    depends on nothing outside it: test_attention_images_isolated).  Those images equal, bit for
    bit, the same images run as a batch of their own, and attn_ref."""
    H, hd = 8, 96
    C = H * hd
    es = 2 if dtype == BF else 4
    img = N * 3 * C * es
    B = (1 << 32) // img + 4
    need(B * N * 4 * C * es + GIB)
    marks = [1 << 31, 1 << 32]
    sel = sorted({b for mk in marks for b in (mk // img - 1, mk // img, mk // img + 1)} | {0, B - 1})
    assert all((b * img < mk < (b + 1) * img) for mk, b in zip(marks, (mk // img for mk in marks)))
    itype, sent = pl.SENTINEL[dtype]
    qkv = torch.full((B * N, 3 * C), sent, dtype=itype, device=DEV).view(dtype)
    out = torch.full((B * N, C), sent, dtype=itype, device=DEV).view(dtype)
    data = rnd(len(sel) * N, 3 * C, dtype=dtype, seed=40, scale=2.0 if norm else 1.0)
    qv = qkv.view(B, N, 3 * C)
    qv[sel] = data.view(len(sel), N, 3 * C)
    qk = tuple(rnd(hd, seed=s) * 0.1 + (1 if s % 2 == 0 else 0) for s in (45, 46, 47, 48)) if norm else None
    add = None
    if mask:
        add = torch.zeros(1, 1, N, N, device=DEV)
        add[0, 0, :, N - 30:] = float("-inf")
        add[0, 0, : N // 2] += rnd(N // 2, N, seed=42)
    small_in = data.clone()
    o1 = torch.empty(len(sel) * N, C, dtype=dtype, device=DEV)
    old = sp.lib().sdp_attention_set_kernel(kern)
    try:
        v = sp.attention_variant(dtype, N, H, hd, mask)
        _CROSSED.append((f"qkv (attention variant {v})", str(dtype).split(".")[-1], tuple(marks)))
        sp.attention(qkv, out, B, N, H, hd, add, 0, 0, qk_norm=qk, eps=1e-5)
        sp.attention(small_in, o1, len(sel), N, H, hd, add, 0, 0, qk_norm=qk, eps=1e-5)
    finally:
        sp.lib().sdp_attention_set_kernel(old)
    torch.cuda.synchronize()
    got = out.view(B, N, C)[sel].reshape(len(sel) * N, C)
    assert torch.equal(got, o1), f"variant {v}: images across the marks differ from a batch of their own"
    if v != 0:   # (the generic kernel applies the head norms in place on qkv)
        assert torch.equal(qv[sel].reshape(-1, 3 * C), data), "qkv changed"
    ref_in = data.float().clone()
    if norm:
        ref_in[:, :C] = F.layer_norm(ref_in[:, :C].view(-1, H, hd), (hd,), qk[0], qk[1]).view(-1, C)
        ref_in[:, C:2 * C] = F.layer_norm(ref_in[:, C:2 * C].view(-1, H, hd), (hd,), qk[2], qk[3]).view(-1, C)
    ref = attn_ref(ref_in.to(dtype), len(sel), N, H, hd, add)
    return v, got, ref


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("N", [200, 260])
@pytest.mark.parametrize("kern", [3, 4, 5])
def test_attention_bf16_tiers(kern, N, norm):
    v, got, ref = _attn_far(BF, N, kern, norm)
    assert v == {3: 3, 5: 5}.get(kern, 4 if N <= 256 else 3)   # tier 4 holds one image's K / V up to N = 256
    close(got, ref, BF, rel=2e-2 if norm else None, what=f"attention variant {v} N {N}")


@pytest.mark.parametrize("dtype,mask", [(F32, False), (BF, True)])
def test_attention_generic(dtype, mask):
    v, got, ref = _attn_far(dtype, 200, 0, True, mask)
    assert v == 0
    close(got, ref, dtype, rel=2e-5 if dtype == F32 else 2e-2, what="generic attention")


def test_attention_refuses_qkv_rows_past_32_bit_offsets():
    """The MFMA tiers keep an image's K / V byte offsets in 32 bits: N * ld_qkv * 2 >= 2^32 is
    refused on the host, before any launch (pointers into a real small allocation)."""
    N, H, hd = 200, 8, 96
    C = H * hd
    qkv = rnd(N, 3 * C, dtype=BF, seed=1)
    out = torch.zeros(N, C, dtype=BF, device=DEV)
    ld = ((1 << 32) // (208 * 2) + 8) // 8 * 8
    assert sp.attention_variant(BF, N, H, hd) == 4
    rc = sp.lib().sdp_attention(sp.BF16, qkv.data_ptr(), ld, out.data_ptr(), C, 1, N, H, hd, None, None, None, None,
                                1e-5, None, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 1   # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert not out.any()
    sp.attention(qkv, out, 1, N, H, hd)
    close(out, attn_ref(qkv, 1, N, H, hd), BF, what="attention after the refusal")


# ------------------------------------------------------------- training kernels, row maps
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_bwd(dtype):
    M, C = M_ROWS, 768
    x, g, _ = _ln_data(M, C, dtype)
    dy, add = rnd(M, C, seed=17, dtype=dtype), rnd(M, C, seed=18, dtype=dtype)
    st = torch.empty(M, 2, device=DEV)
    sp.rowstats(sp.dense(x), 1e-6, st, M, C)

    def call(P):
        dg, db = sp.ln_bwd(P["x"].rows, st, g, P["dy"].rows, P["dx"].rows, M, C, add=P["add"].rows)
        return {"dg": dg, "db": db}

    spec = {"x": (C, dtype, x), "dy": (C, dtype, dy), "add": (C, dtype, add), "dx": (C, dtype, None)}
    got = run_placements(spec, {"dx"}, call, [("x",), ("dy",), ("add",), ("dx",), ("add=dx", "dx")], M=M)
    xr = x.float().clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = torch.zeros(C, device=DEV, requires_grad=True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(xr, (C,), gr, br, 1e-6), (xr, gr, br), dy.float())
    tol = 2e-5 if dtype == F32 else 2e-2
    tclose(got["dx"], gx + add.float(), tol * 4, "ln dx")
    tclose(got["dg"], gg, tol * 4, "ln dgamma")
    tclose(got["db"], gb, tol * 4, "ln dbeta")


def test_ln_bwd_fused(monkeypatch):
    """sdp_ln_bwd_fused (fp32 stream, bf16 gradient, the branch gradient emitted in the same launch):
    far as near, and -- as its own test asserts -- bit-identical to the separate passes."""
    M, C = GROUPS * 64, 768
    x, g, _ = _ln_data(M, C, F32)
    da, add, z = rnd(M, C, seed=53, dtype=BF), rnd(M, C, seed=52), rnd(M, C, seed=57, dtype=BF)
    scale = torch.tensor([1.25, 0.0, 1.25, 0.5, 1.0], device=DEV)
    st = torch.empty(M, 2, device=DEV)
    sp.rowstats(sp.dense(x), 1e-6, st, M, C)

    def call(P):
        o2 = torch.empty(M, C, device=DEV, dtype=BF)
        dg, db = sp.ln_bwd(P["x"].rows, st, g, P["da"].rows, P["dx"].rows, M, C, add=P["add"].rows,
                           emit=dict(scale=scale, sgrp=64, z=z, act=1, out=o2))
        return {"dg": dg, "db": db, "o2": o2}

    spec = {"x": (C, F32, x), "da": (C, BF, da), "add": (C, F32, add), "dx": (C, F32, None)}
    monkeypatch.setattr(sp, "_LN_BWD_FUSED", True)
    got = run_placements(spec, {"dx"}, call, [("x",), ("da",), ("add",), ("dx",)], M=M)
    monkeypatch.setattr(sp, "_LN_BWD_FUSED", False)
    dx, o2 = torch.empty(M, C, device=DEV), torch.empty(M, C, device=DEV, dtype=BF)
    dg, db = sp.ln_bwd(sp.dense(x), st, g, sp.dense(da), sp.dense(dx), M, C, add=sp.dense(add),
                       emit=dict(scale=scale, sgrp=64, z=z, act=1, out=o2))
    assert torch.equal(got["dx"], dx) and torch.equal(got["o2"], o2)
    tclose(got["dg"], dg, 1e-5, "dgamma")
    tclose(got["db"], db, 1e-5, "dbeta")
    tclose(got["db"], da.float().sum(0), 1e-4, "dbeta vs torch")


@pytest.mark.parametrize("xdt,ydt,adt,act,p", [(BF, F32, BF, 1, 0.0), (BF, BF, BF, 0, 0.2), (F32, F32, F32, 0, 0.0)])
def test_add_ln_fwd(xdt, ydt, adt, act, p):
    M, C = GROUPS * 64, 768
    z = rnd(M, C, seed=71, dtype=xdt)
    tok = rnd(M, C, seed=72, dtype=ydt, scale=2.0) + 0.5
    g, b = rnd(C, seed=73) * 0.2 + 1, rnd(C, seed=74) * 0.2
    scale = torch.tensor([1.25, 0.0, 1.25, 0.5, 1.0], device=DEV)
    kw = dict(scale=scale, sgrp=64, act=act, p=p, seed=1234, dmode=1 if p > 0 else 0)

    def call(P):
        st = torch.full((M, 2), float("nan"), device=DEV)
        assert sp.add_ln_fwd(P["z"].rows, P["y"].rows, P["a"].rows, M, C, P["r"].rows, 1e-5, g, b, st, **kw)
        return {"st": st}

    spec = {"z": (C, xdt, z), "y": (C, ydt, None), "a": (C, adt, None), "r": (C, ydt, tok)}
    got = run_placements(spec, {"y", "a"}, call, [("z",), ("y",), ("a",), ("r",), ("r=y", "y")], M=M)
    y = torch.empty(M, C, dtype=ydt, device=DEV)
    a = torch.empty(M, C, dtype=adt, device=DEV)
    st = torch.empty(M, 2, device=DEV)
    sp.rowscale_add(sp.dense(z), sp.dense(y), M, C, resid=sp.dense(tok), **kw)
    sp.ln_fwd(sp.dense(y), 1e-5, g, b, st, sp.dense(a), M, C)
    assert torch.equal(got["y"], y) and torch.equal(got["a"], a) and torch.equal(got["st"], st)
    tclose(got["a"], F.layer_norm(y.float(), (C,), g, b, 1e-5), 1e-2 if adt == BF else 1e-5, "add_ln_fwd LN")


@pytest.mark.parametrize("dtype,C", [(F32, 64), (BF, 96)])
def test_dw_wgrad(dtype, C):
    B, H, W, k = GROUPS, 8, 8, 7
    M = B * H * W
    a, dy = rnd(M, C, seed=22, dtype=dtype), rnd(M, C, seed=23, dtype=dtype)

    def call(P):
        return {"dw": sp.dw_wgrad(P["a"].rows, P["dy"].rows, B, H, W, C, k)}

    got = run_placements({"a": (C, dtype, a), "dy": (C, dtype, dy)}, set(), call, [("a",), ("dy",)], M=M)
    an = a.float().view(B, H, W, C).permute(0, 3, 1, 2)
    w = torch.zeros(C, 1, k, k, device=DEV, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(an, w, padding="same", groups=C), w,
                                dy.float().view(B, H, W, C).permute(0, 3, 1, 2))
    tclose(got["dw"], gw.view(C, k * k), 1e-4 if dtype == F32 else 2e-2, "dw wgrad")


def test_gemm_train_epi_dense_past_4gib():
    """sdp_gemm_train_epi takes dense rows only: operands just over 4 GiB, p = 0.  The rows across
    the 2^31- and 2^32-byte marks and the last ones equal the same rows run on their own through
    the fast GEMM + sdp_act_fwd / sdp_act_bwd (what its own test asserts bit for bit)."""
    N, K, K2, code = 768, 768, 256, 1
    M = (1 << 32) // (2 * N) + 300
    need(14 * GIB)
    marks = [1 << 31, 1 << 32]
    _CROSSED.append(("x,z,h,dz", "bfloat16", tuple(marks)))
    x = torch.empty(M, K, dtype=BF, device=DEV).normal_()
    w, b = rnd(N, K, seed=2, dtype=BF, scale=0.05), rnd(N, seed=3, scale=0.1)
    z = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    h = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    assert sp.gemm_train_epi(1, x, w, z, M, N, K, bias=b, y2=h, act=code)
    sl = [slice(mk // (2 * N) - 150, mk // (2 * N) + 150) for mk in marks] + [slice(0, 300), slice(M - 300, M)]
    for s in sl:
        xs = x[s].clone()
        zr, hr = torch.empty(300, N, dtype=BF, device=DEV), torch.empty(300, N, dtype=BF, device=DEV)
        sp.gemm(sp.dense(xs), w, sp.dense(zr), 300, N, K, bias=b)
        sp.act_fwd(zr, hr, 300, N, code)
        assert torch.equal(z[s], zr) and torch.equal(h[s], hr), f"mode 1 rows {s}"
        close(zr, xs.float() @ w.float().t() + b, BF, what="mode 1 z")
    del x, h
    torch.cuda.empty_cache()
    dy = torch.empty(M, K2, dtype=BF, device=DEV).normal_()
    wt = rnd(N, K2, seed=5, dtype=BF, scale=0.05)
    dz = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    assert sp.gemm_train_epi(2, dy, wt, dz, M, N, K2, z=z, act=code)
    for s in sl:
        dh, ref = torch.empty(300, N, dtype=BF, device=DEV), torch.empty(300, N, dtype=BF, device=DEV)
        sp.gemm(sp.dense(dy[s].clone()), wt, sp.dense(dh), 300, N, K2)
        sp.act_bwd(z[s].clone(), dh, ref, 300, N, code)
        assert torch.equal(dz[s], ref), f"mode 2 rows {s}"
    assert torch.isfinite(dz[-1].float()).all()


# ------------------------------------------- strided kernels on rows one group stride apart
def sparse(name, C, dtype, far, data=None, M=GROUPS):
    """M rows, one per group of the far map (the last row of each group: both sides of every mark),
    as a placement with groups of one row; .view() is the strided tensor the bindings take."""
    fm = pl.Placement.far_map(C, dtype, pl.marks_for(dtype), 64, 2 if dtype == BF else 1)
    if far:
        far_block(fm["total_rows"] * fm["ld"] * (2 if dtype == BF else 4))
        p = pl.Placement(M, C, dtype, DEV, 1, fm["gstride"], pl.OFF + 63, fm["ld"], fm["total_rows"], pl.marks_for(dtype))
        assert p.crossed() == list(p.marks)
        _CROSSED.append((name, str(dtype).split(".")[-1], p.marks))
    else:
        p = pl.Placement(M, C, dtype, DEV, 1, 69, pl.OFF + 63, fm["ld"], (M - 1) * 69 + pl.OFF + 64 + pl.TAIL)
    if data is not None:
        p.scatter(data)
    return p


def run_sparse(spec, outs, call, configs, cmp=None):
    """run_placements for the strided form: spec name -> (C, dtype, data)."""
    base = None
    for far in [()] + list(configs):
        P = {n: sparse(n, C, dt, n in far, d) for n, (C, dt, d) in spec.items()}
        extra = call(P) or {}
        torch.cuda.synchronize()
        got = dict(extra)
        for n, p in P.items():
            p.check(f"{n} [far {far}]", written=n in outs)
            if n in outs:
                got[n] = p.gather().clone()
            else:
                assert torch.equal(p.gather(), spec[n][2]), f"input {n} changed"
        if base is None:
            base = got
        else:
            for n, v in got.items():
                if cmp and n in cmp:
                    cmp[n](v, base[n], f"{n} [far {far}] vs near")
                else:
                    assert torch.equal(v, base[n]), f"{n} [far {far}] differs from the near placement"
        del P, p, extra, got
    return base


@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_qk_headnorm_seg_colsum(dtype):
    H, hd = 8, 96
    C = H * hd
    qkv = rnd(GROUPS, 3 * C, dtype=dtype, seed=24, scale=2.0)
    gq, bq, gk, bk = (rnd(hd, seed=s) * 0.1 + (1 if s % 2 == 0 else 0) for s in (25, 26, 27, 28))

    def call(P):
        x = P["x"].view()
        out = torch.empty(1, 3 * C, device=DEV)
        sp.seg_colsum(x, out, 1, GROUPS, 0, 1, 3 * C, ldx=x.stride(0))
        res = {"t": sp.transpose(x), "sum": out}
        P["n"].scatter(qkv)
        sp.qk_headnorm(P["n"].view(), GROUPS, H, hd, gq, bq, gk, bk, 1e-5)
        return res

    got = run_sparse({"x": (3 * C, dtype, qkv), "n": (3 * C, dtype, None)}, {"n"}, call, [("x",), ("n",)])
    assert torch.equal(got["t"], qkv.t().contiguous())
    tclose(got["sum"], qkv.float().sum(0, keepdim=True), 1e-5, "seg_colsum")
    ref = qkv.float().clone()
    ref[:, :C] = F.layer_norm(ref[:, :C].view(-1, H, hd), (hd,), gq, bq).view(-1, C)
    ref[:, C:2 * C] = F.layer_norm(ref[:, C:2 * C].view(-1, H, hd), (hd,), gk, bk).view(-1, C)
    close(got["n"], ref, dtype, what="qk headnorm")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_loss_and_softmax(dtype):
    B, K, eps = GROUPS, 1000, 0.1
    logits = rnd(B, K, seed=24, dtype=dtype, scale=3)
    labels = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    N, Npad, scale = 260, 264, 1 / 96 ** 0.5
    S = rnd(B, Npad, seed=19, scale=4)
    dP = rnd(B, Npad, seed=20, dtype=dtype)
    L = sp.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def call(P):
        loss = torch.zeros(1, device=DEV)
        sp.ce_loss(P["logits"].view(), labels, eps, 8.0, P["d"].view(), loss)
        s, p_, dp, ds = (P[n] for n in ("S", "P", "dP", "dS"))
        ld = lambda q: q.gstride * q.ld   # noqa: E731
        ptr = lambda q: q.view().data_ptr()   # noqa: E731
        rc = L.sdp_softmax_fwd(sp.dcode(dtype), ptr(s), ld(s), ptr(p_), None, ld(p_), B, N, Npad, scale, 0.0, 0, stream)
        assert rc == 0
        rc = L.sdp_softmax_bwd(sp.dcode(dtype), ptr(p_), ld(p_), ptr(dp), ld(dp), ptr(ds), ld(ds), B, N, Npad, 0.0, 0,
                               stream)
        assert rc == 0
        return {"loss": loss}

    spec = {"logits": (K, dtype, logits), "d": (K, dtype, None), "S": (Npad, F32, S), "P": (Npad, dtype, None),
            "dP": (Npad, dtype, dP), "dS": (Npad, dtype, None)}
    # the loss is summed over the rows by atomic adds, in no fixed order: its own test's 1e-5
    got = run_sparse(spec, {"d", "P", "dS"}, call, [("logits",), ("d",), ("S",), ("P",), ("dP",), ("dS",)],
                     cmp={"loss": lambda a, b, what: tclose(a, b, 1e-5, what)})
    lr = logits.float().clone().requires_grad_(True)
    ref = F.cross_entropy(lr, labels, label_smoothing=eps)
    (g,) = torch.autograd.grad(ref * 8.0, lr)
    tclose(got["loss"], ref.detach().view(1), 1e-5, "ce loss")
    tclose(got["d"], g, 1e-5 if dtype == F32 else 2e-2, "ce dlogits")
    Sr = S[:, :N].clone().requires_grad_(True)
    Pr = torch.softmax(Sr * scale, -1)
    tclose(got["P"][:, :N], Pr.detach(), 2e-6 if dtype == F32 else 1e-2, "softmax")
    assert (got["P"][:, N:] == 0).all()
    (gS,) = torch.autograd.grad(Pr, Sr, dP[:, :N].float())
    tclose(got["dS"][:, :N] * scale, gS, 1e-5 if dtype == F32 else 2e-2, "softmax bwd")


def test_gemm_wgrad_far_token_rows():
    N, K, M = 256, 512, GROUPS
    dy, x = rnd(M, N, seed=31, dtype=BF, scale=0.5), rnd(M, K, seed=32, dtype=BF)

    def call(P):
        out = torch.full((1, N, K), float("nan"), device=DEV)
        sp.gemm_wgrad(P["dy"].view(), P["x"].view(), out, M, 1, split_stride=N * K)
        return {"dw": out}

    got = run_sparse({"dy": (N, BF, dy), "x": (K, BF, x)}, set(), call, [("dy",), ("x",)])
    tclose(got["dw"][0], dy.float().t() @ x.float(), 1e-5, "wgrad")


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_flex_batched_over_groups(dtype, ta, tb):
    """Batch z = group z of a placement (batch stride gstride * ld): all four transposes, A, B or C far."""
    Z, G = GROUPS, 64
    Ca = 64
    Cb = 64 if tb else 40
    M, K = (Ca, G) if ta else (G, Ca)
    N = G if tb else Cb
    assert (K == G or not tb) and (M == G)
    A, B = rnd(Z * G, Ca, seed=1, dtype=dtype), rnd(Z * G, Cb, seed=2, dtype=dtype)

    def call(P):
        a, b, c = P["A"], P["B"], P["C"]
        sp.gemm_flex(a.t, b.t, c.t, M, N, K, ta=bool(ta), tb=bool(tb), lda=a.ld, ldb=b.ld, ldc=c.ld, Z=Z, zdiv=1,
                     sa=(a.gstride * a.ld, 0), sb=(b.gstride * b.ld, 0), sc=(c.gstride * c.ld, 0), alpha=0.5,
                     a_off=a.off * a.ld, b_off=b.off * b.ld, c_off=c.off * c.ld)

    spec = {"A": (Ca, dtype, A), "B": (Cb, dtype, B), "C": (N, F32, None)}
    got = run_placements(spec, {"C"}, call, [("A",), ("B",), ("C",)])
    Af, Bf = A.float().view(Z, G, Ca), B.float().view(Z, G, Cb)
    ref = 0.5 * (Af.transpose(1, 2) if ta else Af) @ (Bf.transpose(1, 2) if tb else Bf)
    tclose(got["C"], ref.reshape(Z * G, N), 1e-5 if dtype == F32 else 2e-2, f"flex ta={ta} tb={tb}")


# --------------------------------------------------------------- flash training attention
@pytest.mark.parametrize("N", [200, 260])
def test_attn_train_past_4gib(N):
    """attn_train_fwd / attn_train_bwd on a QKV (and dQKV) tensor just over 4 GiB: the images across
    the marks and the last one equal the same images as a batch of their own, and torch autograd."""
    import math
    H, hd, p, seed = 8, 96, 0.0, 99
    C = H * hd
    img = N * 3 * C * 2
    B = (1 << 32) // img + 4
    need(15 * GIB)
    marks = [1 << 31, 1 << 32]
    sel = sorted({b for mk in marks for b in (mk // img, mk // img + 1)} | {0, B - 1})
    _CROSSED.append(("qkv,dqkv", "bfloat16", tuple(marks)))
    assert sp.attn_train_applies(BF, N, hd)
    scale = 1.0 / math.sqrt(hd)
    qkv = torch.empty(B * N, 3 * C, dtype=BF, device=DEV).normal_()
    do = torch.empty(B * N, C, dtype=BF, device=DEV).normal_()
    o = torch.full((B * N, C), float("nan"), dtype=BF, device=DEV)
    lse = torch.empty(B * H * N, device=DEV)
    delta = torch.empty(B * H * N, device=DEV)
    dqkv = torch.full((B * N, 3 * C), float("nan"), dtype=BF, device=DEV)
    sp.attn_train_fwd(qkv, o, lse, B, N, H, hd, scale, p, seed)
    sp.attn_train_bwd(qkv, o, do, lse, delta, (dqkv, 0), (dqkv, C), (dqkv, 2 * C), B, N, H, hd, scale, p, seed)
    n = len(sel)
    pick = lambda t, w: t.view(B, N, w)[sel].reshape(n * N, w)   # noqa: E731
    q1, do1 = pick(qkv, 3 * C).clone(), pick(do, C).clone()
    o1 = torch.empty(n * N, C, dtype=BF, device=DEV)
    lse1, delta1 = torch.empty(n * H * N, device=DEV), torch.empty(n * H * N, device=DEV)
    d1 = torch.full((n * N, 3 * C), float("nan"), dtype=BF, device=DEV)
    sp.attn_train_fwd(q1, o1, lse1, n, N, H, hd, scale, p, seed)
    sp.attn_train_bwd(q1, o1, do1, lse1, delta1, (d1, 0), (d1, C), (d1, 2 * C), n, N, H, hd, scale, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(pick(o, C), o1), "O differs from a batch of the same images"
    assert torch.equal(lse.view(B, H * N)[sel].reshape(-1), lse1), "lse differs"
    assert torch.equal(pick(dqkv, 3 * C), d1), "dQKV differs from a batch of the same images"
    x = q1.float().view(n, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = (t.clone().requires_grad_(True) for t in x)
    s = q @ k.transpose(-1, -2) * scale
    ref_o = torch.softmax(s, -1) @ v
    ref_o.backward(do1.float().view(n, N, H, hd).permute(0, 2, 1, 3))
    tclose(o1.float().view(n, N, H, hd).permute(0, 2, 1, 3), ref_o.detach(), 1e-2, "O")
    tclose(lse1.view(n, H, N), torch.logsumexp(s.detach(), -1) / math.log(2.0), 1e-4, "lse")
    g = d1.float().view(n, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    tclose(g[2], v.grad, 2e-2, "dV")
    gs = max(1.0, float(v.grad.abs().max()))
    for got, ref, what in ((g[0], q.grad, "dQ"), (g[1], k.grad, "dK")):
        err = float((got - ref).abs().max())
        assert err <= 2e-2 * max(gs, float(ref.abs().max())), f"{what}: {err:.3e} (scale {gs:.3e})"


# ---------------------------------------------------------------------------- whole model
def test_model_xl_geometry_hidden_and_qkv_past_4gib():
    """XL geometry (d 768, patch 14, 256 patches + registers), 2 blocks, bf16 eval, at a batch whose
    FFN hidden buffer (5.8 GB) and QKV buffer (4.3 GB) both cross 4 GiB: the logits equal,
    bit for bit, the same images run in shards of 256 (as test_config4_... does at 2 GiB), and a few
    images are within the bf16 tolerance of test_gpu_model.py (1e-2) of the CPU oracle."""
    import model as ours
    import sdpnet_oracle as orc
    import synth
    need(15 * GIB)
    cfg = synth.canonical("XL", num_blocks=2)
    B = 3640
    assert B * 259 * 3 * 768 * 2 > 1 << 32   # the QKV rows of 256 patches + 3 registers per image
    _CROSSED.append(("ffn hidden, qkv", "bfloat16", (1 << 31, 1 << 32)))
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    sd = synth.synth_state_dict(m, 231424314)
    m.load_state_dict(sd)
    m = m.to(DEV).eval().to(BF)
    x = torch.empty(B, 3, 224, 224, dtype=BF, device=DEV).normal_()
    # the forward's live buffers peak below 8 GiB, but the caching allocator would keep every freed
    # one (17 GiB reserved): cap the process at 16 GiB for this test, so that it releases them instead
    total = torch.cuda.get_device_properties(0).total_memory
    torch.cuda.set_per_process_memory_fraction(min(1.0, 16 * GIB / total))
    try:
        with torch.no_grad():
            y = m(x)
            assert y.shape == (B, 1000) and torch.isfinite(y.float()).all()
            for lo in range(0, B, 256):
                assert torch.equal(m(x[lo:lo + 256]), y[lo:lo + 256]), f"shard at {lo} differs from the whole batch"
    finally:
        torch.cuda.set_per_process_memory_fraction(1.0)
    pick = [0, 1792, B - 1]
    ref = orc.forward(x[pick].float().cpu(), sd, cfg)
    err = (y[pick].float().cpu() - ref).abs().max().item()
    assert err <= 1e-2, f"bf16 logits max abs err {err:.3e} against the oracle"
