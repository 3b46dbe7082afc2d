"""CPU: the MX quantiser of tests/mx_oracle.py against the format's own properties (include/
sdpnet_hip.h, "MX operand format"), and the host-side surface of the MXFP8 path: the pure
``mx_applies``, the switch, and the C entry points' argument checks (no kernel is launched).

One property differs from a naive reading of the format: a block whose largest element rounds
*down* to 224 2^e (scaled maximum in (224, 232]) decodes to a maximum with m = 1.75 exactly, for
which the scale rule picks e - 1.  Re-quantising such a block stores the same values under a scale
one step lower (448 2^(e-1)), so "same bytes" holds for every other block and "same values" for all.
"""
import pytest
import torch

import mx_oracle as mo
import sdpnet_hip as sp

HIP_INVALID = 1


def blocks(seed, n=2048):
    """Rows of 32 with row scales spread over 2^+-46 (fp32-exact)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 32, generator=g, dtype=torch.float64)
            * torch.exp2(torch.randint(-46, 47, (n, 1), generator=g).double())).float()


def test_scaled_block_maximum_and_no_saturation():
    x = blocks(1)
    q, s = mo.encode(x)
    y = x.double() * torch.exp2(127.0 - s.double())          # the scaled values, before rounding
    top = y.abs().amax(-1)
    assert (top > 224).all() and (top <= 448).all()
    mag = mo.decode(q, torch.full_like(s, 127)).abs()        # the bytes' own magnitudes
    assert torch.isfinite(mag).all() and (mag <= 448).all()
    assert (mag.amax(-1) >= 224).all()


def test_decoded_normals_within_half_a_step():
    x = blocks(2)
    q, s = mo.encode(x)
    d = mo.decode(q, s)
    normal = ((q & 0x78) != 0)
    rel = ((d - x.double()).abs() / x.double().abs())[normal]
    assert float(rel.max()) <= 2.0 ** -4
    sub = ~normal
    assert ((d - x.double()).abs()[sub] <= 2.0 ** -10 * torch.exp2(s.double() - 127.0).expand_as(d)[sub]).all()


def test_requantising_decoded_values():
    x = blocks(3)
    q, s = mo.encode(x)
    d = mo.decode(q, s)
    q2, s2 = mo.encode(d.float())
    assert torch.equal(mo.decode(q2, s2), d)                 # the values: every block
    top224 = ((q & 0x7F).amax(-1, keepdim=True) == 0x76)     # largest byte is 224 (module docstring)
    assert torch.equal(s2[~top224], s[~top224])
    assert torch.equal(q2[~top224.expand_as(q)], q[~top224.expand_as(q)])
    assert (s2[top224].int() == s[top224].int() - 1).all() and bool(top224.any())


def test_elements_agree_with_torch_float8_cast():
    """torch's CPU float8_e4m3fn cast rounds to nearest even (1.0625 -> 1.0, 1.1875 -> 1.25)."""
    assert torch.tensor([1.0625, 1.1875]).to(torch.float8_e4m3fn).float().tolist() == [1.0, 1.25]
    g = torch.Generator().manual_seed(4)
    y = torch.cat([torch.randn(50000, generator=g) * 60, torch.randn(50000, generator=g) * 0.02,
                   torch.arange(-448, 449).float() / 512, torch.tensor([0.0, -0.0, 448.0, -448.0, 2.0 ** -10])])
    y = y.clamp(-448, 448)
    assert torch.equal(mo.e4m3_bytes(y.double()).to(torch.uint8), y.to(torch.float8_e4m3fn).view(torch.uint8))


def test_zero_tiny_and_nonfinite_blocks():
    z = torch.zeros(2, 64)
    z[1, 3] = -0.0
    q, s = mo.encode(z)
    assert (s == 127).all() and q[0].eq(0).all() and int(q[1, 3]) == 0x80 and (mo.decode(q, s) == 0).all()
    tiny = torch.full((1, 32), 2.0 ** -140)                  # fp32 subnormals: the code clamps at 0
    tiny[0, 1] = 3 * 2.0 ** -136
    q, s = mo.encode(tiny)
    assert int(s[0, 0]) == 0
    assert torch.equal(mo.decode(q, s), torch.round(tiny.double() * 2.0 ** 136) * 2.0 ** -136)
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = blocks(5, 4).view(2, 64)
        x[0, 40] = bad
        q, s = mo.encode(x)
        assert q[0, 32:].eq(mo.NAN_BYTE).all() and int(s[0, 1]) == 127
        d = mo.decode(q, s)
        assert torch.isnan(d[0, 32:]).all() and torch.isfinite(d[0, :32]).all() and torch.isfinite(d[1]).all()
        assert torch.equal(q[1], mo.encode(x[1:])[0][0])


def test_threshold_is_m_1_75():
    t = torch.tensor(1.75)
    up, dn = torch.nextafter(t, torch.tensor(2.0)), torch.nextafter(t, torch.tensor(0.0))
    for ex in (-20, 0, 30):
        x = torch.zeros(3, 32)
        x[:, 0] = torch.stack([dn, t, up]) * 2.0 ** ex
        _, s = mo.encode(x)
        assert s.view(-1).tolist() == [ex - 8 + 127, ex - 8 + 127, ex - 7 + 127]


def test_truncation_is_visible_to_the_oracle():
    """The faulty variant the model criterion must reject: rms error 2x the nearest-even one."""
    x = blocks(6)
    r = (mo.fake_quant(x) - x.double()).pow(2).mean().sqrt()
    t = (mo.fake_quant(x, "trunc") - x.double()).pow(2).mean().sqrt()
    assert 1.8 <= float(t / r) <= 2.2


# ----------------------------------------------------------------------------- host surface
@pytest.mark.parametrize("M,N,K,ok", [(1, 32, 128, True), (50176, 3072, 768, True), (197, 768, 3072, True),
                                      (0, 64, 128, False), (4, 48, 128, False), (4, 64, 64, False),
                                      (4, 64, 192, False), (4, 96, 384, True), (4, 16, 128, False)])
def test_mx_applies_is_pure_and_equals_the_library(M, N, K, ok):
    for out_mx in (False, True):
        assert sp.mx_applies(M, N, K, out_mx) is ok
        assert bool(sp.lib().sdp_gemm_mx_applies(M, N, K, int(out_mx))) is ok


def test_switch_and_context_manager():
    assert sp.mx_fp8_enabled() is False
    with sp.mx_fp8():
        assert sp.mx_fp8_enabled() is True
        with sp.mx_fp8(False):
            assert sp.mx_fp8_enabled() is False
        assert sp.mx_fp8_enabled() is True
    assert sp.mx_fp8_enabled() is False
    assert sp.set_mx_fp8(True) is False and sp.set_mx_fp8(False) is True


def test_entry_points_refuse_invalid_arguments_before_launch():
    L = sp.lib()
    p = 4096  # any aligned non-null address: nothing is dereferenced on a refusal
    assert L.sdp_mx_quant_rows(1, None, 128, 0, 0, 0, None, p, 128, p, 4, 4, 128, None) == HIP_INVALID
    assert L.sdp_mx_quant_rows(1, p, 192, 0, 0, 0, None, p, 192, p, 8, 4, 192, None) == HIP_INVALID   # K % 128
    assert L.sdp_mx_quant_rows(2, p, 128, 0, 0, 0, None, p, 128, p, 4, 4, 128, None) == HIP_INVALID   # dtype
    assert L.sdp_mx_quant_rows(1, p, 128, 0, 0, 0, None, p, 128, p, 4, 0, 128, None) == 0             # M = 0

    def gemm(xs=p, ws=p, y=p, yq=None, ys=None, r=None, part=None, N=64, K=128):
        return L.sdp_gemm_mx(p, K, xs, K // 32, p, K, ws, K // 32, None, r, N, 0, 0, 0, y, N, 0, 0, 0,
                             yq, N, ys, N // 32, 4, N, K, 0, 0, part, None)
    assert gemm(xs=None) == HIP_INVALID and gemm(ws=None) == HIP_INVALID
    assert gemm(K=192) == HIP_INVALID and gemm(N=48) == HIP_INVALID
    assert gemm(y=None) == HIP_INVALID and gemm(yq=p, ys=p) == HIP_INVALID       # neither / both outputs
    assert gemm(y=None, yq=p, ys=None) == HIP_INVALID
    assert gemm(y=None, yq=p, ys=p, r=p) == HIP_INVALID and gemm(y=None, yq=p, ys=p, part=p) == HIP_INVALID
    assert gemm(part=p, N=96) == HIP_INVALID                                      # part needs whole chunks


def test_wrappers_reject_cpu_tensors():
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.mx_quant_rows(sp.dense(x), 4, 128)


# ----------------------------------------------------------------------------- routing, model criterion
def test_pair_routing_is_a_pure_function():
    assert sp.mx_pair_applies(50176, 768, 3072)
    assert sp.mx_pair_applies(1, 256, 1024)
    assert not sp.mx_pair_applies(392, 96, 384)        # embedding_dim 96: K % 128
    assert not sp.mx_pair_applies(392, 192, 768)       # K = 192
    assert not sp.mx_pair_applies(0, 256, 1024)
    # low_latency on: a pair of which gemm_split_plan takes either GEMM stays on split-K
    assert sp.gemm_split_plan(197, 1024, 256, 256) is not None
    assert not sp.mx_pair_applies(197, 256, 1024, low_latency=True, cus=256)
    assert sp.mx_pair_applies(197, 256, 1024, low_latency=False, cus=256)
    assert sp.gemm_split_plan(50176, 3072, 768, 256) is None and sp.gemm_split_plan(50176, 768, 3072, 256) is None
    assert sp.mx_pair_applies(50176, 768, 3072, low_latency=True, cus=256)


def test_model_criterion_rejects_truncating_quantisers():
    """The GPU model test asserts err_hip^2 <= (1.25 err_emul)^2 + err_bf16^2.  On s_c256_h2 a
    truncating activation quantiser and a truncating weight quantiser each raise the emulation's rms
    logit error by >= 1.5 x (measured 2.03 x and 1.88 x), so a kernel with either defect fails it."""
    import golden_util as gu
    import model as ours
    meta, _ = gu.load_case("s_c256_h2")
    torch.manual_seed(0)
    sd, x = gu.build_inputs(meta, ours.MainModel.from_dict(**meta["config"]))
    cfg, nr = meta["config"], meta["num_registers"]
    ref = mo.forward_mx(x, sd, cfg, nr, None, None)

    def rms(rx, rw):
        return float((mo.forward_mx(x, sd, cfg, nr, rx, rw) - ref).pow(2).mean().sqrt())
    good, tx, tw = rms("rne", "rne"), rms("trunc", "rne"), rms("rne", "trunc")
    print(f"MX emulation rms logit error: rne {good:.3e}  trunc activations {tx / good:.2f}x  trunc weights {tw / good:.2f}x")
    assert tx >= 1.5 * good and tw >= 1.5 * good
