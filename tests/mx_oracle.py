"""The MX (block-scaled e4m3) quantiser of include/sdpnet_hip.h, "MX operand format", in exact
fp64 / integer torch: encode to bytes, decode to fp64.

Not a restatement of the kernels' bit manipulation: the scale comes from ``torch.frexp`` of the
fp64 block maximum, the element from ``torch.round`` (half to even) of the exactly scaled fp64
value on the e4m3 grid.  Inputs are fp32-exact values (fp32 or bf16 tensors, or fp64 holding such).

``rounding="trunc"`` drops the low bits instead (the faulty variants of the self-checks).
"""
import torch

BLOCK = 32
NAN_BYTE = 0x7F
E4M3_MAX = 448.0


def _pow2(ex):
    return torch.ldexp(torch.ones_like(ex, dtype=torch.float64), ex)


def codes_of_amax(amax):
    """E8M0 codes (int64) of fp64 block maxima (finite, >= 0); monotone in amax."""
    f, x = torch.frexp(amax.double())           # amax = f 2^x, f in [0.5, 1): m = 2 f, E = x - 1
    e = torch.where(2.0 * f <= 1.75, x - 9, x - 8)
    codes = (e.long() + 127).clamp(0, 254)
    return torch.where(amax == 0, torch.full_like(codes, 127), codes)


def scale_codes(v):
    """(codes int64 [..., K/32], bad bool [..., K/32]) of fp32-exact values v [..., K]."""
    b = v.double().reshape(*v.shape[:-1], -1, BLOCK)
    bad = ~torch.isfinite(b).all(-1)
    amax = torch.where(bad[..., None], torch.zeros_like(b), b).abs().amax(-1)
    return codes_of_amax(amax), bad


def e4m3_bytes(y, rounding="rne"):
    """e4m3fn bytes (int64) of fp64 values |y| <= 448, nearest-even (or truncated) on the grid."""
    a = y.abs()
    _, x = torch.frexp(a)
    E = (x - 1).clamp_min(-6)                   # binade of a, the subnormals share the first one's grid
    step = _pow2(E - 3)
    r = torch.round(a / step) if rounding == "rne" else torch.floor(a / step)
    q = r * step                                # on the grid (may be the next binade's first value)
    assert float(q.max()) <= E4M3_MAX if q.numel() else True
    f2, x2 = torch.frexp(q)
    E2 = x2 - 1
    normal = q >= 2.0 ** -6
    mant = torch.where(normal, (2.0 * f2 - 1.0) * 8.0, q * 512.0).long()
    expf = torch.where(normal, E2 + 7, torch.zeros_like(E2)).long()
    return (torch.signbit(y).long() << 7) | (expf << 3) | mant


def encode(v, rounding="rne"):
    """(Q uint8 [..., K], S uint8 [..., K/32]) of fp32-exact v [..., K], K % 32 == 0."""
    assert v.shape[-1] % BLOCK == 0
    codes, bad = scale_codes(v)
    b = v.double().reshape(*v.shape[:-1], -1, BLOCK)
    b = torch.where(bad[..., None], torch.zeros_like(b), b)
    y = b * _pow2(127 - codes)[..., None]       # exact: a power of two
    q = e4m3_bytes(y, rounding)
    q = torch.where(bad[..., None], torch.full_like(q, NAN_BYTE), q)
    return q.reshape(v.shape).to(torch.uint8), codes.to(torch.uint8)


def decode(q, s):
    """fp64 values of bytes q [..., K] under scales s [..., K/32]."""
    b = q.long()
    expf, mant = (b >> 3) & 15, b & 7
    mag = torch.where(expf == 0, mant.double() * 2.0 ** -9, (1.0 + mant.double() / 8.0) * _pow2(expf - 7))
    mag = torch.where((b & 0x7F) == NAN_BYTE, torch.full_like(mag, float("nan")), mag)
    val = torch.where((b & 0x80) != 0, -mag, mag)
    sc = _pow2(s.long() - 127)
    return (val.reshape(*q.shape[:-1], -1, BLOCK) * sc[..., None]).reshape(q.shape)


def fake_quant(v, rounding="rne"):
    """decode(encode(v)): the fp64 values an MX operand made from v holds."""
    return decode(*encode(v, rounding))


def e4m3_spacing(mag64, s):
    """Spacing of the e4m3 grid at magnitudes mag64 [..., K] under the scales s [..., K/32] (fp64)."""
    sc = _pow2(s.long() - 127)
    a = mag64.double().abs().reshape(*mag64.shape[:-1], -1, BLOCK) / sc[..., None]
    _, x = torch.frexp(a)
    return (_pow2((x - 1).clamp(-6, 8) - 3) * sc[..., None]).reshape(mag64.shape)


# --------------------------------------------------------------------------- fp64 MX forward
def _mlp_mx(t, gamma, beta, eps, w1, b1, w2, b2, act, rx, rw):
    """down(act(up(LN(t)))) of token rows t [..., C] (fp64) with the MX path's quantisation points:
    the LayerNorm without affine, W1 * gamma, the hidden activations and W2 (include/sdpnet_hip.h,
    layers.py _mlp_mx); everything else exact.  rx / rw: rounding of activations / weights."""
    import sdpnet_oracle as orc
    mean = t.mean(-1, keepdim=True)
    var = t.var(-1, unbiased=False, keepdim=True)
    xq = fake_quant(((t - mean) / torch.sqrt(var + eps)).float(), rx)
    w1q = fake_quant((w1.double() * gamma.double()).float(), rw)
    c = w1.double() @ beta.double() + (b1.double() if b1 is not None else 0.0)
    hq = fake_quant(orc.activation(act, xq @ w1q.t() + c).float(), rx)
    out = hq @ fake_quant(w2.float(), rw).t()
    return out + b2.double() if b2 is not None else out


def forward_mx(x, sd, cfg, num_registers=3, rx="rne", rw="rne"):
    """The oracle's forward in fp64 with the MLP pairs of every ConvMixer and EncoderLayer
    fake-quantised.  ``conv_mixer`` / ``encoder_layer`` are wrapped from outside: each runs the
    oracle's own function with the pair's down projection zeroed (which returns the pair's input
    stream) and adds the MX pair to it.  rx = rw = None: the plain fp64 forward."""
    import sdpnet_oracle as orc
    sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    x = x.double()
    if rx is None:
        return orc.forward(x, sd, cfg, num_registers)
    mixer0, enc0 = orc.conv_mixer, orc.encoder_layer

    def zeroed(sd_, *keys):
        out = dict(sd_)
        for k in keys:
            if out.get(k) is not None:
                out[k] = torch.zeros_like(out[k])
        return out

    def mixer(x, sd_, pre, act):
        x_ = mixer0(x, zeroed(sd_, pre + "conv1d.2.weight", pre + "conv1d.2.bias"), pre, act)
        C = x_.shape[1]
        t = x_.permute(0, 2, 3, 1)
        z = _mlp_mx(t, sd_[pre + "layer_norm_2.gamma"], sd_[pre + "layer_norm_2.beta"], 1e-6,
                    sd_[pre + "conv1d.0.weight"].reshape(4 * C, C), sd_.get(pre + "conv1d.0.bias"),
                    sd_[pre + "conv1d.2.weight"].reshape(C, 4 * C), sd_.get(pre + "conv1d.2.bias"), act, rx, rw)
        return x_ + z.permute(0, 3, 1, 2)

    def encoder(x, reg, sd_, pre, n_head, act, *a, **kw):
        xf, rg = enc0(x, reg, zeroed(sd_, pre + "ff_linear2.weight", pre + "ff_linear2.bias"), pre, n_head, act,
                      *a, **kw)
        B, C, H, W = xf.shape
        R = rg.shape[1]
        t = torch.cat([rg, xf.flatten(2).transpose(1, 2)], dim=1)
        t = t + _mlp_mx(t, sd_[pre + "norm2.weight"], sd_[pre + "norm2.bias"], 1e-5, sd_[pre + "ff_linear1.weight"],
                        sd_[pre + "ff_linear1.bias"], sd_[pre + "ff_linear2.weight"], sd_[pre + "ff_linear2.bias"],
                        act, rx, rw)
        rg, xf = t.split([R, H * W], dim=-2)
        return xf.transpose(1, 2).reshape(B, C, H, W).contiguous(), rg

    orc.conv_mixer, orc.encoder_layer = mixer, encoder
    try:
        return orc.forward(x, sd, cfg, num_registers)
    finally:
        orc.conv_mixer, orc.encoder_layer = mixer0, enc0
