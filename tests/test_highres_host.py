"""Host: moving a checkpoint to another patch grid (sdpnet_engine.resize_positions).

The reference defines no resampling of its position parameters; the project's rule is linear with
half-pixel centres along each table's own length and bicubic for the ConvEmbedding bone, in fp64,
rounded once to fp32.  The tables are compared with a numpy restatement written here (the
function under test is not called to make the expected values), the bone with F.interpolate in
fp64.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth

CFG = dict(embedding_dim=32, num_blocks=1, n_head=2, conv_kernel_size=3, patch_size=4, conv_block_num=1,
           max_image_size=[14, 14], max_num_registers=5, output_classes=10)
V = "embedding_layer.vertical_embedding_layer.weight"      # sized by max_image_size[0]
H = "embedding_layer.horizontal_embedding_layer.weight"    # sized by max_image_size[1], indexed by rows
GRID_KEYS = {V, H, "embedding_layer.vertical_embedding", "embedding_layer.horizontal_embedding",
             "embedding_layer.bone"}


def _state(cfg, seed=5):
    import model as ours
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    return synth.synth_state_dict(m, seed)


def _fma(a, b, c):
    """a * b + c rounded once to fp64 (exact rational arithmetic, then one rounding)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def linear_np(w, n_new):
    """[n_old, C] -> [n_new, C]: output row i samples the source at (i + 0.5) n_old / n_new - 0.5,
    clamped to the table's ends, and mixes the two neighbouring rows with weights 1 - t and t,
    in fp64, rounded once to fp32.

    With fp32 rows and a dyadic t (every third row of 14 -> 24 has t = 3/8, 1/8, 7/8) the exact
    mix often lies on or next to a tie between two fp32 values, so the last fp64 bit decides the
    fp32 result and the restatement has to round where the fp64 rule rounds: the sample point
    scale * (i + 0.5) - 0.5 and the mix (1 - t) x0 + t x1 are each one multiply-add rounded
    once, as torch's CPU kernel evaluates them; scale = n_old / n_new is one fp64 division."""
    w = np.asarray(w, dtype=np.float64)
    n_old = w.shape[0]
    scale = n_old / n_new
    out = np.empty((n_new, w.shape[1]), dtype=np.float64)
    for i in range(n_new):
        src = max(_fma(scale, i + 0.5, -0.5), 0.0)
        i0 = min(int(np.floor(src)), n_old - 1)
        i1 = min(i0 + 1, n_old - 1)
        t = src - i0
        for c in range(w.shape[1]):
            out[i, c] = _fma(1.0 - t, w[i0, c], t * w[i1, c])
    return out.astype(np.float32)


@pytest.mark.parametrize("conv_embedding", [False, True])
def test_same_size_returns_the_same_tensors(conv_embedding):
    import sdpnet_engine as eng
    cfg = dict(CFG, conv_embedding=conv_embedding)
    sd = _state(cfg)
    out, cfg2 = eng.resize_positions(sd, cfg, [14, 14])
    assert cfg2 == cfg and cfg2 is not cfg
    assert list(out) == list(sd)
    for k in sd:
        assert out[k].dtype == sd[k].dtype and torch.equal(out[k], sd[k]), k


@pytest.mark.parametrize("old,new", [([14, 14], [24, 24]), ([16, 16], [14, 20])])
def test_tables_equal_a_numpy_restatement(old, new):
    import sdpnet_engine as eng
    cfg = dict(CFG, max_image_size=old)
    sd = _state(cfg)
    out, cfg2 = eng.resize_positions(sd, cfg, new)
    assert cfg2["max_image_size"] == new and cfg["max_image_size"] == old
    for key, n in ((V, new[0]), (H, new[1])):
        want = linear_np(sd[key].numpy(), n)
        assert out[key].dtype == torch.float32 and tuple(out[key].shape) == (n, 32)
        assert np.array_equal(out[key].numpy(), want), (key, np.abs(out[key].numpy() - want).max())
    for key, n in (("embedding_layer.vertical_embedding", new[0]), ("embedding_layer.horizontal_embedding", new[1])):
        assert out[key].dtype == sd[key].dtype and torch.equal(out[key], torch.arange(n, dtype=sd[key].dtype))


@pytest.mark.parametrize("old,new", [([14, 14], [24, 24]), ([16, 16], [14, 20])])
def test_bone_equals_fp64_bicubic(old, new):
    import sdpnet_engine as eng
    k = 5
    cfg = dict(CFG, max_image_size=old, conv_embedding=True, conv_embedding_kernel_size=k)
    sd = _state(cfg)
    out, _ = eng.resize_positions(sd, cfg, new)
    bone = sd["embedding_layer.bone"]
    assert tuple(bone.shape) == (1, 32, old[0] + k, old[1] + k)
    want = F.interpolate(bone.double(), size=(new[0] + k, new[1] + k), mode="bicubic", align_corners=False).float()
    assert torch.equal(out["embedding_layer.bone"], want)
    assert out["embedding_layer.register"] is sd["embedding_layer.register"]


def test_affine_table_stays_affine_on_the_interior():
    import sdpnet_engine as eng
    n_old, n_new = 14, 24
    sd = _state(CFG)
    slope = torch.linspace(-1.0, 1.0, 32)
    sd[H] = (0.25 + torch.arange(n_old, dtype=torch.float32)[:, None] * slope[None]).contiguous()
    out, _ = eng.resize_positions(sd, CFG, [n_old, n_new])
    assert out[V] is sd[V]
    t = out[H].double()
    # rows whose sample point lies between the first and last source rows (no edge clamp)
    src = (torch.arange(n_new, dtype=torch.float64) + 0.5) * (n_old / n_new) - 0.5
    inner = ((src >= 0) & (src <= n_old - 1)).nonzero().flatten()
    assert len(inner) >= n_new - 2
    d = t[inner[1:]] - t[inner[:-1]]
    want = (slope.double() * (n_old / n_new)).expand_as(d)
    assert torch.allclose(d, want, rtol=0, atol=2e-6), (d - want).abs().max()
    assert torch.allclose(t[inner], 0.25 + src[inner][:, None] * slope.double()[None], rtol=0, atol=2e-6)


@pytest.mark.parametrize("conv_embedding", [False, True])
@pytest.mark.parametrize("prefix", ["", "module.", "module._orig_mod."])
def test_result_loads_strictly_and_other_tensors_are_equal(conv_embedding, prefix):
    import model as ours
    import sdpnet_engine as eng
    cfg = dict(CFG, conv_embedding=conv_embedding)
    sd = _state(cfg)
    out, cfg2 = eng.resize_positions({prefix + k: v for k, v in sd.items()}, cfg, [24, 20])
    assert set(out) == set(sd)
    for k in sd:
        if k in GRID_KEYS:
            assert out[k].shape != sd[k].shape, k
        else:
            assert out[k] is sd[k], k
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg2)
    m.load_state_dict(out, strict=True)
    assert m.config["max_image_size"] == [24, 20]
    got = m.state_dict()
    for k in out:
        assert torch.equal(got[k], out[k]), k


def test_prefix_names_a_model_inside_a_larger_dict():
    import sdpnet_engine as eng
    sd = _state(CFG)
    both = {"student." + k: v for k, v in sd.items()}
    both.update({"teacher." + k: v for k, v in sd.items()})
    out, _ = eng.resize_positions(both, CFG, [20, 20], prefix="student.")
    assert out["student." + V].shape[0] == 20 and out["teacher." + V] is sd[V]
    with pytest.raises(KeyError):
        eng.resize_positions({"x": torch.zeros(1)}, CFG, [20, 20])
