"""The lifecycle judge can fail, and the cache key sees what it must (no GPU).

tests/test_gpu_lifecycle.py judges the eval logits after every fused optimizer step against the
fp64 oracle trajectory of tests/lifecycle.py, with a bound capped at lifecycle.LOGIT_CAP.  Here, on
the CPU oracle alone:

* a forward that mixes last step's derived weights into this step's (q / k / v / ff_linear1 and the
  two encoder LayerNorms from step k-1, everything else current: what the fp32 eval forward
  computes when its prepared-weight cache is not rebuilt) misses the fp64 trajectory by 36x to
  380x the cap on every config at every step >= 2, so the trajectory test cannot pass on it;
* the patch-conv weight alone or the positional tables alone, stale, move the s_base logits by
  2e-5 to 4e-5 -- BELOW its 4e-4 cap -- and s_convemb has no trained positional table at all.  The
  trajectory judge is blind to those two entries there; on s_poolhead_bias (mean-pool head, cap
  9e-5) it sees both (3.5e-3 and 1.4e-3).  For the patch weight and the positional tables the
  suite therefore relies on the bit-exact twin tests of test_gpu_lifecycle.py (the MainModel
  cases, the ConvPatcher / EmbeddingLayer / ConvEmbedding sub-module cases and the
  training-forward table cases), which see a single stale ulp;
* every per-step movement of the fp64 logits is at least 1e3 times the cap;
* sdpnet_engine.cached() on CPU parameters with a counting ``build``: what rebuilds an entry, what
  does not, and the notifications (version bump, ``invalidate``) for writes it cannot see.
"""
import ctypes

import pytest
import torch
import torch.nn as nn

import lifecycle as lc
import sdpnet_oracle as orc

DERIVED = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "ff_linear1.weight", "ff_linear1.bias",
           ".norm1.", ".norm2.")
PATCH = ("conv_init.conv.weight",)
POS = ("horizontal_embedding_layer.weight", "vertical_embedding_layer.weight")


def _stale_misses(name, pats):
    """max|logits(stale mix at step k) - fp64 logits at step k| for k = 2 .. STEPS."""
    c = lc.trajectories(name)
    steps = c["t64"]["steps"]
    out = []
    for k in range(1, lc.STEPS):
        cur, prev = steps[k], steps[k - 1]
        hit = [kk for kk in cur["params"] if any(p in kk for p in pats)]
        assert hit, (name, pats)
        mixed = {kk: (prev["params"][kk] if kk in hit else v) for kk, v in cur["params"].items()}
        logits = orc.forward(c["xval"].double(), mixed, c["cfg"], num_registers=c["nreg"])
        out.append(lc.maxabs(logits, cur["logits"]))
    return out


@pytest.mark.parametrize("name", lc.TRAJ_CONFIGS)
def test_stale_derived_weights_miss_the_trajectory(name):
    miss = _stale_misses(name, DERIVED)
    print(name, "stale q/k/v/ff1/norm1/norm2:", [f"{m:.2e}" for m in miss], "cap", lc.LOGIT_CAP[name])
    assert len(miss) == lc.STEPS - 1 and all(m > lc.LOGIT_CAP[name] for m in miss), miss


def test_stale_patch_weight_and_positional_tables():
    """Seen by the trajectory judge on s_poolhead_bias; below the cap on s_base (see the module
    docstring: those entries are covered by the bit-exact twin tests)."""
    for pats in (PATCH, POS):
        seen = _stale_misses("s_poolhead_bias", pats)
        blind = _stale_misses("s_base", pats)
        print(pats[0], "s_poolhead_bias", [f"{m:.2e}" for m in seen], "s_base", [f"{m:.2e}" for m in blind])
        assert all(m > lc.LOGIT_CAP["s_poolhead_bias"] for m in seen), (pats, seen)
        assert all(0 < m < lc.LOGIT_CAP["s_base"] for m in blind), (pats, blind)


@pytest.mark.parametrize("name", lc.TRAJ_CONFIGS)
def test_every_step_moves_the_logits_a_thousand_caps(name):
    c = lc.trajectories(name)
    mv = lc.movements(c["t64"])
    dev = lc.deviation(c["t32"], c["t64"])
    print(name, "fp64 movement", [f"{m:.3f}" for m in mv], "fp32 oracle vs fp64: params",
          [f"{d[0]:.1e}" for d in dev], "logits", [f"{d[2]:.1e}" for d in dev])
    assert len(mv) == lc.STEPS and all(m >= 1e3 * lc.LOGIT_CAP[name] for m in mv), mv
    # the number format alone stays three orders under the cap: the cap is no invitation
    assert all(d[2] <= 1e-2 * lc.LOGIT_CAP[name] for d in dev), dev


# --------------------------------------------------------------------------- sdpnet_engine.cached
class _Counted:
    def __init__(self, lin):
        self.lin, self.builds = lin, 0

    def get(self):
        import sdpnet_engine as eng

        def build():
            self.builds += 1
            return self.lin.weight.detach().clone()
        return eng.cached(self.lin, "w", [self.lin.weight, self.lin.bias], torch.float32, build)


def _poke(t: torch.Tensor, value: float):
    """Write t[0, 0] behind torch's back, as a kernel given data_ptr() does."""
    v = ctypes.c_float(value)
    ctypes.memmove(t.data_ptr(), ctypes.addressof(v), 4)


def test_cached_rebuilds_when_torch_sees_the_write_and_not_otherwise():
    c = _Counted(nn.Linear(4, 3))
    w0 = c.get()
    assert c.builds == 1 and c.get() is w0 and c.get() is w0 and c.builds == 1  # nothing changed
    with torch.no_grad():
        c.lin.weight.mul_(2.0)                                                   # an in-place op
    assert torch.equal(c.get(), c.lin.weight) and c.builds == 2
    c.lin.load_state_dict({k: v + 1 for k, v in c.lin.state_dict().items()})     # load_state_dict
    assert torch.equal(c.get(), c.lin.weight) and c.builds == 3
    c.lin.weight.detach().add_(1.0)                                              # through a detached alias
    assert torch.equal(c.get(), c.lin.weight) and c.builds == 4
    c.get()
    assert c.builds == 4


def test_cached_needs_a_notification_for_raw_writes():
    import sdpnet_engine as eng
    c = _Counted(nn.Linear(4, 3))
    c.get()
    v = c.lin.weight._version
    _poke(c.lin.weight, 7.0)
    assert float(c.lin.weight.detach()[0, 0]) == 7.0 and c.lin.weight._version == v
    stale = c.get()                      # the key cannot see a raw write: this is why writers notify
    assert c.builds == 1 and float(stale[0, 0]) != 7.0
    with torch.no_grad():                # what sdpnet_train.AdamW.step does after its launches
        torch.autograd.graph.increment_version([c.lin.weight, c.lin.bias])
    assert float(c.get()[0, 0]) == 7.0 and c.builds == 2
    _poke(c.lin.weight, 9.0)
    c.lin.bias.data.mul_(2.0)            # .data writes bump nothing either
    assert c.builds == 2 and float(c.get()[0, 0]) == 7.0
    eng.invalidate(c.lin)                # the documented call for writes nobody can detect
    assert float(c.get()[0, 0]) == 9.0 and c.builds == 3
    c.get()
    assert c.builds == 3


def test_invalidate_reaches_the_children():
    import sdpnet_engine as eng
    seq = nn.Sequential(nn.Linear(4, 3), nn.Sequential(nn.Linear(3, 3)))
    cs = [_Counted(seq[0]), _Counted(seq[1][0])]
    for c in cs:
        c.get()
    eng.invalidate(seq)
    assert all("_sdp_cache" not in m.__dict__ for m in seq.modules())
    for c in cs:
        c.get()
    assert [c.builds for c in cs] == [2, 2]


def test_cached_rebuilds_after_load_state_dict_onto_inference_tensors():
    """Parameters made under torch.inference_mode() have no version counter (they key as -1), and
    load_state_dict copies into them in place at the same address."""
    with torch.inference_mode():
        parent = nn.Sequential(nn.Linear(4, 3))
        lin = parent[0]
        assert lin.weight.is_inference()
        c = _Counted(lin)
        c.get()
        c.get()
        assert c.builds == 1
        ptr = lin.weight.data_ptr()
        parent.load_state_dict({k: v + 1 for k, v in parent.state_dict().items()})  # through the parent
        assert lin.weight.data_ptr() == ptr
        assert torch.equal(c.get(), lin.weight) and c.builds == 2
        c.get()
        assert c.builds == 2
