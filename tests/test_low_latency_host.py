"""CPU: ``sdpnet_hip.gemm_split_plan``, the rule that sends a bf16 GEMM to the split-K kernel while
``low_latency`` is on.  It is a pure function of (M, N, K, cus): no library call, no GPU.

The throughput paths must keep their kernels even with the switch on: every GEMM over the token
rows of the benchmarked forwards (SdP-Net-M at 256 images, SdP-Net-XL at 512, two sub-batch streams
each) is unplanned.  The GEMMs of those forwards that do NOT run over token rows -- the final
encoder's register rows (M = 4 B) and the head (M = B) -- have the shapes of a small batch's token
GEMMs (4 x 128 = 512 rows against 796 for four images), which no function of (M, N, K) can tell
apart; they are 6 of ~260 launches, under-fill the chip exactly as the small batch does, and are
planned.  ``test_register_row_gemms_of_a_large_batch_are_small_gemms`` states that."""
import itertools
import math

import pytest

import sdpnet_hip as sp

CUS = 256
C = 768
# (N, K) of the SdP-Net-M / XL encoder and mixer GEMMs: 1x1 convs / out-projection, the fused
# QKV, FFN up and down; the patch GEMM (K = 3 p^2 padded to 64: 768 at p = 16, 640 at p = 14)
NK_M = [(C, C), (3 * C, C), (4 * C, C), (C, 4 * C)]
NK_XL = NK_M + [(C, 640)]


def token_rows(batch, streams, patches, registers=4):
    b = batch // streams
    return [b * patches, b * (patches + registers)]


def test_throughput_shapes_keep_todays_kernels():
    for M in token_rows(256, 2, 196):          # SdP-Net-M, bs 256
        for N, K in NK_M:
            assert sp.gemm_split_plan(M, N, K, CUS) is None, (M, N, K)
    for M in token_rows(512, 2, 256):          # SdP-Net-XL, bs 512
        for N, K in NK_XL:
            assert sp.gemm_split_plan(M, N, K, CUS) is None, (M, N, K)
    # the classifier (1000 classes) is unaligned at every batch
    assert sp.gemm_split_plan(128, 1000, 1024, CUS) is None


def test_register_row_gemms_of_a_large_batch_are_small_gemms():
    # (512, N, K) is the final encoder's register rows at 128 images and, within one tile, the
    # token rows of 2.6 images: one plan for both
    for N, K in NK_M:
        assert sp.gemm_split_plan(4 * 128, N, K, CUS) == sp.gemm_split_plan(512, N, K, CUS) is not None


@pytest.mark.parametrize("M,N,K", [(196, 100, 768), (196, 1000, 1024), (196, 768, 100), (196, 768, 96),
                                   (196, 32, 768), (1, 768, 32), (196, 800, 768 + 32)])
def test_unaligned_is_unplanned(M, N, K):
    assert sp.gemm_split_plan(M, N, K, CUS) is None


def check_plan(M, N, K, cus):
    plan = sp.gemm_split_plan(M, N, K, cus)
    assert plan is not None, (M, N, K, cus)
    assert plan == sp.gemm_split_plan(M, N, K, cus)          # pure: the same answer twice
    bm, splits = plan
    assert bm in (64, 128)
    assert 1 <= splits <= K // 64
    blocks = math.ceil(M / bm) * (N // 64) * splits
    assert blocks <= 2 * cus, (M, N, K, plan, blocks)
    return plan, blocks


@pytest.mark.parametrize("M", [1, 3, 196, 199, 796])
def test_small_batch_shapes_are_planned(M):
    for N, K in NK_M:
        check_plan(M, N, K, CUS)


def test_one_image_fills_the_chip():
    # the rule is sized for one image's token rows: 1/2 .. 1 x cus workgroups there
    for M, (N, K) in itertools.product([196, 199, 200], NK_M):
        _, blocks = check_plan(M, N, K, CUS)
        assert CUS // 2 <= blocks <= CUS, (M, N, K, blocks)


def test_splits_do_not_depend_on_m():
    # the K-slices decide the summation order: one per (N, K), so that an image's logits do not
    # depend on the batch it runs in while its GEMMs stay planned
    for N, K in NK_M + [(256, 1024), (128, 512), (1024, 128)]:
        got = {sp.gemm_split_plan(M, N, K, CUS) for M in [1, 3, 64, 65, 196, 199, 398, 796]}
        assert None not in got and len({s for _, s in got}) == 1, (N, K, got)


def test_every_plan_over_a_sweep_is_valid():
    n = 0
    for M in [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 196, 199, 200, 255, 256, 257, 392, 796, 1592, 3184, 6368, 12736]:
        for N in [64, 128, 192, 768, 1024, 2304, 3072]:
            for K in [64, 128, 192, 320, 768, 3072]:
                for cus in [64, 256, 304]:
                    if sp.gemm_split_plan(M, N, K, cus) is not None:
                        check_plan(M, N, K, cus)
                        n += 1
    assert n > 100


def test_switch_is_off_by_default_and_restores():
    assert sp.low_latency_enabled() is False
    with sp.low_latency():
        assert sp.low_latency_enabled() is True
        with sp.low_latency(False):
            assert sp.low_latency_enabled() is False
        assert sp.low_latency_enabled() is True
    assert sp.low_latency_enabled() is False
    assert sp.set_low_latency(True) is False
    assert sp.set_low_latency(False) is True
