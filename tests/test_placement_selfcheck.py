"""The far-placement harness (placement.py) judged on CPU tensors: marks scaled down to 2^16 and
2^17 bytes (and 2^16 elements), and a torch emulation of a row-mapped copy kernel in five
versions.  The harness must pass the correct one and fail each of the four wrong ones with a
message that names what it saw -- the evidence that test_gpu_placement.py can fail.  No mutated
kernel is built or run on a GPU."""
import pytest
import torch

import placement as pl

DTYPES = [torch.bfloat16, torch.float32]
MARK0 = 1 << 16
M_C = 24     # logical columns; ld = 32 (the near twin of 5 groups stays below 2^16 bytes)


def emulated_copy(src: pl.Placement, dst: pl.Placement, bug: str = ""):
    """dst rows = src rows the way a kernel does it: a byte offset per element into the flat
    destination allocation, with the arithmetic slip named by ``bug``."""
    es, ld, C, M = dst.es, dst.ld, dst.C, dst.M
    flat = dst.ibuf.view(-1)
    sflat = src.ibuf.view(-1)
    rows = M + 1 if bug == "row_past_end" else M
    cols = C + 2 if bug == "padding" else C
    m = torch.arange(rows)
    c = torch.arange(cols)
    ms = m.clamp(max=M - 1)
    drow = (ms // dst.grp) * dst.gstride + dst.off + ms % dst.grp + (m - ms)   # row M: the row after row M - 1
    srow = (ms // src.grp) * src.gstride + src.off + ms % src.grp
    doff = ((drow * ld)[:, None] + c[None]) * es                       # byte offsets
    soff = (srow * src.ld)[:, None] + c.clamp(max=C - 1)[None]          # element offsets
    keep = torch.ones_like(doff, dtype=torch.bool)
    if bug == "wrap":          # 16-bit byte offset (the scaled-down uint32_t)
        doff = doff % MARK0
    if bug == "short_extent":  # descriptor one row short: the range check drops the stores
        keep = doff < int(drow[M - 1]) * ld * es
    flat[(doff // es)[keep]] = sflat[soff[keep]]


def _pair(dtype, grp=64):
    marks = pl.marks_for(dtype, MARK0)
    dst = pl.Placement.far(M_C, dtype, marks, "cpu", grp=grp, sub=2 if dtype == torch.bfloat16 else 1)
    src = pl.Placement.near(M_C, dtype, "cpu", grp=grp, groups=dst.groups)
    g = torch.Generator().manual_seed(1)
    data = torch.randn(src.M, M_C, generator=g).to(dtype)
    src.scatter(data)
    return src, dst, data


@pytest.mark.parametrize("dtype", DTYPES)
def test_far_placement_has_the_promised_shape(dtype):
    src, dst, _ = _pair(dtype)
    assert dst.groups == 5 and dst.off > 0 and dst.ld > dst.C and dst.ld % 8 == 0
    assert dst.crossed() == list(dst.marks)          # rows on both sides of every mark
    rowb = dst.ld * dst.es
    for mk in dst.marks:                              # one group straddles each mark
        assert any(dst.row_byte(g * 64) + rowb <= mk <= dst.row_byte(g * 64 + 63) for g in range(5))
    starts = [dst.row_byte(g * 64) for g in range(5)]
    assert all(b - a > 64 * rowb for a, b in zip(starts, starts[1:]))   # groups in different regions
    assert dst.nbytes - (dst.row_byte(dst.M - 1) + rowb) == pl.TAIL * rowb  # ends a few rows early
    assert src.nbytes < MARK0 and (src.grp, src.off, src.ld, src.groups) == (dst.grp, dst.off, dst.ld, dst.groups)
    assert torch.isnan(dst.t).all() and not torch.isfinite(src.t[0]).any()   # sentinels are NaNs


@pytest.mark.parametrize("grp", [64, 77])
@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_copy_passes(dtype, grp):
    src, dst, data = _pair(dtype, grp)
    emulated_copy(src, dst)
    dst.check("copy", written=True)
    src.assert_untouched("copy source")
    assert torch.equal(dst.gather(), data) and torch.equal(src.gather(), data)


def _kinds(dtype, bug):
    src, dst, _ = _pair(dtype)
    emulated_copy(src, dst, bug)
    f = dst.findings(written=True)
    with pytest.raises(AssertionError) as e:
        dst.check(f"copy[{bug}]", written=True)
    return {k for k, _ in f}, str(e.value), dst


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrapped_byte_offset_is_seen(dtype):
    kinds, msg, dst = _kinds(dtype, "wrap")
    # the rows past 2^16 bytes never arrive, and land on low addresses instead
    assert "dropped" in kinds and kinds - {"dropped"}, msg
    assert f"beyond the mark at byte {MARK0}" in msg and "still hold the sentinel" in msg
    first = next(m for m in range(dst.M) if dst.row_byte(m) + dst.ld * dst.es > MARK0)
    assert f"logical row(s) {first}..{dst.M - 1}" in msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_short_extent_is_seen(dtype):
    kinds, msg, dst = _kinds(dtype, "short_extent")
    assert kinds == {"dropped"}, msg
    assert f"1 logical row(s) {dst.M - 1}..{dst.M - 1} still hold the sentinel" in msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_past_the_end_is_seen(dtype):
    kinds, msg, dst = _kinds(dtype, "row_past_end")
    assert kinds == {"past_end"}, msg
    assert "row past the end written" in msg and "1 row(s) after the last logical row" in msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_columns_are_seen(dtype):
    kinds, msg, dst = _kinds(dtype, "padding")
    assert kinds == {"padding"}, msg
    assert f"padding column written: physical row {dst.off} column {dst.C}" in msg


def test_the_four_messages_differ():
    msgs = [_kinds(torch.bfloat16, b)[1] for b in ("wrap", "short_extent", "row_past_end", "padding")]
    assert len(set(msgs)) == 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_between_groups_and_before_the_operand(dtype):
    src, dst, data = _pair(dtype)
    emulated_copy(src, dst)
    dst.t[dst.off - 1, 0] = 1.0
    dst.t[dst.off + 64, 5] = 1.0
    kinds = {k for k, _ in dst.findings(written=True)}
    assert kinds == {"before", "between"}
    src.t[0, 0] = 0.0                                  # an input that a kernel wrote to
    with pytest.raises(AssertionError, match="row before the first group written"):
        src.assert_untouched("copy source")
