"""osr_avgpool_rows: the spatial mean behind res5 ([d2] Res5ROIHeads: box_features.mean(dim=[2, 3])) on channels-last rows.

Tolerance: the kernel adds a RoI's s positions to an fp32 accumulator in ascending order and divides by s. Each of the s - 1 additions
and the division round once, each by at most 2^-24 of a partial sum that is at most s * max|x| in magnitude; divided by s that is
(s - 1 + 1) * 2^-24 * max|x| against the float64 mean of the same stored values: 49 * 2^-24 * max|x| = 2.9e-6 * max|x| covers every
s <= 49 the test uses."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
BOUND = 49 * 2.0 ** -24
SEG = 53  # 1537 = 29 segments of 53 rows


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def rows(r, s, c, dtype, seed=0):
    gg = torch.Generator().manual_seed(seed * 7919 + r * 31 + s * 7 + c)
    x = (torch.randn(r, s, c, generator=gg) * 3 + 1).to(dtype)   # a mean away from zero: the partial sums grow
    return x


def check(out, x, exists):
    ref = x[exists].double().mean(1)
    err = (out[exists].double() - ref).abs().max().item() if ref.numel() else 0.0
    bound = BOUND * (x[exists].abs().max().item() if ref.numel() else 0.0)
    print(f"avgpool_rows r={x.shape[0]} s={x.shape[1]} c={x.shape[2]} {x.dtype}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert bool((out[~exists] == 0).all()), "rows that do not exist are not zeros"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", [2048, 64])
@pytest.mark.parametrize("s", [49, 16, 1])
@pytest.mark.parametrize("r", [0, 1, 1537])
def test_mean_over_positions(ops, r, s, c, dtype):
    x = rows(r, s, c, DTYPES[dtype])
    out = ops.avgpool_rows(x.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (r, c) and out.dtype == torch.float32
    check(out.cpu(), x, torch.ones(r, dtype=torch.bool))
    if r:
        x4 = x.view(r, 7, 7, c) if s == 49 else x.view(r, 4, 4, c) if s == 16 else x.view(r, 1, 1, c)
        assert torch.equal(ops.avgpool_rows(x4.to(DEV)).cpu(), out.cpu())  # (r, h, w, c) is the same rows


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", [2048, 64])
@pytest.mark.parametrize("s", [49, 16, 1])
def test_rows_valid_with_empty_partial_and_full_segments(ops, s, c, dtype):
    r = 1537
    gg = torch.Generator().manual_seed(3)
    valid = torch.randint(0, SEG + 1, (r // SEG,), generator=gg, dtype=torch.int32)
    valid[0], valid[1], valid[2], valid[-1] = 0, SEG, 17, 0
    exists = (torch.arange(r) % SEG) < valid[torch.arange(r) // SEG]
    x = rows(r, s, c, DTYPES[dtype], seed=1)
    xin = x.clone()
    xin[~exists] = float("nan")  # what a row that does not exist holds reaches nothing
    out = ops.avgpool_rows(xin.to(DEV), valid.to(DEV), SEG).cpu()
    check(out, x, exists)
    plain = ops.avgpool_rows(x.to(DEV)).cpu()
    assert torch.equal(out[exists], plain[exists])  # an existing row is the same bits with and without the segment table


@pytest.mark.parametrize("valid", [0, 1])
def test_one_row_segment(ops, valid):
    x = rows(1, 49, 2048, torch.float16, seed=2)
    out = ops.avgpool_rows(x.to(DEV), torch.tensor([valid], dtype=torch.int32, device=DEV), 1).cpu()
    check(out, x, torch.tensor([bool(valid)]))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_width_that_is_no_multiple_of_eight_and_the_largest_s(ops, dtype):
    """c = 36: 16-bit rows then take 8-byte loads. s = 196 is the limit; the bound scales with s."""
    x = rows(131, 196, 36, DTYPES[dtype], seed=4)
    out = ops.avgpool_rows(x.to(DEV)).cpu()
    err = (out.double() - x.double().mean(1)).abs().max().item()
    assert err <= 196 * 2.0 ** -24 * x.abs().max().item()


def test_repeats_are_bit_identical(ops):
    x = rows(1537, 49, 2048, torch.float16, seed=5).to(DEV)
    first = ops.avgpool_rows(x)
    for _ in range(3):
        assert torch.equal(ops.avgpool_rows(x), first)


def test_refusals(ops, osr):
    for shape in ((4, 197, 64), (4, 49, 6), (4, 49, 66)):
        with pytest.raises(osr._lib.OsrError, match=r"status -2"):
            ops.avgpool_rows(torch.zeros(shape, dtype=torch.float16, device=DEV))
    with pytest.raises(osr._lib.OsrError):
        ops.avgpool_rows(torch.zeros(4, 49, 64, dtype=torch.float16))  # a CPU tensor: refused, not computed on the host
    with pytest.raises(osr._lib.OsrError):
        ops.avgpool_rows(torch.zeros(8, 49, 64, dtype=torch.float16, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), 4)
