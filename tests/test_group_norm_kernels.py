"""osr_group_norm_stats and osr_gn_relu_merge (csrc/osr_semseg.hip) against float64 torch-CPU references on the stored inputs
(tests/panoptic_common.py). fp32 storage: max |got - ref| <= 1e-4 max |ref| (the project's fp32 contract). fp16 / bf16 storage: the
reference is rounded once to the storage type and the bound is two ulps of that type relative to max |ref| (2^-10 / 2^-7): the kernel
rounds once, the reference's own rounding is the other ulp. The statistics are fp32 whatever the storage is: 1e-4 max |ref|."""
import pytest
import torch

from tests.panoptic_common import EPS, gn_merge_reference, gn_stats_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = {torch.float32: 1e-4, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
# (n, h, w, c): one partial chunk, several pixels per thread, and (1, 100, 168, 128) = 16800 pixels, 17 chunks of 1024 (the last partial)
SHAPES = [(2, 3, 5, 128), (2, 16, 20, 128), (1, 100, 168, 128), (2, 16, 20, 64), (2, 16, 20, 256)]


def _input(shape, dtype, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    n, h, w, c = shape
    # a per-channel scale and offset, so that groups differ and a wrong channel -> group map shows
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand(c, generator=g)) + torch.randn(c, generator=g) + offset
    return x.to(dtype)


def _affine(c, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)


def _check(got, ref64, dtype, what):
    ref = ref64.to(dtype).double() if dtype != torch.float32 else ref64
    err = float((got.detach().cpu().double() - ref).abs().max())
    scale = float(ref64.abs().max())
    print(f"[gn] {what} {str(dtype)[6:]}: max err {err:.3e} = {err / scale:.3e} of max |ref| {scale:.3e} (bound {BOUND[dtype]:.3e})")
    assert err <= BOUND[dtype] * scale, (what, err, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_stats_and_one_term_merge(osr, shape, dtype):
    ops = osr.ops
    x = _input(shape, dtype, 1)
    gamma, beta = _affine(shape[3], 2)
    xd = x.to(DEV)
    mean, rstd = ops.group_norm_stats(xd)
    rmean, rrstd = gn_stats_reference(x)
    for got, ref, what in ((mean, rmean, "mean"), (rstd, rrstd, "rstd")):
        assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], 32)
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[gn] {what} {shape} {str(dtype)[6:]}: {err / float(ref.abs().max()):.3e}")
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)
    m2, r2 = ops.group_norm_stats(xd)
    assert torch.equal(m2, mean) and torch.equal(r2, rstd)  # repeats are bit-identical
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for up2 in (False, True):
        out = ops.gn_relu_merge([(xd, (mean, rstd), gd, bd, up2)])
        f = 2 if up2 else 1
        assert out.dtype == dtype and tuple(out.shape) == (shape[0], shape[1] * f, shape[2] * f, shape[3])
        _check(out, gn_merge_reference([(x, gamma, beta, up2)]), dtype, f"merge {shape} up2={up2}")
        assert torch.equal(ops.gn_relu_merge([(xd, (mean, rstd), gd, bd, up2)]), out)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_four_terms_with_mixed_up2_and_a_term_without_stats(osr, dtype):
    """The head's last launch: p2 plain + three upsampled terms, in term order; then the NORM "" form of it, where a term is only rectified."""
    ops = osr.ops
    n, h, w, c = 2, 12, 20, 128
    shapes = [(n, h, w, c), (n, h // 2, w // 2, c), (n, h // 2, w // 2, c), (n, h // 2, w // 2, c)]
    xs = [_input(s, dtype, 10 + i) for i, s in enumerate(shapes)]
    aff = [_affine(c, 20 + i) for i in range(4)]
    ups = [False, True, True, True]
    dev_terms, ref_terms = [], []
    for x, (gamma, beta), up2 in zip(xs, aff, ups):
        xd = x.to(DEV)
        dev_terms.append((xd, ops.group_norm_stats(xd), gamma.to(DEV), beta.to(DEV), up2))
        ref_terms.append((x, gamma, beta, up2))
    out = ops.gn_relu_merge(dev_terms)
    _check(out, gn_merge_reference(ref_terms), dtype, "four terms")
    assert torch.equal(ops.gn_relu_merge(dev_terms), out)
    # terms 1 and 3 without statistics: relu only
    mixed_dev = [t if i in (0, 2) else (t[0], None, None, None, t[4]) for i, t in enumerate(dev_terms)]
    mixed_ref = [t if i in (0, 2) else (t[0], None, None, t[3]) for i, t in enumerate(ref_terms)]
    _check(ops.gn_relu_merge(mixed_dev), gn_merge_reference(mixed_ref), dtype, "mixed terms")
    plain = ops.gn_relu_merge([(dev_terms[0][0], None, None, None, False)])
    assert torch.equal(plain, torch.relu(dev_terms[0][0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_group_means_thirty_standard_deviations_out(osr, dtype):
    """|mean| = 30 std in every group: E[x^2] - mean^2 of the raw values would lose three digits of the variance here."""
    ops = osr.ops
    shape = (1, 40, 52, 128)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(shape, generator=g) + 30.0 * torch.where(torch.arange(128) // 4 % 2 == 0, 1.0, -1.0)).to(dtype)
    rmean, rrstd = gn_stats_reference(x)
    assert float((rmean.abs() * rrstd).min()) > 25.0
    xd = x.to(DEV)
    mean, rstd = ops.group_norm_stats(xd)
    for got, ref, what in ((mean, rmean, "mean"), (rstd, rrstd, "rstd")):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[gn] offset input {what} {str(dtype)[6:]}: {err / float(ref.abs().max()):.3e}")
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)
    gamma, beta = _affine(128, 6)
    out = ops.gn_relu_merge([(xd, (mean, rstd), gamma.to(DEV), beta.to(DEV), True)])
    _check(out, gn_merge_reference([(x, gamma, beta, True)]), dtype, "offset input merge")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_constant_group_has_variance_zero(osr, dtype):
    """Groups 3 and 17 are constant over the whole image (and over their channels): M2 is exactly zero and rstd = 1 / sqrt(eps)."""
    ops = osr.ops
    x = _input((2, 16, 20, 128), dtype, 7)
    x[..., 12:16], x[..., 68:72] = 2.5, -0.375  # (exact in every storage type)
    rmean, rrstd = gn_stats_reference(x)
    assert float(rrstd[:, [3, 17]].min()) == float(rrstd.max()) == 1.0 / EPS ** 0.5
    mean, rstd = ops.group_norm_stats(x.to(DEV))
    for got, ref, what in ((mean, rmean, "mean"), (rstd, rrstd, "rstd")):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[gn] constant groups {what} {str(dtype)[6:]}: {err / float(ref.abs().max()):.3e}")
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)
    assert bool((rstd.cpu()[:, [3, 17]].double() - 1.0 / EPS ** 0.5).abs().max() <= 1e-4 / EPS ** 0.5)
    gamma, beta = _affine(128, 8)
    out = ops.gn_relu_merge([(x.to(DEV), (mean, rstd), gamma.to(DEV), beta.to(DEV), False)])
    _check(out, gn_merge_reference([(x, gamma, beta, False)]), dtype, "constant groups merge")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [64, 128, 256])
def test_a_one_pixel_map(osr, c, dtype):
    """h = w = 1: a group is c / 32 values, one thread per vector slot holds them all, 255 of the 256 threads' triples are empty."""
    ops = osr.ops
    x = _input((3, 1, 1, c), dtype, 9)
    rmean, rrstd = gn_stats_reference(x)
    mean, rstd = ops.group_norm_stats(x.to(DEV))
    for got, ref, what in ((mean, rmean, "mean"), (rstd, rrstd, "rstd")):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[gn] 1 x 1 map c={c} {what} {str(dtype)[6:]}: {err / float(ref.abs().max()):.3e}")
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)
    gamma, beta = _affine(c, 10)
    for up2 in (False, True):
        out = ops.gn_relu_merge([(x.to(DEV), (mean, rstd), gamma.to(DEV), beta.to(DEV), up2)])
        _check(out, gn_merge_reference([(x, gamma, beta, up2)]), dtype, f"1 x 1 map c={c} up2={up2}")


def test_bad_arguments_are_refused(osr):
    ops = osr.ops
    with pytest.raises(osr.OsrError):
        ops.group_norm_stats(torch.zeros(1, 4, 4, 128))  # CPU tensor
    with pytest.raises(osr.OsrError):
        ops.group_norm_stats(torch.zeros(1, 4, 4, 96, device=DEV))  # 3 channels per group
    x = torch.zeros(1, 4, 4, 128, device=DEV)
    with pytest.raises(osr.OsrError):
        ops.gn_relu_merge([(x, None, None, None, False), (x, None, None, None, True)])  # sizes disagree
    with pytest.raises(osr.OsrError):
        ops.gn_relu_merge([(x, None, None, None, False)] * 5)
    with pytest.raises(osr.OsrError):
        ops.gn_relu_merge([(x.cpu(), None, None, None, False)])
