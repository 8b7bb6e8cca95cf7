"""osr_preprocess, osr_maxpool3x3s2 and osr_subsample2 (csrc/osr_preproc_pool.hip) against torch on the CPU, bit for bit, at every
destination / storage type, at ragged and one-pixel sizes, and past one pass of their grid-stride loops.

The three kernels run under a grid capped at 8192 blocks of 256 lanes: CAP = 2,097,152 items per pass (an item is one padded output
pixel of the preprocess, one 8-channel vector of the pool, one 16-byte chunk of the subsample). The past-the-cap tests assert their
own item count against CAP. Every test here hands the C entry a buffer of its own, pre-filled with NaN (777 where NaN is a legitimate
result; the ops wrappers allocate with torch.empty, and a recycled block may still hold an earlier, correct result): an element no
lane wrote shows as the fill.

References. preprocess: (src.float() - mean) / std in torch-CPU fp32 (IEEE subtraction and division, as the kernel's: the file is
built without fast-math and without contraction), rounded once to the destination type, at offset (3, 3) of a zero tensor.
pool / subsample: F.max_pool2d(x.float(), 3, 2, 1) / F.max_pool2d(x.float(), 1, 2, 0), converted back to the storage type (exact:
the maximum is one of the inputs), non-finite values included."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 8192 * 256
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
DT_IDS = ["fp16", "bf16", "fp32"]
MEAN, STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- osr_preprocess ----------------------------------------------------------------------------------------------------------------
def _preprocess(ops, src, hp, wp, dt):
    """-> (the NaN-pre-filled (n, hp + 6, wpad, 4) destination after the call, on the CPU; the reference)."""
    n, _, h, w = src.shape
    wd = ops.stem_padded_width(wp)
    assert wd == (wp + 8 + 7) // 8 * 8
    dst = torch.full((n, hp + 6, wd, 4), NAN, dtype=dt, device=DEV)
    d = src.to(DEV)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    status = ops._lib.load().osr_preprocess(C.c_void_p(d.data_ptr()), int(src.dtype == torch.uint8), n, h, w, hp, wp, mean, std,
                                            C.c_void_p(dst.data_ptr()), ops.dtype_code(dt), _stream())
    assert status == 0
    torch.cuda.synchronize()
    nrm = (src.float() - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)  # fp32
    ref = torch.zeros(n, hp + 6, wd, 4)
    ref[:, 3:3 + h, 3:3 + w, :3] = nrm.permute(0, 2, 3, 1)
    return dst.cpu(), ref.to(dt)


# n, h, w, hp, wp: wp + 8 a multiple of 8 (64) and not (61 -> 69 -> 72); no padding at all; a one-pixel image
PRE_CASES = [(2, 37, 50, 64, 64), (2, 30, 45, 40, 61), (1, 16, 24, 16, 24), (2, 1, 1, 1, 1)]


@pytest.mark.parametrize("case", PRE_CASES, ids=["37x50-in-64x64", "30x45-in-40x61", "16x24-unpadded", "1x1"])
@pytest.mark.parametrize("src_dt", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_preprocess_every_destination(ops, dt, src_dt, case):
    n, h, w, hp, wp = case
    img = torch.randint(0, 256, (n, 3, h, w), generator=g(100 + h + w), dtype=torch.uint8)
    src = img if src_dt == torch.uint8 else img.float() + 0.25
    got, ref = _preprocess(ops, src, hp, wp, dt)
    assert not bool(torch.isnan(got).any()), "a destination element was not written"
    assert torch.equal(_bits(got), _bits(ref))
    assert float(got[..., 3].abs().max()) == 0.0 and float(got[:, :3].abs().max()) == 0.0  # the 4th channel and the halo are zeros


def test_preprocess_past_the_grid_cap(ops):
    """Three 795 x 1330 images in (800, 1344): 3 x 806 x 1352 = 3,269,136 padded pixels, 1.56 passes of the capped grid."""
    n, h, w, hp, wp = 3, 795, 1330, 800, 1344
    total = n * (hp + 6) * ops.stem_padded_width(wp)
    assert total == 3269136 and total > CAP, "the shape must need a second pass of the grid-stride loop"
    src = torch.randint(0, 256, (n, 3, h, w), generator=g(101), dtype=torch.uint8)
    got, ref = _preprocess(ops, src, hp, wp, F16)
    assert not bool(torch.isnan(got).any()), "a destination element was not written"
    assert torch.equal(_bits(got), _bits(ref))


# ---- osr_maxpool3x3s2 / osr_subsample2 ------------------------------------------------------------------------------------------------
def _pooled(ops, entry, x, fill=NAN):
    """x (n, hi, wi, c) on the CPU -> the `fill`-pre-filled output of the C entry (osr_maxpool3x3s2 / osr_subsample2), on the CPU."""
    n, hi, wi, c = x.shape
    out = torch.full((n, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, c), fill, dtype=x.dtype, device=DEV)
    d = x.contiguous().to(DEV)
    status = getattr(ops._lib.load(), entry)(C.c_void_p(d.data_ptr()), n, hi, wi, c, C.c_void_p(out.data_ptr()), ops.dtype_code(x.dtype), _stream())
    assert status == 0
    torch.cuda.synchronize()
    return out.cpu()


def _ref_pool(x, k, pad):
    """torch-CPU max_pool2d(k, 2, pad) of an NHWC tensor in fp32 -> NHWC in x's dtype."""
    return F.max_pool2d(x.permute(0, 3, 1, 2).float(), k, 2, pad).permute(0, 2, 3, 1).contiguous().to(x.dtype)


POOL_MAPS = [(hi, wi) for hi in (1, 2, 3) for wi in (1, 2, 30)] + [(21, 30)]
POOLS = [("osr_maxpool3x3s2", 3, 1), ("osr_subsample2", 1, 0)]


@pytest.mark.parametrize("entry, k, pad", POOLS, ids=["maxpool", "subsample"])
@pytest.mark.parametrize("c", [8, 64])  # subsample: c = 8 is one 16-byte chunk per pixel in fp16 / bf16 and two in fp32
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_pool_and_subsample_types_and_edges(ops, dt, c, entry, k, pad):
    for hi, wi in POOL_MAPS:
        x = torch.randn(2, hi, wi, c, generator=g(200 + 31 * hi + wi + c)).to(dt)
        got = _pooled(ops, entry, x)
        assert not bool(torch.isnan(got).any()), (hi, wi, "an output element was not written")
        assert torch.equal(_bits(got), _bits(_ref_pool(x, k, pad))), (hi, wi)


def test_maxpool_past_the_grid_cap(ops):
    n, hi, wi, c = 1, 1025, 1025, 64
    total = n * ((hi - 1) // 2 + 1) * ((wi - 1) // 2 + 1) * (c // 8)
    assert total == 2105352 and total > CAP, "the shape must need a second pass of the grid-stride loop"
    x = torch.randn(n, hi, wi, c, generator=torch.Generator(device=DEV).manual_seed(201), device=DEV, dtype=F16).cpu()  # (135 MB: drawn on the device)
    got = _pooled(ops, "osr_maxpool3x3s2", x)
    assert not bool(torch.isnan(got).any()), "an output element was not written"
    assert torch.equal(_bits(got), _bits(_ref_pool(x, 3, 1)))


def test_subsample_past_the_grid_cap(ops):
    n, hi, wi, c = 1, 363, 363, 256
    total = n * ((hi - 1) // 2 + 1) * ((wi - 1) // 2 + 1) * (c * 4 // 16)  # 16-byte chunks of fp32
    assert total == 2119936 and total > CAP, "the shape must need a second pass of the grid-stride loop"
    x = torch.randn(n, hi, wi, c, generator=torch.Generator(device=DEV).manual_seed(202), device=DEV).cpu()
    got = _pooled(ops, "osr_subsample2", x)
    assert not bool(torch.isnan(got).any()), "an output element was not written"
    assert torch.equal(_bits(got), _bits(_ref_pool(x, 1, 0)))


@pytest.mark.parametrize("dt", [F32, F16], ids=["fp32", "fp16"])
def test_maxpool_non_finite_inputs_follow_max_pool2d(ops, dt):
    """A 9 x 10 map: the windows of output pixels (0, 0) (four pixels inside the map) and (1, 1) (nine) hold nothing but -inf -> -inf;
    a +inf wins its windows; a NaN with a larger finite neighbour (8.0, the map's largest value) is every window's result that holds
    it, in the channels that have it (0..3 of 8) and in no other. Expected: F.max_pool2d, as bits, NaNs matched by position."""
    x = torch.randn(2, 9, 10, 8, generator=g(203)).clamp(-4.0, 4.0).to(dt)
    x[:, 0:4, 0:4] = -INF
    x[0, 6, 7] = INF
    x[1, 5, 6, :4] = NAN
    x[1, 5, 7] = 8.0
    ref = _ref_pool(x, 3, 1)
    assert bool((ref[:, 0, 0] == -INF).all()) and bool((ref[:, 1, 1] == -INF).all()) and bool((ref[0, 3, 3:5] == INF).all())
    nan = torch.isnan(ref)
    assert bool(nan[1, 2:4, 3, :4].all()) and not bool(nan[1, :, :, 4:].any()) and not bool(nan[0].any())
    assert bool((ref[1, 2:4, 3:5, 4:] == 8.0).all())
    got = _pooled(ops, "osr_maxpool3x3s2", x, fill=777.0)
    assert not bool((got == 777.0).any()), "an output element was not written"
    print(f"[non-finite pool, {dt}] -inf window: got {got[0, 1, 1].tolist()}; NaN window: got {got[1, 2, 3].tolist()}")
    assert torch.equal(torch.isnan(got), nan), "NaNs are not where max_pool2d puts them"
    assert torch.equal(_bits(got)[~nan], _bits(ref)[~nan])
