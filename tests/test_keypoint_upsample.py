"""osr_keypoint_upsample (csrc/osr_keypoint.hip): ConvTranspose2d(cin -> k, 4 x 4, stride 2, padding 1) + bias and the bilinear x2
(align_corners=False) in one launch, against the float64 chain F.conv_transpose2d -> F.interpolate on the same storage-rounded
operands (tests/keypoint_common.py upsample_chain; no intermediate rounding).

Bound: B = max(32 * e32, 1e-5), e32 = the error of the same chain in torch-CPU fp32 against float64, computed here (the form of
tests/test_mask_upsample_predict.py). The weights are drawn so that the heatmaps have a standard deviation of at least 0.5 (asserted).
A chain that rounded the 2s x 2s map to fp16 exceeds the bound (test_a_lossy_low_resolution_map_would_be_caught, CPU only).

(r, cin, k): (1, 64, 17) one chunk of the channel stream; (3, 512, 17) the production width, eight chunks (sixteen in fp32);
(2, 128, 5); k = 1 and k = 32 the ends of the padded N tile (k = 32 takes two interpolation passes, as 17 does). s = 14 has a
partial last M block (196 = 6 * 32 + 4), s = 8 exactly two. s = 9 .. 13, the other sizes the entry point accepts: the index splits by a
float reciprocal ((int)((m + 0.5f) * (1 / s)), also for 4s and 16 s^2 in the interpolation), partial last M blocks of 17, 4, 25, 16 and
9 rows, and 648 .. 1352 prefetch pieces for 256 threads (three to six rounds, the last partial). Measured on the MI355X for s = 9 .. 13:
err 0.6e-6 .. 2.8e-6 = 0.3 .. 1.4 e32 (bounds 1.5e-5 .. 9.7e-5)."""
import functools

import pytest
import torch

from tests.keypoint_common import upsample_chain

DEV = "cuda:0"
gpu = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
CASES = [(1, 64, 17, 14), (3, 512, 17, 14), (2, 128, 5, 14), (1, 64, 1, 14), (1, 64, 32, 14), (2, 128, 5, 8),
         (1, 128, 17, 9), (1, 64, 17, 10), (1, 64, 17, 11), (1, 64, 5, 12), (2, 64, 17, 13)]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


@functools.lru_cache(maxsize=None)
def _operands(r: int, c: int, k: int, s: int, dt: torch.dtype):
    """x (r, s, s, c) and the score_lowres weight (c, k, 4, 4) rounded to dt; bias (k) fp32. Four taps of c channels meet in an output
    pixel: std (1 / (4 c)) ** 0.5 * 1.5 gives heatmaps of unit scale."""
    g = torch.Generator().manual_seed(1000 * r + c + 7 * k + s)
    x = torch.randn(r, s, s, c, generator=g).to(dt)
    w = (torch.randn(c, k, 4, 4, generator=g) * 1.5 * (1.0 / (4 * c)) ** 0.5).to(dt)
    b = torch.randn(k, generator=g) * 0.5
    return x, w, b


@functools.lru_cache(maxsize=None)
def _reference(r: int, c: int, k: int, s: int, dt: torch.dtype):
    x, w, b = _operands(r, c, k, s, dt)
    ref = upsample_chain(x, w, b, torch.float64)
    e32 = float((upsample_chain(x, w, b, torch.float32).double() - ref).abs().max()) if r else 0.0
    return ref, e32


def _run(ops, r, c, k, s, dt, rows_valid=None, seg_rows=0, x=None):
    from openset_rcnn_amd.host.weights import pack_keypoint_deconv_weight
    x0, w, b = _operands(r, c, k, s, dt)
    rv = None if rows_valid is None else torch.tensor(rows_valid, dtype=torch.int32, device=DEV)
    return ops.keypoint_upsample((x0 if x is None else x).to(DEV), pack_keypoint_deconv_weight(w, dt).to(DEV), b.to(DEV), rv, seg_rows)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("r, c, k, s", CASES)
def test_against_the_float64_chain(ops, r, c, k, s, dt):
    ref, e32 = _reference(r, c, k, s, dt)
    assert float(ref.std()) >= 0.5, f"the reference heatmaps must spread (std {float(ref.std()):.3f})"
    bound = max(32 * e32, 1e-5)
    out = _run(ops, r, c, k, s, dt)
    assert out.shape == (r, k, 4 * s, 4 * s) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print(f"r={r} c={c} k={k} s={s} {dt}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}, heatmap std {float(ref.std()):.3f}")
    assert err <= bound, f"max |heatmaps - float64| {err:.3e} > {bound:.3e} (e32 {e32:.3e})"
    assert torch.equal(_run(ops, r, c, k, s, dt), out), "two runs are bit-identical"


def test_a_lossy_low_resolution_map_would_be_caught():
    """The bound tells the fused form from one that stores the 2s x 2s map in fp16: rounding it costs more than B (CPU only)."""
    x, w, b = _operands(3, 512, 17, 14, torch.float16)
    ref, e32 = _reference(3, 512, 17, 14, torch.float16)
    lossy = upsample_chain(x, w, b, torch.float32, low_dtype=torch.float16)
    err = float((lossy.double() - ref).abs().max())
    print(f"fp16 low-resolution map: err {err:.3e}, bound {max(32 * e32, 1e-5):.3e}")
    assert err > 4 * max(32 * e32, 1e-5)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
def test_padding_rows_are_zeros(ops, dt):
    """Six RoIs as three segments of two with rows_valid (2, 0, 1): RoIs 2, 3 and 5 do not exist and come out as exact zeros, whatever
    their inputs hold (NaN: they are selected away, not multiplied away); the live ones as the reference's."""
    r, c, k, s = 6, 128, 17, 14
    ref, e32 = _reference(r, c, k, s, dt)
    bound = max(32 * e32, 1e-5)
    out = _run(ops, r, c, k, s, dt, (2, 0, 1), 2).cpu()
    for i in range(r):
        if i in (0, 1, 4):
            assert float((out[i].double() - ref[i]).abs().max()) <= bound, i
        else:
            assert float(out[i].abs().max()) == 0.0, f"RoI {i} must be zeros"
    xn = _operands(r, c, k, s, dt)[0].clone()
    xn[[2, 3, 5]] = float("nan")
    assert torch.equal(_run(ops, r, c, k, s, dt, (2, 0, 1), 2, x=xn).cpu(), out)
    full = _run(ops, r, c, k, s, dt).cpu()  # without rows_valid every RoI exists
    assert torch.equal(full[[0, 1, 4]], out[[0, 1, 4]]) and float((full.double() - ref).abs().max()) <= bound


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
def test_no_rois(ops, dt):
    out = _run(ops, 0, 64, 17, 14, dt)
    assert out.shape == (0, 17, 56, 56) and out.dtype == torch.float32


@gpu
def test_shape_rules(ops, osr):
    import ctypes
    lib = osr._lib.load()
    a = ctypes.c_void_p(256)  # (never dereferenced: the shape rules come first)
    dt = osr.ops._DT[torch.float16]
    for (s, cin, k) in ((7, 64, 17), (15, 64, 17), (14, 32, 17), (14, 96, 17), (14, 576, 17), (14, 64, 0), (14, 64, 33)):
        assert lib.osr_keypoint_upsample(a, dt, 1, s, cin, k, a, a, None, 0, a, None) == osr._lib.ERR_UNSUPPORTED, (s, cin, k)
        assert b"osr_keypoint_upsample" in lib.osr_last_error()
    x = torch.zeros(1, 14, 14, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(osr.OsrError, match="w_packed"):
        osr.ops.keypoint_upsample(x, torch.zeros(16, 8, dtype=torch.float16, device=DEV), torch.zeros(17, device=DEV))
    with pytest.raises(osr.OsrError, match="rows_valid"):
        _run(osr.ops, 2, 128, 5, 14, torch.float16, (1,), 1)
