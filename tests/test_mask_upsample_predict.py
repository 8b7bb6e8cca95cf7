"""osr_mask_upsample_predict (csrc/osr_mask_head.hip): ConvTranspose2d(2 x 2, stride 2) + bias + ReLU + the 1 x 1 predictor row of each
RoI's class + sigmoid in one launch, against the float64 chain conv_transpose2d -> relu -> conv2d -> select -> sigmoid on the same
storage-rounded operands (no intermediate rounding).

Bound: B = max(32 * e32, 1e-5), e32 = the error of the same chain in torch-CPU fp32 against float64, computed here. Measured on the
CPU at R = 3, C = 256: e32 = 2.5e-7, so B = 1e-5; a kernel that rounded the (R, 28, 28, C) intermediate to fp16 would err by 1.7e-4.
The weights are drawn so that the logits have a standard deviation of at least 0.5 (asserted): detectron2's std = 0.001 predictor
initialiser would put every probability at 0.5 and make the comparison vacuous.

R = 1 (196 rows) ends in a partial tile; R = 3 (588 rows) has tile boundaries inside every RoI, for the 64-row tiles of the fp16 / bf16
kernel and the 32-row tiles of the fp32 one."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 14


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


@functools.lru_cache(maxsize=None)
def _operands(r: int, c: int, k: int, dt: torch.dtype):
    """x (r, S, S, c) and the deconv weight (c, c, 2, 2) rounded to dt; bias, predictor weight (k, c) and bias in fp32."""
    g = torch.Generator().manual_seed(1000 * r + c + k)
    x = torch.randn(r, S, S, c, generator=g).to(dt)
    w = (torch.randn(c, c, 2, 2, generator=g) * (2.0 / c) ** 0.5).to(dt)
    b = torch.randn(c, generator=g) * 0.1
    pw = torch.randn(k, c, generator=g) * (2.0 / c) ** 0.5
    pb = torch.randn(k, generator=g) * 0.1
    return x, w, b, pw, pb


def _chain(x, w, b, pw, pb, classes, dtype):
    """-> (probs (r, 2S, 2S), logits of the selected rows) in `dtype`; classes None: row 0."""
    xx = x.to(dtype).permute(0, 3, 1, 2)
    h = F.relu(F.conv_transpose2d(xx, w.to(dtype), b.to(dtype), stride=2))
    z = F.conv2d(h, pw.to(dtype)[:, :, None, None], pb.to(dtype))
    idx = torch.zeros(x.shape[0], dtype=torch.int64) if classes is None else classes.clamp(min=0)
    z = z[torch.arange(x.shape[0]), idx]
    return torch.sigmoid(z), z


@functools.lru_cache(maxsize=None)
def _reference(r: int, c: int, k: int, dt: torch.dtype, classes_key):
    ops_ = _operands(r, c, k, dt)
    classes = None if classes_key is None else torch.tensor(classes_key, dtype=torch.int64)
    ref, z = _chain(*ops_, classes, torch.float64)
    p32, _ = _chain(*ops_, classes, torch.float32)
    e32 = float((p32.double() - ref).abs().max())
    return ref, z, e32


def _run(ops, osr, r, c, k, dt, classes, rows_valid=None, seg_rows=0):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb = _operands(r, c, k, dt)
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV)
    rv = None if rows_valid is None else torch.tensor(rows_valid, dtype=torch.int32, device=DEV)
    return ops.mask_upsample_predict(x.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV), cl, rv, seg_rows)


def _classes_for(r: int, k: int):
    if k == 1:
        return None
    return {1: (k - 1,), 3: (0, k - 1, 2)}[r]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c", [256, 64])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("r", [1, 3])
def test_against_the_float64_chain(ops, osr, r, c, k, dt):
    classes = _classes_for(r, k)
    ref, z, e32 = _reference(r, c, k, dt, classes)
    assert float(z.std()) >= 0.5, f"the reference logits must spread (std {float(z.std()):.3f})"
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, r, c, k, dt, classes)
    assert out.shape == (r, 2 * S, 2 * S) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print(f"r={r} c={c} k={k} {dt}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}, logit std {float(z.std()):.3f}")
    assert err <= bound, f"max |probs - float64| {err:.3e} > {bound:.3e} (e32 {e32:.3e})"
    assert torch.equal(_run(ops, osr, r, c, k, dt, classes), out), "two runs are bit-identical"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [1, 5])
def test_no_rois(ops, osr, k, dt):
    out = _run(ops, osr, 0, 64, k, dt, None if k == 1 else ())
    assert out.shape == (0, 2 * S, 2 * S) and out.dtype == torch.float32


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [1, 5])
def test_padding_rows_and_class_minus_one_are_zeros(ops, osr, k, dt):
    """Six RoIs as two segments of three with rows_valid (2, 1): RoIs 2, 4 and 5 do not exist; RoI 1 exists with class -1. The four
    rows come out as exact zeros (their inputs are finite but arbitrary), the two live ones as the reference's."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    c = 256
    classes = (0, -1, 3, k - 1, 2, 1) if k > 1 else (0, -1, 0, 0, 0, 0)
    x, w, b, pw, pb = _operands(6, c, k, dt)
    live = [0, 3]
    ref, z, e32 = _reference(6, c, k, dt, classes)
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, 6, c, k, dt, classes, (2, 1), 3).cpu()
    for i in range(6):
        if i in live:
            err = float((out[i].double() - ref[i]).abs().max())
            assert err <= bound, (i, err, bound)
            assert float(out[i].min()) > 0.0
        else:
            assert float(out[i].abs().max()) == 0.0, f"RoI {i} must be zeros"
    # the same rows with non-finite inputs still come out as zeros: they are selected away, not multiplied away
    xn = x.clone()
    xn[[1, 2, 4, 5]] = float("nan")
    outn = ops.mask_upsample_predict(xn.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV),
                                     torch.tensor(classes, dtype=torch.int64, device=DEV), torch.tensor([2, 1], dtype=torch.int32, device=DEV), 3).cpu()
    assert torch.equal(outn, out)
    # without rows_valid only the class decides
    out2 = _run(ops, osr, 6, c, k, dt, classes).cpu()
    assert float(out2[1].abs().max()) == 0.0 and all(float(out2[i].min()) > 0.0 for i in (0, 2, 3, 4, 5))
    assert torch.equal(out2[live], out[live])


def test_a_lossy_intermediate_would_be_caught():
    """The bound tells the fused form from one that stores the deconv output in fp16: rounding h costs more than B (CPU only)."""
    x, w, b, pw, pb = _operands(3, 256, 1, torch.float16)
    ref, _, e32 = _reference(3, 256, 1, torch.float16, None)
    h = F.relu(F.conv_transpose2d(x.float().permute(0, 3, 1, 2), w.float(), b, stride=2)).half().float()
    lossy = torch.sigmoid(F.conv2d(h, pw[:, :, None, None], pb))[:, 0]
    assert float((lossy.double() - ref).abs().max()) > 4 * max(32 * e32, 1e-5)


def test_shape_rules(ops, osr):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb = [t.to(DEV) if i != 1 else t for i, t in enumerate(_operands(1, 64, 5, torch.float16))]
    wp = pack_deconv_weight(w, torch.float16).to(DEV)
    with pytest.raises(osr.OsrError, match="classes"):  # a class-specific predictor needs the classes
        ops.mask_upsample_predict(x, wp, b, pw, pb, None)
    with pytest.raises(osr.OsrError, match="multiples of 64"):
        ops.mask_upsample_predict(x[..., :32].contiguous(), wp[:, :, :2].contiguous(), b, pw, pb, torch.zeros(1, dtype=torch.int64, device=DEV))
