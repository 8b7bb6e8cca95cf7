"""The stem's backward kernels (csrc/osr_stem_bwd.hip) against fp64 torch on the same fp16 inputs.

osr_stem_pool_bwd is checked against the gradient of F.max_pool2d(3, 2, 1) on the kernel's own stem output (so the windows' maxima,
ties and NaNs are the same ones), times the ReLU's mask (output <= 0: no gradient). osr_stem_wgrad is checked against F.conv2d's weight
gradient in fp64 over the same fp16 image and fp16 stem-output gradient. Its products are exact in fp32 (fp16 x fp16), so the error is
the fp32 summation over up to 4.3 M pixels in 512 fixed ranges. Bound: 2e-4 of max|ref|. A fp32 sum of N terms has relative error
<= N * 2^-24 in the worst case. Over one range of <= 8 400 terms plus 512 partials that is about 5e-4 of the sum of |terms|; with random
signs the observed error is far below that.
The training forward keeps the stem output (osr_conv2d_fwd stem view + osr_maxpool3x3s2): its pooled output must be the fused
osr_stem_maxpool_fwd_raw's, bit for bit, so that training and evaluation see the same res2 input."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (103.53, 116.28, 123.675), (1.0, 1.0, 1.0)


def _stem_view(seed, bias_shift=0.0):
    from openset_rcnn_amd.host.weights import pack_stem_weight
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.02
    b = torch.randn(64, generator=g) * 0.5 + bias_shift
    return pack_stem_weight(w, torch.float16).to(DEV), b.float().to(DEV)


def _forward(osr, images, hp, wp, view, bias):
    from openset_rcnn_amd.host import ops
    xpad = ops.preprocess(images, hp, wp, MEAN, STD, torch.float16)
    s = ops.stem_conv(xpad, view, bias, hp, wp, relu=True)
    return ops, xpad, s, ops.maxpool3x3s2(s)


def _pool_ref(s, dpool):
    """fp64 gradient of relu's output through max_pool2d (torch indices), masked where s <= 0 (torch's threshold_backward)."""
    s64 = s.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    out = F.max_pool2d(s64, 3, 2, 1)
    out.backward(dpool.permute(0, 3, 1, 2).double().cpu())
    g = s64.grad.permute(0, 2, 3, 1)
    return torch.where(s.double().cpu() <= 0, torch.zeros_like(g), g)


def _wgrad_ref(xpad, ds, hp, wp):
    xin = xpad[:, 3:hp + 3, 3:wp + 3, :3].permute(0, 3, 1, 2).double().cpu()
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xin, w, None, 2, 3)
    y.backward(ds.permute(0, 3, 1, 2).double().cpu())
    return w.grad


def _unpack(dw):
    v = dw.view(64, 8, 8, 4)
    assert float(v[:, 7].abs().max()) == 0, "8th row"
    assert float(v[:, :, 7].abs().max()) == 0, "8th tap"
    assert float(v[..., 3].abs().max()) == 0, "4th channel"
    return v[:, :7, :7, :3].permute(0, 3, 1, 2).double().cpu()


def _check_wgrad(ops, xpad, ds, hp, wp, bound=2e-4):
    dw = ops.stem_wgrad(xpad, ds, hp, wp)
    dw2 = ops.stem_wgrad(xpad, ds, hp, wp)
    assert torch.equal(dw, dw2), "repeats must be bit-identical"
    got, ref = _unpack(dw), _wgrad_ref(xpad, ds, hp, wp)
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    print(f"stem wgrad {tuple(ds.shape)}: max err {err:.2e} of max|ref| {float(ref.abs().max()):.3e}")
    assert err <= bound, err
    return dw


def test_full_resolution_image(osr):
    g = torch.Generator().manual_seed(1)
    hp, wp = 800, 1344
    images = torch.randint(0, 256, (1, 3, 800, 1333), generator=g, dtype=torch.uint8).to(DEV)
    view, bias = _stem_view(2)
    ops, xpad, s, pooled = _forward(osr, images, hp, wp, view, bias)
    fused = ops.stem_maxpool_raw(images, hp, wp, MEAN, STD, view, bias)
    assert torch.equal(pooled, fused), "the training forward's pooled output must be the fused kernel's"
    dpool = (torch.randn(pooled.shape, generator=g) * 4).half().to(DEV)
    ds = ops.stem_pool_bwd(s, dpool)
    assert torch.equal(ds, ops.stem_pool_bwd(s, dpool))
    ref = _pool_ref(s, dpool)
    # fp32 sums of <= 4 fp16 values rounded once to fp16, against fp64 rounded nowhere: within one fp16 rounding
    torch.testing.assert_close(ds.double().cpu(), ref, rtol=1e-3, atol=1e-3)
    assert bool(((ds.cpu() == 0) | (s.cpu() > 0)).all()), "no gradient where the stem output is <= 0"
    _check_wgrad(ops, xpad, ds, hp, wp)


def test_tied_maxima_and_all_nonpositive_windows(osr):
    """A flat image gives a constant stem output inside the image (every window a tie: the first position wins); a strongly negative
    bias makes every stem output 0 (every window <= 0: no gradient anywhere, a zero weight gradient)."""
    hp, wp = 64, 96
    images = torch.full((2, 3, 64, 90), 117, dtype=torch.uint8)
    images[1, :, 20:40, 30:50] = 200
    images = images.to(DEV)
    view, bias = _stem_view(3)
    ops, xpad, s, pooled = _forward(osr, images, hp, wp, view, bias)
    dpool = (torch.randn(pooled.shape, generator=torch.Generator().manual_seed(4)) * 4).half().to(DEV)
    ds = ops.stem_pool_bwd(s, dpool)
    torch.testing.assert_close(ds.double().cpu(), _pool_ref(s, dpool), rtol=1e-3, atol=1e-3)
    _check_wgrad(ops, xpad, ds, hp, wp)
    view, bias = _stem_view(3, bias_shift=-1e4)
    ops, xpad, s, pooled = _forward(osr, images, hp, wp, view, bias)
    assert float(s.abs().max()) == 0
    ds = ops.stem_pool_bwd(s, dpool)
    assert float(ds.abs().max()) == 0
    assert float(ops.stem_wgrad(xpad, ds, hp, wp).abs().max()) == 0


def test_pool_backward_with_ties_and_nan(osr):
    """Synthetic stem outputs of small integers (many ties), zeros, negatives and NaNs: the kernel follows torch's max_pool2d indices
    (a NaN wins its window, the last NaN of a window wins) and passes the gradient at a NaN output (threshold_backward)."""
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(5)
    s = torch.randint(-2, 4, (2, 37, 51, 64), generator=g).float()
    nan_at = torch.rand(s.shape, generator=g) < 0.02
    s[nan_at] = float("nan")
    s = s.half().to(DEV)
    ho, wo = (37 - 1) // 2 + 1, (51 - 1) // 2 + 1
    dpool = (torch.randn(2, ho, wo, 64, generator=g) * 3).half().to(DEV)
    ds = ops.stem_pool_bwd(s, dpool)
    assert torch.equal(ds, ops.stem_pool_bwd(s, dpool))
    torch.testing.assert_close(ds.double().cpu(), _pool_ref(s, dpool), rtol=1e-3, atol=1e-3, equal_nan=True)
    assert bool((ds.cpu()[nan_at.view(ds.shape)] != 0).any()), "NaN outputs that win a window pass the gradient"


def test_batch16_weight_gradient_is_deterministic(osr):
    """Production size (16 x 800 x 1344: 4.3 M stem pixels): repeats bit-identical, finite, padding exactly zero, and equal to the
    per-image gradients' sum within the summation bound."""
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(6)
    hp, wp, n = 800, 1344, 16
    images = torch.randint(0, 256, (n, 3, hp, wp), generator=g, dtype=torch.uint8).to(DEV)
    xpad = ops.preprocess(images, hp, wp, MEAN, STD, torch.float16)
    ds = torch.randn((n, hp // 2, wp // 2, 64), generator=torch.Generator().manual_seed(7)).half().to(DEV)
    dw = ops.stem_wgrad(xpad, ds, hp, wp)
    assert torch.equal(dw, ops.stem_wgrad(xpad, ds, hp, wp))
    assert bool(torch.isfinite(dw).all())
    _unpack(dw)
    acc = torch.zeros_like(dw)
    for i in range(0, n, 4):
        ops.stem_wgrad(xpad[i:i + 4], ds[i:i + 4], hp, wp, dw=acc, accumulate=i > 0)
    err = float((acc - dw).abs().max()) / float(dw.abs().max())
    print(f"batch-16 stem wgrad: whole batch vs four accumulated quarters {err:.2e} of max|dW|")
    assert err <= 2e-4, err
