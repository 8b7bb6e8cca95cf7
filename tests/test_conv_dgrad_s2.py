"""GPU parity of the stride-2 3x3 layers that MODEL.RESNETS.STRIDE_IN_1X1 False puts in the first block of res3-res5:
the backward-data kernel of its own (osr_conv2d_dgrad_s2: four pixel-parity phases in one launch), and the forward / weight
gradient of that layer shape, against torch on the CPU (fp32 on the same fp16- / bf16-rounded operands). Tolerance as
tests/test_conv_bwd.py: 2e-3 of the tensor's max with an fp32 dx (bf16 storage rounds to 2^-8, so its stored dx gets 1e-2)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PRODUCTION = [  # n, cin, cout, hi, wi: res3.0 / res4.0 / res5.0 conv2 at batch 16 on the 800 x 1344 pad
    (16, 128, 128, 200, 336),
    (16, 256, 256, 100, 168),
    (16, 512, 512, 50, 84),
]
SMALL = [
    (2, 64, 64, 7, 9),     # odd input sizes: the odd phases lack their last row / column of taps
    (2, 64, 64, 8, 10),    # even input sizes
    (1, 128, 128, 13, 17),  # batch 1
    (2, 192, 128, 9, 11),  # cin != cout, partial input-channel tile
    (2, 64, 256, 8, 10),   # cin != cout
    (1, 48, 64, 1, 5),     # one input row: the odd-row phases are empty; 48 channels leave a wave's last 16 idle
]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-6))


def operands(n, cin, cout, hi, wi, dtype, seed):
    """dy, w (rounded to dtype, kept fp32 on the CPU), the fp32 reference dx (NHWC), and an activation / addend of dx's shape."""
    gg = torch.Generator().manual_seed(seed)
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    w = (torch.randn(cout, cin, 3, 3, generator=gg) * 0.05).to(dtype).float()
    dy = torch.randn(n, cout, ho, wo, generator=gg).to(dtype).float()
    ref = nhwc(torch.nn.grad.conv2d_input((n, cin, hi, wi), w, dy, stride=2, padding=1))
    act = torch.randn(n, hi, wi, cin, generator=gg).to(dtype)
    other = torch.randn(n, hi, wi, cin, generator=gg).to(dtype)
    return w, dy, ref, act, other


def run_abi(osr, ops, dyd, wd, hi, wi, mask, add, out):
    """osr_conv2d_dgrad_s2 straight through the C ABI into a caller-given dx (so that its prior contents are visible)."""
    n, ho, wo, cout = dyd.shape
    cin = wd.shape[0]
    p = ops._conv_params(n, hi, wi, cin, ho, wo, cout, 3, 3, 2, 1, dyd.dtype, out.dtype)
    st = osr._lib.load().osr_conv2d_dgrad_s2(ctypes.byref(p), ops._p(dyd), ops._p(wd), ops._p(mask), ops._p(add), ops._p(out), ops._stream())
    ops.check(st, "osr_conv2d_dgrad_s2")
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n,cin,cout,hi,wi", SMALL)
def test_dgrad_s2_small(ops, osr, n, cin, cout, hi, wi, dtype):
    from openset_rcnn_amd.host.weights import pack_dgrad_weight
    w, dy, ref, act, other = operands(n, cin, cout, hi, wi, dtype, cin * 7 + cout + hi * wi)
    wd = pack_dgrad_weight(w, dtype).to(DEV)
    dyd = nhwc(dy).to(dtype).to(DEV)
    actd, otherd = act.to(DEV), other.to(DEV)
    keep = (act.float() > 0).float()
    # fp32 dx: plain, masked, with an addend, and both (mask after the sum)
    dx = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, out_dtype=torch.float32)
    assert dx.shape == (n, hi, wi, cin)
    assert rel(dx, ref) < 2e-3, rel(dx, ref)
    dxm = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, mask=actd, out_dtype=torch.float32)
    assert rel(dxm, ref * keep) < 2e-3
    dxa = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, add=otherd, out_dtype=torch.float32)
    assert rel(dxa, ref + other.float()) < 2e-3
    dxb = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, add=otherd, post_mask=actd, out_dtype=torch.float32)
    assert rel(dxb, (ref + other.float()) * keep) < 2e-3
    # storage-dtype dx, the training step's form
    dxs = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, mask=actd)
    assert dxs.dtype == dtype
    assert rel(dxs, ref * keep) < (2e-3 if dtype == torch.float16 else 1e-2)
    # every pixel written: a NaN-filled dx has none left, and a second run gives the same bits
    for out_dtype in (dtype, torch.float32):
        out = torch.full((n, hi, wi, cin), float("nan"), dtype=out_dtype, device=DEV)
        run_abi(osr, ops, dyd, wd, hi, wi, actd, otherd, out)
        assert not torch.isnan(out).any(), "osr_conv2d_dgrad_s2 left pixels of dx unwritten"
        again = torch.full_like(out, float("nan"))
        run_abi(osr, ops, dyd, wd, hi, wi, actd, otherd, again)
        assert torch.equal(out, again)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n,cin,cout,hi,wi", PRODUCTION, ids=["res3", "res4", "res5"])
def test_dgrad_s2_production(ops, osr, n, cin, cout, hi, wi, dtype):
    from openset_rcnn_amd.host.weights import pack_dgrad_weight
    w, dy, ref, act, other = operands(n, cin, cout, hi, wi, dtype, cin + hi)
    wd = pack_dgrad_weight(w, dtype).to(DEV)
    dyd = nhwc(dy).to(dtype).to(DEV)
    dx = ops.conv2d_dgrad(dyd, wd, (hi, wi), 2, 1, out_dtype=torch.float32)
    assert rel(dx, ref) < 2e-3, rel(dx, ref)
    del dx
    actd, otherd = act.to(DEV), other.to(DEV)
    out = torch.full((n, hi, wi, cin), float("nan"), dtype=dtype, device=DEV)
    run_abi(osr, ops, dyd, wd, hi, wi, actd, otherd, out)
    assert not torch.isnan(out).any(), "osr_conv2d_dgrad_s2 left pixels of dx unwritten"
    want = (ref + other.float()) * (act.float() > 0)
    assert rel(out, want) < (2e-3 if dtype == torch.float16 else 1e-2)
    again = torch.empty_like(out)
    run_abi(osr, ops, dyd, wd, hi, wi, actd, otherd, again)
    assert torch.equal(out, again), "repeated runs must be bit-identical"


def test_dgrad_s2_refuses_unsupported_shapes(ops):
    from openset_rcnn_amd.host.ops import OsrError
    dy = torch.zeros(1, 4, 5, 96, dtype=torch.float16, device=DEV)  # cout 96: not a multiple of 64
    wd = torch.zeros(64, 3, 3, 96, dtype=torch.float16, device=DEV)
    with pytest.raises(OsrError, match="cout a multiple of 64"):
        ops.conv2d_dgrad(dy, wd, (8, 9), 2, 1)
    with pytest.raises(OsrError, match="inconsistent"):
        ops.conv2d_dgrad(dy, wd, (10, 9), 2, 1)


@pytest.mark.parametrize("n,cin,cout,hi,wi", PRODUCTION, ids=["res3", "res4", "res5"])
def test_stride2_3x3_forward_and_wgrad_production(ops, n, cin, cout, hi, wi):
    """The forward (osr_conv2d_fwd) and the weight gradient (osr_conv2d_wgrad) of the same layers: their address arithmetic takes
    any stride; here at the shapes the stride-in-3x3 layout trains."""
    gg = torch.Generator().manual_seed(hi + cin)
    x = torch.randn(n, cin, hi, wi, generator=gg).half().float()
    w = (torch.randn(cout, cin, 3, 3, generator=gg) * 0.05).half().float()
    b = torch.randn(cout, generator=gg) * 0.1
    xd = nhwc(x).half().to(DEV)
    y = ops.conv2d(xd, nhwc(w).half().to(DEV), b.to(DEV), 2, 1, relu=False, out_dtype=torch.float32)
    ref = nhwc(F.conv2d(x, w, b, 2, 1))
    assert rel(y, ref) < 2e-3, rel(y, ref)
    del y, ref
    dy = torch.randn(n, cout, (hi - 1) // 2 + 1, (wi - 1) // 2 + 1, generator=gg).half().float()
    dw = ops.conv2d_wgrad(xd, nhwc(dy).half().to(DEV), 3, 3, 2, 1)
    ref_w = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=2, padding=1)
    assert rel(dw.permute(0, 3, 1, 2), ref_w) < 2e-3, rel(dw.permute(0, 3, 1, 2), ref_w)


def test_res3_chain_at_stride2_production(ops):
    """res3.0's conv2 (3x3, stride 2 with the stride in the 3x3) -> conv3 + shortcut as the one chained launch the engine and the
    training step use, against two CPU convolutions; the stored conv2 output too."""
    n, hi, wi = 16, 200, 336
    gg = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(n, 128, hi, wi, generator=gg)).half().float()
    w2 = (torch.randn(128, 128, 3, 3, generator=gg) * 0.05).half().float()
    b2 = torch.randn(128, generator=gg) * 0.1
    w3 = (torch.randn(512, 128, 1, 1, generator=gg) * 0.05).half().float()
    b3 = torch.randn(512, generator=gg) * 0.1
    sc = torch.randn(n, 512, 100, 168, generator=gg).half().float()
    mid = torch.relu(F.conv2d(x, w2, b2, 2, 1))
    ref = torch.relu(F.conv2d(mid.half().float(), w3, b3) + sc)
    res = ops.conv2d_chain(nhwc(x).half().to(DEV), nhwc(w2).half().to(DEV), b2.to(DEV), nhwc(w3).half().to(DEV), b3.to(DEV),
                           nhwc(sc).half().to(DEV), 2, 1, keep_mid=True)
    assert res is not None, "the chained launch refused the stride-2 shape"
    y, m = res
    assert rel(m, nhwc(mid)) < 2e-3
    assert rel(y, nhwc(ref)) < 2e-3
