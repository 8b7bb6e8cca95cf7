"""The split-precision convolution (ops.conv2d_split / ops.stem_conv_split -> osr_conv2d_split_fwd, csrc/osr_conv_split.hip) on the GPU.

Errors are e(y) = max|y - y64| / max|y64|, y64 = the same layer by torch on the CPU in float64 from the identical fp32 inputs.
  A: e(split) <= 1e-4                       (the bar tests/test_e2e_parity.py applies to the parity mode's dense stages)
  B: e(split) <= max(32 e(f32), 1e-5)       e(f32) = the error of the existing fp32 kernel (ops.conv2d on fp32 tensors) on the same
                                            inputs in the same test
The shapes are the smallest that reach every edge of the 128 x 128 x 32 tile: a partial row tile, a second row tile of two rows, odd
output sizes under stride 2, cout 64 (the narrow tile) and cout 192 (a partial last column tile). Every test also checks that its
launches went to osr_conv2d_split_fwd (ops.CONV_SPLIT_COUNT)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A_BOUND = 1e-4


def b_bound(e_f32):
    return max(32.0 * e_f32, 1e-5)


def err(y, y64):
    return float((y.detach().cpu().double() - y64).abs().max() / y64.abs().max())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


@pytest.fixture()
def counted(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    osr.ops.CONV_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    yield osr.ops.CONV_SPLIT_COUNT
    osr.ops.CONV_SPLIT_COUNT = None


def _check_a_b(tag, ys, yf, y64):
    e_s, e_f = err(ys, y64), err(yf, y64)
    print(f"\n[{tag}] e(split) {e_s:.3e}  e(f32) {e_f:.3e}  ratio {e_s / max(e_f, 1e-30):.1f}  B bound {b_bound(e_f):.3e}")
    assert e_s <= A_BOUND, (tag, e_s)
    assert e_s <= b_bound(e_f), (tag, e_s, e_f)


def _layer(k, cin, cout, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g).clamp(min=0) * torch.exp(torch.randn(n, 1, h, w, generator=g) * 0.7)  # post-ReLU pixels of mixed size
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.02
    return x, wt, b


CASES = [
    # id,              k, stride, pad, cin,  cout, n, h, w,  relu,  res_mode
    ("1x1_64_64",      1, 1, 0, 64,   64,  1, 5, 7,  False, 0),
    ("1x1s2_256_128",  1, 2, 0, 256,  128, 1, 9, 11, False, 0),
    ("3x3_64_64_relu", 3, 1, 1, 64,   64,  1, 6, 5,  True,  0),
    ("3x3s2_128_128",  3, 2, 1, 128,  128, 1, 9, 10, False, 0),
    ("1x1_2048_256",   1, 1, 0, 2048, 256, 2, 5, 13, False, 0),  # 130 rows: one full row tile and a second holding two rows
    ("1x1_64_192",     1, 1, 0, 64,   192, 1, 4, 8,  False, 0),
    ("1x1_128_512_r1", 1, 1, 0, 128,  512, 1, 7, 9,  True,  1),
    ("1x1_512_256_r2", 1, 1, 0, 512,  256, 1, 7, 9,  False, 2),
    ("3x3_64_64_r3",   3, 1, 1, 64,   64,  1, 6, 5,  False, 3),
]


@pytest.mark.parametrize("k,stride,pad,cin,cout,n,h,w,relu,res_mode", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_a_and_b_at_the_tile_edges(osr, counted, k, stride, pad, cin, cout, n, h, w, relu, res_mode):
    from openset_rcnn_amd.host.weights import pack_conv_weight, split_conv_weight
    ops = osr.ops
    x, wt, b = _layer(k, cin, cout, n, h, w, 1000 + cin + cout + k + stride)
    y64 = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=pad)
    ho, wo = y64.shape[2:]
    res = None
    if res_mode:
        g = torch.Generator().manual_seed(9)
        res = torch.randn((n, cout, ho, wo) if res_mode != 2 else (n, cout, (ho + 1) // 2, (wo + 1) // 2), generator=g)
        if res_mode == 1:
            y64 = y64 + res.double()
        elif res_mode == 2:
            y64 = y64 + F.interpolate(res.double(), scale_factor=2, mode="nearest")[:, :, :ho, :wo]
        else:
            y64 = torch.where(res > 0, y64, torch.zeros_like(y64))
    if relu:
        y64 = y64.clamp(min=0)
    xd, bd = nhwc(x).to(DEV), b.to(DEV)
    rd = None if res is None else nhwc(res).to(DEV)
    ws = tuple(t.to(DEV) for t in split_conv_weight(wt))
    ys = ops.conv2d_split(xd, ws, bd, stride, pad, relu, rd, res_mode)
    ys2 = ops.conv2d_split(xd, ws, bd, stride, pad, relu, rd, res_mode)
    yf = ops.conv2d(xd, pack_conv_weight(wt, torch.float32).to(DEV), bd, stride, pad, relu, rd, res_mode)
    torch.cuda.synchronize()
    assert counted["launches"] == 2 and counted["flops"] == 2 * 2.0 * n * ho * wo * cout * k * k * cin
    assert ys.dtype == torch.float32 and tuple(ys.shape) == (n, ho, wo, cout)
    assert torch.equal(ys, ys2)  # bit-identical on a second launch
    if res_mode == 3:
        assert bool((nchw(ys)[res <= 0] == 0).all())
    _check_a_b(f"conv2d_split {k}x{k} s{stride} {cin} -> {cout}, {n}x{h}x{w}, res_mode {res_mode}", nchw(ys), nchw(yf), y64)


def test_stem_view_against_the_7x7_convolution(osr, counted):
    from openset_rcnn_amd.host.weights import pack_stem_weight, split_stem_weight
    ops = osr.ops
    g = torch.Generator().manual_seed(31)
    img = torch.randn(2, 3, 32, 64, generator=g) * 60.0
    wt = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    b = torch.randn(64, generator=g) * 0.02
    y64 = F.conv2d(img.double(), wt.double(), b.double(), stride=2, padding=3).clamp(min=0)
    xpad = ops.preprocess(img.to(DEV), 32, 64, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dtype=torch.float32)  # (the pixels pass unchanged)
    ws = tuple(t.to(DEV) for t in split_stem_weight(wt))
    ys = ops.stem_conv_split(xpad, ws, b.to(DEV), 32, 64, relu=True)
    yf = ops.stem_conv(xpad, pack_stem_weight(wt, torch.float32).to(DEV), b.to(DEV), 32, 64, relu=True)
    torch.cuda.synchronize()
    assert counted["launches"] == 1 and counted["flops"] == 2.0 * 2 * 16 * 32 * 64 * 147
    assert tuple(ys.shape) == (2, 16, 32, 64)
    _check_a_b("stem_conv_split 3x32x64", nchw(ys), nchw(yf), y64)


@pytest.mark.parametrize("stride", [1, 2])
def test_border_taps_contribute_exactly_zero(osr, counted, stride):
    """x = 1, w = 2^-6, cin 64: an output is its number of taps inside the image, exactly (every term and every sum is a small integer
    over a power of two: nothing rounds)."""
    from openset_rcnn_amd.host.weights import split_conv_weight
    x = torch.ones(1, 4, 5, 64)
    wt = torch.full((64, 64, 3, 3), 2.0 ** -6)
    ws = tuple(t.to(DEV) for t in split_conv_weight(wt))
    y = osr.ops.conv2d_split(x.to(DEV), ws, torch.zeros(64, device=DEV), stride, 1).cpu()
    taps = F.conv2d(torch.ones(1, 1, 4, 5), torch.ones(1, 1, 3, 3), stride=stride, padding=1)[0, 0]  # valid taps per output pixel
    assert torch.equal(y, taps.view(1, *taps.shape, 1).expand_as(y).contiguous())
    if stride == 1:
        assert float(y[0, 0, 0, 0]) == 4.0 and float(y[0, 0, 2, 5]) == 6.0 and float(y[0, 2, 0, 63]) == 6.0 and float(y[0, 1, 3, 17]) == 9.0
        assert float(y[0, 3, 4, 0]) == 4.0
    assert counted["launches"] == 1


def test_mixed_magnitudes_meet_b_block_by_block(osr, counted):
    """Pixels scaled by 2^-20 .. 2^20, one power per 32 output rows: bf16 terms carry fp32's exponent, so each block on its own is as
    accurate as any other (160 rows: a full row tile and a partial one)."""
    from openset_rcnn_amd.host.weights import pack_conv_weight, split_conv_weight
    ops = osr.ops
    x, wt, _ = _layer(1, 128, 128, 1, 10, 16, 77)
    powers = [-20, -7, 0, 9, 20]
    scale = torch.tensor([2.0 ** p for p in powers]).repeat_interleave(32).view(1, 1, 10, 16)
    x = x * scale
    b = torch.zeros(128)
    y64 = F.conv2d(x.double(), wt.double())
    xd = nhwc(x).to(DEV)
    ys = nchw(ops.conv2d_split(xd, tuple(t.to(DEV) for t in split_conv_weight(wt)), b.to(DEV)))
    yf = nchw(ops.conv2d(xd, pack_conv_weight(wt, torch.float32).to(DEV), b.to(DEV)))
    rows = lambda t, i: t.permute(0, 2, 3, 1).reshape(160, 128)[32 * i:32 * i + 32]  # noqa: E731
    for i, p in enumerate(powers):
        _check_a_b(f"rows scaled by 2^{p}", rows(ys, i), rows(yf, i), rows(y64, i))


def test_an_image_does_not_depend_on_its_batch(osr, counted):
    from openset_rcnn_amd.host.weights import split_conv_weight
    ops = osr.ops
    x, wt, b = _layer(3, 64, 128, 3, 6, 7, 55)
    xd, bd = nhwc(x).to(DEV), b.to(DEV)
    ws = tuple(t.to(DEV) for t in split_conv_weight(wt))
    y3 = ops.conv2d_split(xd, ws, bd, 1, 1, True)
    y3b = ops.conv2d_split(xd, ws, bd, 1, 1, True)
    y1 = ops.conv2d_split(xd[:1].contiguous(), ws, bd, 1, 1, True)
    torch.cuda.synchronize()
    assert torch.equal(y3, y3b)
    assert torch.equal(y3[:1], y1)
    assert counted["launches"] == 3


def test_refusals(osr, counted):
    from openset_rcnn_amd.host.weights import split_conv_weight
    ops = osr.ops
    planes = lambda cout, cin, k=1: tuple(t.to(DEV) for t in split_conv_weight(torch.zeros(cout, cin, k, k)))  # noqa: E731
    with pytest.raises(osr.OsrError):
        ops.conv2d_split(torch.zeros(1, 4, 4, 48, device=DEV), planes(64, 48), torch.zeros(64, device=DEV))
    with pytest.raises(osr.OsrError):
        ops.conv2d_split(torch.zeros(1, 4, 4, 64, device=DEV), planes(96, 64), torch.zeros(96, device=DEV))
    with pytest.raises(osr.OsrError):
        ops.conv2d_split(torch.zeros(1, 8, 8, 64, device=DEV), planes(64, 64, 5), torch.zeros(64, device=DEV), pad=2)  # 5x5: not a shape it takes
    with pytest.raises(osr.OsrError):
        ops.conv2d_split(torch.zeros(1, 4, 4, 64), planes(64, 64), torch.zeros(64, device=DEV))  # a CPU tensor
    with pytest.raises(osr.OsrError):
        ops.conv2d_split(torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.float16), planes(64, 64), torch.zeros(64, device=DEV))
    assert counted["launches"] == 0
