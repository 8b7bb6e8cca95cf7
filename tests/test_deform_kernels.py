"""osr_deform_cols (the gather of a 3x3 deformable convolution) and ops.deform_conv2d against a float64 restatement of the definition in
include/osr.h, written here with index arithmetic and torch.gather. Shapes: n = 2, c = 64, maps of 5 x 7 and 6 x 8 (odd and even, so
stride 2 meets both edge cases; 2 x 35 x 9 x 8 = 5040 work items: ten 256-lane blocks at two items per lane, one trip round the
kernel's loop each). The last test runs 6,451,200 items, more than three steps of the grid capped at 8192 blocks: a second trip.

Bounds. u = 2^-24 (fp32 unit roundoff), S = the sum of |weight * value * m| over the four corners of one sample.
  gather: |err| <= 6 u S + half_ulp(ref, dtype). The kernel never rounds a sample position (the cell and the fraction come from the fp32
          offset alone, exactly), so what is left is the four products, the three sums and the mask multiply in fp32 and one rounding
          to the storage dtype.
  layer:  |err| <= (9 c + 2) u S + half_ulp(ref, dtype), S over all 9 c products and the bias: the bound of tests/test_conv_fwd_plans.py
          for a K = 9 c contraction. Its reference multiplies the GPU's own (already rounded, separately checked) cols, so the gather's
          storage rounding is not counted twice."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
DT_IDS = ["fp16", "bf16", "fp32"]
MAPS = ((5, 7), (6, 8))
U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from openset_rcnn_amd.host import ops as o
    o._lib.load()
    return o


def _half_ulp(v, dt):
    if dt == F32:
        return torch.zeros_like(v)
    bits = 11 if dt == F16 else 8
    return torch.maximum(v.abs() * 2.0 ** -bits, torch.full_like(v, 2.0 ** -25 if dt == F16 else 0.0))


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def offset_channels(groups, modulated):
    return (27 if modulated else 18) * groups


def ref_cols(x, om, stride, groups, modulated):
    """float64: (cols (n*ho*wo, 9, c), S of the same shape). x (n,h,w,c), om (n,ho,wo,ch >= 18 G or 27 G) fp32."""
    n, h, w, c = x.shape
    ho, wo = om.shape[1:3]
    G, cg, dev = groups, c // groups, x.device
    off = om[..., :18 * G].double().view(n, ho, wo, G, 9, 2)
    k = torch.arange(9, device=dev)
    hs = (torch.arange(ho, device=dev).view(1, ho, 1, 1, 1) * stride - 1 + (k // 3).view(1, 1, 1, 1, 9)).double() + off[..., 0]
    ws = (torch.arange(wo, device=dev).view(1, 1, wo, 1, 1) * stride - 1 + (k % 3).view(1, 1, 1, 1, 9)).double() + off[..., 1]
    m = torch.sigmoid(om[..., 18 * G:27 * G].double().view(n, ho, wo, G, 9)) if modulated else torch.ones_like(hs)
    valid = (hs > -1) & (ws > -1) & (hs < h) & (ws < w)  # False for NaN
    hs, ws = torch.where(valid, hs, torch.zeros_like(hs)), torch.where(valid, ws, torch.zeros_like(ws))
    h0, w0 = hs.floor(), ws.floor()
    lh, lw = hs - h0, ws - w0
    xg = x.double().view(n, h * w, G, cg).permute(0, 2, 1, 3)  # (n, G, h*w, cg)
    out = torch.zeros((n, ho, wo, G, 9, cg), dtype=torch.float64, device=dev)
    S = torch.zeros_like(out)
    for a, b, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hy, wx = h0.long() + a, w0.long() + b
        ok = valid & (hy >= 0) & (hy <= h - 1) & (wx >= 0) & (wx <= w - 1)
        idx = (hy.clamp(0, h - 1) * w + wx.clamp(0, w - 1)).permute(0, 3, 1, 2, 4).reshape(n, G, ho * wo * 9, 1)
        v = torch.gather(xg, 2, idx.expand(-1, -1, -1, cg)).view(n, G, ho, wo, 9, cg).permute(0, 2, 3, 1, 4, 5)
        term = torch.where(ok, wt * m, torch.zeros_like(wt)).unsqueeze(-1) * v
        out += term
        S += term.abs()
    to_cols = lambda t: t.permute(0, 1, 2, 4, 3, 5).reshape(n * ho * wo, 9, c)  # noqa: E731
    return to_cols(out), to_cols(S)


def im2col(x, stride):
    """(n,h,w,c) -> (n*ho*wo, 9, c): the 3x3 / pad 1 taps of the zero-padded input, x's dtype, no arithmetic."""
    n, h, w, c = x.shape
    ho, wo = out_hw(h, w, stride)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride] for i in range(3) for j in range(3)]
    return torch.stack(taps, 3).reshape(n * ho * wo, 9, c)


def _x(shape, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV).to(dt)


def _padded_om(om):
    """om with its channel count padded to the next multiple of 8 by NaN: the row pitch the engine hands over; the padding is never read."""
    ch = om.shape[-1]
    pad = (ch + 7) // 8 * 8 + 8 - ch
    return torch.cat((om, torch.full(om.shape[:-1] + (pad,), NAN, device=om.device)), -1).contiguous()


def _check(got, ref, S, dt, what, factor=6):
    got = got.double()
    assert bool(torch.isfinite(got).all()), what
    tol = factor * U * S + _half_ulp(ref, dt)
    err = (got - ref).abs()
    ratio = float((err / tol.clamp(min=1e-300)).max())
    print(f"[err] {what}: max |err| {float(err.max()):.3e}, max |err| / bound {ratio:.3e}")
    assert bool((got[ref == 0] == 0).all()), f"{what}: a sample the rule makes zero is not zero"
    assert ratio <= 1.0, f"{what}: |err| / bound {ratio:.3e} > 1"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("stride", [1, 2])
def test_zero_offsets_are_im2col(ops, stride, groups, dt):
    for h, w in MAPS:
        x = _x((2, h, w, 64), dt, 10 + h)
        ho, wo = out_hw(h, w, stride)
        om = _padded_om(torch.zeros((2, ho, wo, offset_channels(groups, False)), device=DEV))
        cols = ops.deform_cols(x, om, stride, groups, False)
        assert cols.shape == (2 * ho * wo, 9, 64) and cols.dtype == dt
        assert torch.equal(cols, im2col(x, stride)), (h, w)
        # modulated, zero logits: m = sigmoid(0) = 1/2 exactly; 0.5 x in fp32 is exact, rounded once to the storage dtype
        om = _padded_om(torch.zeros((2, ho, wo, offset_channels(groups, True)), device=DEV))
        cols = ops.deform_cols(x, om, stride, groups, True)
        assert torch.equal(cols, im2col((0.5 * x.float()).to(dt), stride)), (h, w, "modulated")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("stride", [1, 2])
def test_integer_offsets_shift_and_leave_the_map(ops, stride, dt):
    for h, w in MAPS:
        x = _x((2, h, w, 64), dt, 20 + h)
        ho, wo = out_hw(h, w, stride)
        g = torch.Generator(device=DEV).manual_seed(21 + w)
        om = torch.randint(-4, 5, (2, ho, wo, 36), generator=g, device=DEV).float()
        cols = ops.deform_cols(x, _padded_om(om), stride, 2, False)
        ref, _ = ref_cols(x, om, stride, 2, False)  # every weight is 0 or 1: the float64 value is one of x's own, or 0
        assert torch.equal(cols, ref.to(dt)), (h, w)
        outside = float((ref == 0).double().mean())
        assert 0.2 < outside < 0.95, outside  # shifts that leave the map are there, and so are shifts that stay
        # one uniform shift, against plain loops: tap (i, j) of pixel (y, x) reads x[y s - 1 + i + 2, x s - 1 + j - 3], zero outside
        om[:] = torch.tensor([2.0, -3.0], device=DEV).repeat(18)
        cols = ops.deform_cols(x, _padded_om(om), stride, 2, False)
        assert torch.equal(cols, _uniform_shift(x, stride, 2, -3)), (h, w, "uniform shift")


def _uniform_shift(x, stride, sy, sx):
    """(n*ho*wo, 9, c): the taps of a 3x3 / pad 1 window moved by (sy, sx) pixels, zero where a moved tap is outside the map."""
    n, h, w, c = x.shape
    ho, wo = out_hw(h, w, stride)
    want = torch.zeros((n, ho, wo, 9, c), dtype=x.dtype, device=x.device)
    for y in range(ho):
        for xx in range(wo):
            for k in range(9):
                yy, xw = y * stride - 1 + k // 3 + sy, xx * stride - 1 + k % 3 + sx
                if 0 <= yy < h and 0 <= xw < w:
                    want[:, y, xx, k] = x[:, yy, xw]
    return want.view(-1, 9, c)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("modulated", [False, True], ids=["dcn", "modulated"])
def test_fractional_offsets_against_float64(ops, modulated, dt):
    for stride in (1, 2):
        for h, w in MAPS:
            x = _x((2, h, w, 64), dt, 30 + h + stride)
            ho, wo = out_hw(h, w, stride)
            g = torch.Generator(device=DEV).manual_seed(31 + w + stride)
            om = torch.randn((2, ho, wo, offset_channels(2, modulated)), generator=g, device=DEV) * 1.5  # std 1.5 px (and mask logits)
            cols = ops.deform_cols(x, _padded_om(om), stride, 2, modulated)
            ref, S = ref_cols(x, om, stride, 2, modulated)
            _check(cols, ref, S, dt, f"{h}x{w} stride {stride}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F16, F32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("modulated", [False, True], ids=["dcn", "modulated"])
def test_borders_and_hostile_positions(ops, modulated, dt):
    """Every pair of the listed sample positions in h and w, on both maps: finite output equal to the reference, zero where the rule says
    zero. x is a view into the middle of an allocation whose surroundings are NaN (a stray read of a neighbouring image shows), and so
    is the padding of om's rows; only memory the process owns is read."""
    for h, w in MAPS:
        n, c, G = 2, 64, 2
        big = torch.full((n + 2, h, w, c), NAN, device=DEV, dtype=dt)
        big[1:n + 1] = _x((n, h, w, c), dt, 40 + h)
        x = big[1:n + 1]
        assert x.is_contiguous() and x.data_ptr() % 16 == 0
        pos_h = [-1.0, -1.0 + 2.0 ** -10, -0.5, h - 1.0, h - 0.5, float(h), 1e9, -1e9, INF, -INF, NAN, 1.25]
        pos_w = [-1.0, -1.0 + 2.0 ** -10, -0.5, w - 1.0, w - 0.5, float(w), 1e9, -1e9, INF, -INF, NAN, 2.75]
        pairs = torch.tensor([(a, b) for a in pos_h for b in pos_w], device=DEV)  # 144 (h, w) positions
        ho, wo = h, w  # stride 1
        slots = n * ho * wo * G * 9
        assert slots >= 2 * len(pairs)
        want = pairs[torch.arange(slots, device=DEV) % len(pairs)].view(n, ho, wo, G, 9, 2)
        k = torch.arange(9, device=DEV)
        base_y = (torch.arange(ho, device=DEV).view(1, ho, 1, 1, 1) - 1 + (k // 3).view(1, 1, 1, 1, 9)).float()
        base_x = (torch.arange(wo, device=DEV).view(1, 1, wo, 1, 1) - 1 + (k % 3).view(1, 1, 1, 1, 9)).float()
        off = torch.stack((want[..., 0] - base_y, want[..., 1] - base_x), -1).reshape(n, ho, wo, 18 * G)  # fp32: exact for the finite border values
        om = off
        if modulated:
            g = torch.Generator(device=DEV).manual_seed(41)
            om = torch.cat((off, torch.randn((n, ho, wo, 9 * G), generator=g, device=DEV)), -1)
        cols = ops.deform_cols(x, _padded_om(om), 1, G, modulated)
        ref, S = ref_cols(x, om, 1, G, modulated)
        assert 0.5 < float((ref == 0).double().mean()) < 0.99
        _check(cols, ref, S, dt, f"{h}x{w} borders")
        assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[n + 1]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("stride", [1, 2])
def test_layer_against_float64(ops, stride, dt):
    """ops.deform_conv2d, c = cout = 128 on a 6 x 9 map with ReLU (modulated, two groups): the gather against the definition, the
    contraction of the GPU's own cols against float64."""
    n, h, w, c, G = 2, 6, 9, 128, 2
    ho, wo = out_hw(h, w, stride)
    x = _x((n, h, w, c), dt, 50 + stride)
    g = torch.Generator(device=DEV).manual_seed(51 + stride)
    om = torch.randn((n, ho, wo, 27 * G), generator=g, device=DEV) * 1.5
    weight = (torch.randn((c, 3, 3, c), generator=g, device=DEV) * (2.0 / (9 * c)) ** 0.5).to(dt)
    bias = torch.randn((c,), generator=g, device=DEV) * 0.1
    omp = _padded_om(om)
    y = ops.deform_conv2d(x, omp, weight, bias, stride, G, True, relu=True)
    assert y.shape == (n, ho, wo, c) and y.dtype == dt
    cols = ops.deform_cols(x, omp, stride, G, True)
    cref, cS = ref_cols(x, om, stride, G, True)
    _check(cols, cref, cS, dt, f"gather, stride {stride}")
    a, wm = cols.double().view(-1, 9 * c), weight.double().view(c, 9 * c)
    pre = a @ wm.t() + bias.double()
    S = a.abs() @ wm.abs().t() + bias.double().abs()
    ref = pre.clamp(min=0)
    got = y.double().view(-1, c)
    assert bool(torch.isfinite(got).all())
    tol = (9 * c + 2) * U * S + _half_ulp(ref, dt)
    ratio = float(((got - ref).abs() / tol.clamp(min=1e-300)).max())
    print(f"[err] layer stride {stride}: max |err| / bound {ratio:.3e}")
    assert ratio <= 1.0
    assert 0.2 < float((got > 0).double().mean()) < 0.8  # the ReLU cuts about half


@pytest.mark.gpu
def test_unsupported_channel_counts_launch_nothing(ops):
    """c = 60 (not a multiple of 8) and G = 3 (64 % 3): OSR_ERR_UNSUPPORTED (-2) and an untouched output."""
    lib = ops._lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for c, groups in ((60, 1), (64, 3), (64, 16)):
        x = torch.ones((2, 5, 7, c), device=DEV, dtype=F16)
        om = torch.zeros((2, 5, 7, 64), device=DEV)
        cols = torch.full((70, 9, c), 7.0, device=DEV, dtype=F16)
        status = lib.osr_deform_cols(C.c_void_p(x.data_ptr()), C.c_void_p(om.data_ptr()), 2, 5, 7, c, 5, 7, 64, 1, groups, 0, C.c_void_p(cols.data_ptr()),
                                     ops._lib.OSR_F16, st)
        assert status == ops._lib.ERR_UNSUPPORTED == -2, (c, groups, status)
        torch.cuda.synchronize()
        assert bool((cols == 7.0).all())
        with pytest.raises(ops.OsrError, match="status -2"):
            ops.deform_cols(x, om, 1, groups, False)
    with pytest.raises(ops.OsrError, match="om"):  # too few offset channels for the groups: refused, not read past the row
        ops.deform_cols(torch.ones((2, 5, 7, 64), device=DEV, dtype=F16), torch.zeros((2, 5, 7, 24), device=DEV), 1, 2, False)


@pytest.mark.gpu
def test_second_loop_iteration_past_the_grid_cap(ops):
    """n, h, w, c = 2, 160, 140, 128 at stride 1 (fp16, modulated, two groups): 2 x 22400 x 9 x 16 = 6,451,200 work items against a grid
    capped at 8192 blocks x 256 lanes = 2,097,152 items per step, two steps per trip round the loop. Every lane makes a second trip;
    its second item there is live on the first 159,744 lanes only (3 steps + 159,744 = total) and dead on the rest. cols is this test's
    own NaN-filled buffer, handed to the C entry: a row no lane wrote fails _check's finiteness. Same bound as above."""
    n, h, w, c, G, dt = 2, 160, 140, 128, 2, F16
    total = n * h * w * 9 * (c // 8)
    assert total == 6451200 and total > 3 * 8192 * 256, "the shape must need a second trip, with a live and a dead second item"
    x = _x((n, h, w, c), dt, 60)
    g = torch.Generator(device=DEV).manual_seed(61)
    om = torch.randn((n, h, w, offset_channels(G, True)), generator=g, device=DEV) * 1.5
    omp = _padded_om(om)
    cols = torch.full((n * h * w, 9, c), NAN, device=DEV, dtype=dt)
    status = ops._lib.load().osr_deform_cols(C.c_void_p(x.data_ptr()), C.c_void_p(omp.data_ptr()), n, h, w, c, h, w, int(omp.shape[3]), 1, G, 1,
                                             C.c_void_p(cols.data_ptr()), ops._lib.OSR_F16, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    ref, S = ref_cols(x, om, 1, G, True)
    _check(cols, ref, S, dt, "160x140 past the grid cap")
