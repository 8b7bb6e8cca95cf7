"""The backward of the split-precision fully connected layer on the GPU: ops.linear_split_wgrad (osr_linear_split_wgrad,
csrc/osr_linear_split_bwd.hip), ops.linear_split_dgrad (osr_linear_split_dgrad) and ops.split_rows_bf16_t (osr_split_rows_bf16_t).

Errors are e(y) = max|y - y64| / max|y64|, y64 = the same contraction by torch on the CPU in float64 from the identical fp32 inputs.
  A:   e(split) <= 1e-4                     the parity mode's bar (tests/test_split_format_bwd.py: the float64 value of the three
                                            products is 12 x inside it)
  Acc: max|y - y3| / max|y64| <= 4 e(f32)   y3 = the float64 value of the SAME three products from the bf16 terms (torch.float64
                                            matmuls on the GPU): what the kernel's fp32 accumulation adds to the format's error.
                                            e(f32) = the error of the exact-f32 kernel on the same inputs in the same test
                                            (ops.gemm_f32_tn for the weight gradient, ops.linear on fp32 tensors for the data gradient).
                                            4: three products per term into one fp32 accumulator, plus the fixed-order partial sums.
Every test also checks through the launch counters that the split kernels ran."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A_BOUND = 1e-4
ACC_FACTOR = 4.0
SHAPES = [(8192, 12544, 1024), (8192, 1024, 1024), (1, 12544, 1024), (1, 1024, 1024), (63, 12544, 1024), (63, 1024, 1024), (257, 12544, 1024),
          (257, 1024, 1024)]
IDS = ["fc1", "fc2", "fc1_m1", "fc2_m1", "fc1_m63", "fc2_m63", "fc1_m257", "fc2_m257"]


def err(y, y64):
    return float((y.detach().cpu().double() - y64).abs().max() / y64.abs().max())


@pytest.fixture()
def counted(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    osr.ops.LINEAR_SPLIT_WGRAD_COUNT = {"launches": 0, "flops": 0.0}
    osr.ops.LINEAR_SPLIT_DGRAD_COUNT = {"launches": 0, "flops": 0.0}
    osr.ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    yield dict(wgrad=osr.ops.LINEAR_SPLIT_WGRAD_COUNT, dgrad=osr.ops.LINEAR_SPLIT_DGRAD_COUNT, fwd=osr.ops.LINEAR_SPLIT_COUNT)
    osr.ops.LINEAR_SPLIT_WGRAD_COUNT = osr.ops.LINEAR_SPLIT_DGRAD_COUNT = osr.ops.LINEAR_SPLIT_COUNT = None


@functools.lru_cache(maxsize=None)  # (computed once per shape, shared by the tests, never written to)
def _layer(m, k, n, seed):
    """x, w as _layer of tests/test_linear_split.py (He-initialised weights; rows of mixed magnitude, per-row scale spread over two
    decades; post-ReLU rows for the FC2 shape); dy: mixed row magnitudes behind a ReLU mask; h: a forward output of width k (the
    data gradient's mask)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g) * 1.2)
    if k == 1024:
        x = x.clamp(min=0)
    w = torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5
    dy = torch.randn(m, n, generator=g) * torch.exp(torch.randn(m, 1, generator=g) * 1.2)
    dy = dy * (torch.rand(m, n, generator=g) < 0.5)
    h = torch.randn(m, k, generator=g).clamp(min=0) if k == 1024 else None
    return x, w, dy, h


def _terms64(v):
    """The two bf16 terms of the split, as float64 on the GPU."""
    from openset_rcnn_amd.host.weights import split_fp32_rows
    hi, lo, _ = split_fp32_rows(v)
    return hi.to(DEV).double(), lo.to(DEV).double()


def _wgrad3(dy, x):
    d0, d1 = _terms64(dy)
    x0, x1 = _terms64(x)
    return ((d0 + d1).t() @ x0 + d0.t() @ x1).cpu()  # dy0 x0 + dy1 x0 + dy0 x1 (d0 + d1 is exact in float64)


def _dgrad3(dy, w):
    d0, d1 = _terms64(dy)
    w0, w1 = _terms64(w)
    return ((d0 + d1) @ w0 + d0 @ w1).cpu()


def _check(tag, y, yf, y3, y64):
    """A and Acc, figures printed first."""
    e_s, e_f = err(y, y64), err(yf, y64)
    fmt = float((y3 - y64).abs().max() / y64.abs().max())
    acc = float((y.detach().cpu().double() - y3).abs().max() / y64.abs().max())
    print(f"\n[{tag}] e(split) {e_s:.3e}  e(f32) {e_f:.3e}  format (three products in float64) {fmt:.3e}  "
          f"Acc {acc:.3e} = {acc / max(e_f, 1e-30):.2f} x e(f32)")
    assert e_s <= A_BOUND, (tag, e_s)
    assert acc <= ACC_FACTOR * e_f, (tag, acc, e_f)
    return e_s, e_f, acc


@pytest.mark.parametrize("m,k,n", SHAPES, ids=IDS)
def test_wgrad_meets_a_and_acc(osr, counted, m, k, n):
    ops = osr.ops
    x, w, dy, _ = _layer(m, k, n, 7 + m + k)
    xd, dyd = x.to(DEV), dy.to(DEV)
    dw = ops.linear_split_wgrad(xd, dyd)
    dw2 = ops.linear_split_wgrad(xd, dyd, dw=torch.full((n, k), float("nan"), device=DEV))
    dwf = ops.gemm_f32_tn(dyd, xd)
    torch.cuda.synchronize()
    assert counted["wgrad"]["launches"] == 2 and counted["wgrad"]["flops"] == 2 * 2.0 * m * k * n
    assert counted["dgrad"]["launches"] == 0 and counted["fwd"]["launches"] == 0
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (n, k)
    assert torch.equal(dw, dw2)  # bit-identical on a second launch
    y64 = dy.double().t() @ x.double()
    _check(f"linear_split_wgrad m {m} k {k} n {n}", dw, dwf, _wgrad3(dy, x), y64)


@pytest.mark.parametrize("m,k,n", SHAPES, ids=IDS)
def test_dgrad_meets_a_and_acc(osr, counted, m, k, n):
    from openset_rcnn_amd.host.weights import split_fp32_rows_t
    ops = osr.ops
    x, w, dy, h = _layer(m, k, n, 7 + m + k)
    mask = h if k == 1024 else None  # FC2's data gradient carries the ReLU mask of h1; FC1's has none
    dyd = dy.to(DEV)
    wt = tuple(t.to(DEV) for t in split_fp32_rows_t(w)[:2])
    md = None if mask is None else mask.to(DEV)
    dx = ops.linear_split_dgrad(dyd, wt, mask=md)
    dx2 = ops.linear_split_dgrad(dyd, wt, mask=md, out=torch.full((m, k), float("nan"), device=DEV))
    dxf = ops.linear(dyd, w.t().contiguous().to(DEV), torch.zeros(k, device=DEV), out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert counted["dgrad"]["launches"] == 2 and counted["dgrad"]["flops"] == 2 * 2.0 * m * k * n
    assert counted["wgrad"]["launches"] == 0 and counted["fwd"]["launches"] == 0
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (m, k)
    assert torch.equal(dx, dx2)
    y64 = dy.double() @ w.double()
    y3 = _dgrad3(dy, w)
    dxf = dxf.cpu()
    if mask is not None:
        keep = mask > 0
        assert bool((dx.cpu()[~keep] == 0).all())  # exactly 0 behind the ReLU
        assert int((~keep).sum()) > 0 and int(keep.sum()) > 0
        y64, y3, dxf = y64 * keep, y3 * keep, dxf * keep
    _check(f"linear_split_dgrad m {m} k {k} n {n}", dx, dxf, y3, y64)


def test_dy_scale_range(osr, counted):
    """dy multiplied by 2^j, j in [-24, 24] (a loss scale and its range): blocks of 16 columns of dy that share j scale 16 rows of dW,
    blocks of 8 rows of dy scale 8 rows of dx; every block meets A against its own y64 maximum (the bf16 terms carry fp32's exponent:
    the split is scale-free)."""
    from openset_rcnn_amd.host.weights import split_fp32_rows_t
    ops = osr.ops
    m, k, n = 49 * 8, 1024, 1024
    x, w, dy, _ = _layer(m, k, n, 99)
    j = torch.randperm(49, generator=torch.Generator().manual_seed(1)) - 24  # every j of [-24, 24] once, shuffled
    two = torch.tensor(2.0)
    dyc = dy.clone()
    dyc[:, :49 * 16] *= torch.pow(two, j.repeat_interleave(16).float()).view(1, -1)
    dw = ops.linear_split_wgrad(x.to(DEV), dyc.to(DEV))
    dyr = dy * torch.pow(two, j.repeat_interleave(8).float()).view(m, 1)
    dx = ops.linear_split_dgrad(dyr.to(DEV), tuple(t.to(DEV) for t in split_fp32_rows_t(w)[:2]))
    torch.cuda.synchronize()
    assert counted["wgrad"]["launches"] == 1 and counted["dgrad"]["launches"] == 1
    w64, x64 = dyc.double().t() @ x.double(), dyr.double() @ w.double()
    worst_w = max((err(dw[b * 16:b * 16 + 16], w64[b * 16:b * 16 + 16]), int(j[b])) for b in range(49))
    worst_x = max((err(dx[b * 8:b * 8 + 8], x64[b * 8:b * 8 + 8]), int(j[b])) for b in range(49))
    print(f"\n[dy scales 2^-24..2^24] worst block: wgrad {worst_w[0]:.3e} at 2^{worst_w[1]}, dgrad {worst_x[0]:.3e} at 2^{worst_x[1]}")
    assert worst_w[0] <= A_BOUND and worst_x[0] <= A_BOUND


@pytest.mark.parametrize("k", [12544, 1024], ids=["fc1", "fc2"])
def test_wgrad_row_lists_keep_nan_padding_rows_out(osr, counted, k):
    """Per-image row lists [cap, 0, 1, cap - 1] (as the forward's test): the padding rows of x hold NaN, those of dy anything; dW is
    finite and is the weight gradient of the real rows alone."""
    ops = osr.ops
    cap, n = 300, 1024
    counts = [cap, 0, 1, cap - 1]
    m = cap * len(counts)
    x, w, dy, _ = _layer(m, k, n, 21 + k)
    real = torch.zeros(m, dtype=torch.bool)
    for s, c in enumerate(counts):
        real[s * cap:s * cap + c] = True
    xn = x.clone()
    xn[~real] = float("nan")  # what uninitialised padding rows may hold
    seg = (torch.tensor(counts, dtype=torch.int32, device=DEV), cap)
    dw = ops.linear_split_wgrad(xn.to(DEV), dy.to(DEV), row_seg=seg)
    dw2 = ops.linear_split_wgrad(xn.to(DEV), dy.to(DEV), row_seg=seg)
    xr, dyr = x[real].contiguous(), dy[real].contiguous()
    dwf = ops.gemm_f32_tn(dyr.to(DEV), xr.to(DEV))
    torch.cuda.synchronize()
    assert counted["wgrad"]["launches"] == 2
    assert bool(torch.isfinite(dw).all()) and torch.equal(dw, dw2)
    _check(f"wgrad row_seg k {k}, {int(real.sum())} real rows of {m}", dw, dwf, _wgrad3(dyr, xr), dyr.double().t() @ xr.double())


def test_dgrad_row_lists_skip_padding_tiles(osr, counted):
    from openset_rcnn_amd.host.weights import split_fp32_rows_t
    ops = osr.ops
    cap, n, k = 300, 1024, 1024
    counts = [cap, 0, 1, cap - 1]
    m = cap * len(counts)
    x, w, dy, h = _layer(m, k, n, 33)
    real = torch.zeros(m, dtype=torch.bool)
    for s, c in enumerate(counts):
        real[s * cap:s * cap + c] = True
    dyn = dy.clone()
    dyn[~real] = float("nan")
    SENT = -777.0
    out = torch.full((m, k), SENT, dtype=torch.float32, device=DEV)
    wt = tuple(t.to(DEV) for t in split_fp32_rows_t(w)[:2])
    dx = ops.linear_split_dgrad(dyn.to(DEV), wt, mask=h.to(DEV), row_seg=(torch.tensor(counts, dtype=torch.int32, device=DEV), cap), out=out).cpu()
    plain = ops.linear_split_dgrad(dy.to(DEV), wt, mask=h.to(DEV)).cpu()
    torch.cuda.synchronize()
    assert counted["dgrad"]["launches"] == 2
    assert torch.equal(dx[real], plain[real])  # rows are independent: a NaN padding row stays in its own row
    skipped = 0
    for t0 in range(0, m, 128):
        if not bool(real[t0:t0 + 128].any()):
            skipped += 1
            assert bool((dx[t0:t0 + 128] == SENT).all()), t0
    assert skipped >= 3


@pytest.mark.parametrize("rows,cols", [(96, 1024), (70, 45), (1, 33), (1024, 12544)], ids=["96x1024", "70x45", "1x33", "fc1"])
def test_transposed_split_kernel_matches_the_host_format(osr, rows, cols):
    from openset_rcnn_amd.host.weights import split_fp32_rows_t
    g = torch.Generator().manual_seed(5)
    w = torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 8)
    w[rows // 2] = 0
    hi, lo, _ = split_fp32_rows_t(w)
    dhi, dlo = osr.ops.split_rows_bf16_t(w.to(DEV))
    assert tuple(dhi.shape) == (cols, rows)
    assert torch.equal(dhi.cpu(), hi) and torch.equal(dlo.cpu(), lo)
    again = osr.ops.split_rows_bf16_t(w.to(DEV), out=(torch.zeros_like(dhi), torch.zeros_like(dlo)))
    assert torch.equal(again[0], dhi) and torch.equal(again[1], dlo)


def test_unsupported_shapes_are_refused_before_launching(osr, counted):
    ops = osr.ops
    bf = dict(dtype=torch.bfloat16, device=DEV)
    for m, k, n in ((8, 100, 64), (8, 64, 100), (8, 96, 64)):
        with pytest.raises(osr.OsrError, match="multiple of 64"):
            ops.linear_split_wgrad(torch.zeros(m, k, device=DEV), torch.zeros(m, n, device=DEV))
        with pytest.raises(osr.OsrError, match="multiple of 64"):
            ops.linear_split_dgrad(torch.zeros(m, n, device=DEV), (torch.zeros(k, n, **bf), torch.zeros(k, n, **bf)))
    assert counted["wgrad"]["launches"] == 0 and counted["dgrad"]["launches"] == 0
    lib, L = osr._lib.load(), osr._lib
    one = ctypes.c_void_p(16)
    assert lib.osr_linear_split_wgrad(one, 64, one, 100, one, 100, 8, 64, 100, None, 0, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.osr_linear_split_wgrad(one, 100, one, 64, one, 64, 8, 100, 64, None, 0, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.osr_linear_split_dgrad(one, 64, one, one, None, 0, one, 100, 8, 64, 100, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.osr_linear_split_dgrad(one, 100, one, one, None, 0, one, 64, 8, 100, 64, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.osr_linear_split_wgrad_workspace_bytes(8192, 1024, 1024) > 0  # FC2: the row axis is cut over workgroups
