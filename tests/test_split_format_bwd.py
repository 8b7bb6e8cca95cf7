"""The operand format of the split-precision box head's backward, on the CPU (no kernel runs here):
  - weights.split_fp32_rows_t, the host twin of osr_split_rows_bf16_t, is split_fp32_rows of the transposed matrix bit for bit;
  - the weight gradient dW = dy^T x over m = 8192 rows, evaluated in float64 from the bf16 terms: the three products the kernel sums
    (dy0 x0 + dy1 x0 + dy0 x1) stay inside 1e-4 of the largest element (the parity mode's bar A), two products do not.
Errors are e(y) = max|y - y64| / max|y64| with y64 from the fp32 inputs in float64."""
import pytest
import torch

A_BOUND = 1e-4


def _terms(v):
    from openset_rcnn_amd.host.weights import split_fp32_rows
    hi, lo, _ = split_fp32_rows(v)
    return hi.double(), lo.double()


def _wgrad_inputs(m=8192, n=64, k=512, seed=11):
    """x: pooled-like rows (log-normal row scales); dy: the gradient behind a ReLU, half of the rows nearly empty."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g) * 1.2)
    dy = torch.randn(m, n, generator=g) * torch.exp(torch.randn(m, 1, generator=g) * 1.2)
    dy = dy * (torch.rand(m, n, generator=g) < 0.5)
    dy[torch.rand(m, generator=g) < 0.5] *= 1e-3
    return x, dy


def _err(y, y64):
    return float((y - y64).abs().max() / y64.abs().max())


def test_transposed_split_is_the_split_of_the_transpose(osr):
    from openset_rcnn_amd.host.weights import split_fp32_rows, split_fp32_rows_t
    g = torch.Generator().manual_seed(5)
    w = torch.randn(96, 200, generator=g) * torch.exp(torch.randn(96, 1, generator=g) * 8)
    w[3] = 0
    hi, lo, ex = split_fp32_rows_t(w)
    rhi, rlo, _ = split_fp32_rows(w.t().contiguous())
    assert ex is None and tuple(hi.shape) == (200, 96) and hi.dtype == torch.bfloat16 and hi.is_contiguous() and lo.is_contiguous()
    assert torch.equal(hi, rhi) and torch.equal(lo, rlo)
    # the format: hi = bf16(w), lo = bf16(w - hi), round to nearest even
    wt = w.t().contiguous()
    assert torch.equal(hi, wt.to(torch.bfloat16)) and torch.equal(lo, (wt - wt.to(torch.bfloat16).float()).to(torch.bfloat16))


@pytest.mark.parametrize("scale", [1.0, 1024.0, 2.0 ** -20], ids=["1", "2^10", "2^-20"])
def test_three_products_of_a_weight_gradient_meet_a_two_do_not(osr, scale):
    x, dy = _wgrad_inputs()
    dy = dy * scale  # (a loss scale is a power of two: the split is scale-free)
    y64 = dy.double().t() @ x.double()
    d0, d1 = _terms(dy)
    x0, x1 = _terms(x)
    three = d0.t() @ x0 + d1.t() @ x0 + d0.t() @ x1
    two_a = d0.t() @ x0 + d1.t() @ x0
    two_b = d0.t() @ x0 + d0.t() @ x1
    e3, e2a, e2b = _err(three, y64), _err(two_a, y64), _err(two_b, y64)
    ef = _err((dy.t() @ x).double(), y64)
    print(f"\n[wgrad m 8192 n 64 k 512, dy x {scale:g}] three products {e3:.3e}  two products {e2a:.3e} / {e2b:.3e}  fp32 matmul {ef:.3e}")
    assert e3 <= A_BOUND
    assert e2a > A_BOUND and e2b > A_BOUND
