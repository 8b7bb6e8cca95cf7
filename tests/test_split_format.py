"""The operand format of the split-precision box head, pinned without a GPU: weights.split_fp32_rows (an fp32 matrix as two bf16
planes), the float64 emulation of the three products the kernel sums (x0 w0 + x1 w0 + x0 w1) against the float64 layer, and the
engine's argument checking for box_head.

Errors are e(y) = max|y - y64| / max|y64| with y64 the layer in float64 from the identical fp32 inputs. Condition A: e <= 1e-4
(the bar of the parity mode's dense stages). Condition B: e <= max(32 e(f32), 1e-5), e(f32) the error of an fp32 matmul on the
same inputs: two bf16 terms and three products sit 8-17 x over fp32's own error, two products or
16-bit-rounded inputs 300-800 x."""
import pytest
import torch

A_BOUND = 1e-4


def b_bound(e_f32):
    return max(32.0 * e_f32, 1e-5)


def err(y, y64):
    return float((y.double() - y64).abs().max() / y64.abs().max())


def _cases():
    g = torch.Generator().manual_seed(3)
    fc1 = torch.randn(64, 12544, generator=g) * (2.0 / 12544) ** 0.5
    special = torch.randn(6, 12544, generator=g)
    special[0] = 0.0
    special[1] *= 1e-30 / special[1].abs().max()
    special[2] *= 1e30 / special[2].abs().max()
    special[3] *= 1e-3
    special[4, ::2] *= 1e-6  # mixed magnitudes inside one row
    return torch.cat((fc1, special))


def test_split_terms_reproduce_the_rows(osr):
    from openset_rcnn_amd.host.weights import split_fp32_rows
    w = _cases()
    hi, lo, exp = split_fp32_rows(w)
    assert exp is None  # bf16 terms: no row exponents, hence no clamp range
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16 and hi.shape == w.shape and lo.shape == w.shape
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all())
    back = hi.double() + lo.double()
    row_max = w.double().abs().amax(dim=1, keepdim=True)
    resid = (back - w.double()).abs()
    assert bool((resid <= 2.0 ** -15 * row_max).all())
    # element-wise the split is tighter than the row bound: two round-to-nearest 8-bit terms leave <= 2^-17 (subnormal terms aside)
    big = w.abs() > 1e-25
    assert bool((resid[big] <= 2.0 ** -17 * w.double().abs()[big]).all())
    assert bool((back[64] == 0).all())  # the row of zeros (first of the special rows) stays zeros
    # the first term is the bf16 rounding of the value, the second the bf16 rounding of what is left
    assert torch.equal(hi, w.to(torch.bfloat16)) and torch.equal(lo, (w - hi.float()).to(torch.bfloat16))


@pytest.mark.parametrize("m,k,n,relu_rows", [(192, 12544, 1024, False), (192, 1024, 1024, True), (1, 12544, 1024, False), (63, 1024, 1024, True)])
def test_three_product_emulation_meets_a_and_b(osr, m, k, n, relu_rows):
    """What the kernel computes, with float64 accumulation: the format, not the MFMA's summation, is what is pinned here."""
    from openset_rcnn_amd.host.weights import split_fp32_rows
    g = torch.Generator().manual_seed(100 + m + k)
    x = torch.randn(m, k, generator=g)
    x *= torch.tensor([0.05, 1.0, 20.0])[torch.arange(m) % 3].view(m, 1)  # mixed-magnitude rows
    if relu_rows:
        x = x.clamp(min=0)
    w = torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5
    b = torch.randn(n, generator=g) * 0.02
    y64 = x.double() @ w.double().t() + b.double()
    x0, x1, _ = split_fp32_rows(x)
    w0, w1, _ = split_fp32_rows(w)
    y = x0.double() @ w0.double().t() + x1.double() @ w0.double().t() + x0.double() @ w1.double().t() + b.double()
    e_split, e_f32 = err(y, y64), err(x @ w.t() + b, y64)
    print(f"\n[split format, m {m} k {k} n {n}] e(split) {e_split:.3e}  e(f32) {e_f32:.3e}  ratio {e_split / e_f32:.1f}")
    assert e_split <= A_BOUND
    assert e_split <= b_bound(e_f32)
    # and the bound does its work: two products instead of three miss both conditions
    y2 = x0.double() @ w0.double().t() + x1.double() @ w0.double().t() + b.double()
    assert err(y2, y64) > b_bound(e_f32)


def test_engine_box_head_argument_checking_needs_no_device(osr):
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    for kw in (dict(dtype=torch.float32, box_head="split"), dict(dtype=torch.float16, box_head="split", fp32_points=("pooled",)),
               dict(dtype=torch.float16, box_head="split", fp32_points=("h1",)), dict(dtype=torch.float16, box_head="fp64")):
        with pytest.raises(ValueError):
            OpensetRCNNEngine({}, device="cuda:0", **kw)  # raised before a parameter is packed or a tensor moved
    assert OpensetRCNNEngine.BOX_HEADS == ("storage", "split")


def test_linear_split_refuses_cpu_tensors(osr):
    from openset_rcnn_amd.host.weights import split_fp32_rows
    with pytest.raises(osr.OsrError):
        osr.ops.linear_split(torch.zeros(4, 64), split_fp32_rows(torch.zeros(64, 64)), torch.zeros(64))
