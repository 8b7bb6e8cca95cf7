"""The operand format of the split-precision convolutions, pinned without a GPU: weights.split_conv_weight / split_stem_weight (the
packed fp32 weight as two bf16 planes), the emulation of the three products the kernel sums (x1 w0 + x0 w1 + x0 w0) carried through
the ~50 stacked layers of the oracle's ResNet-50 + FPN, and the engine's argument checking for conv=.

Errors are e(y) = max|y - y64| / max|y64| with y64 computed in float64 from the identical fp32 inputs. Condition A: e <= 1e-4 (the
bar of the parity mode's dense stages). Condition B: e <= max(32 e(f32), 1e-5), e(f32) the error of the fp32 path on the same inputs
(tests/test_split_format.py states where the two bounds come from)."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

A_BOUND = 1e-4


def b_bound(e_f32):
    return max(32.0 * e_f32, 1e-5)


def err(y, y64):
    return float((y.double() - y64).abs().max() / y64.abs().max())


def split(t):
    t0 = t.to(torch.bfloat16).float()
    return t0, (t - t0).to(torch.bfloat16).float()


def conv_split(x, w, b=None, products=3, **kw):
    """The kernel's arithmetic on the CPU: bf16 terms, fp32 sums, the small products first."""
    x0, x1 = split(x)
    w0, w1 = split(w)
    y = F.conv2d(x1, w0, None, **kw)
    if products == 3:
        y = y + F.conv2d(x0, w1, None, **kw)
    y = y + F.conv2d(x0, w0, None, **kw)
    return y if b is None else y + b.view(1, -1, 1, 1)


def test_split_conv_weight_is_the_packed_weight_in_two_bf16_planes(osr):
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_stem_weight, split_conv_weight, split_stem_weight
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 32, 3, 3, generator=g) * 0.1
    w[0, 0] = 0.0
    w[1] *= 1e-20
    w[2] *= 1e20
    stem = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    for planes, packed in ((split_conv_weight(w), pack_conv_weight(w, torch.float32)), (split_stem_weight(stem), pack_stem_weight(stem, torch.float32))):
        hi, lo = planes
        assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16
        assert hi.shape == packed.shape and lo.shape == packed.shape and hi.is_contiguous() and lo.is_contiguous()
        assert torch.equal(hi, packed.to(torch.bfloat16)) and torch.equal(lo, (packed - hi.float()).to(torch.bfloat16))
        back, p64 = hi.double() + lo.double(), packed.double()
        big = packed.abs() > 1e-25
        assert bool(((back - p64).abs()[big] <= 2.0 ** -17 * p64.abs()[big]).all())
        assert bool((back[packed == 0] == 0).all())
    hi, lo = split_stem_weight(stem)
    assert tuple(hi.shape) == (64, 8, 1, 32)
    assert bool((hi[:, 7] == 0).all()) and bool((lo[:, 7] == 0).all())  # the zero-weight eighth tap row stays zero
    v = hi.view(64, 8, 8, 4)
    assert bool((v[:, :, 7] == 0).all()) and bool((v[:, :, :, 3] == 0).all())  # and so do the eighth tap and the fourth channel


@pytest.fixture(scope="module")
def trunk(osr):
    """Seed-0 oracle weights, 2 seeded 256 x 384 images: the float64 pyramid and the fp32 one, computed once."""
    from openset_rcnn_amd.host.weights import random_params
    p = {k: v for k, v in random_params(0).items() if k.startswith("backbone.")}
    g = torch.Generator().manual_seed(11)
    images = torch.randint(0, 256, (2, 3, 256, 384), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        batch, _ = O.preprocess_images([im for im in images])
        y64 = O.resnet_fpn_forward(batch.double(), {k: v.double() for k, v in p.items()})
        y32 = O.resnet_fpn_forward(batch, p)
    return dict(p=p, batch=batch, y64=y64, e32={k: err(y32[k], y64[k]) for k in y64})


def _pyramid_with(monkeypatch, trunk, products):
    shim = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
    shim.conv2d = lambda t, w, b=None, stride=1, padding=0: conv_split(t, w, b, products, stride=stride, padding=padding)
    monkeypatch.setattr(O, "F", shim)  # (the oracle file stays as it is: its F is swapped for the length of this test)
    with torch.no_grad():
        return O.resnet_fpn_forward(trunk["batch"], trunk["p"])


def test_three_products_survive_fifty_stacked_layers(osr, trunk, monkeypatch):
    y = _pyramid_with(monkeypatch, trunk, 3)
    e3 = {k: err(y[k], trunk["y64"][k]) for k in ("p2", "p3", "p4", "p5", "p6")}
    y2 = _pyramid_with(monkeypatch, trunk, 2)
    e2 = {k: err(y2[k], trunk["y64"][k]) for k in e3}
    for k in e3:
        print(f"\n[conv split format, {k}] e(three products) {e3[k]:.3e}  e(x0 w1 dropped) {e2[k]:.3e}  e(f32) {trunk['e32'][k]:.3e}")
    for k in e3:
        assert e3[k] <= A_BOUND, (k, e3[k])
    # and the bound does its work: without the x0 w1 product a level misses A or sits 32 x over the three-product error
    assert any(e2[k] > A_BOUND or e2[k] > 32.0 * e3[k] for k in e3), (e2, e3)


def test_one_3x3_layer_meets_a_and_b(osr):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 256, 16, 16, generator=g).clamp(min=0)
    w = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / 2304) ** 0.5
    b = torch.randn(256, generator=g) * 0.02
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    e_split, e_f32 = err(conv_split(x, w, b, padding=1), y64), err(F.conv2d(x, w, b, padding=1), y64)
    print(f"\n[conv split format, 3x3 256 -> 256] e(split) {e_split:.3e}  e(f32) {e_f32:.3e}")
    assert e_split <= A_BOUND
    assert e_split <= b_bound(e_f32)


def test_engine_conv_argument_checking_needs_no_device(osr):
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    assert OpensetRCNNEngine.CONVS == ("storage", "split")
    for kw in (dict(dtype=torch.float16, conv="split"), dict(dtype=torch.bfloat16, conv="split"), dict(conv="split"),
               dict(dtype=torch.float32, conv="fp64"), dict(dtype=torch.float32, conv="split", box_head="split")):
        with pytest.raises(ValueError):
            OpensetRCNNEngine({}, device="cuda:0", **kw)  # raised before a parameter is packed or a tensor moved
    with pytest.raises(ValueError):
        StandardRCNNEngine({}, dtype=torch.float32, device="cuda:0", conv="split")
    with pytest.raises(ValueError):
        OpensetRCNNTrainer({}, dtype=torch.float32, device="cuda:0", conv="split")


def test_conv2d_split_refuses_cpu_tensors(osr):
    from openset_rcnn_amd.host.weights import split_conv_weight
    with pytest.raises(osr.OsrError):
        osr.ops.conv2d_split(torch.zeros(1, 4, 4, 64), split_conv_weight(torch.zeros(64, 64, 1, 1)), torch.zeros(64))
