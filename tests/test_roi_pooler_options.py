"""MODEL.ROI_BOX_HEAD.POOLER_TYPE "ROIAlign" (aligned=False) and POOLER_SAMPLING_RATIO > 0 through the RoIAlign kernels:
the yaml mapping (CPU), the forward against the C oracle, the two backward kernels against autograd through a float64 torch
restatement of the forward that this file pins against the oracle's roi_align_ref."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import c_binding as CO
from oracle import osr_oracle as O

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.25, 0.125, 0.0625, 0.03125)
NEW_PAIRS = [(True, 2), (False, 0), (False, 2)]            # (aligned, sampling_ratio) beside the default (True, 0)
FWD_PAIRS = NEW_PAIRS + [(True, 1), (True, 3), (True, 5)]


def _id(p):
    return f"{'V2' if p[0] else 'ROIAlign'}-S{p[1]}"


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(x):  # (N,C,H,W) -> contiguous NHWC
    return x.permute(0, 2, 3, 1).contiguous()


def assert_close(a, b, rtol=1e-4, atol=None, name=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    if atol is None:
        atol = rtol * max(float(b.abs().max()), 1e-6)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    print(f"{name}: max abs err {float(err.max()):.3e} (max |ref| {float(b.abs().max()):.3e})")
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err {float(err.max()):.3e}"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


# ------------------------------------------------------------------------------------------------------
# a differentiable restatement of roi_align_ref with both options
# ------------------------------------------------------------------------------------------------------
def _axis_matrix(start, bs, grid, size, P):
    """(P, size) float64: entry (bin, pixel) sums the bilinear weights of the bin's `grid` samples on that pixel along one axis.
    Sample positions in fp32, operation by operation as oracle.osr_oracle.roi_align_ref computes them; a sample outside [-1, size]
    contributes nothing. The validity rule and the clamps are per axis, so the 2-d weights are the outer product of two of these."""
    f32 = np.float32
    M = np.zeros((P, size), dtype=np.float64)
    for p in range(P):
        for i in range(grid):
            v = f32(start + f32(p) * bs + f32(f32(i) + f32(0.5)) * bs / f32(grid))
            if v < -1.0 or v > size:
                continue
            v = max(v, f32(0.0))
            lo = int(v)
            if lo >= size - 1:
                hi = lo = size - 1
                v = f32(lo)
            else:
                hi = lo + 1
            frac = f32(v - f32(lo))
            M[p, lo] += float(f32(f32(1.0) - frac))
            M[p, hi] += float(frac)
    return M


def roi_align_t(feat, rois, scale, out_size=7, sampling_ratio=0, aligned=True):
    """torchvision roi_align in differentiable torch ops, float64: feat (N,C,H,W), rois (K,5) [batch,x1,y1,x2,y2] -> (K,C,P,P).
    Modelled on oracle.osr_oracle.roi_align_torch, which is fixed to (aligned, adaptive grid); only the weighted sums are traced."""
    f32 = np.float32
    _, _, height, width = feat.shape
    off = f32(0.5) if aligned else f32(0.0)
    outs = []
    for r in range(rois.shape[0]):
        b = int(rois[r, 0])
        sw_, sh_ = f32(rois[r, 1]) * f32(scale) - off, f32(rois[r, 2]) * f32(scale) - off
        ew_, eh_ = f32(rois[r, 3]) * f32(scale) - off, f32(rois[r, 4]) * f32(scale) - off
        rw, rh = f32(ew_ - sw_), f32(eh_ - sh_)
        if not aligned:
            rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
        bh, bw = f32(rh / f32(out_size)), f32(rw / f32(out_size))
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rh) / out_size))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rw) / out_size))
        wy = torch.from_numpy(_axis_matrix(sh_, bh, gh, height, out_size))
        wx = torch.from_numpy(_axis_matrix(sw_, bw, gw, width, out_size))
        outs.append(torch.einsum("ph,chw,qw->cpq", wy, feat[b].double(), wx) / float(max(gh * gw, 1)))
    return torch.stack(outs) if outs else feat.new_zeros((0, feat.shape[1], out_size, out_size), dtype=torch.float64)


def _autograd_levels(shapes, n, c, boxes, bidx, dout, pair):
    """d feature pyramid of roi_align_t for the list (boxes, bidx >= 0) with upstream gradient dout (m,P,P,c): [(n,c,h,w)] float64."""
    lv = O.assign_levels(boxes)
    grads = []
    for l, (h, w) in enumerate(shapes):
        feat = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
        ids = torch.nonzero((lv == l) & (bidx >= 0)).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
            roi_align_t(feat, rois, SCALES[l], 7, pair[1], pair[0]).backward(dout[ids].permute(0, 3, 1, 2).double())
            grads.append(feat.grad)
        else:
            grads.append(torch.zeros(n, c, h, w, dtype=torch.float64))
    return grads


# ------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------
def _build(osr, yaml, opts):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return M.build_model(cfg)


@pytest.mark.parametrize("yaml", ["voc_coco.yaml", "base_rcnn_fpn.yaml"])
def test_model_from_yaml_resolves_the_pooler_options(osr, yaml):
    model = _build(osr, yaml, ["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlign", "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2])
    for ec in (model.roi_heads._eng_cfg, model._eng_cfg):  # the heads' engine and the whole model's (the trainer's)
        assert ec["pooler_aligned"] is False and ec["pooler_sampling_ratio"] == 2
    model = _build(osr, yaml, [])
    for ec in (model.roi_heads._eng_cfg, model._eng_cfg):
        assert ec["pooler_aligned"] is True and ec["pooler_sampling_ratio"] == 0
    with pytest.raises(ValueError, match="ROIAlignV2.*ROIAlign"):
        _build(osr, yaml, ["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIPool"])
    with pytest.raises(ValueError, match="ROIAlignV2.*ROIAlign"):
        _build(osr, yaml, ["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlignRotated"])
    for ratio in (-1, 65):
        with pytest.raises(ValueError, match="POOLER_SAMPLING_RATIO"):
            _build(osr, yaml, ["MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", ratio])


def test_engine_refuses_bad_pooler_options_before_it_touches_a_device(osr):
    from openset_rcnn_amd.host import engine, engine_std
    assert engine.DEFAULT_CFG["pooler_aligned"] is True and engine.DEFAULT_CFG["pooler_sampling_ratio"] == 0
    for cls in (engine.OpensetRCNNEngine, engine_std.StandardRCNNEngine):
        for bad in ({"pooler_sampling_ratio": -1}, {"pooler_sampling_ratio": 1.5}, {"pooler_aligned": 2}, {"pooler_aligned": "ROIAlign"}):
            with pytest.raises(ValueError, match="RoIAlign"):
                cls({}, device="cuda:0", cfg=bad)


def _pin_case():
    gg = g(5)
    feat = torch.randn(2, 6, 20, 28, generator=gg)
    ctr = torch.rand(12, 2, generator=gg) * torch.tensor([28.0 * 4, 20.0 * 4])
    size = torch.exp(torch.rand(12, 2, generator=gg) * 4.0 + 0.5)
    boxes = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
    boxes[0] = torch.tensor([40.0, 30.0, 40.0, 30.0])      # zero area
    boxes[1] = torch.tensor([-30.0, -20.0, 25.0, 18.0])    # crosses the top-left border
    boxes[2] = torch.tensor([50.3, 40.2, 51.1, 41.0])      # a fifth of a level pixel
    boxes[3] = torch.tensor([90.0, 60.0, 140.0, 110.0])    # crosses the bottom-right border
    bidx = torch.randint(0, 2, (12,), generator=gg)
    return feat, torch.cat((bidx.float().unsqueeze(1), boxes), dim=1)


@pytest.mark.parametrize("pair", [(True, 0)] + NEW_PAIRS, ids=_id)
def test_backward_reference_is_pinned_to_the_oracle_forward(pair):
    """roi_align_t (the autograd reference of the backward tests) against roi_align_ref. The reference sums at most 4 x 4 samples of
    4 taps in fp32 per bin here (64 products of 2^-24 relative error each): 1e-5 of the largest output bounds it."""
    feat, rois = _pin_case()
    ref = torch.from_numpy(O.roi_align_ref(feat.numpy(), rois.numpy(), 0.25, 7, pair[1], pair[0]))
    got = roi_align_t(feat, rois, 0.25, 7, pair[1], pair[0])
    assert float((got - ref.double()).abs().max()) <= 1e-5 * float(ref.abs().max())
    zero_area = float(ref[0].abs().max())
    assert (zero_area == 0.0) == (pair == (True, 0)), "a zero-area box pools to zeros under the default options only"
    # the C restatement the GPU tests compare against computes the same thing
    assert float((CO.roi_align(feat, rois, 0.25, 7, pair[1], pair[0]) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------
# GPU, forward
# ------------------------------------------------------------------------------------------------------
def _roi_case(seed, n=2, c=256, hw=(64, 96)):
    """The four-level case of tests/test_hip_ops.py: 300 boxes of 1..400 px, a zero-area box, border crossers, a padding row."""
    gg = g(seed)
    h, w = hw
    feats = [torch.randn(n, c, h // s, w // s, generator=gg) for s in (4, 8, 16, 32)]
    m = 300
    ctr = torch.rand(m, 2, generator=gg) * torch.tensor([w * 1.0, h * 1.0])
    size = torch.exp(torch.rand(m, 2, generator=gg) * 6.0)  # 1 .. 400 px: all four levels, tiny and huge
    boxes = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
    boxes[0] = torch.tensor([10.0, 10.0, 10.0, 10.0])      # zero area
    boxes[1] = torch.tensor([-50.0, -40.0, 30.0, 20.0])    # crosses the top-left border
    boxes[2] = torch.tensor([0.0, 0.0, float(w), float(h)])  # whole image
    boxes[3] = torch.tensor([w - 5.0, h - 5.0, w + 300.0, h + 300.0])  # mostly outside
    bidx = torch.randint(0, n, (m,), generator=gg, dtype=torch.int32)
    bidx[7] = -1
    return feats, boxes, bidx


def _pyramid_ref(fq, boxes, bidx, pair):
    """The C oracle per level, rows in list order; padding rows zero. fq: (n,c,h,w) per level."""
    lv = O.assign_levels(boxes)
    ref = torch.zeros(len(boxes), fq[0].shape[1], 7, 7)
    for l, s in enumerate(SCALES[:len(fq)]):
        ids = torch.nonzero((lv == l) & (bidx >= 0)).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
            ref[ids] = CO.roi_align(fq[l].float(), rois, s, 7, pair[1], pair[0])
    return ref


@functools.lru_cache(maxsize=None)
def _four_level_ref(dt, pair):
    feats, boxes, bidx = _roi_case(21)
    return _pyramid_ref([f.to(dt) for f in feats], boxes, bidx, pair)


def _check(out, ref, odt, name):
    if odt == torch.float32:
        assert_close(out, ref, rtol=1e-4, atol=1e-5, name=name)
    else:
        assert_close(out, ref, rtol=2.0 ** -10, atol=2e-3, name=name + " f16 out")


@pytest.mark.gpu
@pytest.mark.parametrize("pair", FWD_PAIRS, ids=_id)
@pytest.mark.parametrize("dt,odt", [(torch.float32, torch.float32), (torch.float16, torch.float32), (torch.float16, torch.float16),
                                    (torch.bfloat16, torch.float32)])
def test_roi_align_options_four_levels_vs_oracle(ops, dt, odt, pair):
    feats, boxes, bidx = _roi_case(21)
    out = ops.roi_align([nhwc(f.to(dt)).to(DEV) for f in feats], SCALES, boxes.to(DEV), bidx.to(DEV), 7, odt,
                        aligned=pair[0], sampling_ratio=pair[1])
    out = out.cpu().float().permute(0, 3, 1, 2)
    ref = _four_level_ref(dt, pair)
    assert float(out[7].abs().max()) == 0.0, "padding row"
    assert float(ref[0].abs().max()) > 0.0 and float(out[0].abs().max()) > 0.0, "zero-area row: the bilinear value at its point"
    _check(out[0:1], ref[0:1], odt, "zero-area row")
    _check(out, ref, odt, f"roi_align {_id(pair)}")


@pytest.mark.gpu
def test_roi_align_default_options_change_nothing(ops):
    feats, boxes, bidx = _roi_case(21)
    for dt, odt in ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.float32)):
        fl = [nhwc(f.to(dt)).to(DEV) for f in feats]
        a = ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 7, odt)
        b = ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 7, odt, aligned=True, sampling_ratio=0)
        assert torch.equal(a, b)
        assert float(a[0].abs().max()) == 0.0, "zero-area row under the default options"
        if odt == torch.float32:
            assert_close(a.cpu().permute(0, 3, 1, 2), _four_level_ref(dt, (True, 0)), rtol=1e-4, atol=1e-5, name="default")


@pytest.mark.gpu
def test_roi_align_options_do_not_depend_on_the_order(ops):
    feats, boxes, bidx = _roi_case(21)
    fl = [nhwc(f.half()).to(DEV) for f in feats]
    m = len(boxes)
    kw = dict(aligned=False, sampling_ratio=2)
    base = ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 7, torch.float32, order=torch.arange(m, dtype=torch.int32, device=DEV), **kw)
    loc = ops.roi_locality_order(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 4, 224, 2)
    for order in (None, loc, torch.arange(m - 1, -1, -1, dtype=torch.int32, device=DEV)):
        assert torch.equal(base, ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 7, torch.float32, order=order, **kw))


def _sweep_boxes(h, w):
    boxes = []
    for n_out in range(1, 41):            # footprint length along the streamed (shorter or equal) side, in level pixels
        for per_bin in (0.4, 1.0, 2.3, 3.1, 4.2, 5.5):  # bin size along the other side: 1..6 pixels per bin
            long_side = min(7 * per_bin, 52.0)
            short_side = max(n_out - 1.3, 0.2)
            x0, y0 = 3.3 + (n_out % 5) * 0.37, 2.6 + (n_out % 3) * 0.41
            boxes.append([x0, y0, x0 + long_side, y0 + short_side])    # streamed along y
            boxes.append([y0, x0, y0 + short_side, x0 + long_side])    # streamed along x
    boxes = torch.tensor(boxes, dtype=torch.float32) * 4.0  # one level at stride 4 (min_level = 2): image coordinates
    boxes[:, 2].clamp_(max=w * 4.0 - 1)
    boxes[:, 3].clamp_(max=h * 4.0 - 1)
    return boxes


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(True, 2), (False, 0)], ids=_id)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_roi_align_options_every_stream_length_and_inner_depth(ops, dt, pair):
    """The sweep of test_roi_align_every_stream_length_and_inner_depth (footprints of 1..40 steps, 1..6 pixels per bin, both
    orientations): every pipeline depth with zero-weight columns in the tables, and bins on both sides of the gather / stream
    switch-over (0.2 .. 5.5 pixels on the shorter side against 2 S = 4)."""
    gg = g(29)
    h, w, c = 56, 72, 16
    f = torch.randn(1, c, h, w, generator=gg).to(dt).float()
    boxes = _sweep_boxes(h, w)
    bidx = torch.zeros(len(boxes), dtype=torch.int32)
    out = ops.roi_align([nhwc(f).to(dt).to(DEV)], (0.25,), boxes.to(DEV), bidx.to(DEV), 7, torch.float32, min_level=2,
                        aligned=pair[0], sampling_ratio=pair[1]).cpu().float().permute(0, 3, 1, 2)
    ref = CO.roi_align(f, torch.cat((bidx.float().unsqueeze(1), boxes), dim=1), 0.25, 7, pair[1], pair[0])
    assert_close(out, ref, rtol=1e-4, atol=1e-5, name=f"stream sweep {_id(pair)}")


EXTREME = torch.tensor([
    [4.0, 100.0, 1300.0, 112.0],     # 324 x 3 px footprint: rows streamed, 47-column bins
    [300.0, 2.0, 330.0, 470.0],      # 7 x 117: columns streamed, 17-row bins
    [10.0, 10.0, 700.0, 400.0],      # big box, 25 x 14 px bins: the gather at S = 2
    [50.3, 60.2, 51.1, 61.0],        # a fifth of a pixel: every bin samples the same pixels
    [-40.0, -30.0, 90.0, 50.0],      # crosses the top-left border
    [1200.0, 400.0, 1400.0, 520.0],  # crosses the bottom-right border
    [0.0, 0.0, 1360.0, 480.0],       # the whole map
    [600.0, 200.0, 640.0, 203.0],    # 10 x 0.75
])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(False, 2), (True, 2), (True, 3), (False, 3), (True, 1), (True, 5)], ids=_id)
def test_roi_align_options_extreme_aspect_footprints(ops, pair):
    """The box lists of test_roi_align_extreme_aspect_footprints. Their 25 x 14, 47- and 72-column bins reach every gather
    instantiation (S = 1, 2 and 3: bins of at least 2 S pixels on the shorter side). (True, 5) has no gather instantiation: on the 24 x 500 map its
    whole-map box (71-pixel bins) overflows the tables and takes the per-sample loop with the fixed grid."""
    gg = g(23)
    f = torch.randn(2, 12, 120, 340, generator=gg)
    bidx = torch.tensor([0, 1, 0, 1, 0, 1, 1, 0], dtype=torch.int32)
    kw = dict(min_level=2, aligned=pair[0], sampling_ratio=pair[1])
    out = ops.roi_align([nhwc(f).to(DEV)], (0.25,), EXTREME.to(DEV), bidx.to(DEV), 7, torch.float32, **kw).cpu().permute(0, 3, 1, 2)
    ref = CO.roi_align(f, torch.cat((bidx.float().unsqueeze(1), EXTREME), 1), 0.25, 7, pair[1], pair[0])
    assert_close(out, ref, rtol=1e-4, atol=1e-5, name=f"extreme aspect {_id(pair)}")
    f2 = torch.randn(1, 4, 24, 500, generator=gg)
    b2 = torch.tensor([[0.0, 0.0, 2000.0, 96.0], [8.0, 8.0, 1900.0, 20.0]])
    z = torch.zeros(2, dtype=torch.int32)
    out2 = ops.roi_align([nhwc(f2).to(DEV)], (0.25,), b2.to(DEV), z.to(DEV), 7, torch.float32, **kw).cpu().permute(0, 3, 1, 2)
    assert_close(out2, CO.roi_align(f2, torch.cat((z.float().unsqueeze(1), b2), 1), 0.25, 7, pair[1], pair[0]), rtol=1e-4, atol=1e-5,
                 name=f"wide map {_id(pair)}")


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(False, 2), (True, 2), (True, 3), (False, 3), (True, 1)], ids=_id)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_roi_align_options_256_channels_every_path(ops, dt, pair):
    """The box list of test_roi_align_256_channels_every_path at the model's channel count: the gather (25- and 72-column bins), the
    streamed path, bins narrower than a pixel, every border, the entirely-outside box (zeros) and a zero-area box (not zeros)."""
    gg = g(29)
    f = torch.randn(2, 256, 60, 500, generator=gg).to(dt)
    boxes = torch.tensor([
        [4.0, 100.0, 1300.0, 112.0], [300.0, 2.0, 330.0, 230.0], [10.0, 10.0, 700.0, 200.0], [50.3, 60.2, 51.1, 61.0],
        [-40.0, -30.0, 90.0, 50.0], [1900.0, 200.0, 2100.0, 260.0], [0.0, 0.0, 2000.0, 240.0], [600.0, 100.0, 640.0, 103.0],
        [700.0, 50.0, 764.0, 114.0], [701.0, 51.0, 769.5, 113.0], [100.0, 100.0, 100.0, 100.0], [5000.0, 5000.0, 5100.0, 5100.0],
        [820.0, 20.0, 1020.0, 26.0],
    ])
    bidx = torch.tensor([0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=torch.int32)
    gb = torch.rand(40, 4, generator=gg)
    ctr = gb[:, :2] * torch.tensor([2000.0, 240.0])
    size = torch.exp(gb[:, 2:] * 5.5)
    boxes = torch.cat((boxes, torch.cat((ctr - size / 2, ctr + size / 2), dim=1)))
    bidx = torch.cat((bidx, torch.randint(0, 2, (40,), generator=gg, dtype=torch.int32)))
    bidx[20] = -1
    valid = bidx >= 0
    ref = torch.zeros(len(boxes), 256, 7, 7)
    ref[valid] = CO.roi_align(f.float(), torch.cat((bidx[valid].float().unsqueeze(1), boxes[valid]), 1), 0.25, 7, pair[1], pair[0])
    for odt in ((torch.float32,) if dt == torch.float32 else (torch.float32, torch.float16)):
        out = ops.roi_align([nhwc(f).to(DEV)], (0.25,), boxes.to(DEV), bidx.to(DEV), 7, odt, min_level=2, aligned=pair[0],
                            sampling_ratio=pair[1]).cpu().float().permute(0, 3, 1, 2)
        assert float(out[20].abs().max()) == 0.0 and float(out[11].abs().max()) == 0.0
        assert float(out[10].abs().max()) > 0.0
        _check(out, ref, odt, f"256 channels {_id(pair)}")


@pytest.mark.gpu
def test_roi_align_unaligned_fixed_grid_linear_ramp_is_exact(ops):
    """A plane is reproduced exactly at the bin centres by any symmetric grid: (False, 2) gives the plane at
    x1 + (pw + .5)(x2 - x1) / 7 with x1 = box / 16, no half-pixel shift."""
    ys, xs = torch.meshgrid(torch.arange(50.0), torch.arange(84.0), indexing="ij")
    f = (0.5 * xs - 0.25 * ys + 3.0).view(1, 1, 50, 84).expand(1, 4, 50, 84).contiguous()
    boxes = torch.tensor([[100.0, 80.0, 400.0, 390.0]])
    out = ops.roi_align([nhwc(f).to(DEV)], (1 / 16,), boxes.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 7, torch.float32,
                        min_level=4, aligned=False, sampling_ratio=2).cpu()[0, :, :, 0]
    x1, y1, x2, y2 = [v / 16 for v in boxes[0].tolist()]
    for ph in range(7):
        for pw in range(7):
            cx, cy = x1 + (pw + 0.5) * (x2 - x1) / 7, y1 + (ph + 0.5) * (y2 - y1) / 7
            assert out[ph, pw].item() == pytest.approx(0.5 * cx - 0.25 * cy + 3.0, rel=1e-5)


@pytest.mark.gpu
def test_roi_align_refuses_bad_options(ops, osr):
    feats, boxes, bidx = _roi_case(21, c=8)
    fl = [nhwc(f).to(DEV) for f in feats]
    for kw in (dict(sampling_ratio=-1), dict(sampling_ratio=65), dict(aligned=2)):
        with pytest.raises(ValueError):
            ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 7, torch.float32, **kw)
    # the C ABI itself: a status code and a message, nothing launched
    import ctypes as C
    lib = osr._lib.load()
    py = ops._pyramid(fl, SCALES)
    out = torch.full((len(boxes), 7, 7, 8), 7.0, device=DEV)
    for bad in (osr._lib.RoiOptions(1, -1), osr._lib.RoiOptions(1, 46341), osr._lib.RoiOptions(2, 0)):
        st = lib.osr_roi_align_fwd_ordered_opt(C.byref(py), 0, 2, C.c_void_p(boxes.to(DEV).data_ptr()), C.c_void_p(bidx.to(DEV).data_ptr()),
                                               len(boxes), 7, 4, 224, 2, None, None, 0, C.byref(bad), C.c_void_p(out.data_ptr()), 0, None)
        assert st == -1 and b"options" in lib.osr_last_error()
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------
# GPU, backward
# ------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(32, 48), (16, 24), (8, 12), (4, 6)]


def _bwd_case(seed, image_wh=(192.0, 128.0)):
    """The list of tests/test_train_bwd.py::test_roi_align_backward(_dense...) plus a zero-area box."""
    gg = g(seed)
    n, c, m = 2, 32, 60
    ctr = torch.rand(m, 2, generator=gg) * torch.tensor(image_wh)
    size = torch.exp(torch.rand(m, 2, generator=gg) * 5.0 + 0.5)
    boxes = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
    boxes[0] = torch.tensor([-20.0, -10.0, 40.0, 30.0])
    boxes[1] = torch.tensor([0.0, 0.0, image_wh[0], image_wh[1]])  # large RoI
    boxes[2] = torch.tensor([50.3, 60.2, 51.1, 61.0])    # sub-pixel
    boxes[3] = torch.tensor([4.0, 100.0, image_wh[0] - 2.0, 104.0])  # wide and thin
    boxes[4] = torch.tensor([70.0, 50.0, 70.0, 50.0])    # zero area
    bidx = torch.randint(0, n, (m,), generator=gg, dtype=torch.int32)
    dout = torch.randn(m, 7, 7, c, generator=gg)
    return n, c, boxes, bidx, dout


@pytest.mark.gpu
@pytest.mark.parametrize("pair", NEW_PAIRS, ids=_id)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_roi_align_options_backward_scatter(ops, dt, pair):
    n, c, boxes, bidx, dout = _bwd_case(81)
    bidx[5] = -1
    dout = dout.to(dt).float()
    got = ops.roi_align_bwd(dout.to(dt).to(DEV), BWD_SHAPES, n, SCALES, boxes.to(DEV), bidx.to(DEV), aligned=pair[0], sampling_ratio=pair[1])
    ref = _autograd_levels(BWD_SHAPES, n, c, boxes, bidx, dout, pair)
    for l in range(4):
        r = rel(got[l].permute(0, 3, 1, 2), ref[l])
        print(f"scatter {_id(pair)} level {l}: rel {r:.3e}")
        assert r < 1e-4, f"level {l}"


def _image_major(boxes, bidx, dout, n):
    """Reorder a RoI list into the (n, S) image-major layout the pixel-centric backward wants (padding rows: batch_idx -1)."""
    per = [torch.nonzero(bidx == b).squeeze(1) for b in range(n)]
    S = max(len(p) for p in per) + 2  # at least two padding rows per image
    bx = torch.zeros(n * S, 4)
    bi = torch.full((n * S,), -1, dtype=torch.int32)
    do = torch.zeros((n * S,) + tuple(dout.shape[1:]))
    src = torch.full((n * S,), -1, dtype=torch.int64)
    for b, ids in enumerate(per):
        bx[b * S:b * S + len(ids)] = boxes[ids]
        bi[b * S:b * S + len(ids)] = b
        do[b * S:b * S + len(ids)] = dout[ids]
        src[b * S:b * S + len(ids)] = ids
    do[bi < 0] = 7.0  # (garbage behind padding rows must not matter)
    return bx, bi, do, S, src


DENSE_SHAPES = [(30, 44), (15, 22), (8, 11), (4, 6)]  # a 176 x 120 image: no level is a multiple of the 8 x 8 tile on both axes


@pytest.mark.gpu
@pytest.mark.parametrize("pair", NEW_PAIRS, ids=_id)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_roi_align_options_backward_dense(ops, dt, pair):
    """osr_roi_align_bwd_dense_opt on an image-major list with padding rows and ragged tiles: against autograd, against the scatter
    kernel, bit-reproducible, and a gradient on the zero-area row reaches the pyramid (under the default options it reaches nothing)."""
    n, c, boxes, bidx, dout = _bwd_case(83, (176.0, 120.0))
    dout = dout.to(dt).float()
    bx, bi, do, S, src = _image_major(boxes, bidx, dout, n)
    kw = dict(aligned=pair[0], sampling_ratio=pair[1])
    args = (do.to(dt).to(DEV), DENSE_SHAPES, n, SCALES, bx.to(DEV), bi.to(DEV))
    got = ops.roi_align_bwd(*args, rois_per_image=S, **kw)
    again = ops.roi_align_bwd(*args, rois_per_image=S, **kw)
    scat = ops.roi_align_bwd(*args, **kw)
    ref = _autograd_levels(DENSE_SHAPES, n, c, boxes, bidx, dout, pair)
    for l in range(4):
        assert torch.equal(got[l], again[l]), "the gather has a fixed summation order"
        rs, ra = rel(got[l], scat[l]), rel(got[l].permute(0, 3, 1, 2), ref[l])
        print(f"dense {_id(pair)} level {l}: vs scatter {rs:.3e}, vs autograd {ra:.3e}")
        assert rs < 1e-5, f"level {l}: gather vs scatter"
        assert ra < 1e-4, f"level {l}"
    # the zero-area row alone
    only = torch.zeros_like(do)
    row = int(torch.nonzero(src == 4).item())
    only[row] = do[row]
    with_opt = ops.roi_align_bwd(only.to(dt).to(DEV), DENSE_SHAPES, n, SCALES, bx.to(DEV), bi.to(DEV), rois_per_image=S, **kw)
    default = ops.roi_align_bwd(only.to(dt).to(DEV), DENSE_SHAPES, n, SCALES, bx.to(DEV), bi.to(DEV), rois_per_image=S)
    assert float(with_opt[0].abs().max()) > 0.0 and all(float(t.abs().max()) == 0.0 for t in with_opt[1:])
    assert all(float(t.abs().max()) == 0.0 for t in default)


@pytest.mark.gpu
def test_roi_align_options_forward_and_backward_are_adjoint(ops):
    """<roi_align(f), g> == <f, roi_align_bwd(g)> at (False, 2) on the four-level case, image-major so that the backward is the
    reproducible gather. Tolerance: four times the relative difference of the same two inner products at the default options on the
    same inputs."""
    feats, boxes, bidx = _roi_case(21)
    n = 2
    gg = g(33)
    dout0 = torch.randn(len(boxes), 7, 7, 256, generator=gg)
    bx, bi, do, S, _ = _image_major(boxes, bidx, dout0, n)
    do[bi < 0] = 0.0
    fl = [nhwc(f).to(DEV) for f in feats]
    shapes = [(f.shape[2], f.shape[3]) for f in feats]
    gdev = do.to(DEV)

    def gap(**kw):
        out = ops.roi_align(fl, SCALES, bx.to(DEV), bi.to(DEV), 7, torch.float32, **kw)
        back = ops.roi_align_bwd(gdev, shapes, n, SCALES, bx.to(DEV), bi.to(DEV), rois_per_image=S, **kw)
        lhs = float((out.double() * gdev.double()).sum())
        rhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(fl, back))
        return abs(lhs - rhs) / max(abs(lhs), abs(rhs)), lhs, rhs

    base, bl, br = gap()
    new, nl, nr = gap(aligned=False, sampling_ratio=2)
    print(f"adjoint: default {bl:.9e} vs {br:.9e} (rel {base:.3e}); (ROIAlign, 2) {nl:.9e} vs {nr:.9e} (rel {new:.3e})")
    assert new <= 4.0 * base
