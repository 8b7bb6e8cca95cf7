"""osr_heatmaps_to_keypoints (csrc/osr_keypoint.hip) against [d2] heatmaps_to_keypoints restated per RoI with F.interpolate(bicubic)
in float64 (tests/keypoint_common.py decode_chain).

maps = 2 * randn(10, 17, 56, 56) under seed 5; ten boxes at binary-fraction offsets (their sides are then exact in fp32, so ceil() is
the same in every precision) with (w, h) = (0.4, 0.7) the 1 x 1 clamp, (1, 1) a single pixel, (3.2, 7.5) and (20, 30) downscales,
(56, 56) the identity, (57, 113), (112, 112), (96.5, 250.25) upscales, (333, 47.9) thin, (500, 300) large.

Measured on the CPU on these inputs: the float64 reference's smallest gap between the largest and the second largest resized value
is 2.2e-3; torch's own fp32 interpolation stays within e32 = 1.6e-5 of float64 and picks the same 170 positions. The test therefore
  - asserts that gap > 1e-3 for every (RoI, keypoint) with more than one pixel (the inputs are well conditioned; nothing is skipped);
  - requires x and y from exactly the reference position: within 1e-4 px of the reference (the float rounding of the affine map);
  - requires logit within max(4 * e32, 1e-5) (4: another product order and fp32 coordinates);
  - requires score within a relative 4 * (e32 of the score), floor 1e-5.
Measured on the MI355X: every position the reference's, |dx|, |dy| <= 9e-6 px; ten boxes |dlogit| 1.6e-5 (e32 1.6e-5), relative
|dscore| 1.6e-5 (e32 1.6e-5); m = 32: 5.8e-6 / 5.7e-6 (e32 5.8e-6); 1333 x 800: 1.7e-6 / 1.7e-6 (e32 1.7e-6), gap 1.1e-3;
m = 36, k = 17: 1.4e-5 / 1.4e-5 (e32 1.5e-5), gap 3.1e-3; m = 52, k = 17: 1.6e-5 / 1.6e-5 (e32 1.5e-5), gap 1.7e-2."""
import functools

import pytest
import torch

from tests.keypoint_common import boxes_at, decode_chain

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(0.4, 0.7), (1, 1), (3.2, 7.5), (20, 30), (56, 56), (57, 113), (112, 112), (96.5, 250.25), (333, 47.9), (500, 300)]
OFFSETS = [(10.25, 3.5), (0.0, 0.0), (7.125, 2.75), (40.5, 60.25), (3.0, 9.0), (12.75, 1.5), (100.0, 50.0), (3.125, 7.5), (5.5, 2.25), (20.25, 30.5)]
GAP = 1e-3
XY_TOL = 1e-4


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


@functools.lru_cache(maxsize=None)
def _main_case():
    torch.manual_seed(5)
    maps = 2 * torch.randn(10, 17, 56, 56)
    rois = boxes_at(OFFSETS, SIZES)
    return maps, rois, decode_chain(maps, rois, torch.float64), decode_chain(maps, rois, torch.float32)


def _errors(ref, r32):
    e_logit = float((r32["logit"].double() - ref["logit"]).abs().max())
    e_score = float(((r32["score"].double() - ref["score"]).abs() / ref["score"]).max())
    return e_logit, e_score


def _check(out, ref, r32, what):
    """out (r, k, 4) from the kernel against the float64 reference under the module docstring's rules; returns the measured errors."""
    e_logit, e_score = _errors(ref, r32)
    many = (ref["size"][:, 0] * ref["size"][:, 1] > 1)[:, None].expand_as(ref["gap"])
    assert float(ref["gap"][many].min()) > GAP, f"{what}: the reference gap must exceed {GAP}"
    o = out.cpu().double()
    dx, dy = float((o[..., 0] - ref["x"]).abs().max()), float((o[..., 1] - ref["y"]).abs().max())
    dl = float((o[..., 2] - ref["logit"]).abs().max())
    ds = float(((o[..., 3] - ref["score"]).abs() / ref["score"]).max())
    print(f"{what}: |dx| {dx:.2e} |dy| {dy:.2e} px; |dlogit| {dl:.2e} (e32 {e_logit:.2e}); rel |dscore| {ds:.2e} (e32 {e_score:.2e}); "
          f"min gap {float(ref['gap'][many].min()) if bool(many.any()) else float('inf'):.2e}")
    assert dx <= XY_TOL and dy <= XY_TOL, f"{what}: a position differs from the reference's ({dx:.3e}, {dy:.3e} px)"
    assert dl <= max(4 * e_logit, 1e-5), f"{what}: logit error {dl:.3e} > max(4 * {e_logit:.3e}, 1e-5)"
    assert ds <= max(4 * e_score, 1e-5), f"{what}: relative score error {ds:.3e} > max(4 * {e_score:.3e}, 1e-5)"
    return dx, dy, dl, ds


def test_against_the_float64_reference(ops):
    maps, rois, ref, r32 = _main_case()
    assert torch.equal(r32["pos"], ref["pos"]), "torch's own fp32 interpolation picks the reference positions"
    # two positions of one map are at least a pixel step apart in x or y: 1e-4 px pins the position
    out = ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV))
    assert out.shape == (10, 17, 4) and out.dtype == torch.float32
    _check(out, ref, r32, "ten boxes")
    assert torch.equal(ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)), out), "two runs are bit-identical"


def test_identity_scale_copies_and_breaks_ties_towards_the_lower_index(ops):
    """A 56 x 56 box: scale 1, t = 0, the cubic weights are exactly (0, 1, 0, 0) and the resize is a copy. Two equal maxima planted in
    one map: the lower row-major position wins and the logit is the planted value bit for bit."""
    torch.manual_seed(6)
    maps = torch.randn(1, 3, 56, 56)
    planted = float(torch.tensor(7.123456, dtype=torch.float32))
    maps[0, 1, 40, 3] = planted
    maps[0, 1, 12, 50] = planted  # (row 12 comes first in row-major order)
    maps[0, 2, 55, 55] = planted
    rois = boxes_at([(8.5, 2.25)], [(56, 56)])
    out = ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)).cpu()
    assert float(out[0, 1, 2]) == planted and float(out[0, 2, 2]) == planted
    assert (float(out[0, 1, 0]), float(out[0, 1, 1])) == (50.5 + 8.5, 12.5 + 2.25)
    assert (float(out[0, 2, 0]), float(out[0, 2, 1])) == (55.5 + 8.5, 55.5 + 2.25)
    am = int(maps[0, 0].flatten().argmax())
    assert float(out[0, 0, 2]) == float(maps[0, 0].max()) and (float(out[0, 0, 0]), float(out[0, 0, 1])) == (am % 56 + 0.5 + 8.5, am // 56 + 0.5 + 2.25)
    want = 1.0 / torch.exp(maps[0].double().reshape(3, -1) - out[0, :, 2].double()[:, None]).sum(1)
    assert float(((out[0, :, 3].double() - want).abs() / want).max()) <= 1e-5


def test_smaller_maps_and_fewer_keypoints(ops):
    torch.manual_seed(7)
    maps = 2 * torch.randn(4, 5, 32, 32)
    rois = boxes_at([(1.5, 2.25), (0.0, 4.0), (9.75, 0.5), (2.0, 2.0)], [(32, 32), (45.5, 70), (10, 13.25), (150, 90)])
    ref, r32 = decode_chain(maps, rois, torch.float64), decode_chain(maps, rois, torch.float32)
    _check(ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)), ref, r32, "m = 32, k = 5")


@pytest.mark.parametrize("m,seed", [(36, 31), (52, 33)])
def test_the_map_sizes_of_the_other_pooler_resolutions(ops, m, seed):
    """m = 4 s for s = 9 and 13: lanes m .. 63 of a wave sit out the vertical blend, the map is no multiple of the 256 staging threads.
    Measured on the CPU: the float64 reference's smallest gap is 3.1e-3 (m = 36) and 1.7e-2 (m = 52); torch's fp32 chain picks the
    same positions."""
    torch.manual_seed(seed)
    maps = 2 * torch.randn(4, 17, m, m)
    rois = boxes_at([(1.5, 2.25), (0.0, 4.0), (9.75, 0.5), (2.0, 2.0)], [(m, m), (45.5, 70), (10, 13.25), (150, 90)])
    ref, r32 = decode_chain(maps, rois, torch.float64), decode_chain(maps, rois, torch.float32)
    assert torch.equal(r32["pos"], ref["pos"]), "torch's own fp32 interpolation picks the reference positions"
    _check(ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)), ref, r32, f"m = {m}, k = 17")


def test_an_image_sized_box(ops):
    """1333 x 800: 1 066 400 resized values per map, 200 barriers of four rows, 21 column steps per lane."""
    torch.manual_seed(8)
    maps = 2 * torch.randn(1, 2, 56, 56)
    rois = boxes_at([(0.0, 0.0)], [(1333, 800)])
    ref, r32 = decode_chain(maps, rois, torch.float64), decode_chain(maps, rois, torch.float32)
    assert tuple(ref["size"][0]) == (800, 1333)
    _check(ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)), ref, r32, "1333 x 800")


def test_padding_rows_are_zeros(ops, osr):
    """Six RoIs as three segments of two with rows_valid (2, 0, 1): RoIs 2, 3 and 5 do not exist (their maps and boxes hold NaN)."""
    maps, rois, ref, r32 = _main_case()
    idx = [4, 5, 0, 0, 7, 0]
    m, b = maps[idx].clone(), rois[idx].clone()
    m[[2, 3, 5]] = float("nan")
    b[[2, 3, 5]] = float("nan")
    rv = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    out = ops.heatmaps_to_keypoints(m.to(DEV), b.to(DEV), rv, 2).cpu()
    full = ops.heatmaps_to_keypoints(maps.to(DEV), rois.to(DEV)).cpu()
    for i, src in enumerate(idx):
        if i in (0, 1, 4):
            assert torch.equal(out[i], full[src]), i
        else:
            assert float(out[i].abs().max()) == 0.0, f"RoI {i} must be zeros"
    with pytest.raises(osr.OsrError, match="rows_valid"):
        ops.heatmaps_to_keypoints(m.to(DEV), b.to(DEV), rv[:2].contiguous(), 2)


def test_no_rois_and_shape_rules(ops, osr):
    out = ops.heatmaps_to_keypoints(torch.zeros(0, 17, 56, 56, device=DEV), torch.zeros(0, 4, device=DEV))
    assert out.shape == (0, 17, 4) and out.dtype == torch.float32
    with pytest.raises(osr.OsrError, match="56"):
        ops.heatmaps_to_keypoints(torch.zeros(1, 2, 57, 57, device=DEV), torch.zeros(1, 4, device=DEV))
    with pytest.raises(osr.OsrError, match="rois"):
        ops.heatmaps_to_keypoints(torch.zeros(2, 2, 56, 56, device=DEV), torch.zeros(1, 4, device=DEV))
