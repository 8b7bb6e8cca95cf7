"""osr_panoptic_pair_counts (csrc/osr_seg_eval.hip) against np.unique over (ground-truth row, predicted id)
(tests/seg_eval_common.py): exact equality of the whole table and of flags[0]."""
import numpy as np
import pytest
import torch

from tests.seg_eval_common import blocky, ids_to_rgb, pair_counts_reference

DEV = "cuda:0"


def _run(osr, ids_map, gt_ids, pred, num_pred, flags=None, out=None):
    flags = torch.zeros((3,), dtype=torch.int64, device=DEV) if flags is None else flags
    counts = osr.ops.panoptic_pair_counts(torch.from_numpy(ids_to_rgb(ids_map)).to(DEV), torch.tensor(gt_ids, dtype=torch.int32, device=DEV),
                                          torch.from_numpy(np.asarray(pred, dtype=np.int32)).to(DEV), num_pred, flags, out=out)
    return counts, flags


def _check(osr, ids_map, gt_ids, pred, num_pred):
    ref, bad = pair_counts_reference(ids_to_rgb(ids_map), gt_ids, pred, num_pred)
    counts, flags = _run(osr, ids_map, gt_ids, pred, num_pred)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (len(gt_ids) + 2, num_pred + 1)
    assert np.array_equal(counts.cpu().numpy(), ref)
    assert flags.tolist() == [bad, 0, 0]
    return ref, bad


# ids that use the G and B bytes, strictly ascending; 70000 is painted but not listed
GT_IDS = [3, 255, 256, 65535, 65536, 1193046, 16777215]
UNLISTED = 70000


def _blocky_case(h=61, w=83, p=9, seed=0):
    rng = np.random.default_rng(seed)
    palette = np.array([0] + GT_IDS + [UNLISTED], dtype=np.int64)  # VOID, the listed ids, the unlisted one
    ids_map = palette[blocky(rng, h, w, len(palette), cell=6)]
    pred = blocky(rng, h, w, p + 1, cell=9)  # 0 = VOID .. p
    return ids_map, pred


@pytest.mark.gpu
def test_blocky_maps_with_void_wide_ids_and_an_unlisted_id(osr):
    ids_map, pred = _blocky_case()
    ref, bad = _check(osr, ids_map, GT_IDS, pred, 9)
    assert bad == 0 and ref.sum() == 61 * 83
    assert ref[0].sum() > 0 and ref[:, 0].sum() > 0 and ref[len(GT_IDS) + 1].sum() == (ids_map == UNLISTED).sum() > 0
    assert all(ref[1 + i].sum() == (ids_map == v).sum() > 0 for i, v in enumerate(GT_IDS))


@pytest.mark.gpu
def test_a_predicted_id_above_p_goes_to_the_flag(osr):
    ids_map, pred = _blocky_case(seed=1)
    pred[7, 10:14], pred[8, 0] = 10, -1
    ref, bad = _check(osr, ids_map, GT_IDS, pred, 9)
    assert bad == 5 and ref.sum() == 61 * 83 - 5


@pytest.mark.gpu
def test_no_ground_truth_and_no_prediction(osr):
    ids_map, pred = _blocky_case(seed=2)
    ref, _ = _check(osr, ids_map, [], pred, 9)  # G = 0: VOID and unlisted only
    assert ref.shape == (2, 10) and ref[1].sum() == (ids_map != 0).sum()
    ref, _ = _check(osr, ids_map, GT_IDS, np.zeros_like(pred), 0)  # P = 0: one column
    assert ref.shape == (len(GT_IDS) + 2, 1)
    _check(osr, ids_map, [], np.zeros_like(pred), 0)


@pytest.mark.gpu
def test_the_largest_table(osr):
    """G = 1023 and P = 2047 on a 64 x 64 map: the table does not fit in LDS and is counted in global memory."""
    rng = np.random.default_rng(3)
    gt_ids = list(range(5, 5 + 2 * 1023, 2))  # odd ids; the even ones in between are unlisted
    ids_map = rng.integers(0, 5 + 2 * 1023 + 3, size=(64, 64))
    pred = rng.integers(0, 2048, size=(64, 64))
    ref, bad = _check(osr, ids_map, gt_ids, pred, 2047)
    assert bad == 0 and ref[1024].sum() > 0 and ref[1:1024].sum() > 0


@pytest.mark.gpu
def test_no_runs_map(osr):
    """Neighbouring pixels, and the pixels 256 apart that one thread visits in turn, all differ on both sides."""
    h, w = 61, 83
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    palette = np.array([0] + GT_IDS + [UNLISTED], dtype=np.int64)
    ids_map = palette[(idx + idx // 256) % len(palette)]
    pred = (idx * 3 + idx // 256) % 10
    _check(osr, ids_map, GT_IDS, pred, 9)


@pytest.mark.gpu
def test_the_call_zeroes_its_output(osr):
    ids_map, pred = _blocky_case(seed=4)
    ref, _ = pair_counts_reference(ids_to_rgb(ids_map), GT_IDS, pred, 9)
    out = torch.full((len(GT_IDS) + 2, 10), 12345, dtype=torch.int32, device=DEV)
    counts, flags = _run(osr, ids_map, GT_IDS, pred, 9, out=out)
    assert counts is out and np.array_equal(out.cpu().numpy(), ref)
    _run(osr, ids_map, GT_IDS, pred, 9, flags=flags, out=out)
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.gpu
def test_one_over_each_limit_is_refused_on_the_device_path(osr):
    ids_map, pred = np.zeros((8, 8), dtype=np.int64), np.zeros((8, 8), dtype=np.int64)
    with pytest.raises(osr.OsrError, match="at most 1023"):
        _run(osr, ids_map, list(range(1, 1025)), pred, 9)
    with pytest.raises(osr.OsrError, match="at most 1023"):
        _run(osr, ids_map, GT_IDS, pred, 2048)


def test_limits_are_refused_with_nothing_launched(osr):
    lib = osr._lib.load()
    a = torch.zeros(64, dtype=torch.int64).data_ptr()
    assert lib.osr_panoptic_pair_counts(a, a, 1024, a, 4, 4, 4, a, a, None) == osr._lib.ERR_UNSUPPORTED and b"at most 1023" in lib.osr_last_error()
    assert lib.osr_panoptic_pair_counts(a, a, 4, a, 2048, 4, 4, a, a, None) == osr._lib.ERR_UNSUPPORTED
    assert lib.osr_panoptic_pair_counts(a, a, -1, a, 4, 4, 4, a, a, None) == -1
    assert lib.osr_panoptic_pair_counts(None, a, 4, a, 4, 4, 4, a, a, None) == -1 and b"null pointer" in lib.osr_last_error()
    assert lib.osr_panoptic_pair_counts(a, a, 4, a, 4, 0, 4, a, a, None) == -1 and b"map" in lib.osr_last_error()
    assert lib.osr_pq_accumulate(a, 1024, 4, a, a, 3, a, a, a, None) == osr._lib.ERR_UNSUPPORTED
    assert lib.osr_pq_accumulate(a, 4, 2048, a, a, 3, a, a, a, None) == osr._lib.ERR_UNSUPPORTED
    assert lib.osr_pq_accumulate(a, 4, 4, a, a, 0, a, a, a, None) == -1 and b"categories" in lib.osr_last_error()
    assert lib.osr_pq_accumulate(None, 4, 4, a, a, 3, a, a, a, None) == -1 and b"null pointer" in lib.osr_last_error()


@pytest.mark.gpu
def test_a_workgroup_chunk_of_more_than_1024_pixels(osr):
    """1100 x 1000 pixels exceed 4 * 256 CUs * 1024: se_chunk gives a workgroup 2048 pixels, its first pixel is no longer
    blockIdx.x * 1024 and a thread walks eight pixels. On a device with more than 268 CUs the case stops reaching chunk > 1024."""
    h, w = 1100, 1000
    assert h * w > 4 * 256 * 1024
    ids_map, pred = _blocky_case(h, w)
    ref, bad = _check(osr, ids_map, GT_IDS, pred, 9)
    assert bad == 0 and ref.sum() == h * w and ref[0].sum() > 0 and ref[len(GT_IDS) + 1].sum() > 0
