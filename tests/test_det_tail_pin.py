"""The stock detection tails in front of the NMS, pinned to what they computed before their decode and their candidates kernel were
merged: tests/golden/det_tail_pin_v1.npz holds fixed inputs and the library's answers on an MI355X at the fixture's `parent_commit`
(tests/golden/make_det_tail_pin.py generates both and describes the cases). The inputs are replayed through ops.box_predictor_tail,
ops.rpn_select (decode mode 1), ops.retinanet_select, ops.fastrcnn_candidates, ops.cascade_candidates (1 .. 4 stages) and
ops.cascade_refine (with and without ground truth and drop_empty); every output is compared by bit pattern, and a position that is
NaN in the record only has to be NaN."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pin(osr, golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    spec = importlib.util.spec_from_file_location("make_det_tail_pin", os.path.join(golden_dir, "make_det_tail_pin.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(os.path.join(golden_dir, "det_tail_pin_v1.npz"))
    want = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    got = gen.replay(osr.ops, {k: z[k] for k in z.files if k.startswith("in_")}, DEV)
    assert len(str(z["parent_commit"])) == 40
    return got, want


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


CASES = {
    "fastrcnn_candidates": ("cand_fr1_", "cand_fr3_"),
    "cascade_candidates_1_stage": ("cand_cc1_",),
    "cascade_candidates_2_stages": ("cand_cc2_",),
    "cascade_candidates_3_stages": ("cand_cc3_",),
    "cascade_candidates_4_stages": ("cand_cc4_",),
    "rpn_select": ("rpn_",),
    "retinanet_select": ("retina_",),
    "box_predictor_tail": ("tail0_", "tail1_"),
    "cascade_refine": ("refine_gt0_drop0_", "refine_gt0_drop1_", "refine_gt1_drop0_", "refine_gt1_drop1_"),
}


def test_every_recorded_output_belongs_to_a_case(pin):
    got, want = pin
    prefixes = tuple(p for ps in CASES.values() for p in ps)
    assert sorted(got) == sorted(want)
    assert all(k.startswith(prefixes) for k in want)


@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_are_the_recorded_bits(pin, case):
    got, want = pin
    keys = [k for k in sorted(want) if k.startswith(CASES[case])]
    assert len(keys) >= 3 * len(CASES[case])
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if w.dtype.kind == "f":
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), k
            g, w = np.where(nan, 0, _bits(g)), np.where(nan, 0, _bits(w))
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{k}: {len(bad)} of {w.size} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]}, recorded {w[tuple(bad[0])]}"
