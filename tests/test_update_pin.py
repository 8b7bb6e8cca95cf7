"""The training update, pinned to what it computed while the library still had three SGD kernels (one launch per tensor, a table of
whole tensors, a table of segments) and two host paths: tests/golden/update_pin_v1.npz holds fixed inputs and the library's answers
on an MI355X at the fixture's `parent_commit` (tests/golden/make_update_pin.py generates both, describes the cases, and asserted at
recording time that the three kernels gave the neutral set's bits). Kernel cases: the inputs are replayed through
ops.sgd_segment_plan / ops.grad_norm_partials_ / ops.sgd_step_multi_ex_, two steps per option set; the neutral set is compared by bit
pattern, the other sets by SHA-256 per tensor, the norm partials by bit pattern. Trainer cases: three model families, options off and
on, two _update(1) calls from a seeded gradient; every master, momentum buffer, low-precision copy and backward-data weight by
digest."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gen(osr, golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    spec = importlib.util.spec_from_file_location("make_update_pin", os.path.join(golden_dir, "make_update_pin.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record(golden_dir):
    z = np.load(os.path.join(golden_dir, "update_pin_v1.npz"))
    assert len(str(z["parent_commit"])) == 40
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def kernels(osr, gen, record):
    want = {k[6:]: v for k, v in record.items() if k.startswith("out_k_")}
    return gen.replay(osr.ops, {k: v for k, v in record.items() if k.startswith("in_k_")}, DEV), want


@pytest.fixture(scope="module")
def trainers(gen, record):
    return gen.replay_trainers(DEV), {k[3:]: v for k, v in record.items() if k.startswith("tr_")}


def test_every_recorded_key_is_replayed(gen, record, kernels, trainers):
    for got, want in (kernels, trainers):
        assert sorted(got) == sorted(want)
    prefixes = ("in_k_", "out_k_", "tr_", "parent_commit", "device")
    assert all(k.startswith(prefixes) for k in record)
    assert len(kernels[1]) >= len(gen.SETS) * 2 * len(gen.MASTERS) and len(trainers[1]) == 2 * 2 * len(gen.YAMLS)


@pytest.mark.parametrize("name", ["neutral", "value", "norm2", "norminf_bias_nesterov", "norm2_flag0"])
def test_kernel_outputs_are_the_recorded_bits(gen, kernels, name):
    assert name in gen.SETS and len(gen.SETS) == 5
    got, want = kernels
    keys = [k for k in sorted(want) if k.startswith(name + "_m") or k == name + "_partials"]
    assert len(keys) == 2 * len(gen.MASTERS) + 3 + (gen.SETS[name][0] == "norm")  # p and v of every master, three copies, the partials
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if w.dtype.kind == "U":
            assert str(g) == str(w), k
        else:
            bad = np.argwhere(g != w)
            assert bad.size == 0, f"{k}: {len(bad)} of {w.size} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]}, recorded {w[tuple(bad[0])]}"


@pytest.mark.parametrize("tag", ["off", "on"])
@pytest.mark.parametrize("yaml", ["voc_coco.yaml", "base_rcnn_fpn.yaml", "cascade_rcnn_fpn.yaml"])
def test_trainer_update_gives_the_recorded_digests(gen, trainers, yaml, tag):
    assert yaml in gen.YAMLS and len(gen.YAMLS) == 3
    got, want = trainers
    pre = f"{yaml[:-5]}_{tag}"
    names = [str(n) for n in want[pre + "_names"]]
    assert [str(n) for n in got[pre + "_names"]] == names
    assert {n.split("/")[0] for n in names} == {"master", "mom", "lowp", "wd"} and len(names) > 200
    bad = [n for n, g, w in zip(names, got[pre + "_sha8"], want[pre + "_sha8"]) if g.tobytes() != w.tobytes()]
    assert not bad, f"{len(bad)} of {len(names)} tensors differ from the record: {bad[:8]}"
