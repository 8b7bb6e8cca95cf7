"""Generator of tests/golden/update_pin_v1.npz: fixed inputs of the training update and what the HIP library answered for them on
an MI355X at one commit (the fixture's `parent_commit`). tests/test_update_pin.py replays the inputs through the same replay() /
replay_trainers() and compares bit patterns and digests, so that a rewrite of the update is held to what it computed before it.

Provenance: DEVICE-generated, not oracle-generated: the record is the library's own earlier answer (tests/test_train_bwd.py and
tests/test_solver_options_gpu.py hold the same kernels to torch.optim.SGD and a float64 restatement). The recorded commit still had
three SGD kernels -- one launch per tensor, a table of whole tensors, a table of segments; main() asserts that all three give the
neutral set's bits before it writes the file, so that one record stands for the three. Regenerate only when the update's result is
meant to change, from a checkout that still has the three routes:
    python tests/golden/make_update_pin.py --parent <commit> [--out <file>]

Kernel cases (`in_k_*` inputs, `out_k_*` the record): six masters, momentum zero, the same gradient applied in two consecutive steps
  m0 (46, 360)  row scale, fp16 copy: 16 560 elements = one 16 384-element chunk + one of 176 (fewer than a workgroup's threads);
                the chunk boundary falls inside row 45, so the second chunk's row cursor starts mid-row
  m1 (5, 256)   two segments, rows [0, 4) and [4, 5) (the pred / rpn_tail shape)
  m2 (5,)       the same two segments; the one master of the bias group
  m3 (9, 33)    row scale, bf16 copy, segments [0, 4) and [4, 9): a segment and a row-scale pointer that do not start at row 0
  m4 (100, 33)  plain
  m5 (3, 7)     fp32 copy
under the option sets of SETS. The neutral set's p, v and copies are stored whole, the other sets' as a SHA-256 per tensor; the
norm partials of the second step are stored for every norm set.

Trainer cases (`tr_*`): voc_coco.yaml, base_rcnn_fpn.yaml and cascade_rcnn_fpn.yaml built under torch.manual_seed(0), a seeded
gradient in grad_flat, _update(1) twice, with the options off and with TRAINER_OPTIONS; the first 8 bytes of the SHA-256 of every
master, momentum buffer, low-precision copy and backward-data weight."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "update_pin_v1.npz")
INF = float("inf")
LARGEST_GOLDEN = 571641  # bytes: the record stays below the largest fixture committed before it

# ---- kernel cases ----
# (shape, row scale, copy dtype, row boundaries of its segments, bias group)
MASTERS = (((46, 360), True, torch.float16, (0, 46), False),
           ((5, 256), False, None, (0, 4, 5), False),
           ((5,), False, None, (0, 4, 5), True),
           ((9, 33), True, torch.bfloat16, (0, 4, 9), False),
           ((100, 33), False, None, (0, 100), False),
           ((3, 7), False, torch.float32, (0, 3), False))
LR, MU, WD, GS = 0.02, 0.9, 1e-4, 1.0 / 3072.0
# name -> (clip, clip value, norm type, bias lr factor, bias weight decay, nesterov, apply flag)
SETS = {"neutral": (None, 1.0, 2.0, 1.0, WD, False, 1),
        "value": ("value", 2e-4, 2.0, 1.0, WD, False, 1),
        "norm2": ("norm", 1e-3, 2.0, 1.0, WD, False, 1),
        "norminf_bias_nesterov": ("norm", 1e-3, INF, 2.0, 0.0, True, 1),
        "norm2_flag0": ("norm", 1e-3, 2.0, 1.0, WD, False, 0)}
NP_COPY = {torch.float16: np.uint16, torch.bfloat16: np.uint16, torch.float32: np.uint32}

# ---- trainer cases ----
YAMLS = ("voc_coco.yaml", "base_rcnn_fpn.yaml", "cascade_rcnn_fpn.yaml")
TRAINER_OPTIONS = (2.0, 0.0, True, "norm", 1e-2, 2.0)  # solver.SolverOptions, positionally


def make_inputs():
    g = torch.Generator().manual_seed(301)
    out = {}
    for i, (shape, scaled, _, _, _) in enumerate(MASTERS):
        out[f"in_k_m{i}_p"] = (torch.randn(shape, generator=g) * 0.05).numpy()
        out[f"in_k_m{i}_g"] = (torch.randn(shape, generator=g) * 3.0).numpy()
        if scaled:
            out[f"in_k_m{i}_rs"] = (torch.rand(shape[0], generator=g) + 0.5).numpy()
    return out


def _sha(t, n=None):
    h = hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest() if n is None else np.frombuffer(h.digest()[:n], np.uint8)


def _upload(inp, dev):
    ms = []
    for i, (shape, scaled, copy, _, _) in enumerate(MASTERS):
        d = dict(p=torch.from_numpy(inp[f"in_k_m{i}_p"]).to(dev), g=torch.from_numpy(inp[f"in_k_m{i}_g"]).to(dev))
        d["v"] = torch.zeros_like(d["p"])
        d["rs"] = torch.from_numpy(inp[f"in_k_m{i}_rs"]).to(dev) if scaled else None
        d["lp"] = torch.zeros(shape, dtype=copy, device=dev) if copy is not None else None
        ms.append(d)
    return ms


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).numpy()


def _segment_run(ops, ms, dev, name):
    clip, cv, p, factor, wd_bias, nesterov, flag_value = SETS[name]
    entries = [(d["p"], d["g"], d["v"], d["rs"], d["lp"], r0, r1, factor if bias else 1.0, wd_bias if bias else WD, nesterov)
               for d, (_, _, _, rows, bias) in zip(ms, MASTERS) for r0, r1 in zip(rows[:-1], rows[1:])]
    plan = ops.sgd_segment_plan(entries, torch.device(dev))
    for _ in range(2):
        flag = torch.full((1,), flag_value, dtype=torch.int32, device=dev)
        if clip == "norm":
            ops.grad_norm_partials_(plan, GS, p, flag)
        ops.sgd_step_multi_ex_(plan, LR, MU, GS, clip, cv, p, flag)
    torch.cuda.synchronize()
    return plan


def replay(ops, inp, dev):
    """Runs every kernel case on `dev`; -> {name: numpy array} under the names of the fixture's `out_k_` entries (without the prefix)."""
    out = {}
    for name in SETS:
        ms = _upload(inp, dev)
        plan = _segment_run(ops, ms, dev, name)
        for i, d in enumerate(ms):
            for key in ("p", "v", "lp"):
                if d[key] is not None:
                    out[f"{name}_m{i}_{key}"] = _bits(d[key]) if name == "neutral" else np.array(_sha(d[key]))
        if SETS[name][0] == "norm":
            out[f"{name}_partials"] = plan.partials.cpu().numpy().view(np.int64)
    return out


def parent_routes(ops, inp, dev):
    """The neutral set through the two launches this record's commit had beside the segment launch: one launch per tensor and the
    table of whole tensors. -> two dicts under replay()'s names."""
    res = []
    for multi in (False, True):
        ms = _upload(inp, dev)
        if multi:
            plan = ops.sgd_multi_plan([(d["p"], d["g"], d["v"], d["rs"], d["lp"]) for d in ms], torch.device(dev))
        for _ in range(2):
            if multi:
                ops.sgd_step_multi_(plan, LR, MU, WD, GS)
            else:
                for d in ms:
                    ops.sgd_step_(d["p"], d["g"], d["v"], LR, MU, WD, GS, d["rs"], d["lp"])
        torch.cuda.synchronize()
        res.append({f"neutral_m{i}_{key}": _bits(d[key]) for i, d in enumerate(ms) for key in ("p", "v", "lp") if d[key] is not None})
    return res


def _cfg(yaml, dev):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", dev, "OPENDET_BENCHMARK", "True"])
    return cfg


def replay_trainers(dev):
    """-> {"<yaml stem>_<off|on>_names": array of "<group>/<key>", "<yaml stem>_<off|on>_sha8": (len(names), 8) uint8}."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.solver import SolverOptions
    out = {}
    for yaml in YAMLS:
        torch.manual_seed(0)
        model = M.build_model(_cfg(yaml, dev))
        model.train()
        for tag, opts in (("off", None), ("on", SolverOptions(*TRAINER_OPTIONS))):
            tr = model.make_trainer()
            tr.solver_options = opts
            g = torch.Generator().manual_seed(302)
            tr.grad_flat.copy_(torch.randn(tr.grad_flat.numel(), generator=g) * (tr.loss_scale * 1e-3))
            for _ in range(2):
                tr._update(1)
            torch.cuda.synchronize()
            assert not tr.poll_overflow(wait=True)
            groups = dict(master=tr.master, mom=tr.mom, lowp={k: v for k, v in tr.lowp.items() if v is not None}, wd=tr.wd)
            names = [f"{grp}/{k}" for grp, d in groups.items() for k in d]
            pre = f"{yaml[:-5]}_{tag}"
            out[pre + "_names"] = np.array(names)
            out[pre + "_sha8"] = np.stack([_sha(groups[n.split("/", 1)[0]][n.split("/", 1)[1]], 8) for n in names])
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit whose library answers are recorded")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg._lib.load()
    dev = "cuda:0"
    inp = make_inputs()
    rec = replay(pkg.ops, inp, dev)
    _same(rec, replay(pkg.ops, inp, dev))  # the record must be a fixed point of the library it was taken from
    neutral = {k: v for k, v in rec.items() if k.startswith("neutral_m")}
    for route in parent_routes(pkg.ops, inp, dev):  # one record for the three SGD kernels of this commit
        _same(route, neutral)
    for i in range(len(MASTERS)):  # the record is of an update that happened
        assert not np.array_equal(rec[f"neutral_m{i}_p"], _bits(torch.from_numpy(inp[f"in_k_m{i}_p"]))), i
        assert rec[f"norm2_flag0_m{i}_p"] == _sha(torch.from_numpy(inp[f"in_k_m{i}_p"])), i
    trainers = replay_trainers(dev)
    _same(trainers, replay_trainers(dev))
    for k in sorted(rec):
        if k.endswith("_partials"):
            print(k, rec[k].view(np.float64).tolist())
    for k in sorted(trainers):
        if k.endswith("_names"):
            print(k, len(trainers[k]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, parent_commit=np.array(args.parent), device=np.array(torch.cuda.get_device_name(0)),
                        **inp, **{"out_k_" + k: v for k, v in rec.items()}, **{"tr_" + k: v for k, v in trainers.items()})
    size = os.path.getsize(args.out)
    print("wrote", args.out, size, "bytes")
    assert size < LARGEST_GOLDEN, size


if __name__ == "__main__":
    main()
