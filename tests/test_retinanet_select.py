"""osr_retinanet_select (csrc/osr_retinanet.hip) against the contract in include/osr.h, restated here on the CPU: candidates
`logit > logit_thresh` over the real channels, a stable sort on an exact integer key (logit descending, flat index ascending), the
first topk, anchors formed in fp32, Box2BoxTransform.apply_deltas in float64.

Indices, classes, counts, c_cand and the order are compared exactly. Scores: within 1e-6 of torch.sigmoid in fp32 (the bound of the
cascade candidates test). Boxes: each coordinate within 12 * 2^-24 * S, S the sum of the magnitudes of that coordinate's terms
(|cx|, |dx * aw|, 0.5 * |pw|) in float64: eleven fp32 roundings on the way to a coordinate (two for the anchor corners, the extent,
the half extent and centre, the division, the product and sum, the clamp's division, expf's product, the half width, the final sum)
with expf assumed within 2 ulp -- an assumption. |dw|, |dh| <= 1.5 in the bounded cases. Measured on an MI355X: scores within 1.2e-7, box
coordinates at most 0.22 of the bound."""
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
CLAMP = math.log(1000.0 / 16.0)
A = 9
# csrc/osr_retinanet.hip: a filter workgroup's chunk (RN_FILTER_THREADS * RN_FILTER_ITEMS vectors of 16 bytes) and the smallest
# survivor list (RN_MIN_SURVIVORS); a list holds max(that, count / 32 + 1) pairs, never more than the segment has elements
CHUNK_BYTES = 256 * 8 * 16
MIN_SURVIVORS = 4096

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _package(osr):
    """(the product package is importable as openset_rcnn_amd once the session fixture has loaded it)"""


def _ops():
    from openset_rcnn_amd.host import ops
    return ops


def cell_anchors(levels):
    """(L, A, 4): three sizes x three ratios per level, size-major ([d2] generate_cell_anchors), fp32."""
    rows = []
    for _, _, s in levels:
        cells = []
        for z in (4.0 * s, 4.0 * s * 2 ** (1 / 3), 4.0 * s * 2 ** (2 / 3)):
            for r in (0.5, 1.0, 2.0):
                w = math.sqrt(z * z / r)
                h = r * w
                cells.append([-w / 2, -h / 2, w / 2, h / 2])
        rows.append(cells)
    return torch.tensor(rows, dtype=torch.float32)


def float_key(z):
    """fp32 -> int64, order preserving, -0 folded onto +0."""
    u = (z + 0.0).contiguous().view(torch.int32).to(torch.int64)
    return torch.where(u >= 0, u, -(u & 0x7FFFFFFF))


def reference(levels, n, k_cls, topk, thresh, rw, logits, deltas, anchors):
    """logits[l] (n, h, w, pitch_cls) any float dtype, deltas[l] (n, h, w, pitch_box) fp32 -> the padded outputs + per-coordinate S."""
    nl = len(levels)
    cap = nl * topk
    o = dict(c_boxes=torch.zeros(n, cap, 4, dtype=torch.float64), c_scores=torch.zeros(n, cap), c_cls=torch.full((n, cap), -1, dtype=torch.int32),
             c_cand=torch.zeros(n, cap, dtype=torch.int32), c_src=torch.full((n, cap), -1, dtype=torch.int32), counts=torch.zeros(n, nl, dtype=torch.int32),
             scale=torch.zeros(n, cap, 4, dtype=torch.float64), flag=0)
    th = torch.tensor(thresh, dtype=torch.float32)
    for li, (h, w, stride) in enumerate(levels):
        for img in range(n):
            z = logits[li][img, :, :, :A * k_cls].float().reshape(-1)
            idx = torch.nonzero(z > th).reshape(-1)
            order = torch.sort(-float_key(z[idx]), stable=True).indices[:topk]
            idx = idx[order]
            cnt = idx.numel()
            sl = slice(li * topk, li * topk + cnt)
            o["counts"][img, li] = cnt
            if cnt == 0:
                continue
            zz = z[idx]
            t = idx // k_cls
            cell, a = t // A, t % A
            d = deltas[li][img].reshape(h * w, -1)[cell][:, :4 * A].reshape(cnt, A, 4)[torch.arange(cnt), a]
            sx, sy = ((cell % w) * stride).float(), ((cell // w) * stride).float()
            ca = anchors[li][a]
            ax1, ay1, ax2, ay2 = (sx + ca[:, 0]).double(), (sy + ca[:, 1]).double(), (sx + ca[:, 2]).double(), (sy + ca[:, 3]).double()
            aw, ah = ax2 - ax1, ay2 - ay1
            cx, cy = ax1 + 0.5 * aw, ay1 + 0.5 * ah
            dd = d.double()
            dx, dy = dd[:, 0] / rw[0], dd[:, 1] / rw[1]
            dw, dh = torch.clamp(dd[:, 2] / rw[2], max=CLAMP), torch.clamp(dd[:, 3] / rw[3], max=CLAMP)
            pw, ph = torch.exp(dw) * aw, torch.exp(dh) * ah
            box = torch.stack((dx * aw + cx - 0.5 * pw, dy * ah + cy - 0.5 * ph, dx * aw + cx + 0.5 * pw, dy * ah + cy + 0.5 * ph), dim=1)
            sxs, sys_ = cx.abs() + (dx * aw).abs() + 0.5 * pw.abs(), cy.abs() + (dy * ah).abs() + 0.5 * ph.abs()
            valid = torch.isfinite(d).all(dim=1) & torch.isfinite(box.float()).all(dim=1)
            if not bool(valid.all()):
                o["flag"] = 1
            o["c_boxes"][img, sl] = torch.where(valid[:, None], box, torch.zeros(()).double())
            o["scale"][img, sl] = torch.where(valid[:, None], torch.stack((sxs, sys_, sxs, sys_), dim=1), torch.zeros(()).double())
            o["c_scores"][img, sl] = torch.sigmoid(zz)
            o["c_cls"][img, sl] = (idx % k_cls).to(torch.int32)
            o["c_cand"][img, sl] = valid.to(torch.int32)
            o["c_src"][img, sl] = idx.to(torch.int32)
    return o


def run(levels, n, k_cls, topk, score_thresh, rw, logits, deltas, anchors, out=None):
    ops = _ops()
    lv = ops.make_rpn_levels([(h, w) for h, w, _ in levels], [s for _, _, s in levels], n, A)
    lg = torch.cat([x.reshape(-1) for x in logits]).to(DEV)
    dl = torch.cat([x.reshape(-1) for x in deltas]).to(DEV)
    return ops.retinanet_select(lv, anchors.to(DEV), lg, dl, n, k_cls, topk, score_thresh, rw, pitch_cls=logits[0].shape[-1],
                                pitch_box=deltas[0].shape[-1], out=out), lv


def compare(got, ref, report=None):
    for key in ("counts", "c_cls", "c_cand", "c_src"):
        assert torch.equal(got[key].cpu(), ref[key]), key
    err_s = (got["c_scores"].cpu() - ref["c_scores"]).abs().max().item()
    err = (got["c_boxes"].cpu().double() - ref["c_boxes"]).abs()
    bound = 12.0 * 2.0 ** -24 * ref["scale"]
    frac = torch.where(bound > 0, err / bound.clamp(min=1e-300), err * 0).max().item()
    print(f"retinanet_select: score error {err_s:.3e}, box error / bound {frac:.3f} (max abs {err.max().item():.3e})")
    if report is not None:
        report.update(score=err_s, frac=frac)
    assert err_s <= 1e-6
    assert bool((err <= bound).all()), f"box error {frac:.3f} of the bound"
    assert int(got["status_flags"].item()) & 1 == ref["flag"]


def make_case(levels, n, k_cls, dtype, pad, seed, shift, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    pc, pb = A * k_cls + (8 if pad else 0), 4 * A + (4 if pad else 0)
    logits, deltas = [], []
    for h, w, _ in levels:
        z = torch.full((n, h, w, pc), float("inf"))  # padding channels hold +inf: they must never appear
        z[..., :A * k_cls] = torch.randn((n, h, w, A * k_cls), generator=g) * scale + shift
        logits.append(z.to(dtype))
        d = torch.full((n, h, w, pb), float("nan"))
        d[..., :4 * A] = (torch.rand((n, h, w, 4 * A), generator=g) * 2 - 1) * 1.5
        deltas.append(d)
    return logits, deltas


LEVELS = [(8, 8, 8), (4, 4, 16), (2, 1, 32)]
THRESH = 0.05


def logit_thresh(t=THRESH):
    return float(np.float32(math.log(t / (1.0 - t))))


# shift of the N(0, 1) logits: about 0.5 % / 5 % / 50 % of them pass the threshold -2.944. With K = 80 the 8 x 8 level has 46 080
# elements and a survivor list of 4096: "sparse" stays below topk = 1000, "mid" (about 2200) takes the radix select on the list,
# "dense" (about 23 000) overflows the list: the threshold is raised on the device and the segment filtered again.
@pytest.mark.parametrize("flavour,shift", [("sparse", -5.5), ("mid", -4.6), ("dense", -3.0)])
@pytest.mark.parametrize("k_cls,topk,pad,dtype", [(80, 1000, False, torch.float16), (80, 8, True, torch.float16), (3, 8, True, torch.float32),
                                                  (3, 1000, False, torch.bfloat16), (80, 1000, True, torch.bfloat16), (80, 1000, True, torch.float32)])
def test_geometry(flavour, shift, k_cls, topk, pad, dtype):
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, k_cls, dtype, pad, 7 + k_cls + topk, shift)
    rw = (1.0, 1.0, 1.0, 1.0) if k_cls == 80 else (2.0, 2.0, 1.5, 1.5)
    got, _ = run(LEVELS, 2, k_cls, topk, THRESH, rw, logits, deltas, anchors)
    ref = reference(LEVELS, 2, k_cls, topk, logit_thresh(), rw, logits, deltas, anchors)
    if k_cls == 80:
        c0 = int(ref["counts"][0, 0])
        passing = int((logits[0][0, :, :, :A * 80].float() > logit_thresh()).sum())
        assert {"sparse": passing < 1000, "mid": 1000 < passing <= MIN_SURVIVORS, "dense": passing > MIN_SURVIVORS}[flavour], passing
        assert c0 == min(passing, topk)
    assert int(ref["counts"][0, 2]) < topk or topk == 8  # the 2 x 1 level: fewer pass than topk = 1000
    assert got["cap"] == 3 * topk
    compare(got, ref)


def test_all_pass_overflows_the_list_and_is_filtered_again():
    """Every logit above the threshold: 8*8*9*80 = 46 080 candidates > the list's 4096 > topk."""
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, 80, torch.float16, False, 3, 2.0)
    logits = [z.clamp(min=-2.0) for z in logits]
    got, _ = run(LEVELS, 2, 80, 1000, THRESH, (1.0,) * 4, logits, deltas, anchors)
    ref = reference(LEVELS, 2, 80, 1000, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    assert ref["counts"].tolist() == [[1000, 1000, 1000]] * 2  # (even the 2 x 1 level has 1440 elements)
    compare(got, ref)


def test_none_pass():
    ops = _ops()
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, 80, torch.float16, True, 4, -20.0)
    got, _ = run(LEVELS, 2, 80, 1000, THRESH, (1.0,) * 4, logits, deltas, anchors)
    assert int(got["counts"].abs().sum()) == 0 and int(got["c_cand"].abs().sum()) == 0
    assert bool((got["c_cls"] == -1).all()) and bool((got["c_src"] == -1).all())
    assert float(got["c_boxes"].abs().sum()) == 0.0 and float(got["c_scores"].abs().sum()) == 0.0
    cap = got["cap"]
    seg = torch.full((2,), cap, dtype=torch.int32, device=DEV)
    _, cnt = ops.nms_topk(got["c_boxes"], got["c_scores"], got["c_cls"], got["c_cand"], 2, cap, seg, 0.5, 100)
    assert cnt.tolist() == [0, 0]


def test_equal_logits_overflow_twice_and_take_the_pass_over_the_logits():
    """46 080 equal logits above the threshold: the raised threshold keeps them all, the list overflows again, and the one-workgroup pass
    over the logits themselves must pick the 1000 lowest indices, in order."""
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, 80, torch.bfloat16, True, 12, 0.0)
    for z in logits:
        z[..., :A * 80] = 0.75
    logits[0][1, 3, 3, 100] = 1.0  # one larger value: it comes first, the equal ones follow from index 0
    got, _ = run(LEVELS, 2, 80, 1000, THRESH, (1.0,) * 4, logits, deltas, anchors)
    ref = reference(LEVELS, 2, 80, 1000, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    assert ref["c_src"][0, :1000].tolist() == list(range(1000)) and ref["c_src"][1, :3].tolist() == [(3 * 8 + 3) * 720 + 100, 0, 1]
    compare(got, ref)


@pytest.mark.parametrize("k_cls", [3, 80])  # 1728 elements: the list holds them all; 46 080: it overflows, ties straddle the new threshold too
def test_ties_lower_index_first_and_repeatable(k_cls):
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, k_cls, torch.float16, True, 5, 0.0)
    g = torch.Generator().manual_seed(11)
    values = torch.linspace(-1.0, 2.75, 16).to(torch.float16)
    for z in logits:
        z[..., :A * k_cls] = values[torch.randint(0, 16, z[..., :A * k_cls].shape, generator=g)]
    ref = reference(LEVELS, 2, k_cls, 200, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    s = ref["c_scores"][0, :200]
    assert s[199] == s[198] or s[199] == s[197]  # the k-th place lies inside a run of equal logits
    got, _ = run(LEVELS, 2, k_cls, 200, THRESH, (1.0,) * 4, logits, deltas, anchors)
    compare(got, ref)
    again, _ = run(LEVELS, 2, k_cls, 200, THRESH, (1.0,) * 4, logits, deltas, anchors)
    for key in ("c_boxes", "c_scores", "c_cls", "c_cand", "c_src", "counts"):
        assert torch.equal(got[key].view(torch.int32), again[key].view(torch.int32)), key


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_segment_split_over_many_workgroups(dtype):
    levels = [(64, 64, 8), (3, 5, 16)]
    seg_bytes = 64 * 64 * A * 8 * torch.finfo(dtype).bits // 8
    assert seg_bytes > 8 * CHUNK_BYTES  # the filter splits this segment over more than eight workgroups
    anchors = cell_anchors(levels)
    logits, deltas = make_case(levels, 2, 8, dtype, True, 6, -5.2)  # about 1.2 %: ~3500 survivors, list capacity 9217
    report = {}
    got, _ = run(levels, 2, 8, 1000, THRESH, (1.0,) * 4, logits, deltas, anchors)
    ref = reference(levels, 2, 8, 1000, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    passing = int((logits[0][0, :, :, :A * 8].float() > logit_thresh()).sum())
    assert 1000 < passing <= 64 * 64 * A * 8 // 32
    compare(got, ref, report)


def test_hostile_values():
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, 3, torch.float32, False, 8, -1.0)
    z0 = logits[0]
    z0[0, 1, 2, 5] = float("nan")
    z0[0, 3, 3, 7] = -float("nan")
    z0[0, 2, 2, 4] = float("inf")       # cell 18, a = 1, k = 1
    z0[1, 0, 0, 0] = 9.0                # image 1's best: cell 0, a = 0
    deltas[0][1, 0, 0, 2] = float("nan")
    z0[1, 7, 7, 26] = 8.0               # image 1's second: cell 63, a = 8
    deltas[0][1, 7, 7, 32 + 2] = 10.0   # dw = 10: clamped at log(1000 / 16)
    deltas[0][1, 7, 7, 32 + 3] = -1.0
    got, _ = run(LEVELS, 2, 3, 1000, THRESH, (1.0,) * 4, logits, deltas, anchors)
    ref = reference(LEVELS, 2, 3, 1000, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    assert ref["flag"] == 1
    src0 = got["c_src"][0].cpu()
    nan_idx = [(1 * 8 + 2) * 27 + 5, (3 * 8 + 3) * 27 + 7]
    assert not any(int(i) in nan_idx for i in src0[:int(got["counts"][0, 0])])
    assert int(src0[0]) == (2 * 8 + 2) * 27 + 4 and float(got["c_scores"][0, 0]) == 1.0 and int(got["c_cls"][0, 0]) == 1
    assert int(got["c_src"][1, 0]) == 0 and int(got["c_cand"][1, 0]) == 0 and int(got["status_flags"].item()) & 1 == 1
    assert int(got["c_src"][1, 1]) == 63 * 27 + 26 and int(got["c_cand"][1, 1]) == 1
    a = anchors[0][8]
    width = float(got["c_boxes"][1, 1, 2] - got["c_boxes"][1, 1, 0])
    assert abs(width - math.exp(CLAMP) * float(a[2] - a[0])) <= 1e-3 * width
    # (the bound of compare() assumes |dw| <= 1.5; the clamped row is compared with it too: exp(4.135) * aw stays below 4096)
    compare(got, ref)


def _sentinel_out(n, cap, nl):
    return dict(c_boxes=torch.full((n, cap, 4), -7.0, device=DEV), c_scores=torch.full((n, cap), -7.0, device=DEV),
                c_cls=torch.full((n, cap), -7, dtype=torch.int32, device=DEV), c_cand=torch.full((n, cap), -7, dtype=torch.int32, device=DEV),
                c_src=torch.full((n, cap), -7, dtype=torch.int32, device=DEV), counts=torch.full((n, nl), -7, dtype=torch.int32, device=DEV),
                status_flags=torch.full((1,), -7, dtype=torch.int32, device=DEV))


def _untouched(out):
    torch.cuda.synchronize()
    return all(bool((v == -7).all()) for v in out.values())


def test_refusals_write_nothing():
    ops = _ops()
    anchors = cell_anchors(LEVELS)
    logits, deltas = make_case(LEVELS, 2, 3, torch.float16, False, 9, 0.0)
    lv = ops.make_rpn_levels([(h, w) for h, w, _ in LEVELS], [s for _, _, s in LEVELS], 2, A)
    lg = torch.cat([x.reshape(-1) for x in logits]).to(DEV)
    dl = torch.cat([x.reshape(-1) for x in deltas]).to(DEV)
    out = _sentinel_out(2, 3 * 4096, 3)
    with pytest.raises(ops.OsrError, match="topk"):
        ops.retinanet_select(lv, anchors.to(DEV), lg, dl, 2, 3, 4096, THRESH, out=out)
    assert _untouched(out)
    out = _sentinel_out(2, 3 * 8, 3)
    with pytest.raises(ops.OsrError, match="pitch"):
        ops.retinanet_select(lv, anchors.to(DEV), lg, dl, 2, 3, 8, THRESH, pitch_cls=A * 3 - 1, out=out)
    assert _untouched(out)
    with pytest.raises(ops.OsrError, match="pitch"):
        ops.retinanet_select(lv, anchors.to(DEV), lg, dl, 2, 3, 8, THRESH, pitch_box=4 * A - 4, out=out)
    assert _untouched(out)
    with pytest.raises(ops.OsrError, match="GPU"):
        ops.retinanet_select(lv, anchors.to(DEV), lg.cpu(), dl, 2, 3, 8, THRESH, out=out)
    assert _untouched(out)
    with pytest.raises(ops.OsrError, match="aligned"):
        ops.retinanet_select(lv, anchors.to(DEV), torch.cat([lg[:1], lg])[1:], dl, 2, 3, 8, THRESH, out=out)
    assert _untouched(out)
    # and the accepted call on the same buffers overwrites every sentinel
    got = ops.retinanet_select(lv, anchors.to(DEV), lg, dl, 2, 3, 8, THRESH, out=out)
    torch.cuda.synchronize()
    assert not any(bool((got[k] == -7).any()) for k in ("c_cls", "c_cand", "c_src", "counts", "status_flags"))
