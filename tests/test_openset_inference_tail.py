"""The Openset second-stage inference tail (csrc/osr_det_tail.hip), kernel by kernel, at its edges and limits: grid-stride second
turns, block-turn carries, LDS limits, non-finite rows, signed zeros, thresholds met exactly, refusals, and the whole chain with
NaN planted wherever "nothing downstream reads".

References are float64 numpy restatements written here (the C oracle for NMS / sort order, the torch oracle for the box decode).
Integers, indices, counts and copied values must match bit for bit; values that come out of an fp32 reduction or expf must be
within 1e-4 of the reference's largest magnitude (the contract in the header of tests/test_hip_ops.py); the decoded boxes are
recomputed from the kernel's own deltas under rtol 1e-5 / atol 1e-3 as test_box_predictor_tail does. A row whose decision may
legitimately flip (score within 1e-6 of the threshold; two class distances within 1e-5 of each other or of unk_thr) is left out
of the exact comparison; each case asserts, from the reference alone, that fewer than 1 % of its rows are.

Measured on an MI355X (largest error of each quantity over all cases of its tests, relative to the reference's largest magnitude;
the bound is 1e-4 on every line; `pytest -s` prints each figure):
  box tail pred_deltas 5.1e-08   pred_iou 9.6e-08   score 1.1e-07      l2norm (row by row)      1.0e-07
  pln_tail min_dist    5.7e-07                                         softmax k_scores         4.1e-07
Rows left out of an exact comparison: 1 of 4400 (softmax candidates, K = 20, one probability within 1e-6 of known_thresh), 0 elsewhere.
The 70 cases take about 3 s together.

Two faults of osr_l2_normalize_rows surfaced here and are fixed in the kernel file: a row of 1e18 at d = 1000 came out as zeros (its
sum of squares is 1e39, past fp32's range), and rows = 0 was refused (an empty tensor's null pointers were checked before the count).
"""
import math

import numpy as np
import pytest
import torch

from oracle import c_binding as CO
from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64
NAN, INF = float("nan"), float("inf")
REL = 1e-4          # fp32 reductions / expf: relative to the reference's largest magnitude
SCALE_CLAMP = f64(f32(math.log(1000.0 / 16)))
INVALID_ARG, UNSUPPORTED = "status -1", "status -2"


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_close(name, got, ref, floor=1e-6):
    """Largest |got - ref| over the finite reference entries <= 1e-4 * largest |ref| (at least `floor`); NaN / Inf entries must agree
    in kind and sign."""
    got, ref = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64)
    assert got.shape == ref.shape, name
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{name}: NaN entries differ"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{name}: Inf entries differ"
    err = 0.0
    if fin.any():
        err = float(np.abs(got[fin] - ref[fin]).max() / max(float(np.abs(ref[fin]).max()), floor))
    print(f"[err] {name}: {err:.3e} of the largest magnitude (bound {REL:.0e})")
    assert err <= REL, f"{name}: {err:.3e} > {REL:.0e}"
    return err


def few(name, flagged, rows):
    """Rows left out of an exact comparison: fewer than 1 % of the case's rows (counted on the reference alone)."""
    k = int(flagged) if np.isscalar(flagged) else int(np.count_nonzero(flagged))
    print(f"[left out] {name}: {k} of {rows} rows (cap {rows / 100:.2f})")
    assert k * 100 < rows, f"{name}: {k} of {rows} rows are within rounding of a decision"


# ======================================================================================================================
# 1. osr_box_predictor_tail
# ======================================================================================================================
HW = np.array([[800, 1333], [640, 1000]], dtype=i32)


def box_case(seed, m, k, bidx):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((m, k)), 0).astype(f32)
    w = (rng.standard_normal((5, k)) / math.sqrt(k)).astype(f32)
    b = (rng.standard_normal(5) * 0.1).astype(f32)
    xy = rng.uniform(0, 1, (m, 2)) * np.array([1200.0, 700.0])
    props = np.concatenate((xy, xy + rng.uniform(1, 300, (m, 2))), 1).astype(f32)
    ctr = (rng.uniform(0, 1, m) ** 2).astype(f32)
    return dict(x=x, w=w, b=b, props=props, ctr=ctr, bidx=np.asarray(bidx, dtype=i32))


def box_tail_ref(c, rw, mean_type, thr):
    """float64 restatement of the kernel's contract. cand = isfinite(decoded box) & isfinite(score) & score > thr."""
    with np.errstate(all="ignore"):
        lin = c["x"].astype(f64) @ c["w"].astype(f64).T + c["b"].astype(f64)
        d, iou = lin[:, :4].copy(), 1.0 / (1.0 + np.exp(-lin[:, 4]))
        p, ctr = c["props"].astype(f64), c["ctr"].astype(f64)
        pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        cx, cy = p[:, 0] + 0.5 * pw, p[:, 1] + 0.5 * ph
        dw, dh = d[:, 2] / rw[2], d[:, 3] / rw[3]
        dw, dh = np.where(dw > SCALE_CLAMP, SCALE_CLAMP, dw), np.where(dh > SCALE_CLAMP, SCALE_CLAMP, dh)  # NaN stays NaN
        pcx, pcy = d[:, 0] / rw[0] * pw + cx, d[:, 1] / rw[1] * ph + cy
        qw, qh = np.exp(dw) * pw, np.exp(dh) * ph
        box = np.stack((pcx - 0.5 * qw, pcy - 0.5 * qh, pcx + 0.5 * qw, pcy + 0.5 * qh), 1)
        score = np.sqrt(iou * ctr) if mean_type == 0 else (iou + ctr) / 2.0
        thr64 = f64(f32(thr))
        valid = np.isfinite(box).all(1) & np.isfinite(score)
        cand = valid & (score > thr64)
        near = valid & (np.abs(score - thr64) < 1e-6)
    pad = c["bidx"] < 0
    d[pad], iou[pad], score[pad], cand[pad], near[pad] = 0.0, 0.0, 0.0, False, False
    return dict(deltas=d, iou=iou, score=score, cand=cand.astype(i32), near=near, pad=pad)


def run_box_tail(ops, c, rw=(10.0, 10.0, 5.0, 5.0), mean_type=0, thr=0.05):
    r = ops.box_predictor_tail(dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["props"]), dev(c["ctr"]), dev(c["bidx"]), dev(HW), rw, mean_type, thr)
    return {k: host(v) for k, v in r.items()}


def check_box_tail(name, c, r, ref, rw, exact_cand=False):
    check_close(name + " pred_deltas", r["pred_deltas"], ref["deltas"])
    check_close(name + " pred_iou", r["pred_iou"], ref["iou"])
    check_close(name + " score", r["score"], ref["score"])
    # the decode, recomputed from the kernel's own deltas (identical inputs: tight tolerance), on the rows where it is finite
    dk, props = torch.from_numpy(r["pred_deltas"]), torch.from_numpy(c["props"])
    fin = np.isfinite(r["pred_deltas"]).all(1) & np.isfinite(c["props"]).all(1) & ~ref["pad"]
    dec = O.b2b_apply_deltas(dk, props, rw)
    for i in range(len(HW)):
        sel = torch.from_numpy(fin & (c["bidx"] == i))
        want, got = O.box_clip(dec[sel], tuple(HW[i].tolist())), torch.from_numpy(r["boxes"])[sel]
        bad = (got - want).abs() > 1e-3 + 1e-5 * want.abs()
        assert not bool(bad.any()), f"{name} boxes of image {i}: {int(bad.sum())} mismatches, max {float((got - want).abs().max()):.3e}"
    if exact_cand:
        assert not ref["near"].any(), name
    few(name + " cand", ref["near"], len(ref["cand"]))
    keep = ~ref["near"]
    assert np.array_equal(r["cand"][keep], ref["cand"][keep]), f"{name}: cand differs"
    pad = ref["pad"]
    for key in ("pred_deltas", "pred_iou", "boxes", "score"):  # rows of no image: exactly zero
        assert same_bits(r[key][pad], np.zeros_like(r[key][pad])), f"{name}: {key} of a batch_idx < 0 row is not +0"


@pytest.mark.parametrize("k", [4, 64, 260, 1024, 3072])
@pytest.mark.parametrize("rw", [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0)])
@pytest.mark.parametrize("mean_type", [0, 1])
def test_box_tail_mean_type_reg_weights_k(ops, mean_type, rw, k):
    """k below one wave's 256-float step, not a multiple of it, and at the 3072 limit of the LDS weight table; both means; two sets
    of regression weights; 37 rows over two images of different sizes."""
    c = box_case(100 + k + mean_type, 37, k, [0] * 20 + [1] * 17)
    ref = box_tail_ref(c, rw, mean_type, 0.3)
    assert 0 < int(ref["cand"].sum()) < 37
    other = box_tail_ref(c, rw, 1 - mean_type, 0.3)
    assert float(np.abs(ref["score"] - other["score"]).max()) > 0.05 and not np.array_equal(ref["cand"], other["cand"])  # the means differ
    check_box_tail(f"box_tail(mean {mean_type}, rw {rw[0]:g}, k {k})", c, run_box_tail(ops, c, rw, mean_type, 0.3), ref, rw)


def test_box_tail_grid_stride_second_turn(ops):
    """4096 blocks of 4 waves take 16384 rows in one turn: rows 16384 .. 16388 are a second turn of the grid-stride loop. The outputs
    come from torch.empty, so a skipped row would show as whatever the memory held."""
    m = 16384 + 5
    rng = np.random.default_rng(7)
    c = box_case(7, m, 64, rng.integers(0, 2, m))
    ref = box_tail_ref(c, (10.0, 10.0, 5.0, 5.0), 0, 0.3)
    r = run_box_tail(ops, c, thr=0.3)
    check_box_tail("box_tail(16389 rows)", c, r, ref, (10.0, 10.0, 5.0, 5.0))
    tail = {k: v[-5:] for k, v in c.items() if k not in ("w", "b")}
    tail.update(w=c["w"], b=c["b"])
    check_box_tail("box_tail(last 5 of 16389 rows)", tail, {k: v[-5:] for k, v in r.items()}, {k: v[-5:] for k, v in ref.items()},
                   (10.0, 10.0, 5.0, 5.0))
    assert 0 < int(ref["cand"][-5:].sum()) + int(ref["cand"][:5].sum()) and int(ref["cand"].sum()) < m


@pytest.mark.parametrize("mean_type", [0, 1])
def test_box_tail_edge_rows(ops, mean_type):
    k = 64
    c = box_case(11, 12, k, [0, 0, 0, 0, 0, 1, 1, 1, 1, -1, -1, -1])
    x, w, props, ctr = c["x"], c["w"], c["props"], c["ctr"]
    x[:, 0] = 0.0
    w[2, 0] = 100.0             # (only row 3 has a feature there)
    ctr[:] = np.clip(ctr, 0.2, None)
    x[1, 5] = NAN               # row 1: NaN feature -> every output NaN, no candidate
    x[2, 5] = INF               # row 2: +Inf feature -> infinite deltas, iou exactly 0 or 1, box not finite, no candidate
    x[3, 0] = 1.0               # row 3: dw = (100 + ...) / 5 is far past log(1000 / 16): clamped, finite box, a candidate
    props[4, 2] = props[4, 0]   # row 4: zero-width proposal: a zero-width box, still a candidate (emptiness is decided later)
    ctr[5] = -0.3               # row 5: geometric mean sqrt(negative) = NaN: no candidate; arithmetic: finite
    ctr[6] = NAN                # row 6: NaN score
    ctr[7] = 0.0                # row 7: geometric 0 (not > thr); arithmetic iou / 2
    x[9:], props[9:], ctr[9:] = NAN, NAN, NAN  # rows of no image: exactly zero outputs whatever their inputs hold
    rw, thr = (10.0, 10.0, 5.0, 5.0), 0.1
    ref = box_tail_ref(c, rw, mean_type, thr)
    r = run_box_tail(ops, c, rw, mean_type, thr)
    check_box_tail(f"box_tail(edge rows, mean {mean_type})", c, r, ref, rw, exact_cand=True)
    assert ref["deltas"][3, 2] / 5.0 > SCALE_CLAMP and np.isfinite(r["boxes"][3]).all()
    want = {0: [1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0]}.get(mean_type)
    if want is not None:
        assert ref["cand"].tolist() == want  # (what the rows above were built to give)
    assert r["cand"].tolist() == ref["cand"].tolist()
    assert ref["cand"][[1, 2, 6, 9, 10, 11]].sum() == 0 and ref["cand"][3] == 1 and ref["cand"][4] == 1
    assert np.isnan(r["score"][6]) and (mean_type == 1 or np.isnan(r["score"][5]))
    assert r["pred_iou"][2] in (0.0, 1.0)


@pytest.mark.parametrize("mean_type", [0, 1])
def test_box_tail_threshold_met_exactly(ops, mean_type):
    """With the IoU weight row zero and b[4] = 0 the kernel's iou is exactly 0.5, so ctr and score_thresh can be chosen for the fp32
    score to EQUAL the threshold (strict >: no candidate) and to be the next float above it (a candidate)."""
    c = box_case(13, 2, 4, [0, 1])
    c["w"][4], c["b"][4] = 0.0, 0.0
    half, two = f32(0.5), f32(2.0)
    if mean_type == 0:   # sqrt(0.5 * 0.5) = 0.5; sqrt(0.25 + 2^-24) rounds to 0.5 + 2^-24, the float after 0.5
        thr, ctr = f32(0.5), np.array([0.5, 0.5 + 2.0 ** -23], dtype=f32)
        score = np.sqrt(half * ctr)
    else:                # (0.5 + 0.25) / 2 = 0.375; 0.5 + (0.25 + 2^-24) is exact and its half is the float after 0.375
        thr, ctr = f32(0.375), np.array([0.25, 0.25 + 2.0 ** -24], dtype=f32)
        score = (half + ctr) / two
    assert score.dtype == f32 and ctr[1] == np.nextafter(np.nextafter(ctr[0], f32(1)), f32(1))
    assert score[0] == thr and score[1] == np.nextafter(thr, f32(1))
    if mean_type == 1:   # one float above 0.25 is not enough: the sum rounds back to 0.75
        assert (half + np.nextafter(ctr[0], f32(1))) / two == thr
    c["ctr"] = ctr
    r = run_box_tail(ops, c, mean_type=mean_type, thr=float(thr))
    assert same_bits(r["pred_iou"], np.array([0.5, 0.5], dtype=f32))
    assert same_bits(r["score"], score)
    assert r["cand"].tolist() == [0, 1]


def test_box_tail_refusals(ops):
    for k, mean_type, status in ((6, 0, UNSUPPORTED), (3076, 0, UNSUPPORTED), (64, 2, INVALID_ARG)):
        c = box_case(1, 3, k, [0, 0, 1])
        with pytest.raises(ops.OsrError, match=status):
            run_box_tail(ops, c, mean_type=mean_type)


# ======================================================================================================================
# 2. osr_nms_topk
# ======================================================================================================================
def nms_inputs(seed, nseg, stride, ncls, extent=300.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, extent, (nseg, stride, 2)).astype(f32)
    boxes = np.concatenate((xy, xy + rng.uniform(10, 120, (nseg, stride, 2)).astype(f32)), 2)
    scores = np.round(rng.uniform(0, 1, (nseg, stride)), 3).astype(f32)  # exact ties
    cls = rng.integers(0, ncls, (nseg, stride)).astype(i32)
    cand = (rng.uniform(0, 1, (nseg, stride)) > 0.2).astype(i32)
    return boxes, scores, cls, cand


def check_nms(ops, boxes, scores, cls, cand, lens, thr, topk):
    nseg, stride = scores.shape
    keep, cnt = ops.nms_topk(dev(boxes), dev(scores), None if cls is None else dev(cls), None if cand is None else dev(cand), nseg, stride,
                             dev(np.asarray(lens, dtype=i32)), thr, topk)
    keep, cnt = host(keep), host(cnt)
    for s in range(nseg):
        n = min(max(int(lens[s]), 0), stride)
        ids = np.arange(n) if cand is None else np.nonzero(cand[s, :n])[0]
        if len(ids) == 0:
            k = ids
        elif thr >= 1.0:
            k = ids[CO.argsort_desc(scores[s, ids])][:topk]
        else:
            cl = np.zeros(len(ids), dtype=i64) if cls is None else cls[s, ids].astype(i64)
            k = ids[CO.batched_nms(boxes[s, ids], scores[s, ids], cl, thr)][:topk]
        assert cnt[s] == len(k), f"segment {s}: kept {cnt[s]} vs {len(k)}"
        assert keep[s, : cnt[s]].tolist() == k.tolist(), f"segment {s}: kept index list differs"
        assert (keep[s, cnt[s]:] == -1).all(), f"segment {s}: padding is not -1"
    return keep, cnt


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_nms_signed_zero_infinite_scores_and_segment_edges(ops, thr):
    """Scores that mix -0.0 / +0.0 (equal: the lower index first), negative and +-Inf scores; seg_len above the stride (read as the
    stride) and negative (read as 0); a segment with no candidate at all."""
    stride, topk = 64, 20
    boxes, scores, cls, cand = nms_inputs(21, 5, stride, 3)
    rng = np.random.default_rng(22)
    pool = np.array([-0.0, 0.0, 0.5, -0.5, 0.25, INF, -INF, -2.0], dtype=f32)
    scores[0] = pool[rng.integers(0, len(pool), stride)]
    scores[3] = np.where(np.arange(stride) % 2 == 0, f32(-0.0), f32(0.0))
    scores[4] = pool[rng.integers(0, 2, stride)]
    cand[2], cand[3], cand[4] = 0, 1, 1
    boxes[3] = boxes[3, :1] + np.arange(stride, dtype=f32)[:, None] * 200.0  # far apart: nothing is suppressed
    boxes[4] = boxes[3]
    assert np.signbit(scores[0]).any() and (scores[0] == 0).sum() > 4 and np.isinf(scores[0]).sum() > 4
    keep, cnt = check_nms(ops, boxes, scores, cls, cand, [stride + 7, -3, stride, 40, stride], thr, topk)
    assert cnt.tolist()[1:] == [0, 0, topk, topk]
    assert keep[3].tolist() == list(range(topk)) and keep[4].tolist() == list(range(topk))  # all scores equal as fp32 values


@pytest.mark.parametrize("thr", [1.0, 0.5])
@pytest.mark.parametrize("stride", [8192, 8193])
def test_nms_sort_lds_global_switch(ops, stride, thr):
    """A padded length of 8192 sorts in LDS, 8193 pads to 16384 and sorts in global memory; the second segment of the 8193 case is
    short enough to sort in LDS inside the same launch."""
    boxes, scores, cls, cand = nms_inputs(stride, 2, stride, 4, extent=4000.0)
    check_nms(ops, boxes, scores, cls, cand, [stride, 5000], thr, 64)


def test_nms_pure_sort_topk_above_nms_table(ops):
    """thr >= 1 never touches the 2048-entry kept table: any topk."""
    boxes, scores, _, cand = nms_inputs(23, 2, 4000, 1)
    _, cnt = check_nms(ops, boxes, scores, None, cand, [4000, 2500], 1.0, 3000)
    assert cnt[0] == 3000 and 0 < cnt[1] < 2500


# ======================================================================================================================
# 3. osr_gather_rows, osr_l2_normalize_rows
# ======================================================================================================================
@pytest.mark.parametrize("row_elems", [1, 4, 6, 1024, 1030])
def test_gather_rows_row_sizes(ops, row_elems):
    """float4 path (row_elems % 4 == 0) and scalar path; counts {topk, 1, 0}; a -1 index inside a count; rows past a count are zero."""
    nseg, stride, topk = 3, 9, 5
    rng = np.random.default_rng(31 + row_elems)
    src = rng.standard_normal((nseg * stride, row_elems)).astype(f32)
    src[3, 0] = -0.0
    keep = np.array([[3, -1, 8, 0, 3], [7, 2, 2, 2, 2], [1, 1, 1, 1, 1]], dtype=i32)
    cnt = np.array([topk, 1, 0], dtype=i32)
    out = host(ops.gather_rows(dev(src[:, 0] if row_elems == 1 else src), stride, dev(keep), dev(cnt)))
    assert out.shape == (nseg, topk, row_elems)
    want = np.zeros((nseg, topk, row_elems), dtype=f32)
    for s in range(nseg):
        for j in range(cnt[s]):
            if keep[s, j] >= 0:
                want[s, j] = src[s * stride + keep[s, j]]
    assert same_bits(out, want)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 256, 1000])
def test_l2_normalize_rows_widths_and_magnitudes(ops, d):
    rng = np.random.default_rng(41 + d)
    x = rng.standard_normal((7, d)).astype(f32)
    x[1] = 0.0          # zero row: 0 / 1e-12
    x[2] = 1e-20        # norm below the 1e-12 floor: divided by the floor
    x[3] = 1e18         # the sum of squares reaches 1e39 at d = 1000: past fp32's range
    x[4] *= 1e-3
    x[5] *= 100.0
    x64 = x.astype(f64)
    ref = x64 / np.maximum(np.sqrt((x64 * x64).sum(1, keepdims=True)), 1e-12)
    assert abs(ref[2, 0] - 1e-8) < 1e-15 and abs(ref[3, 0] - 1 / math.sqrt(d)) < 1e-12
    out = host(ops.l2_normalize_rows(dev(x)))
    for r in range(7):  # row by row, so that the tiny rows are held to their own magnitude
        check_close(f"l2norm(d {d}) row {r}", out[r], ref[r], floor=1e-30)
    assert same_bits(out[1], np.zeros(d, dtype=f32))
    assert host(ops.l2_normalize_rows(torch.empty((0, d), dtype=torch.float32, device=DEV))).shape == (0, d)


# ======================================================================================================================
# 4. osr_pln_tail_ex
# ======================================================================================================================
def unit_rows(a):
    a = a.astype(f64)
    return (a / np.sqrt((a * a).sum(1, keepdims=True))).astype(f32)


def pln_ref(emb, protos, num_known, reps, distance, thr, unknown_id, class_map=None, rows_valid=None, seg_rows=0):
    rows = emb.shape[0]
    valid = np.ones(rows, dtype=bool)
    if rows_valid is not None:
        valid = (np.arange(rows) % seg_rows) < np.repeat(np.asarray(rows_valid), seg_rows)
    e = np.where(valid[:, None], emb, 0).astype(f64)
    eh = e / np.maximum(np.sqrt((e * e).sum(1, keepdims=True)), 1e-12)
    p = protos.astype(f64)
    if distance == "COS":
        dist = 1.0 - eh @ p.T
    elif distance == "L1":
        dist = np.abs(eh[:, None, :] - p[None]).sum(2)
    else:
        dist = np.sqrt(((eh[:, None, :] - p[None]) ** 2).sum(2))
    md = dist.reshape(rows, num_known, reps).min(2)
    best, arg = md.min(1), md.argmin(1)  # argmin: the first (lowest) class among equals
    thr64 = f64(f32(thr))
    cls = (arg if class_map is None else np.asarray(class_map)[arg]).astype(i64)
    cls = np.where(best > thr64, i64(unknown_id), cls)
    amb = np.abs(best - thr64) < 1e-5
    if num_known > 1:
        two = np.sort(md, 1)[:, :2]
        amb |= (two[:, 1] - two[:, 0]) < 1e-5
    cls[~valid], best[~valid], amb[~valid] = -1, 0.0, False
    return cls, best, amb, valid


def pln_embeddings(rng, protos, rows, d, lo=0.005, hi=0.15):
    """Rows that sit at growing distances from a prototype each, so that both sides of any threshold are populated."""
    pick = rng.integers(0, protos.shape[0], rows)
    return (protos[pick] * 1.7 + rng.standard_normal((rows, d)) * np.linspace(lo, hi, rows)[:, None]).astype(f32)


def check_pln(name, ops, emb, protos, num_known, reps, distance, thr, unknown_id, class_map=None, rows_valid=None, seg_rows=0):
    cls, best, amb, valid = pln_ref(emb, protos, num_known, reps, distance, thr, unknown_id, class_map, rows_valid, seg_rows)
    few(name + " class", amb, len(cls))
    pc, md = ops.pln_tail(dev(emb), dev(protos), num_known, reps, float(f32(thr)), unknown_id, None if class_map is None else dev(class_map),
                          None if rows_valid is None else dev(np.asarray(rows_valid, dtype=i32)), seg_rows, distance=distance)
    pc, md = host(pc), host(md)
    check_close(name + " min_dist", md, best)
    assert np.array_equal(pc[~amb], cls[~amb]), f"{name}: {int((pc[~amb] != cls[~amb]).sum())} classes differ"
    assert same_bits(md[~valid], np.zeros(int((~valid).sum()), dtype=f32))
    return pc, md, cls, best


@pytest.mark.parametrize("d", [100, 256])
@pytest.mark.parametrize("distance", ["COS", "L1", "L2"])
@pytest.mark.parametrize("reps", [1, 3])
def test_pln_tail_engine_combination(ops, reps, distance, d):
    """rows_valid + reps + distance + class_map at once, as the engine passes them; d = 100 is no multiple of the wave's 64-float
    step; the rows past each image's count hold NaN and must come out as (-1, 0)."""
    num_known, seg_rows, rows_valid, unknown_id = 6, 50, [50, 17], 1000
    rng = np.random.default_rng(50 + d + reps)
    protos = unit_rows(rng.standard_normal((num_known * reps, d)))
    emb = pln_embeddings(rng, protos, 2 * seg_rows, d)
    emb[50 + 17:] = NAN
    class_map = (np.arange(num_known) * 3 + 1).astype(i64)
    # the threshold: halfway between the two middle distances of the reference over the rows that exist, so that both decisions occur
    _, best, _, valid = pln_ref(emb, protos, num_known, reps, distance, 0.0, unknown_id, class_map, rows_valid, seg_rows)
    srt = np.sort(best[valid])
    thr = f32((srt[len(srt) // 2 - 1] + srt[len(srt) // 2]) / 2)
    assert srt[len(srt) // 2] - srt[len(srt) // 2 - 1] > 1e-3
    pc, _, cls, _ = check_pln(f"pln_tail({distance}, reps {reps}, d {d})", ops, emb, protos, num_known, reps, distance, thr, unknown_id, class_map,
                              rows_valid, seg_rows)
    assert (cls[valid] == unknown_id).sum() > 10 and (cls[valid] != unknown_id).sum() > 10
    assert set(cls[valid].tolist()) <= set(class_map.tolist()) | {unknown_id}
    assert (pc[~valid] == -1).all() and int((~valid).sum()) == 33


def test_pln_tail_grid_stride_second_turn(ops):
    """2048 blocks of 4 waves take 8192 rows in one turn; rows 8192 .. 8194 are a second turn of the grid-stride loop."""
    rows, d, num_known = 8192 + 3, 64, 3
    rng = np.random.default_rng(61)
    protos = unit_rows(rng.standard_normal((num_known, d)))
    emb = pln_embeddings(rng, protos, rows, d, 0.005, 0.3)
    emb[-3:] = emb[:3]  # the last three compare like the first
    pc, md, cls, best = check_pln("pln_tail(8195 rows)", ops, emb, protos, num_known, 1, "COS", 0.23, 80)
    assert np.array_equal(pc[-3:], pc[:3]) and same_bits(md[-3:], md[:3])
    assert np.array_equal(pc[-3:], cls[-3:]) and (cls == 80).sum() > 100 and (cls != 80).sum() > 100


def test_pln_tail_known_answers(ops):
    """Unit-vector prototypes: every product is exact, so are the distances 0 and 1."""
    d, num_known, reps = 64, 6, 2
    protos = np.zeros((num_known * reps, d), dtype=f32)
    for c in range(num_known):
        protos[c * reps, 2 * c], protos[c * reps + 1, 2 * c + 1] = 1.0, 1.0
    protos[5 * reps] = protos[2 * reps]        # classes 2 and 5 hold the same prototype
    protos[4 * reps + 1] = protos[1 * reps]    # class 4's second prototype is class 1's first
    emb = np.zeros((5, d), dtype=f32)
    emb[0, 4] = 3.0    # = the prototype of classes 2 and 5: distance 0 to both, class 2 wins
    emb[1, 2] = 0.5    # = class 1's first and class 4's second prototype: class 1 wins
    emb[2, 40] = 1.0   # orthogonal to every prototype: COS distance exactly 1.0
    # row 3: the zero embedding: 0 / 1e-12 = 0, distance exactly 1.0 to everything
    emb[4, 9] = 2.0    # class 4's first prototype... is e8; e9 is class 4's second before it was replaced: orthogonal now
    one, below = f32(1.0), np.nextafter(f32(1.0), f32(0.0))
    for thr, want in ((one, [2, 1, 0, 0, 0]), (below, [2, 1, 80, 80, 80])):  # strict >: a distance EQUAL to unk_thr stays known
        pc, md = ops.pln_tail(dev(emb), dev(protos), num_known, reps, float(thr), 80)
        assert host(pc).tolist() == want, (float(thr), host(pc).tolist())
        assert same_bits(host(md), np.array([0.0, 0.0, 1.0, 1.0, 1.0], dtype=f32))
    cm = (np.arange(num_known) * 7 + 100).astype(i64)
    pc, _ = ops.pln_tail(dev(emb), dev(protos), num_known, reps, float(below), 80, class_map=dev(cm))
    assert host(pc).tolist() == [114, 107, 80, 80, 80]


def test_pln_tail_prototype_table_limit_and_refusals(ops, osr):
    """144 x 1 x 256 floats fill the 144 KB LDS table exactly; one prototype more is refused; so are an unknown distance type and a
    rows_valid layout whose rows are not a whole number of segments (its last rows would index rows_valid past its end)."""
    d = 256
    rng = np.random.default_rng(71)
    protos = unit_rows(rng.standard_normal((145, d)))
    emb = pln_embeddings(rng, protos[:144], 8, d, 0.01, 0.08)
    _, _, cls, _ = check_pln("pln_tail(144 prototypes)", ops, emb, protos[:144], 144, 1, "COS", 0.3, 1000)
    assert (cls != 1000).any()
    with pytest.raises(ops.OsrError, match=UNSUPPORTED):
        ops.pln_tail(dev(emb), dev(protos), 145, 1, 0.3, 1000)
    e, p = dev(emb), dev(protos[:6])
    pc, md = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.float32, device=DEV)
    lib = osr._lib.load()
    for dist_type, status in ((3, -1), (-1, -1), (0, 0)):  # (the raw ABI: ops.pln_tail takes the distance by name)
        assert lib.osr_pln_tail_ex(e.data_ptr(), 8, d, p.data_ptr(), 6, 1, dist_type, 0.3, 1000, None, None, 0, pc.data_ptr(), md.data_ptr(),
                                   None) == status
    torch.cuda.synchronize()
    rv = dev(np.array([4, 2], dtype=i32))
    for rows, seg_rows in ((7, 4), (5, 4), (8, 3)):
        with pytest.raises(ops.OsrError, match=INVALID_ARG):
            ops.pln_tail(e[:rows].contiguous(), p, 6, 1, 0.3, 1000, rows_valid=rv, seg_rows=seg_rows)
    pc2, _ = ops.pln_tail(e, p, 6, 1, 0.3, 1000, rows_valid=rv, seg_rows=4)  # whole segments: accepted
    assert (host(pc2)[[4, 5]] != -1).all() and (host(pc2)[[6, 7]] == -1).all()


# ======================================================================================================================
# 5. osr_softmax_candidates
# ======================================================================================================================
UNK = 80
KNOWN_THR, UNKNOWN_THR = 0.05, 0.0


def softmax_case(num_known, seg_rows, counts, seed):
    rng = np.random.default_rng(seed)
    n = len(counts)
    logits = (rng.standard_normal((n, seg_rows, num_known + 1)) * 2.0).astype(f32)
    xy = rng.uniform(0, 1, (n, seg_rows, 2)) * np.array([1000.0, 600.0])
    boxes = np.concatenate((xy, xy + rng.uniform(5, 250, (n, seg_rows, 2))), 2).astype(f32)
    scores = rng.uniform(-0.2, 1.0, (n, seg_rows)).astype(f32)
    pcls = np.where(rng.uniform(0, 1, (n, seg_rows)) > 0.4, rng.integers(0, num_known, (n, seg_rows)), UNK).astype(i64)
    for j0 in (0, 1030):  # planted rows, inside the first and inside the second turn of the 1024-thread block
        if j0 + 8 > seg_rows:
            continue
        for i in range(n):
            pcls[i, j0:j0 + 4], pcls[i, j0 + 4:j0 + 8] = 0, UNK
            logits[i, j0:j0 + 4, 0] = 3.0                    # (each would pass on its class 0 otherwise)
            logits[i, j0, num_known] = NAN                    # a NaN logit: every probability NaN, row dropped
            logits[i, j0 + 1, num_known] = INF                # a +Inf logit: Inf - Inf = NaN, row dropped
            logits[i, j0 + 2, :] = -INF                       # all -Inf: NaN, row dropped
            boxes[i, j0 + 3, 2] = NAN                         # a NaN box coordinate: row dropped
            scores[i, j0 + 4], scores[i, j0 + 5], scores[i, j0 + 6] = NAN, 0.0, -0.0  # none is > 0.0
            boxes[i, j0 + 7, 1] = INF                         # an unknown row with a non-finite box: dropped
            scores[i, j0 + 7] = 0.9
    if seg_rows > 1027:  # one known and one unknown row that pass, just inside the second turn (below every count used here)
        pcls[:, 1025], scores[:, 1025], boxes[:, 1025] = UNK, 0.5, [10.0, 20.0, 30.0, 40.0]
        pcls[:, 1026], logits[:, 1026, 0], boxes[:, 1026] = 0, 3.0, [15.0, 25.0, 35.0, 45.0]
        logits[:, 1026, 1:] = 0.0
    for i, c in enumerate(counts):  # past the count: NaN everywhere, classes of any kind
        c = max(min(c, seg_rows), 0)
        logits[i, c:], boxes[i, c:], scores[i, c:] = NAN, NAN, NAN
        pcls[i, c:] = rng.choice(np.array([UNK, 0, -1, 12345, -(2 ** 40)], dtype=i64), seg_rows - c)
    return dict(logits=logits, boxes=boxes, scores=scores, pcls=pcls, counts=np.asarray(counts, dtype=i32), num_known=num_known, seg_rows=seg_rows)


def softmax_ref(c):
    """Per image, over rows below min(count, seg_rows). Returns per image the known (row, class, p) list in row-major order, the
    unknown row list, and the rows with a probability within 1e-6 of the threshold."""
    K, out = c["num_known"], []
    thr64 = f64(f32(KNOWN_THR))
    for i, cnt in enumerate(c["counts"]):
        cnt = max(min(int(cnt), c["seg_rows"]), 0)
        known, unknown, amb = [], [], set()
        with np.errstate(all="ignore"):
            for j in range(cnt):
                okbox = bool(np.isfinite(c["boxes"][i, j]).all())
                if c["pcls"][i, j] != UNK:
                    lg = c["logits"][i, j].astype(f64)
                    e = np.exp(lg - lg.max())
                    p = e / e.sum()
                    if not (okbox and np.isfinite(p).all()):
                        continue
                    if (np.abs(p[:K] - thr64) < 1e-6).any():
                        amb.add(j)
                    known += [(j, k, p[k]) for k in range(K) if p[k] > thr64]
                else:
                    s = c["scores"][i, j]
                    if okbox and np.isfinite(s) and s > f32(UNKNOWN_THR):
                        unknown.append(j)
        out.append((known, unknown, amb))
    return out


def check_softmax_candidates(name, ops, c):
    n, seg, K = len(c["counts"]), c["seg_rows"], c["num_known"]
    ref = softmax_ref(c)
    few(name, sum(len(a) for _, _, a in ref), n * seg)
    r = ops.softmax_candidates(dev(c["logits"].reshape(-1, K + 1)), K, dev(c["boxes"].reshape(-1, 4)), dev(c["scores"].reshape(-1)),
                               dev(c["pcls"].reshape(-1)), dev(c["counts"]), n, seg, UNK, KNOWN_THR, UNKNOWN_THR)
    r = {k: host(v) for k, v in r.items()}
    errs = []
    for i, (known, unknown, amb) in enumerate(ref):
        kc, uc = int(r["k_count"][i]), int(r["u_count"][i])
        assert 0 <= kc <= seg * K and 0 <= uc <= seg
        det, cls = r["k_det"][i, :kc], r["k_cls"][i, :kc]
        sure = ~np.isin(det, sorted(amb))
        want = [(j, k, p) for j, k, p in known if j not in amb]
        assert list(zip(det[sure].tolist(), cls[sure].tolist())) == [(j, k) for j, k, _ in want], f"{name} image {i}: known (row, class) list"
        if not amb:
            assert kc == len(known)
        assert same_bits(r["k_boxes"][i, :kc], c["boxes"][i, det]), f"{name} image {i}: known boxes are not the input rows"
        if want:
            errs.append((np.abs(r["k_scores"][i, :kc][sure].astype(f64) - np.array([p for _, _, p in want])).max(), max(p for _, _, p in want)))
        assert uc == len(unknown) and r["u_det"][i, :uc].tolist() == unknown, f"{name} image {i}: unknown row list"
        unknown = np.asarray(unknown, dtype=np.intp)
        assert same_bits(r["u_boxes"][i, :uc], c["boxes"][i, unknown]) and same_bits(r["u_scores"][i, :uc], c["scores"][i, unknown])
    err = max(e for e, _ in errs) / max(m for _, m in errs)
    print(f"[err] {name} k_scores: {err:.3e} of the largest magnitude (bound {REL:.0e})")
    assert err <= REL
    return ref, r


@pytest.mark.parametrize("num_known", [1, 20, 64])
def test_softmax_candidates_block_turns_counts_and_planted_rows(ops, num_known):
    """seg_rows = 1100 needs a second turn of the 1024-thread block with the running counts carried over; counts at, below and above
    seg_rows (clamped) and 0; dropped rows planted in both turns; NaN and arbitrary classes past every count."""
    seg = 1100
    c = softmax_case(num_known, seg, [seg, 1030, seg + 9, 0], 80 + num_known)
    ref, r = check_softmax_candidates(f"softmax_candidates(K {num_known})", ops, c)
    for i in (0, 1, 2):  # both lists are fed in both turns, so a dropped carry cannot go unseen
        known, unknown, _ = ref[i]
        assert any(j < 1024 for j, _, _ in known) and any(j >= 1024 for j, _, _ in known)
        assert any(j < 1024 for j in unknown) and any(j >= 1024 for j in unknown)
        planted = set(range(0, 8)) | set(range(1030, 1038))
        assert not planted & {j for j, _, _ in known} and not planted & set(unknown)
    assert len(ref[2][0]) > 0 and max(j for j, _, _ in ref[2][0]) > 1030  # the count above seg_rows reads every row
    assert r["k_count"][3] == 0 and r["u_count"][3] == 0


def test_softmax_candidates_refuses_65_known(ops):
    c = softmax_case(65, 8, [8], 1)
    with pytest.raises(ops.OsrError, match=INVALID_ARG):
        check_softmax_candidates("softmax_candidates(K 65)", ops, c)


# ======================================================================================================================
# 6. osr_assemble_detections, osr_detector_postprocess
# ======================================================================================================================
@pytest.mark.parametrize("mapped", [False, True])
def test_assemble_detections_every_slot(ops, mapped):
    """Hand-built candidate and keep lists (no NMS involved): keep counts above topk are clamped; images with no unknown, no known,
    neither; every output slot is asserted, padding included."""
    n, k_stride, u_stride, k_topk, u_topk, num_known = 4, 12, 7, 5, 3, 6
    rng = np.random.default_rng(91)
    cands = dict(k_boxes=rng.uniform(0, 500, (n, k_stride, 4)).astype(f32), k_scores=rng.uniform(0, 1, (n, k_stride)).astype(f32),
                 k_cls=rng.integers(0, num_known, (n, k_stride)).astype(i32), u_boxes=rng.uniform(0, 500, (n, u_stride, 4)).astype(f32),
                 u_scores=rng.uniform(0, 1, (n, u_stride)).astype(f32))
    k_keep = np.array([[11, 0, 5, 5, 3], [2, 9, 1, -1, -1], [-1] * 5, [-1] * 5], dtype=i32)
    u_keep = np.array([[6, 0, -1], [-1] * 3, [1, 4, 2], [-1] * 3], dtype=i32)
    k_cnt, u_cnt = np.array([7, 3, 0, 0], dtype=i32), np.array([2, 0, 5, 0], dtype=i32)  # 7 > k_topk and 5 > u_topk: clamped
    class_map = (np.arange(num_known) * 5 + 200).astype(i64) if mapped else None
    ob, osc, ocl, on = ops.assemble_detections({k: dev(v) for k, v in cands.items()}, dev(k_keep), dev(k_cnt), dev(u_keep), dev(u_cnt), n, UNK,
                                               None if class_map is None else dev(class_map))
    cap = k_topk + u_topk
    wb, ws, wc = np.zeros((n, cap, 4), dtype=f32), np.zeros((n, cap), dtype=f32), np.full((n, cap), -1, dtype=i64)
    for i in range(n):
        nu, nk = min(u_cnt[i], u_topk), min(k_cnt[i], k_topk)
        for j in range(nu):
            wb[i, j], ws[i, j], wc[i, j] = cands["u_boxes"][i, u_keep[i, j]], cands["u_scores"][i, u_keep[i, j]], UNK
        for j in range(nk):
            q = k_keep[i, j]
            cl = int(cands["k_cls"][i, q])
            wb[i, nu + j], ws[i, nu + j], wc[i, nu + j] = cands["k_boxes"][i, q], cands["k_scores"][i, q], cl if class_map is None else class_map[cl]
    assert host(on).tolist() == [2 + 5, 3, 3, 0]
    assert same_bits(host(ob), wb) and same_bits(host(osc), ws) and np.array_equal(host(ocl), wc)


@pytest.mark.parametrize("cap", [100, 256, 257, 600])
def test_detector_postprocess_block_turns(ops, osr, cap):
    """cap above the block's 256 threads takes several turns with the output position carried over; counts {cap, cap + 5 (clamped),
    1, 0}; a different scale in x and y; boxes that become empty only after the clip in the first and in the last turn."""
    n = 4
    rng = np.random.default_rng(95 + cap)
    xy = rng.uniform(-20, 280, (n, cap, 2))
    boxes = np.concatenate((xy, xy + rng.uniform(1, 80, (n, cap, 2))), 2).astype(f32)
    for i in (0, 1):
        boxes[i, 3] = [330.0, 10.0, 380.0, 30.0]           # right of the clipped width: empty only after the clip (first turn)
        boxes[i, cap - 2] = [10.0, 250.0, 30.0, 290.0]     # below the clipped height (last turn)
        boxes[i, cap // 2, 3] = boxes[i, cap // 2, 1]      # zero height before anything
    boxes[2, 0] = [10.0, 10.0, 50.0, 60.0]                 # the one box of image 2: kept
    scores = rng.uniform(0, 1, (n, cap)).astype(f32)
    classes = rng.integers(0, 21, (n, cap)).astype(i64)
    count = np.array([cap, cap + 5, 1, 0], dtype=i32)
    scale = np.array([[1.5, 0.75], [0.5, 1.25], [2.0, 3.0], [1.0, 1.0]], dtype=f32)
    out_hw = np.array([[180, 480], [300, 160], [700, 600], [240, 320]], dtype=i32)  # (scaled 320 x 240 frames)
    ob, os_, oc, on = [host(t) for t in ops.detector_postprocess(dev(boxes), dev(scores), dev(classes), dev(count), dev(scale), dev(out_hw))]
    for i in range(n):
        c = min(int(count[i]), cap)
        b = boxes[i, :c] * np.array([scale[i, 0], scale[i, 1], scale[i, 0], scale[i, 1]], dtype=f32)
        b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], f32(0)), f32(out_hw[i, 1]))
        b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], f32(0)), f32(out_hw[i, 0]))
        keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        m = int(keep.sum())
        if i < 2:
            assert not keep[3] and not keep[cap - 2] and not keep[cap // 2] and m < c
            raw = boxes[i]
            assert raw[3, 2] > raw[3, 0] and raw[cap - 2, 3] > raw[cap - 2, 1]  # (not empty before the clip)
        assert int(on[i]) == m, f"image {i}: {int(on[i])} vs {m}"
        assert same_bits(ob[i, :m], b[keep]) and same_bits(os_[i, :m], scores[i, :c][keep]) and np.array_equal(oc[i, :m], classes[i, :c][keep])
        assert same_bits(ob[i, m:], np.zeros((cap - m, 4), dtype=f32)) and same_bits(os_[i, m:], np.zeros(cap - m, dtype=f32))
        assert (oc[i, m:] == -1).all()
    assert on[2] == 1 and on[3] == 0
    bd, sd, cd, nd = dev(boxes), dev(scores), dev(classes), dev(count)
    so, co, no = torch.empty_like(sd), torch.empty_like(cd), torch.empty_like(nd)
    xd, hd = dev(scale), dev(out_hw)
    status = osr._lib.load().osr_detector_postprocess(bd.data_ptr(), sd.data_ptr(), cd.data_ptr(), nd.data_ptr(), n, cap, xd.data_ptr(), hd.data_ptr(),
                                                      bd.data_ptr(), so.data_ptr(), co.data_ptr(), no.data_ptr(), None)
    assert status == -1  # in place: refused, nothing launched
    assert same_bits(host(bd), boxes)


# ======================================================================================================================
# 7. the chain, with the padding poisoned
# ======================================================================================================================
def chain_case():
    n, length, k, d, num_known, rec = 2, 64, 64, 32, 5, 64
    counts = [40, 23]
    rng = np.random.default_rng(111)
    protos = unit_rows(rng.standard_normal((num_known, d)))
    x = np.maximum(rng.standard_normal((n * length, k)), 0).astype(f32)
    # the encoder copies the first d features: even rows sit on a prototype (known), odd rows are far from all of them (unknown)
    x[0::2, :d] = protos[rng.integers(0, num_known, n * length // 2)] * 2.0 + rng.standard_normal((n * length // 2, d)).astype(f32) * 0.05
    x[1::2, :d] = rng.standard_normal((n * length // 2, d))
    xy = rng.uniform(0, 1, (n * length, 2)) * np.array([1200.0, 600.0])
    props = np.concatenate((xy, xy + rng.uniform(20, 300, (n * length, 2))), 1).astype(f32)
    ctr = rng.uniform(0.3, 1, n * length).astype(f32)
    bidx = np.repeat(np.arange(n), length).astype(i32)
    pad = np.concatenate([np.arange(length) >= c for c in counts])
    bidx[pad] = -1
    enc_w = np.zeros((d, k), dtype=f32)
    enc_w[np.arange(d), np.arange(d)] = 1.0
    w = dict(pred_w=(rng.standard_normal((5, k)) / math.sqrt(k)).astype(f32), pred_b=(rng.standard_normal(5) * 0.1).astype(f32), enc_w=enc_w,
             enc_b=np.zeros(d, dtype=f32), dec_w=(rng.standard_normal((rec, d)) / math.sqrt(d)).astype(f32), dec_b=np.zeros(rec, dtype=f32),
             cls_w=(rng.standard_normal((num_known + 1, rec)) * 0.5).astype(f32), cls_b=np.zeros(num_known + 1, dtype=f32), protos=protos,
             class_map=(np.arange(num_known) * 2 + 10).astype(i64))
    return dict(n=n, length=length, num_known=num_known, counts=np.asarray(counts, dtype=i32), x=x, props=props, ctr=ctr, bidx=bidx, pad=pad, w=w)


def run_chain(ops, c, fill):
    """The launches of OpensetRCNNEngine._roi_heads after the box head, in its order and with its arguments."""
    n, length, num_known, topk1 = c["n"], c["length"], c["num_known"], 32
    x, props, ctr = c["x"].copy(), c["props"].copy(), c["ctr"].copy()
    x[c["pad"]], props[c["pad"]], ctr[c["pad"]] = fill, fill, fill
    if fill != 0.0:  # the buffers the launches allocate come out of the allocator's cache: leave NaN there for them to pick up
        junk = torch.full((1 << 22,), NAN, dtype=torch.float32, device=DEV)
        del junk
    w = {k: dev(v) for k, v in c["w"].items()}
    box_feats, counts = dev(x), dev(c["counts"])
    pt = ops.box_predictor_tail(box_feats, w["pred_w"], w["pred_b"], dev(props), dev(ctr), dev(c["bidx"]), dev(HW), (10.0, 10.0, 5.0, 5.0), 0, 0.05)
    keep1, cnt1 = ops.nms_topk(pt["boxes"], pt["score"], None, pt["cand"], n, length, counts, 1.0, topk1)
    det_boxes = ops.gather_rows(pt["boxes"], length, keep1, cnt1)
    det_scores = ops.gather_rows(pt["score"], length, keep1, cnt1)
    det_feats = ops.gather_rows(box_feats, length, keep1, cnt1)
    emb = ops.gemm_f32(det_feats.view(n * topk1, -1), w["enc_w"], w["enc_b"])
    rec = ops.gemm_f32(emb, w["dec_w"], w["dec_b"])
    pcls, _ = ops.pln_tail(emb, w["protos"], num_known, 1, 0.4, UNK, w["class_map"], cnt1, topk1, distance="COS")
    logits = ops.gemm_f32(rec, w["cls_w"], w["cls_b"])
    cands = ops.softmax_candidates(logits, num_known, det_boxes.view(-1, 4), det_scores.view(-1), pcls, cnt1, n, topk1, UNK, KNOWN_THR, UNKNOWN_THR)
    kk, kc = ops.nms_topk(cands["k_boxes"], cands["k_scores"], cands["k_cls"], None, n, topk1 * num_known, cands["k_count"], 0.5, 10)
    uk, uc = ops.nms_topk(cands["u_boxes"], cands["u_scores"], None, None, n, topk1, cands["u_count"], 0.5, 10)
    out = ops.assemble_detections(cands, kk, kc, uk, uc, n, UNK, w["class_map"])
    return [host(t) for t in out], host(cnt1)


def test_chain_ignores_what_lies_past_each_count(ops):
    """engine.py promises that nothing downstream of the box head reads past an image's count (its padding tiles stay unwritten):
    the chain's result with NaN in every padding row equals, bit for bit, its result with zeros there, run after run."""
    c = chain_case()
    zero, cnt_z = run_chain(ops, c, 0.0)
    nan1, cnt_1 = run_chain(ops, c, NAN)
    nan2, cnt_2 = run_chain(ops, c, NAN)
    assert cnt_z.tolist() == cnt_1.tolist() == cnt_2.tolist() == [32, 23]
    for other in (nan1, nan2):
        for name, a, b in zip(("boxes", "scores", "classes", "counts"), zero, other):
            same = same_bits(a, b) if a.dtype == f32 else np.array_equal(a, b)
            assert same, f"{name} depend on what lies past an image's count"
    ob, osc, ocl, on = zero
    mapped = set(c["w"]["class_map"].tolist())
    for i in range(c["n"]):
        kept = ocl[i, : on[i]]
        assert (kept == UNK).any() and (kept != UNK).any(), f"image {i} keeps {kept.tolist()}"
        assert set(kept.tolist()) <= mapped | {UNK} and (ocl[i, on[i]:] == -1).all()
        assert np.isfinite(ob[i]).all() and np.isfinite(osc[i]).all()
