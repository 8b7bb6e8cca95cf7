"""osr_fastrcnn_candidates (+ osr_nms_topk), the stock box predictor's inference tail, fed logits and deltas directly and compared
with [d2] fast_rcnn_inference_single_image restated in fp32 torch (oracle.fast_rcnn_inference_from_outputs).

Paths reached: seg_rows 1025 and 2051 exceed the kernel's 1024-thread block, so the exclusive scan carries its running count across
block turns; image 0 yields more than 8192 candidates, so osr_nms_topk sorts that segment in global memory (SORT_LDS_CAP)."""
import numpy as np
import pytest
import torch

from oracle import osr_oracle as O

DEV = "cuda:0"
THR = 0.05
RW = (10.0, 10.0, 5.0, 5.0)


def _probs32(logits):
    return torch.softmax(logits.float(), dim=-1)


def _clear_threshold_band(logits, g):
    """Move every fp32 probability within 1e-5 relative of the threshold out of that band (the device's expf may round the other
    way there), by nudging that row's logits (non-finite logits stay as they are)."""
    for _ in range(20):
        p = _probs32(logits)[:, :-1]
        band = ((p - THR).abs() <= 1e-5 * THR).any(1)
        if not bool(band.any()):
            return logits
        logits[band] += torch.randn(int(band.sum()), logits.shape[1], generator=g) * 0.01
    raise AssertionError("could not clear the threshold band")


def _case(seed, seg_rows, k, agnostic):
    g = torch.Generator().manual_seed(seed)
    n = 3
    image_hw = torch.tensor([[800, 1333], [600, 901], [512, 640]], dtype=torch.int32)
    counts = [seg_rows - 7, 0, seg_rows]
    kbox = 1 if agnostic else k
    # image 0: ~11 classes per row above the threshold -> more than 8192 candidates; elsewhere a few per row
    logits = torch.randn(n, seg_rows, k + 1, generator=g) * 0.5 - 5.0
    hot = torch.rand(n, seg_rows, k, generator=g) < torch.tensor([11.0 / k, 2.0 / k, 2.0 / k]).view(n, 1, 1)
    logits[..., :k] += hot * (8.0 + torch.rand(n, seg_rows, k, generator=g) * 0.5)
    deltas = torch.randn(n, seg_rows, kbox * 4, generator=g) * torch.tensor([1.0, 1.0, 0.3, 0.3]).repeat(kbox)
    xy = torch.rand(n, seg_rows, 2, generator=g) * torch.tensor([1300.0, 780.0])
    wh = 4.0 + torch.rand(n, seg_rows, 2, generator=g) * 300.0
    prop = torch.cat([xy, xy + wh], -1)  # many boxes reach past their image's border: they are clipped
    # rows to be dropped (d2: valid_mask over the whole row), each with a class that would otherwise pass
    L, D = logits[0], deltas[0]
    L[0:8, 1] = 8.0
    L[0, 3] = float("inf")
    L[1, 4] = float("nan")
    L[2, :k] = -6.0
    L[2, 5] = 8.0
    D[2, 4 * (7 if kbox > 1 else 0) + 1] = float("nan")  # class 7's probability is below the threshold
    D[3, 0] = 3.0e38                                       # dx: x1 / x2 overflow to -Inf / +Inf
    # rows to be kept
    L[4, 9] = -float("inf")
    D[5, 2:4] = 100.0                                      # dw, dh above the clamp log(1000 / 16)
    prop[0, 6, 2] = prop[0, 6, 0]                          # zero-width proposal
    prop[0, 7] = torch.tensor([1320.0, 790.0, 1400.0, 850.0])  # past the bottom-right corner of image 0 (800 x 1333)
    prop[2, 3] = torch.tensor([-30.0, -20.0, 40.0, 30.0])  # past the top-left corner
    logits = _clear_threshold_band(logits.view(-1, k + 1), g).view(n, seg_rows, k + 1)
    return n, image_hw, counts, logits, deltas, prop


def _reference(logits, deltas, prop, image_hw, counts, k):
    """Per image: the oracle's candidates, in row-major (row, class) order, before its NMS. Which pairs pass is decided in fp32 as
    d2 decides it; their scores are given in fp64."""
    out = []
    for i, c in enumerate(counts):
        lg, dl, pb = logits[i, :c], deltas[i, :c], prop[i, :c]
        size = tuple(int(v) for v in image_hw[i])
        probs = torch.softmax(lg, dim=-1)
        boxes = O.b2b_apply_deltas_multi(dl, pb, RW)
        valid = torch.isfinite(boxes).all(1) & torch.isfinite(probs).all(1)
        rows = torch.arange(c)[valid]
        probs, boxes = probs[valid, :-1], boxes[valid]
        kb = boxes.shape[1] // 4
        boxes = O.box_clip(boxes.reshape(-1, 4), size).view(-1, kb, 4)
        inds = (probs > THR).nonzero()
        b = boxes[inds[:, 0], inds[:, 1]] if kb > 1 else boxes[inds[:, 0], 0]
        p64 = torch.softmax(lg.double(), dim=-1)[valid, :-1]
        out.append((rows[inds[:, 0]], inds[:, 1], p64[inds[:, 0], inds[:, 1]], b))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seg_rows,k,agnostic", [(1000, 80, False), (1025, 80, True), (1025, 80, False), (2051, 80, False),
                                                 (2051, 128, False), (1025, 128, True)],
                         ids=["1000-K80", "1025-K80-agnostic", "1025-K80", "2051-K80", "2051-K128", "1025-K128-agnostic"])
def test_fastrcnn_candidates_and_nms_match_the_oracle(osr, seg_rows, k, agnostic):
    from openset_rcnn_amd.host import ops
    n, image_hw, counts, logits, deltas, prop = _case(seg_rows + k, seg_rows, k, agnostic)
    cand = ops.fastrcnn_candidates(logits.view(-1, k + 1).to(DEV), deltas.view(n * seg_rows, -1).to(DEV), prop.contiguous().to(DEV),
                                   torch.tensor(counts, dtype=torch.int32, device=DEV), image_hw.to(DEV), k, RW, THR)
    torch.cuda.synchronize()
    ref = _reference(logits, deltas, prop, image_hw, counts, k)
    cnt = cand["count"].cpu()
    assert cnt.tolist() == [len(r[0]) for r in ref]
    assert cnt[1] == 0 and cnt[0] > 8192  # (empty image; the global-memory sort path of osr_nms_topk)
    rows0 = set(ref[0][0].tolist())
    assert not rows0 & {0, 1, 2, 3} and {4, 5, 6, 7} <= rows0
    for i, (r_row, r_cls, r_sc, r_box) in enumerate(ref):
        c = int(cnt[i])
        assert torch.equal(cand["row"][i, :c].cpu().long(), r_row) and torch.equal(cand["cls"][i, :c].cpu().long(), r_cls)
        # (the kernel sums the K+1 exponentials of a row in order in fp32: within (K + 3) * 2^-24 relative of the exact softmax)
        torch.testing.assert_close(cand["scores"][i, :c].cpu().double(), r_sc, rtol=(k + 3) * 2.0 ** -24, atol=0)
        torch.testing.assert_close(cand["boxes"][i, :c].cpu(), r_box, rtol=1e-5, atol=1e-4)
        hw = image_hw[i].float()
        b = cand["boxes"][i, :c].cpu()
        assert (b >= 0).all() and (b[:, 0::2] <= hw[1]).all() and (b[:, 1::2] <= hw[0]).all()
    # osr_nms_topk over these candidates keeps what the oracle's batched NMS keeps over the same candidates. (Scores that differ by
    # an ulp between the device's expf and the CPU's exp may sort either way; the NMS contract is stated on identical inputs.)
    keep, kcnt = ops.nms_topk(cand["boxes"], cand["scores"], cand["cls"], None, n, cand["cap"], cand["count"], 0.5, 100)
    torch.cuda.synchronize()
    keep, kcnt = keep.cpu(), kcnt.cpu()
    for i in range(n):
        c = int(cnt[i])
        bx, sc, cl = cand["boxes"][i, :c].cpu().numpy(), cand["scores"][i, :c].cpu().numpy(), cand["cls"][i, :c].cpu().numpy()
        want = O.batched_nms_ref(bx, sc, cl, 0.5)[:100]
        got = keep[i, :int(kcnt[i])].numpy()
        assert np.array_equal(got, want), i
        assert (keep[i, int(kcnt[i]):] == -1).all()


@pytest.mark.gpu
def test_fastrcnn_candidates_end_to_end_kept_rows_match_the_oracle(osr):
    """The whole [d2] inference tail on one moderate image: kernel candidates + osr_nms_topk give the (row, class) list of
    oracle.fast_rcnn_inference_from_outputs. One class per row passes, with scores spread so that no two lie within a few ulps."""
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(5)
    rows, k = 600, 80
    logits = torch.full((rows, k + 1), -8.0)
    top = torch.randint(0, k, (rows,), generator=g)
    logits[torch.arange(rows), top] = torch.linspace(-1.0, 3.0, rows)[torch.randperm(rows, generator=g)]
    deltas = torch.randn(rows, 4 * k, generator=g) * 0.5
    deltas.view(rows, k, 4)[..., 2:] = 0.0  # (exp(0) = 1 on both sides: the boxes, and so the IoUs, are bit-equal)
    xy = torch.rand(rows, 2, generator=g) * 500.0
    prop = torch.cat([xy, xy + 20.0 + torch.rand(rows, 2, generator=g) * 200.0], 1)
    hw = (480, 560)
    cand = ops.fastrcnn_candidates(logits.to(DEV), deltas.to(DEV), prop.view(1, rows, 4).to(DEV), torch.tensor([rows], dtype=torch.int32, device=DEV),
                                   torch.tensor([hw], dtype=torch.int32, device=DEV), k, RW, THR)
    keep, kcnt = ops.nms_topk(cand["boxes"], cand["scores"], cand["cls"], None, 1, cand["cap"], cand["count"], 0.5, 100)
    torch.cuda.synchronize()
    cfg = dict(O.BASE_RCNN_CFG, score_thresh_test=THR, nms_thresh_test=0.5, detections_per_image=100)
    _, s_ref, _, rc_ref = O.fast_rcnn_inference_from_outputs(logits, deltas, prop, hw, cfg)
    s_sorted = s_ref.sort(descending=True).values
    assert bool(((s_sorted[:-1] - s_sorted[1:]) > 1e-6 * s_sorted[:-1]).all())  # (the premise of an exact comparison)
    kk = keep[0, :int(kcnt[0])].cpu().long()
    got = torch.stack([cand["row"][0].cpu().long()[kk], cand["cls"][0].cpu().long()[kk]], 1)
    assert torch.equal(got, rc_ref)
