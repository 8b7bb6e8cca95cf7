"""osr_rpn_select_wide: proposal selection with up to 8192 proposals per level -- the single-level C4 RPN ([d2] Base-RCNN-C4.yaml: one
level at stride 16, 5 sizes x 3 ratios = 15 anchors per cell, PRE_NMS_TOPK_TEST 6000) -- against the CPU oracle.

One level, A = 15, n = 2. Two grids: 20 x 28 (8400 anchors: above the 8192-pair list, so every k selects) and 16 x 20 (4800 anchors:
every k clamps to the count and the level is taken whole). The scores are multiples of 1/64, so ties are many (a few hundred distinct
values over 8400 anchors) and the order inside them -- lower index first -- decides most of the list.

Exact: counts, src_index, scores, level, batch_idx, the padding, the ltrb boxes. The Box2BoxTransform boxes go through expf, which is
a different function on the two sides: rtol 1e-5, atol 1e-4, the tolerance tests/test_standard_rcnn.py holds the same decode to."""
import pytest
import torch

from oracle import c_binding as CO
from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A, N, STRIDE = 15, 2, 16
SIZES, RATIOS = (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)
BIG, SMALL = (20, 28), (16, 20)
IMAGE_SIZES = {BIG: [(320, 448), (300, 430)], SMALL: [(256, 320), (250, 300)]}
ONES = (1.0, 1.0, 1.0, 1.0)
POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000
KS = [2049, 4096, 6000, 8192]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def bits(t):
    return t.contiguous().view(torch.int32)


def set_bits(t, index, pattern):
    t.view(torch.int32)[index] = pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def stock_cells():
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    return cell_anchor_table([list(SIZES)], RATIOS)  # (1, 15, 4), size-major


def dyadic_cells():
    base = torch.tensor([[-16.0, -8.0, 16.0, 8.0], [-16.0, -16.0, 16.0, 16.0], [-8.0, -16.0, 8.0, 16.0]])
    return torch.cat([base * 2 ** s for s in range(5)]).view(1, A, 4)


def grid_anchors(shape, cell):
    h, w = shape
    sx, sy = torch.arange(0, w * STRIDE, step=STRIDE, dtype=torch.float32), torch.arange(0, h * STRIDE, step=STRIDE, dtype=torch.float32)
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
    return (shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4)


def oracle_anchors(shape):
    """[d2] DefaultAnchorGenerator with five sizes on one level, from O.anchor_grid (one size per call): size-major, then ratio."""
    hw = shape[0] * shape[1]
    per = [O.anchor_grid([shape], [STRIDE], [z], RATIOS)[0].view(hw, len(RATIOS), 4) for z in SIZES]
    return torch.cat(per, dim=1).reshape(-1, 4)


class Case:
    def __init__(self, shape, kind, seed, weights):
        self.shape, self.weights = shape, weights
        self.cnt = shape[0] * shape[1] * A
        self.image_sizes = IMAGE_SIZES[shape]
        gg = torch.Generator().manual_seed(seed)
        self.scores = ((2 * torch.randn(N, self.cnt, generator=gg)) * 64).round() / 64  # multiples of 1/64
        if kind == "float":
            self.cell = stock_cells()
            self.anchors = oracle_anchors(shape)
            assert torch.equal(self.anchors, grid_anchors(shape, self.cell))
            d = torch.randn(N, self.cnt, 4, generator=gg) * torch.tensor([0.5, 0.5, 1.0, 1.0])
            d[..., 2:] = torch.where(torch.rand(N, self.cnt, 1, generator=gg) < 0.5, torch.zeros(()), d[..., 2:])
        else:  # dyadic anchors, dw = dh = 0, dx and dy multiples of 1/8: every decoded coordinate is exact in fp32
            self.cell = dyadic_cells()
            self.anchors = grid_anchors(shape, self.cell)
            d = torch.zeros(N, self.cnt, 4)
            d[..., :2] = torch.randint(-16, 17, (N, self.cnt, 2), generator=gg).float() / 8
        self.deltas = d

    def decoded(self):
        flat = self.anchors.unsqueeze(0).expand(N, -1, -1).reshape(-1, 4)
        if self.weights is None:
            return O.ltrb_apply_deltas(self.deltas.reshape(-1, 4), flat).view(N, -1, 4)
        return O.b2b_apply_deltas(self.deltas.reshape(-1, 4), flat, self.weights).view(N, -1, 4)

    def reference(self, k):
        props = self.decoded()
        ref = O.find_top_rpn_proposals([props], [self.scores], self.image_sizes, k, 0.0)
        v, idx = O.stable_topk(self.scores, min(self.cnt, k))
        b = props[torch.arange(N)[:, None], idx]
        bad = not bool(torch.isfinite(b).all() and torch.isfinite(v).all())
        return props, ref, bad

    def select(self, ops, k, wide=True):
        lv = ops.make_rpn_levels([self.shape], (STRIDE,), N, A)
        hw = torch.tensor(self.image_sizes, dtype=torch.int32)
        fn = ops.rpn_select_wide if wide else ops.rpn_select
        r = fn(lv, self.cell.to(DEV), self.scores.reshape(-1).to(DEV), self.deltas.reshape(-1, 4).to(DEV), N, hw.to(DEV), k, 0.0,
               b2b_weights=self.weights)
        torch.cuda.synchronize()
        return r


def check(c, r, ref, bad, k, name):
    cap = min(c.cnt, k)
    assert r["cap"] == cap
    counts, src, scores, boxes = r["counts"].cpu(), r["src_index"].cpu(), r["scores"].cpu(), r["boxes"].cpu()
    bidx = r["batch_idx"].cpu().view(N, cap)
    assert (c.weights is None) == ("level" not in r)
    flag = int(r["status_flags"].cpu()[0])
    assert (flag != 0) == bad, f"{name}: status_flags {flag}, the reference meets non-finite: {bad}"
    for i, (rb, rs, ri) in enumerate(ref):
        cnt = int(counts[i])
        assert cnt == len(rb), f"{name} image {i}: count {cnt} vs {len(rb)}"
        assert torch.equal(src[i, :cnt].long(), ri), f"{name} image {i}: selected anchor indices (or their order inside ties) differ"
        assert torch.equal(bits(scores[i, :cnt]), bits(rs)), f"{name} image {i}: scores differ"
        if "level" in r:
            lv = r["level"].cpu()
            assert bool((lv[i, :cnt] == 0).all()) and bool((lv[i, cnt:] == -1).all())
        assert bool((bidx[i, :cnt] == i).all()) and bool((bidx[i, cnt:] == -1).all()) and bool((src[i, cnt:] == -1).all())
        assert bool((bits(boxes[i, cnt:]) == 0).all()) and bool((bits(scores[i, cnt:]) == 0).all()), f"{name} image {i}: padding is not zero"
        if c.weights is None:
            assert torch.equal(boxes[i, :cnt], rb), f"{name} image {i}: ltrb boxes not bit-exact"
        else:
            assert torch.allclose(boxes[i, :cnt], rb, rtol=1e-5, atol=1e-4), \
                f"{name} image {i}: boxes differ by {float((boxes[i, :cnt] - rb).abs().max()):.3e}"


def same_outputs(r1, r2):
    keys = ["boxes", "scores", "src_index", "counts", "batch_idx", "status_flags"] + (["level"] if "level" in r1 else [])
    assert ("level" in r1) == ("level" in r2) and r1["cap"] == r2["cap"]
    for key in keys:
        a, b = r1[key].cpu(), r2[key].cpu()
        if not torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b):
            return False
    return True


@pytest.fixture(scope="module")
def cases():
    """The inputs of every test below, built once: (grid, decode mode) -> Case."""
    out = {}
    for shape in (BIG, SMALL):
        for mode, weights in ((1, ONES), (0, None)):
            out[shape, mode] = Case(shape, "float", seed=11 + mode, weights=weights)
    return out


@pytest.mark.parametrize("mode", [1, 0], ids=["b2b", "ltrb"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", [BIG, SMALL], ids=["8400", "4800"])
def test_against_the_oracle(ops, cases, shape, k, mode):
    c = cases[shape, mode]
    assert (c.cnt > 8192) == (shape == BIG)
    distinct = len(torch.unique(c.scores[0]))
    assert distinct < c.cnt // 4, f"{distinct} distinct scores among {c.cnt}: ties are the rule"
    _, ref, bad = c.reference(k)
    assert not bad
    v, _ = O.stable_topk(c.scores, min(c.cnt, k))
    if shape == BIG and k < 8192:  # the k-th value is shared with anchors that are not selected: the tie rule decides who is
        assert all(int((c.scores[i] == v[i, -1]).sum()) > int((v[i] == v[i, -1]).sum()) for i in range(N))
    r = c.select(ops, k)
    check(c, r, ref, bad, k, f"{shape} k={k} mode {mode}")


@pytest.mark.parametrize("mode", [1, 0], ids=["b2b", "ltrb"])
def test_nan_of_each_sign_ranks_first_is_dropped_and_flagged(ops, cases, mode):
    base = cases[BIG, mode]
    c = Case(BIG, "float", seed=11 + mode, weights=base.weights)
    low0, low1 = int(c.scores[0].argmin()), int(c.scores[1].argmin())  # (the worst anchors: never selected as numbers)
    set_bits(c.scores, (0, low0), POS_NAN)
    set_bits(c.scores, (1, low1), NEG_NAN)
    assert int(bits(c.scores)[1, low1]) == NEG_NAN - (1 << 32)
    _, ref, bad = c.reference(6000)
    assert bad
    _, clean, _ = base.reference(6000)
    r = c.select(ops, 6000)
    check(c, r, ref, True, 6000, f"NaN mode {mode}")
    for i, low in enumerate((low0, low1)):
        assert low not in set(ref[i][2].tolist()) and low not in set(r["src_index"].cpu()[i].tolist())
        # the NaN took a slot of the 6000 and was dropped: the selection is the clean top 5999, so the kept list is the clean one, short
        # of its last entry when that was the clean selection's 6000th anchor
        got, want = ref[i][2], clean[i][2]
        assert len(want) - len(got) in (0, 1) and torch.equal(got, want[:len(got)])
    assert int(base.select(ops, 6000)["status_flags"].cpu()[0]) == 0


@pytest.mark.parametrize("mode", [1, 0], ids=["b2b", "ltrb"])
@pytest.mark.parametrize("k", [1000, 2048])
@pytest.mark.parametrize("shape", [BIG, SMALL], ids=["8400", "4800"])
def test_bit_identical_to_rpn_select_where_both_serve(ops, cases, shape, k, mode):
    c = cases[shape, mode]
    assert same_outputs(c.select(ops, k, wide=True), c.select(ops, k, wide=False))


def test_refused_above_8192(ops, osr):
    c = Case(SMALL, "dyadic", seed=3, weights=ONES)
    with pytest.raises(osr._lib.OsrError, match=r"status -2"):
        c.select(ops, 8193)
    lib, lv = osr._lib.load(), ops.make_rpn_levels([SMALL], (STRIDE,), N, A)
    import ctypes
    assert lib.osr_rpn_select_wide_capacity(ctypes.byref(lv), 8193) == -2
    assert lib.osr_rpn_select_wide_workspace_bytes(ctypes.byref(lv), N, 8193) == -2
    assert lib.osr_rpn_select_wide_capacity(ctypes.byref(lv), 8192) == 4800
    assert c.select(ops, 8192)["cap"] == 4800  # the limit itself is served
    with pytest.raises(osr._lib.OsrError):
        c.select(ops, 0)


def test_select_nms_topk_chain_at_6000(ops, monkeypatch):
    """The C4 RPN's chain as the engine runs it: wide select (6000) -> NMS at 0.7 -> the first 1000, on inputs whose decode is exact."""
    monkeypatch.setattr(O, "batched_nms_ref", CO.batched_nms)  # (same kept list as the numpy one: tests/test_oracle_kat.py)
    c = Case(BIG, "dyadic", seed=8, weights=ONES)
    props, ref, bad = c.reference(6000)
    sel = c.select(ops, 6000)
    check(c, sel, ref, bad, 6000, "chain")
    for i, (rb, _, _) in enumerate(ref):
        assert torch.equal(sel["boxes"].cpu()[i, :len(rb)], rb)  # exact inputs: exact boxes
    cap, post = sel["cap"], 1000
    pk, pcnt = ops.nms_topk(sel["boxes"], sel["scores"], sel["level"], None, N, cap, sel["counts"], 0.7, post)
    boxes = ops.gather_rows(sel["boxes"].view(-1, 4), cap, pk, pcnt).cpu()
    scores = ops.gather_rows(sel["scores"].view(-1), cap, pk, pcnt).view(N, post).cpu()
    want = O.standard_find_top_rpn_proposals([props], [c.scores], c.image_sizes, 0.7, 6000, post, 0.0)
    pcnt = pcnt.cpu()
    for i, (wb, ws, _) in enumerate(want):
        m = int(pcnt[i])
        assert m == len(wb), f"image {i}: {m} proposals vs {len(wb)}"
        assert torch.equal(bits(scores[i, :m]), bits(ws)) and torch.equal(boxes[i, :m], wb), f"image {i}: kept proposals differ"
        assert bool((pk.cpu()[i, m:] == -1).all())


def test_repeats_are_bit_identical(ops, cases):
    c = cases[BIG, 1]
    first = c.select(ops, 6000)
    for _ in range(2):
        assert same_outputs(first, c.select(ops, 6000))
