"""osr_mask_upsample_predict (csrc/osr_mask_head.hip): ConvTranspose2d(2 x 2, stride 2) + bias + ReLU + the 1 x 1 predictor row of each
RoI's class + sigmoid in one launch, against the float64 chain conv_transpose2d -> relu -> conv2d -> select -> sigmoid on the same
storage-rounded operands (no intermediate rounding).

Bound: B = max(32 * e32, 1e-5), e32 = the error of the same chain in torch-CPU fp32 against float64, computed here. Measured on the
CPU at R = 3, C = 256: e32 = 2.5e-7, so B = 1e-5; a kernel that rounded the (R, 28, 28, C) intermediate to fp16 would err by 1.7e-4.
The weights are drawn so that the logits have a standard deviation of at least 0.5 (asserted): detectron2's std = 0.001 predictor
initialiser would put every probability at 0.5 and make the comparison vacuous.

R = 1 (196 rows) ends in a partial tile; R = 3 (588 rows) has tile boundaries inside every RoI, for the 64-row tiles of the fp16 / bf16
kernel and the 32-row tiles of the fp32 one. cin != cmid (64 / 128, 128 / 64, 256 / 64, 192 / 320) tells the two widths apart; cin 448
is the largest row tile that fits the LDS and 512 is refused with nothing written; s = 1, 7, 8, 9 put 64, two, one and two RoIs of
different classes into a tile (s < 8 is legal at inference), with class -1, class == num_rows and rows beyond rows_valid as exact zeros.
Measured on gfx950, the cases above in fp16 / bf16 / fp32: error 8e-8 .. 5.5e-7 at e32 1e-7 .. 5.5e-7, 0.01 .. 0.03 of the bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 14


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


@functools.lru_cache(maxsize=None)
def _operands(r: int, c: int, k: int, dt: torch.dtype, cmid=None, s: int = S):
    """x (r, s, s, c) and the deconv weight (c, cmid, 2, 2) rounded to dt; bias, predictor weight (k, cmid) and bias in fp32. cmid None:
    c. (The seed of a square case at s = 14 does not know of cmid and s: those cases keep their values.)"""
    g = torch.Generator().manual_seed(1000 * r + c + k + (0 if cmid is None else 31 * cmid) + (0 if s == S else 100003 * s))
    cmid = c if cmid is None else cmid
    x = torch.randn(r, s, s, c, generator=g).to(dt)
    w = (torch.randn(c, cmid, 2, 2, generator=g) * (2.0 / c) ** 0.5).to(dt)
    b = torch.randn(cmid, generator=g) * 0.1
    pw = torch.randn(k, cmid, generator=g) * (2.0 / cmid) ** 0.5
    pb = torch.randn(k, generator=g) * 0.1
    return x, w, b, pw, pb


def _chain(x, w, b, pw, pb, classes, dtype):
    """-> (probs (r, 2S, 2S), logits of the selected rows) in `dtype`; classes None: row 0."""
    xx = x.to(dtype).permute(0, 3, 1, 2)
    h = F.relu(F.conv_transpose2d(xx, w.to(dtype), b.to(dtype), stride=2))
    z = F.conv2d(h, pw.to(dtype)[:, :, None, None], pb.to(dtype))
    idx = torch.zeros(x.shape[0], dtype=torch.int64) if classes is None else classes.clamp(0, pw.shape[0] - 1)  # (dead RoIs: any row)
    z = z[torch.arange(x.shape[0]), idx]
    return torch.sigmoid(z), z


@functools.lru_cache(maxsize=None)
def _reference(r: int, c: int, k: int, dt: torch.dtype, classes_key, cmid=None, s: int = S):
    ops_ = _operands(r, c, k, dt, cmid, s)
    classes = None if classes_key is None else torch.tensor(classes_key, dtype=torch.int64)
    ref, z = _chain(*ops_, classes, torch.float64)
    p32, _ = _chain(*ops_, classes, torch.float32)
    e32 = float((p32.double() - ref).abs().max())
    return ref, z, e32


def _run(ops, osr, r, c, k, dt, classes, rows_valid=None, seg_rows=0, cmid=None, s: int = S):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb = _operands(r, c, k, dt, cmid, s)
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV)
    rv = None if rows_valid is None else torch.tensor(rows_valid, dtype=torch.int32, device=DEV)
    return ops.mask_upsample_predict(x.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV), cl, rv, seg_rows)


def _classes_for(r: int, k: int):
    if k == 1:
        return None
    return {1: (k - 1,), 3: (0, k - 1, 2)}[r]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c", [256, 64])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("r", [1, 3])
def test_against_the_float64_chain(ops, osr, r, c, k, dt):
    classes = _classes_for(r, k)
    ref, z, e32 = _reference(r, c, k, dt, classes)
    assert float(z.std()) >= 0.5, f"the reference logits must spread (std {float(z.std()):.3f})"
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, r, c, k, dt, classes)
    assert out.shape == (r, 2 * S, 2 * S) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print(f"r={r} c={c} k={k} {dt}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}, logit std {float(z.std()):.3f}")
    assert err <= bound, f"max |probs - float64| {err:.3e} > {bound:.3e} (e32 {e32:.3e})"
    assert torch.equal(_run(ops, osr, r, c, k, dt, classes), out), "two runs are bit-identical"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [1, 5])
def test_no_rois(ops, osr, k, dt):
    out = _run(ops, osr, 0, 64, k, dt, None if k == 1 else ())
    assert out.shape == (0, 2 * S, 2 * S) and out.dtype == torch.float32


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k", [1, 5])
def test_padding_rows_and_class_minus_one_are_zeros(ops, osr, k, dt):
    """Six RoIs as two segments of three with rows_valid (2, 1): RoIs 2, 4 and 5 do not exist; RoI 1 exists with class -1. The four
    rows come out as exact zeros (their inputs are finite but arbitrary), the two live ones as the reference's."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    c = 256
    classes = (0, -1, 3, k - 1, 2, 1) if k > 1 else (0, -1, 0, 0, 0, 0)
    x, w, b, pw, pb = _operands(6, c, k, dt)
    live = [0, 3]
    ref, z, e32 = _reference(6, c, k, dt, classes)
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, 6, c, k, dt, classes, (2, 1), 3).cpu()
    for i in range(6):
        if i in live:
            err = float((out[i].double() - ref[i]).abs().max())
            assert err <= bound, (i, err, bound)
            assert float(out[i].min()) > 0.0
        else:
            assert float(out[i].abs().max()) == 0.0, f"RoI {i} must be zeros"
    # the same rows with non-finite inputs still come out as zeros: they are selected away, not multiplied away
    xn = x.clone()
    xn[[1, 2, 4, 5]] = float("nan")
    outn = ops.mask_upsample_predict(xn.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV),
                                     torch.tensor(classes, dtype=torch.int64, device=DEV), torch.tensor([2, 1], dtype=torch.int32, device=DEV), 3).cpu()
    assert torch.equal(outn, out)
    # without rows_valid only the class decides
    out2 = _run(ops, osr, 6, c, k, dt, classes).cpu()
    assert float(out2[1].abs().max()) == 0.0 and all(float(out2[i].min()) > 0.0 for i in (0, 2, 3, 4, 5))
    assert torch.equal(out2[live], out[live])


def _against_float64(ops, osr, r, c, k, dt, classes, cmid, s=S, name=""):
    ref, z, e32 = _reference(r, c, k, dt, classes, cmid, s)
    assert float(z.std()) >= 0.5, f"the reference logits must spread (std {float(z.std()):.3f})"
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, r, c, k, dt, classes, cmid=cmid, s=s)
    assert out.shape == (r, 2 * s, 2 * s) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print(f"{name} r={r} cin={c} cmid={cmid} k={k} s={s} {dt}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e} ({err / bound:.2f} of it)")
    assert err <= bound, f"max |probs - float64| {err:.3e} > {bound:.3e} (e32 {e32:.3e})"
    return out


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cin,cmid", [(64, 128), (128, 64), (256, 64), (192, 320)])
@pytest.mark.parametrize("k", [1, 5])
def test_input_and_output_widths_differ(ops, osr, cin, cmid, k, dt):
    """cin rules the LDS row, the K loop and the weight's fragment stride; cmid the chunk loop, the bias and the predictor row: with
    cin == cmid an exchange of the two goes unseen. 192 is three K blocks of 64, 320 five chunks."""
    _against_float64(ops, osr, 3, cin, k, dt, _classes_for(3, k), cmid)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
def test_the_widest_input_that_fits_and_the_first_that_does_not(ops, osr, dt):
    """cin 448 is the largest row tile that fits 64 KB of LDS (58 KB dynamic); 512 is refused with nothing written."""
    import ctypes as C
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    _against_float64(ops, osr, 2, 448, 5, dt, (1, 4), 64)
    esz, bm = torch.empty(0, dtype=dt).element_size(), 32 if dt == torch.float32 else 64
    assert bm * (448 * esz + 16) + bm * 4 <= 65536 < bm * (512 * esz + 16) + bm * 4, "csrc/osr_mask_head.hip mask_head_launch's rule"
    x, w, b, pw, pb = (t.to(DEV) for t in _operands(2, 512, 5, dt, 64))
    wp = pack_deconv_weight(w, dt).to(DEV)
    cl = torch.tensor([1, 4], dtype=torch.int64, device=DEV)
    with pytest.raises(osr.OsrError, match="does not fit"):
        ops.mask_upsample_predict(x, wp, b, pw, pb, cl)
    L, lib = osr._lib, osr._lib.load()
    probs = torch.full((2, 2 * S, 2 * S), -7.0, device=DEV)
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = lib.osr_mask_upsample_predict(p_(x), ops.dtype_code(dt), 2, S, 512, 64, p_(wp), p_(b), p_(pw), p_(pb), 5, p_(cl), None, 0, p_(probs), None)
    torch.cuda.synchronize()
    assert st == L.ERR_UNSUPPORTED and b"does not fit" in lib.osr_last_error()
    assert bool((probs == -7.0).all())


def _small_side_case(s: int):
    r = 70 if s == 1 else 5
    classes = tuple((0, 1, 2, 3, 4, -1, 5)[i % 7] for i in range(r)) if s == 1 else (0, 3, -1, 5, 4)
    seg, rv = (35, (33, 20)) if s == 1 else (3, (2, 1))
    return r, classes, seg, rv


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("segments", [False, True])
@pytest.mark.parametrize("s", [1, 7, 8, 9])
def test_other_sides(ops, osr, s, segments, dt):
    """s < 8 is legal at inference: a 64-row tile then holds RoIs of several classes (s = 1: 64 of them, s = 7: 49 rows each), and
    every row takes the predictor row of its own RoI. s = 8 is exactly one RoI per tile, 9 moves the boundaries in every RoI. Classes
    -1 and 5 == num_rows, and with `segments` the RoIs beyond rows_valid, are exact zeros whatever their inputs."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    k, c = 5, 64
    r, classes, seg, rv = _small_side_case(s)
    live = [0 <= cl < k and (not segments or i % seg < rv[i // seg]) for i, cl in enumerate(classes)]
    assert len({classes[i] for i in range(min(r, max(64 // (s * s), 2))) if live[i]}) >= 2, "the first tile holds RoIs of different classes"
    assert not all(live) and (not segments or sum(live) < sum(0 <= cl < k for cl in classes))
    ref, z, e32 = _reference(r, c, k, dt, classes, None, s)
    lv = torch.tensor(live)
    assert float(z[lv].std()) >= 0.5
    bound = max(32 * e32, 1e-5)
    out = _run(ops, osr, r, c, k, dt, classes, rv if segments else None, seg if segments else 0, s=s).cpu()
    assert out.shape == (r, 2 * s, 2 * s)
    err = float((out[lv].double() - ref[lv]).abs().max())
    print(f"s={s} segments={segments} {dt}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e} ({err / bound:.2f} of it)")
    assert err <= bound
    assert float(out[lv].min()) > 0.0 and torch.equal(out[~lv], torch.zeros_like(out[~lv]))
    x, w, b, pw, pb = _operands(r, c, k, dt, None, s)
    xn = x.clone()
    xn[~lv] = float("nan")
    outn = ops.mask_upsample_predict(xn.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV),
                                     torch.tensor(classes, dtype=torch.int64, device=DEV),
                                     torch.tensor(rv, dtype=torch.int32, device=DEV) if segments else None, seg if segments else 0).cpu()
    assert torch.equal(outn, out), "RoIs that do not count are selected away, not multiplied away"


def test_logits_entry_point_with_unequal_widths(ops, osr):
    """tests/test_mask_tail_bwd.py test_logits_output_and_unchanged_probs's rule at cin != cmid: with the logits as a second output the
    probabilities are mask_upsample_predict's, bit for bit."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    r, cin, cmid, k, dt = 3, 64, 128, 5, torch.float16
    classes = _classes_for(r, k)
    x, w, b, pw, pb = _operands(r, cin, k, dt, cmid)
    args = (x.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV), torch.tensor(classes, dtype=torch.int64, device=DEV))
    probs = ops.mask_upsample_predict(*args)
    logits, again = ops.mask_upsample_logits(*args, probs=True)
    assert torch.equal(again, probs) and torch.equal(probs, _run(ops, osr, r, cin, k, dt, classes, cmid=cmid))
    assert torch.equal(ops.mask_upsample_logits(*args), logits)


def test_a_lossy_intermediate_would_be_caught():
    """The bound tells the fused form from one that stores the deconv output in fp16: rounding h costs more than B (CPU only)."""
    x, w, b, pw, pb = _operands(3, 256, 1, torch.float16)
    ref, _, e32 = _reference(3, 256, 1, torch.float16, None)
    h = F.relu(F.conv_transpose2d(x.float().permute(0, 3, 1, 2), w.float(), b, stride=2)).half().float()
    lossy = torch.sigmoid(F.conv2d(h, pw[:, :, None, None], pb))[:, 0]
    assert float((lossy.double() - ref).abs().max()) > 4 * max(32 * e32, 1e-5)


def test_shape_rules(ops, osr):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb = [t.to(DEV) if i != 1 else t for i, t in enumerate(_operands(1, 64, 5, torch.float16))]
    wp = pack_deconv_weight(w, torch.float16).to(DEV)
    with pytest.raises(osr.OsrError, match="classes"):  # a class-specific predictor needs the classes
        ops.mask_upsample_predict(x, wp, b, pw, pb, None)
    with pytest.raises(osr.OsrError, match="multiples of 64"):
        ops.mask_upsample_predict(x[..., :32].contiguous(), wp[:, :, :2].contiguous(), b, pw, pb, torch.zeros(1, dtype=torch.int64, device=DEV))
