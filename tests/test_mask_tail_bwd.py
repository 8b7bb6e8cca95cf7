"""osr_mask_upsample_predict_bwd and the logits output of the tail's forward (csrc/osr_mask_train.hip, csrc/osr_mask_head.hip) against
the float64 autograd of conv_transpose2d -> relu -> conv2d -> select on the storage-rounded operands. The operands are drawn as
tests/test_mask_upsample_predict.py draws them (He-scaled weights, a bias of 0.1), so that about half of the upsampled activation is
cut by the ReLU.

Bounds:
  dx, deconv dw        2e-3 of the tensor's largest magnitude -- what tests/test_conv_bwd.py grants the MFMA gradient kernels (the
                       gradient of the upsampled activation enters both contractions in the storage type); dx is read in
                       fp32, as that test reads a data gradient, and in the storage type against the same values rounded once
  d_pred_w, d_pred_b,  max(32 * e32, 1e-5) relative, e32 = the error of the same chain's torch-CPU fp32 autograd against float64,
  d_deconv_b           computed here: they come from fp32 accumulators (the rule of the forward's test)
Measured on gfx950: fp16 dx / dw 1.6e-4 .. 2.5e-4, the three fp32 sums 2e-8 .. 9e-7. bf16 would carry the gradient of the upsampled
activation with 8 significant bits (dx / dw 1.3e-3 .. 2.5e-3, over the bound in three cases), so the kernel splits it into two bf16
planes, hi + lo: dx / dw 2.0e-6 .. 3.3e-6.
R = 1 (196 rows) ends in a partial tile, R = 3 has tile boundaries inside every RoI; R = 6 as two segments with rows_valid (2, 0)
has an empty segment, a RoI that does not exist and one with class -1.
Further cases, same bounds: cin 320 / 448 (the four-blocks-per-wave instantiation, 10 and 14 column blocks of dx, each compared);
cin 192 (6 blocks) and cmid 64 / 320 (one and five chunks); s = 8, 9, 11, 13 (where a RoI begins in its tile); 40 RoIs, 123 tiles and
80 predictor rows; want_g=False; the LDS limit (bf16 448 / 576 runs, 448 / 640, fp16 448 / 1408 and cin 512 are refused with nothing
written); one test that the forward, the loss and both backwards agree on which rows count.
Measured on gfx950 over these: fp16 dx 1.8e-4 .. 3.0e-4, dw 1.6e-4 .. 2.5e-4 (at most 0.15 of the bound); bf16 dx 2.3e-6 .. 3.2e-6, dw
2.2e-6 .. 3.3e-6; the three fp32 sums 4.6e-8 .. 4.2e-7 relative, at most 0.03 of their bounds (e32 3e-7 .. 2.5e-6)."""
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
def _operands(r: int, cin: int, cmid: int, k: int, dt: torch.dtype, s: int = S):
    g = torch.Generator().manual_seed(1000 * r + cin + k + (0 if s == S else 100003 * s))  # (s = 14: the seed it has always had)
    x = torch.randn(r, s, s, cin, generator=g).to(dt)
    w = (torch.randn(cin, cmid, 2, 2, generator=g) * (2.0 / cin) ** 0.5).to(dt)
    b = torch.randn(cmid, generator=g) * 0.1
    pw = torch.randn(k, cmid, generator=g) * (2.0 / cmid) ** 0.5
    pb = torch.randn(k, generator=g) * 0.1
    dl = torch.randn(r, 2 * s, 2 * s, generator=g)
    # No pre-activation may sit on the ReLU's kink: within fp32's error of 0 the float64 reference and any fp32 evaluation take
    # different branches of a derivative that is not defined there. A channel with |u| < 1e-4 somewhere gets its bias moved by 1e-3.
    for _ in range(50):
        u = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2)
        near = (u.abs() < 1e-4).any(dim=3).any(dim=2).any(dim=0)
        if not bool(near.any()):
            break
        b[near] += 1e-3
    else:
        raise AssertionError("could not move the pre-activations off the ReLU's kink")
    return x, w, b, pw, pb, dl


def _autograd(x, w, b, pw, pb, dl, classes, live, dtype):
    """-> (logits (r, 2S, 2S), dict of gradients) of sum(logits * dl) over the live RoIs, everything in `dtype`."""
    xx = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    ww, bb, pww, pbb = (t.to(dtype).requires_grad_(True) for t in (w, b, pw, pb))
    u = F.conv_transpose2d(xx, ww, bb, stride=2)
    frac = float((u > 0).double().mean())
    z = F.conv2d(F.relu(u), pww[:, :, None, None], pbb)
    idx = torch.zeros(x.shape[0], dtype=torch.int64) if classes is None else classes.clamp(0, pw.shape[0] - 1)  # (dead RoIs: any row)
    z = z[torch.arange(x.shape[0]), idx]
    keep = live.to(dtype)[:, None, None]
    (z * dl.to(dtype) * keep).sum().backward()
    grads = dict(dx=xx.grad.permute(0, 2, 3, 1), dw=ww.grad, d_deconv_b=bb.grad, d_pred_w=pww.grad, d_pred_b=pbb.grad)
    return (z * keep).detach(), grads, frac


@functools.lru_cache(maxsize=None)
def _reference(r, cin, cmid, k, dt, classes_key, live_key, s=S):
    o = _operands(r, cin, cmid, k, dt, s)
    classes = None if classes_key is None else torch.tensor(classes_key, dtype=torch.int64)
    live = torch.tensor(live_key, dtype=torch.bool)
    z, ref, frac = _autograd(*o, classes, live, torch.float64)
    _, g32, _ = _autograd(*o, classes, live, torch.float32)
    e32 = {n: float((g32[n].double() - ref[n]).abs().max() / ref[n].abs().max().clamp(min=1e-30)) for n in ("d_pred_w", "d_pred_b", "d_deconv_b")}
    return z, ref, e32, frac


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _run(ops, r, cin, cmid, k, dt, classes, rows_valid=None, seg_rows=0, dx_dtype=None, s=S, want_g=True):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb, dl = _operands(r, cin, cmid, k, dt, s)
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV)
    rv = None if rows_valid is None else torch.tensor(rows_valid, dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    out = ops.mask_upsample_predict_bwd(xd, pack_deconv_weight(w, dt).to(DEV), pack_deconv_weight(w.transpose(0, 1), dt).to(DEV), b.to(DEV),
                                        pw.to(DEV), dl.to(DEV), cl, rv, seg_rows, want_g=want_g, dx_dtype=dx_dtype)
    if want_g:
        out["dw"] = ops.deconv_wgrad(xd, out["g"])
    return out


def _check(out, ref, e32, dt, name):
    errs = {n: _rel(out[n], ref[n]) for n in ("dx", "dw", "d_pred_w", "d_pred_b", "d_deconv_b")}
    bounds = {"dx": 2e-3, "dw": 2e-3, **{n: max(32 * e32[n], 1e-5) for n in e32}}
    print(name, " ".join(f"{n} {errs[n]:.2e} (<= {bounds[n]:.2e})" for n in errs))
    for n in errs:
        assert errs[n] <= bounds[n], f"{name}: {n} relative error {errs[n]:.3e} > {bounds[n]:.3e}"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cmid", [(256, 256), (64, 128)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("r", [1, 3])
def test_against_float64_autograd(ops, r, cin, cmid, k, dt):
    classes = None if k == 1 else {1: (k - 1,), 3: (0, -1, 2)}[r]  # (R = 3, K = 3: the middle RoI has class -1)
    live = tuple(True if classes is None else c >= 0 for c in (classes or (0,) * r))
    z, ref, e32, frac = _reference(r, cin, cmid, k, dt, classes, live)
    assert 0.2 < frac < 0.8, f"the ReLU must cut a real share of the activation (u > 0 on {frac:.2f})"
    out = _run(ops, r, cin, cmid, k, dt, classes, dx_dtype=torch.float32)
    assert out["dx"].dtype == torch.float32 and out["g"].dtype == dt and tuple(out["g"].shape) == (4 if dt == torch.float16 else 8, r * S * S, cmid)
    _check(out, ref, e32, dt, f"r={r} cin={cin} cmid={cmid} k={k} {dt}:")
    again = _run(ops, r, cin, cmid, k, dt, classes, dx_dtype=torch.float32)
    for n in ("dx", "g", "dw", "d_pred_w", "d_pred_b", "d_deconv_b"):
        assert torch.equal(again[n], out[n]), f"{n}: two launches are bit-identical"
    # dx in the storage type is the fp32 result rounded once
    stored = _run(ops, r, cin, cmid, k, dt, classes)
    assert stored["dx"].dtype == dt and torch.equal(stored["dx"], out["dx"].to(dt))
    for i, alive in enumerate(live):
        if not alive:
            assert float(out["dx"][i].abs().max()) == 0.0 and float(out["g"][:, i * S * S:(i + 1) * S * S].abs().max()) == 0.0


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 3])
def test_segments_with_an_empty_one(ops, k, dt):
    """Six RoIs as two segments of three with rows_valid (2, 0): RoI 2 and the whole second segment do not exist, RoI 1 has class -1
    when the predictor is class-specific. Their inputs are NaN: they are selected away, not multiplied away."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    cin = cmid = 256
    classes = (k - 1, -1, 0, 1, 0, 2) if k > 1 else None
    live = (True, k == 1, False, False, False, False)
    z, ref, e32, _ = _reference(6, cin, cmid, k, dt, classes, live)
    out = _run(ops, 6, cin, cmid, k, dt, classes, (2, 0), 3, dx_dtype=torch.float32)
    _check(out, ref, e32, dt, f"segments k={k} {dt}:")
    dead = [i for i, a in enumerate(live) if not a]
    assert float(out["dx"][dead].abs().max()) == 0.0
    x, w, b, pw, pb, dl = _operands(6, cin, cmid, k, dt)
    xn, dn = x.clone(), dl.clone()
    xn[dead] = float("nan")
    dn[dead] = float("nan")
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV)
    rv = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    if k == 1:  # (class-agnostic: RoI 1 is live; only the rows beyond rows_valid are dead)
        cl = None
    outn = ops.mask_upsample_predict_bwd(xn.to(DEV), pack_deconv_weight(w, dt).to(DEV), pack_deconv_weight(w.transpose(0, 1), dt).to(DEV), b.to(DEV),
                                         pw.to(DEV), dn.to(DEV), cl, rv, 3, dx_dtype=torch.float32)
    for n in ("dx", "g", "d_pred_w", "d_pred_b", "d_deconv_b"):
        assert torch.equal(outn[n], out[n]), n
    # nothing counts at all: every gradient is an exact zero
    none = ops.mask_upsample_predict_bwd(xn.to(DEV), pack_deconv_weight(w, dt).to(DEV), pack_deconv_weight(w.transpose(0, 1), dt).to(DEV), b.to(DEV),
                                         pw.to(DEV), dn.to(DEV), cl, torch.zeros(2, dtype=torch.int32, device=DEV), 3)
    for n in ("dx", "g", "d_pred_w", "d_pred_b", "d_deconv_b"):
        assert float(none[n].float().abs().max()) == 0.0, n


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 3])
def test_logits_output_and_unchanged_probs(ops, k, dt):
    """The logits of the sibling entry point against float64 (the forward test's rule: max(32 * e32, 1e-5), on the logits), against
    logit(probs) of the existing entry point, and that entry point's probs bit for bit with and without the second output."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    r, cin, cmid = 3, 256, 256
    classes = None if k == 1 else (0, -1, 2)
    live = tuple(True if classes is None else c >= 0 for c in (classes or (0,) * r))
    x, w, b, pw, pb, dl = _operands(r, cin, cmid, k, dt)
    z64, _, _, _ = _reference(r, cin, cmid, k, dt, classes, live)
    z32, _, _ = _autograd(x, w, b, pw, pb, dl, None if classes is None else torch.tensor(classes), torch.tensor(live), torch.float32)
    e32 = float((z32.double() - z64).abs().max())
    args = (x.to(DEV), pack_deconv_weight(w, dt).to(DEV), b.to(DEV), pw.to(DEV), pb.to(DEV),
            None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV))
    before = ops.mask_upsample_predict(*args)
    logits, probs = ops.mask_upsample_logits(*args, probs=True)
    after = ops.mask_upsample_predict(*args)
    assert torch.equal(before, probs) and torch.equal(before, after), "the probabilities do not move"
    assert torch.equal(ops.mask_upsample_logits(*args), logits)
    err = float((logits.cpu().double() - z64).abs().max())
    print(f"k={k} {dt}: logits err {err:.3e}, e32 {e32:.3e}")
    assert err <= max(32 * e32, 1e-5)
    lv = torch.tensor(live)
    assert float(logits.cpu()[~lv].abs().max() if (~lv).any() else 0.0) == 0.0
    gap = float((torch.sigmoid(logits.cpu().double()[lv]) - probs.cpu().double()[lv]).abs().max())
    assert gap <= 1e-5, f"sigmoid(logits) is the probability the existing entry point returns (gap {gap:.3e})"


def _live(classes, k, r, rows_valid=None, seg_rows=0):
    """mt_row_class >= 0 (csrc/osr_mask_mfma.h) restated: the RoI exists in its segment, and its class is a predictor row -- any class
    >= 0 when the predictor has one row."""
    return tuple((rows_valid is None or i % seg_rows < rows_valid[i // seg_rows])
                 and (classes is None or (classes[i] >= 0 and (k == 1 or classes[i] < k))) for i in range(r))


def _against_float64(ops, r, cin, cmid, k, dt, classes, rows_valid=None, seg_rows=0, s=S, name=""):
    live = _live(classes, k, r, rows_valid, seg_rows)
    z, ref, e32, frac = _reference(r, cin, cmid, k, dt, classes, live, s)
    assert 0.2 < frac < 0.8, f"the ReLU must cut a real share of the activation (u > 0 on {frac:.2f})"
    out = _run(ops, r, cin, cmid, k, dt, classes, rows_valid, seg_rows, dx_dtype=torch.float32, s=s)
    _check(out, ref, e32, dt, f"{name} r={r} s={s} cin={cin} cmid={cmid} k={k} {dt}:")
    dead = [i for i, a in enumerate(live) if not a]
    if dead:
        assert torch.equal(out["dx"][dead], torch.zeros_like(out["dx"][dead])), "RoIs that do not count have exact zeros"
    return out, ref, live


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cmid", [(320, 64), (448, 128)])
@pytest.mark.parametrize("k", [1, 3])
def test_more_than_256_input_channels(ops, cin, cmid, k, dt):
    """cin > 256 takes the instantiation in which a wave owns up to four 32-column blocks of dx (blocks wave, wave + 4, wave + 8,
    wave + 12) behind the `blk < nblk` guard: 10 blocks end the third round at wave 1, 14 the fourth. Every block is compared."""
    classes = None if k == 1 else (0, -1, 2)
    nblk = cin // 32
    assert nblk in (10, 14) and nblk > 8
    out, ref, live = _against_float64(ops, 3, cin, cmid, k, dt, classes, name="NB=4")
    top = float(ref["dx"].abs().max())
    worst = 0.0
    for b in range(nblk):
        blk = ref["dx"][..., b * 32:(b + 1) * 32]
        assert float(blk.abs().max()) > 0.05 * top, f"on the reference: column block {b} of dx must not be (all but) zero"
        err = float((out["dx"][..., b * 32:(b + 1) * 32].double().cpu() - blk).abs().max()) / top
        worst = max(worst, err)
        assert err <= 2e-3, f"dx column block {b}: {err:.3e}"
    print(f"  worst of the {nblk} column blocks of dx: {worst:.2e}")
    stored = _run(ops, 3, cin, cmid, k, dt, classes)
    assert stored["dx"].dtype == dt and torch.equal(stored["dx"], out["dx"].to(dt))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin,cmid", [(192, 320), (64, 64)])
def test_six_column_blocks_and_odd_chunk_counts(ops, cin, cmid, dt):
    """cin 192: 6 blocks of dx, waves 0 and 1 own two, waves 2 and 3 one. cmid 320 is five chunks, 64 a single one."""
    assert (cmid // 64) % 2 == 1
    _against_float64(ops, 3, cin, cmid, 3, dt, (0, -1, 2), name="chunks")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("s", [8, 9, 11, 13])
def test_every_side_the_trainer_accepts(ops, s, dt):
    """A 64-row tile reaches at most two RoIs: at s = 8 exactly one; at 9, 11 and 13 (81, 121 and 169 rows per RoI) the boundary falls
    on a different row of every tile. Class 3 == num_rows has no predictor row."""
    r, c, k, classes = 5, 64, 3, (0, -1, 2, 3, 1)
    assert _live(classes, k, r) == (True, False, True, False, True)
    offsets = {(i * s * s) % 64 for i in range(r)}
    assert offsets == {0} if s == 8 else len(offsets) == r, "where in its tile a RoI begins"
    out, ref, live = _against_float64(ops, r, c, c, k, dt, classes, s=s, name="side")
    stored = _run(ops, r, c, c, k, dt, classes, s=s)
    assert stored["dx"].dtype == dt and torch.equal(stored["dx"], out["dx"].to(dt))
    for n in ("d_pred_w", "d_pred_b", "d_deconv_b"):
        assert torch.equal(stored[n], out[n]), n
    if s == 8:  # two segments of three with rows_valid (2, 1): RoIs 2, 4 and 5 do not exist
        classes6 = (0, 2, 1, 3, 1, 0)
        assert _live(classes6, k, 6, (2, 1), 3) == (True, True, False, False, False, False)
        _against_float64(ops, 6, c, c, k, dt, classes6, (2, 1), 3, s=s, name="side, segments")


def _many_classes():
    classes = [(i * 13) % 80 for i in range(40)]
    classes[5], classes[9], classes[20], classes[31], classes[39] = -1, 80, classes[3], classes[3], 79
    return tuple(classes)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_many_tiles_rois_and_classes(ops, dt):
    """40 RoIs as two segments of 20 with rows_valid (17, 20), 80 predictor rows: 7840 rows, 123 tiles. mask_bwd_bias_reduce's 16
    threads per column walk 7 or 8 tiles each, mask_bwd_class_reduce has 80 x 64 + 80 outputs (21 workgroups) over 40 RoIs, and every
    RoI spreads over four or five tiles."""
    r, c, k, classes = 40, 64, 80, _many_classes()
    live = _live(classes, k, r, (17, 20), 20)
    assert sum(live) == 35 and not any(live[i] for i in (5, 9, 17, 18, 19)) and -1 in classes and 80 in classes and 0 in classes and 79 in classes
    assert sum(1 for i in range(r) if live[i] and classes[i] == classes[3]) == 3, "a predictor row that several RoIs share"
    assert (r * S * S + 63) // 64 == 123
    out, ref, _ = _against_float64(ops, r, c, c, k, dt, classes, (17, 20), 20, name="many")
    used = sorted({classes[i] for i in range(r) if live[i]})
    unused = [j for j in range(k) if j not in used]
    assert torch.equal(out["d_pred_w"][unused], torch.zeros_like(out["d_pred_w"][unused])) and float(out["d_pred_b"][unused].abs().max()) == 0.0
    assert all(float(ref["d_pred_w"][j].abs().max()) > 0 for j in used)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_without_the_activation_gradient(ops, dt):
    """want_g=False (a null g_out) changes nothing else. RoI 1 has class -1 and holds a whole tile (rows 256 .. 319 of 196 .. 391), so
    the zero path runs without g as well."""
    r, cin, cmid, k, classes = 3, 64, 128, 3, (0, -1, 2)
    assert S * S <= 4 * 64 and 5 * 64 <= 2 * S * S
    full = _run(ops, r, cin, cmid, k, dt, classes)
    lean = _run(ops, r, cin, cmid, k, dt, classes, want_g=False)
    assert lean["g"] is None
    for n in ("dx", "d_pred_w", "d_pred_b", "d_deconv_b"):
        assert torch.equal(lean[n], full[n]), n
    assert float(full["dx"][1].abs().max()) == 0.0 and float(full["dx"][0].abs().max()) > 0.0


def _bwd_lds(cin, cmid, planes):
    """csrc/osr_mask_train.hip mask_bwd_lds: the x tile, the planes' four taps of g, three column sums per tap, d_logits per (tap, row)."""
    return 64 * (cin * 2 + 16) + planes * 4 * 64 * (64 * 2 + 16) + 4 * 3 * cmid * 4 + 4 * 64 * 4


BWD_MAX_LDS = 160 * 1024 - 1024


@pytest.mark.parametrize("dt,cin,cmid", [(torch.bfloat16, 448, 640), (torch.float16, 448, 1408), (torch.float16, 512, 64), (torch.bfloat16, 512, 64)])
def test_tiles_that_do_not_fit_are_refused(osr, ops, dt, cin, cmid):
    """bf16 keeps two planes of g in LDS, fp16 one: at cin 448 the first cmid that does not fit is 640 and 1408; cin 512 is refused
    whatever cmid. OSR_ERR_UNSUPPORTED with nothing launched: the four caller-owned outputs keep their sentinels."""
    import ctypes as C
    planes = 2 if dt == torch.bfloat16 else 1
    if cin == 448:
        assert _bwd_lds(cin, cmid - 64, planes) <= BWD_MAX_LDS < _bwd_lds(cin, cmid, planes)
    L, lib = osr._lib, osr._lib.load()
    r, s, k = 1, 8, 1
    x = torch.zeros(r, s, s, cin, dtype=dt, device=DEV)
    wp, wt = torch.zeros(4 * cin * cmid, dtype=dt, device=DEV), torch.zeros(4 * cin * cmid, dtype=dt, device=DEV)
    b, pw, dl = torch.zeros(cmid, device=DEV), torch.zeros(k, cmid, device=DEV), torch.zeros(r, 2 * s, 2 * s, device=DEV)
    outs = dict(dx=torch.full((r, s, s, cin), -7.0, dtype=dt, device=DEV), d_pred_w=torch.full((k, cmid), -7.0, device=DEV),
                d_pred_b=torch.full((k,), -7.0, device=DEV), d_deconv_b=torch.full((cmid,), -7.0, device=DEV))
    wsb = lib.osr_mask_upsample_predict_bwd_workspace_bytes(r, s, cmid)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    code = ops.dtype_code(dt)
    st = lib.osr_mask_upsample_predict_bwd(p_(x), code, r, s, cin, cmid, p_(wp), p_(wt), p_(b), p_(pw), k, None, None, 0, p_(dl), p_(outs["dx"]), code, None,
                                           p_(outs["d_pred_w"]), p_(outs["d_pred_b"]), p_(outs["d_deconv_b"]), p_(ws), wsb, None)
    torch.cuda.synchronize()
    assert st == L.ERR_UNSUPPORTED and (b"does not fit" if cin == 448 else b"at most 448") in lib.osr_last_error()
    for n, t in outs.items():
        assert bool((t == -7.0).all()), f"{n} was written"


def test_the_largest_tile_that_fits(ops):
    """bf16 at cin 448, cmid 576: 160 768 bytes of dynamic LDS, the most the kernel ever asks for (fp16 reaches it at cmid 1344)."""
    assert _bwd_lds(448, 576, 2) == _bwd_lds(448, 1344, 1) == 160768 <= BWD_MAX_LDS < 160768 + 48 * 64
    _against_float64(ops, 1, 448, 576, 3, torch.bfloat16, (2,), name="largest LDS")


def test_one_rule_for_the_rows_that_count(ops):
    """The forward's logits, the loss, its gradient and the tail's backward on the same (classes, rows_valid, seg_rows, num_rows): the
    rows each treats as live are the same set, and it is mt_row_class's (class -1, class == num_rows and a row beyond its segment's
    count are not)."""
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    r, s, c, k, dt = 6, 8, 64, 3, torch.float16
    classes, rv, seg = (0, -1, 3, 2, 1, 0), (3, 2), 3
    want = list(_live(classes, k, r, rv, seg))
    assert want == [True, False, False, True, True, False]
    x, w, b, pw, pb, dl = _operands(r, c, c, k, dt, s)
    cl, rvd = torch.tensor(classes, dtype=torch.int64, device=DEV), torch.tensor(rv, dtype=torch.int32, device=DEV)
    wp, wt = pack_deconv_weight(w, dt).to(DEV), pack_deconv_weight(w.transpose(0, 1), dt).to(DEV)
    nonzero = lambda t: [bool(v) for v in (t.reshape(r, -1) != 0).any(dim=1).cpu()]  # noqa: E731
    logits = ops.mask_upsample_logits(x.to(DEV), wp, b.to(DEV), pw.to(DEV), pb.to(DEV), cl, rvd, seg)
    assert nonzero(logits) == want, "forward"
    # the loss reads arbitrary logits, so that a row's zeros are the loss's own doing
    g = torch.Generator().manual_seed(3)
    lg = torch.randn(r, 2 * s, 2 * s, generator=g).to(DEV)
    tg = (torch.rand(r, 2 * s, 2 * s, generator=g) < 0.4).to(torch.uint8).to(DEV)
    assert float(ops.mask_loss_fwd(lg, tg, k, cl, rvd, seg)[1]) == float(sum(want))
    entered = []
    for i in range(r):  # row i alone: every other row gets class -1
        only = torch.full((r,), -1, dtype=torch.int64)
        only[i] = classes[i]
        entered.append(float(ops.mask_loss_fwd(lg, tg, k, only.to(DEV), rvd, seg)[1]) == 1.0)
    assert entered == want, "loss"
    d_logits = ops.mask_loss_bwd(lg, tg, k, cl, rvd, seg, scale=64.0)
    assert nonzero(d_logits) == want, "loss gradient"
    out = ops.mask_upsample_predict_bwd(x.to(DEV), wp, wt, b.to(DEV), pw.to(DEV), dl.to(DEV), cl, rvd, seg)
    assert nonzero(out["dx"]) == want and nonzero(out["g"].view(4, r, -1).transpose(0, 1)) == want, "backward"


def test_shape_rules(osr, ops):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb, dl = _operands(1, 64, 128, 3, torch.float16)
    wp, wt = pack_deconv_weight(w, torch.float16).to(DEV), pack_deconv_weight(w.transpose(0, 1), torch.float16).to(DEV)
    with pytest.raises(osr.OsrError, match="classes"):
        ops.mask_upsample_predict_bwd(x.to(DEV), wp, wt, b.to(DEV), pw.to(DEV), dl.to(DEV), None)
    xs = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(osr.OsrError, match="s >= 8"):
        ops.mask_upsample_predict_bwd(xs, wp, wt, b.to(DEV), pw.to(DEV), torch.zeros(1, 8, 8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
