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
has an empty segment, a RoI that does not exist and one with class -1."""
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
def _operands(r: int, cin: int, cmid: int, k: int, dt: torch.dtype):
    g = torch.Generator().manual_seed(1000 * r + cin + k)
    x = torch.randn(r, S, S, cin, generator=g).to(dt)
    w = (torch.randn(cin, cmid, 2, 2, generator=g) * (2.0 / cin) ** 0.5).to(dt)
    b = torch.randn(cmid, generator=g) * 0.1
    pw = torch.randn(k, cmid, generator=g) * (2.0 / cmid) ** 0.5
    pb = torch.randn(k, generator=g) * 0.1
    dl = torch.randn(r, 2 * S, 2 * S, generator=g)
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
    idx = torch.zeros(x.shape[0], dtype=torch.int64) if classes is None else classes.clamp(min=0)
    z = z[torch.arange(x.shape[0]), idx]
    keep = live.to(dtype)[:, None, None]
    (z * dl.to(dtype) * keep).sum().backward()
    grads = dict(dx=xx.grad.permute(0, 2, 3, 1), dw=ww.grad, d_deconv_b=bb.grad, d_pred_w=pww.grad, d_pred_b=pbb.grad)
    return (z * keep).detach(), grads, frac


@functools.lru_cache(maxsize=None)
def _reference(r, cin, cmid, k, dt, classes_key, live_key):
    o = _operands(r, cin, cmid, k, dt)
    classes = None if classes_key is None else torch.tensor(classes_key, dtype=torch.int64)
    live = torch.tensor(live_key, dtype=torch.bool)
    z, ref, frac = _autograd(*o, classes, live, torch.float64)
    _, g32, _ = _autograd(*o, classes, live, torch.float32)
    e32 = {n: float((g32[n].double() - ref[n]).abs().max() / ref[n].abs().max().clamp(min=1e-30)) for n in ("d_pred_w", "d_pred_b", "d_deconv_b")}
    return z, ref, e32, frac


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _run(ops, r, cin, cmid, k, dt, classes, rows_valid=None, seg_rows=0, dx_dtype=None):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb, dl = _operands(r, cin, cmid, k, dt)
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int64, device=DEV)
    rv = None if rows_valid is None else torch.tensor(rows_valid, dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    out = ops.mask_upsample_predict_bwd(xd, pack_deconv_weight(w, dt).to(DEV), pack_deconv_weight(w.transpose(0, 1), dt).to(DEV), b.to(DEV),
                                        pw.to(DEV), dl.to(DEV), cl, rv, seg_rows, dx_dtype=dx_dtype)
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


def test_shape_rules(osr, ops):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    x, w, b, pw, pb, dl = _operands(1, 64, 128, 3, torch.float16)
    wp, wt = pack_deconv_weight(w, torch.float16).to(DEV), pack_deconv_weight(w.transpose(0, 1), torch.float16).to(DEV)
    with pytest.raises(osr.OsrError, match="classes"):
        ops.mask_upsample_predict_bwd(x.to(DEV), wp, wt, b.to(DEV), pw.to(DEV), dl.to(DEV), None)
    xs = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(osr.OsrError, match="s >= 8"):
        ops.mask_upsample_predict_bwd(xs, wp, wt, b.to(DEV), pw.to(DEV), torch.zeros(1, 8, 8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
