"""The dense layers' backward kernels at the training step's own layer shapes (res2-res5, FPN, box head, RPN conv), against explicit
fp64 restatements (per-tap shifted-view GEMMs in torch.float64 on the GPU; never a torch fp16 / fp32 convolution).

Layer table: `backward_table` lists every dense backward launch of OpensetRCNNTrainer._backward / _backward_trunk (ops.conv2d_dgrad,
ops.conv2d_wgrad, ops.bias_grad) in the trainer's order, for batch 16 at 800 x 1344 (configs 3 / 5) and batch 8 at 768 x 1344 (config 4
per rank). test_table_is_the_trainers_backward records one real trainer step per geometry at FREEZE_AT 0 and 2 and requires the table,
so it cannot drift from the trainer. Every launch runs under ops.concurrent_streams(2), as step() does.

Paths reached (test_plans_reached asserts them from osr_conv2d_fwd_describe / osr_conv2d_wgrad_workspace_bytes):
- data gradients (osr_conv2d_fwd / osr_conv2d_fwd_masked on flipped weights): the 256 x 256 8-phase tile (FC1, fpn_output2-4, res4
  conv2, res5 conv2 / conv3 / first shortcut; fpn_output2 with a split-K tail launch and its reduction), 128 x 128 double buffer (FC2),
  128 x 64 double buffer (fpn_output5), 128 x 64 single buffer (res2's launches with 64 output channels: conv2, conv3, the first block's
  conv1 with one K slice and its shortcut), 128 x 128 single buffer (the rest); epilogues add (res_mode 1), mask (res_mode 3),
  post_mask, add + post_mask, the strided 1 x 1 writes with and without strided_only;
- weight gradients (osr_conv2d_wgrad): 256^2 8-phase (fpn_lateral2, fpn_output2-4, res4 conv2), 256^2 one-barrier (the other laterals,
  fpn_output5, res4 / res5 1 x 1, res5 conv2, FC2, the sparse RPN rows),
  128^2 (res2 / res3 128- and 64-wide layers, cin = 64 in a half-empty ci tile, up to 382 splits: an uneven XCD remap), the direct
  one-split path (FC1), wgrad_reduce_kernel behind every other one, accumulate=True over the five RPN levels (sparse_rpn_bwd=False);
- osr_bias_grad at every layer's rows; pool_bwd modes 0 and 1 at the FPN's shapes.

At batch 16, res5 and p5 have M = 16 800 = 262.5 x 64 rows: their weight gradients end in a ragged 64-row step at production.

Exact runs: x, dy, the weights, addends and biases hold small integers (|v| <= 2, zeros mixed in). Every product is exact and every
fp32 partial sum stays below 2^24, so the kernels must equal the fp64 reference BIT FOR BIT, over the whole tensor: one dropped,
duplicated or misaddressed row, split, tap or tile is a nonzero integer. "Hot" blocks of positive values push data-gradient results
past 2048 (fp16) / 256 (bf16), where odd integers round to even as torch's .half() / .bfloat16() do; a scaled case (weights x 64)
goes past 65504 and must give +-Inf, not a saturated value (the loss-scale overflow skip depends on that Inf). Masks are ReLU outputs
with exact +0.0 and -0.0 (> 0 keeps).
Float runs: random data; elementwise error against the fp64 result, bound (chain + 2) * 2^-24 * sum|terms| (+ half an ulp of a 16-bit
output), sum|terms| being the same fp64 restatement on |operands|.
Edges off the production shapes: M not a multiple of 64 (n = 1 and 3 at odd h * w: ragged last step and last M tile), last split shorter,
wgrad grids that are not a multiple of 8, cin = 64 on the 128^2 tile, the direct path with a ragged step, osr_bias_grad with fewer rows
than one block and with rows per block = 24..31 mod 32 (the unrolled loop's last turn ends exactly at the block's end), Inf / NaN in dy
(dw stays non-finite on both tiles, check_finite_ clears the flag, the other output channels stay finite)."""
import ctypes as C
import inspect
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
GEOMS = {"b16_800x1344": (16, 800, 1344), "b8_768x1344": (8, 768, 1344)}
R50 = ((2, 3, 64, 256), (3, 4, 128, 512), (4, 6, 256, 1024), (5, 3, 512, 2048))  # stage, blocks, bottleneck width, output channels
RPN_BATCH, ROIS = 256, 512  # rpn_batch_size, roi_batch_size of the engine's defaults


def stage_hw(H, W):
    """(h, w) of res2..res5 (= p2..p5) and p6 for a padded H x W batch (engine.pyramid_shapes)."""
    h, w = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    out = {}
    for s in (2, 3, 4, 5, 6):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out[s] = (h, w)
    return out


def _epi(mask=False, add=False, post_mask=False, strided_only=False):
    return "+".join(k for k, v in (("mask", mask), ("add", add), ("post_mask", post_mask), ("strided_only", strided_only)) if v) or "-"


def DG(name, dy, w, x_hw, stride, pad, epi, dt):
    return ("dgrad", name, (tuple(dy), tuple(w), tuple(x_hw), stride, pad, epi, dt))


def WG(name, x, dy, k, stride, pad, dt, acc=False):
    return ("wgrad", name, (tuple(x), tuple(dy), k, k, stride, pad, acc, dt))


def BG(name, dy, dt, acc=False):
    return ("bias", name, (tuple(dy), acc, dt))


def backward_table(n, H, W, freeze_at=0, dt=F16):
    """Every dense backward launch of one trainer step (sparse_rpn_bwd=True), in the trainer's order: (kind, layer, signature)."""
    hw = stage_hw(H, W)
    T = []
    cap, m = n * 2 * RPN_BATCH, n * ROIS
    rn = "proposal_generator.rpn_head.conv"
    T += [WG(rn, (1, cap, 1, 9 * 256), (1, cap, 1, 256), 1, 1, 0, dt), BG(rn, (cap, 256), dt)]  # the sparse row list's im2col rows
    T += [DG("fc2", (1, m, 1, 1024), (1024, 1, 1, 1024), (m, 1), 1, 0, _epi(mask=True), dt),
          WG("fc2", (1, m, 1, 1024), (1, m, 1, 1024), 1, 1, 0, dt), BG("fc2", (m, 1024), dt),
          DG("fc1", (1, m, 1, 1024), (12544, 1, 1, 1024), (m, 1), 1, 0, _epi(), dt),
          WG("fc1", (1, m, 1, 12544), (1, m, 1, 1024), 1, 1, 0, dt), BG("fc1", (m, 1024), dt)]
    for lvl in (2, 3, 4, 5):
        h, w = hw[lvl]
        c = R50[lvl - 2][3]
        on, ln = f"backbone.fpn_output{lvl}", f"backbone.fpn_lateral{lvl}"
        T += [DG(on, (n, h, w, 256), (256, 3, 3, 256), (h, w), 1, 1, _epi(add=lvl > 2), dt),
              WG(on, (n, h, w, 256), (n, h, w, 256), 3, 1, 1, dt), BG(on, (n, h, w, 256), dt),
              WG(ln, (n, h, w, c), (n, h, w, 256), 1, 1, 0, dt), BG(ln, (n, h, w, 256), dt)]
    blocks = []
    cin = 64
    for stage, nb, mid, cout in R50:
        hy, wy = hw[stage]
        for b in range(nb):
            stride = 2 if b == 0 and stage > 2 else 1
            hx, wx = (hw[stage - 1] if stride == 2 else hw[stage])
            blocks.append((stage, b, nb, cin, mid, cout, stride, hx, wx, hy, wy))
            cin = cout
    G = False  # a gradient w.r.t. the block's output exists
    for stage, b, nb, cin, mid, cout, stride, hx, wx, hy, wy in reversed(blocks):
        if stage <= freeze_at:
            break
        pre = f"backbone.bottom_up.res{stage}.{b}"
        first = b == 0
        if b == nb - 1:
            T.append(DG(f"backbone.fpn_lateral{stage}", (n, hy, wy, 256), (cout, 1, 1, 256), (hy, wy), 1, 0, _epi(add=G, post_mask=True), dt))
            G = True
        T += [DG(pre + ".conv3", (n, hy, wy, cout), (mid, 1, 1, cout), (hy, wy), 1, 0, _epi(mask=True), dt),
              WG(pre + ".conv3", (n, hy, wy, mid), (n, hy, wy, cout), 1, 1, 0, dt),
              DG(pre + ".conv2", (n, hy, wy, mid), (mid, 3, 3, mid), (hy, wy), 1, 1, _epi(mask=True), dt),
              WG(pre + ".conv2", (n, hy, wy, mid), (n, hy, wy, mid), 3, 1, 1, dt),
              WG(pre + ".conv1", (n, hx, wx, cin), (n, hy, wy, mid), 1, stride, 0, dt)]
        if first:
            T.append(WG(pre + ".shortcut", (n, hx, wx, cin), (n, hy, wy, cout), 1, stride, 0, dt))
            if stage == freeze_at + 1:
                break
        pm = not (first and stage > 2)  # the block below is the last of its stage: the lateral's launch masks its G
        if first:
            T += [DG(pre + ".conv1", (n, hy, wy, mid), (cin, 1, 1, mid), (hx, wx), stride, 0, _epi(strided_only=stride > 1), dt),
                  DG(pre + ".shortcut", (n, hy, wy, cout), (cin, 1, 1, cout), (hx, wx), stride, 0, _epi(add=True, post_mask=pm), dt)]
        else:
            T.append(DG(pre + ".conv1", (n, hy, wy, mid), (cin, 1, 1, mid), (hx, wx), 1, 0, _epi(add=True, post_mask=pm), dt))
    return T


def dense_rpn_entries(n, H, W, dt=F16):
    """sparse_rpn_bwd=False: the RPN conv's weight and bias gradients accumulated over p2..p6 (one entry: run in sequence)."""
    hw = stage_hw(H, W)
    return [("rpn_dense", "proposal_generator.rpn_head.conv", (tuple((n,) + hw[s] + (256,) for s in (2, 3, 4, 5, 6)), dt))]


def _unique(table):
    seen, out = set(), []
    for e in table:
        if (e[0], e[2]) not in seen:
            seen.add((e[0], e[2]))
            out.append(e)
    return out


def _cases(geoms, dt=F16):
    out = []
    for gname in geoms:
        n, H, W = GEOMS[gname]
        for e in _unique(backward_table(n, H, W, 0, dt)) + dense_rpn_entries(n, H, W, dt):
            out.append(pytest.param(e, id=f"{gname}-{e[0]}-{e[1].replace('backbone.', '').replace('bottom_up.', '')}"))
    return out


# a bf16 subset: one launch per plan
BF16_LAYERS = {("dgrad", "backbone.fpn_output2"), ("dgrad", "backbone.fpn_output5"), ("dgrad", "backbone.bottom_up.res2.1.conv2"),
               ("dgrad", "backbone.bottom_up.res3.0.shortcut"), ("dgrad", "backbone.bottom_up.res4.0.conv1"),
               ("wgrad", "backbone.fpn_output2"), ("wgrad", "backbone.fpn_lateral3"), ("wgrad", "backbone.bottom_up.res2.1.conv2"),
               ("wgrad", "fc1"), ("bias", "backbone.fpn_output2")}


def _bf16_cases():
    n, H, W = GEOMS["b16_800x1344"]
    return [pytest.param(e, id=f"b16_800x1344-bf16-{e[0]}-{e[1].replace('backbone.', '').replace('bottom_up.', '')}")
            for e in _unique(backward_table(n, H, W, 0, BF16)) if (e[0], e[1]) in BF16_LAYERS]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def _report(name, err, tol):
    """Prints the observed error next to its bound (pytest -s shows it) and checks it."""
    print(f"[err] {name}: {err:.3e} (tol {tol:.1e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.1e}"


# ------------------------------------------------------------------------------------------------------------------------------
# fp64 restatements (NHWC, weights (cout, kh, kw, cin)); exact for integer data
# ------------------------------------------------------------------------------------------------------------------------------
def dgrad_ref(dy, w, x_hw, stride, pad):
    """dx (n, hi, wi, cin) fp64 of y = conv(x, w, stride, pad): per tap one GEMM dy @ w[:, a, b, :], scattered to its shifted view."""
    n, ho, wo, co = dy.shape
    _, kh, kw, ci = w.shape
    hi, wi = x_hw
    dy2 = dy.reshape(-1, co).double()
    hp, wp = max(hi + 2 * pad, stride * (ho - 1) + kh), max(wi + 2 * pad, stride * (wo - 1) + kw)
    out = torch.zeros((n, hp, wp, ci), dtype=torch.float64, device=dy.device)
    for a in range(kh):
        for b in range(kw):
            out[:, a:a + stride * (ho - 1) + 1:stride, b:b + stride * (wo - 1) + 1:stride] += (dy2 @ w[:, a, b, :].double()).view(n, ho, wo, ci)
    return out[:, pad:pad + hi, pad:pad + wi]


def wgrad_ref(x, dy, kh, kw, stride, pad):
    """dw (cout, kh, kw, cin) fp64: per tap dy^T @ (the shifted, strided view of the zero-padded x)."""
    n, hi, wi, ci = x.shape
    _, ho, wo, co = dy.shape
    xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
    dyT = dy.reshape(-1, co).double().t()
    dw = torch.empty((co, kh, kw, ci), dtype=torch.float64, device=x.device)
    for a in range(kh):
        for b in range(kw):
            dw[:, a, b, :] = dyT @ xp[:, a:a + stride * (ho - 1) + 1:stride, b:b + stride * (wo - 1) + 1:stride].reshape(-1, ci)
    return dw


def _ints(shape, g, dt, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).to(dt)


def _relu_out(shape, g, dt):
    """A ReLU output: +0.0, -0.0 and positive integers, a quarter each of the zeros, half positive."""
    k = torch.randint(0, 4, shape, generator=g, device=DEV)
    v = torch.randint(1, 4, shape, generator=g, device=DEV).to(dt)
    v[k == 0] = 0.0
    v[k == 1] = -0.0
    return v


def _hot(shape, g, dt, region):
    """Integers in {-2..2}; the block `region` (an index tuple) holds positives in {1, 2}: results there sum many same-signed terms."""
    t = _ints(shape, g, dt)
    sub = t[region]
    sub.copy_(torch.randint(1, 3, sub.shape, generator=g, device=DEV).to(dt))
    return t


def _dgrad_inputs(sig, g, exact=True, scale=1.0):
    dyshape, wshape, x_hw, stride, pad, epi, dt = sig
    n, ho, wo, co = dyshape
    ci = wshape[0]
    kh, kw = wshape[1], wshape[2]
    fshape = (co, kh, kw, ci)  # forward weight
    if exact:
        dy = _hot(dyshape, g, dt, (slice(0, 1), slice(0, 4)))                 # image 0, pixel rows 0..3
        w = _hot(fshape, g, dt, (slice(None), slice(None), slice(None), slice(0, 16))) * scale  # input channels 0..15
        add = _ints((n,) + tuple(x_hw) + (ci,), g, dt) if "add" in epi else None
    else:
        dy = torch.randn(dyshape, generator=g, device=DEV).to(dt)
        w = (torch.randn(fshape, generator=g, device=DEV) / (co * kh * kw) ** 0.5).to(dt)
        add = torch.randn((n,) + tuple(x_hw) + (ci,), generator=g, device=DEV).to(dt) if "add" in epi else None
    aux = (n,) + tuple(x_hw) + (ci,)
    mask = _relu_out(aux, g, dt) if "mask" in epi.split("+") else None
    post = _relu_out(aux, g, dt) if "post_mask" in epi else None
    return dy, w.to(dt), add, mask, post


def _run_dgrad(ops, sig, dy, w, add, mask, post):
    _, _, x_hw, stride, pad, epi, dt = sig
    with ops.concurrent_streams(2):
        wd = ops.pack_dgrad_weight(w)
        return ops.conv2d_dgrad(dy, wd, x_hw, stride, pad, mask=mask, add=add, post_mask=post, strided_only="strided_only" in epi)


def _dgrad_expect(sig, dy, w, add, mask, post, absolute=False):
    """fp64 result of the launch (conv + add at the written pixels, masks, zeros at the pixels a stride skips) and the pixels compared."""
    _, _, x_hw, stride, pad, epi, dt = sig
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    v = dgrad_ref(f(dy), f(w), x_hw, stride, pad)
    if add is not None:
        if stride > 1:
            v[:, ::stride, ::stride] += f(add[:, ::stride, ::stride]).double()
        else:
            v += f(add).double()
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    if post is not None:
        v = torch.where(post > 0, v, torch.zeros_like(v))
    sel = (slice(None), slice(None, None, stride), slice(None, None, stride)) if "strided_only" in epi else (slice(None),)
    return v, sel


def _exact_dgrad(ops, sig, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dy, w, add, mask, post = _dgrad_inputs(sig, g, True, scale)
    got = _run_dgrad(ops, sig, dy, w, add, mask, post)
    ref64, sel = _dgrad_expect(sig, dy, w, add, mask, post)
    assert ref64.abs().max().item() < 2 ** 24
    ref = ref64.to(sig[-1])
    torch.cuda.synchronize()
    got, ref, ref64 = got[sel], ref[sel], ref64[sel]
    if not torch.equal(got, ref):
        bad = (got.double() != ref.double()) & ~(got.isnan() & ref.isnan())
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{bad.sum().item()} of {got.numel()} elements differ; first at {i}: got {got[tuple(i)].item()} "
                             f"ref {ref[tuple(i)].item()} (fp64 {ref64[tuple(i)].item()})")
    return ref64


def _exact_wgrad(ops, x, dy, k, stride, pad, acc_init=None):
    with ops.concurrent_streams(2):
        dw = None if acc_init is None else acc_init.clone()
        dw = ops.conv2d_wgrad(x, dy, k, k, stride, pad, dw=dw, accumulate=acc_init is not None)
    ref = wgrad_ref(x, dy, k, k, stride, pad)
    if acc_init is not None:
        ref += acc_init.double()
    torch.cuda.synchronize()
    assert ref.abs().max().item() < 2 ** 24
    if not torch.equal(dw, ref.float()):
        bad = dw.double() != ref
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"dw: {bad.sum().item()} of {dw.numel()} elements differ; first at {i}: got {dw[tuple(i)].item()} ref {ref[tuple(i)].item()}")
    return dw


def _exact_bias(ops, dy, acc_init=None):
    with ops.concurrent_streams(2):
        db = ops.bias_grad(dy, None if acc_init is None else acc_init.clone(), accumulate=acc_init is not None)
    ref = dy.reshape(-1, dy.shape[-1]).double().sum(0)
    if acc_init is not None:
        ref += acc_init.double()
    torch.cuda.synchronize()
    assert torch.equal(db, ref.float()), f"db: max |diff| {(db.double() - ref).abs().max().item()}"


def _padded(shape, g, dt, fill=7.0):
    """Integer tensor whose allocation continues with 32 rows of `fill` (a read past the end lands on nonzero values)."""
    rows = 1
    for s in shape[:-1]:
        rows *= s
    buf = torch.full((rows + 32, shape[-1]), fill, dtype=dt, device=DEV)
    buf[:rows] = _ints((rows, shape[-1]), g, dt)
    return buf[:rows].view(shape)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the table against the trainer
# ------------------------------------------------------------------------------------------------------------------------------
def _step_args(tr, n, H, W):
    g = torch.Generator().manual_seed(n + H)
    images = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)
    ngt = 6
    ctr = torch.rand(n, ngt, 2, generator=g) * torch.tensor([W * 0.8, H * 0.8]) + 40
    size = torch.rand(n, ngt, 2, generator=g) * 300 + 32
    gt = torch.cat((ctr - size / 2, ctr + size / 2), dim=2)
    gt[..., 0::2].clamp_(0, W)
    gt[..., 1::2].clamp_(0, H)
    gcls = torch.randint(1, 20, (n, ngt), generator=g)
    shapes = tr.eng.pyramid_shapes(H, W)
    r = sum(a * b for a, b in shapes)
    cap = sum(min(2000, a * b) for a, b in shapes)
    keys = {k: torch.rand(sz, generator=g).to(DEV) for k, sz in (("rpn_reg", (n, r)), ("rpn_obj", (n, r)), ("roi", (n, cap + ngt)))}
    return (images.to(DEV), torch.tensor([(H, W)] * n, dtype=torch.int32).to(DEV), H, W, gt.to(DEV), gcls.to(DEV),
            torch.full((n,), ngt, dtype=torch.int32).to(DEV), keys)


def test_table_is_the_trainers_backward(ops):
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params

    real = dict(dgrad=ops.conv2d_dgrad, wgrad=ops.conv2d_wgrad, bias=ops.bias_grad)
    sigs = {k: inspect.signature(f) for k, f in real.items()}
    log = []

    def rec(kind):
        def f(*a, **k):
            b = sigs[kind].bind(*a, **k)
            b.apply_defaults()
            v = b.arguments
            if kind == "dgrad":
                epi = _epi(v["mask"] is not None, v["add"] is not None, v["post_mask"] is not None, v["strided_only"])
                s = (tuple(v["dy"].shape), tuple(v["w_dgrad"].shape), tuple(v["x_hw"]), v["stride"], v["pad"], epi, v["dy"].dtype)
                assert v["out_dtype"] in (None, v["dy"].dtype)
            elif kind == "wgrad":
                s = (tuple(v["x"].shape), tuple(v["dy"].shape), v["kh"], v["kw"], v["stride"], v["pad"], bool(v["accumulate"]), v["x"].dtype)
            else:
                s = (tuple(v["dy"].shape), bool(v["accumulate"]), v["dy"].dtype)
            log.append((kind, s, ops._CONCURRENCY[0]))
            return real[kind](*a, **k)
        return f

    params = random_params(0)
    for gname, (n, H, W) in GEOMS.items():
        for fz in (0, 2):
            tr = OpensetRCNNTrainer(params, dtype=F16, device=DEV, lr=1e-4, loss_scale=1024.0, freeze_at=fz)
            assert tr.sparse_rpn_bwd and tr.backward_concurrency_hint == 2
            args = _step_args(tr, n, H, W)
            log.clear()
            ops.conv2d_dgrad, ops.conv2d_wgrad, ops.bias_grad = rec("dgrad"), rec("wgrad"), rec("bias")
            try:
                tr.step(*args)
                torch.cuda.synchronize()
            finally:
                ops.conv2d_dgrad, ops.conv2d_wgrad, ops.bias_grad = real["dgrad"], real["wgrad"], real["bias"]
            want = backward_table(n, H, W, fz)
            # (the fp32 heads' bias gradients -- cls / dec / enc / pred, _f32_linear_bwd -- are not dense-layer launches)
            assert all(k == "bias" for k, s, _ in log if s[-1] == torch.float32)
            log[:] = [r for r in log if r[1][-1] != torch.float32]
            got = [(k, s) for k, s, _ in log]
            exp = [(k, s) for k, _, s in want]
            for i, (a, b) in enumerate(zip(got, exp)):
                assert a == b, f"{gname} FREEZE_AT {fz}: launch {i} ({want[i][1]}): trainer {a} != table {b}"
            assert len(got) == len(exp), f"{gname} FREEZE_AT {fz}: {len(got)} launches, table {len(exp)}: {got[len(exp):] or exp[len(got):]}"
            assert all(c == 2 for _, _, c in log), "every backward launch runs under concurrent_streams(2)"
            del tr
            torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the plans the table reaches
# ------------------------------------------------------------------------------------------------------------------------------
def dgrad_plan(osr, sig, conc=2):
    """osr_conv2d_fwd_describe of the launch ops.conv2d_dgrad makes for this signature."""
    from openset_rcnn_amd.host import ops
    L = osr._lib
    dyshape, wshape, (hi, wi), stride, pad, epi, dt = sig
    n, ho, wo, co = dyshape
    ci, kh, kw, _ = wshape
    with ops.concurrent_streams(conc):
        if stride == 1:
            p = ops._conv_params(n, ho, wo, co, hi, wi, ci, kh, kw, 1, kh - 1 - pad, dt, dt)
        else:
            p = ops._conv_params(n, ho, wo, co, ho, wo, ci, 1, 1, 1, 0, dt, dt)
            p.out_stride_n, p.out_stride_h, p.out_stride_w = hi * wi * ci, stride * wi * ci, stride * ci
    p.res_mode = 3 if "mask" in epi.split("+") else (1 if "add" in epi else 0)
    ws = int(ops.SPLIT_K_TAIL and "post_mask" not in epi and p.res_mode == 0 and stride == 1 and L.load().osr_conv2d_fwd_workspace_bytes(C.byref(p)) > 0)
    buf = C.create_string_buffer(256)
    L.load().osr_conv2d_fwd_describe(C.byref(p), ws, buf, 256)
    return buf.value.decode()


def wgrad_plan(osr, xshape, dyshape, k, stride, pad, dt=F16, acc=False):
    """(plan name, splits, rows per split, grid) of osr_conv2d_wgrad, from osr_conv2d_wgrad_workspace_bytes and the launcher's arithmetic."""
    from openset_rcnn_amd.host import ops
    L = osr._lib
    n, hi, wi, ci = xshape
    _, ho, wo, co = dyshape
    with ops.concurrent_streams(2):
        p = ops._conv_params(n, hi, wi, ci, ho, wo, co, k, k, stride, pad, dt, dt)
    splits = int(L.load().osr_conv2d_wgrad_workspace_bytes(C.byref(p))) // (co * k * k * ci * 4)
    M = n * ho * wo
    rps = ((M + splits - 1) // splits + 63) // 64 * 64
    splits = (M + rps - 1) // rps
    big = co % 256 == 0 and ci % 256 == 0
    tt = 256 if big else 128
    grid = ((co + tt - 1) // tt) * ((ci + tt - 1) // tt) * k * k * splits
    if splits == 1 and not acc:
        name = "wgrad direct"
    elif big:
        name = "wgrad 256^2 8-phase" if rps // 64 >= 48 else "wgrad 256^2 one-barrier"
    else:
        name = "wgrad 128^2"
    return name, splits, rps, grid


# plan -> layers of the batch-16 table that must take it (the cost model's choice at concurrency 2)
DGRAD_PLANS = {
    "256x256/2": ["fc1", "backbone.fpn_output2", "backbone.fpn_output3", "backbone.fpn_output4", "backbone.bottom_up.res4.1.conv2",
                  "backbone.bottom_up.res5.1.conv2", "backbone.bottom_up.res5.1.conv3", "backbone.bottom_up.res5.0.shortcut"],
    "128x128/2": ["fc2"],
    "128x64/2": ["backbone.fpn_output5"],
    "128x64/1": ["backbone.bottom_up.res2.1.conv2", "backbone.bottom_up.res2.1.conv3", "backbone.bottom_up.res2.0.conv1"],
    "128x128/1": ["backbone.bottom_up.res3.1.conv2", "backbone.bottom_up.res4.1.conv1"],
}
WGRAD_PLANS = {
    "wgrad 256^2 8-phase": ["backbone.fpn_lateral2", "backbone.fpn_output2", "backbone.fpn_output3", "backbone.fpn_output4", "backbone.bottom_up.res4.1.conv2"],
    "wgrad 256^2 one-barrier": ["backbone.fpn_lateral3", "backbone.fpn_lateral4", "backbone.bottom_up.res4.1.conv1", "backbone.bottom_up.res5.1.conv3"],
    "wgrad 128^2": ["backbone.bottom_up.res2.1.conv2", "backbone.bottom_up.res2.0.conv1", "backbone.bottom_up.res3.1.conv2"],
    "wgrad direct": ["fc1"],
}


def test_plans_reached(osr):
    L = osr._lib
    L.load()
    n, H, W = GEOMS["b16_800x1344"]
    table = backward_table(n, H, W, 0)
    dplan = {e[1]: dgrad_plan(osr, e[2]) for e in table if e[0] == "dgrad"}
    wplan = {e[1]: wgrad_plan(osr, e[2][0], e[2][1], e[2][2], e[2][4], e[2][5]) for e in table if e[0] == "wgrad"}
    for name in sorted(dplan):
        print(f"[plan] dgrad {name}: {dplan[name]}")
    for name in sorted(wplan):
        print(f"[plan] {name}: {wplan[name]}")
    for plan, layers in DGRAD_PLANS.items():
        for ly in layers:
            assert dplan[ly].startswith(plan + " "), f"data-gradient plan {plan} is no longer reached by {ly}: {dplan[ly]}"
    for plan, layers in WGRAD_PLANS.items():
        for ly in layers:
            assert wplan[ly][0] == plan, f"weight-gradient plan {plan} is no longer reached by {ly}: {wplan[ly]}"
    # the 128^2 tile with cin = 64 (half-empty ci tile), an uneven XCD remap (grid % 8 != 0), a ragged last split, > 300 splits
    assert wplan["backbone.bottom_up.res2.0.conv1"][0] == "wgrad 128^2"
    assert any(v[3] % 8 != 0 for v in wplan.values()), "no weight-gradient grid of the table is uneven over the 8 XCDs any more"
    assert max(v[1] for v in wplan.values()) >= 300, "no layer of the table runs hundreds of splits any more"
    assert "split-K" in dplan["backbone.fpn_output2"], "fpn_output2's data gradient no longer cuts its last round along K"
    # res5 / p5 (25 x 42 per image): M = 16 800 = 262.5 x 64 -- a ragged last 64-row step at production (p4 and finer: multiples of 64)
    ragged = sorted({e[1] for e in table if e[0] == "wgrad" and (e[2][1][0] * e[2][1][1] * e[2][1][2]) % 64})
    print(f"[plan] wgrad launches with M % 64 != 0: {ragged}")
    assert "backbone.fpn_output5" in ragged and "backbone.bottom_up.res5.1.conv2" in ragged


# ------------------------------------------------------------------------------------------------------------------------------
# 3. exact runs (integer data) at the table's launches
# ------------------------------------------------------------------------------------------------------------------------------
_SEEN_BIG_ODD = {}


def _exact_case(ops, e, seed):
    kind, name, sig = e
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "dgrad":
        ref64 = _exact_dgrad(ops, sig, seed)
        lim = 2048 if sig[-1] == F16 else 256
        big = ref64.abs() > lim
        _SEEN_BIG_ODD[name] = bool((big & (torch.remainder(ref64, 2) == 1)).any())
        K = sig[0][3] * sig[1][1] * sig[1][2]
        if K >= 1024:  # (2.25 K on average in the hot block)
            assert _SEEN_BIG_ODD[name], f"{name}: no odd result above {lim} (the rounding to even is not exercised)"
    elif kind == "wgrad":
        xs, dys, k, _, stride, pad, acc, dt = sig
        _exact_wgrad(ops, _ints(xs, g, dt), _ints(dys, g, dt), k, stride, pad)
        # the same launch accumulating into integers
        co, ci = dys[-1], xs[-1]
        if xs[0] * dys[1] * dys[2] <= 1 << 20:
            _exact_wgrad(ops, _ints(xs, g, dt), _ints(dys, g, dt), k, stride, pad, acc_init=_ints((co, k, k, ci), g, torch.float32))
    elif kind == "bias":
        dys, acc, dt = sig
        _exact_bias(ops, _padded(dys, g, dt))
        _exact_bias(ops, _padded(dys, g, dt), acc_init=_ints((dys[-1],), g, torch.float32))
    else:  # the dense RPN conv: weight and bias gradients accumulated over p2..p6
        shapes, dt = sig
        xs = [_ints(s, g, dt) for s in shapes]
        dys = [_ints(s, g, dt) for s in shapes]
        dw = torch.empty((256, 3, 3, 256), dtype=torch.float32, device=DEV)
        db = torch.empty((256,), dtype=torch.float32, device=DEV)
        with ops.concurrent_streams(2):
            for li, (x, dy) in enumerate(zip(xs, dys)):
                ops.conv2d_wgrad(x, dy, 3, 3, 1, 1, dw=dw, accumulate=li > 0)
                ops.bias_grad(dy, db, accumulate=li > 0)
        ref = sum(wgrad_ref(x, dy, 3, 3, 1, 1) for x, dy in zip(xs, dys))
        rb = sum(dy.reshape(-1, 256).double().sum(0) for dy in dys)
        torch.cuda.synchronize()
        assert torch.equal(dw, ref.float()), f"dw: {(dw.double() != ref).sum().item()} elements differ"
        assert torch.equal(db, rb.float())


@pytest.mark.parametrize("e", _cases(GEOMS))
def test_exact_fp16(ops, e):
    _exact_case(ops, e, 1000 + zlib.crc32(e[1].encode()) % 1000)


@pytest.mark.parametrize("e", _bf16_cases())
def test_exact_bf16(ops, e):
    _exact_case(ops, e, 2000 + zlib.crc32(e[1].encode()) % 1000)


@pytest.mark.parametrize("layer", ["backbone.fpn_output2", "backbone.bottom_up.res2.1.conv2", "backbone.bottom_up.res3.0.shortcut",
                                   "backbone.bottom_up.res5.1.conv3"])
@pytest.mark.parametrize("dt", [F16, BF16])
def test_exact_dgrad_overflows_to_inf(ops, layer, dt):
    """Weights x 64: exact products, fp32 sums < 2^24; fp16 results past 65504 must be +-Inf as .half() makes them (not 65504), bf16
    results round to 8 significant bits at magnitudes up to ~6e5."""
    n, H, W = GEOMS["b16_800x1344"]
    e = next(x for x in backward_table(n, H, W, 0, dt) if x[0] == "dgrad" and x[1] == layer)
    ref64 = _exact_dgrad(ops, e[2], 77, scale=64.0)
    if dt == F16:
        assert (ref64.abs() > 65520).any(), "no result past fp16's range"


@pytest.mark.parametrize("gname", list(GEOMS))
@pytest.mark.parametrize("dt", [F16, BF16])
def test_exact_pool_bwd(ops, gname, dt):
    n, H, W = GEOMS[gname]
    hw = stage_hw(H, W)
    g = torch.Generator(device=DEV).manual_seed(5)
    for lvl in (3, 4, 5):  # mode 0: the FPN top-down sum (coarse <- 2 x 2 of the finer level), with and without a base
        fine = _ints((n,) + hw[lvl - 1] + (256,), g, dt)
        base = _ints((n,) + hw[lvl] + (256,), g, dt)
        for b in (None, base):
            got = ops.pool_bwd(fine, hw[lvl], b, 0)
            ref = fine.double().view(n, hw[lvl][0], 2, hw[lvl][1], 2, 256).sum((2, 4))
            if b is not None:
                ref += b.double()
            assert torch.equal(got, ref.to(dt)), f"pool_bwd mode 0 p{lvl - 1} -> p{lvl}"
    src = _ints((n,) + hw[6] + (256,), g, dt)  # mode 1: p6 = p5[::2, ::2]
    base = _ints((n,) + hw[5] + (256,), g, dt)
    got = ops.pool_bwd(src, hw[5], base, 1)
    ref = base.double()
    ref[:, ::2, ::2] += src.double()
    assert torch.equal(got, ref.to(dt))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. float runs (random data): rounding against sum|terms|
# ------------------------------------------------------------------------------------------------------------------------------
def _half_ulp(v, dt):
    if dt == torch.float32:
        return torch.zeros_like(v)
    bits = 11 if dt == F16 else 8
    return torch.maximum(v.abs() * 2.0 ** -bits, torch.full_like(v, 2.0 ** -25 if dt == F16 else 0.0))


@pytest.mark.parametrize("e", [c for c in _cases(["b16_800x1344"]) if c.values[0][0] in ("dgrad", "wgrad")])
def test_float_vs_fp64(osr, ops, e):
    kind, name, sig = e
    g = torch.Generator(device=DEV).manual_seed(3000 + zlib.crc32(name.encode()) % 1000)
    if kind == "dgrad":
        dt = sig[-1]
        dy, w, add, mask, post = _dgrad_inputs(sig, g, exact=False)
        got = _run_dgrad(ops, sig, dy, w, add, mask, post)
        ref, sel = _dgrad_expect(sig, dy, w, add, mask, post)
        S, _ = _dgrad_expect(sig, dy, w, add, mask, post, absolute=True)
        chain = sig[0][3] * sig[1][1] * sig[1][2]
    else:
        xs, dys, k, _, stride, pad, acc, dt = sig
        x = torch.randn(xs, generator=g, device=DEV).to(dt)
        dy = torch.randn(dys, generator=g, device=DEV).to(dt)
        with ops.concurrent_streams(2):
            got = ops.conv2d_wgrad(x, dy, k, k, stride, pad)
        ref, S, sel = wgrad_ref(x, dy, k, k, stride, pad), wgrad_ref(x.abs(), dy.abs(), k, k, stride, pad), (slice(None),)
        _, splits, rps, _ = wgrad_plan(osr, xs, dys, k, stride, pad, dt)
        chain, dt = rps + splits, torch.float32
    torch.cuda.synchronize()
    got, ref, S = got[sel].double(), ref[sel], S[sel]
    tol = (chain + 2) * 2.0 ** -24 * S + _half_ulp(ref, dt)
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    ratio = float((err / tol.clamp(min=1e-300)).max())
    print(f"[err] {kind} {name}: max |err| {err.max().item():.3e}, max |err| / bound {ratio:.3e} (chain {chain})")
    _report(f"{kind} {name} err/bound", ratio, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. edges off the production shapes
# ------------------------------------------------------------------------------------------------------------------------------
# (n, cin, cout, h, w, k, stride): M = n * ho * wo not a multiple of 64
WGRAD_EDGES = [
    (3, 256, 256, 13, 21, 3, 1),     # 256^2 one-barrier, 4 splits of 256 rows, the last of 51 (ragged step), grid 36
    (1, 256, 256, 263, 259, 3, 1),   # 256^2 8-phase: 22 splits of 3136 rows, the last of 2261; grid 198
    (3, 1024, 1024, 111, 111, 1, 1),  # 256^2 8-phase over 16 tiles: last split of 2467 rows
    (1, 64, 256, 37, 41, 1, 1),      # 128^2 with cin = 64: 6 splits, the last of 237 rows; grid 12
    (3, 128, 128, 27, 31, 3, 1),     # 128^2 3 x 3: ragged, grid 9 taps x splits
    (3, 256, 512, 29, 23, 1, 2),     # strided 1 x 1 (res3.0.shortcut-like) at odd sizes: 15 x 12 outputs per image
    (1, 12544, 1024, 301, 1, 1, 1),  # direct path (one split) with a ragged last step
]


@pytest.mark.parametrize("case", WGRAD_EDGES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dt", [F16, BF16])
def test_edge_wgrad_exact(osr, ops, case, dt):
    n, cin, cout, h, w, k, stride = case
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    name, splits, rps, grid = wgrad_plan(osr, (n, h, w, cin), (n, ho, wo, cout), k, stride, pad, dt)
    M = n * ho * wo
    print(f"[plan] {case}: {name}, {splits} splits x {rps} rows (last {M - (splits - 1) * rps}), grid {grid}")
    assert M % 64 != 0
    g = torch.Generator(device=DEV).manual_seed(sum(case))
    x, dy = _ints((n, h, w, cin), g, dt), _ints((n, ho, wo, cout), g, dt)
    _exact_wgrad(ops, x, dy, k, stride, pad)
    _exact_wgrad(ops, x, dy, k, stride, pad, acc_init=_ints((cout, k, k, cin), g, torch.float32))


def test_edge_wgrad_plans(osr):
    """The edge cases reach what their comments say."""
    got = {}
    for n, cin, cout, h, w, k, stride in WGRAD_EDGES:
        pad = k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        got[(n, cin, cout, h, w, k, stride)] = wgrad_plan(osr, (n, h, w, cin), (n, ho, wo, cout), k, stride, pad) + (n * ho * wo,)
    names = {v[0] for v in got.values()}
    assert names == {"wgrad 256^2 one-barrier", "wgrad 256^2 8-phase", "wgrad 128^2", "wgrad direct"}, got
    assert any(v[3] % 8 for v in got.values() if v[0] == "wgrad 256^2 8-phase"), got
    assert any(v[3] % 8 for v in got.values() if v[0] == "wgrad 128^2"), got
    for v in got.values():  # every case has a last split shorter than the others, ending in a ragged step
        name, splits, rps, grid, M = v
        assert M - (splits - 1) * rps < rps and (M - (splits - 1) * rps) % 64 != 0, v


# (n, cin, cout, h, w, k, stride, epi): ragged last M tile (M % 128 != 0) on each tile width, with the trainer's epilogues
DGRAD_EDGES = [
    (3, 256, 256, 13, 21, 3, 1, "mask"), (1, 256, 256, 13, 21, 3, 1, "add"), (3, 64, 64, 27, 31, 3, 1, "mask"),
    (3, 256, 64, 27, 31, 1, 1, "add+post_mask"), (3, 512, 128, 29, 23, 1, 2, "strided_only"), (3, 512, 256, 29, 23, 1, 2, "add+post_mask"),
    (1, 1024, 12544, 301, 1, 1, 1, "-"),
]


@pytest.mark.parametrize("case", DGRAD_EDGES, ids=lambda c: "x".join(map(str, c)))
def test_edge_dgrad_exact(ops, case):
    n, cout, cin, h, w, k, stride, epi = case  # dy (n, ho, wo, cout) -> dx (n, h, w, cin)
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    _exact_dgrad(ops, ((n, ho, wo, cout), (cin, k, k, cout), (h, w), stride, pad, epi, F16), sum(case[:7]))


@pytest.mark.parametrize("m,cout", [(1, 256), (5, 256), (37, 1024), (63, 256), (45000, 256), (44826, 1024), (48200, 256)])
@pytest.mark.parametrize("dt", [F16, BF16])
def test_edge_bias_grad(ops, m, cout, dt):
    """Fewer rows than one block (< 64: some of the 8 row lanes have no row at all); rows per block 88 = 24 mod 32 (45000, 44826 rows)
    and 95 = 31 mod 32 (48200 rows): the unrolled loop's last turn ends exactly at the block's end for one of the row lanes. The rows
    are followed by sentinel rows in the same allocation (a read past the last block shows too)."""
    rpb = max(64, (m + 511) // 512)
    g = torch.Generator(device=DEV).manual_seed(m)
    dy = _padded((m, cout), g, dt)
    _exact_bias(ops, dy)
    _exact_bias(ops, dy, acc_init=_ints((cout,), g, torch.float32))
    if m >= 44826:
        assert rpb % 32 >= 24, rpb


@pytest.mark.parametrize("case", [(3, 256, 256, 13, 21, 3), (1, 256, 256, 263, 259, 3), (3, 128, 128, 27, 31, 3), (1, 64, 256, 37, 41, 1)],
                         ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_edge_wgrad_nonfinite_dy(osr, ops, case, bad):
    """An Inf / NaN in dy leaves the layer's dw non-finite (check_finite_ then skips the step); the other output channels stay finite."""
    n, cin, cout, h, w, k = case
    g = torch.Generator(device=DEV).manual_seed(sum(case))
    x = _ints((n, h, w, cin), g, F16)
    x[x == 0] = 1  # every product with the bad value is non-finite
    dy = _ints((n, h, w, cout), g, F16)
    co = cout - 3
    dy[n - 1, h - 1, w // 2, co] = bad  # in the last split
    with ops.concurrent_streams(2):
        dw = ops.conv2d_wgrad(x, dy, k, k, 1, k // 2)
        flag = torch.ones((1,), dtype=torch.int32, device=DEV)
        ops.check_finite_(dw, flag)
    torch.cuda.synchronize()
    assert not torch.isfinite(dw[co]).any()  # (x has no zeros; the 3 x 3 taps that read padding give 0 * Inf = NaN)
    assert torch.isfinite(torch.cat((dw[:co], dw[co + 1:]))).all()
    assert flag.item() == 0
