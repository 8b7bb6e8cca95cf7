"""Thin torch-tensor wrappers over the C ABI (include/osr.h). torch is plumbing here: device memory, the
current HIP stream and output allocation. Every op runs on the HIP library or raises; there is no eager path."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ConvParams, OsrError, Pyramid, RpnLevels, check

_DT = {torch.float32: _lib.OSR_F32, torch.float16: _lib.OSR_F16, torch.bfloat16: _lib.OSR_BF16}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise OsrError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise OsrError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise OsrError(f"{name} must be contiguous")
    return t


def dtype_code(dt: torch.dtype) -> int:
    return _DT[dt]


# ----------------------------------------------------------------------------------------------------------
def stem_padded_width(wp: int) -> int:
    return int(_lib.load().osr_stem_padded_width(wp))


def preprocess(images: torch.Tensor, hp: int, wp: int, mean, std, dtype=torch.float16) -> torch.Tensor:
    """(n,3,h,w) uint8/float32 -> normalised, zero-haloed (n, hp+6, wpad, 4) NHWC tensor for the stem."""
    lib = _lib.load()
    _need(images, name="images")
    if images.dtype not in (torch.uint8, torch.float32):
        raise OsrError("images must be uint8 or float32")
    n, c, h, w = images.shape
    assert c == 3
    out = torch.empty((n, hp + 6, stem_padded_width(wp), 4), dtype=dtype, device=images.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(lib.osr_preprocess(_p(images), int(images.dtype == torch.uint8), n, h, w, hp, wp, m, s, _p(out), _DT[dtype], _stream()),
          "osr_preprocess")
    return out


_CONCURRENCY = [1]
# bench.py's train_step leg sets this to a dict {"conv": 0.0, "wgrad": 0.0}: algorithmic FLOPs (2*M*K*N of the layer definition)
# of every MFMA conv / FC launch (forward and data-gradient launches both go through conv2d) and of every weight-gradient launch
FLOP_COUNT = None
# osr_conv2d_fwd may cut the partial last dispatch round of a deep-K 1x1 / FC layer along K when it is handed a workspace
# (include/osr.h); False keeps every layer a single launch (A/B runs)
SPLIT_K_TAIL = True


class concurrent_streams:
    """Context manager: the launches inside run on `n` HIP streams side by side (the engine's micro-batch streams). Passed to
    the conv kernels as osr_conv_params.concurrency, a tile-selection hint (results do not depend on it)."""

    def __init__(self, n: int):
        self.n = int(n)

    def __enter__(self):
        self.prev = _CONCURRENCY[0]
        _CONCURRENCY[0] = self.n
        return self

    def __exit__(self, *exc):
        _CONCURRENCY[0] = self.prev
        return False


def _new_conv_params() -> "ConvParams":
    p = ConvParams()
    p.concurrency = _CONCURRENCY[0]
    return p


def _conv_params(n, hi, wi, cin, ho, wo, cout, kh, kw, stride, pad, dt_in, dt_out, relu=False, res_mode=0) -> ConvParams:
    """A convolution over dense NHWC tensors."""
    p = _new_conv_params()
    p.n, p.hi, p.wi, p.cin, p.ho, p.wo, p.cout = n, hi, wi, cin, ho, wo, cout
    p.kh, p.kw, p.stride_h, p.stride_w, p.pad_h, p.pad_w = kh, kw, stride, stride, pad, pad
    p.in_stride_n, p.in_stride_h, p.in_stride_w = hi * wi * cin, wi * cin, cin
    p.out_stride_n, p.out_stride_h, p.out_stride_w = ho * wo * cout, wo * cout, cout
    p.relu, p.res_mode, p.pad_mode = int(relu), int(res_mode), 0
    p.in_dtype, p.out_dtype = _DT[dt_in], _DT[dt_out]
    return p


def _stem_params(n, hd, wd, ho, wo, cout, kh, relu, dt) -> ConvParams:
    """The stem view (pad_mode 1): a (kh, 1, 32) stride-2 convolution over the pre-padded NHWC4 image, whose 'pixels' are 4-element groups."""
    p = _conv_params(n, hd, wd, 32, ho, wo, cout, kh, 1, 2, 0, dt, dt, relu)
    p.in_stride_n, p.in_stride_h, p.in_stride_w = hd * wd * 4, wd * 4, 4
    p.pad_mode = 1
    return p


def _set_residual(p: ConvParams, residual: torch.Tensor, dtype, name: str = "residual") -> None:
    """Shape check and strides of p's residual: the output's shape (res_mode 1, 3) or its 2x-coarser parent (res_mode 2, FPN top-down)."""
    _need(residual, dtype, name)
    rn, rh, rw, rc = residual.shape
    exp = (p.n, p.ho, p.wo, p.cout) if p.res_mode in (1, 3) else (p.n, (p.ho + 1) // 2, (p.wo + 1) // 2, p.cout)
    if (rn, rh, rw, rc) != exp:
        raise OsrError(f"residual shape {tuple(residual.shape)} != expected {exp} for res_mode {p.res_mode}")
    p.res_stride_n, p.res_stride_h, p.res_stride_w = rh * rw * rc, rw * rc, rc


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, stride: int = 1, pad: int = 0, relu: bool = False,
           residual: Optional[torch.Tensor] = None, res_mode: int = 0, out_dtype: Optional[torch.dtype] = None,
           out: Optional[torch.Tensor] = None, post_mask: Optional[torch.Tensor] = None,
           row_seg: Optional[Tuple[torch.Tensor, int]] = None) -> torch.Tensor:
    """NHWC implicit-GEMM convolution. x (n,h,w,cin) f16/bf16; weight (cout,kh,kw,cin) same dtype; bias f32.
    post_mask (n,ho,wo,cout), x's dtype: the result is zeroed where post_mask <= 0, in the same launch
    (osr_conv2d_fwd_masked; needs cin % 64 == 0, else the mask is applied by a second launch).
    row_seg = (counts int32 (s,), rows per segment): the output rows are s segments of which only the first counts[i] rows carry
    data (padded per-image lists); tiles without a data row are skipped and their rows left unwritten."""
    lib = _lib.load()
    _need(x, name="x"); _need(weight, x.dtype, "weight"); _need(bias, torch.float32, "bias")
    n, hi, wi, cin = x.shape
    cout, kh, kw, cin2 = weight.shape
    if cin2 != cin:
        raise OsrError(f"weight cin {cin2} != input cin {cin}")
    ho = (hi + 2 * pad - kh) // stride + 1
    wo = (wi + 2 * pad - kw) // stride + 1
    out_dtype = out_dtype or x.dtype
    if out is None:
        out = torch.empty((n, ho, wo, cout), dtype=out_dtype, device=x.device)
    else:
        _need(out, out_dtype, "out")
        assert out.numel() == n * ho * wo * cout
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * ho * wo * cout * kh * kw * cin
    p = _conv_params(n, hi, wi, cin, ho, wo, cout, kh, kw, stride, pad, x.dtype, out_dtype, relu, res_mode)
    if row_seg is not None:
        counts, seg_rows = row_seg
        _need(counts, torch.int32, "row_seg counts")
        if seg_rows < 1 or counts.numel() * seg_rows < n * ho * wo:
            raise OsrError("row_seg does not cover the output rows")
        p.row_seg_counts, p.row_seg_rows = counts.data_ptr(), int(seg_rows)
    if res_mode:
        _set_residual(p, residual, x.dtype)
    if post_mask is not None:
        _need(post_mask, x.dtype, "post_mask")
        if tuple(post_mask.shape) != (n, ho, wo, cout):
            raise OsrError(f"post_mask shape {tuple(post_mask.shape)} != {(n, ho, wo, cout)}")
        st = lib.osr_conv2d_fwd_masked(C.byref(p), _p(x), _p(weight), _p(bias), _p(residual) if res_mode else None, _p(post_mask), _p(out),
                                       _stream())
        if st != _lib.ERR_UNSUPPORTED:
            check(st, "osr_conv2d_fwd_masked")
            return out
    ws = None
    if SPLIT_K_TAIL and post_mask is None and res_mode == 0 and stride == 1:
        wsb = int(lib.osr_conv2d_fwd_workspace_bytes(C.byref(p)))  # > 0: a deep-K 1x1 / FC layer whose last dispatch round is mostly empty
        if wsb > 0:
            ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
            p.workspace, p.workspace_bytes = ws.data_ptr(), wsb
    check(lib.osr_conv2d_fwd(C.byref(p), _p(x), _p(weight), _p(bias), _p(residual) if res_mode else None, _p(out), _stream()),
          "osr_conv2d_fwd")
    if post_mask is not None:
        relu_mask_(out, post_mask)
    return out


def stem_conv(xpad: torch.Tensor, w_view: torch.Tensor, bias: torch.Tensor, hp: int, wp: int, relu: bool = True) -> torch.Tensor:
    """7x7/s2/p3 stem on the pre-padded NHWC4 image (see preprocess): a (kh=7, kw=1, cin=32) implicit GEMM whose
    'pixels' are 4-element groups, 8 of which (7 taps + a zero-weight one) form one K slice. With the 8-row weight
    view (pack_stem_weight) K = 256 and the BK=64 kernel takes it; the 8th row reads the halo with zero weights."""
    lib = _lib.load()
    _need(xpad, name="xpad"); _need(w_view, xpad.dtype, "w_view"); _need(bias, torch.float32, "bias")
    n, hd, wd, c4 = xpad.shape
    assert c4 == 4 and hd == hp + 6 and wd == stem_padded_width(wp)
    cout = w_view.shape[0]
    assert tuple(w_view.shape[1:]) in ((7, 1, 32), (8, 1, 32))
    kh = w_view.shape[1]
    ho, wo = hp // 2, wp // 2
    out = torch.empty((n, ho, wo, cout), dtype=xpad.dtype, device=xpad.device)
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * ho * wo * cout * 147  # 7*7*3 real taps
    p = _stem_params(n, hd, wd, ho, wo, cout, kh, relu, xpad.dtype)
    check(lib.osr_conv2d_fwd(C.byref(p), _p(xpad), _p(w_view), _p(bias), None, _p(out), _stream()), "osr_conv2d_fwd(stem)")
    return out


def stem_maxpool(xpad: torch.Tensor, w_view: torch.Tensor, bias: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
    """[d2] BasicStem in one launch (osr_stem_maxpool_fwd): 7x7/s2/p3 conv + ReLU + 3x3/s2/p1 max pool on the pre-padded NHWC4 image;
    the (n, hp/2, wp/2, 64) stem output stays in LDS. Same bits as stem_conv + maxpool3x3s2. f16 / bf16."""
    lib = _lib.load()
    _need(xpad, name="xpad"); _need(w_view, xpad.dtype, "w_view"); _need(bias, torch.float32, "bias")
    n, hd, wd, c4 = xpad.shape
    assert c4 == 4 and hd == hp + 6 and wd == stem_padded_width(wp) and hp % 2 == 0 and wp % 2 == 0
    assert w_view.shape[0] == 64 and tuple(w_view.shape[2:]) == (1, 32) and w_view.shape[1] in (7, 8)
    hs, ws = hp // 2, wp // 2
    out = torch.empty((n, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1, 64), dtype=xpad.dtype, device=xpad.device)
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * hs * ws * 64 * 147  # 7*7*3 real taps of every stem pixel (the pool's halo recompute is not credited)
    check(lib.osr_stem_maxpool_fwd(_p(xpad), n, hp, wp, _p(w_view), int(w_view.shape[1]), _p(bias), _p(out), _DT[xpad.dtype], _stream()), "osr_stem_maxpool_fwd")
    return out


def stem_maxpool_raw(images: torch.Tensor, hp: int, wp: int, mean, std, w_view: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """preprocess + stem_maxpool in one launch (osr_stem_maxpool_fwd_raw): (n,3,h,w) uint8 / float32 images -> (n, hp/4, wp/4, 64) in
    w_view's dtype; the normalised, padded copy of the batch is never written. Same bits as preprocess -> stem_maxpool."""
    lib = _lib.load()
    _need(images, name="images"); _need(w_view, name="w_view"); _need(bias, torch.float32, "bias")
    if images.dtype not in (torch.uint8, torch.float32) or w_view.dtype not in (torch.float16, torch.bfloat16):
        raise OsrError("stem_maxpool_raw: uint8 / float32 images, f16 / bf16 weights")
    n, c, h, w = images.shape
    assert c == 3 and hp >= h and wp >= w and hp % 2 == 0 and wp % 2 == 0
    assert w_view.shape[0] == 64 and tuple(w_view.shape[2:]) == (1, 32) and w_view.shape[1] in (7, 8)
    hs, ws = hp // 2, wp // 2
    out = torch.empty((n, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1, 64), dtype=w_view.dtype, device=images.device)
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * hs * ws * 64 * 147
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(lib.osr_stem_maxpool_fwd_raw(_p(images), int(images.dtype == torch.uint8), n, h, w, hp, wp, m, s, _p(w_view), int(w_view.shape[1]), _p(bias),
                                       _p(out), _DT[w_view.dtype], _stream()), "osr_stem_maxpool_fwd_raw")
    return out


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, relu: bool = False,
           out_dtype: Optional[torch.dtype] = None, row_seg: Optional[Tuple[torch.Tensor, int]] = None) -> torch.Tensor:
    """Fully connected layer on the MFMA path: x (m,k) f16/bf16, weight (n,k). row_seg: see conv2d."""
    m, k = x.shape
    y = conv2d(x.view(1, m, 1, k), weight.view(weight.shape[0], 1, 1, k), bias, relu=relu, out_dtype=out_dtype, row_seg=row_seg)
    return y.view(m, weight.shape[0])


# set to a dict {"launches": 0, "flops": 0.0}: every osr_linear_split_fwd launch and its algorithmic FLOPs (2*m*k*n, one product per
# element pair: the three bf16 products behind it are the kernel's business) are counted -- how a test or a script sees that a layer
# ran on the split-precision kernel and on nothing else
LINEAR_SPLIT_COUNT = None


def _split_planes(w: torch.Tensor, shape, out, name: str):
    _need(w, torch.float32, "w")
    if w.dim() != 2 or w.numel() == 0:
        raise OsrError(f"{name}: a non-empty 2-d matrix")
    if out is None:
        return torch.empty(shape, dtype=torch.bfloat16, device=w.device), torch.empty(shape, dtype=torch.bfloat16, device=w.device)
    hi, lo = out[0], out[1]
    _need(hi, torch.bfloat16, "out hi"); _need(lo, torch.bfloat16, "out lo")
    if tuple(hi.shape) != tuple(shape) or tuple(lo.shape) != tuple(shape):
        raise OsrError(f"{name}: the planes must be {tuple(shape)}")
    return hi, lo


def split_rows_bf16(w: torch.Tensor, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (rows, cols) on the GPU -> its two bf16 planes (osr_split_rows_bf16): the same bits as weights.split_fp32_rows.
    out: (hi, lo) to refill in place."""
    hi, lo = _split_planes(w, tuple(w.shape), out, "split_rows_bf16")
    check(_lib.load().osr_split_rows_bf16(_p(w), w.shape[0], w.shape[1], _p(hi), _p(lo), _stream()), "osr_split_rows_bf16")
    return hi, lo


def split_rows_bf16_t(w: torch.Tensor, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (rows, cols) on the GPU -> the two bf16 planes (cols, rows) of its transpose (osr_split_rows_bf16_t): the weight operand of
    linear_split_dgrad, the same bits as weights.split_fp32_rows_t. out: (hi, lo) to refill in place."""
    hi, lo = _split_planes(w, tuple(w.shape[::-1]), out, "split_rows_bf16_t")
    check(_lib.load().osr_split_rows_bf16_t(_p(w), w.shape[0], w.shape[1], _p(hi), _p(lo), _stream()), "osr_split_rows_bf16_t")
    return hi, lo


# as LINEAR_SPLIT_COUNT, for the two backward kernels: {"launches": 0, "flops": 0.0} counts every osr_linear_split_dgrad /
# osr_linear_split_wgrad launch and its algorithmic FLOPs (2*m*n*k)
LINEAR_SPLIT_DGRAD_COUNT = None
LINEAR_SPLIT_WGRAD_COUNT = None


def _row_seg_args(row_seg, m: int):
    if row_seg is None:
        return None, 0
    counts, seg_rows = row_seg
    _need(counts, torch.int32, "row_seg counts")
    if seg_rows < 1 or counts.numel() * seg_rows < m:
        raise OsrError("row_seg does not cover the rows")
    return counts.data_ptr(), int(seg_rows)


def linear_split_dgrad(dy: torch.Tensor, wt_split, mask: Optional[torch.Tensor] = None, row_seg: Optional[Tuple[torch.Tensor, int]] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Data gradient of linear_split at fp32 quality on the bf16 MFMA (osr_linear_split_dgrad): dy (m, n) fp32, wt_split = (hi, lo) the
    (k, n) bf16 planes of the TRANSPOSED weight (split_rows_bf16_t / weights.split_fp32_rows_t) -> dx (m, k) fp32. mask (m, k) fp32: the
    saved forward output of the layer below; dx is exactly 0 where it is <= 0. row_seg: as linear_split (rows of skipped tiles are left
    unwritten)."""
    hi, lo = wt_split[0], wt_split[1]
    _need(dy, torch.float32, "dy"); _need(hi, torch.bfloat16, "wt_split hi"); _need(lo, torch.bfloat16, "wt_split lo")
    if dy.dim() != 2 or hi.dim() != 2 or hi.shape != lo.shape or hi.shape[1] != dy.shape[1] or dy.shape[0] < 1:
        raise OsrError(f"linear_split_dgrad: dy {tuple(dy.shape)}, transposed weight planes {tuple(hi.shape)} / {tuple(lo.shape)}")
    (m, n), k = dy.shape, hi.shape[0]
    if mask is not None:
        _need(mask, torch.float32, "mask")
        if tuple(mask.shape) != (m, k):
            raise OsrError(f"linear_split_dgrad: mask {tuple(mask.shape)} for dx {(m, k)}")
    if out is None:
        out = torch.empty((m, k), dtype=torch.float32, device=dy.device)
    else:
        _need(out, torch.float32, "out")
        assert tuple(out.shape) == (m, k)
    seg_p, seg_rows = _row_seg_args(row_seg, m)
    check(_lib.load().osr_linear_split_dgrad(_p(dy), n, _p(hi), _p(lo), _p(mask), k, _p(out), k, m, n, k, seg_p, seg_rows, _stream()),
          "osr_linear_split_dgrad")
    if LINEAR_SPLIT_DGRAD_COUNT is not None:
        LINEAR_SPLIT_DGRAD_COUNT["launches"] += 1
        LINEAR_SPLIT_DGRAD_COUNT["flops"] += 2.0 * m * k * n
    return out


def linear_split_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: Optional[torch.Tensor] = None,
                       row_seg: Optional[Tuple[torch.Tensor, int]] = None) -> torch.Tensor:
    """Weight gradient of linear_split at fp32 quality on the bf16 MFMA (osr_linear_split_wgrad): x (m, k), dy (m, n) fp32 ->
    dW (n, k) = dy^T x fp32, the forward weight's layout. row_seg = (counts, seg_rows): rows at or beyond their segment's count
    (padding of the per-image lists) contribute nothing, whatever they hold."""
    lib = _lib.load()
    _need(x, torch.float32, "x"); _need(dy, torch.float32, "dy")
    if x.dim() != 2 or dy.dim() != 2 or x.shape[0] != dy.shape[0] or x.shape[0] < 1:
        raise OsrError(f"linear_split_wgrad: x {tuple(x.shape)}, dy {tuple(dy.shape)}")
    (m, k), n = x.shape, dy.shape[1]
    if dw is None:
        dw = torch.empty((n, k), dtype=torch.float32, device=x.device)
    else:
        _need(dw, torch.float32, "dw")
        assert tuple(dw.shape) == (n, k)
    seg_p, seg_rows = _row_seg_args(row_seg, m)
    nb = int(lib.osr_linear_split_wgrad_workspace_bytes(m, n, k))
    ws = torch.empty((nb,), dtype=torch.uint8, device=x.device) if nb else None
    check(lib.osr_linear_split_wgrad(_p(dy), n, _p(x), k, _p(dw), k, m, n, k, seg_p, seg_rows, _p(ws), nb, _stream()), "osr_linear_split_wgrad")
    if LINEAR_SPLIT_WGRAD_COUNT is not None:
        LINEAR_SPLIT_WGRAD_COUNT["launches"] += 1
        LINEAR_SPLIT_WGRAD_COUNT["flops"] += 2.0 * m * k * n
    return dw


def linear_split(x: torch.Tensor, w_split, bias: torch.Tensor, relu: bool = False, row_seg: Optional[Tuple[torch.Tensor, int]] = None,
                 x_exp: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fully connected layer at fp32 quality on the bf16 MFMA (osr_linear_split_fwd): x (m, k) fp32, w_split = (hi, lo[, None]) the
    bf16 planes of the (n, k) fp32 weight (weights.split_fp32_rows / split_rows_bf16), bias fp32 -> fp32 (m, n). row_seg: see conv2d
    (skipped tiles are 128 rows). x_exp: per-row exponents of an fp16-term split; the bf16 terms need none, so it must be None."""
    if x_exp is not None:
        raise OsrError("linear_split: the bf16 split carries no row exponents (x_exp must be None)")
    hi, lo = w_split[0], w_split[1]
    _need(x, torch.float32, "x"); _need(hi, torch.bfloat16, "w_split hi"); _need(lo, torch.bfloat16, "w_split lo"); _need(bias, torch.float32, "bias")
    if x.dim() != 2 or hi.dim() != 2 or hi.shape != lo.shape or hi.shape[1] != x.shape[1] or bias.numel() != hi.shape[0] or x.shape[0] < 1:
        raise OsrError(f"linear_split: x {tuple(x.shape)}, weight planes {tuple(hi.shape)} / {tuple(lo.shape)}, bias {tuple(bias.shape)}")
    (m, k), n = x.shape, hi.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    else:
        _need(out, torch.float32, "out")
        assert tuple(out.shape) == (m, n)
    p = _lib.LinearSplitParams()
    p.m, p.n, p.k, p.relu, p.ldx, p.ldo = m, n, k, int(relu), k, n
    if row_seg is not None:
        counts, seg_rows = row_seg
        _need(counts, torch.int32, "row_seg counts")
        if seg_rows < 1 or counts.numel() * seg_rows < m:
            raise OsrError("row_seg does not cover the output rows")
        p.row_seg_counts, p.row_seg_rows = counts.data_ptr(), int(seg_rows)
    check(_lib.load().osr_linear_split_fwd(C.byref(p), _p(x), _p(hi), _p(lo), _p(bias), _p(out), _stream()), "osr_linear_split_fwd")
    if LINEAR_SPLIT_COUNT is not None:
        LINEAR_SPLIT_COUNT["launches"] += 1
        LINEAR_SPLIT_COUNT["flops"] += 2.0 * m * k * n
    return out


# as LINEAR_SPLIT_COUNT, for the split-precision convolution: {"launches": 0, "flops": 0.0} counts every osr_conv2d_split_fwd launch and
# the layer's algorithmic FLOPs (2 * pixels * cout * kh*kw*cin; 147 real taps per output for the stem)
CONV_SPLIT_COUNT = None


def _conv_split_planes(w_split, name: str):
    hi, lo = w_split[0], w_split[1]
    _need(hi, torch.bfloat16, name + " hi"); _need(lo, torch.bfloat16, name + " lo")
    if hi.dim() != 4 or hi.shape != lo.shape:
        raise OsrError(f"{name}: two (cout,kh,kw,cin) bf16 planes, got {tuple(hi.shape)} / {tuple(lo.shape)}")
    return hi, lo


def conv2d_split(x: torch.Tensor, w_split, bias: torch.Tensor, stride: int = 1, pad: int = 0, relu: bool = False,
                 residual: Optional[torch.Tensor] = None, res_mode: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2d at fp32 quality on the bf16 MFMA (osr_conv2d_split_fwd): x (n,h,w,cin) fp32, w_split = (hi, lo) the bf16 planes of the
    (cout,kh,kw,cin) fp32 weight (weights.split_conv_weight), bias fp32, residual fp32 -> fp32 (n,ho,wo,cout). stride, pad, relu,
    residual and res_mode as conv2d. cin % 32 == 0, cout % 64 == 0, 1x1 / 3x3 at stride 1 / 2."""
    lib = _lib.load()
    _need(x, torch.float32, "x"); _need(bias, torch.float32, "bias")
    hi, lo = _conv_split_planes(w_split, "w_split")
    if x.dim() != 4:
        raise OsrError(f"conv2d_split: x must be (n,h,w,cin), got {tuple(x.shape)}")
    n, hi_, wi, cin = x.shape
    cout, kh, kw, cin2 = hi.shape
    if cin2 != cin:
        raise OsrError(f"weight cin {cin2} != input cin {cin}")
    ho = (hi_ + 2 * pad - kh) // stride + 1
    wo = (wi + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    else:
        _need(out, torch.float32, "out")
        if tuple(out.shape) not in ((n, ho, wo, cout), (n * ho * wo, cout)):
            raise OsrError(f"conv2d_split: out {tuple(out.shape)} for a result of {(n, ho, wo, cout)} (or its {(n * ho * wo, cout)} rows)")
    p = _conv_params(n, hi_, wi, cin, ho, wo, cout, kh, kw, stride, pad, torch.float32, torch.float32, relu, res_mode)
    if res_mode:
        _set_residual(p, residual, torch.float32)
    check(lib.osr_conv2d_split_fwd(C.byref(p), _p(x), _p(hi), _p(lo), _p(bias), _p(residual) if res_mode else None, _p(out), _stream()),
          "osr_conv2d_split_fwd")
    if CONV_SPLIT_COUNT is not None:
        CONV_SPLIT_COUNT["launches"] += 1
        CONV_SPLIT_COUNT["flops"] += 2.0 * n * ho * wo * cout * kh * kw * cin
    return out


def stem_conv_split(xpad: torch.Tensor, w_split, bias: torch.Tensor, hp: int, wp: int, relu: bool = True) -> torch.Tensor:
    """stem_conv at fp32 quality on the bf16 MFMA: xpad the fp32 pre-padded NHWC4 image (preprocess(..., dtype=float32)), w_split the
    bf16 planes of the (cout,8,1,32) stem view (weights.split_stem_weight) -> fp32 (n, hp/2, wp/2, cout)."""
    lib = _lib.load()
    _need(xpad, torch.float32, "xpad"); _need(bias, torch.float32, "bias")
    hi, lo = _conv_split_planes(w_split, "w_split")
    n, hd, wd, c4 = xpad.shape
    assert c4 == 4 and hd == hp + 6 and wd == stem_padded_width(wp)
    cout = hi.shape[0]
    assert tuple(hi.shape[1:]) == (8, 1, 32)
    ho, wo = hp // 2, wp // 2
    out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=xpad.device)
    p = _stem_params(n, hd, wd, ho, wo, cout, 8, relu, torch.float32)
    check(lib.osr_conv2d_split_fwd(C.byref(p), _p(xpad), _p(hi), _p(lo), _p(bias), None, _p(out), _stream()), "osr_conv2d_split_fwd(stem)")
    if CONV_SPLIT_COUNT is not None:
        CONV_SPLIT_COUNT["launches"] += 1
        CONV_SPLIT_COUNT["flops"] += 2.0 * n * ho * wo * cout * 147  # 7*7*3 real taps
    return out


def conv2d_chain(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, residual: torch.Tensor,
                 stride: int = 1, pad: int = 0, keep_mid: bool = False):
    """A bottleneck's conv2 -> conv3 in one launch (osr_conv2d_chain_fwd): relu(conv1x1(relu(conv(x, weight) + bias), w3) + b3 +
    residual). x (n,h,w,cin) f16/bf16, weight (cmid,kh,kw,cin), w3 (cout3,1,1,cmid), residual (n,ho,wo,cout3). Returns None when the
    shape is outside the fused kernel's envelope (the caller then runs conv2d twice). keep_mid: also return the first convolution's
    activated output (n,ho,wo,cmid) -- (out, mid) -- as the training step needs it."""
    lib = _lib.load()
    _need(x, name="x")
    if x.dtype not in (torch.float16, torch.bfloat16):
        return None
    _need(weight, x.dtype, "weight"); _need(w3, x.dtype, "w3"); _need(residual, x.dtype, "residual")
    _need(bias, torch.float32, "bias"); _need(b3, torch.float32, "b3")
    n, hi, wi, cin = x.shape
    cmid, kh, kw, cin2 = weight.shape
    cout3 = w3.shape[0]
    if cin2 != cin or tuple(w3.shape) != (cout3, 1, 1, cmid) or bias.numel() != cmid or b3.numel() != cout3:
        raise OsrError("conv2d_chain: weight shapes do not form conv -> 1x1 conv")
    ho = (hi + 2 * pad - kh) // stride + 1
    wo = (wi + 2 * pad - kw) // stride + 1
    if tuple(residual.shape) != (n, ho, wo, cout3):
        raise OsrError(f"conv2d_chain: residual shape {tuple(residual.shape)} != {(n, ho, wo, cout3)}")
    p = _conv_params(n, hi, wi, cin, ho, wo, cmid, kh, kw, stride, pad, x.dtype, x.dtype, relu=True)
    out = torch.empty((n, ho, wo, cout3), dtype=x.dtype, device=x.device)
    mid = torch.empty((n, ho, wo, cmid), dtype=x.dtype, device=x.device) if keep_mid else None
    st = lib.osr_conv2d_chain_fwd_ex(C.byref(p), _p(x), _p(weight), _p(bias), _p(w3), _p(b3), cout3, _p(residual), _p(out), _p(mid), _stream())
    if st == _lib.ERR_UNSUPPORTED:
        return None
    check(st, "osr_conv2d_chain_fwd")
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * ho * wo * (cmid * kh * kw * cin + cout3 * cmid)
    return (out, mid) if keep_mid else out


def bottleneck(x: torch.Tensor, w1, b1, w2, b2, w3, b3, wsc=None, bsc=None) -> Optional[torch.Tensor]:
    """One whole bottleneck block in one launch (osr_bottleneck_fwd): x (n,h,w,cin) f16/bf16, weights packed (cout,kh,kw,cin) in
    x's dtype, biases fp32; wsc / bsc = the projection shortcut (None: identity). Returns y (n,h,w,cout), or None when the shape
    is outside the fused kernel's envelope (the caller then runs the separate convolutions)."""
    lib = _lib.load()
    _need(x, name="x")
    if x.dtype not in (torch.float16, torch.bfloat16):
        return None
    n, h, w, cin = x.shape
    cmid, cout = w1.shape[0], w3.shape[0]
    for t, nm in ((w1, "w1"), (w2, "w2"), (w3, "w3")):
        _need(t, x.dtype, nm)
    for t, nm in ((b1, "b1"), (b2, "b2"), (b3, "b3")):
        _need(t, torch.float32, nm)
    if tuple(w1.shape) != (cmid, 1, 1, cin) or tuple(w2.shape) != (cmid, 3, 3, cmid) or tuple(w3.shape) != (cout, 1, 1, cmid):
        raise OsrError("bottleneck: weight shapes do not form a 1x1 -> 3x3 -> 1x1 block")
    p = _lib.BottleneckParams()
    p.n, p.h, p.w, p.cin, p.cmid, p.cout = n, h, w, cin, cmid, cout
    p.dtype, p.has_proj = _DT[x.dtype], int(wsc is not None)
    if wsc is not None:
        _need(wsc, x.dtype, "wsc"); _need(bsc, torch.float32, "bsc")
        if tuple(wsc.shape) != (cout, 1, 1, cin):
            raise OsrError("bottleneck: projection weight shape")
    out = torch.empty((n, h, w, cout), dtype=x.dtype, device=x.device)
    st = lib.osr_bottleneck_fwd(C.byref(p), _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), _p(wsc), _p(bsc), _p(out), _stream())
    if st == _lib.ERR_UNSUPPORTED:
        return None
    check(st, "osr_bottleneck_fwd")
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * h * w * (cin * cmid + 9 * cmid * cmid + cmid * cout + (cin * cout if wsc is not None else 0))
    return out


def resize_bilinear_u8(img: torch.Tensor, xbounds, xcoef, kx: int, ybounds, ycoef, ky: int, y_first: int, y_rows: int, nh: int, nw: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL Image.resize(BILINEAR) of an (h, w, 3) uint8 CUDA image with Pillow's coefficient tables (host/data.py:
    pil_resample_coeffs) -> (3, nh, nw) uint8 (osr_resize_bilinear_u8)."""
    lib = _lib.load()
    _need(img, torch.uint8, "img")
    for t, nm in ((xbounds, "xbounds"), (xcoef, "xcoef"), (ybounds, "ybounds"), (ycoef, "ycoef")):
        _need(t, torch.int32, nm)
    h, w, c = img.shape
    if c != 3 or xbounds.shape[0] != nw or ybounds.shape[0] != nh or xcoef.shape[1] != kx or ycoef.shape[1] != ky:
        raise OsrError("resize_bilinear_u8: table shapes do not match the sizes")
    tmp_bytes = int(lib.osr_resize_tmp_bytes(y_rows, nw))
    tmp = torch.empty((tmp_bytes,), dtype=torch.uint8, device=img.device)
    if out is None:
        out = torch.empty((3, nh, nw), dtype=torch.uint8, device=img.device)
    else:
        _need(out, torch.uint8, "out")
        if tuple(out.shape) != (3, nh, nw):
            raise OsrError("resize_bilinear_u8: out must be (3, nh, nw)")
    check(lib.osr_resize_bilinear_u8(_p(img), h, w, w * 3, _p(xbounds), _p(xcoef), kx, _p(ybounds), _p(ycoef), ky, y_first, y_rows, nh, nw, _p(tmp),
                                     tmp_bytes, _p(out), _stream()), "osr_resize_bilinear_u8")
    return out


def resize_bilinear_u8_planar(img: torch.Tensor, xbounds, xcoef, kx: int, ybounds, ycoef, ky: int, y_first: int, y_rows: int, nh: int, nw: int,
                              mirror: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL Image.resize(BILINEAR) of planar uint8 CUDA images, (3, h, w) or a stacked (n, 3, h, w), with Pillow's coefficient tables
    (host/data.py: pil_resample_coeffs) -> the same shape at (nh, nw); mirror: flipped along x after the resize
    (osr_resize_bilinear_u8_planar)."""
    lib = _lib.load()
    _need(img, torch.uint8, "img")
    for t, nm in ((xbounds, "xbounds"), (xcoef, "xcoef"), (ybounds, "ybounds"), (ycoef, "ycoef")):
        _need(t, torch.int32, nm)
    if img.dim() not in (3, 4):
        raise OsrError("resize_bilinear_u8_planar: img must be (planes, h, w) or (n, planes, h, w)")
    h, w = int(img.shape[-2]), int(img.shape[-1])
    planes = img.numel() // max(h * w, 1)
    if tuple(xbounds.shape) != (nw, 2) or tuple(ybounds.shape) != (nh, 2) or tuple(xcoef.shape) != (nw, kx) or tuple(ycoef.shape) != (nh, ky):
        raise OsrError("resize_bilinear_u8_planar: table shapes do not match the sizes")
    tmp_bytes = planes * y_rows * nw
    tmp = torch.empty((tmp_bytes,), dtype=torch.uint8, device=img.device)
    shape = tuple(img.shape[:-2]) + (nh, nw)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    else:
        _need(out, torch.uint8, "out")
        if tuple(out.shape) != shape:
            raise OsrError(f"resize_bilinear_u8_planar: out must be {shape}")
    check(lib.osr_resize_bilinear_u8_planar(_p(img), planes, h, w, _p(xbounds), _p(xcoef), kx, _p(ybounds), _p(ycoef), ky, y_first, y_rows, nh, nw,
                                            int(bool(mirror)), _p(tmp), tmp_bytes, _p(out), _stream()), "osr_resize_bilinear_u8_planar")
    return out


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, name="x")
    n, h, w, c = x.shape
    out = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
    check(lib.osr_maxpool3x3s2(_p(x), n, h, w, c, _p(out), _DT[x.dtype], _stream()), "osr_maxpool3x3s2")
    return out


def stem_pool_bwd(s: torch.Tensor, dpool: torch.Tensor) -> torch.Tensor:
    """Backward of ReLU -> max_pool2d(3, 2, 1) of the stem (osr_stem_pool_bwd): s the (n, hs, ws, c) stem output (post-ReLU), dpool
    the pooled output's gradient -> ds (n, hs, ws, c), zero where s <= 0."""
    lib = _lib.load()
    _need(s, name="s"); _need(dpool, s.dtype, "dpool")
    n, hs, ws, c = s.shape
    if tuple(dpool.shape) != (n, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1, c):
        raise OsrError(f"dpool shape {tuple(dpool.shape)} does not match the stem output {tuple(s.shape)}")
    ds = torch.empty_like(s)
    check(lib.osr_stem_pool_bwd(_p(s), _p(dpool), n, hs, ws, c, _p(ds), _DT[s.dtype], _stream()), "osr_stem_pool_bwd")
    return ds


def stem_wgrad(xpad: torch.Tensor, ds: torch.Tensor, hp: int, wp: int, dw: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """Weight gradient of the stem in the stem view's layout (64, 8, 1, 32), fp32 (osr_stem_wgrad): xpad = preprocess(...), ds the
    stem output's gradient (n, hp/2, wp/2, 64). The 8th row, the 8th tap and the 4th channel come out exactly 0."""
    lib = _lib.load()
    _need(xpad, name="xpad"); _need(ds, xpad.dtype, "ds")
    n = xpad.shape[0]
    if tuple(xpad.shape) != (n, hp + 6, stem_padded_width(wp), 4) or tuple(ds.shape) != (n, hp // 2, wp // 2, 64):
        raise OsrError(f"stem_wgrad: xpad {tuple(xpad.shape)} / ds {tuple(ds.shape)} do not match hp={hp}, wp={wp}")
    if dw is None:
        dw = torch.empty((64, 8, 1, 32), dtype=torch.float32, device=xpad.device)
        accumulate = False
    else:
        _need(dw, torch.float32, "dw")
        if tuple(dw.shape) != (64, 8, 1, 32):
            raise OsrError(f"stem_wgrad: dw must be (64, 8, 1, 32), got {tuple(dw.shape)}")
    wsb = int(lib.osr_stem_wgrad_workspace_bytes(n, hp, wp))
    if wsb < 0:
        check(wsb, "osr_stem_wgrad_workspace_bytes")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=xpad.device)
    if FLOP_COUNT is not None:
        FLOP_COUNT["wgrad"] += 2.0 * n * (hp // 2) * (wp // 2) * 64 * 147
    check(lib.osr_stem_wgrad(_p(xpad), _p(ds), n, hp, wp, _p(dw), int(accumulate), _p(ws), wsb, _DT[xpad.dtype], _stream()), "osr_stem_wgrad")
    return dw


def subsample2(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, name="x")
    n, h, w, c = x.shape
    out = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
    check(lib.osr_subsample2(_p(x), n, h, w, c, _p(out), _DT[x.dtype], _stream()), "osr_subsample2")
    return out


def deform_offset_channels(groups: int, modulated: bool) -> int:
    """Channels of a deformable layer's `conv2_offset` output: 18 G offsets (dy, dx per tap and group), then 9 G mask logits when modulated."""
    return (27 if modulated else 18) * int(groups)


def deform_cols(x: torch.Tensor, om: torch.Tensor, stride: int = 1, groups: int = 1, modulated: bool = False) -> torch.Tensor:
    """The gather of a 3x3 deformable convolution (osr_deform_cols, include/osr.h): x (n,h,w,c) f16 / bf16 / f32, om (n,ho,wo,ch) fp32
    with ch >= deform_offset_channels(groups, modulated) as the row pitch -> cols (n*ho*wo, 9, c) in x's dtype, the masked bilinear
    sample of every (output pixel, tap, channel). c, and c / groups, must be multiples of 8: OsrError (status -2, nothing launched)."""
    lib = _lib.load()
    _need(x, name="x"); _need(om, torch.float32, "om")
    n, h, w, c = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if om.dim() != 4 or tuple(om.shape[:3]) != (n, ho, wo):
        raise OsrError(f"deform_cols: om {tuple(om.shape)} does not match the output pixels {(n, ho, wo)} of x {tuple(x.shape)} at stride {stride}")
    cols = torch.empty((n * ho * wo, 9, c), dtype=x.dtype, device=x.device)
    check(lib.osr_deform_cols(_p(x), _p(om), n, h, w, c, ho, wo, int(om.shape[3]), int(stride), int(groups), int(bool(modulated)), _p(cols),
                              _DT[x.dtype], _stream()), "osr_deform_cols")
    return cols


def deform_conv2d(x: torch.Tensor, om: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, stride: int = 1, groups: int = 1,
                  modulated: bool = False, relu: bool = False) -> torch.Tensor:
    """3x3 deformable convolution, padding 1 ([d2] DeformConv / ModulatedDeformConv; `groups` = deformable groups, the weight is dense)
    as two launches: deform_cols, then the 1x1 contraction of its (pixels, 9 c) rows with weight (cout,3,3,c) viewed as (cout, 9 c) --
    conv2d's kernels, fp32 ones for fp32 tensors. -> (n,ho,wo,cout) in x's dtype."""
    n, h, w, c = x.shape
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (3, 3, c):
        raise OsrError(f"deform_conv2d: weight {tuple(weight.shape)} is not (cout, 3, 3, {c})")
    cols = deform_cols(x, om, stride, groups, modulated)
    m = cols.shape[0]
    y = conv2d(cols.view(1, m, 1, 9 * c), weight.view(cout, 1, 1, 9 * c), bias, relu=relu)
    return y.view(n, (h - 1) // stride + 1, (w - 1) // stride + 1, cout)


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = False) -> torch.Tensor:
    lib = _lib.load()
    _need(a, torch.float32, "a"); _need(w, torch.float32, "w")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    check(lib.osr_gemm_f32(_p(a), k, _p(w), _p(bias), _p(out), n, m, n, k, int(relu), _stream()), "osr_gemm_f32")
    return out


def gemm_f32_tn(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = sum_k a[k, m] * b[k, n] (= a^T b) in exact fp32: the weight gradient dy^T x of an fp32 linear layer."""
    lib = _lib.load()
    _need(a, torch.float32, "a"); _need(b, torch.float32, "b")
    k, m = a.shape
    assert b.shape[0] == k
    n = b.shape[1]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    else:
        _need(out, torch.float32, "out")
        assert tuple(out.shape) == (m, n)
    nb = int(lib.osr_gemm_f32_tn_workspace_bytes(m, n, k))
    ws = torch.empty((nb,), dtype=torch.uint8, device=a.device) if nb else None
    check(lib.osr_gemm_f32_tn(_p(a), m, _p(b), n, _p(out), n, m, n, k, _p(ws), nb, _stream()), "osr_gemm_f32_tn")
    return out


def cfrpn_head_tail(t: torch.Tensor, w_delta, b_delta, w_ctr, b_ctr) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    _need(t, name="t")
    rows, c = t.shape
    for x in (w_delta, b_delta, w_ctr, b_ctr):
        _need(x, torch.float32, "head weight")
    deltas = torch.empty((rows, 4), dtype=torch.float32, device=t.device)
    ctr = torch.empty((rows,), dtype=torch.float32, device=t.device)
    check(lib.osr_cfrpn_head_tail(_p(t), _DT[t.dtype], rows, c, _p(w_delta), _p(b_delta), _p(w_ctr), _p(b_ctr), _p(deltas), _p(ctr),
                                  _stream()), "osr_cfrpn_head_tail")
    return deltas, ctr


def cfrpn_head_fused(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, w_tail: torch.Tensor, b_tail: torch.Tensor,
                     deltas_out: Optional[torch.Tensor] = None, ctr_out: Optional[torch.Tensor] = None, hidden_out: Optional[torch.Tensor] = None):
    """ClsFreeRPNHead.forward for one level in one launch. x (n,h,w,256) f16/bf16, weight (256,3,3,256) packed,
    w_tail (5,256) fp32 [deltas rows 0-3, centerness row 4], b_tail (5). Returns deltas (n*h*w, 4), ctr (n*h*w).
    hidden_out (n*h*w, 256), x's dtype: also receives the hidden state relu(conv + bias) (the training step keeps it)."""
    lib = _lib.load()
    _need(x, name="x"); _need(weight, x.dtype, "weight"); _need(bias, torch.float32, "bias")
    _need(w_tail, torch.float32, "w_tail"); _need(b_tail, torch.float32, "b_tail")
    n, hi, wi, cin = x.shape
    cout, kh, kw, _ = weight.shape
    pad = kh // 2
    rows = n * hi * wi
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * rows * cout * (kh * kw * cin + 5)  # the 3x3 conv + the five 1x1 outputs of the fused tail
    deltas = deltas_out if deltas_out is not None else torch.empty((rows, 4), dtype=torch.float32, device=x.device)
    ctr = ctr_out if ctr_out is not None else torch.empty((rows,), dtype=torch.float32, device=x.device)
    _need(deltas, torch.float32, "deltas"); _need(ctr, torch.float32, "ctr")
    assert deltas.numel() == rows * 4 and ctr.numel() == rows
    p = _conv_params(n, hi, wi, cin, hi, wi, cout, kh, kw, 1, pad, x.dtype, x.dtype, relu=True)
    if hidden_out is not None:
        _need(hidden_out, x.dtype, "hidden_out")
        assert hidden_out.numel() == rows * 256
    check(lib.osr_cfrpn_head_fwd_ex(C.byref(p), _p(x), _p(weight), _p(bias), _p(w_tail), _p(b_tail), _p(deltas), _p(ctr), _p(hidden_out), _stream()),
          "osr_cfrpn_head_fwd")
    return deltas, ctr


def conv2d_pair(x: torch.Tensor, w_a: torch.Tensor, b_a: torch.Tensor, relu_a: bool, w_b: torch.Tensor, b_b: torch.Tensor, relu_b: bool,
                stride: int = 1, pad: int = 0):
    """Two convolutions of the same input and geometry in ONE launch (osr_conv2d_fwd_pair: the projection shortcut and conv1 of a
    stage's first bottleneck). Returns (out_a, out_b), or None outside the launch's envelope (the caller runs conv2d twice)."""
    lib = _lib.load()
    ca, kh, kw, cin = w_a.shape
    cb = w_b.shape[0]
    if tuple(w_b.shape[1:]) != (kh, kw, cin) or ca % 128 or cb % 128 or cin % 64 or x.dtype not in (torch.float16, torch.bfloat16):
        return None
    _need(x, name="x"); _need(w_a, x.dtype, "w_a"); _need(w_b, x.dtype, "w_b"); _need(b_a, torch.float32, "b_a"); _need(b_b, torch.float32, "b_b")
    n, hi, wi, _ = x.shape
    ho, wo = (hi + 2 * pad - kh) // stride + 1, (wi + 2 * pad - kw) // stride + 1
    out_a = torch.empty((n, ho, wo, ca), dtype=x.dtype, device=x.device)
    out_b = torch.empty((n, ho, wo, cb), dtype=x.dtype, device=x.device)
    p = _conv_params(n, hi, wi, cin, ho, wo, ca + cb, kh, kw, stride, pad, x.dtype, x.dtype)
    st = lib.osr_conv2d_fwd_pair(C.byref(p), _p(x), _p(w_a), _p(b_a), ca, int(relu_a), _p(out_a), _p(w_b), _p(b_b), cb, int(relu_b), _p(out_b), _stream())
    if st == _lib.ERR_UNSUPPORTED:
        return None
    check(st, "osr_conv2d_fwd_pair")
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * ho * wo * (ca + cb) * kh * kw * cin
    return out_a, out_b


def _conv_levels(xs: Sequence[torch.Tensor], outs, deltas=None, ctrs=None, weights=None, biases=None):
    assert 1 <= len(xs) <= _lib.MAX_CONV_LEVELS
    arr = (_lib.ConvLevel * len(xs))()
    for i, x in enumerate(xs):
        n, hi, wi, _ = x.shape
        arr[i].in_ = x.data_ptr()
        arr[i].out = outs[i].data_ptr() if outs is not None and outs[i] is not None else None
        arr[i].deltas = deltas[i].data_ptr() if deltas is not None else None
        arr[i].ctr = ctrs[i].data_ptr() if ctrs is not None else None
        arr[i].weight = weights[i].data_ptr() if weights is not None else None
        arr[i].bias = biases[i].data_ptr() if biases is not None else None
        arr[i].n, arr[i].hi, arr[i].wi = n, hi, wi
    return arr


def _levels_params(x0: torch.Tensor, weight: torch.Tensor, relu: bool):
    cout, kh, kw, cin = weight.shape
    assert kh == kw and kh % 2 == 1 and x0.shape[3] == cin
    p = _new_conv_params()
    p.cin, p.cout, p.kh, p.kw, p.stride_h, p.stride_w, p.pad_h, p.pad_w = cin, cout, kh, kw, 1, 1, kh // 2, kw // 2
    p.in_stride_w, p.out_stride_w = cin, cout
    p.relu, p.res_mode, p.pad_mode = 1 if relu else 0, 0, 0
    p.in_dtype = p.out_dtype = _DT[x0.dtype]
    return p


def conv2d_levels(xs: Sequence[torch.Tensor], weight, bias, relu: bool = False, outs: Optional[Sequence[torch.Tensor]] = None):
    """Stride-1, same-padding convolutions of one shape on several NHWC feature maps in ONE launch (osr_conv2d_fwd_levels: the FPN's output
    convs). weight / bias: one tensor shared by all levels, or a list with one per level. Returns the list of outputs, or None when the
    shape is outside the launch's envelope (cout % 256, cin % 64, f16 / bf16): the caller then runs conv2d per level."""
    lib = _lib.load()
    ws = list(weight) if isinstance(weight, (list, tuple)) else None
    bs = list(bias) if isinstance(bias, (list, tuple)) else None
    w0 = ws[0] if ws is not None else weight
    cout, kh, kw, cin = w0.shape
    if cout % 256 or cin % 64 or kh != kw or kh % 2 == 0 or kh * kw * cin // 64 < 2 or xs[0].dtype not in (torch.float16, torch.bfloat16) or len(xs) > _lib.MAX_CONV_LEVELS:
        return None
    assert (ws is None) == (bs is None) and (ws is None or (len(ws) == len(xs) and len(bs) == len(xs)))
    for w_, b_ in zip(ws if ws is not None else [weight], bs if bs is not None else [bias]):
        _need(w_, xs[0].dtype, "weight"); _need(b_, torch.float32, "bias")
        assert tuple(w_.shape) == (cout, kh, kw, cin) and b_.numel() == cout
    for x in xs:
        _need(x, xs[0].dtype, "x")
        assert x.shape[3] == cin
    if outs is None:
        outs = [torch.empty(tuple(x.shape[:3]) + (cout,), dtype=x.dtype, device=x.device) for x in xs]
    for x, o in zip(xs, outs):
        _need(o, x.dtype, "out")
        assert tuple(o.shape) == tuple(x.shape[:3]) + (cout,)
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += sum(2.0 * x.shape[0] * x.shape[1] * x.shape[2] * cout * kh * kw * cin for x in xs)
    p = _levels_params(xs[0], w0, relu)
    arr = _conv_levels(xs, outs, weights=ws, biases=bs)
    st = lib.osr_conv2d_fwd_levels(C.byref(p), len(xs), arr, None if ws is not None else _p(weight), None if bs is not None else _p(bias), _stream())
    if st == _lib.ERR_UNSUPPORTED:
        return None
    check(st, "osr_conv2d_fwd_levels")
    return list(outs)


def cfrpn_head_fused_levels(xs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, w_tail: torch.Tensor, b_tail: torch.Tensor,
                            deltas_outs: Sequence[torch.Tensor], ctr_outs: Sequence[torch.Tensor],
                            hidden_outs: Optional[Sequence[Optional[torch.Tensor]]] = None) -> bool:
    """ClsFreeRPNHead.forward over all the given levels in ONE launch (osr_cfrpn_head_fwd_levels). deltas_outs[i] (n*h*w, 4) / ctr_outs[i]
    (n*h*w) fp32 receive level i's outputs (views of the level-major buffers rpn_select reads). Returns False -- nothing launched -- outside
    the fused kernel's envelope."""
    lib = _lib.load()
    cout, kh, kw, cin = weight.shape
    if cout != 256 or cin % 64 or kh != kw or kh % 2 == 0 or kh * kw * cin // 64 < 8 or xs[0].dtype not in (torch.float16, torch.bfloat16) or len(xs) > _lib.MAX_CONV_LEVELS:
        return False
    _need(weight, xs[0].dtype, "weight"); _need(bias, torch.float32, "bias")
    _need(w_tail, torch.float32, "w_tail"); _need(b_tail, torch.float32, "b_tail")
    for i, x in enumerate(xs):
        _need(x, xs[0].dtype, "x")
        rows = x.shape[0] * x.shape[1] * x.shape[2]
        _need(deltas_outs[i], torch.float32, "deltas"); _need(ctr_outs[i], torch.float32, "ctr")
        assert deltas_outs[i].numel() == rows * 4 and ctr_outs[i].numel() == rows and x.shape[3] == cin
        if hidden_outs is not None and hidden_outs[i] is not None:
            _need(hidden_outs[i], x.dtype, "hidden_out")
            assert hidden_outs[i].numel() == rows * 256
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += sum(2.0 * x.shape[0] * x.shape[1] * x.shape[2] * cout * (kh * kw * cin + 5) for x in xs)
    p = _levels_params(xs[0], weight, True)
    arr = _conv_levels(xs, hidden_outs, deltas_outs, ctr_outs)
    st = lib.osr_cfrpn_head_fwd_levels(C.byref(p), len(xs), arr, _p(weight), _p(bias), _p(w_tail), _p(b_tail), _stream())
    if st == _lib.ERR_UNSUPPORTED:
        return False
    check(st, "osr_cfrpn_head_fwd_levels")
    return True


def make_rpn_levels(shapes: Sequence[Tuple[int, int]], strides: Sequence[int], n: int, num_anchors: int = 1) -> RpnLevels:
    lv = RpnLevels()
    lv.num_levels, lv.num_anchors = len(shapes), num_anchors
    off = 0
    for i, ((h, w), s) in enumerate(zip(shapes, strides)):
        lv.h[i], lv.w[i], lv.stride[i], lv.offset[i] = h, w, s, off
        off += n * h * w * num_anchors
    return lv


def rpn_select(lv: RpnLevels, cell_anchors: torch.Tensor, ctr: torch.Tensor, deltas: torch.Tensor, n: int,
               image_hw: torch.Tensor, pre_nms_topk: int, min_box_size: float = 0.0, b2b_weights: Optional[Sequence[float]] = None):
    """ctr/deltas: level-major concatenation (see osr.h). Returns dict of padded outputs. b2b_weights: decode with
    [d2] Box2BoxTransform(weights) instead of the CF-RPN's ltrb rule and also return the pyramid level of every slot (the stock
    RPN of Base-RCNN-FPN.yaml, osr_rpn_select_ex)."""
    if b2b_weights is not None:
        return _rpn_select_ex(lv, cell_anchors, ctr, deltas, n, image_hw, pre_nms_topk, min_box_size, b2b_weights)
    lib = _lib.load()
    _need(cell_anchors, torch.float32, "cell_anchors"); _need(ctr, torch.float32, "ctr"); _need(deltas, torch.float32, "deltas")
    _need(image_hw, torch.int32, "image_hw")
    cap = lib.osr_rpn_select_capacity(C.byref(lv), pre_nms_topk)
    if cap < 0:
        check(cap, "osr_rpn_select_capacity")
    wsb = lib.osr_rpn_select_workspace_bytes(C.byref(lv), n, pre_nms_topk)
    dev = ctr.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    boxes = torch.empty((n, cap, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
    src = torch.empty((n, cap), dtype=torch.int32, device=dev)
    bidx = torch.empty((n * cap,), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    check(lib.osr_rpn_select(C.byref(lv), _p(cell_anchors), _p(ctr), _p(deltas), n, _p(image_hw), pre_nms_topk, float(min_box_size),
                             _p(boxes), _p(scores), _p(src), _p(bidx), _p(counts), _p(flags), _p(ws), wsb, _stream()), "osr_rpn_select")
    return dict(boxes=boxes, scores=scores, src_index=src, batch_idx=bidx, counts=counts, status_flags=flags, cap=cap)


def _rpn_select_ex(lv, cell_anchors, ctr, deltas, n, image_hw, pre_nms_topk, min_box_size, weights):
    lib = _lib.load()
    _need(cell_anchors, torch.float32, "cell_anchors"); _need(ctr, torch.float32, "scores"); _need(deltas, torch.float32, "deltas")
    _need(image_hw, torch.int32, "image_hw")
    cap = lib.osr_rpn_select_capacity(C.byref(lv), pre_nms_topk)
    if cap < 0:
        check(cap, "osr_rpn_select_capacity")
    wsb = lib.osr_rpn_select_workspace_bytes(C.byref(lv), n, pre_nms_topk)
    dev = ctr.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    boxes = torch.empty((n, cap, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
    src = torch.empty((n, cap), dtype=torch.int32, device=dev)
    level = torch.empty((n, cap), dtype=torch.int32, device=dev)
    bidx = torch.empty((n * cap,), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    rw = (C.c_float * 4)(*[float(v) for v in weights])
    check(lib.osr_rpn_select_ex(C.byref(lv), _p(cell_anchors), _p(ctr), _p(deltas), n, _p(image_hw), pre_nms_topk, float(min_box_size), 1, rw,
                                _p(boxes), _p(scores), _p(src), _p(bidx), _p(level), _p(counts), _p(flags), _p(ws), wsb, _stream()), "osr_rpn_select_ex")
    return dict(boxes=boxes, scores=scores, src_index=src, batch_idx=bidx, level=level, counts=counts, status_flags=flags, cap=cap)


def rpn_select_wide(lv: RpnLevels, cell_anchors: torch.Tensor, ctr: torch.Tensor, deltas: torch.Tensor, n: int,
                    image_hw: torch.Tensor, pre_nms_topk: int, min_box_size: float = 0.0, b2b_weights: Optional[Sequence[float]] = None):
    """rpn_select with pre_nms_topk up to RPN_SELECT_WIDE_MAXK per level (osr_rpn_select_wide: the single-level C4 RPN keeps 6000).
    Same arguments, same dict; `level` is returned with b2b_weights as there. For pre_nms_topk <= RPN_SELECT_MAXK the outputs are
    bit-identical to rpn_select's."""
    lib = _lib.load()
    _need(cell_anchors, torch.float32, "cell_anchors"); _need(ctr, torch.float32, "scores"); _need(deltas, torch.float32, "deltas")
    _need(image_hw, torch.int32, "image_hw")
    cap = lib.osr_rpn_select_wide_capacity(C.byref(lv), pre_nms_topk)
    if cap < 0:
        check(cap, "osr_rpn_select_wide_capacity")
    wsb = lib.osr_rpn_select_wide_workspace_bytes(C.byref(lv), n, pre_nms_topk)
    dev = ctr.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    boxes = torch.empty((n, cap, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
    src = torch.empty((n, cap), dtype=torch.int32, device=dev)
    level = torch.empty((n, cap), dtype=torch.int32, device=dev) if b2b_weights is not None else None
    bidx = torch.empty((n * cap,), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    rw = (C.c_float * 4)(*[float(v) for v in b2b_weights]) if b2b_weights is not None else None
    check(lib.osr_rpn_select_wide(C.byref(lv), _p(cell_anchors), _p(ctr), _p(deltas), n, _p(image_hw), pre_nms_topk, float(min_box_size),
                                  0 if b2b_weights is None else 1, rw, _p(boxes), _p(scores), _p(src), _p(bidx), _p(level), _p(counts), _p(flags),
                                  _p(ws), wsb, _stream()), "osr_rpn_select_wide")
    out = dict(boxes=boxes, scores=scores, src_index=src, batch_idx=bidx, counts=counts, status_flags=flags, cap=cap)
    if level is not None:
        out["level"] = level
    return out


RPN_SELECT_MAXK, RPN_SELECT_WIDE_MAXK = _lib.RPN_SELECT_MAXK, _lib.RPN_SELECT_WIDE_MAXK


def retinanet_logit_thresh(score_thresh: float) -> float:
    """log(t / (1 - t)) in double, rounded once to fp32 (include/osr.h osr_retinanet_select: the candidates are `logit > this`)."""
    t = float(score_thresh)
    if t <= 0.0:
        return float("-inf")
    if t >= 1.0:
        return float("inf")
    return float(torch.tensor(math.log(t / (1.0 - t)), dtype=torch.float64).to(torch.float32))


def retinanet_select(lv: RpnLevels, cell_anchors: torch.Tensor, logits: torch.Tensor, deltas: torch.Tensor, n: int, num_classes: int, topk: int,
                     score_thresh: float, reg_weights: Sequence[float] = (1.0, 1.0, 1.0, 1.0), pitch_cls: Optional[int] = None,
                     pitch_box: Optional[int] = None, out: Optional[dict] = None):
    """[d2] RetinaNet.inference_single_image before its NMS (osr_retinanet_select, include/osr.h): logits / deltas are the level-major
    buffers with row pitches pitch_cls (default A*K) / pitch_box (default 4A). -> dict(c_boxes, c_scores, c_cls, c_cand, c_src, counts,
    status_flags, cap). `out`: a dict of these tensors to write into instead of fresh ones."""
    lib = _lib.load()
    a = lv.num_anchors
    pitch_cls = a * num_classes if pitch_cls is None else int(pitch_cls)
    pitch_box = 4 * a if pitch_box is None else int(pitch_box)
    _need(cell_anchors, torch.float32, "cell_anchors"); _need(logits, None, "logits"); _need(deltas, torch.float32, "deltas")
    if logits.dtype not in _DT:
        raise OsrError(f"logits must be float32 / float16 / bfloat16, got {logits.dtype}")
    cells = sum(n * lv.h[i] * lv.w[i] for i in range(lv.num_levels))
    if pitch_cls >= a * num_classes and pitch_box >= 4 * a and (logits.numel() < cells * pitch_cls or deltas.numel() < cells * pitch_box):
        raise OsrError(f"retinanet_select: logits ({logits.numel()}) / deltas ({deltas.numel()}) are shorter than {cells} cells x the pitches")
    if tuple(cell_anchors.shape) != (lv.num_levels, a, 4):
        raise OsrError(f"retinanet_select: cell_anchors {tuple(cell_anchors.shape)} != ({lv.num_levels}, {a}, 4)")
    cap = lib.osr_retinanet_select_capacity(C.byref(lv), topk)
    if cap < 0:
        check(cap, "osr_retinanet_select_capacity")
    wsb = lib.osr_retinanet_select_workspace_bytes(C.byref(lv), n, num_classes, topk)
    if wsb < 0:
        check(int(wsb), "osr_retinanet_select_workspace_bytes")
    dev = logits.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    if out is None:
        out = dict(c_boxes=torch.empty((n, cap, 4), dtype=torch.float32, device=dev), c_scores=torch.empty((n, cap), dtype=torch.float32, device=dev),
                   c_cls=torch.empty((n, cap), dtype=torch.int32, device=dev), c_cand=torch.empty((n, cap), dtype=torch.int32, device=dev),
                   c_src=torch.empty((n, cap), dtype=torch.int32, device=dev), counts=torch.empty((n, lv.num_levels), dtype=torch.int32, device=dev),
                   status_flags=torch.zeros((1,), dtype=torch.int32, device=dev))
    else:
        out = dict(out)
        for key, dt in (("c_boxes", torch.float32), ("c_scores", torch.float32), ("c_cls", torch.int32), ("c_cand", torch.int32), ("c_src", torch.int32),
                        ("counts", torch.int32), ("status_flags", torch.int32)):
            _need(out[key], dt, key)
        assert out["c_boxes"].numel() == n * cap * 4 and out["c_scores"].numel() == n * cap and out["counts"].numel() == n * lv.num_levels
    rw = (C.c_float * 4)(*[float(v) for v in reg_weights])
    check(lib.osr_retinanet_select(C.byref(lv), _p(cell_anchors), _p(logits), _DT[logits.dtype], pitch_cls, _p(deltas), pitch_box, n, num_classes, topk,
                                   retinanet_logit_thresh(score_thresh), rw, _p(out["c_boxes"]), _p(out["c_scores"]), _p(out["c_cls"]), _p(out["c_cand"]),
                                   _p(out["c_src"]), _p(out["counts"]), _p(out["status_flags"]), _p(ws), wsb, _stream()), "osr_retinanet_select")
    out["cap"] = cap
    return out


def fastrcnn_candidates(logits, deltas, prop_boxes, prop_count, image_hw, num_classes: int, reg_weights=(10.0, 10.0, 5.0, 5.0),
                        score_thresh: float = 0.05):
    """[d2] fast_rcnn_inference_single_image before its NMS. logits (n*rows, K+1), deltas (n*rows, K*4 or 4), prop_boxes (n,rows,4)."""
    lib = _lib.load()
    _need(logits, torch.float32, "logits"); _need(deltas, torch.float32, "deltas"); _need(prop_boxes, torch.float32, "prop_boxes")
    _need(prop_count, torch.int32, "prop_count"); _need(image_hw, torch.int32, "image_hw")
    n, rows = prop_boxes.shape[0], prop_boxes.shape[1]
    kbox = deltas.shape[1] // 4
    if logits.shape != (n * rows, num_classes + 1) or deltas.shape[0] != n * rows or kbox not in (1, num_classes):
        raise OsrError(f"fastrcnn_candidates: logits {tuple(logits.shape)} / deltas {tuple(deltas.shape)} do not fit {n} x {rows} rows, {num_classes} classes")
    dev, cap = logits.device, rows * num_classes
    o = dict(boxes=torch.empty((n, cap, 4), dtype=torch.float32, device=dev), scores=torch.empty((n, cap), dtype=torch.float32, device=dev),
             cls=torch.empty((n, cap), dtype=torch.int32, device=dev), row=torch.empty((n, cap), dtype=torch.int32, device=dev),
             count=torch.empty((n,), dtype=torch.int32, device=dev), cap=cap)
    rw = (C.c_float * 4)(*[float(v) for v in reg_weights])
    check(lib.osr_fastrcnn_candidates(_p(logits), _p(deltas), num_classes, kbox, _p(prop_boxes), _p(prop_count), n, rows, _p(image_hw), rw,
                                      float(score_thresh), _p(o["boxes"]), _p(o["scores"]), _p(o["cls"]), _p(o["row"]), _p(o["count"]), _stream()),
          "osr_fastrcnn_candidates")
    return o


CASCADE_MAX_STAGES = 4   # include/osr.h OSR_CASCADE_MAX_STAGES
CASCADE_MAX_GT = 1024    # csrc/osr_cascade.hip CR_MAX_GT: an image's ground truth in the refine kernel's LDS table


def cascade_refine(boxes, batch_idx, deltas, n: int, image_hw, reg_weights, drop_empty: bool = False, gt_boxes=None, gt_classes=None,
                   gt_count=None, num_classes: int = 0, iou_thr: float = 0.5):
    """[d2] CascadeROIHeads between two stages (include/osr.h osr_cascade_refine): boxes (m,4) fp32, batch_idx (m) int32 (-1: the row
    does not exist), deltas (m,4) class-agnostic, m = n x rows per image. -> dict(boxes (m,4), batch_idx (m), counts (n,3) = {rows,
    foreground, background}); with ground truth (gt_boxes (n,gmax,4), gt_classes (n,gmax) int64, gt_count (n) int32) also gt_classes (m)
    int64 (-1: no row), gt_boxes (m,4) the matched box, gt_idx (m) int32 (-1 off foreground)."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(batch_idx, torch.int32, "batch_idx"); _need(deltas, torch.float32, "deltas")
    _need(image_hw, torch.int32, "image_hw")
    m, dev = batch_idx.numel(), boxes.device
    if n < 1 or m % n or m == 0 or boxes.numel() != m * 4 or tuple(deltas.shape) != (m, 4) or image_hw.numel() != 2 * n:
        raise OsrError(f"cascade_refine: boxes {tuple(boxes.shape)} / deltas {tuple(deltas.shape)} / batch_idx {tuple(batch_idx.shape)} do not fit "
                       f"{n} images (class-agnostic deltas (m,4), m a multiple of n)")
    o = dict(boxes=torch.empty((m, 4), dtype=torch.float32, device=dev), batch_idx=torch.empty((m,), dtype=torch.int32, device=dev),
             counts=torch.empty((n, 3), dtype=torch.int32, device=dev))
    gmax = 0
    if gt_boxes is not None:
        _need(gt_boxes, torch.float32, "gt_boxes"); _need(gt_classes, torch.int64, "gt_classes"); _need(gt_count, torch.int32, "gt_count")
        gmax = gt_boxes.shape[1]
        if gt_boxes.shape[0] != n or tuple(gt_classes.shape) != (n, gmax) or gt_count.numel() != n:
            raise OsrError(f"cascade_refine: ground truth {tuple(gt_boxes.shape)} / {tuple(gt_classes.shape)} does not fit {n} images")
        o.update(gt_classes=torch.empty((m,), dtype=torch.int64, device=dev), gt_boxes=torch.empty((m, 4), dtype=torch.float32, device=dev),
                 gt_idx=torch.empty((m,), dtype=torch.int32, device=dev))
    check(lib.osr_cascade_refine(_p(boxes), _p(batch_idx), _p(deltas), n, m // n, _p(image_hw), _f4(reg_weights), int(bool(drop_empty)),
                                 _p(gt_boxes), _p(gt_classes), _p(gt_count), gmax, int(num_classes), float(iou_thr), _p(o["boxes"]),
                                 _p(o["batch_idx"]), _p(o.get("gt_classes")), _p(o.get("gt_boxes")), _p(o.get("gt_idx")), _p(o["counts"]),
                                 _stream()), "osr_cascade_refine")
    return o


def cascade_candidates(logits: Sequence[torch.Tensor], deltas, boxes, batch_idx, image_hw, num_classes: int, reg_weights=(30.0, 30.0, 15.0, 15.0),
                       score_thresh: float = 0.05):
    """[d2] CascadeROIHeads._forward_box at inference up to the NMS (include/osr.h osr_cascade_candidates): logits[s] (n*rows, K+1)
    per stage, the last stage's deltas (n*rows, 4) and input boxes (n, rows, 4), batch_idx (n*rows) int32. The outputs of
    fastrcnn_candidates; with one stage it is the same kernel instantiation."""
    lib = _lib.load()
    logits = list(logits)
    if not 1 <= len(logits) <= CASCADE_MAX_STAGES:
        raise OsrError(f"cascade_candidates: 1 .. {CASCADE_MAX_STAGES} stages, got {len(logits)}")
    for s, l in enumerate(logits):
        _need(l, torch.float32, f"logits[{s}]")
    _need(deltas, torch.float32, "deltas"); _need(boxes, torch.float32, "boxes"); _need(batch_idx, torch.int32, "batch_idx")
    _need(image_hw, torch.int32, "image_hw")
    n, rows = boxes.shape[0], boxes.shape[1]
    if any(tuple(l.shape) != (n * rows, num_classes + 1) for l in logits) or tuple(deltas.shape) != (n * rows, 4) or batch_idx.numel() != n * rows:
        raise OsrError(f"cascade_candidates: logits {[tuple(l.shape) for l in logits]} / deltas {tuple(deltas.shape)} do not fit {n} x {rows} rows, "
                       f"{num_classes} classes, class-agnostic deltas")
    dev, cap = deltas.device, rows * num_classes
    o = dict(boxes=torch.empty((n, cap, 4), dtype=torch.float32, device=dev), scores=torch.empty((n, cap), dtype=torch.float32, device=dev),
             cls=torch.empty((n, cap), dtype=torch.int32, device=dev), row=torch.empty((n, cap), dtype=torch.int32, device=dev),
             count=torch.empty((n,), dtype=torch.int32, device=dev), cap=cap)
    ptrs = (C.c_void_p * len(logits))(*[l.data_ptr() for l in logits])
    check(lib.osr_cascade_candidates(ptrs, len(logits), _p(deltas), num_classes, _p(boxes), _p(batch_idx), n, rows, _p(image_hw), _f4(reg_weights),
                                     float(score_thresh), _p(o["boxes"]), _p(o["scores"]), _p(o["cls"]), _p(o["row"]), _p(o["count"]), _stream()),
          "osr_cascade_candidates")
    return o


def _pyramid(feats, scales) -> "Pyramid":
    py = Pyramid()
    py.num_levels, py.c = len(feats), feats[0].shape[3]
    for i, (f, s) in enumerate(zip(feats, scales)):
        _need(f, feats[0].dtype, f"feats[{i}]")
        py.h[i], py.w[i], py.scale[i], py.data[i] = f.shape[1], f.shape[2], float(s), f.data_ptr()
    return py


# RoIAlign pools the RoIs in locality order (osr_roi_locality_order) unless told otherwise: same output bits, ~8x fewer re-reads
# from HBM than the score order the proposal lists arrive in.
ROI_LOCALITY_ORDER = True


def roi_locality_order(feats: List[torch.Tensor], scales: Sequence[float], boxes: torch.Tensor, batch_idx: torch.Tensor,
                       canonical_level: int = 4, canonical_size: int = 224, min_level: int = 2) -> torch.Tensor:
    """(m + 1,) int32: a permutation of the RoI list that puts RoIs of one image / level / 32-pixel tile next to each other, padding
    rows (batch index -1) last, followed by one more entry: the number of non-padding rows."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(batch_idx, torch.int32, "batch_idx")
    py = _pyramid(feats, scales)
    m, n = boxes.shape[0], feats[0].shape[0]
    order = torch.empty((m + 1,), dtype=torch.int32, device=boxes.device)
    nb = int(lib.osr_roi_locality_order_workspace_bytes(n, m))
    ws = torch.empty((max(nb, 4),), dtype=torch.uint8, device=boxes.device)
    check(lib.osr_roi_locality_order(C.byref(py), n, _p(boxes), _p(batch_idx), m, canonical_level, canonical_size, min_level, _p(order),
                                     C.c_void_p(order.data_ptr() + 4 * m), _p(ws), nb, _stream()), "osr_roi_locality_order")
    return order


MAX_SAMPLING_RATIO = 64  # include/osr.h OSR_ROI_MAX_SAMPLING_RATIO
MAX_POOLED_FWD = 14      # include/osr.h OSR_ROI_MAX_POOLED_FWD (the scatter backward too; the pixel-centric backward takes 1..7)


def check_pooler_options(aligned, sampling_ratio) -> Tuple[bool, int]:
    """The pooler options the RoIAlign kernels implement, as (aligned, sampling_ratio); ValueError for anything else."""
    if not isinstance(aligned, (bool, int)) or aligned not in (0, 1):
        raise ValueError(f"RoIAlign: aligned must be True (POOLER_TYPE 'ROIAlignV2') or False ('ROIAlign'), got {aligned!r}")
    if isinstance(sampling_ratio, bool) or not isinstance(sampling_ratio, int) or not 0 <= sampling_ratio <= MAX_SAMPLING_RATIO:
        raise ValueError(f"RoIAlign: sampling_ratio must be an integer 0 .. {MAX_SAMPLING_RATIO} (0 = adaptive grid, S > 0 = S x S samples per bin), "
                         f"got {sampling_ratio!r}")
    return bool(aligned), int(sampling_ratio)


def _roi_options(aligned, sampling_ratio):
    aligned, sampling_ratio = check_pooler_options(aligned, sampling_ratio)
    return C.byref(_lib.RoiOptions(int(aligned), sampling_ratio))


def roi_align(feats: List[torch.Tensor], scales: Sequence[float], boxes: torch.Tensor, batch_idx: torch.Tensor,
              pooled: int = 7, out_dtype: Optional[torch.dtype] = None, canonical_level: int = 4, canonical_size: int = 224,
              min_level: int = 2, order: Optional[torch.Tensor] = None, fill_padding: bool = True, aligned: bool = True,
              sampling_ratio: int = 0, bin_stride: int = 1) -> torch.Tensor:
    """feats: NHWC per level; boxes (m,4) fp32; batch_idx (m) int32. Returns (m, pooled, pooled, c), pooled 1 .. MAX_POOLED_FWD. order: processing order, (m,)
    int32 or (m + 1,) as roi_locality_order returns it (None: that order when ROI_LOCALITY_ORDER, else list order); the result
    does not depend on it. fill_padding=False: the rows of padding entries (batch index -1) are left unwritten instead of zeroed.
    aligned / sampling_ratio: torchvision roi_align's (include/osr.h osr_roi_options); the defaults are POOLER_TYPE "ROIAlignV2" with
    the adaptive grid, aligned=False is "ROIAlign", sampling_ratio=S > 0 a fixed S x S grid per bin.
    bin_stride=2 (pooled 8 .. MAX_POOLED_FWD): only the bins at even positions are pooled, into (m, q, q, c) with q = ceil(pooled / 2),
    each bit-identical to the full grid's (osr_roi_align_fwd_strided: what a stride-2 1 x 1 convolution reads of the grid)."""
    lib = _lib.load()
    opt = _roi_options(aligned, sampling_ratio)
    _need(boxes, torch.float32, "boxes"); _need(batch_idx, torch.int32, "batch_idx")
    py = _pyramid(feats, scales)
    m = boxes.shape[0]
    if order is None and ROI_LOCALITY_ORDER and m > 0:
        order = roi_locality_order(feats, scales, boxes, batch_idx, canonical_level, canonical_size, min_level)
    nvalid = None
    if order is not None:
        _need(order, torch.int32, "order")
        assert order.numel() in (m, m + 1)
        if order.numel() == m + 1:
            nvalid = C.c_void_p(order.data_ptr() + 4 * m)
    out_dtype = out_dtype or feats[0].dtype
    if bin_stride != 1:
        if isinstance(bin_stride, bool) or not isinstance(bin_stride, int) or bin_stride < 1:
            raise ValueError(f"RoIAlign: bin_stride must be a positive integer, got {bin_stride!r}")
        q = -(-pooled // bin_stride)
        out = torch.empty((m, q, q, py.c), dtype=out_dtype, device=boxes.device)
        check(lib.osr_roi_align_fwd_strided(C.byref(py), _DT[feats[0].dtype], feats[0].shape[0], _p(boxes), _p(batch_idx), m, pooled, bin_stride,
                                            canonical_level, canonical_size, min_level, _p(order), nvalid, 0 if fill_padding else 1, opt,
                                            _p(out), _DT[out_dtype], _stream()), "osr_roi_align_fwd_strided")
        return out
    out = torch.empty((m, pooled, pooled, py.c), dtype=out_dtype, device=boxes.device)
    check(lib.osr_roi_align_fwd_ordered_opt(C.byref(py), _DT[feats[0].dtype], feats[0].shape[0], _p(boxes), _p(batch_idx), m, pooled,
                                            canonical_level, canonical_size, min_level, _p(order), nvalid, 0 if fill_padding else 1, opt,
                                            _p(out), _DT[out_dtype], _stream()), "osr_roi_align_fwd")
    return out


def box_predictor_tail(x, w, b, proposals, ctr, batch_idx, image_hw, reg_weights=(10.0, 10.0, 5.0, 5.0), mean_type=0,
                       score_thresh=0.05):
    lib = _lib.load()
    for t, nme in ((x, "x"), (w, "w"), (b, "b"), (proposals, "proposals"), (ctr, "ctr")):
        _need(t, torch.float32, nme)
    _need(batch_idx, torch.int32, "batch_idx"); _need(image_hw, torch.int32, "image_hw")
    m, k = x.shape
    dev = x.device
    pd = torch.empty((m, 4), dtype=torch.float32, device=dev)
    pi = torch.empty((m,), dtype=torch.float32, device=dev)
    bx = torch.empty((m, 4), dtype=torch.float32, device=dev)
    sc = torch.empty((m,), dtype=torch.float32, device=dev)
    cd = torch.empty((m,), dtype=torch.int32, device=dev)
    rw = (C.c_float * 4)(*[float(v) for v in reg_weights])
    check(lib.osr_box_predictor_tail(_p(x), m, k, _p(w), _p(b), _p(proposals), _p(ctr), _p(batch_idx), _p(image_hw), rw, mean_type,
                                     float(score_thresh), _p(pd), _p(pi), _p(bx), _p(sc), _p(cd), _stream()), "osr_box_predictor_tail")
    return dict(pred_deltas=pd, pred_iou=pi, boxes=bx, score=sc, cand=cd)


def nms_topk(boxes, scores, cls, cand, num_segments: int, seg_stride: int, seg_len, thr: float, topk: int):
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(seg_len, torch.int32, "seg_len")
    if cls is not None:
        _need(cls, torch.int32, "cls")
    if cand is not None:
        _need(cand, torch.int32, "cand")
    dev = boxes.device
    wsb = lib.osr_nms_topk_workspace_bytes(num_segments, seg_stride)
    if wsb < 0:
        check(int(wsb), "osr_nms_topk_workspace_bytes")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    keep = torch.empty((num_segments, topk), dtype=torch.int32, device=dev)
    cnt = torch.empty((num_segments,), dtype=torch.int32, device=dev)
    check(lib.osr_nms_topk(_p(boxes), _p(scores), _p(cls), _p(cand), num_segments, seg_stride, _p(seg_len), float(thr), topk, _p(keep),
                           _p(cnt), _p(ws), wsb, _stream()), "osr_nms_topk")
    return keep, cnt


def gather_rows(src, seg_stride: int, keep, keep_count) -> torch.Tensor:
    lib = _lib.load()
    _need(src, torch.float32, "src"); _need(keep, torch.int32, "keep"); _need(keep_count, torch.int32, "keep_count")
    nseg, topk = keep.shape
    row = src.shape[-1] if src.dim() > 1 else 1
    dst = torch.empty((nseg, topk, row), dtype=torch.float32, device=src.device)
    check(lib.osr_gather_rows(_p(src), seg_stride, row, _p(keep), _p(keep_count), nseg, topk, _p(dst), _stream()), "osr_gather_rows")
    return dst


def padded_batch_idx(counts: torch.Tensor, width: int) -> torch.Tensor:
    """batch_idx (n * width,) int32 of n padded lists of `width` slots: image i in its first counts[i] slots, -1 behind them."""
    n, dev = counts.numel(), counts.device
    ar = torch.arange(width, device=dev, dtype=torch.int32)[None, :]
    return torch.where(ar < counts.view(n, 1), torch.arange(n, device=dev, dtype=torch.int32)[:, None],
                       torch.full((1, 1), -1, device=dev, dtype=torch.int32)).reshape(-1).contiguous()


def nms_gather(boxes, scores, cls, cand, n: int, cap: int, counts, thresh: float, topk: int, timed=None):
    """The tail behind a candidate list ([d2] batched_nms by class + the best `topk`): one nms_topk over n segments of `cap` candidates
    (boxes (n, cap, 4), scores, cls int32, cand int32 flags or None, counts (n,) int32), then the kept boxes, scores and classes
    gathered into padded lists. -> (boxes (n, topk, 4), scores (n, topk), classes (n, topk) int64 with -1 behind the count, counts,
    keep). timed: a callable that runs the NMS launch (an engine's profiling wrapper); None calls it directly."""
    nms = lambda: nms_topk(boxes, scores, cls, cand, n, cap, counts, thresh, topk)  # noqa: E731
    keep, cnt = timed(nms) if timed is not None else nms()
    ob = gather_rows(boxes.view(-1, 4), cap, keep, cnt)
    osc = gather_rows(scores.view(-1), cap, keep, cnt).view(n, topk)
    # (class ids travel through the fp32 row gather as bit patterns: it only copies)
    ocl = gather_rows(cls.view(-1).view(torch.float32), cap, keep, cnt).view(n, topk).view(torch.int32).to(torch.int64)
    ocl = torch.where(torch.arange(topk, device=ocl.device)[None, :] < cnt[:, None], ocl, torch.full_like(ocl, -1))
    return ob, osc, ocl, cnt, keep


def l2_normalize_rows(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, torch.float32, "x")
    out = torch.empty_like(x)
    check(lib.osr_l2_normalize_rows(_p(x), x.shape[0], x.shape[1], _p(out), _stream()), "osr_l2_normalize_rows")
    return out


def _pln_distance(name: str) -> int:
    if name not in _lib.PLN_DISTANCES:
        raise OsrError(f"MODEL.PLN.DISTANCE_TYPE '{name}': one of {sorted(_lib.PLN_DISTANCES)}")
    return _lib.PLN_DISTANCES[name]


def pln_tail(emb, protos_normed, num_known: int, reps: int, unk_thr: float, unknown_id: int, class_map=None, rows_valid=None,
             seg_rows: int = 0, distance: str = "COS"):
    lib = _lib.load()
    _need(emb, torch.float32, "emb"); _need(protos_normed, torch.float32, "protos")
    if class_map is not None:
        _need(class_map, torch.int64, "class_map")
    if rows_valid is not None:
        _need(rows_valid, torch.int32, "rows_valid")
    rows, d = emb.shape
    pc = torch.empty((rows,), dtype=torch.int64, device=emb.device)
    md = torch.empty((rows,), dtype=torch.float32, device=emb.device)
    check(lib.osr_pln_tail_ex(_p(emb), rows, d, _p(protos_normed), num_known, reps, _pln_distance(distance), float(unk_thr), int(unknown_id),
                              _p(class_map), _p(rows_valid), seg_rows, _p(pc), _p(md), _stream()), "osr_pln_tail")
    return pc, md


def softmax_candidates(logits, num_known, det_boxes, det_scores, pred_class, det_count, n, seg_rows, unknown_id, known_thresh,
                       unknown_thresh):
    lib = _lib.load()
    _need(logits, torch.float32, "logits"); _need(det_boxes, torch.float32, "det_boxes"); _need(det_scores, torch.float32, "det_scores")
    _need(pred_class, torch.int64, "pred_class"); _need(det_count, torch.int32, "det_count")
    dev = logits.device
    kcap = seg_rows * num_known
    o = dict(
        k_boxes=torch.empty((n, kcap, 4), dtype=torch.float32, device=dev), k_scores=torch.empty((n, kcap), dtype=torch.float32, device=dev),
        k_cls=torch.empty((n, kcap), dtype=torch.int32, device=dev), k_det=torch.empty((n, kcap), dtype=torch.int32, device=dev),
        k_count=torch.empty((n,), dtype=torch.int32, device=dev),
        u_boxes=torch.empty((n, seg_rows, 4), dtype=torch.float32, device=dev), u_scores=torch.empty((n, seg_rows), dtype=torch.float32, device=dev),
        u_det=torch.empty((n, seg_rows), dtype=torch.int32, device=dev), u_count=torch.empty((n,), dtype=torch.int32, device=dev))
    check(lib.osr_softmax_candidates(_p(logits), num_known, _p(det_boxes), _p(det_scores), _p(pred_class), _p(det_count), n, seg_rows,
                                     int(unknown_id), float(known_thresh), float(unknown_thresh), _p(o["k_boxes"]), _p(o["k_scores"]),
                                     _p(o["k_cls"]), _p(o["k_det"]), _p(o["k_count"]), _p(o["u_boxes"]), _p(o["u_scores"]), _p(o["u_det"]),
                                     _p(o["u_count"]), _stream()), "osr_softmax_candidates")
    return o


def assemble_detections(cands, k_keep, k_keep_count, u_keep, u_keep_count, n, unknown_id, class_map=None):
    lib = _lib.load()
    k_topk, u_topk = k_keep.shape[1], u_keep.shape[1]
    dev = k_keep.device
    cap = k_topk + u_topk
    ob = torch.empty((n, cap, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((n, cap), dtype=torch.float32, device=dev)
    oc = torch.empty((n, cap), dtype=torch.int64, device=dev)
    on = torch.empty((n,), dtype=torch.int32, device=dev)
    check(lib.osr_assemble_detections(_p(cands["k_boxes"]), _p(cands["k_scores"]), _p(cands["k_cls"]), _p(k_keep), _p(k_keep_count),
                                      cands["k_boxes"].shape[1], k_topk, _p(cands["u_boxes"]), _p(cands["u_scores"]), _p(u_keep),
                                      _p(u_keep_count), cands["u_boxes"].shape[1], u_topk, n, int(unknown_id), _p(class_map), _p(ob),
                                      _p(os_), _p(oc), _p(on), _stream()), "osr_assemble_detections")
    return ob, os_, oc, on


def detector_postprocess(boxes, scores, classes, count, scale_xy, out_hw):
    """Padded (n,cap,.) detections -> rescaled, clipped, empties dropped (order kept); scale_xy (n,2) fp32, out_hw (n,2) int32."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes")
    _need(count, torch.int32, "count"); _need(scale_xy, torch.float32, "scale_xy"); _need(out_hw, torch.int32, "out_hw")
    n, cap = scores.shape
    ob, os_, oc = torch.empty_like(boxes), torch.empty_like(scores), torch.empty_like(classes)
    on = torch.empty_like(count)
    check(lib.osr_detector_postprocess(_p(boxes), _p(scores), _p(classes), _p(count), n, cap, _p(scale_xy), _p(out_hw), _p(ob), _p(os_), _p(oc),
                                       _p(on), _stream()), "osr_detector_postprocess")
    return ob, os_, oc, on


def mask_upsample_predict(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, pred_w: torch.Tensor, pred_b: torch.Tensor,
                          classes: Optional[torch.Tensor] = None, rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0) -> torch.Tensor:
    """[d2] MaskRCNNConvUpsampleHead's deconv (2 x 2, stride 2) + ReLU + 1 x 1 predictor and mask_rcnn_inference's sigmoid of each RoI's
    class row, one launch. x (r, s, s, cin) NHWC; w_packed: weights.pack_deconv_weight in x's dtype; bias (cmid), pred_w (k, cmid),
    pred_b (k) fp32; classes (r) int64 (may be None when k == 1: class-agnostic); rows_valid (segments) int32 with seg_rows RoIs per
    segment: the RoIs beyond a segment's count, and those with class -1, come out as zeros. Returns probs (r, 2s, 2s) fp32."""
    lib = _lib.load()
    _need(x, name="x"); _need(w_packed, x.dtype, "w_packed")
    for t, nme in ((bias, "bias"), (pred_w, "pred_w"), (pred_b, "pred_b")):
        _need(t, torch.float32, nme)
    r, s, s2, cin = x.shape
    k, cmid = pred_w.shape
    if s != s2 or bias.numel() != cmid or pred_b.numel() != k or w_packed.numel() != 4 * cin * cmid:
        raise OsrError(f"mask_upsample_predict: x {tuple(x.shape)}, bias {tuple(bias.shape)}, pred_w {tuple(pred_w.shape)}, pred_b {tuple(pred_b.shape)}, "
                       f"w_packed {tuple(w_packed.shape)} do not fit together")
    if classes is not None:
        _need(classes, torch.int64, "classes")
        if classes.numel() != r:
            raise OsrError(f"mask_upsample_predict: {classes.numel()} classes for {r} RoIs")
    if rows_valid is not None:
        _need(rows_valid, torch.int32, "rows_valid")
        if seg_rows < 1 or rows_valid.numel() * seg_rows < r:
            raise OsrError("mask_upsample_predict: rows_valid does not cover the RoIs")
    probs = torch.empty((r, 2 * s, 2 * s), dtype=torch.float32, device=x.device)
    check(lib.osr_mask_upsample_predict(_p(x), _DT[x.dtype], r, s, cin, cmid, _p(w_packed), _p(bias), _p(pred_w), _p(pred_b), k, _p(classes),
                                        _p(rows_valid), int(seg_rows), _p(probs), _stream()), "osr_mask_upsample_predict")
    return probs


def avgpool_rows(x: torch.Tensor, rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0) -> torch.Tensor:
    """[d2] Res5ROIHeads' box_features.mean(dim=[2, 3]) on channels-last rows (include/osr.h osr_avgpool_rows). x (r, s, c) or
    (r, h, w, c); returns (r, c) fp32 = the fp32 sum over the positions in ascending order / their number. rows_valid (segments) int32
    with seg_rows RoIs per segment: the RoIs beyond a segment's count come out as zeros."""
    lib = _lib.load()
    _need(x, name="x")
    if x.dim() not in (3, 4):
        raise OsrError(f"avgpool_rows: x {tuple(x.shape)} is not (r, s, c) or (r, h, w, c)")
    r, c = x.shape[0], x.shape[-1]
    s = x.shape[1] if x.dim() == 3 else x.shape[1] * x.shape[2]
    _rows_valid_arg(rows_valid, seg_rows, r, "avgpool_rows")
    out = torch.empty((r, c), dtype=torch.float32, device=x.device)
    check(lib.osr_avgpool_rows(_p(x), _DT[x.dtype], r, s, c, _p(rows_valid), int(seg_rows), _p(out), _stream()), "osr_avgpool_rows")
    return out


def _rows_valid_arg(rows_valid, seg_rows, r, name):
    if rows_valid is not None:
        _need(rows_valid, torch.int32, "rows_valid")
        if seg_rows < 1 or rows_valid.numel() * seg_rows < r:
            raise OsrError(f"{name}: rows_valid does not cover the RoIs")


def keypoint_upsample(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, rows_valid: Optional[torch.Tensor] = None,
                      seg_rows: int = 0) -> torch.Tensor:
    """[d2] KRCNNConvDeconvUpsampleHead's tail in one launch (include/osr.h osr_keypoint_upsample): score_lowres =
    ConvTranspose2d(cin -> k, 4 x 4, stride 2, padding 1) and the bilinear x2 (align_corners=False). x (r, s, s, cin) NHWC; w_packed:
    weights.pack_keypoint_deconv_weight in x's dtype; bias (k) fp32; rows_valid (segments) int32 with seg_rows RoIs per segment: the
    RoIs beyond a segment's count come out as zeros. Returns heatmaps (r, k, 4s, 4s) fp32."""
    lib = _lib.load()
    _need(x, name="x"); _need(w_packed, x.dtype, "w_packed"); _need(bias, torch.float32, "bias")
    if x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise OsrError(f"keypoint_upsample: x {tuple(x.shape)} is not (r, s, s, cin)")
    r, s, _, cin = x.shape
    k = bias.numel()
    if w_packed.numel() != 16 * cin * 32:
        raise OsrError(f"keypoint_upsample: w_packed {tuple(w_packed.shape)} is not pack_keypoint_deconv_weight of a ({cin}, k, 4, 4) weight")
    _rows_valid_arg(rows_valid, seg_rows, r, "keypoint_upsample")
    heat = torch.empty((r, k, 4 * s, 4 * s), dtype=torch.float32, device=x.device)
    check(lib.osr_keypoint_upsample(_p(x), _DT[x.dtype], r, s, cin, k, _p(w_packed), _p(bias), _p(rows_valid), int(seg_rows), _p(heat), _stream()),
          "osr_keypoint_upsample")
    return heat


def heatmaps_to_keypoints(maps: torch.Tensor, rois: torch.Tensor, rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0) -> torch.Tensor:
    """[d2] heatmaps_to_keypoints on the device without the resized maps (include/osr.h osr_heatmaps_to_keypoints): maps (r, k, m, m)
    fp32, m <= 56; rois (r, 4) fp32 xyxy. Returns (r, k, 4) fp32 {x, y, logit, score}: the first row-major maximum of the map resized
    bicubically to the RoI's ceil(h) x ceil(w), mapped into the image; zeros for the RoIs beyond a segment's count."""
    lib = _lib.load()
    _need(maps, torch.float32, "maps"); _need(rois, torch.float32, "rois")
    if maps.dim() != 4 or maps.shape[2] != maps.shape[3] or rois.shape != (maps.shape[0], 4):
        raise OsrError(f"heatmaps_to_keypoints: maps {tuple(maps.shape)} / rois {tuple(rois.shape)} are not (r, k, m, m) / (r, 4)")
    r, k, m, _ = maps.shape
    _rows_valid_arg(rows_valid, seg_rows, r, "heatmaps_to_keypoints")
    out = torch.empty((r, k, 4), dtype=torch.float32, device=maps.device)
    check(lib.osr_heatmaps_to_keypoints(_p(maps), _p(rois), r, k, m, _p(rows_valid), int(seg_rows), _p(out), _stream()), "osr_heatmaps_to_keypoints")
    return out


def _mask_tail_args(x, w_packed, bias, pred_w, classes, rows_valid, seg_rows, name):
    _need(x, name="x"); _need(w_packed, x.dtype, "w_packed")
    _need(bias, torch.float32, "bias"); _need(pred_w, torch.float32, "pred_w")
    r, s, s2, cin = x.shape
    k, cmid = pred_w.shape
    if s != s2 or bias.numel() != cmid or w_packed.numel() != 4 * cin * cmid:
        raise OsrError(f"{name}: x {tuple(x.shape)}, bias {tuple(bias.shape)}, pred_w {tuple(pred_w.shape)}, w_packed {tuple(w_packed.shape)} "
                       "do not fit together")
    if classes is not None:
        _need(classes, torch.int64, "classes")
        if classes.numel() != r:
            raise OsrError(f"{name}: {classes.numel()} classes for {r} RoIs")
    if rows_valid is not None:
        _need(rows_valid, torch.int32, "rows_valid")
        if seg_rows < 1 or rows_valid.numel() * seg_rows < r:
            raise OsrError(f"{name}: rows_valid does not cover the RoIs")
    return r, s, cin, k, cmid


def mask_upsample_logits(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, pred_w: torch.Tensor, pred_b: torch.Tensor,
                         classes: Optional[torch.Tensor] = None, rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0,
                         probs: bool = False):
    """mask_upsample_predict's launch with the class row's LOGIT as output (training: mask_loss_fwd reads it): (r, 2s, 2s) fp32, zeros
    on RoIs that do not exist or have no predictor row. probs=True: -> (logits, probs), the probabilities bit-identical to
    mask_upsample_predict's."""
    lib = _lib.load()
    r, s, cin, k, cmid = _mask_tail_args(x, w_packed, bias, pred_w, classes, rows_valid, seg_rows, "mask_upsample_logits")
    _need(pred_b, torch.float32, "pred_b")
    logits = torch.empty((r, 2 * s, 2 * s), dtype=torch.float32, device=x.device)
    pr = torch.empty_like(logits) if probs else None
    check(lib.osr_mask_upsample_predict_ex(_p(x), _DT[x.dtype], r, s, cin, cmid, _p(w_packed), _p(bias), _p(pred_w), _p(pred_b), k, _p(classes),
                                           _p(rows_valid), int(seg_rows), _p(pr), _p(logits), _stream()), "osr_mask_upsample_predict")
    return (logits, pr) if probs else logits


def mask_upsample_predict_bwd(x: torch.Tensor, w_packed: torch.Tensor, w_packed_t: torch.Tensor, bias: torch.Tensor, pred_w: torch.Tensor,
                              d_logits: torch.Tensor, classes: Optional[torch.Tensor] = None, rows_valid: Optional[torch.Tensor] = None,
                              seg_rows: int = 0, want_g: bool = True, dx_dtype: Optional[torch.dtype] = None):
    """Backward of mask_upsample_logits. w_packed_t = weights.pack_deconv_weight(deconv_weight.transpose(0, 1), dtype). d_logits
    (r, 2s, 2s) fp32. Returns dict(dx (r, s, s, cin) like x (or dx_dtype = torch.float32), g (4, r*s*s, cmid) like x -- tap-major gradient of the upsampled
    activation, for deconv_wgrad; bf16: (8, ...), a hi and a lo plane of four taps each; None without want_g --, d_pred_w (k, cmid), d_pred_b (k), d_deconv_b (cmid) fp32)."""
    lib = _lib.load()
    r, s, cin, k, cmid = _mask_tail_args(x, w_packed, bias, pred_w, classes, rows_valid, seg_rows, "mask_upsample_predict_bwd")
    _need(w_packed_t, x.dtype, "w_packed_t"); _need(d_logits, torch.float32, "d_logits")
    if w_packed_t.numel() != 4 * cin * cmid or tuple(d_logits.shape) != (r, 2 * s, 2 * s):
        raise OsrError(f"mask_upsample_predict_bwd: w_packed_t {tuple(w_packed_t.shape)} / d_logits {tuple(d_logits.shape)} do not fit x {tuple(x.shape)}")
    dev = x.device
    if dx_dtype not in (None, torch.float32, x.dtype):
        raise OsrError("mask_upsample_predict_bwd: dx_dtype must be float32 or x's dtype")
    o = dict(dx=torch.empty_like(x, dtype=dx_dtype or x.dtype), g=torch.empty((8 if x.dtype == torch.bfloat16 else 4, r * s * s, cmid), dtype=x.dtype, device=dev) if want_g else None,
             d_pred_w=torch.empty((k, cmid), dtype=torch.float32, device=dev), d_pred_b=torch.empty((k,), dtype=torch.float32, device=dev),
             d_deconv_b=torch.empty((cmid,), dtype=torch.float32, device=dev))
    wsb = lib.osr_mask_upsample_predict_bwd_workspace_bytes(r, s, cmid)
    if wsb < 0:
        check(int(wsb), "osr_mask_upsample_predict_bwd_workspace_bytes")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib.osr_mask_upsample_predict_bwd(_p(x), _DT[x.dtype], r, s, cin, cmid, _p(w_packed), _p(w_packed_t), _p(bias), _p(pred_w), k, _p(classes),
                                            _p(rows_valid), int(seg_rows), _p(d_logits), _p(o["dx"]), _DT[o["dx"].dtype], _p(o["g"]), _p(o["d_pred_w"]), _p(o["d_pred_b"]),
                                            _p(o["d_deconv_b"]), _p(ws), wsb, _stream()), "osr_mask_upsample_predict_bwd")
    return o


def deconv_wgrad(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The 2 x 2 stride-2 deconvolution's weight gradient (cin, cmid, 2, 2) fp32 from x (r, s, s, cin) and the tap-major g
    (4, r*s*s, cmid) of mask_upsample_predict_bwd: tap t's (cmid, cin) matrix is the 1 x 1 weight gradient of x against g[t]."""
    cin, cmid = x.shape[-1], g.shape[-1]
    m = g.shape[1]
    dw = torch.empty((4, cmid, cin), dtype=torch.float32, device=x.device)
    for t in range(g.shape[0]):  # (bf16: the lo plane's four taps are added to the hi plane's)
        conv2d_wgrad(x.view(1, m, 1, cin), g[t].view(1, m, 1, cmid), 1, 1, dw=dw[t % 4].view(cmid, 1, 1, cin), accumulate=t >= 4)
    return dw.view(2, 2, cmid, cin).permute(3, 2, 0, 1).contiguous()


def mask_targets(gt_masks: torch.Tensor, boxes: torch.Tensor, gt_idx: torch.Tensor, rows_valid: torch.Tensor, m_side: int,
                 image_hw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[d2] BitMasks.crop_and_resize for the mask rows of a batch. gt_masks (n, gmax, hm, wm) uint8 planes padded to the batch's image
    size, boxes (n, F, 4) fp32 and gt_idx (n, F) int32 of the F mask rows per image of which the first rows_valid[i] (n, int32) exist,
    image_hw (n, 2) int32 true image sizes (None: the planes' size). Returns targets (n * F, m_side, m_side) uint8:
    roi_align(plane, box, m_side, aligned) >= 0.5; zeros for rows that do not exist or have gt_idx < 0."""
    lib = _lib.load()
    _need(gt_masks, torch.uint8, "gt_masks"); _need(boxes, torch.float32, "boxes"); _need(gt_idx, torch.int32, "gt_idx")
    _need(rows_valid, torch.int32, "rows_valid")
    n, gmax, hm, wm = gt_masks.shape
    seg = boxes.numel() // (4 * n) if n else 0
    if boxes.numel() != n * seg * 4 or gt_idx.numel() != n * seg or rows_valid.numel() != n or seg < 1:
        raise OsrError(f"mask_targets: gt_masks {tuple(gt_masks.shape)}, boxes {tuple(boxes.shape)}, gt_idx {tuple(gt_idx.shape)}, "
                       f"rows_valid {tuple(rows_valid.shape)} do not fit together")
    if image_hw is not None:
        _need(image_hw, torch.int32, "image_hw")
        if image_hw.numel() != 2 * n:
            raise OsrError(f"mask_targets: image_hw must be (n, 2), got {tuple(image_hw.shape)}")
    out = torch.empty((n * seg, m_side, m_side), dtype=torch.uint8, device=gt_masks.device)
    check(lib.osr_mask_targets(_p(gt_masks), n, gmax, hm, wm, _p(image_hw), _p(boxes), _p(gt_idx), _p(rows_valid), seg, int(m_side), _p(out),
                               _stream()), "osr_mask_targets")
    return out


def _mask_loss_args(logits, targets, num_rows, classes, rows_valid, seg_rows, name):
    _need(logits, torch.float32, "logits"); _need(targets, torch.uint8, "targets")
    rows, m, m2 = logits.shape
    if m != m2 or tuple(targets.shape) != tuple(logits.shape):
        raise OsrError(f"{name}: logits {tuple(logits.shape)} and targets {tuple(targets.shape)} must both be (rows, M, M)")
    if classes is not None:
        _need(classes, torch.int64, "classes")
        if classes.numel() != rows:
            raise OsrError(f"{name}: {classes.numel()} classes for {rows} rows")
    if rows_valid is not None:
        _need(rows_valid, torch.int32, "rows_valid")
        if seg_rows < 1 or rows_valid.numel() * seg_rows < rows:
            raise OsrError(f"{name}: rows_valid does not cover the rows")
    return rows, m


def mask_loss_fwd(logits: torch.Tensor, targets: torch.Tensor, num_rows: int = 1, classes: Optional[torch.Tensor] = None,
                  rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0, loss_weight: float = 1.0) -> torch.Tensor:
    """[d2] mask_rcnn_loss on each row's own logit channel: logits (rows, M, M) fp32, targets (rows, M, M) uint8, classes (rows) int64
    against num_rows predictor rows (1: class-agnostic, classes may be None), rows_valid / seg_rows as mask_upsample_predict.
    Returns (6,) fp32 {loss_mask, foreground rows, incorrect, positive, false positive, false negative}."""
    lib = _lib.load()
    rows, m = _mask_loss_args(logits, targets, num_rows, classes, rows_valid, seg_rows, "mask_loss_fwd")
    out = torch.empty((6,), dtype=torch.float32, device=logits.device)
    ws = _loss_ws(logits.device, 6)
    check(lib.osr_mask_loss_fwd(_p(logits), _p(targets), rows, m, int(num_rows), _p(classes), _p(rows_valid), int(seg_rows), loss_weight, _p(out),
                                _p(ws), ws.numel(), _stream()), "osr_mask_loss_fwd")
    return out


def mask_loss_bwd(logits: torch.Tensor, targets: torch.Tensor, num_rows: int = 1, classes: Optional[torch.Tensor] = None,
                  rows_valid: Optional[torch.Tensor] = None, seg_rows: int = 0, scale: float = 1.0) -> torch.Tensor:
    """d loss_mask / d logits times `scale` (loss weight x loss scale): (rows, M, M) fp32, exact zeros on rows that do not count."""
    lib = _lib.load()
    rows, m = _mask_loss_args(logits, targets, num_rows, classes, rows_valid, seg_rows, "mask_loss_bwd")
    out = torch.empty_like(logits)
    ws = torch.empty((16,), dtype=torch.uint8, device=logits.device)
    check(lib.osr_mask_loss_bwd(_p(logits), _p(targets), rows, m, int(num_rows), _p(classes), _p(rows_valid), int(seg_rows), scale, _p(out), _p(ws), 16,
                                _stream()), "osr_mask_loss_bwd")
    return out


def mask_loss_scalars(out6: torch.Tensor, m_side: int) -> Dict[str, float]:
    """[d2] mask_rcnn_loss's three event scalars from mask_loss_fwd's counts (one device-to-host copy)."""
    _, fg, wrong, pos, fp, fn = (float(v) for v in out6.cpu())
    numel = fg * m_side * m_side
    return {"mask_rcnn/accuracy": 1.0 - wrong / max(numel, 1.0), "mask_rcnn/false_positive": fp / max(numel - pos, 1.0),
            "mask_rcnn/false_negative": fn / max(pos, 1.0)}


def paste_masks(probs: torch.Tensor, boxes: torch.Tensor, out_h: int, out_w: int, threshold: float = 0.5,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[d2] paste_masks_in_image for one image: probs (r, m, m) fp32, boxes (r, 4) fp32 at the output resolution -> (r, out_h, out_w)
    uint8, 0 or 1. Every byte of the result is written (out, if given, needs no fill)."""
    lib = _lib.load()
    _need(probs, torch.float32, "probs"); _need(boxes, torch.float32, "boxes")
    r, m, m2 = probs.shape
    if m != m2 or tuple(boxes.shape) != (r, 4):
        raise OsrError(f"paste_masks: probs {tuple(probs.shape)} / boxes {tuple(boxes.shape)}")
    if out is None:
        out = torch.empty((r, out_h, out_w), dtype=torch.uint8, device=probs.device)
    else:
        _need(out, torch.uint8, "out")
        assert tuple(out.shape) == (r, out_h, out_w)
    check(lib.osr_paste_masks(_p(probs), _p(boxes), r, m, int(out_h), int(out_w), float(threshold), _p(out), _stream()), "osr_paste_masks")
    return out


# ---- Panoptic FPN (csrc/osr_semseg.hip, csrc/osr_panoptic.hip; host/engine_panoptic.py) ----------------------------------------------
GN_GROUPS = 32
GN_EPS = 1e-5


def _nhwc_float(x: torch.Tensor, name: str):
    _need(x, None, name)
    if x.dtype not in _DT:
        raise OsrError(f"{name} must be float32 / float16 / bfloat16, got {x.dtype}")
    if x.dim() != 4:
        raise OsrError(f"{name} must be (n, h, w, c), got {tuple(x.shape)}")
    return tuple(int(v) for v in x.shape)


def group_norm_stats(x: torch.Tensor, eps: float = GN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """GroupNorm(32) statistics of x (n, h, w, c) NHWC, c in {64, 128, 256} -> (mean, rstd), each (n, 32) fp32 (include/osr.h
    osr_group_norm_stats: biased variance, rstd = 1 / sqrt(var + eps))."""
    lib = _lib.load()
    n, h, w, c = _nhwc_float(x, "x")
    wsb = int(lib.osr_group_norm_stats_workspace_bytes(n, h, w, c))
    if wsb < 0:
        check(wsb, "osr_group_norm_stats")
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=x.device)
    mean = torch.empty((n, GN_GROUPS), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    check(lib.osr_group_norm_stats(_p(x), _DT[x.dtype], n, h, w, c, float(eps), _p(mean), _p(rstd), _p(ws), wsb, _stream()), "osr_group_norm_stats")
    return mean, rstd


def gn_relu_merge(terms: Sequence[tuple], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_t up_t(relu(gn_t(x_t))) in one launch (include/osr.h osr_gn_relu_merge). A term is (x, stats, gamma, beta, up2): x (n, h, w, c)
    NHWC; stats = (mean, rstd) from group_norm_stats with gamma / beta (c) fp32, or None (gamma and beta then None too: the term is only
    rectified); up2: bilinear x2 after the ReLU. Every term has the output's dtype and, after its up2, the output's size."""
    lib = _lib.load()
    if not 1 <= len(terms) <= _lib.GN_MAX_TERMS:
        raise OsrError(f"gn_relu_merge: 1 .. {_lib.GN_MAX_TERMS} terms, got {len(terms)}")
    arr = (_lib.GnTerm * len(terms))()
    n0 = c0 = ho = wo = dt = None
    for i, (x, stats, gamma, beta, up2) in enumerate(terms):
        n, h, w, c = _nhwc_float(x, f"term {i}")
        f = 2 if up2 else 1
        if n0 is None:
            n0, c0, ho, wo, dt = n, c, h * f, w * f, x.dtype
        if (n, c, x.dtype) != (n0, c0, dt):
            raise OsrError(f"gn_relu_merge: term {i} is {tuple(x.shape)} {x.dtype}; term 0 has n {n0}, c {c0}, {dt}")
        arr[i].x, arr[i].h, arr[i].w, arr[i].up2 = x.data_ptr(), h, w, int(bool(up2))
        if stats is not None:
            mean, rstd = stats
            for t, shape, nm in ((mean, (n, GN_GROUPS), "mean"), (rstd, (n, GN_GROUPS), "rstd"), (gamma, (c,), "gamma"), (beta, (c,), "beta")):
                if t is None:
                    raise OsrError(f"gn_relu_merge: term {i} has statistics but no {nm}")
                _need(t, torch.float32, f"term {i} {nm}")
                if tuple(t.shape) != shape:
                    raise OsrError(f"gn_relu_merge: term {i} {nm} {tuple(t.shape)} != {shape}")
            arr[i].mean, arr[i].rstd, arr[i].gamma, arr[i].beta = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
        elif gamma is not None or beta is not None:
            raise OsrError(f"gn_relu_merge: term {i} has gamma / beta but no statistics")
    if out is None:
        out = torch.empty((n0, ho, wo, c0), dtype=dt, device=terms[0][0].device)
    else:
        _need(out, dt, "out")
        if tuple(out.shape) != (n0, ho, wo, c0):
            raise OsrError(f"gn_relu_merge: out {tuple(out.shape)} != {(n0, ho, wo, c0)}")
    check(lib.osr_gn_relu_merge(arr, len(terms), _DT[dt], n0, ho, wo, c0, _p(out), _stream()), "osr_gn_relu_merge")
    return out


def semseg_resample(logits: torch.Tensor, num_classes: int, crop_hw: Tuple[int, int], out_hw: Tuple[int, int], labels: bool,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[d2] sem_seg_postprocess (+ argmax) of ONE image from its stride-4 logits (h4, w4, pitch) (include/osr.h osr_semseg_resample):
    bilinear x4, crop to crop_hw, bilinear resize to out_hw, composed. labels=True -> (oh, ow) int32 argmax over the first num_classes
    channels; labels=False -> (num_classes, oh, ow) fp32."""
    lib = _lib.load()
    _need(logits, None, "logits")
    if logits.dtype not in _DT or logits.dim() != 3:
        raise OsrError(f"semseg_resample: logits must be (h4, w4, pitch) float32 / float16 / bfloat16, got {tuple(logits.shape)} {logits.dtype}")
    h4, w4, pitch = (int(v) for v in logits.shape)
    (ih, iw), (oh, ow) = (int(v) for v in crop_hw), (int(v) for v in out_hw)
    shape, dt = ((oh, ow), torch.int32) if labels else ((int(num_classes), oh, ow), torch.float32)
    if min(oh, ow, ih, iw, int(num_classes)) < 1:
        raise OsrError(f"semseg_resample: crop {crop_hw}, output {out_hw}, {num_classes} classes")
    if out is None:
        out = torch.empty(shape, dtype=dt, device=logits.device)
    else:
        _need(out, dt, "out")
        if tuple(out.shape) != shape:
            raise OsrError(f"semseg_resample: out {tuple(out.shape)} != {shape}")
    check(lib.osr_semseg_resample(_p(logits), _DT[logits.dtype], h4, w4, pitch, int(num_classes), ih, iw, oh, ow,
                                  _lib.SEMSEG_LABELS if labels else _lib.SEMSEG_VALUES, _p(out), _stream()), "osr_semseg_resample")
    return out


def panoptic_combine(masks: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, labels: torch.Tensor, overlap_thresh: float,
                     stuff_area_limit: int, instances_confidence_thresh: float, count: Optional[torch.Tensor] = None):
    """[d2] combine_semantic_and_instance_outputs for ONE image on the device (include/osr.h osr_panoptic_combine). masks (k, H, W) bool /
    uint8, scores (k) fp32, classes (k) int64, labels (H, W) int32, count (1) int32 or None (= k). -> (panoptic_seg (H, W) int32,
    seg_table (k + 255, 4) int32, seg_scores (k + 255) fp32, seg_count (1) int32); segments_info_from_table turns the last three
    into [d2]'s list of dicts."""
    lib = _lib.load()
    _need(masks, None, "masks"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes"); _need(labels, torch.int32, "labels")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise OsrError(f"panoptic_combine: masks must be bool or uint8, got {masks.dtype}")
    if labels.dim() != 2 or masks.dim() != 3 or tuple(masks.shape[1:]) != tuple(labels.shape):
        raise OsrError(f"panoptic_combine: masks {tuple(masks.shape)} / labels {tuple(labels.shape)}: (k, H, W) and (H, W)")
    k, h, w = (int(v) for v in masks.shape)
    if k > _lib.PANOPTIC_MAX_INSTANCES:
        raise OsrError(f"panoptic_combine: at most {_lib.PANOPTIC_MAX_INSTANCES} instances per image, got {k}")
    if scores.numel() != k or classes.numel() != k:
        raise OsrError(f"panoptic_combine: {scores.numel()} scores and {classes.numel()} classes for {k} masks")
    if count is not None:
        _need(count, torch.int32, "count")
    wsb = int(lib.osr_panoptic_combine_workspace_bytes(k, h, w))
    if wsb < 0:
        check(wsb, "osr_panoptic_combine")
    dev = labels.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    cap = k + _lib.PANOPTIC_MAX_STUFF
    pan = torch.empty((h, w), dtype=torch.int32, device=dev)
    table = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    sscores = torch.zeros((cap,), dtype=torch.float32, device=dev)
    scount = torch.zeros((1,), dtype=torch.int32, device=dev)
    check(lib.osr_panoptic_combine(_p(masks), _p(scores), _p(classes), _p(count), k, _p(labels), h, w, float(overlap_thresh), int(stuff_area_limit),
                                   float(instances_confidence_thresh), _p(pan), _p(table), _p(sscores), _p(scount), _p(ws), wsb, _stream()),
          "osr_panoptic_combine")
    return pan, table, sscores, scount


def segments_info_from_table(table: torch.Tensor, seg_scores: torch.Tensor, seg_count: torch.Tensor) -> List[dict]:
    """panoptic_combine's table -> [d2]'s segments_info, with ONE device-to-host copy (the three tensors are packed first).
    Things: {id, isthing True, score, category_id, instance_id}; stuff: {id, isthing False, category_id, area}."""
    rows = table.shape[0]
    packed = torch.cat((seg_count.reshape(1).to(torch.int32), table.reshape(-1).to(torch.int32), seg_scores.reshape(-1).view(torch.int32)))
    host = packed.cpu()
    cnt = int(host[0])
    tab = host[1:1 + rows * 4].view(rows, 4).tolist()
    sc = host[1 + rows * 4:].view(torch.float32).tolist()
    out = []
    for r in range(min(cnt, rows)):
        isthing, cat, inst, area = tab[r]
        if isthing:
            out.append({"id": r + 1, "isthing": True, "score": sc[r], "category_id": cat, "instance_id": inst})
        else:
            out.append({"id": r + 1, "isthing": False, "category_id": cat, "area": area})
    return out


# ---- segmentation evaluators (csrc/osr_seg_eval.hip; host/seg_evaluation.py) -----------------------------------------------------------
def semseg_confusion(pred: torch.Tensor, gt: torch.Tensor, num_classes: int, ignore_value: int, conf: torch.Tensor, invalid: torch.Tensor) -> None:
    """ONE image added into the running confusion matrix (include/osr.h osr_semseg_confusion). pred (H, W) int32 labels or
    (num_classes, H, W) fp32 values (the argmax is fused: lowest class on a tie); gt (H, W) uint8; conf (num_classes + 1,
    num_classes + 1) int64 indexed [pred][gt], column num_classes = ignore_value; invalid (1) int64. Both accumulate in place."""
    lib = _lib.load()
    _need(pred, None, "pred"); _need(gt, torch.uint8, "gt"); _need(conf, torch.int64, "conf"); _need(invalid, torch.int64, "invalid")
    c = int(num_classes)
    if pred.dtype == torch.int32 and pred.dim() == 2:
        mode, hw = _lib.CONF_LABELS, tuple(pred.shape)
    elif pred.dtype == torch.float32 and pred.dim() == 3 and pred.shape[0] == c:
        mode, hw = _lib.CONF_VALUES, tuple(pred.shape[1:])
    else:
        raise OsrError(f"semseg_confusion: pred must be (H, W) int32 or ({c}, H, W) float32, got {tuple(pred.shape)} {pred.dtype}")
    if tuple(gt.shape) != hw:
        raise OsrError(f"semseg_confusion: gt {tuple(gt.shape)} != prediction {hw}")
    if tuple(conf.shape) != (c + 1, c + 1) or invalid.numel() < 1:
        raise OsrError(f"semseg_confusion: conf {tuple(conf.shape)} must be {(c + 1, c + 1)}, invalid (1)")
    check(lib.osr_semseg_confusion(_p(pred), mode, _p(gt), int(hw[0]), int(hw[1]), c, int(ignore_value), _p(conf), _p(invalid), _stream()),
          "osr_semseg_confusion")


def panoptic_pair_counts(gt_rgb: torch.Tensor, gt_ids: torch.Tensor, pred: torch.Tensor, num_pred: int, flags: torch.Tensor,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE image's (ground-truth segment, predicted segment) pixel counts (include/osr.h osr_panoptic_pair_counts). gt_rgb (H, W, 3)
    uint8, the panoptic PNG as decoded; gt_ids (G) int32 strictly ascending; pred (H, W) int32 with ids 0 .. num_pred; flags (3)
    int64, accumulated. -> counts (G + 2, num_pred + 1) int32: row 0 VOID, 1 + i gt_ids[i], G + 1 unlisted ids."""
    lib = _lib.load()
    _need(gt_rgb, torch.uint8, "gt_rgb"); _need(gt_ids, torch.int32, "gt_ids"); _need(pred, torch.int32, "pred"); _need(flags, torch.int64, "flags")
    if pred.dim() != 2 or tuple(gt_rgb.shape) != tuple(pred.shape) + (3,) or gt_ids.dim() != 1 or flags.numel() < 3:
        raise OsrError(f"panoptic_pair_counts: gt_rgb {tuple(gt_rgb.shape)}, pred {tuple(pred.shape)}, gt_ids {tuple(gt_ids.shape)}: (H, W, 3), (H, W), (G); flags (3)")
    g, p = int(gt_ids.numel()), int(num_pred)
    h, w = (int(v) for v in pred.shape)
    if out is None:
        out = torch.empty((max(g, 0) + 2, max(p, 0) + 1), dtype=torch.int32, device=pred.device)
    else:
        _need(out, torch.int32, "out")
        if tuple(out.shape) != (g + 2, p + 1):
            raise OsrError(f"panoptic_pair_counts: out {tuple(out.shape)} != {(g + 2, p + 1)}")
    check(lib.osr_panoptic_pair_counts(_p(gt_rgb), _p(gt_ids) if g else None, g, _p(pred), p, h, w, _p(out), _p(flags), _stream()), "osr_panoptic_pair_counts")
    return out


def pq_accumulate(counts: torch.Tensor, gt_meta: torch.Tensor, pred_slot: torch.Tensor, pq_counts: torch.Tensor, pq_iou: torch.Tensor,
                  flags: torch.Tensor) -> None:
    """ONE image's matches added into the running PQ statistics (include/osr.h osr_pq_accumulate). counts (G + 2, P + 1) int32 from
    panoptic_pair_counts; gt_meta (G, 4) int32 {slot, iscrowd, area, crowd_pick}; pred_slot (P) int32; pq_counts (ncat, 3) int64
    {tp, fp, fn}, pq_iou (ncat) float64, flags (3) int64: all accumulated in place."""
    lib = _lib.load()
    _need(counts, torch.int32, "counts"); _need(gt_meta, torch.int32, "gt_meta"); _need(pred_slot, torch.int32, "pred_slot")
    _need(pq_counts, torch.int64, "pq_counts"); _need(pq_iou, torch.float64, "pq_iou"); _need(flags, torch.int64, "flags")
    g, p = int(gt_meta.shape[0]), int(pred_slot.numel())
    ncat = int(pq_iou.numel())
    if counts.dim() != 2 or tuple(counts.shape) != (g + 2, p + 1) or tuple(gt_meta.shape) != (g, 4) or tuple(pq_counts.shape) != (ncat, 3) or flags.numel() < 3:
        raise OsrError(f"pq_accumulate: counts {tuple(counts.shape)} must be {(g + 2, p + 1)}, gt_meta {tuple(gt_meta.shape)} (G, 4), "
                       f"pq_counts {tuple(pq_counts.shape)} ({ncat}, 3), flags (3)")
    check(lib.osr_pq_accumulate(_p(counts), g, p, _p(gt_meta) if g else None, _p(pred_slot) if p else None, ncat, _p(pq_counts), _p(pq_iou), _p(flags),
                                _stream()), "osr_pq_accumulate")


# ---- COCO box / keypoint matching (csrc/osr_coco_eval.hip; host/coco_evaluation.py) ------------------------------------------------------
def coco_match(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor, num_categories: int, gt_seg_off: torch.Tensor,
               gt_box: torch.Tensor, gt_area: torch.Tensor, gt_flags: torch.Tensor, max_gt_per_group: int, iou_thrs: Sequence[float],
               area_rng: Sequence[Sequence[float]], max_det: int, keypoints: Optional[torch.Tensor] = None, gt_kpts: Optional[torch.Tensor] = None,
               sigmas: Optional[torch.Tensor] = None, want_match: bool = False, want_sim: bool = False):
    """A batch of images scored against its ground truth in one launch (include/osr.h osr_coco_match, which states every rule).
    boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap) int64, counts (n) int32; gt_seg_off (n * K + 1) int32,
    gt_box (NG, 4) / gt_area (NG) float64, gt_flags (NG) uint8; iou_thrs and area_rng are host sequences of doubles. With
    `keypoints` (n, cap, Kp, 3) fp32 the task is OKS and needs gt_kpts (NG, Kp, 3) and sigmas (Kp) float64.
    -> (flags (n, cap, A) int32 holding the uint32 words, rank (n, cap) int32, match (n, cap, A, T) int32 or None, sim (min(cap,
    max_det) * NG) float64 in the header's layout or None)."""
    lib = _lib.load()
    kp = keypoints is not None
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes"); _need(counts, torch.int32, "counts")
    _need(gt_seg_off, torch.int32, "gt_seg_off"); _need(gt_box, torch.float64, "gt_box"); _need(gt_area, torch.float64, "gt_area")
    _need(gt_flags, torch.uint8, "gt_flags")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise OsrError(f"coco_match: boxes {tuple(boxes.shape)} must be (n, cap, 4)")
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    k, ng = int(num_categories), int(gt_area.numel())
    kpn = 0
    if kp:
        _need(keypoints, torch.float32, "keypoints")
        if gt_kpts is None or sigmas is None:
            raise OsrError("coco_match: the keypoint task needs gt_kpts and sigmas")
        _need(gt_kpts, torch.float64, "gt_kpts"); _need(sigmas, torch.float64, "sigmas")
        kpn = int(sigmas.numel())
        if keypoints.dim() != 4 or tuple(keypoints.shape) != (n, cap, kpn, 3) or tuple(gt_kpts.shape) != (ng, kpn, 3):
            raise OsrError(f"coco_match: keypoints {tuple(keypoints.shape)} must be {(n, cap, kpn, 3)}, gt_kpts {tuple(gt_kpts.shape)} {(ng, kpn, 3)}")
    if tuple(scores.shape) != (n, cap) or tuple(classes.shape) != (n, cap) or counts.numel() != n or gt_seg_off.numel() != n * k + 1 or \
            tuple(gt_box.shape) != (ng, 4) or gt_flags.numel() != ng:
        raise OsrError(f"coco_match: scores {tuple(scores.shape)} / classes {tuple(classes.shape)} must be {(n, cap)}, counts ({n}), gt_seg_off "
                       f"({n * k + 1}) got {gt_seg_off.numel()}, gt_box {tuple(gt_box.shape)} ({ng}, 4), gt_flags ({ng})")
    thrs = [float(v) for v in iou_thrs]
    rng = [float(v) for r in area_rng for v in r]
    t, a = len(thrs), len(rng) // 2
    dev = boxes.device
    flags = torch.empty((n, cap, a), dtype=torch.int32, device=dev)
    rank = torch.empty((n, cap), dtype=torch.int32, device=dev)
    match = torch.empty((n, cap, a, t), dtype=torch.int32, device=dev) if want_match else None
    ws_bytes = int(lib.osr_coco_match_workspace_bytes(cap, int(max_det), ng))
    sim = torch.empty((max(ws_bytes, 0) // 8,), dtype=torch.float64, device=dev)  # the matrix itself; handed over as `sim` or as the workspace
    check(lib.osr_coco_match(_lib.COCO_KEYPOINTS if kp else _lib.COCO_BBOX, _p(boxes), _p(scores), _p(classes), _p(counts), _p(keypoints) if kp else None,
                             n, cap, k, kpn, _p(gt_seg_off), _p(gt_box) if ng else None, _p(gt_area) if ng else None, _p(gt_flags) if ng else None,
                             _p(gt_kpts) if kp and ng else None, _p(sigmas) if kp else None, ng, int(max_gt_per_group), (C.c_double * t)(*thrs), t,
                             (C.c_double * (2 * a))(*rng), a, int(max_det), _p(flags), _p(rank), _p(match), _p(sim) if want_sim else None,
                             None if want_sim else _p(sim), 0 if want_sim else ws_bytes, _stream()), "osr_coco_match")
    return flags, rank, match, (sim if want_sim else None)


# ---- LVIS federated box matching (csrc/osr_lvis_eval.hip; host/lvis_evaluation.py) ------------------------------------------------------
def lvis_match(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor, num_categories: int, img_off: torch.Tensor,
               ev_cat: torch.Tensor, ev_gt_off: torch.Tensor, ev_flags: torch.Tensor, gt_box: torch.Tensor, gt_area: torch.Tensor, gt_flags: torch.Tensor,
               max_gt_per_group: int, iou_thrs: Sequence[float], area_rng: Sequence[Sequence[float]], max_dets: int, want_match: bool = False,
               want_sim: bool = False):
    """A batch of images cut, grouped and scored against its sparse LVIS ground truth in two launches (include/osr.h osr_lvis_match,
    which states every rule). boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap) int64, counts (n) int32; img_off
    (n + 1) int32, per evaluated (image, category) entry ev_cat (NE) int32 ascending within an image, ev_gt_off (NE + 1) int32 and
    ev_flags (NE) uint8 (bit 0 not exhaustive); gt_box (NG, 4) / gt_area (NG) float64, gt_flags (NG) uint8 (bit 1 ignore); iou_thrs
    and area_rng are host sequences of doubles.
    -> (flags (n, cap, A) int32 holding the uint32 words, rank (n, cap) int32, match (n, cap, A, T) int32 or None, sim (min(cap,
    max_dets) * NG) float64 in the header's layout or None)."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes"); _need(counts, torch.int32, "counts")
    _need(img_off, torch.int32, "img_off"); _need(ev_cat, torch.int32, "ev_cat"); _need(ev_gt_off, torch.int32, "ev_gt_off"); _need(ev_flags, torch.uint8, "ev_flags")
    _need(gt_box, torch.float64, "gt_box"); _need(gt_area, torch.float64, "gt_area"); _need(gt_flags, torch.uint8, "gt_flags")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise OsrError(f"lvis_match: boxes {tuple(boxes.shape)} must be (n, cap, 4)")
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    ne, ng = int(ev_cat.numel()), int(gt_area.numel())
    if tuple(scores.shape) != (n, cap) or tuple(classes.shape) != (n, cap) or counts.numel() != n or img_off.numel() != n + 1 or \
            ev_gt_off.numel() != ne + 1 or ev_flags.numel() != ne or tuple(gt_box.shape) != (ng, 4) or gt_flags.numel() != ng:
        raise OsrError(f"lvis_match: scores {tuple(scores.shape)} / classes {tuple(classes.shape)} must be {(n, cap)}, counts ({n}), img_off ({n + 1}) "
                       f"got {img_off.numel()}, ev_gt_off ({ne + 1}) got {ev_gt_off.numel()}, ev_flags ({ne}), gt_box {tuple(gt_box.shape)} ({ng}, 4), "
                       f"gt_flags ({ng})")
    thrs = [float(v) for v in iou_thrs]
    rng = [float(v) for r in area_rng for v in r]
    t, a = len(thrs), len(rng) // 2
    dev = boxes.device
    flags = torch.empty((n, cap, a), dtype=torch.int32, device=dev)
    rank = torch.empty((n, cap), dtype=torch.int32, device=dev)
    match = torch.empty((n, cap, a, t), dtype=torch.int32, device=dev) if want_match else None
    ws_bytes = max(int(lib.osr_lvis_match_workspace_bytes(n, cap, int(max_dets), ng)), 0)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)  # the similarities, then the group tables
    sim = torch.empty((min(cap, max(int(max_dets), 0)) * ng,), dtype=torch.float64, device=dev) if want_sim else None
    check(lib.osr_lvis_match(_p(boxes), _p(scores), _p(classes), _p(counts), n, cap, int(num_categories), _p(img_off), _p(ev_cat) if ne else None,
                             _p(ev_gt_off), _p(ev_flags) if ne else None, ne, _p(gt_box) if ng else None, _p(gt_area) if ng else None,
                             _p(gt_flags) if ng else None, ng, int(max_gt_per_group), (C.c_double * t)(*thrs), t, (C.c_double * (2 * a))(*rng), a,
                             int(max_dets), _p(flags), _p(rank), _p(match), _p(sim), _p(ws) if ws_bytes else None, ws_bytes, _stream()), "osr_lvis_match")
    return flags, rank, match, sim


# ---- open-set COCO matching (csrc/osr_os_coco_eval.hip; host/os_coco_evaluation.py) ------------------------------------------------------
def os_coco_match(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor, class_slot: torch.Tensor, num_known: int,
                  gt_img_off: torch.Tensor, gt_box: torch.Tensor, gt_area: torch.Tensor, gt_slot: torch.Tensor, gt_pos: torch.Tensor,
                  gt_crowd: torch.Tensor, max_gt_per_image: int, iou_thrs: Sequence[float], area_rng: Sequence[Sequence[float]], max_det: int,
                  want_match: bool = False):
    """A batch of images scored against its open-set ground truth in one launch (include/osr.h osr_os_coco_match, which states every
    rule). boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap) int64, counts (n) int32; class_slot (L) int32: class
    value -> slot 0 .. num_known (the last one unknown) or -1; gt_img_off (n + 1) int32, gt_box (NG, 4) / gt_area (NG) float64,
    gt_slot / gt_pos (NG) int32, gt_crowd (NG) uint8, each image's entries sorted by (slot, annotation order); iou_thrs and area_rng
    are host sequences of doubles.
    -> (flags (n, cap, A, 3) int32 holding the uint32 words, rank (n, cap) int32, match (n, cap, A, 3, T) int32 or None)."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes"); _need(counts, torch.int32, "counts")
    _need(class_slot, torch.int32, "class_slot"); _need(gt_img_off, torch.int32, "gt_img_off"); _need(gt_box, torch.float64, "gt_box")
    _need(gt_area, torch.float64, "gt_area"); _need(gt_slot, torch.int32, "gt_slot"); _need(gt_pos, torch.int32, "gt_pos"); _need(gt_crowd, torch.uint8, "gt_crowd")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise OsrError(f"os_coco_match: boxes {tuple(boxes.shape)} must be (n, cap, 4)")
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    ng, nl = int(gt_area.numel()), int(class_slot.numel())
    if tuple(scores.shape) != (n, cap) or tuple(classes.shape) != (n, cap) or counts.numel() != n or gt_img_off.numel() != n + 1 or \
            tuple(gt_box.shape) != (ng, 4) or gt_slot.numel() != ng or gt_pos.numel() != ng or gt_crowd.numel() != ng or nl < 1:
        raise OsrError(f"os_coco_match: scores {tuple(scores.shape)} / classes {tuple(classes.shape)} must be {(n, cap)}, counts ({n}), gt_img_off "
                       f"({n + 1}) got {gt_img_off.numel()}, gt_box {tuple(gt_box.shape)} ({ng}, 4), gt_slot / gt_pos / gt_crowd ({ng}), class_slot "
                       f"({nl}) at least one entry")
    thrs = [float(v) for v in iou_thrs]
    rng = [float(v) for r in area_rng for v in r]
    t, a = len(thrs), len(rng) // 2
    dev = boxes.device
    flags = torch.empty((n, cap, a, _lib.OS_COCO_SETS), dtype=torch.int32, device=dev)
    rank = torch.empty((n, cap), dtype=torch.int32, device=dev)
    match = torch.empty((n, cap, a, _lib.OS_COCO_SETS, t), dtype=torch.int32, device=dev) if want_match else None
    ws_bytes = int(lib.osr_os_coco_match_workspace_bytes(cap, ng))
    ws = torch.empty((max(ws_bytes, 0) // 8,), dtype=torch.float64, device=dev)
    check(lib.osr_os_coco_match(_p(boxes), _p(scores), _p(classes), _p(counts), n, cap, _p(class_slot), nl, int(num_known), _p(gt_img_off),
                                _p(gt_box) if ng else None, _p(gt_area) if ng else None, _p(gt_slot) if ng else None, _p(gt_pos) if ng else None,
                                _p(gt_crowd) if ng else None, ng, int(max_gt_per_image), (C.c_double * t)(*thrs), t, (C.c_double * (2 * a))(*rng), a,
                                int(max_det), _p(flags), _p(rank), _p(match), _p(ws) if ws_bytes > 0 else None, max(ws_bytes, 0), _stream()),
          "osr_os_coco_match")
    return flags, rank, match


# ---- open-set VOC matching (csrc/osr_voc_eval.hip; host/evaluation.py) ------------------------------------------------------------------
def voc_match(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor, image_index: torch.Tensor, num_classes: int,
              gt_img_off: torch.Tensor, gt_box: torch.Tensor, gt_cls: torch.Tensor, gt_difficult: torch.Tensor, max_gt_per_image: int,
              ovthresh: float = 0.5, want_match: bool = False, want_deci: bool = False):
    """A batch of images scored against the dataset's VOC ground truth for every class in one launch (include/osr.h osr_voc_match,
    which states every rule). boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap) int64, counts (n) / image_index (n)
    int32; gt_img_off (num_images + 1) int32, gt_box (NG, 4) float64, gt_cls (NG) int32, gt_difficult (NG) uint8.
    -> (flags (n, cap) uint8, milli (n, cap) int32, match (n, cap) int32 or None, deci (n, cap, 4) int64 or None, status (1) int32)."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes"); _need(counts, torch.int32, "counts")
    _need(image_index, torch.int32, "image_index"); _need(gt_img_off, torch.int32, "gt_img_off"); _need(gt_box, torch.float64, "gt_box")
    _need(gt_cls, torch.int32, "gt_cls"); _need(gt_difficult, torch.uint8, "gt_difficult")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise OsrError(f"voc_match: boxes {tuple(boxes.shape)} must be (n, cap, 4)")
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    ng, num_images = int(gt_cls.numel()), int(gt_img_off.numel()) - 1
    if tuple(scores.shape) != (n, cap) or tuple(classes.shape) != (n, cap) or counts.numel() != n or image_index.numel() != n or num_images < 0 or \
            tuple(gt_box.shape) != (ng, 4) or gt_difficult.numel() != ng:
        raise OsrError(f"voc_match: scores {tuple(scores.shape)} / classes {tuple(classes.shape)} must be {(n, cap)}, counts / image_index ({n}), "
                       f"gt_img_off at least one entry, gt_box {tuple(gt_box.shape)} ({ng}, 4), gt_difficult ({ng})")
    dev = boxes.device
    launched = n > 0 and cap > 0  # (else the call writes nothing)
    flags = torch.empty((n, cap), dtype=torch.uint8, device=dev)
    milli = torch.empty((n, cap), dtype=torch.int32, device=dev)
    match = torch.empty((n, cap), dtype=torch.int32, device=dev) if want_match else None
    deci = torch.empty((n, cap, 4), dtype=torch.int64, device=dev) if want_deci else None
    status = torch.empty((1,), dtype=torch.int32, device=dev) if launched else torch.zeros((1,), dtype=torch.int32, device=dev)
    check(lib.osr_voc_match(_p(boxes), _p(scores), _p(classes), _p(counts), _p(image_index), n, cap, int(num_classes), _p(gt_img_off), num_images,
                            _p(gt_box) if ng else None, _p(gt_cls) if ng else None, _p(gt_difficult) if ng else None, ng, int(max_gt_per_image),
                            float(ovthresh), _p(flags), _p(milli), _p(match), _p(deci), _p(status), _stream()), "osr_voc_match")
    return flags, milli, match, deci, status


# ---- box-proposal recall (csrc/osr_proposal_recall.hip; host/proposal_evaluation.py) -------------------------------------------------
def proposal_recall(boxes: torch.Tensor, logits: torch.Tensor, counts: torch.Tensor, gt_boxes: torch.Tensor, gt_area: torch.Tensor,
                    seg_off: torch.Tensor, max_gt_per_image: int, area_ranges: torch.Tensor, limits: Sequence[int], thresholds: torch.Tensor,
                    want_overlaps: bool = False):
    """A batch's proposals matched to its non-crowd ground truth in one launch (include/osr.h osr_proposal_recall, which states every
    rule). boxes (n, cap, 4) fp32 xyxy, logits (n, cap) fp32, counts (n) int32; gt_boxes (NG, 4) / gt_area (NG) fp32, seg_off (n + 1)
    int32. area_ranges (A, 2) and thresholds (T) are fp32 CPU tensors whose bits the kernel compares with; limits a host sequence.
    -> (hits (n, A, L, T) int32, num_pos (n, A) int32, gt_overlap (A, L, NG) fp32 or None)."""
    lib = _lib.load()
    _need(boxes, torch.float32, "boxes"); _need(logits, torch.float32, "logits"); _need(counts, torch.int32, "counts")
    _need(gt_boxes, torch.float32, "gt_boxes"); _need(gt_area, torch.float32, "gt_area"); _need(seg_off, torch.int32, "seg_off")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise OsrError(f"proposal_recall: boxes {tuple(boxes.shape)} must be (n, cap, 4)")
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    ng = int(gt_area.numel())
    if tuple(logits.shape) != (n, cap) or counts.numel() != n or seg_off.numel() != n + 1 or tuple(gt_boxes.shape) != (ng, 4):
        raise OsrError(f"proposal_recall: logits {tuple(logits.shape)} must be {(n, cap)}, counts ({n}), seg_off ({n + 1}) got {seg_off.numel()}, "
                       f"gt_boxes {tuple(gt_boxes.shape)} ({ng}, 4)")
    for t, name in ((area_ranges, "area_ranges"), (thresholds, "thresholds")):
        if t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise OsrError(f"proposal_recall: {name} must be a contiguous float32 CPU tensor")
    if area_ranges.dim() != 2 or area_ranges.shape[1] != 2 or thresholds.dim() != 1:
        raise OsrError(f"proposal_recall: area_ranges {tuple(area_ranges.shape)} must be (A, 2), thresholds {tuple(thresholds.shape)} (T)")
    lim = [int(v) for v in limits]
    a, l, t = int(area_ranges.shape[0]), len(lim), int(thresholds.numel())
    dev = boxes.device
    hits = torch.empty((n, a, l, t), dtype=torch.int32, device=dev)
    num_pos = torch.empty((n, a), dtype=torch.int32, device=dev)
    ov = torch.full((a, l, ng), -1.0, dtype=torch.float32, device=dev) if want_overlaps else None
    check(lib.osr_proposal_recall(_p(boxes) if cap else None, _p(logits) if cap else None, _p(counts), n, cap, _p(gt_boxes) if ng else None,
                                  _p(gt_area) if ng else None, _p(seg_off), ng, int(max_gt_per_image), C.c_void_p(area_ranges.data_ptr()), a,
                                  (C.c_int32 * max(l, 1))(*lim), l, C.c_void_p(thresholds.data_ptr()), t, _p(hits), _p(num_pos), _p(ov), _stream()),
          "osr_proposal_recall")
    return hits, num_pos, ov


# ---- test-time augmentation glue (csrc/osr_tta.hip; host/tta.py) ---------------------------------------------------------------
def _tta_lists(boxes, counts, sizes, name):
    _need(boxes, torch.float32, "boxes"); _need(counts, torch.int32, "counts"); _need(sizes, torch.int32, "sizes")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or counts.numel() != boxes.shape[0] or tuple(sizes.shape) != (boxes.shape[0], 4):
        raise OsrError(f"{name}: boxes (n, topk, 4), counts (n), sizes (n, 4); got {tuple(boxes.shape)}, {tuple(counts.shape)}, {tuple(sizes.shape)}")
    return int(boxes.shape[0]), int(boxes.shape[1])


def tta_boxes_to_original(boxes, scores, classes, counts, sizes, ha: int, wa: int, flip: bool, slot: int, c_boxes, c_scores, c_cls, c_cand) -> None:
    """One augmentation's padded detections (boxes (n, topk, 4), scores (n, topk), classes (n, topk) int64, counts (n)) mapped back to
    each image's output resolution -- sizes (n, 4) int32 {hi, wi, ho, wo} -- and clipped, into rows [slot, slot + topk) of the
    per-image candidate lists c_boxes (n, cap, 4), c_scores, c_cls int32, c_cand int32 (osr_tta_boxes_to_original)."""
    lib = _lib.load()
    n, topk = _tta_lists(boxes, counts, sizes, "tta_boxes_to_original")
    _need(scores, torch.float32, "scores"); _need(classes, torch.int64, "classes")
    _need(c_boxes, torch.float32, "c_boxes"); _need(c_scores, torch.float32, "c_scores"); _need(c_cls, torch.int32, "c_cls"); _need(c_cand, torch.int32, "c_cand")
    cap = int(c_scores.shape[1]) if c_scores.dim() == 2 else -1
    if tuple(scores.shape) != (n, topk) or tuple(classes.shape) != (n, topk) or tuple(c_boxes.shape) != (n, cap, 4) or \
            tuple(c_scores.shape) != (n, cap) or tuple(c_cls.shape) != (n, cap) or tuple(c_cand.shape) != (n, cap):
        raise OsrError("tta_boxes_to_original: scores / classes (n, topk); c_boxes (n, cap, 4), c_scores / c_cls / c_cand (n, cap)")
    check(lib.osr_tta_boxes_to_original(_p(boxes), _p(scores), _p(classes), _p(counts), _p(sizes), n, topk, int(ha), int(wa), int(bool(flip)), int(slot),
                                        cap, _p(c_boxes), _p(c_scores), _p(c_cls), _p(c_cand), _stream()), "osr_tta_boxes_to_original")


def tta_boxes_to_augmented(boxes, counts, sizes, ha: int, wa: int, flip: bool) -> torch.Tensor:
    """Merged padded boxes (n, topk, 4) at each image's output resolution -> the augmentation's (ha, wa) space, not clipped; rows
    beyond an image's count are zeros (osr_tta_boxes_to_augmented)."""
    lib = _lib.load()
    n, topk = _tta_lists(boxes, counts, sizes, "tta_boxes_to_augmented")
    out = torch.empty_like(boxes)
    check(lib.osr_tta_boxes_to_augmented(_p(boxes), _p(counts), _p(sizes), n, topk, int(ha), int(wa), int(bool(flip)), _p(out), _stream()),
          "osr_tta_boxes_to_augmented")
    return out


def tta_reduce_masks(maps, flip, counts) -> torch.Tensor:
    """maps (A, n, topk, m, m) fp32, flip (A) int32 0 / 1, counts (n) int32 -> (n, topk, m, m): the mean over the augmentations of the
    maps, those of flipped augmentations mirrored along x; fp32 sum in augmentation order, then / A; zeros beyond the counts
    (osr_tta_reduce_masks)."""
    lib = _lib.load()
    _need(maps, torch.float32, "maps"); _need(flip, torch.int32, "flip"); _need(counts, torch.int32, "counts")
    if maps.dim() != 5 or maps.shape[3] != maps.shape[4] or flip.numel() != maps.shape[0] or counts.numel() != maps.shape[1]:
        raise OsrError(f"tta_reduce_masks: maps (A, n, topk, m, m), flip (A), counts (n); got {tuple(maps.shape)}, {tuple(flip.shape)}, {tuple(counts.shape)}")
    a, n, topk, m, _ = (int(v) for v in maps.shape)
    out = torch.empty((n, topk, m, m), dtype=torch.float32, device=maps.device)
    check(lib.osr_tta_reduce_masks(_p(maps), _p(flip), a, _p(counts), n, topk, m, _p(out), _stream()), "osr_tta_reduce_masks")
    return out


# ----------------------------------------------------------------------------------------------------------
# training step, forward half (targets + losses)
# ----------------------------------------------------------------------------------------------------------
def _levels_r(lv: RpnLevels) -> int:
    return sum(lv.h[i] * lv.w[i] for i in range(lv.num_levels)) * lv.num_anchors


def rpn_match_anchors(lv: RpnLevels, cell_anchors, n: int, gt_boxes, gt_count, reg_thr=(0.3, 0.7), obj_thr=(0.1, 0.3)):
    """gt_boxes (n,gmax,4) fp32 padded, gt_count (n) int32. Returns matched_idx, matched_iou, labels_reg, labels_obj (n,R)."""
    lib = _lib.load()
    _need(cell_anchors, torch.float32, "cell_anchors"); _need(gt_boxes, torch.float32, "gt_boxes"); _need(gt_count, torch.int32, "gt_count")
    gmax, r, dev = gt_boxes.shape[1], _levels_r(lv), gt_boxes.device
    midx = torch.empty((n, r), dtype=torch.int32, device=dev)
    miou = torch.empty((n, r), dtype=torch.float32, device=dev)
    lr = torch.empty((n, r), dtype=torch.int8, device=dev)
    lo = torch.empty((n, r), dtype=torch.int8, device=dev)
    ws = torch.empty((n * gmax * 4,), dtype=torch.uint8, device=dev)
    check(lib.osr_rpn_match_anchors(C.byref(lv), _p(cell_anchors), n, _p(gt_boxes), _p(gt_count), gmax, reg_thr[0], reg_thr[1], obj_thr[0],
                                    obj_thr[1], _p(midx), _p(miou), _p(lr), _p(lo), _p(ws), ws.numel(), _stream()), "osr_rpn_match_anchors")
    return midx, miou, lr, lo


def subsample_labels_(labels, keys, num_samples: int, positive_fraction: float):
    """In place on labels (n,r) int8; keys (n,r) fp32 uniform. Returns (num_pos, num_neg) int32 (n)."""
    lib = _lib.load()
    _need(labels, torch.int8, "labels"); _need(keys, torch.float32, "keys")
    if labels.shape != keys.shape or labels.dim() != 2:
        raise OsrError("labels and keys must both be (n, r)")
    n, r = labels.shape
    npos = torch.empty((n,), dtype=torch.int32, device=labels.device)
    nneg = torch.empty((n,), dtype=torch.int32, device=labels.device)
    check(lib.osr_subsample_labels(_p(labels), _p(keys), n, r, num_samples, positive_fraction, _p(npos), _p(nneg), _stream()),
          "osr_subsample_labels")
    return npos, nneg


def rpn_anchor_targets(lv: RpnLevels, cell_anchors, n: int, gt_boxes, gt_count, matched_idx, labels_obj):
    lib = _lib.load()
    _need(matched_idx, torch.int32, "matched_idx"); _need(labels_obj, torch.int8, "labels_obj")
    r, dev = _levels_r(lv), gt_boxes.device
    mb = torch.empty((n, r, 4), dtype=torch.float32, device=dev)
    ct = torch.empty((n, r), dtype=torch.float32, device=dev)
    check(lib.osr_rpn_anchor_targets(C.byref(lv), _p(cell_anchors), n, _p(gt_boxes), _p(gt_count), gt_boxes.shape[1], _p(matched_idx),
                                     _p(labels_obj), _p(mb), _p(ct), _stream()), "osr_rpn_anchor_targets")
    return mb, ct


def _loss_options(box, aux_beta):
    """box = (type name, smooth-L1 beta) as the yaml names it; aux_beta: beta of the centerness / IoU smooth-L1 loss."""
    o = _lib.LossOptions()
    if box[0] not in _lib.BOX_LOSS_TYPES:
        raise OsrError(f"box regression loss type '{box[0]}': one of {sorted(_lib.BOX_LOSS_TYPES)}")
    o.box_loss_type, o.box_smooth_l1_beta, o.aux_smooth_l1_beta = _lib.BOX_LOSS_TYPES[box[0]], float(box[1]), float(aux_beta)
    return o


def rpn_losses_fwd(lv: RpnLevels, cell_anchors, n: int, pred_deltas, pred_ctr, labels_reg, labels_obj, matched_boxes, ctr_target,
                   loc_weight=0.5, ctr_weight=0.5, batch_size_per_image=256, box_loss=("iou", 0.0), ctr_beta=0.0) -> torch.Tensor:
    """pred_*: level-major (as the RPN head writes them). Returns 6 floats: loss_rpn_loc, loss_rpn_ctr, 4 anchor counts.
    box_loss: (MODEL.RPN.BBOX_REG_LOSS_TYPE, MODEL.RPN.SMOOTH_L1_BETA); ctr_beta: MODEL.RPN.CTR_SMOOTH_L1_BETA."""
    lib = _lib.load()
    _need(pred_deltas, torch.float32, "pred_deltas"); _need(pred_ctr, torch.float32, "pred_ctr")
    _need(matched_boxes, torch.float32, "matched_boxes"); _need(ctr_target, torch.float32, "ctr_target")
    dev = pred_ctr.device
    out = torch.empty((6,), dtype=torch.float32, device=dev)
    ws = _loss_ws(dev, 6)
    opt = _loss_options(box_loss, ctr_beta)
    check(lib.osr_rpn_losses_fwd_ex(C.byref(lv), _p(cell_anchors), n, _p(pred_deltas), _p(pred_ctr), _p(labels_reg), _p(labels_obj),
                                    _p(matched_boxes), _p(ctr_target), loc_weight, ctr_weight, batch_size_per_image, C.byref(opt), _p(out), _p(ws),
                                    ws.numel(), _stream()), "osr_rpn_losses_fwd")
    return out


def roi_match_and_sample(prop_boxes, prop_logits, prop_count, gt_boxes, gt_classes, gt_count, keys, num_classes: int,
                         batch_size: int = 512, positive_fraction: float = 0.25, iou_thr: float = 0.5):
    """prop_boxes (n,pcap,4), prop_logits (n,pcap), prop_count (n) int32, gt_boxes (n,gmax,4), gt_classes (n,gmax) int64,
    gt_count (n) int32, keys (n,pcap+gmax). Returns a dict of padded (n,batch_size,...) outputs."""
    lib = _lib.load()
    _need(prop_boxes, torch.float32, "prop_boxes"); _need(prop_logits, torch.float32, "prop_logits"); _need(prop_count, torch.int32, "prop_count")
    _need(gt_boxes, torch.float32, "gt_boxes"); _need(gt_classes, torch.int64, "gt_classes"); _need(gt_count, torch.int32, "gt_count")
    _need(keys, torch.float32, "keys")
    n, pcap = prop_boxes.shape[0], prop_boxes.shape[1]
    gmax, dev = gt_boxes.shape[1], prop_boxes.device
    if tuple(keys.shape) != (n, pcap + gmax):
        raise OsrError(f"keys must be (n, pcap+gmax) = ({n}, {pcap + gmax}), got {tuple(keys.shape)}")
    wsb = lib.osr_roi_match_sample_workspace_bytes(n, pcap, gmax)
    if wsb < 0:
        check(int(wsb), "osr_roi_match_sample_workspace_bytes")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    o = dict(boxes=torch.empty((n, batch_size, 4), dtype=torch.float32, device=dev),
             logits=torch.empty((n, batch_size), dtype=torch.float32, device=dev),
             gt_classes=torch.empty((n, batch_size), dtype=torch.int64, device=dev),
             ious=torch.empty((n, batch_size), dtype=torch.float32, device=dev),
             gt_boxes=torch.empty((n, batch_size, 4), dtype=torch.float32, device=dev),
             src=torch.empty((n, batch_size), dtype=torch.int32, device=dev),
             batch_idx=torch.empty((n * batch_size,), dtype=torch.int32, device=dev),
             counts=torch.empty((n, 3), dtype=torch.int32, device=dev),
             gt_idx=torch.empty((n, batch_size), dtype=torch.int32, device=dev))  # matched GT index; -1: background / padding
    check(lib.osr_roi_match_and_sample_ex(_p(prop_boxes), _p(prop_logits), _p(prop_count), pcap, _p(gt_boxes), _p(gt_classes), _p(gt_count), gmax, n,
                                          _p(keys), num_classes, batch_size, positive_fraction, iou_thr, _p(o["boxes"]), _p(o["logits"]),
                                          _p(o["gt_classes"]), _p(o["ious"]), _p(o["gt_boxes"]), _p(o["src"]), _p(o["batch_idx"]), _p(o["counts"]),
                                          _p(o["gt_idx"]), _p(ws), wsb, _stream()), "osr_roi_match_and_sample")
    return o


def _loss_ws(dev, nv: int):
    return torch.empty((256 * nv * 4,), dtype=torch.uint8, device=dev)


def roi_box_losses_fwd(pred_deltas, pred_iou, proposal_boxes, gt_boxes, gt_classes, gt_iou, num_classes: int,
                       reg_weights=(10.0, 10.0, 5.0, 5.0), box_weight=0.5, iou_weight=0.5, iou_is_logit: bool = False,
                       box_loss=("smooth_l1", 0.0), iou_beta=0.0) -> torch.Tensor:
    """pred_deltas (m,>=4) / pred_iou (m) may be column views of one row-major predictor output (stride(1) == 1).
    Returns 3 floats: loss_box_reg, loss_iou, rows counted (class >= 0). box_loss: (MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE,
    SMOOTH_L1_BETA); iou_beta: IOU_SMOOTH_L1_BETA."""
    lib = _lib.load()
    for t, nm in ((proposal_boxes, "proposal_boxes"), (gt_boxes, "gt_boxes"), (gt_iou, "gt_iou")):
        _need(t, torch.float32, nm)
    _need(gt_classes, torch.int64, "gt_classes")
    for t, nm in ((pred_deltas, "pred_deltas"), (pred_iou, "pred_iou")):
        if not t.is_cuda or t.dtype != torch.float32 or (t.dim() == 2 and t.stride(1) != 1):
            raise OsrError(f"{nm} must be an fp32 GPU tensor with unit stride inside a row")
    m, dev = gt_classes.numel(), proposal_boxes.device
    out = torch.empty((3,), dtype=torch.float32, device=dev)
    ws = _loss_ws(dev, 3)
    rw = (C.c_float * 4)(*reg_weights)
    opt = _loss_options(box_loss, iou_beta)
    check(lib.osr_roi_box_losses_fwd_ex(_p(pred_deltas), pred_deltas.stride(0), _p(pred_iou), pred_iou.stride(0), int(iou_is_logit), _p(proposal_boxes),
                                        _p(gt_boxes), _p(gt_classes), _p(gt_iou), m, num_classes, rw, box_weight, iou_weight, C.byref(opt), _p(out), _p(ws),
                                        ws.numel(), _stream()), "osr_roi_box_losses_fwd")
    return out


def pln_loss_fwd(emb, protos_normed, gt_classes, ious, iou_thr: float, alpha: float, beta: float, loss_weight: float, reps: int = 1,
                 distance: str = "COS") -> torch.Tensor:
    """protos_normed: (num_known * reps, d), the reps prototypes of a class next to each other (prototype_learning_network.py:163)."""
    lib = _lib.load()
    _need(emb, torch.float32, "emb"); _need(protos_normed, torch.float32, "protos_normed"); _need(gt_classes, torch.int64, "gt_classes")
    _need(ious, torch.float32, "ious")
    m, d = emb.shape
    out = torch.empty((1,), dtype=torch.float32, device=emb.device)
    ws = _loss_ws(emb.device, 4)
    assert protos_normed.shape[0] % reps == 0
    check(lib.osr_pln_loss_fwd_ex(_p(emb), m, d, _p(protos_normed), protos_normed.shape[0] // reps, reps, _pln_distance(distance), _p(gt_classes),
                                  _p(ious), iou_thr, alpha, beta, loss_weight, _p(out), _p(ws), ws.numel(), _stream()), "osr_pln_loss_fwd")
    return out


def softmax_ce_loss_fwd(logits, gt_classes, num_classes: int, loss_weight: float) -> torch.Tensor:
    lib = _lib.load()
    _need(logits, torch.float32, "logits"); _need(gt_classes, torch.int64, "gt_classes")
    m, nk1 = logits.shape
    out = torch.empty((1,), dtype=torch.float32, device=logits.device)
    ws = _loss_ws(logits.device, 2)
    check(lib.osr_softmax_ce_loss_fwd(_p(logits), m, nk1 - 1, _p(gt_classes), num_classes, loss_weight, _p(out), _p(ws), ws.numel(), _stream()),
          "osr_softmax_ce_loss_fwd")
    return out


# ----------------------------------------------------------------------------------------------------------
# training step, backward half: dense layers
# ----------------------------------------------------------------------------------------------------------
def conv2d_dgrad(dy: torch.Tensor, w_dgrad: torch.Tensor, x_hw: Tuple[int, int], stride: int = 1, pad: int = 0,
                 mask: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
                 post_mask: Optional[torch.Tensor] = None, strided_only: bool = False) -> torch.Tensor:
    """Gradient w.r.t. the input of a convolution: dy (n,ho,wo,cout), w_dgrad = pack_dgrad_weight(w) (cin,kh,kw,cout).
    mask: forward activation at dx's positions (n,hi,wi,cin) -> dx is zeroed where mask <= 0 (the ReLU below);
    add: a second gradient of dx's shape summed in (residual / shortcut branch). At most one of the two (they share the
    epilogue's auxiliary operand); post_mask: a forward activation of dx's shape applied as a ReLU mask AFTER the sum (the
    join of a residual block: osr_conv2d_fwd_masked); stride 2 is supported for 1x1 layers (every second pixel of a zeroed dx)
    and for 3x3 layers with pad 1 (osr_conv2d_dgrad_s2: every pixel written; mask / post_mask and add may then be combined,
    the mask applying after the sum).
    strided_only (stride > 1): the caller reads dx only at the pixels the stride visits (as the `add` of a second strided launch
    does), so the other pixels are left unwritten instead of zero-filled."""
    lib = _lib.load()
    _need(dy, name="dy"); _need(w_dgrad, dy.dtype, "w_dgrad")
    n, ho, wo, cout = dy.shape
    cin, kh, kw, cout2 = w_dgrad.shape
    hi, wi = x_hw
    if cout2 != cout:
        raise OsrError(f"w_dgrad cout {cout2} != dy channels {cout}")
    if stride == 2 and kh == 3 and kw == 3 and pad == 1:
        return _conv2d_dgrad_s2(dy, w_dgrad, hi, wi, mask, add, out_dtype, post_mask)
    if mask is not None and add is not None:
        raise OsrError("conv2d_dgrad takes a mask or an addend, not both")
    aux, mode = (mask, 3) if mask is not None else ((add, 1) if add is not None else (None, 0))
    out_dtype = out_dtype or dy.dtype
    zero_bias = _zero_bias(cin, dy.device)
    if stride == 1:
        if (hi + 2 * pad - kh) + 1 != ho or (wi + 2 * pad - kw) + 1 != wo:
            raise OsrError("x_hw inconsistent with dy and the kernel geometry")
        return conv2d(dy, w_dgrad, zero_bias, 1, kh - 1 - pad, False, aux, mode, out_dtype, post_mask=post_mask)
    if not (kh == 1 and kw == 1 and pad == 0):
        raise OsrError("strided backward-data is implemented for 1x1 layers only (the reference's R-50 strides in the 1x1)")
    if (hi - 1) // stride + 1 != ho or (wi - 1) // stride + 1 != wo:
        raise OsrError("x_hw inconsistent with dy and the stride")
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * ho * wo * cout * cin
    dx = (torch.empty if strided_only else torch.zeros)((n, hi, wi, cin), dtype=out_dtype, device=dy.device)
    p = _conv_params(n, ho, wo, cout, ho, wo, cin, 1, 1, 1, 0, dy.dtype, out_dtype)
    p.out_stride_n, p.out_stride_h, p.out_stride_w = hi * wi * cin, stride * wi * cin, stride * cin
    p.res_mode = mode
    if aux is not None:
        _need(aux, dy.dtype, "mask/add")
        if tuple(aux.shape) != (n, hi, wi, cin):
            raise OsrError(f"mask/add shape {tuple(aux.shape)} != {(n, hi, wi, cin)}")
        p.res_stride_n, p.res_stride_h, p.res_stride_w = hi * wi * cin, stride * wi * cin, stride * cin
    if post_mask is not None:
        _need(post_mask, dy.dtype, "post_mask")
        if tuple(post_mask.shape) != (n, hi, wi, cin):
            raise OsrError(f"post_mask shape {tuple(post_mask.shape)} != {(n, hi, wi, cin)}")
        if mode == 3:
            raise OsrError("conv2d_dgrad: mask and post_mask are the same thing; pass one")
        st = lib.osr_conv2d_fwd_masked(C.byref(p), _p(dy), _p(w_dgrad), _p(zero_bias), _p(aux), _p(post_mask), _p(dx), _stream())
        if st != _lib.ERR_UNSUPPORTED:
            check(st, "osr_conv2d_fwd_masked(dgrad)")
            return dx  # (the pixels the stride skips stay zero: masking them changes nothing)
    check(lib.osr_conv2d_fwd(C.byref(p), _p(dy), _p(w_dgrad), _p(zero_bias), _p(aux), _p(dx), _stream()), "osr_conv2d_fwd(dgrad)")
    if post_mask is not None:
        relu_mask_(dx, post_mask)
    return dx


def _conv2d_dgrad_s2(dy: torch.Tensor, w_dgrad: torch.Tensor, hi: int, wi: int, mask: Optional[torch.Tensor], add: Optional[torch.Tensor],
                     out_dtype: Optional[torch.dtype], post_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """conv2d_dgrad of a 3x3 / stride 2 / pad 1 layer: osr_conv2d_dgrad_s2, dx = mask > 0 ? conv + add : 0 in one launch."""
    lib = _lib.load()
    n, ho, wo, cout = dy.shape
    cin = w_dgrad.shape[0]
    if (hi - 1) // 2 + 1 != ho or (wi - 1) // 2 + 1 != wo:
        raise OsrError("x_hw inconsistent with dy and the stride")
    if mask is not None and post_mask is not None:
        raise OsrError("conv2d_dgrad: mask and post_mask are the same thing; pass one")
    m = mask if mask is not None else post_mask
    for t, name in ((m, "mask"), (add, "add")):
        if t is not None:
            _need(t, dy.dtype, name)
            if tuple(t.shape) != (n, hi, wi, cin):
                raise OsrError(f"{name} shape {tuple(t.shape)} != {(n, hi, wi, cin)}")
    out_dtype = out_dtype or dy.dtype
    if FLOP_COUNT is not None:
        FLOP_COUNT["conv"] += 2.0 * n * hi * wi * cin * cout * 9 / 4
    dx = torch.empty((n, hi, wi, cin), dtype=out_dtype, device=dy.device)
    p = _conv_params(n, hi, wi, cin, ho, wo, cout, 3, 3, 2, 1, dy.dtype, out_dtype)
    check(lib.osr_conv2d_dgrad_s2(C.byref(p), _p(dy), _p(w_dgrad), _p(m), _p(add), _p(dx), _stream()), "osr_conv2d_dgrad_s2")
    return dx


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, kh: int, kw: int, stride: int = 1, pad: int = 0, dw: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """Weight gradient in the packed forward layout (cout,kh,kw,cin), fp32. x (n,hi,wi,cin), dy (n,ho,wo,cout) f16/bf16."""
    lib = _lib.load()
    _need(x, name="x"); _need(dy, x.dtype, "dy")
    n, hi, wi, cin = x.shape
    n2, ho, wo, cout = dy.shape
    if n2 != n or (hi + 2 * pad - kh) // stride + 1 != ho or (wi + 2 * pad - kw) // stride + 1 != wo:
        raise OsrError("dy shape inconsistent with x and the kernel geometry")
    if FLOP_COUNT is not None:
        FLOP_COUNT["wgrad"] += 2.0 * n * ho * wo * cout * kh * kw * cin
    p = _conv_params(n, hi, wi, cin, ho, wo, cout, kh, kw, stride, pad, x.dtype, x.dtype)
    if dw is None:
        dw = torch.empty((cout, kh, kw, cin), dtype=torch.float32, device=x.device)
        accumulate = False
    else:
        _need(dw, torch.float32, "dw")
    wsb = lib.osr_conv2d_wgrad_workspace_bytes(C.byref(p))
    if wsb < 0:
        check(int(wsb), "osr_conv2d_wgrad_workspace_bytes")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    check(lib.osr_conv2d_wgrad(C.byref(p), _p(x), _p(dy), _p(dw), int(accumulate), _p(ws), wsb, _stream()), "osr_conv2d_wgrad")
    return dw


def linear_wgrad(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dW (n_out, k) fp32 of a fully connected layer: x (m,k), dy (m,n_out)."""
    m, k = x.shape
    return conv2d_wgrad(x.view(1, m, 1, k), dy.view(1, m, 1, dy.shape[1]), 1, 1).view(dy.shape[1], k)


def bias_grad(dy: torch.Tensor, db: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """db[c] = sum over all leading dimensions of dy[..., c] (fp32)."""
    lib = _lib.load()
    _need(dy, name="dy")
    cout = dy.shape[-1]
    m = dy.numel() // cout
    if db is None:
        db = torch.empty((cout,), dtype=torch.float32, device=dy.device)
        accumulate = False
    ws = torch.empty((512 * cout * 4,), dtype=torch.uint8, device=dy.device)
    check(lib.osr_bias_grad(_p(dy), _DT[dy.dtype], m, cout, _p(db), int(accumulate), _p(ws), ws.numel(), _stream()), "osr_bias_grad")
    return db


# ----------------------------------------------------------------------------------------------------------
# training step, backward half: losses, per-row stages, elementwise, optimiser
# ----------------------------------------------------------------------------------------------------------
def rpn_losses_bwd(lv: RpnLevels, cell_anchors, n: int, pred_deltas, pred_ctr, labels_reg, labels_obj, matched_boxes, ctr_target,
                   loc_weight=0.5, ctr_weight=0.5, batch_size_per_image=256, loss_scale=1.0, box_loss=("iou", 0.0), ctr_beta=0.0) -> torch.Tensor:
    """-> d_out5 (rows, 5) fp32, level-major: gradient w.r.t. the head's {4 deltas, centerness logit}."""
    lib = _lib.load()
    out = torch.empty((pred_ctr.numel(), 5), dtype=torch.float32, device=pred_ctr.device)
    opt = _loss_options(box_loss, ctr_beta)
    check(lib.osr_rpn_losses_bwd_ex(C.byref(lv), _p(cell_anchors), n, _p(pred_deltas), _p(pred_ctr), _p(labels_reg), _p(labels_obj),
                                    _p(matched_boxes), _p(ctr_target), loc_weight, ctr_weight, batch_size_per_image, loss_scale, C.byref(opt), _p(out),
                                    _stream()), "osr_rpn_losses_bwd")
    return out


def cfrpn_tail_bwd(t: torch.Tensor, w_tail: torch.Tensor, d_out5: torch.Tensor):
    """t (rows,256) f16/bf16, w_tail (5,256) fp32, d_out5 (rows,5) fp32 -> dt (rows,256) like t, dw_tail (5,256), db_tail (5)."""
    lib = _lib.load()
    _need(t, name="t"); _need(w_tail, torch.float32, "w_tail"); _need(d_out5, torch.float32, "d_out5")
    rows = t.shape[0]
    dt = torch.empty_like(t)
    dw = torch.empty((5, 256), dtype=torch.float32, device=t.device)
    db = torch.empty((5,), dtype=torch.float32, device=t.device)
    wsb = lib.osr_cfrpn_tail_bwd_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device=t.device)
    check(lib.osr_cfrpn_tail_bwd(_p(t), _DT[t.dtype], rows, _p(w_tail), _p(d_out5), _p(dt), _p(dw), _p(db), 0, _p(ws), wsb, _stream()),
          "osr_cfrpn_tail_bwd")
    return dt, dw, db


def rpn_sparse_rows(d_out5: torch.Tensor, cap: int):
    """The rows of d_out5 (rows,5) with a non-zero gradient: (row_ids (cap) int32 ascending, -1 behind them; row_map (rows) int32 =
    list slot or -1; count2 = {listed, found})."""
    lib = _lib.load()
    _need(d_out5, torch.float32, "d_out5")
    rows = d_out5.shape[0]
    dev = d_out5.device
    ids = torch.empty((cap,), dtype=torch.int32, device=dev)
    rmap = torch.empty((rows,), dtype=torch.int32, device=dev)
    cnt = torch.empty((2,), dtype=torch.int32, device=dev)
    wsb = lib.osr_rpn_sparse_rows_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib.osr_rpn_sparse_rows(_p(d_out5), rows, cap, _p(ids), _p(rmap), _p(cnt), _p(ws), wsb, _stream()), "osr_rpn_sparse_rows")
    return ids, rmap, cnt


def rpn_gather_cols(lv: RpnLevels, feats: List[torch.Tensor], n: int, row_ids: torch.Tensor, d_out5: torch.Tensor):
    """-> (cols (cap, 2304) in the feature dtype: the im2col rows (tap-major) of the listed anchors; d_out5_rows (cap, 5))."""
    lib = _lib.load()
    _need(row_ids, torch.int32, "row_ids"); _need(d_out5, torch.float32, "d_out5")
    py = _pyramid(feats, [1.0] * len(feats))
    cap = row_ids.shape[0]
    cols = torch.empty((cap, 9 * 256), dtype=feats[0].dtype, device=row_ids.device)
    d5r = torch.empty((cap, 5), dtype=torch.float32, device=row_ids.device)
    check(lib.osr_rpn_gather_cols(C.byref(lv), C.byref(py), _DT[feats[0].dtype], n, _p(row_ids), cap, _p(d_out5), _p(cols), _p(d5r), _stream()),
          "osr_rpn_gather_cols")
    return cols, d5r


def rpn_scatter_cols_add_(lv: RpnLevels, n: int, row_map: torch.Tensor, y: torch.Tensor, grads: List[torch.Tensor]) -> List[torch.Tensor]:
    """In place on grads[l] (n, h_l, w_l, 256): += the per-tap data gradients y (cap, 2304) fp32 of the listed anchors (col2im)."""
    lib = _lib.load()
    _need(row_map, torch.int32, "row_map"); _need(y, torch.float32, "y")
    for i, gr in enumerate(grads):
        _need(gr, grads[0].dtype, f"grads[{i}]")
        if gr.shape[0] != n or gr.shape[1] != lv.h[i] or gr.shape[2] != lv.w[i] or gr.shape[3] != 256:
            raise OsrError(f"grads[{i}] must be ({n}, {lv.h[i]}, {lv.w[i]}, 256)")
    if len(grads) != lv.num_levels or y.shape[1] != 9 * 256:
        raise OsrError("one gradient tensor per level; y must be (cap, 2304)")
    ptrs = (C.c_void_p * len(grads))(*[gr.data_ptr() for gr in grads])
    check(lib.osr_rpn_scatter_cols_add(C.byref(lv), n, _p(row_map), _p(y), ptrs, _DT[grads[0].dtype], _stream()), "osr_rpn_scatter_cols_add")
    return grads


def roi_box_losses_bwd(pred5, proposal_boxes, gt_boxes, gt_classes, gt_iou, num_classes: int, reg_weights=(10.0, 10.0, 5.0, 5.0),
                       box_weight=0.5, iou_weight=0.5, loss_scale=1.0, box_loss=("smooth_l1", 0.0), iou_beta=0.0) -> torch.Tensor:
    lib = _lib.load()
    _need(pred5, torch.float32, "pred5")
    m = gt_classes.numel()
    out = torch.empty((m, 5), dtype=torch.float32, device=pred5.device)
    ws = torch.empty((16,), dtype=torch.uint8, device=pred5.device)
    rw = (C.c_float * 4)(*reg_weights)
    opt = _loss_options(box_loss, iou_beta)
    check(lib.osr_roi_box_losses_bwd_ex(_p(pred5), _p(proposal_boxes), _p(gt_boxes), _p(gt_classes), _p(gt_iou), m, num_classes, rw, box_weight,
                                        iou_weight, loss_scale, C.byref(opt), _p(out), _p(ws), 16, _stream()), "osr_roi_box_losses_bwd")
    return out


def softmax_ce_loss_bwd(logits, gt_classes, num_classes: int, loss_weight: float, loss_scale=1.0) -> torch.Tensor:
    lib = _lib.load()
    _need(logits, torch.float32, "logits")
    m, nk1 = logits.shape
    out = torch.empty_like(logits)
    ws = torch.empty((16,), dtype=torch.uint8, device=logits.device)
    check(lib.osr_softmax_ce_loss_bwd(_p(logits), m, nk1 - 1, _p(gt_classes), num_classes, loss_weight, loss_scale, _p(out), _p(ws), 16, _stream()),
          "osr_softmax_ce_loss_bwd")
    return out


def pln_loss_bwd(emb, protos_raw, gt_classes, ious, iou_thr: float, alpha: float, beta: float, loss_weight: float, loss_scale=1.0, reps: int = 1,
                 distance: str = "COS"):
    """-> (d_emb (m,d), d_protos (K * reps,d)) fp32; protos_raw are the un-normalised prototype parameters."""
    lib = _lib.load()
    _need(emb, torch.float32, "emb"); _need(protos_raw, torch.float32, "protos_raw")
    m, d = emb.shape
    de = torch.empty_like(emb)
    dp = torch.empty_like(protos_raw)
    wsb = lib.osr_pln_loss_bwd_workspace_bytes(m)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=emb.device)
    assert protos_raw.shape[0] % reps == 0
    check(lib.osr_pln_loss_bwd_ex(_p(emb), m, d, _p(protos_raw), protos_raw.shape[0] // reps, reps, _pln_distance(distance), _p(gt_classes), _p(ious),
                                  iou_thr, alpha, beta, loss_weight, loss_scale, _p(de), _p(dp), 0, _p(ws), wsb, _stream()), "osr_pln_loss_bwd")
    return de, dp


def roi_align_bwd(dout: torch.Tensor, shapes: Sequence[Tuple[int, int]], n: int, scales: Sequence[float], boxes, batch_idx,
                  canonical_level: int = 4, canonical_size: int = 224, min_level: int = 2, rois_per_image: Optional[int] = None,
                  out_dtype: Optional[torch.dtype] = None, aligned: bool = True, sampling_ratio: int = 0,
                  per_sample: bool = False) -> List[torch.Tensor]:
    """dout (m,P,P,c) -> list of (n,h,w,c) feature gradients, one per level: fp32, or out_dtype (= dout's dtype: the fp32 sums rounded
    once; the scatter path casts afterwards). rois_per_image: the list is image-major with this
    fixed stride (rows [b*S, (b+1)*S) are image b's or padding) -- the pixel-centric kernel then gathers (osr_roi_align_bwd_dense: no
    atomics, no zero fill, reproducible bit for bit); otherwise the scatter kernel adds into a zeroed pyramid with fp32 atomics.
    aligned / sampling_ratio: the forward's (roi_align).
    per_sample: pooled 8 .. MAX_POOLED_FWD (the mask pooler) exist only as the scatter kernel's per-sample form (osr_roi_align_bwd:
    one workgroup per RoI, fp32 atomics, not bitwise reproducible, whatever rois_per_image says); a caller asks for it by name,
    otherwise those sizes stay refused as they always were."""
    lib = _lib.load()
    opt = _roi_options(aligned, sampling_ratio)
    _need(dout, name="dout"); _need(boxes, torch.float32, "boxes"); _need(batch_idx, torch.int32, "batch_idx")
    m, pooled, _, c = dout.shape
    if pooled > 7 and not per_sample:
        raise OsrError(f"roi_align_bwd: pooled size 1..7, got {pooled} (8..{MAX_POOLED_FWD}: the per-sample scatter, per_sample=True)")
    # (pooled 8..14, the mask pooler: the scatter kernel's per-sample form; the pixel-centric kernel holds 7 bins per axis)
    dense = rois_per_image is not None and m == n * rois_per_image and rois_per_image <= 1024 and c <= 256 and pooled <= 7
    if out_dtype not in (None, torch.float32, dout.dtype):
        raise OsrError("roi_align_bwd: out_dtype must be float32 or dout's dtype")
    odt = out_dtype or torch.float32
    outs = [torch.empty((n, h, w, c), dtype=odt, device=dout.device) if dense else torch.zeros((n, h, w, c), dtype=torch.float32, device=dout.device)
            for h, w in shapes]
    py = Pyramid()
    py.num_levels, py.c = len(outs), c
    for i, (f, s) in enumerate(zip(outs, scales)):
        py.h[i], py.w[i], py.scale[i], py.data[i] = f.shape[1], f.shape[2], float(s), f.data_ptr()
    if dense:
        st = lib.osr_roi_align_bwd_dense_opt(C.byref(py), n, _p(boxes), _p(batch_idx), m, int(rois_per_image), pooled, canonical_level,
                                             canonical_size, min_level, _p(dout), _DT[dout.dtype], _DT[odt], opt, _stream())
        if st != _lib.ERR_UNSUPPORTED:
            check(st, "osr_roi_align_bwd_dense")
            return outs
        outs = [torch.zeros((n, h, w, c), dtype=torch.float32, device=dout.device) for h, w in shapes]
        for i, f in enumerate(outs):
            py.data[i] = f.data_ptr()
    check(lib.osr_roi_align_bwd_opt(C.byref(py), n, _p(boxes), _p(batch_idx), m, pooled, canonical_level, canonical_size, min_level, _p(dout),
                                    _DT[dout.dtype], opt, _stream()), "osr_roi_align_bwd")
    return outs if odt == torch.float32 else [add_cast(f, None, odt) for f in outs]


def relu_mask_(g: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(g, name="g"); _need(act, name="act")
    if g.numel() != act.numel():
        raise OsrError("relu_mask_: size mismatch")
    check(lib.osr_relu_mask(_p(g), _DT[g.dtype], _p(act), _DT[act.dtype], g.numel(), _stream()), "osr_relu_mask")
    return g


def add_cast(a_f32: Optional[torch.Tensor], b: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    lib = _lib.load()
    ref = a_f32 if a_f32 is not None else b
    if a_f32 is not None:
        _need(a_f32, torch.float32, "a_f32")
    if b is not None:
        _need(b, dtype, "b")
    out = torch.empty(ref.shape, dtype=dtype, device=ref.device)
    check(lib.osr_add_cast(_p(a_f32), _p(b), _p(out), _DT[dtype], out.numel(), _stream()), "osr_add_cast")
    return out


def pool_bwd(src: torch.Tensor, out_hw: Tuple[int, int], base: Optional[torch.Tensor], mode: int) -> torch.Tensor:
    """mode 0: FPN top-down backward (out = base + 2x2 sums of src); mode 1: p6 subsample backward."""
    lib = _lib.load()
    _need(src, name="src")
    n, hs, ws_, c = src.shape
    ho, wo = out_hw
    if base is not None:
        _need(base, src.dtype, "base")
    out = torch.empty((n, ho, wo, c), dtype=src.dtype, device=src.device)
    check(lib.osr_pool_bwd(_p(src), hs, ws_, _p(base), _p(out), n, ho, wo, c, mode, _DT[src.dtype], _stream()), "osr_pool_bwd")
    return out


def pack_dgrad_weight(w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(cout,kh,kw,cin) -> (cin,kh,kw,cout) spatially flipped (a 2-d (n,k) matrix is transposed to (k,n)); out: reuse this buffer."""
    lib = _lib.load()
    _need(w, name="w")
    if w.dim() == 2:
        cout, cin, kh, kw = w.shape[0], w.shape[1], 1, 1
        shape = (cin, cout)
    else:
        cout, kh, kw, cin = w.shape
        shape = (cin, kh, kw, cout)
    if out is None:
        out = torch.empty(shape, dtype=w.dtype, device=w.device)
    else:
        _need(out, w.dtype, "out")
        if out.numel() != w.numel():
            raise OsrError("pack_dgrad_weight: out has the wrong size")
    check(lib.osr_pack_dgrad_weight(_p(w), _p(out), cout, kh, kw, cin, _DT[w.dtype], _stream()), "osr_pack_dgrad_weight")
    return out


class MultiTensorPlan:
    """Device-resident table + chunk list of a multi-tensor launch (osr_sgd_step_multi_ex / osr_pack_dgrad_weight_multi). `keep` holds the
    tensors the table points at: the plan is only valid while they live at the same addresses."""

    def __init__(self, table: torch.Tensor, chunks: torch.Tensor, num_chunks: int, keep, chunk_elems: int = 0):
        self.table, self.chunks, self.num_chunks, self.keep, self.chunk_elems = table, chunks, num_chunks, keep, chunk_elems


def _upload_struct_array(arr, device) -> torch.Tensor:
    raw = bytes(memoryview(arr).cast("B"))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


SGD_CHUNK_ELEMS = 16384


CLIP_MODES = {None: _lib.OSR_CLIP_NONE, "value": _lib.OSR_CLIP_VALUE, "norm": _lib.OSR_CLIP_NORM}


def sgd_segment_plan(entries, device) -> MultiTensorPlan:
    """The table of osr_sgd_step_multi_ex / osr_grad_norm_partials. entries: [(param, grad, momentum_buf, row_scale | None, lowp | None,
    row0, row1, lr_factor, weight_decay, nesterov)]: one parameter each, rows [row0, row1) of the leading dimension of a master (fp32
    param / grad / buf of equal size). The plan also owns the norm partials (float64, one per chunk)."""
    tab = (_lib.SgdSegment * len(entries))()
    chunks: List[int] = []
    keep = []
    for ti, (pm, gr, buf, rs, lp, r0, r1, lr_factor, wd, nesterov) in enumerate(entries):
        _need(pm, torch.float32, "param"); _need(gr, torch.float32, "grad"); _need(buf, torch.float32, "buf")
        if gr.numel() != pm.numel() or buf.numel() != pm.numel() or (lp is not None and lp.numel() != pm.numel()):
            raise OsrError("sgd_segment_plan: size mismatch")
        rows = pm.shape[0]
        if not 0 <= r0 < r1 <= rows:
            raise OsrError(f"sgd_segment_plan: rows [{r0}, {r1}) outside a master of {rows} rows")
        re = pm.numel() // rows
        if rs is not None:
            _need(rs, torch.float32, "row_scale")
            if rs.numel() != rows:
                raise OsrError("sgd_segment_plan: row_scale must hold one value per row")
        if lp is not None:
            _need(lp, name="lowp")
        t = tab[ti]
        off = r0 * re
        t.param, t.grad, t.momentum = pm.data_ptr() + 4 * off, gr.data_ptr() + 4 * off, buf.data_ptr() + 4 * off
        t.row_scale = rs.data_ptr() + 4 * r0 if rs is not None else None
        t.lowp = lp.data_ptr() + lp.element_size() * off if lp is not None else None
        t.n = (r1 - r0) * re
        t.row_elems = re if rs is not None else 1
        t.lowp_dtype = _DT[lp.dtype] if lp is not None else 0
        t.chunk0 = len(chunks) // 2
        t.nchunks = (t.n + SGD_CHUNK_ELEMS - 1) // SGD_CHUNK_ELEMS
        t.lr_factor, t.weight_decay, t.nesterov = float(lr_factor), float(wd), int(bool(nesterov))
        for c in range(t.nchunks):
            chunks += [ti, c]
        keep += [pm, gr, buf, rs, lp]
    ch = torch.tensor(chunks, dtype=torch.int32).to(device)
    plan = MultiTensorPlan(_upload_struct_array(tab, device), ch, len(chunks) // 2, keep, SGD_CHUNK_ELEMS)
    plan.partials = torch.zeros((max(plan.num_chunks, 1),), dtype=torch.float64, device=device)
    plan.segments = [(t.chunk0, t.nchunks) for t in tab]
    return plan


def grad_norm_partials_(plan: MultiTensorPlan, grad_scale: float, norm_type: float, finite_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """osr_grad_norm_partials: plan.partials[c] = sum over chunk c of |grad*grad_scale*row_scale|^norm_type (max for inf); clears
    finite_flag where a gradient of the plan is inf / NaN. Returns plan.partials."""
    lib = _lib.load()
    if finite_flag is not None:
        _need(finite_flag, torch.int32, "finite_flag")
    check(lib.osr_grad_norm_partials(_p(plan.table), _p(plan.chunks), plan.num_chunks, plan.chunk_elems, grad_scale, float(norm_type),
                                     _p(plan.partials), _p(finite_flag), _stream()), "osr_grad_norm_partials")
    return plan.partials


def sgd_step_multi_ex_(plan: MultiTensorPlan, lr: float, momentum: float, grad_scale: float = 1.0, clip: Optional[str] = None,
                       clip_value: float = 1.0, norm_type: float = 2.0, apply_flag: Optional[torch.Tensor] = None) -> None:
    """osr_sgd_step_multi_ex over every segment of the plan, one launch. clip None / "value" / "norm" ("norm" reads the partials of
    the grad_norm_partials_ call before it)."""
    lib = _lib.load()
    if clip not in CLIP_MODES:
        raise ValueError(f"clip mode {clip!r}: None, 'value' or 'norm'")
    check(lib.osr_sgd_step_multi_ex(_p(plan.table), _p(plan.chunks), plan.num_chunks, plan.chunk_elems, lr, momentum, grad_scale, CLIP_MODES[clip],
                                    clip_value, float(norm_type), _p(plan.partials), _p(apply_flag), _stream()), "osr_sgd_step_multi_ex")


def pack_dgrad_multi_plan(pairs, device) -> MultiTensorPlan:
    """pairs: [(w, out)] as pack_dgrad_weight takes them (w (cout,kh,kw,cin) or a 2-d (n,k) matrix; out of the same size and dtype)."""
    tab = (_lib.PackTensor * len(pairs))()
    chunks: List[int] = []
    keep = []
    for ti, (w, out) in enumerate(pairs):
        _need(w, name="w"); _need(out, w.dtype, "out")
        if out.numel() != w.numel() or w.element_size() not in (2, 4):
            raise OsrError("pack_dgrad_multi_plan: out has the wrong size / unsupported element size")
        cout, kh, kw, cin = (w.shape[0], 1, 1, w.shape[1]) if w.dim() == 2 else tuple(w.shape)
        t = tab[ti]
        t.src, t.dst, t.cout, t.kh, t.kw, t.cin, t.elem_bytes = w.data_ptr(), out.data_ptr(), cout, kh, kw, cin, w.element_size()
        for c in range(kh * kw * ((cout + 31) // 32) * ((cin + 31) // 32)):
            chunks += [ti, c]
        keep += [w, out]
    ch = torch.tensor(chunks, dtype=torch.int32).to(device)
    return MultiTensorPlan(_upload_struct_array(tab, device), ch, len(chunks) // 2, keep)


def pack_dgrad_weight_multi_(plan: MultiTensorPlan) -> None:
    """osr_pack_dgrad_weight on every pair of the plan, one launch."""
    lib = _lib.load()
    check(lib.osr_pack_dgrad_weight_multi(_p(plan.table), _p(plan.chunks), plan.num_chunks, _stream()), "osr_pack_dgrad_weight_multi")


_ZERO_BIAS = {}


def _zero_bias(n: int, device) -> torch.Tensor:
    """A shared all-zero fp32 bias (the data-gradient launches have none): allocated and filled once per (size, device)."""
    key = (n, str(device))
    if key not in _ZERO_BIAS:
        _ZERO_BIAS[key] = torch.zeros((n,), dtype=torch.float32, device=device)
    return _ZERO_BIAS[key]


def check_finite_(x: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """Clears flag (int32 (1,), preset to 1 by the caller) when x holds an inf / NaN. Asynchronous."""
    lib = _lib.load()
    _need(x, torch.float32, "x"); _need(flag, torch.int32, "flag")
    check(lib.osr_check_finite(_p(x), x.numel(), _p(flag), _stream()), "osr_check_finite")
    return flag


def sgd_step_(param, grad, buf, lr: float, momentum: float, weight_decay: float, grad_scale: float = 1.0, row_scale=None, lowp=None,
              apply_flag: Optional[torch.Tensor] = None):
    """Plain SGD on one tensor: a one-segment plan through sgd_step_multi_ex_ (a convenience: a training step builds its plan once)."""
    plan = sgd_segment_plan([(param, grad, buf, row_scale, lowp, 0, param.shape[0], 1.0, weight_decay, False)], param.device)
    sgd_step_multi_ex_(plan, lr, momentum, grad_scale, apply_flag=apply_flag)


# ----------------------------------------------------------------------------------------------------------
# stock heads (Base-RCNN-FPN.yaml: RPN + StandardROIHeads): losses, their gradients, the RPN head's tail backward
# ----------------------------------------------------------------------------------------------------------
def _f4(vals) -> "C.Array":
    return (C.c_float * 4)(*[float(v) for v in vals])


def std_rpn_losses_fwd(lv: RpnLevels, cell_anchors, n: int, pred_logits, pred_deltas, labels, matched_boxes, b2b_weights=(1.0, 1.0, 1.0, 1.0),
                       beta: float = 0.0, cls_weight: float = 1.0, loc_weight: float = 1.0, batch_size_per_image: int = 256) -> torch.Tensor:
    """[d2] RPN.losses: pred_logits (rows*A,) / pred_deltas (rows*A, 4) level-major, labels (n,R) int8, matched_boxes (n,R,4).
    Returns 4 floats: loss_rpn_cls, loss_rpn_loc, num_pos, num_neg."""
    lib = _lib.load()
    _need(pred_logits, torch.float32, "pred_logits"); _need(pred_deltas, torch.float32, "pred_deltas")
    _need(labels, torch.int8, "labels"); _need(matched_boxes, torch.float32, "matched_boxes")
    dev = pred_logits.device
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    ws = _loss_ws(dev, 4)
    check(lib.osr_std_rpn_losses_fwd(C.byref(lv), _p(cell_anchors), n, _p(pred_logits), _p(pred_deltas), _p(labels), _p(matched_boxes),
                                     _f4(b2b_weights), beta, cls_weight, loc_weight, batch_size_per_image, _p(out), _p(ws), ws.numel(), _stream()),
          "osr_std_rpn_losses_fwd")
    return out


def std_rpn_losses_bwd(lv: RpnLevels, cell_anchors, n: int, pred_logits, pred_deltas, labels, matched_boxes, b2b_weights=(1.0, 1.0, 1.0, 1.0),
                       beta: float = 0.0, cls_weight: float = 1.0, loc_weight: float = 1.0, batch_size_per_image: int = 256,
                       loss_scale: float = 1.0) -> torch.Tensor:
    """Gradient of std_rpn_losses_fwd times loss_scale: (rows, 5A) fp32 over the pixel rows -- A logit columns, then 4A delta columns."""
    lib = _lib.load()
    _need(pred_logits, torch.float32, "pred_logits"); _need(pred_deltas, torch.float32, "pred_deltas")
    _need(labels, torch.int8, "labels"); _need(matched_boxes, torch.float32, "matched_boxes")
    a = lv.num_anchors
    d = torch.empty((pred_logits.numel() // a, 5 * a), dtype=torch.float32, device=pred_logits.device)
    check(lib.osr_std_rpn_losses_bwd(C.byref(lv), _p(cell_anchors), n, _p(pred_logits), _p(pred_deltas), _p(labels), _p(matched_boxes),
                                     _f4(b2b_weights), beta, cls_weight, loc_weight, batch_size_per_image, loss_scale, _p(d), _stream()),
          "osr_std_rpn_losses_bwd")
    return d


def fastrcnn_losses_fwd(logits, pred_deltas, proposal_boxes, gt_boxes, gt_classes, num_classes: int, cls_agnostic: bool,
                        reg_weights=(10.0, 10.0, 5.0, 5.0), beta: float = 0.0, cls_weight: float = 1.0, box_weight: float = 1.0) -> torch.Tensor:
    """[d2] FastRCNNOutputLayers.losses over the sampled rows (class -1 = padding). Returns 7 floats: loss_cls, loss_box_reg, rows,
    correct, foreground, foreground correct, foreground predicted as background."""
    lib = _lib.load()
    _need(logits, torch.float32, "logits"); _need(proposal_boxes, torch.float32, "proposal_boxes"); _need(gt_boxes, torch.float32, "gt_boxes")
    _need(gt_classes, torch.int64, "gt_classes"); _need(pred_deltas, torch.float32, "pred_deltas")
    m = logits.shape[0]
    out = torch.empty((7,), dtype=torch.float32, device=logits.device)
    ws = _loss_ws(logits.device, 7)
    check(lib.osr_fastrcnn_losses_fwd(_p(logits), _p(pred_deltas), pred_deltas.shape[1], int(cls_agnostic), _p(proposal_boxes), _p(gt_boxes),
                                      _p(gt_classes), m, num_classes, _f4(reg_weights), beta, cls_weight, box_weight, _p(out), _p(ws), ws.numel(),
                                      _stream()), "osr_fastrcnn_losses_fwd")
    return out


def fastrcnn_losses_bwd(logits, pred_deltas, proposal_boxes, gt_boxes, gt_classes, num_classes: int, cls_agnostic: bool,
                        reg_weights=(10.0, 10.0, 5.0, 5.0), beta: float = 0.0, cls_weight: float = 1.0, box_weight: float = 1.0,
                        loss_scale: float = 1.0):
    """Gradient of fastrcnn_losses_fwd times loss_scale: (d_logits (m, K+1), d_deltas (m, 4 | 4K)), fp32."""
    lib = _lib.load()
    _need(logits, torch.float32, "logits"); _need(pred_deltas, torch.float32, "pred_deltas")
    _need(proposal_boxes, torch.float32, "proposal_boxes"); _need(gt_boxes, torch.float32, "gt_boxes"); _need(gt_classes, torch.int64, "gt_classes")
    m = logits.shape[0]
    dl = torch.empty_like(logits)
    dd = torch.empty_like(pred_deltas)
    ws = torch.empty((16,), dtype=torch.uint8, device=logits.device)
    check(lib.osr_fastrcnn_losses_bwd(_p(logits), _p(pred_deltas), pred_deltas.shape[1], int(cls_agnostic), _p(proposal_boxes), _p(gt_boxes),
                                      _p(gt_classes), m, num_classes, _f4(reg_weights), beta, cls_weight, box_weight, loss_scale, _p(dl), _p(dd),
                                      _p(ws), ws.numel(), _stream()), "osr_fastrcnn_losses_bwd")
    return dl, dd


def std_rpn_tail_bwd(t: torch.Tensor, w_tail: torch.Tensor, d_rows: torch.Tensor, dt_dtype: torch.dtype,
                     dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None):
    """t (rows,256) fp32 (after the 3x3 conv's ReLU), w_tail (5A,256) = [W_obj; W_delta], d_rows (rows,5A) -> dt (rows,256) in dt_dtype
    (masked by t > 0), dw_tail (5A,256), db_tail (5A) -- written into dw / db when given (e.g. the gradient buffer's views)."""
    lib = _lib.load()
    _need(t, torch.float32, "t"); _need(w_tail, torch.float32, "w_tail"); _need(d_rows, torch.float32, "d_rows")
    rows, q = d_rows.shape
    if t.shape != (rows, 256) or w_tail.shape != (q, 256):
        raise OsrError("std_rpn_tail_bwd: t (rows,256), w_tail (width,256), d_rows (rows,width)")
    dt = torch.empty((rows, 256), dtype=dt_dtype, device=t.device)
    if dw is None:
        dw = torch.empty((q, 256), dtype=torch.float32, device=t.device)
    if db is None:
        db = torch.empty((q,), dtype=torch.float32, device=t.device)
    _need(dw, torch.float32, "dw"); _need(db, torch.float32, "db")
    if dw.shape != (q, 256) or db.shape != (q,):
        raise OsrError("std_rpn_tail_bwd: dw (width,256), db (width)")
    wsb = lib.osr_std_rpn_tail_bwd_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device=t.device)
    check(lib.osr_std_rpn_tail_bwd(_p(t), rows, _p(w_tail), q, _p(d_rows), _p(dt), _DT[dt_dtype], _p(dw), _p(db), _p(ws), wsb, _stream()),
          "osr_std_rpn_tail_bwd")
    return dt, dw, db


def rpn_sparse_rows_ex(d_rows: torch.Tensor, cap: int):
    """rpn_sparse_rows for a gradient of any row width (d_rows (rows, width) fp32)."""
    lib = _lib.load()
    _need(d_rows, torch.float32, "d_rows")
    rows, width = d_rows.shape
    dev = d_rows.device
    ids = torch.empty((cap,), dtype=torch.int32, device=dev)
    rmap = torch.empty((rows,), dtype=torch.int32, device=dev)
    cnt = torch.empty((2,), dtype=torch.int32, device=dev)
    wsb = lib.osr_rpn_sparse_rows_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib.osr_rpn_sparse_rows_ex(_p(d_rows), rows, width, cap, _p(ids), _p(rmap), _p(cnt), _p(ws), wsb, _stream()), "osr_rpn_sparse_rows_ex")
    return ids, rmap, cnt


def rpn_gather_cols_ex(lv: RpnLevels, feats: List[torch.Tensor], n: int, row_ids: torch.Tensor, d_rows: torch.Tensor):
    """rpn_gather_cols for a gradient of any row width: -> (cols (cap, 2304), d_rows of the listed rows (cap, width)). lv: pixel levels."""
    lib = _lib.load()
    _need(row_ids, torch.int32, "row_ids"); _need(d_rows, torch.float32, "d_rows")
    py = _pyramid(feats, [1.0] * len(feats))
    cap, width = row_ids.shape[0], d_rows.shape[1]
    cols = torch.empty((cap, 9 * 256), dtype=feats[0].dtype, device=row_ids.device)
    dl = torch.empty((cap, width), dtype=torch.float32, device=row_ids.device)
    check(lib.osr_rpn_gather_cols_ex(C.byref(lv), C.byref(py), _DT[feats[0].dtype], n, _p(row_ids), cap, _p(d_rows), width, _p(cols), _p(dl),
                                     _stream()), "osr_rpn_gather_cols_ex")
    return cols, dl
