"""References for the keypoint branch (no tests here): torch CPU code written from the contracts in include/osr.h
(osr_keypoint_upsample, osr_heatmaps_to_keypoints), evaluated in float64 on the stored operands, and the same chains in fp32 as the
yardstick of what single precision itself costs. Nothing here imports the package."""
import math

import torch
import torch.nn.functional as F


def upsample_chain(x_nhwc: torch.Tensor, w: torch.Tensor, b: torch.Tensor, dtype=torch.float64, low_dtype=None) -> torch.Tensor:
    """score_lowres + bilinear x2: x (r, s, s, cin) NHWC, w (cin, k, 4, 4), b (k) -> heatmaps (r, k, 4s, 4s) in `dtype`.
    low_dtype: round the 2s x 2s map to that type on the way (what a kernel that stored it in half precision would compute)."""
    low = F.conv_transpose2d(x_nhwc.to(dtype).permute(0, 3, 1, 2), w.to(dtype), b.to(dtype), stride=2, padding=1)
    if low_dtype is not None:
        low = low.to(low_dtype).to(dtype)
    return F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False)


def decode_chain(maps: torch.Tensor, rois: torch.Tensor, dtype=torch.float64) -> dict:
    """[d2] heatmaps_to_keypoints, one RoI at a time, in `dtype`: maps (r, k, m, m), rois (r, 4) fp32 xyxy.
    -> x, y, logit, score (r, k) in `dtype`; pos (r, k) int64 = py * wc + px of the first row-major maximum; gap (r, k) = largest minus
    second largest resized value (inf for a single pixel); size (r, 2) int64 {hc, wc}."""
    r, k, m, _ = maps.shape
    out = {n: torch.zeros((r, k), dtype=dtype) for n in ("x", "y", "logit", "score", "gap")}
    out["pos"] = torch.zeros((r, k), dtype=torch.int64)
    out["size"] = torch.zeros((r, 2), dtype=torch.int64)
    for i in range(r):
        x0, y0, x1, y1 = [float(v) for v in rois[i]]  # (fp32 values, exact as Python floats)
        w, h = max(x1 - x0, 1.0), max(y1 - y0, 1.0)
        assert w == max(float(rois[i, 2] - rois[i, 0]), 1.0) and h == max(float(rois[i, 3] - rois[i, 1]), 1.0), \
            "precondition: the box sides are exact in fp32, so that ceil() does not depend on the precision"
        wc, hc = int(math.ceil(w)), int(math.ceil(h))
        out["size"][i] = torch.tensor([hc, wc])
        u = F.interpolate(maps[i:i + 1].to(dtype), size=(hc, wc), mode="bicubic", align_corners=False)[0].reshape(k, -1)
        top = torch.topk(u, min(2, u.shape[1]), dim=1).values
        logit = top[:, 0]
        pos = (u == logit[:, None]).to(torch.int64).argmax(dim=1)  # (the first maximum in row-major order)
        out["pos"][i] = pos
        out["gap"][i] = top[:, 0] - top[:, 1] if u.shape[1] > 1 else float("inf")
        out["x"][i] = ((pos % wc).to(dtype) + 0.5) * (w / wc) + x0
        out["y"][i] = (torch.div(pos, wc, rounding_mode="floor").to(dtype) + 0.5) * (h / hc) + y0
        out["logit"][i] = logit
        out["score"][i] = 1.0 / torch.exp(maps[i].to(dtype).reshape(k, -1) - logit[:, None]).sum(dim=1)
    return out


def boxes_at(offsets, sizes) -> torch.Tensor:
    """(r, 4) fp32 xyxy boxes from (x0, y0) offsets and (w, h) sizes."""
    o, s = torch.tensor(offsets, dtype=torch.float32), torch.tensor(sizes, dtype=torch.float32)
    return torch.cat((o, o + s), dim=1)
