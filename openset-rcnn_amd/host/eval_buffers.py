"""The two copies an evaluator that matches on the device makes: its tables go up in ONE buffer (`upload_sections`), and everything
it left on the device comes back in ONE buffer (`fetch_chunks`). What the arrays mean, which rows exist and what the evaluator
builds from them stay with the evaluator."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch


_TORCH = {np.dtype(n): getattr(torch, n) for n in ("float64", "float32", "int64", "int32", "uint8")}


def upload_sections(arrays: Sequence[np.ndarray], device) -> List[torch.Tensor]:
    """Each array's bytes at an 8-byte-aligned offset of one uint8 buffer, ONE host-to-device copy; -> per array a view of the device
    buffer with the array's dtype and shape (8-aligned: a float64 or int64 section may follow bytes). This runs once per batch, so
    it makes no call it can do without."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, end = [], 0
    for a in arrays:
        offs.append(end)
        end += (a.nbytes + 7) // 8 * 8
    buf = np.zeros(end, dtype=np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dbuf = torch.from_numpy(buf).to(device, non_blocking=True)
    views = [dbuf[o:o + a.nbytes].view(_TORCH[a.dtype]) for a, o in zip(arrays, offs)]
    return [v if a.ndim == 1 else v.view(a.shape) for a, v in zip(arrays, views)]


def fetch_chunks(chunks: Sequence[dict], fields: Sequence[Tuple[str, type]]) -> List[Dict[str, np.ndarray]]:
    """chunks: per batch a dict of device tensors; fields: (key, numpy dtype) of those to fetch. Every field of every chunk comes over in
    ONE device-to-host copy; -> per chunk {key: flat host array of that dtype}."""
    if not chunks:
        return []
    host = torch.cat([c[f].reshape(-1).view(torch.uint8) for c in chunks for f, _ in fields]).cpu().numpy()  # the one copy
    out, o = [], 0
    for c in chunks:
        got = {}
        for f, dt in fields:
            nbytes = c[f].numel() * c[f].element_size()
            got[f] = host[o:o + nbytes].view(dt)
            o += nbytes
        out.append(got)
    return out
