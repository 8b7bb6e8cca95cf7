"""host/eval_buffers.py on the CPU: the sections go up in one 8-aligned buffer and come back as their sources; the chunks' fields come
back bit for bit."""
import numpy as np
import torch


def test_upload_sections_are_aligned_views_of_one_buffer(osr):
    from openset_rcnn_amd.host.eval_buffers import upload_sections
    rng = np.random.default_rng(0)
    arrays = [rng.random((3, 4)), rng.integers(-9, 9, size=5), rng.integers(-9, 9, size=3).astype(np.int32), np.zeros((0, 17, 3)),
              rng.random(7).astype(np.float32), rng.integers(0, 255, size=13).astype(np.uint8), rng.random(1)]  # 96, 40, 12, 0, 28, 13, 8 bytes
    views = upload_sections(arrays, "cpu")
    assert len(views) == len(arrays)
    base = views[0].untyped_storage().data_ptr()
    end = 0
    for a, v in zip(arrays, views):
        assert v.dtype == torch.from_numpy(a).dtype and tuple(v.shape) == a.shape
        assert np.array_equal(v.numpy(), a)
        assert v.untyped_storage().data_ptr() == base  # one buffer
        if a.size:  # (an empty section has no first byte)
            off = v.data_ptr() - base
            assert off % 8 == 0 and off >= end  # 8-aligned, in order, no overlap
            end = off + a.nbytes
    assert views[0].untyped_storage().nbytes() == 96 + 40 + 16 + 0 + 32 + 16 + 8


def test_fetch_chunks_round_trips_every_field(osr):
    from openset_rcnn_amd.host.eval_buffers import fetch_chunks
    rng = np.random.default_rng(1)
    fields = (("boxes", np.float32), ("classes", np.int64), ("counts", np.int32), ("flags", np.uint32), ("bytes", np.uint8))
    chunks, want = [], []
    for n, cap in ((2, 5), (3, 8)):  # different caps: every field's length differs between the chunks
        src = dict(boxes=rng.random((n, cap, 4)).astype(np.float32), classes=rng.integers(-1, 80, size=(n, cap)), counts=rng.integers(0, cap, size=n).astype(np.int32),
                   flags=rng.integers(0, 2 ** 32, size=(n, cap, 4), dtype=np.uint32), bytes=rng.integers(0, 255, size=(n, cap)).astype(np.uint8))
        src["boxes"][0, 0, 0] = np.nan  # (bit for bit: a NaN's payload too)
        want.append(src)
        chunks.append(dict({k: torch.from_numpy(v) for k, v in src.items()}, n=n, cap=cap, unused=None))
    got = fetch_chunks(chunks, fields)
    assert len(got) == 2
    for g, w in zip(got, want):
        assert sorted(g) == sorted(k for k, _ in fields)
        for k, dt in fields:
            assert g[k].dtype == dt and g[k].ndim == 1
            assert g[k].tobytes() == w[k].tobytes()
    assert fetch_chunks([], fields) == []
