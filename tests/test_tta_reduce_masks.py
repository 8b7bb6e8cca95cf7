"""osr_tta_reduce_masks: the mean over the augmentations of the (n, topk, M, M) probability maps, those of flipped augmentations
mirrored along their last axis. A = 1 is the identity (the mirror when flagged); A = 3 with flags (0, 1, 0) lies within A * 2^-23 of
the float64 mean (A - 1 fp32 additions of values in [0, 1]: the partial sums stay below 4, so each addition rounds by at most
2^-23, and the sum is then divided by A, which leaves (A - 1) * 2^-23 / A plus the division's own rounding of a value below 1),
is zero beyond the counts, and repeats bit for bit. M = 28 takes the 16-byte path, M = 7 the scalar one -- and so does M = 28 when the
maps do not start on a 16-byte boundary (the last tests, whose output is a NaN-filled buffer of their own handed to the C entry)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, TOPK = 2, 4
COUNTS = (4, 1)


def _maps(a, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((a, N, TOPK, m, m), generator=g, dtype=torch.float32)


def _mask(m):
    live = torch.zeros((N, TOPK, 1, 1), dtype=torch.bool)
    for i, c in enumerate(COUNTS):
        live[i, :c] = True
    return live.expand(N, TOPK, m, m)


def _reduce(osr, maps, flags):
    out = osr.ops.tta_reduce_masks(maps.to(DEV), torch.tensor(flags, dtype=torch.int32, device=DEV), torch.tensor(COUNTS, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("m", [28, 7])
@pytest.mark.parametrize("flag", [0, 1])
def test_one_augmentation_is_the_identity_or_the_mirror(osr, m, flag):
    maps = _maps(1, m, 3)
    got = _reduce(osr, maps, [flag])
    want = torch.flip(maps[0], dims=[-1]) if flag else maps[0]
    assert not torch.equal(maps[0], torch.flip(maps[0], dims=[-1]))
    assert torch.equal(got[_mask(m)], want[_mask(m)])
    assert float(got[~_mask(m)].abs().max()) == 0.0


@pytest.mark.parametrize("m", [28, 7])
def test_three_augmentations(osr, m):
    a, flags = 3, [0, 1, 0]
    maps = _maps(a, m, 4)
    got = _reduce(osr, maps, flags)
    ref = torch.stack([torch.flip(maps[k], dims=[-1]) if f else maps[k] for k, f in enumerate(flags)]).double().mean(dim=0)
    live = _mask(m)
    err = float((got.double() - ref)[live].abs().max())
    print(f"M={m}: max |mean - float64 mean| {err:.3e} (bound {a * 2.0 ** -23:.3e})")
    assert err <= a * 2.0 ** -23
    assert float(got[~live].abs().max()) == 0.0  # rows beyond the counts, whatever the inputs hold there
    assert float(ref[~live].abs().max()) > 0.0
    # the stated order: ((m0 + m1) + m2) / 3 in fp32 -- bit for bit
    exact = ((maps[0] + torch.flip(maps[1], dims=[-1])) + maps[2]) / np.float32(3.0)
    assert torch.equal(got[live], exact[live])
    assert torch.equal(_reduce(osr, maps, flags), got)  # two launches


def _reduce_into(osr, maps_dev, flags):
    """osr_tta_reduce_masks on device maps (A, N, TOPK, m, m) as they lie (no copy) into a NaN-filled output of the test's own."""
    a, m = int(maps_dev.shape[0]), int(maps_dev.shape[-1])
    assert maps_dev.is_contiguous()
    flip = torch.tensor(flags, dtype=torch.int32, device=DEV)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    out = torch.full((N, TOPK, m, m), float("nan"), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    status = osr._lib.load().osr_tta_reduce_masks(p(maps_dev), p(flip), a, p(counts), N, TOPK, m, p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert not bool(torch.isnan(got).any()), "an output sample was not written"
    return got


def test_unaligned_maps_take_the_scalar_kernel_at_a_vector_eligible_size(osr):
    """m = 28 (m % 4 == 0) with maps one float into a larger allocation: 16-byte loads would fault or read the wrong samples, so the
    entry must take the scalar kernel. Same bits as the aligned call on the same values, and as the fixed-order expression."""
    a, m, flags = 3, 28, [0, 1, 0]
    maps = _maps(a, m, 5)
    big = torch.zeros(maps.numel() + 4, device=DEV)
    view = big[1:1 + maps.numel()].view(maps.shape)
    view.copy_(maps.to(DEV))
    aligned = maps.to(DEV)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    got = _reduce_into(osr, view, flags)
    assert torch.equal(got, _reduce_into(osr, aligned, flags))
    live = _mask(m)
    exact = ((maps[0] + torch.flip(maps[1], dims=[-1])) + maps[2]) / np.float32(3.0)
    assert torch.equal(got[live], exact[live])
    assert float(got[~live].abs().max()) == 0.0


@pytest.mark.parametrize("m", [28, 7, 1])
def test_two_flipped_augmentations_and_a_one_sample_map(osr, m):
    """A = 2 with both flags set: (flip(m0) + flip(m1)) / 2, one fp32 addition and an exact halving; A = 3 at m = 1, where the mirror is the
    identity and a row is a single sample."""
    maps = _maps(2, m, 6)
    got = _reduce_into(osr, maps.to(DEV), [1, 1])
    live = _mask(m)
    exact = (torch.flip(maps[0], dims=[-1]) + torch.flip(maps[1], dims=[-1])) / np.float32(2.0)
    assert torch.equal(got[live], exact[live])
    assert float(got[~live].abs().max()) == 0.0
    if m == 1:
        maps = _maps(3, m, 7)
        got = _reduce_into(osr, maps.to(DEV), [0, 1, 0])
        assert torch.equal(got[live], (((maps[0] + maps[1]) + maps[2]) / np.float32(3.0))[live])
        assert float(got[~live].abs().max()) == 0.0
