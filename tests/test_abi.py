"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, and exports exactly the entry
points include/osr.h declares; the ctypes binding covers each of them; the product path refuses to run
without a GPU instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "osr.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(osr_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_expected_surface():
    fns = _header_functions()
    for must in ("osr_conv2d_fwd", "osr_cfrpn_head_tail", "osr_rpn_select", "osr_roi_align_fwd", "osr_box_predictor_tail",
                 "osr_nms_topk", "osr_pln_tail", "osr_softmax_candidates", "osr_gemm_f32", "osr_last_error"):
        assert must in fns


def test_library_exports_every_declared_symbol(osr):
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(osr._lib.LIB_PATH)
    for fn in _header_functions():
        assert hasattr(lib, fn), f"{fn} declared in include/osr.h but not exported by libosr_hip.so"
    assert lib.osr_abi_version() == 1


def test_binding_covers_header(osr):
    assert sorted(osr._lib.PROTOTYPES) == _header_functions()


def test_struct_layouts_match_header(osr):
    L = osr._lib
    assert ctypes.sizeof(L.ConvParams) == 13 * 4 + 4 + 9 * 8 + 6 * 4 + 8 + 8 + 8 + 8  # 13 int32 (+4 pad) + 9 int64 + 6 int32 + workspace pointer + its size + row_seg_counts + row_seg_rows (+4 pad)
    assert ctypes.sizeof(L.RpnLevels) == 8 + 3 * 8 * 4 + 8 * 8
    assert ctypes.sizeof(L.Pyramid) == 8 + 3 * 8 * 4 + 8 * 8
    assert ctypes.sizeof(L.BottleneckParams) == 8 * 4
    assert ctypes.sizeof(L.ConvLevel) == 6 * 8 + 4 * 4 and L.MAX_CONV_LEVELS == 6  # osr_conv_level: six pointers + n, hi, wi, reserved; OSR_MAX_CONV_LEVELS
    assert ctypes.sizeof(L.SgdSegment) == 80 and ctypes.sizeof(L.PackTensor) == 2 * 8 + 6 * 4


def test_argument_validation_needs_no_gpu(osr):
    lib = osr._lib.load()
    p = osr._lib.ConvParams()
    st = lib.osr_conv2d_fwd(ctypes.byref(p), None, None, None, None, None, None)
    assert st == -1 and b"null pointer" in lib.osr_last_error()
    assert lib.osr_stem_padded_width(1344) == 1352
    lv = osr.ops.make_rpn_levels([(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], (4, 8, 16, 32, 64), 16)
    assert lib.osr_rpn_select_capacity(ctypes.byref(lv), 1000) == 4273
    assert lib.osr_rpn_select_capacity(ctypes.byref(lv), 2000) == 7323
    assert lib.osr_rpn_select_capacity(ctypes.byref(lv), 5000) == -1


def test_no_cpu_fallback(osr):
    with pytest.raises(osr.OsrError):
        osr.ops.l2_normalize_rows(torch.zeros(4, 8))  # CPU tensor: refused, not computed on the host


def test_shipped_library_has_no_environment_dependence(osr):
    """The tuning knobs are compile-time constants in the product build (an -DOSR_EXPERIMENT diagnostic build reads them from the
    environment; scripts/ab_*.sh): libosr_hip.so neither imports getenv nor carries a knob's name."""
    import subprocess
    import __graft_entry__ as ge
    ge.build()
    und = subprocess.run(["nm", "-D", "--undefined-only", osr._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    blob = open(osr._lib.LIB_PATH, "rb").read()
    for knob in (b"OSR_CONV_BK32", b"OSR_CONV_FORCE_TILE", b"OSR_CONV_MODEL_BIG", b"OSR_RPN_BIG_MIN_TILES", b"OSR_CONV_TAP_MINOR"):
        assert knob not in blob, knob
