"""Argument checks of the BK=64 convolution's entry points (csrc/osr_conv_gemm64.hip, and osr_conv2d_fwd in front of it), on the CPU.

Every call below starts from a valid small problem with non-null, 16-byte aligned dummy addresses and has ONE thing wrong (the last
group: two things, which pins the order of the checks). Each must return its status before anything touches the GPU, and
osr_last_error() must name the entry point. The status is part of the ABI: on OSR_ERR_UNSUPPORTED (-2) ops.conv2d_chain,
ops.conv2d_pair, ops.conv2d_levels and ops.bottleneck take their separate-launch path, on OSR_ERR_INVALID_ARG (-1) they raise.
No call here is fully valid: a valid one would launch."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -2
F32, F16, BF16 = 0, 1, 2
A = [0x10000 * (i + 1) for i in range(16)]  # dummy addresses, never dereferenced
OFF = 8                                      # breaks the 16-byte alignment


def _params(osr, cout, k=3, cin=64, n=1, h=8, w=8, stride=1, dt=F16):
    p = osr._lib.ConvParams()
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    p.n, p.hi, p.wi, p.cin, p.ho, p.wo, p.cout = n, h, w, cin, ho, wo, cout
    p.kh, p.kw, p.stride_h, p.stride_w, p.pad_h, p.pad_w = k, k, stride, stride, pad, pad
    p.in_stride_n, p.in_stride_h, p.in_stride_w = h * w * cin, w * cin, cin
    p.out_stride_n, p.out_stride_h, p.out_stride_w = ho * wo * cout, wo * cout, cout
    p.in_dtype = p.out_dtype = dt
    p.concurrency = 1
    return p


def _set_cin(p, cin):
    p.cin = cin
    p.in_stride_n, p.in_stride_h, p.in_stride_w = p.hi * p.wi * cin, p.wi * cin, cin


def _set_k(p, k):
    p.kh = p.kw = k
    p.pad_h = p.pad_w = k // 2


def _storage(p, dt):
    p.in_dtype = p.out_dtype = dt


class Call:
    """One entry point with a valid argument set: p, the named arguments in call order, and (multi-level forms) the levels."""

    def __init__(self, osr, fn, prefix, p, args, levels=None):
        self.osr, self.fn, self.prefix, self.p, self.args, self.levels = osr, fn, prefix, p, dict(args), levels

    def run(self):
        lib = self.osr._lib.load()
        argv = []
        for k, v in self.args.items():
            if k == "p":
                argv.append(C.byref(self.p))
            elif k == "levels":
                arr = (self.osr._lib.ConvLevel * max(len(self.levels), 1))()
                for i, lv in enumerate(self.levels):
                    for f, x in lv.items():
                        setattr(arr[i], f, x)
                argv += [self.args["nlevels"] if self.args["nlevels"] is not None else len(self.levels), arr]
            elif k != "nlevels":
                argv.append(v)
        st = getattr(lib, self.fn)(*argv)
        return st, (lib.osr_last_error() or b"").decode()


def _level(i, head, n=1, h=8, w=8):
    return dict(in_=A[8] + i * 0x100, out=None if head else A[9] + i * 0x100, deltas=A[10] + i * 0x100 if head else None,
                ctr=A[11] + i * 0x100 if head else None, weight=None, bias=None, n=n, hi=h, wi=w)


def _levels_params(osr, cout=256):
    p = _params(osr, cout)
    p.n = p.hi = p.wi = p.ho = p.wo = 0  # the levels ABI: sizes come per level
    p.in_stride_n = p.in_stride_h = p.out_stride_n = p.out_stride_h = 0
    return p


ENTRIES = {
    "fwd": lambda osr: Call(osr, "osr_conv2d_fwd", "osr_conv2d_fwd", _params(osr, 64),
                            dict(p=0, inp=A[0], weight=A[1], bias=A[2], residual=None, out=A[3], stream=None)),
    "masked": lambda osr: Call(osr, "osr_conv2d_fwd_masked", "osr_conv2d_fwd", _params(osr, 64),
                               dict(p=0, inp=A[0], weight=A[1], bias=A[2], residual=None, mask=A[4], out=A[3], stream=None)),
    "head": lambda osr: Call(osr, "osr_cfrpn_head_fwd_ex", "osr_cfrpn_head_fwd", _params(osr, 256),
                             dict(p=0, inp=A[0], weight=A[1], bias=A[2], w_tail=A[3], b_tail=A[4], deltas=A[5], ctr=A[6], hidden_out=A[7], stream=None)),
    "pair": lambda osr: Call(osr, "osr_conv2d_fwd_pair", "osr_conv2d_fwd_pair", _params(osr, 256),
                             dict(p=0, inp=A[0], w_a=A[1], bias_a=A[2], cout_a=128, relu_a=0, out_a=A[3], w_b=A[4], bias_b=A[5], cout_b=128, relu_b=1,
                                  out_b=A[6], stream=None)),
    "levels": lambda osr: Call(osr, "osr_conv2d_fwd_levels", "osr_conv2d_fwd_levels", _levels_params(osr),
                               dict(p=0, nlevels=None, levels=0, weight=A[1], bias=A[2], stream=None), [_level(0, False), _level(1, False, h=4, w=4)]),
    "head_levels": lambda osr: Call(osr, "osr_cfrpn_head_fwd_levels", "osr_cfrpn_head_fwd_levels", _levels_params(osr),
                                    dict(p=0, nlevels=None, levels=0, weight=A[1], bias=A[2], w_tail=A[3], b_tail=A[4], stream=None),
                                    [_level(0, True), _level(1, True, h=4, w=4)]),
    "chain": lambda osr: Call(osr, "osr_conv2d_chain_fwd_ex", "osr_conv2d_chain_fwd", _params(osr, 128),
                              dict(p=0, inp=A[0], weight=A[1], bias=A[2], w3=A[3], bias3=A[4], cout3=512, residual=A[5], out=A[6], mid_out=A[7], stream=None)),
}
SINGLE = ("fwd", "masked", "head", "pair", "chain")   # one problem, described by p
FUSED = ("head", "pair", "levels", "head_levels", "chain")
MULTI = ("levels", "head_levels")


def _arg(name, value):
    return lambda c: c.args.__setitem__(name, value)


def _p(fn, *a):
    return lambda c: fn(c.p, *a)


def _field(name, value):
    return lambda c: setattr(c.p, name, value)


def _lv(i, name, value):
    return lambda c: c.levels[i].__setitem__(name, value)


def _both(*muts):
    return lambda c: [m(c) for m in muts]


def _bump_ho(c):
    c.p.ho += 1


CASES = []
for e in SINGLE:
    CASES += [(e, "null input", _arg("inp", None), INVALID), (e, "misaligned input", _arg("inp", A[0] + OFF), INVALID),
              (e, "ho off by one", _bump_ho, INVALID)]
for e in ("head", "pair", "chain"):
    CASES += [(e, "cin 96", _p(_set_cin, 96), UNSUPPORTED), (e, "f32 storage", _p(_storage, F32), UNSUPPORTED),
              (e, "2 GiB input by its strides", _field("in_stride_n", 1 << 30), UNSUPPORTED), (e, "in_stride_n 0", _field("in_stride_n", 0), INVALID),
              (e, "in_stride_h 4", _field("in_stride_h", 4), INVALID), (e, "stem view", _field("pad_mode", 1), UNSUPPORTED)]
for e in MULTI:
    CASES += [(e, "null level input", _lv(1, "in_", None), INVALID), (e, "misaligned level input", _lv(1, "in_", A[8] + OFF), INVALID),
              (e, "misaligned shared weight", _arg("weight", A[1] + OFF), INVALID), (e, "cin 96", _p(_set_cin, 96), UNSUPPORTED),
              (e, "f32 storage", _p(_storage, F32), UNSUPPORTED), (e, "0 levels", _arg("nlevels", 0), INVALID), (e, "7 levels", _arg("nlevels", 7), INVALID),
              (e, "stride 2", _both(_field("stride_h", 2), _field("stride_w", 2)), UNSUPPORTED), (e, "cout 128", _field("cout", 128), UNSUPPORTED),
              (e, "level of 2 GiB or more", _both(_lv(0, "n", 16), _lv(0, "hi", 2048), _lv(0, "wi", 2048)), UNSUPPORTED),
              (e, "level without rows", _lv(1, "n", 0), INVALID), (e, "even kernel", _p(_set_k, 2), UNSUPPORTED)]
CASES += [
    # (an input of 2 GiB or more alone is a valid osr_conv2d_fwd call: the BK=32 kernel takes it. With 2^32 output rows it is refused.)
    ("fwd", "2 GiB input by its strides, 2^32 rows", lambda c: setattr(c, "p", _params(c.osr, 64, n=16, h=16384, w=16384)), UNSUPPORTED),
    ("fwd", "cin 48", _p(_set_cin, 48), UNSUPPORTED), ("fwd", "cout 12", _field("cout", 12), UNSUPPORTED), ("fwd", "17 x 17 kernel", _p(_set_k, 17), INVALID),
    ("fwd", "in_stride_h 4", _field("in_stride_h", 4), INVALID), ("fwd", "res_mode 1 without residual", _field("res_mode", 1), INVALID),
    ("masked", "cin 96", _p(_set_cin, 96), UNSUPPORTED), ("masked", "null mask", _arg("mask", None), INVALID),
    ("masked", "misaligned mask", _arg("mask", A[4] + OFF), INVALID), ("masked", "res_mode 2", _both(_field("res_mode", 2), _arg("residual", A[5])), INVALID),
    ("masked", "2 GiB input by its strides", _field("in_stride_n", 1 << 30), UNSUPPORTED), ("masked", "f32 storage", _p(_storage, F32), UNSUPPORTED),
    ("head", "cout 128", _field("cout", 128), UNSUPPORTED), ("head", "residual", _field("res_mode", 1), UNSUPPORTED),
    ("head", "misaligned hidden_out", _arg("hidden_out", A[7] + OFF), INVALID), ("head", "null w_tail", _arg("w_tail", None), INVALID),
    ("head", "7 x 7: 49 taps", _p(_set_k, 7), UNSUPPORTED), ("head", "17 x 17 kernel", _p(_set_k, 17), INVALID),
    ("pair", "cout_a 64", _arg("cout_a", 64), UNSUPPORTED), ("pair", "cout_b 192", _arg("cout_b", 192), UNSUPPORTED),
    ("pair", "out_dtype f32", _field("out_dtype", F32), UNSUPPORTED), ("pair", "residual", _field("res_mode", 1), UNSUPPORTED),
    ("pair", "row segments", _both(_field("row_seg_counts", A[12]), _field("row_seg_rows", 64)), UNSUPPORTED),
    ("pair", "7 x 7: 49 taps", _p(_set_k, 7), INVALID), ("pair", "misaligned out_b", _arg("out_b", A[6] + OFF), INVALID),
    ("pair", "null bias_b", _arg("bias_b", None), INVALID),
    ("levels", "null level output", _lv(0, "out", None), INVALID), ("levels", "out_dtype f32", _field("out_dtype", F32), UNSUPPORTED),
    ("levels", "no weight at all", _arg("weight", None), INVALID), ("levels", "1 x 1 over 64 channels: one K slice", _both(_p(_set_k, 1)), UNSUPPORTED),
    ("head_levels", "cout 512", _field("cout", 512), UNSUPPORTED), ("head_levels", "1 x 1 over 128 channels: fewer than eight K slices", _both(_p(_set_k, 1), _p(_set_cin, 128)), UNSUPPORTED),
    ("head_levels", "null level ctr", _lv(0, "ctr", None), INVALID), ("head_levels", "null w_tail", _arg("w_tail", None), INVALID),
    ("chain", "cout3 256", _arg("cout3", 256), UNSUPPORTED), ("chain", "cout 256", _field("cout", 256), UNSUPPORTED),
    ("chain", "out_dtype f32", _field("out_dtype", F32), UNSUPPORTED), ("chain", "misaligned mid_out", _arg("mid_out", A[7] + OFF), INVALID),
    ("chain", "null residual", _arg("residual", None), INVALID), ("chain", "7 x 7: 49 taps", _p(_set_k, 7), UNSUPPORTED),
    ("chain", "17 x 17 kernel", _p(_set_k, 17), INVALID), ("chain", "misaligned w3", _arg("w3", A[3] + OFF), INVALID),
    # two things wrong: the first check in the entry point's order decides
    ("head", "cin 96 and ho off by one", _both(_p(_set_cin, 96), _bump_ho), UNSUPPORTED),
    ("head", "misaligned hidden_out and f32 storage", _both(_arg("hidden_out", A[7] + OFF), _p(_storage, F32)), INVALID),
    ("pair", "cout_a 64 and misaligned input", _both(_arg("cout_a", 64), _arg("inp", A[0] + OFF)), UNSUPPORTED),
    ("pair", "misaligned input and 2 GiB input", _both(_arg("inp", A[0] + OFF), _field("in_stride_n", 1 << 30)), INVALID),
    ("chain", "cout3 256 and misaligned input", _both(_arg("cout3", 256), _arg("inp", A[0] + OFF)), UNSUPPORTED),
    ("chain", "null out and f32 storage", _both(_arg("out", None), _p(_storage, F32)), INVALID),
    ("levels", "7 levels and stride 2", _both(_arg("nlevels", 7), _field("stride_h", 2)), INVALID),
    ("levels", "f32 storage and misaligned shared weight", _both(_p(_storage, F32), _arg("weight", A[1] + OFF)), UNSUPPORTED),
    ("head_levels", "cout 512 and 0 levels", _both(_field("cout", 512), _arg("nlevels", 0)), UNSUPPORTED),
    ("fwd", "cin 48 and misaligned input", _both(_p(_set_cin, 48), _arg("inp", A[0] + OFF)), UNSUPPORTED),
]


def test_the_table_covers_every_entry_point_and_status():
    assert {c[0] for c in CASES} == set(ENTRIES)
    for e in ENTRIES:
        assert {c[3] for c in CASES if c[0] == e} == {INVALID, UNSUPPORTED}, e
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}".replace(" ", "_"))
def test_status_and_message(osr, case):
    entry, what, mutate, want = case
    call = ENTRIES[entry](osr)
    mutate(call)
    st, msg = call.run()
    print(f"{call.fn}: {what}: status {st}: {msg}")
    assert st == want, f"{call.fn} with {what}: status {st} ({msg}), expected {want}"
    assert msg.startswith(call.prefix), f"{call.fn} with {what}: message '{msg}' does not name {call.prefix}"
