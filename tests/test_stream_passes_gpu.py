"""The four streaming passes of the training step, on the MI355X: the fp16 record pass (objgan_h2_records), the activation
gradient (objgan_act_backward) and the two ordered sums of split partials (splitk_combine_kernel behind objgan_conv_igemm,
wgrad_combine_kernel behind objgan_conv_wgrad).  Each moves 16 bytes per lane where pointers and sizes allow and keeps
an element-wise form for the rest; every result is required bit for bit.

    records      against a torch evaluation of the layout rec[n][c / 16][h | l][pixel][c % 16] and of the two cuts (the
                 construction of test_kernels_gpu.py::test_h2_records_layout_and_split); a guard behind the record stays
                 untouched; x at a 16-byte boundary and one float behind it
    act gradient against the torch expression of each kind, one rounding per operation; pointers at a 16-byte boundary
                 and one float behind it; the maximum of the 1 024 slots is max |dz|.  Kind 2 evaluates 1 - y * y in one
                 rounding in the kernel (a fused multiply-add, as before this file existed): its reference forms
                 1 - y * y in float64 and rounds it to fp32 once (_act_reference says why that is the same number)
    combines     the sums have no entry point of their own, so the 16-byte path and the element-wise path
                 must agree: the same split convolution / weight gradient with the output at a 16-byte boundary and
                 4 bytes behind it (16-byte loads, element stores), and with the workspace 4 bytes behind one as well
                 (the element-wise kernel).  The plan queries prove that every case splits.
"""
import contextlib
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                  # floats behind a record that must stay as they were
SENTINEL = 0x5A5A5A5A


def _ops():
    from objgan_hip import ops
    return ops


def _lib():
    from objgan_hip import _lib
    return _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _offset_copy(t, floats):
    """the values of t (flat) in fresh memory `floats` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()]
    v.copy_(t.reshape(-1))
    return v


# ---- records -------------------------------------------------------------------------------------------------------
REC_SHAPES = [(1, 1, 1), (2, 15, 25), (1, 17, 289), (2, 194, 255), (1, 16, 256), (1, 33, 257),
              (1, 20, 1000)]            # the last: four workgroups of 256 pixels (289, 257: five of 64)


def _record_reference(x):
    """(h, l) [N, Cp / 16, HW, 16] of x [N, C, HW] (cpu), as test_h2_records_layout_and_split builds them"""
    N, C, HW = x.shape
    Cp = (C + 15) // 16 * 16
    m = float(x.abs().max())
    e = math.frexp(m)[1] - 1
    sc = 2.0 ** (14 - e)
    assert 2.0 ** 14 <= m * sc < 2.0 ** 15
    xs = torch.zeros(N, Cp, HW)
    xs[:, :C] = x * sc
    h = xs.half().float()
    l = (xs - h).half().float()
    return (h.view(N, Cp // 16, 16, HW).permute(0, 1, 3, 2), l.view(N, Cp // 16, 16, HW).permute(0, 1, 3, 2))


def _check_records(dev, shape, x_offset):
    ops, lib = _ops(), _lib()
    N, C, HW = shape
    Cp = (C + 15) // 16 * 16
    x = torch.randn(N, C, HW, generator=torch.Generator().manual_seed(11 + C + HW)) * 3.7
    xd = x.to(dev)
    amax = ops._absmax(xd)                                  # (the maxima pass needs the aligned tensor: same values)
    xk = _offset_copy(xd, x_offset) if x_offset else xd
    assert xk.data_ptr() % 16 == 4 * x_offset
    nrec = lib.load().objgan_h2_records_floats(N, C, HW)
    assert nrec == N * Cp * HW
    buf = torch.full((nrec + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    lib.call("objgan_h2_records", _ptr(xk), _ptr(amax), _ptr(buf), N, C, HW, ops._stream())
    torch.cuda.synchronize()
    assert bool((buf[nrec:] == SENTINEL).all()), "the record pass wrote behind the record"
    r = buf[:nrec].view(torch.float16).view(N, Cp // 16, 2, HW, 16).float().cpu()
    want_h, want_l = _record_reference(x)
    assert torch.equal(r[:, :, 0], want_h)
    assert torch.equal(r[:, :, 1], want_l)
    if Cp > C:                                              # channels C .. Cp - 1 of the last chunk: +0 in both pieces
        pad = buf[:nrec].view(torch.int16).view(N, Cp // 16, 2, HW, 16)[:, -1, :, :, C % 16:]
        assert bool((pad == 0).all())


@pytest.mark.parametrize("shape", REC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_records_bit_for_bit(dev, shape):
    _check_records(dev, shape, 0)


@pytest.mark.parametrize("shape", [(2, 15, 25), (1, 16, 256)], ids=lambda s: "x".join(map(str, s)))
def test_records_of_x_one_float_behind_a_16_byte_boundary(dev, shape):
    _check_records(dev, shape, 1)


# ---- activation gradient -------------------------------------------------------------------------------------------
# 4 * 256 * 1024 + 3: one full trip of the 1 024 slot-owning workgroups and a tail; the last: two groups per trip for
# every thread, a third trip that holds a single group for 100 of them, and a tail
ACT_TOTALS = [1, 3, 4, 5, 1023, 1025, 4 * 256 * 1024 + 3, 2 * 4 * 256 * 1024 + 401]


def _act_reference(kind, d, o):
    one = torch.ones((), dtype=torch.float32, device=d.device)
    if kind == 1:
        return d * torch.where(o > 0, one, 0.2 * one)
    if kind == 2:
        # the kernel rounds 1 - y * y once (a contracted multiply-add, as before this file existed).  In float64 p = y * y
        # is exact (48 bits) and f = 1 - p is rounded to 53 bits; rounding f to fp32 gives the fp32 rounding of the exact
        # value (a representable float64 cannot be crossed by the first rounding) unless f was rounded AND lands exactly
        # half way between two fp32 numbers.  Fast2Sum (1 >= p) gives the error of the subtraction exactly; the draw has
        # no such element, which is checked.  (An exact f half way between two fp32 numbers is a tie in both forms.)
        p = o.double() * o.double()
        f = 1.0 - p
        err = -p - (f - 1.0)
        half_way = (f.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
        assert not bool((half_way & (err != 0)).any()), "test design: a rounded 1 - y * y half way between two fp32 numbers"
        return d * f.float()
    if kind == 3:
        return d * o * (1.0 - o)
    return torch.where(o > 0, d, torch.zeros_like(d))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-float-behind"])
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_act_backward_bit_for_bit(dev, kind, offset):
    ops, lib = _ops(), _lib()
    g = torch.Generator().manual_seed(100 + kind)
    nmax = max(ACT_TOTALS)
    d_all = torch.randn(nmax, generator=g).to(dev)
    y_all = torch.randn(nmax, generator=g)
    if kind == 2:
        y_all = torch.tanh(y_all)
    elif kind == 3:
        y_all = torch.sigmoid(y_all)
    y_all = y_all.to(dev)
    for total in ACT_TOTALS:
        d, y = _offset_copy(d_all[:total], offset), _offset_copy(y_all[:total], offset)
        for with_max in ((True, False) if total == ACT_TOTALS[-1] else (True,)):
            zbuf = torch.full((total + 8,), float("nan"), dtype=torch.float32, device=dev)
            dz = zbuf[offset:offset + total]
            amax = torch.full((1024,), float("nan"), dtype=torch.float32, device=dev) if with_max else None
            lib.call("objgan_act_backward", _ptr(d), _ptr(y), _ptr(dz), total, kind,
                     None if amax is None else _ptr(amax), ops._stream())
            torch.cuda.synchronize()
            want = _act_reference(kind, d, y)
            assert torch.equal(dz, want), (kind, total, offset)
            assert bool(torch.isnan(zbuf[:offset]).all()) and bool(torch.isnan(zbuf[offset + total:]).all())
            if amax is not None:
                assert float(amax.max()) == float(want.abs().max()), (kind, total, offset)
                assert bool((amax >= 0).all())


# ---- ordered sums of split partials --------------------------------------------------------------------------------
@pytest.fixture
def fp32_convs():
    ops = _ops()
    prev = ops.get_conv_math()
    ops.set_conv_math("fp32")
    yield ops
    ops.set_conv_math(prev)


@contextlib.contextmanager
def _workspace_shifted(floats, dev):
    """objgan_conv_igemm calls inside see their split-K workspace `floats` floats behind a 16-byte boundary (ops._igemm
    allocates it aligned); yields the list of workspace addresses modulo 16 the calls were given"""
    lib = _lib()
    orig, seen, keep = lib.call, [], []

    def call(name, *a):
        if name == "objgan_conv_igemm":
            a = list(a)
            nws = int(a[36])
            assert a[35] is not None and nws > 0, "test design: the call has no workspace"
            buf = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
            keep.append(buf)
            a[35] = ctypes.c_void_p(buf.data_ptr() + 4 * floats)
            seen.append(a[35].value % 16)
        return orig(name, *a)

    lib.call = call
    try:
        yield seen
    finally:
        lib.call = orig


# (N, Cin, H, W, Cout, k, pad, bias, act): HW of the output 289, 25, 64; 193 * 289 leaves a tail of one element
FWD_SPLIT = [(1, 768, 17, 17, 192, 1, 0, True, "relu"), (3, 384, 8, 8, 384, 4, 0, False, "none"),
             (2, 320, 8, 8, 384, 3, 1, True, "lrelu"), (1, 768, 17, 17, 193, 1, 0, True, "relu")]


def test_forward_combine_paths_agree(dev, fp32_convs):
    ops, lib = fp32_convs, _lib().load()
    split_cases = 0
    for ci, (N, Cin, H, W, Cout, k, pad, has_bias, act) in enumerate(FWD_SPLIT):
        OH, OW = H + 2 * pad - k + 1, W + 2 * pad - k + 1
        T = k * k
        plan = (ctypes.c_int * 11)()
        assert lib.objgan_conv_igemm_plan(N, Cin, H, W, 0, 0, Cout, Cin, T, 0, T, OH, OW, 1, OH, OW, 1, 1, ops._ACT[act], 0,
                                          0, 0, plan) == 1
        if plan[8] <= 1:
            continue
        split_cases += 1
        g = torch.Generator().manual_seed(40 + ci)
        x = torch.randn(N, Cin, H, W, generator=g).to(dev)
        w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.05).to(dev)
        bias = torch.randn(Cout, generator=g).to(dev) if has_bias else None
        dh = [kh - pad for kh in range(k) for kw in range(k)]
        dw = [kw - pad for kh in range(k) for kw in range(k)]
        outs, maxima = [], []
        # y at a 16-byte boundary (16-byte loads and stores), 4 bytes behind one (16-byte loads, element stores), and
        # with the workspace 4 bytes behind one as well (the element-wise kernel)
        for offset, ws_offset in ((0, 0), (1, 0), (1, 1)):
            buf = torch.full((N * Cout * OH * OW + 8,), float("nan"), dtype=torch.float32, device=dev)
            y = buf[offset:offset + N * Cout * OH * OW].view(N, Cout, OH, OW)
            assert y.data_ptr() % 16 == 4 * offset
            ym = torch.zeros(1024, dtype=torch.float32, device=dev) if act != "none" else None
            with _workspace_shifted(ws_offset, dev) as seen:
                ops._igemm(x, w, bias, y, N, Cin, H, W, 0, 0, Cout, Cin, T, 0, dh, dw, list(range(T)), OH, OW, 1, OH, OW,
                           1, 1, 0, 0, ops._ACT[act], cache=False, ymax=ym)
                torch.cuda.synchronize()
            assert seen == [4 * ws_offset], seen
            assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + y.numel():]).all())
            outs.append(y)
            maxima.append(ym)
        assert torch.equal(outs[0], outs[1]), (N, Cin, H, W, Cout, k)
        assert torch.equal(outs[0], outs[2]), (N, Cin, H, W, Cout, k)          # 16-byte form == element-wise kernel
        if maxima[0] is not None:
            assert float(maxima[0].max()) == float(maxima[1].max()) == float(maxima[2].max()) == float(outs[0].abs().max())
    if split_cases < len(FWD_SPLIT):
        pytest.fail("test design: only %d of %d forward cases split" % (split_cases, len(FWD_SPLIT)))


# (N, Cin, H, W, Cout, k, stride, pad, reflect): extra rows behind the 192 main rows (ncol = 1 746: no 16-byte rows);
# the stride-2 layer; 32 splits (the unrolled slot loop)
WGRAD_SPLIT = [(2, 194, 32, 32, 194, 3, 1, 1, 1), (4, 96, 32, 32, 192, 4, 2, 1, 0), (16, 64, 32, 32, 64, 3, 1, 1, 0)]


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
def test_wgrad_combine_paths_agree(dev, accumulate):
    ops, lib = _ops(), _lib()
    L = lib.load()
    for ci, (N, Cin, H, W, Cout, k, stride, pad, refl) in enumerate(WGRAD_SPLIT):
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        geo = (N, Cin, H, W, 0, refl, Cout, OH, OW, k, stride, pad, 0)
        plan = (ctypes.c_int * 43)()
        assert L.objgan_conv_wgrad_plan(*(geo + (plan,))) == 1
        assert plan[9] >= 1 and plan[10 + 10] > 1, "test design: the weight gradient does not split"
        if ci == 0:
            assert plan[8] == 1 and plan[10 + 5] > 0, "test design: no extra rows"
        nws = L.objgan_conv_wgrad_ws_floats(*geo)
        assert nws > 0
        g = torch.Generator().manual_seed(70 + ci)
        x = torch.randn(N, Cin, H, W, generator=g).to(dev)
        dy = torch.randn(N, Cout, OH, OW, generator=g).to(dev)
        start = torch.randn(Cout * Cin * k * k, generator=g).to(dev)
        outs = []
        for dw_off, ws_off in ((0, 0), (1, 0), (1, 1)):
            buf = torch.full((start.numel() + 8,), float("nan"), dtype=torch.float32, device=dev)
            dw = buf[dw_off:dw_off + start.numel()]
            if accumulate:
                dw.copy_(start)
            wsbuf = torch.full((nws + 8,), float("nan"), dtype=torch.float32, device=dev)
            ws = wsbuf[ws_off:ws_off + nws]
            lib.call("objgan_conv_wgrad", _ptr(x), _ptr(dy), _ptr(dw), *geo, accumulate, None, None, _ptr(ws), nws,
                     ops._stream())
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:dw_off]).all()) and bool(torch.isnan(buf[dw_off + dw.numel():]).all())
            outs.append(dw)
        assert torch.equal(outs[0], outs[1]), geo
        assert torch.equal(outs[0], outs[2]), geo
