"""Convolution cases that reach the launch plans the small shapes of tests/test_kernels_gpu.py never do -- tall forward
tiles, the second ("rest") launch, 8-wave workgroups, two pixel groups per wave, the multi-part weight gradient -- with
their fp64 references, shared by tests/test_conv_plans_cpu.py and tests/test_conv_plans_gpu.py (no GPU import here).

Which kernel instance a convolution runs is decided on the host (igemm2_plan / og_row_plan in csrc/conv_igemm.hip and
csrc/conv_igemm_host.h, og_wgrad_plan in csrc/conv_igemm_wgrad.hip) from the size of the grid.  A case is a conv2d geometry
with an `id` that names the plan features it is there for and the plan (PLANS below) the library states for each of its
launches under each arithmetic; the CPU file proves every stated plan with the host-only plan queries of the built
library, the GPU file checks that the arguments of the run are the proven ones and compares y, dx, dw (db) with float64.

`launches(case, arith, q)` restates the host side of objgan_hip.ops (_conv_fwd, _conv_dgrad, _conv_wgrad, the phased
up-convolution): the argument tuples of the size queries ops makes during one forward + backward, in call order.

Metric, as tests/kernel_edge_cases.py: e = max |a - ref64| / max |ref64| per tensor, e_kernel <= M * max(e_oracle32, 2^-23),
and rel_l2 < 1e-4 against fp64 (the bound of test_conv2d_forward_backward).
"""
import zlib

import torch

from kernel_edge_cases import EPS32, max_err, rel_l2
from oracle import torch_ref as tr

RL2 = 1e-4
ARITHS = ("fp32", "bf16x3", "fp16x2", "fp16x2-rec")
MODE = {"fp32": 0, "bf16x3": 2, "fp16x2": 4, "fp16x2-rec": 4}
_ACT = {None: 0, "none": 0, "lrelu": 1, "tanh": 2, "sigmoid": 3, "relu": 4}

IGEMM_Q, PHASES_Q, WGRAD_Q = "objgan_conv_igemm_ws_floats", "objgan_conv_dgrad_s2_phases_ws_floats", "objgan_conv_wgrad_ws_floats"
IGEMM_FIELDS = ("cls", "kmath", "nw", "ng", "TM", "full_rows", "rest", "tiles_n", "splits", "full_cover", "direct")
WGRAD_HEAD = ("rc", "kmath", "v2", "bfb", "rec", "rec2", "dyp", "h2", "xrows", "nparts")
WGRAD_PART = ("tm", "rows", "cfg", "m_begin", "m_end", "xr_count", "nw", "use3", "b128", "tiles_n", "splits")


def out_size(L, k, s, p):
    return (L + 2 * p - k) // s + 1


# =====================================================================================================================
# the host side of ops.conv2d, restated: which size queries one forward + backward makes
# =====================================================================================================================
def _igemm(q, mode, rec, N, C, H, W, upsample, pad_mode, Cout, Cin, Torig, transpose, Tg, PH, PW, stride, OHf, OWf, osh, osw,
           act, y_prezeroed=0, ring=0):
    """ops._igemm with the fp16x2 FLOP threshold at zero: the arithmetic the call asks for, then its size query"""
    M = Cin if transpose else Cout
    math = mode
    if math == 4 and (q("objgan_conv_bank_layout", N, C, H, W, M, Tg, PH, PW, act, math) & 255) != 5:
        math = 2                                    # thin / first-generation kernels: no fp16x2 form
    kmath = 5 if (math == 4 and rec) else math
    return (IGEMM_Q, N, C, H, W, int(upsample), int(pad_mode), Cout, Cin, Torig, int(transpose), Tg, PH, PW, stride, OHf, OWf,
            osh, osw, act, int(y_prezeroed), kmath, ring)


def _phases(mode, rec, N, Cout, OH, OW, Cin, LH, LW):
    """ops._dgrad_s2_phases, k = 4: (size query, arguments of the plan query)"""
    return (PHASES_Q, N, Cout, OH, OW, mode), (N, Cout, OH, OW, Cin, 4, LH // 2, LW // 2, 5 if (mode == 4 and rec) else mode)


def _fwd(q, mode, rec, N, Cin, H, W, Cout, k, stride, pad, refl, upsample, act):
    LH, LW = (2 * H, 2 * W) if upsample else (H, W)
    OH, OW = out_size(LH, k, stride, pad), out_size(LW, k, stride, pad)
    return _igemm(q, mode, rec, N, Cin, H, W, upsample, refl, Cout, Cin, k * k, 0, k * k, OH, OW, stride, OH, OW, 1, 1, _ACT[act])


def _dgrad(q, mode, rec, N, Cin, H, W, Cout, k, stride, pad, refl, upsample):
    """-> list of launches, each ("igemm", query tuple) or ("phases", query tuple, plan arguments)"""
    LH, LW = (2 * H, 2 * W) if upsample else (H, W)
    OH, OW = out_size(LH, k, stride, pad), out_size(LW, k, stride, pad)
    if stride == 1:
        TH, TW = (LH + 2 * pad, LW + 2 * pad) if refl else (LH, LW)
        ring = (refl and pad == 1 and LH >= 3 and LW >= 3 and
                (q("objgan_conv_bank_layout", N, Cout, OH, OW, Cin, k * k, TH, TW, 0, mode) & 255) in (1, 3, 4, 5))
        if ring:
            return [("igemm", _igemm(q, mode, rec, N, Cout, OH, OW, 0, 0, Cout, Cin, k * k, 1, k * k, TH, TW, 1, LH, LW, 1, 1, 0,
                                     ring=1))]
        return [("igemm", _igemm(q, mode, rec, N, Cout, OH, OW, 0, 0, Cout, Cin, k * k, 1, k * k, TH, TW, 1, TH, TW, 1, 1, 0))]
    assert stride == 2 and not refl
    assert not (k == 4 and pad == 1 and Cin <= 12), "the thin four-phase VALU kernel is not a case of this table"
    if k % 2 == 0 and LH % 2 == 0 and LW % 2 == 0 and Cin > 32:
        assert k == 4                               # (2 x 2 taps per phase whatever the padding)
        return [("phases",) + _phases(mode, rec, N, Cout, OH, OW, Cin, LH, LW)]
    out = []
    for ph in range(2):
        khs = [kh for kh in range(k) if (ph + pad - kh) % 2 == 0]
        PHg = (LH - ph + 1) // 2
        for pw in range(2):
            kws = [kw for kw in range(k) if (pw + pad - kw) % 2 == 0]
            PWg = (LW - pw + 1) // 2
            if PHg <= 0 or PWg <= 0:
                continue
            Tg = max(1, len(khs) * len(kws))
            out.append(("igemm", _igemm(q, mode, rec, N, Cout, OH, OW, 0, 0, Cout, Cin, k * k, 1, Tg, PHg, PWg, 1, LH, LW, 2, 2, 0,
                                        y_prezeroed=1)))
    return out


def _wgrad(q, mode, rec, N, Cin, H, W, Cout, OH, OW, k, stride, pad, refl, upsample):
    """ops._conv_wgrad with _REC["wgrad"] = "all" (records wherever the geometry allows) and the in-loop split of dy"""
    math = mode
    if mode == 4 and rec and q("objgan_conv_wgrad_rec_ok", N, Cin, H, W, Cout, OH, OW, k):
        math = 5
    return (WGRAD_Q, N, Cin, H, W, int(upsample), int(refl), Cout, OH, OW, k, stride, pad, math)


def up_phased(case):
    """ops._up_phased_ok: the up-convolution runs as the transposed 4x4 stride-2 form"""
    N, Cin, H, W, Cout, k, stride, pad, pad_mode, upsample, bias, act = case["geo"]
    return bool(upsample and stride == 1 and pad == 1 and pad_mode != "reflect" and not bias and act is None and k == 3
                and Cout > 32 and Cin > 32 and H >= 2 and W >= 2)


def launches(case, arith, q):
    """{"fwd": launch, "wgrad": query tuple, "dgrad": [launches]} of one forward + backward of the case under `arith`;
    q(name, *ints) answers the library's host-only queries (objgan_hip.ops._q on either machine)."""
    N, Cin, H, W, Cout, k, stride, pad, pad_mode, upsample, bias, act = case["geo"]
    mode, rec = MODE[arith], arith == "fp16x2-rec"
    refl = 1 if pad_mode == "reflect" else 0
    if up_phased(case):
        # y = the data gradient of the virtual 4x4 stride-2 convolution [N, Cout, 2H, 2W] -> [N, Cin, H, W]; dx its
        # forward, dw its weight gradient (ops._UpConv3x3Fn)
        return {"fwd": ("phases",) + _phases(mode, rec, N, Cin, H, W, Cout, 2 * H, 2 * W),
                "dgrad": [("igemm", _fwd(q, mode, rec, N, Cout, 2 * H, 2 * W, Cin, 4, 2, 1, 0, False, None))],
                "wgrad": _wgrad(q, mode, rec, N, Cout, 2 * H, 2 * W, Cin, H, W, 4, 2, 1, 0, False)}
    LH, LW = (2 * H, 2 * W) if upsample else (H, W)
    OH, OW = out_size(LH, k, stride, pad), out_size(LW, k, stride, pad)
    return {"fwd": ("igemm", _fwd(q, mode, rec, N, Cin, H, W, Cout, k, stride, pad, refl, upsample, act)),
            "dgrad": _dgrad(q, mode, rec, N, Cin, H, W, Cout, k, stride, pad, refl, upsample),
            "wgrad": _wgrad(q, mode, rec, N, Cin, H, W, Cout, OH, OW, k, stride, pad, refl, upsample)}


def expected_queries(case, arith, q):
    """the size queries ops makes during the call, in call order: forward; backward: weight gradient, then data
    gradient (the phased up-convolution asks for its data gradient first)"""
    L = launches(case, arith, q)
    back = [L["wgrad"]] + [d[1] for d in L["dgrad"]]
    return [L["fwd"][1]] + (back[1:] + back[:1] if up_phased(case) else back)


def launch_kind(launch):
    """"phases" (one four-phase launch), "ring" (reflect data gradient on the padded grid), "cover" (every output
    element written by the launch) or "partial" (one output parity phase into a pre-zeroed tensor)"""
    if launch[0] == "phases":
        return "phases"
    a = launch[1]
    if a[-1]:
        return "ring"
    return "cover" if (a[17], a[18], a[12], a[13]) == (1, 1, a[15], a[16]) else "partial"


def igemm_plan(lib, launch):
    """the 11 IGEMM_FIELDS the library plans for a forward / data-gradient launch of `launches`"""
    import ctypes
    out = (ctypes.c_int * 11)()
    if launch[0] == "phases":
        rc = lib.objgan_conv_dgrad_s2_phases_plan(*(launch[2] + (out,)))
    else:
        rc = lib.objgan_conv_igemm_plan(*(launch[1][1:] + (out,)))
    assert rc == 1, (rc, launch)
    return tuple(out)


def wgrad_plan(lib, query):
    """(the 10 WGRAD_HEAD fields, [the 11 WGRAD_PART fields of every part]) of a weight-gradient query of `launches`"""
    import ctypes
    out = (ctypes.c_int * 43)()
    rc = lib.objgan_conv_wgrad_plan(*(query[1:] + (out,)))
    assert rc == 1, (rc, query)
    v = tuple(out)
    return v[:10], [v[10 + 11 * i:21 + 11 * i] for i in range(v[9])]


def plans_of(lib, case, arith, q):
    """{"fwd": (kind, fields), "dgrad": [(kind, fields)], "wgrad": (head, [parts])} as PLANS states them"""
    L = launches(case, arith, q)
    return {"fwd": (launch_kind(L["fwd"]), igemm_plan(lib, L["fwd"])),
            "dgrad": [(launch_kind(d), igemm_plan(lib, d)) for d in L["dgrad"]],
            "wgrad": wgrad_plan(lib, L["wgrad"])}


# =====================================================================================================================
# cases: N, Cin, H, W, Cout, k, stride, pad, pad_mode, upsample, bias, act -- the smallest shapes that reach each plan
# =====================================================================================================================
_Z, _R = "zeros", "reflect"


def _case(cid, *geo):
    assert len(geo) == 12
    return dict(id=cid, geo=geo)


CASES = [
    # ---- forward launch, stride 1, full cover: (Cout, N * OH * OW) decide the block rows
    _case("fwd-tm2-cout33-last-group-1-row", 1, 16, 256, 256, 33, 1, 1, 0, _Z, False, False, None),
    _case("fwd-tm3-cout65-last-group-1-row-3x3", 6, 16, 64, 64, 65, 3, 1, 1, _Z, False, False, None),
    _case("fwd-tm4-cout97", 1, 16, 256, 256, 97, 1, 1, 0, _Z, False, False, None),
    _case("fwd-tm5-cout129-reflect-3x3", 2, 16, 128, 128, 129, 3, 1, 1, _R, False, False, None),
    _case("fwd-tm6-cout161", 1, 16, 256, 256, 161, 1, 1, 0, _Z, False, False, None),
    _case("fwd-tm7x2-cout417", 1, 16, 128, 128, 417, 1, 1, 0, _Z, False, False, None),
    _case("fwd-tm3x4-rest1-cout388+wgrad-xrows-b128-frag+wgrad-nw8-b128-tm7-tm6+wgrad-rec-two-parts-nw8",
          1, 16, 128, 128, 388, 3, 1, 1, _Z, False, False, None),
    _case("fwd-tm2x4-rest1-cout257", 6, 16, 64, 64, 257, 1, 1, 0, _Z, False, False, None),
    _case("fwd-tm5-rest4-cout257-bias-lrelu+fwd-nw8-rest", 1, 16, 256, 256, 257, 1, 1, 0, _Z, False, True, "lrelu"),
    _case("fwd-tm7-rest6-cout385-last-group-1-row-3x3+fwd-nw8-rest", 1, 16, 256, 256, 385, 3, 1, 1, _Z, False, False, None),
    _case("fwd-tm7-cout194-last-group-2-rows+wgrad-xrows-b128-frag+wgrad-rec-two-parts-nw8",
          1, 16, 256, 256, 194, 1, 1, 0, _Z, False, False, None),
    _case("fwd-nw8-tm4-cout97", 2, 16, 256, 256, 97, 1, 1, 0, _Z, False, False, None),
    _case("fwd-nw8-tm7-cout193", 2, 16, 256, 256, 193, 1, 1, 0, _Z, False, False, None),
    _case("fwd-s2-4x4-tm5-cout160-lrelu+wgrad-s2-4x4", 4, 16, 256, 256, 160, 4, 2, 1, _Z, False, False, "lrelu"),
    # ---- data gradient, ring mode (reflect 3x3: M = Cin rows over the padded grid)
    _case("ring-tm3-cin65", 6, 65, 64, 64, 16, 3, 1, 1, _R, False, False, None),
    _case("ring-rest-cin385+ring-nw8-rest", 4, 385, 128, 128, 16, 3, 1, 1, _R, False, False, None),
    _case("ring-rec-ng2-tm1-cin65", 8, 65, 128, 128, 16, 3, 1, 1, _R, False, False, None),
    _case("ring-rec-ng2-tm2-rest-cin321", 3, 321, 128, 128, 16, 3, 1, 1, _R, False, False, None),
    # ---- data gradient, the four-phase 4x4 stride-2 launch (Cin > 32, even sizes)
    _case("ph4-tm3-rest-cin385", 1, 385, 128, 128, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-tm5-cin129", 2, 129, 128, 128, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-tm6-cin161", 4, 161, 128, 128, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-tm7x2-cin417", 1, 417, 128, 128, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-nw8-tm4-cin97", 2, 97, 256, 256, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-rec-ng2-tm1-cin257", 2, 257, 128, 128, 16, 4, 2, 1, _Z, False, False, None),
    _case("ph4-rec-ng2-tm3-cin65", 4, 65, 256, 256, 16, 4, 2, 1, _Z, False, False, None),
    # ---- data gradient, one partial-cover launch per output parity phase (stride-2 3x3 on odd sizes)
    _case("perphase-s2-3x3-odd-sizes-tm3-cin65", 6, 65, 127, 129, 16, 3, 2, 1, _Z, False, False, None),
    # ---- the phased up-convolution: its forward is a four-phase launch
    _case("up-phased-fwd-tm3-cout65", 1, 48, 64, 96, 65, 3, 1, 1, _Z, True, False, None),
    # ---- weight gradient (og_wgrad_plan)
    _case("wgrad-xrows-b128-frag-1x1-cout130-cin32+wgrad-nw8-tm5-1x1", 1, 32, 128, 128, 130, 1, 1, 0, _Z, False, False, None),
    _case("wgrad-xrows-lds-upsample-cout260+wgrad-rec-upsample-nw8", 1, 16, 64, 64, 260, 3, 1, 1, _Z, True, False, None),
    _case("wgrad-two-parts-both-split-cout388+wgrad-rec-two-parts-nw4", 1, 16, 64, 64, 388, 3, 1, 1, _Z, False, False, None),
]
BY_ID = {c["id"]: c for c in CASES}


def fields(plan):
    return dict(zip(IGEMM_FIELDS, plan))


def _f(pred):
    """a row about the forward launch: stride 1, full cover, on the MFMA implicit-GEMM kernel"""
    return lambda c, p: (p["fwd"][0] == "cover" and c["geo"][6] == 1 and fields(p["fwd"][1])["cls"] not in (0, 2)
                         and pred(c, fields(p["fwd"][1])))


def _d(kind, pred, count=1):
    return lambda c, p: (len(p["dgrad"]) == count and all(k == kind and pred(c, fields(f)) for k, f in p["dgrad"]))


def _w(pred):
    return lambda c, p: p["wgrad"][0][0] == 1 and pred(c, dict(zip(WGRAD_HEAD, p["wgrad"][0])),
                                                        [dict(zip(WGRAD_PART, q)) for q in p["wgrad"][1]])


A3, A4, SPLIT3, REC = ARITHS[:3], ARITHS, ARITHS[1:], ARITHS[3:]
X3H2 = ARITHS[1:3]
# (row, word of the case id, arithmetics that must each reach it, predicate on (case, stated plan))
COVERAGE = (
    [("forward main launch at TM %d" % t, "fwd-tm%d" % t, A3, _f(lambda c, f, t=t: f["TM"] == t and f["nw"] == 4)) for t in range(2, 8)] + [
        ("forward rest launch of one row group", "rest1", A3, _f(lambda c, f: f["rest"] == 1 and f["TM"] >= 2)),
        ("forward rest launch of >= 4 row groups, 5 + 4", "fwd-tm5-rest4", A3, _f(lambda c, f: (f["TM"], f["rest"]) == (5, 4))),
        ("forward rest launch of >= 4 row groups, 7 + 6", "fwd-tm7-rest6", A3, _f(lambda c, f: (f["TM"], f["rest"]) == (7, 6))),
        ("last row group with one valid row", "last-group-1-row", A3, _f(lambda c, f: c["geo"][4] % 32 == 1 and f["TM"] >= 2)),
        ("last row group with one valid row, in the rest launch", "rest6-cout385-last-group-1-row", A3,
         _f(lambda c, f: c["geo"][4] % 32 == 1 and f["rest"] >= 2)),
        ("last row group with two valid rows", "last-group-2-rows", A3, _f(lambda c, f: c["geo"][4] % 32 == 2 and f["TM"] >= 2)),
        ("forward 8-wave workgroups at TM 4", "fwd-nw8-tm4", SPLIT3, _f(lambda c, f: (f["nw"], f["TM"], f["rest"]) == (8, 4, 0))),
        ("forward 8-wave workgroups at TM 7", "fwd-nw8-tm7", SPLIT3, _f(lambda c, f: (f["nw"], f["TM"], f["rest"]) == (8, 7, 0))),
        ("forward 8-wave workgroups with a rest launch", "fwd-nw8-rest", SPLIT3, _f(lambda c, f: f["nw"] == 8 and f["rest"] > 0)),
        ("bias + lrelu on TM >= 2 with a rest launch", "bias-lrelu", A4,
         _f(lambda c, f: c["geo"][10] and c["geo"][11] == "lrelu" and f["TM"] >= 2 and f["rest"] > 0 and f["splits"] == 1)),
        ("stride-2 4x4 forward at TM >= 2", "fwd-s2-4x4", A4,
         lambda c, p: c["geo"][5:8] == (4, 2, 1) and p["fwd"][0] == "cover" and fields(p["fwd"][1])["TM"] >= 2),
        ("ring data gradient at TM >= 2", "ring-tm", A4, _d("ring", lambda c, f: f["TM"] >= 2)),
        ("ring data gradient with a rest launch", "ring-rest", A4, _d("ring", lambda c, f: f["rest"] > 0)),
        ("ring data gradient, 8 waves with a rest launch", "ring-nw8-rest", SPLIT3, _d("ring", lambda c, f: f["nw"] == 8 and f["rest"] > 0)),
        ("ring data gradient, records ng 2 at TM 1", "ring-rec-ng2-tm1", REC, _d("ring", lambda c, f: (f["ng"], f["TM"]) == (2, 1))),
        ("ring data gradient, records ng 2 at TM 2 with rest", "ring-rec-ng2-tm2-rest", REC,
         _d("ring", lambda c, f: (f["ng"], f["TM"]) == (2, 2) and f["rest"] > 0))] + [
        ("four-phase data gradient at TM %d" % t, "ph4-tm%d" % t, A3, _d("phases", lambda c, f, t=t: f["TM"] == t and f["ng"] == 1))
        for t in (3, 5, 6, 7)] + [
        ("four-phase data gradient with a rest launch", "ph4-tm3-rest", A4, _d("phases", lambda c, f: f["rest"] > 0)),
        ("four-phase data gradient, 8 waves", "ph4-nw8", SPLIT3, _d("phases", lambda c, f: f["nw"] == 8)),
        ("four-phase data gradient, records ng 2 at TM 1", "ph4-rec-ng2-tm1", REC, _d("phases", lambda c, f: (f["ng"], f["TM"]) == (2, 1))),
        ("four-phase data gradient, records ng 2 at TM 3", "ph4-rec-ng2-tm3", REC, _d("phases", lambda c, f: (f["ng"], f["TM"]) == (2, 3))),
        ("per-phase partial-cover data gradient at TM >= 2", "perphase", A4,
         _d("partial", lambda c, f: f["TM"] >= 2 and f["full_cover"] == 0 and f["splits"] == 1, count=4)),
        ("phased up-convolution: four-phase forward at TM >= 2", "up-phased", A4,
         lambda c, p: p["fwd"][0] == "phases" and fields(p["fwd"][1])["TM"] >= 2),
        ("fp32 weight gradient: extra rows + b128 + register fragments, 3x3", "wgrad-xrows-b128-frag", A3[:1],
         _w(lambda c, h, q: c["geo"][5] == 3 and h["xrows"] and q[0]["xr_count"] > 0 and q[0]["b128"] and q[0]["use3"] and q[0]["tm"] >= 2)),
        ("fp32 weight gradient: extra rows + b128 + register fragments, 1x1", "wgrad-xrows-b128-frag-1x1", A3[:1],
         _w(lambda c, h, q: c["geo"][5] == 1 and h["xrows"] and q[0]["xr_count"] > 0 and q[0]["b128"] and q[0]["use3"] and q[0]["tm"] >= 2)),
        ("fp32 weight gradient: extra rows on the LDS form (upsample)", "wgrad-xrows-lds-upsample", A3[:1],
         _w(lambda c, h, q: c["geo"][9] and h["xrows"] and q[0]["xr_count"] > 0 and not q[0]["use3"] and not q[0]["b128"])),
        ("split arithmetics: two parts, both split (second slot offset > 0)", "wgrad-two-parts-both-split", X3H2,
         _w(lambda c, h, q: h["nparts"] == 2 and q[0]["splits"] > 1 and q[1]["splits"] > 1 and not h["rec"])),
        ("split arithmetics: 8 waves with b128 at tm 7 + 6", "wgrad-nw8-b128-tm7-tm6", X3H2,
         _w(lambda c, h, q: [(p["tm"], p["nw"], p["b128"], p["use3"]) for p in q] == [(7, 8, 1, 1), (6, 8, 1, 1)])),
        ("split arithmetics: 8 waves at tm 5, 1x1", "wgrad-nw8-tm5-1x1", X3H2,
         _w(lambda c, h, q: c["geo"][5] == 1 and [(p["tm"], p["nw"]) for p in q] == [(5, 8)])),
        ("records: two parts on 4 waves", "wgrad-rec-two-parts-nw4", REC,
         _w(lambda c, h, q: h["rec"] and [p["nw"] for p in q] == [4, 4] and all(p["splits"] > 1 for p in q))),
        ("records: two parts on 8 waves", "wgrad-rec-two-parts-nw8", REC,
         _w(lambda c, h, q: h["rec"] and [p["nw"] for p in q] == [8, 8] and all(p["splits"] > 1 for p in q))),
        ("records: the upsample form on 8 waves", "wgrad-rec-upsample-nw8", REC,
         _w(lambda c, h, q: h["rec"] and c["geo"][9] and all(p["nw"] == 8 for p in q))),
        ("stride-2 4x4 weight gradient", "wgrad-s2-4x4", A4,
         _w(lambda c, h, q: c["geo"][5:8] == (4, 2, 1) and h["v2"] and q[0]["tm"] >= 2)),
    ])


def implied_igemm_ws(query, plan):
    """floats objgan_conv_igemm_ws_floats must return for a launch with this plan (fp32 / split arithmetics: no operand
    copy): one slot of the output (+ ring) per split"""
    f = fields(plan)
    if f["cls"] in (0, 2) or f["splits"] <= 1 or not f["full_cover"]:
        return 0
    N, Cout, Cin, transpose, PH, PW, OHf, OWf, ring = (query[1], query[7], query[8], query[10], query[12], query[13], query[15],
                                                       query[16], query[22])
    M = Cin if transpose else Cout
    return (N * M * OHf * OWf + (N * M * (2 * PW + 2 * PH) if ring else 0)) * f["splits"]


def implied_wgrad_ws(query, plan):
    """floats objgan_conv_wgrad_ws_floats must return (maths 0 / 2 / 4 / 5: no operand copy): every split part takes
    `splits` slots of (rows + extra rows) x Cin k^2 floats, the parts one behind the other"""
    Cin, k = query[2], query[10]
    return sum((q["m_end"] - q["m_begin"] + q["xr_count"]) * Cin * k * k * q["splits"]
               for q in (dict(zip(WGRAD_PART, p)) for p in plan[1]) if q["splits"] > 1)


# =====================================================================================================================
# inputs, runner, references
# =====================================================================================================================
def inputs(case):
    """seeded fp32 inputs of a geometry: x ~ N(0, 1), w ~ N(0, 1) / sqrt(Cin k^2), bias, gy ~ N(0, 1)"""
    N, Cin, H, W, Cout, k, stride, pad, pad_mode, upsample, bias, act = case["geo"]
    g = torch.Generator().manual_seed(zlib.crc32(repr(case["geo"]).encode()) & 0x7FFFFFFF)
    LH, LW = (2 * H, 2 * W) if upsample else (H, W)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / float(Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) if bias else None
    gy = torch.randn(N, Cout, out_size(LH, k, stride, pad), out_size(LW, k, stride, pad), generator=g)
    return x, w, b, gy


def run_conv(ns, case, dtype, device):
    """one ns.conv2d forward + backward -> ({"y", "dx", "dw"[, "db"]}, the output tensor object)"""
    stride, pad, pad_mode, upsample, _, act = case["geo"][6:]
    x, w, b, gy = (None if t is None else t.to(device=device, dtype=dtype) for t in inputs(case))
    x.requires_grad_()
    w.requires_grad_()
    if b is not None:
        b.requires_grad_()
    y = ns.conv2d(x, w, b, stride, pad, pad_mode, upsample, act)
    assert tuple(y.shape) == tuple(gy.shape), (tuple(y.shape), tuple(gy.shape))
    y.backward(gy)
    got = {"y": y.detach(), "dx": x.grad, "dw": w.grad}
    if b is not None:
        got["db"] = b.grad
    return got, y


_CACHE = {}


def _cached(kind, case, dtype):
    """The tests walk the table case by case (all arithmetics of a case one after the other), so only the references of
    the geometry in hand are kept: a few hundred megabytes at most, never the whole table's."""
    key = (kind, case["geo"])
    if key not in _CACHE:
        for other in [k for k in _CACHE if k[1] != case["geo"]]:
            del _CACHE[other]
        got, _ = run_conv(tr, case, dtype, torch.device("cpu"))
        _CACHE[key] = {k: v.detach().clone() for k, v in got.items()}
    return _CACHE[key]


def release():
    """drop the cached references (the test modules call this when they are done: nothing stays behind in the session)"""
    _CACHE.clear()


def reference(case):
    """float64 reference (oracle.torch_ref.conv2d on the CPU), computed once per geometry and never modified"""
    return _cached("ref64", case, torch.float64)


def oracle32(case):
    return _cached("oracle32", case, torch.float32)


# =====================================================================================================================
# metric and bounds
# =====================================================================================================================
# One constant per (tensor, arithmetic).  Rule (tests/kernel_edge_cases.py): the largest e_k / max(e_o, 2^-23) seen on
# the MI355X over all cases (the `plan-max` lines of the parity log conftest.note() writes), times 4 (the summation
# order differs from shape to shape, and one seed is one sample), rounded up to a power of two.  Beside each value: the
# observed maximum and its case.  No constant is below 4 -- the rule applied to a ratio of 1: under a smaller one the
# bound would follow the ORACLE's error (db: torch's fp32 channel sum of 65 536 terms is 67 times worse than the ordered
# sum of objgan_channel_sum, ratio 0.015), which changes with the oracle's thread count, not with the kernel.
M = {
    ("y", "fp32"): 16.0,            # 2.86   ring-rec-ng2-tm2-rest-cin321 (direct TM 1 instance, 3 splits of K = 2889)
    ("y", "bf16x3"): 16.0,          # 2.34   ring-rec-ng2-tm2-rest-cin321
    ("y", "fp16x2"): 16.0,          # 2.10   ring-rec-ng2-tm2-rest-cin321
    ("y", "fp16x2-rec"): 16.0,      # 2.10   ring-rec-ng2-tm2-rest-cin321
    ("dx", "fp32"): 16.0,           # 2.16   wgrad-xrows-b128-frag-1x1-cout130-cin32+wgrad-nw8-tm5-1x1
    ("dx", "bf16x3"): 8.0,          # 1.74   ph4-rec-ng2-tm3-cin65
    ("dx", "fp16x2"): 8.0,          # 1.20   fwd-tm3x4-rest1-cout388+...
    ("dx", "fp16x2-rec"): 8.0,      # 1.20   fwd-tm3x4-rest1-cout388+...
    ("dw", "fp32"): 4.0,            # 0.986  fwd-tm2x4-rest1-cout257
    ("dw", "bf16x3"): 8.0,          # 1.03   fwd-tm2x4-rest1-cout257
    ("dw", "fp16x2"): 4.0,          # 0.934  fwd-nw8-tm4-cout97
    ("dw", "fp16x2-rec"): 4.0,      # 0.934  fwd-nw8-tm4-cout97
    ("db", "fp32"): 4.0, ("db", "bf16x3"): 4.0, ("db", "fp16x2"): 4.0, ("db", "fp16x2-rec"): 4.0,     # 0.0149 (see above)
}
# A tensor the thin VALU kernels write (bank layout class 2: at most 32 output rows on 65 536 pixels or more -- the
# forward of the 16-output data-gradient cases, the data gradient of the 16-input forward cases) has a bound of its own,
# as running_var has in tests/kernel_edge_cases.py, so that the MFMA launches this table is about keep theirs.  Those
# kernels add their K products one after the other in fp32 in every arithmetic: 3465 terms where the ratio peaks.
M_THIN = {"y": 32.0,                # 7.90   ring-rest-cin385+ring-nw8-rest (K = 385 * 9)
          "dx": 32.0}               # 7.03   fwd-tm7-rest6-cout385-last-group-1-row-3x3+fwd-nw8-rest (K = 385 * 9)


def written_by_thin(case, arith, name):
    p = PLANS[case["id"]][arith]
    return (name == "y" and p["fwd"][1][0] == 2) or (name == "dx" and any(f[0] == 2 for _, f in p["dgrad"]))


def m_bound(case, arith, name):
    return M_THIN[name] if written_by_thin(case, arith, name) else M[(name, arith)]


def where_worst(name, a, ref):
    """the element with the largest error: its index, its 32-row group and its 128-pixel tile -- which launch wrote it"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    flat = int((a - ref).abs().reshape(-1).argmax())
    idx = []
    for s in reversed(a.shape):
        idx.append(flat % s)
        flat //= s
    idx = tuple(reversed(idx))
    if a.dim() != 4:
        return "worst at %s (row group %d)" % (idx, idx[0] // 32)
    if name == "dw":
        return "worst at (co, ci, kh, kw) = %s: row group %d, column %d" % (idx, idx[0] // 32, (idx[1] * a.shape[2] + idx[2]) * a.shape[3] + idx[3])
    pixel = (idx[0] * a.shape[2] + idx[2]) * a.shape[3] + idx[3]
    return "worst at (n, c, h, w) = %s: row group %d, pixel %d = 128-pixel tile %d" % (idx, idx[1] // 32, pixel, pixel // 128)


def compare(case, arith, got, note=None):
    """e_k <= M * max(e_o, 2^-23) and rel_l2 < 1e-4 against fp64, for every tensor of the case; every figure is noted
    before anything is asserted.  Returns {tensor: e_k / max(e_o, 2^-23)}."""
    ref, o32 = reference(case), oracle32(case)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    bad, ratios = [], {}
    for name in sorted(ref):
        e_k, e_o = max_err(got[name], ref[name]), max_err(o32[name], ref[name])
        ratios[name] = e_k / max(e_o, EPS32)
        r2 = rel_l2(got[name], ref[name])
        if note is not None:
            note("plan %s %s %s" % (arith, case["id"][:60], name), "e_k %.3g e_o %.3g ratio %.3g rel_l2 %.3g" % (e_k, e_o, ratios[name], r2))
            note("plan-max %s %s%s" % (name, arith, " thin" if written_by_thin(case, arith, name) else ""),
                 "ratio %.3g %s" % (ratios[name], case["id"][:60]))
        mb = m_bound(case, arith, name)
        if not (e_k <= mb * max(e_o, EPS32)):
            bad.append("%s: e_k %.3g > %g * max(e_o %.3g, 2^-23); %s" % (name, e_k, mb, e_o, where_worst(name, got[name], ref[name])))
        if not (r2 < RL2):
            bad.append("%s: rel_l2 %.3g >= %g; %s" % (name, r2, RL2, where_worst(name, got[name], ref[name])))
    assert not bad, "%s [%s]  %s" % (case["id"], arith, "; ".join(bad))
    return ratios


def exact_properties(got, y):
    """what must hold as an equality: no NaN / infinity in y, dx, dw; where ops attached partial maxima to y (the
    LeakyReLU epilogue under fp16x2), the maximum of the slots is max |y| bit for bit"""
    for name in ("y", "dx", "dw"):
        assert bool(torch.isfinite(got[name]).all()), "%s holds a NaN or an infinity" % name
    am = getattr(y, "_og_absmax", None)
    if am is not None:
        for _, slots in am.values():
            assert float(slots.max()) == float(got["y"].abs().max()), "the partial maxima of y are not max |y|"
    return am is not None


def check_case(ns, device, case, arith, note=None):
    """The body of one test: run ns.conv2d forward + backward on `device` in float32, compare y, dx, dw (db) with the
    float64 reference, then the exact properties.  -> ({tensor: ratio}, whether y carried partial maxima)"""
    got, y = run_conv(ns, case, torch.float32, device)
    if device.type == "cuda":
        torch.cuda.synchronize()
    failed = None
    try:
        ratios = compare(case, arith, got, note)
    except AssertionError as e:             # (every figure is noted by now; the exact properties are still looked at)
        failed, ratios = e, None
    had_max = exact_properties(got, y)
    if failed is not None:
        raise failed
    return ratios, had_max


# =====================================================================================================================
# The plan of every launch of every case under every arithmetic, as the plan queries of the library state it
# (tests/test_conv_plans_cpu.py compares each entry with the built library: a retuned planner fails there, and the
# coverage rows above are then checked against the new table).  "fwd" / "dgrad": (kind, IGEMM_FIELDS); "wgrad":
# (WGRAD_HEAD, [WGRAD_PART per part]).  A launch on the thin VALU kernels (class 2) has no plan: zeros behind the class.
# =====================================================================================================================
PLANS = {
    'fwd-tm2-cout33-last-group-1-row': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 2, 1, 0, 512, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 33, 0, 4, 1, 1, 1, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 2, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 33, 0, 4, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 2, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(2, 1, 0, 0, 33, 0, 4, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 2, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 33, 0, 8, 1, 1, 1, 128)])},
    },
    'fwd-tm3-cout65-last-group-1-row-3x3': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 3, 1, 0, 192, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 192, 5, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(2, 1, 0, 0, 64, 1, 4, 1, 1, 2, 48)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 3, 1, 0, 192, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 192, 5, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(3, 1, 0, 0, 65, 0, 4, 1, 1, 2, 48)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 3, 1, 0, 192, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 192, 5, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(3, 1, 0, 0, 65, 0, 4, 1, 1, 2, 48)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 3, 1, 0, 192, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 192, 5, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(3, 1, 0, 0, 65, 0, 8, 1, 1, 2, 48)])},
    },
    'fwd-tm4-cout97': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 4, 1, 0, 512, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(3, 1, 0, 0, 96, 1, 4, 1, 1, 1, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 4, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 4, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 4, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 128)])},
    },
    'fwd-tm5-cout129-reflect-3x3': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 5, 1, 0, 256, 1, 1, 0)),
                 'dgrad': [('ring', (1, 0, 4, 1, 1, 1, 0, 265, 4, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(4, 1, 0, 0, 128, 1, 4, 1, 1, 2, 64)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 5, 1, 0, 256, 1, 1, 0)),
                   'dgrad': [('ring', (4, 2, 4, 1, 1, 1, 0, 265, 4, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 129, 0, 8, 1, 1, 1, 64)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 5, 1, 0, 256, 1, 1, 0)),
                   'dgrad': [('ring', (5, 4, 4, 1, 1, 1, 0, 265, 4, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(5, 1, 0, 0, 129, 0, 8, 1, 1, 1, 64)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 5, 1, 0, 256, 1, 1, 0)),
                       'dgrad': [('ring', (5, 5, 4, 1, 1, 1, 0, 265, 4, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 129, 0, 8, 1, 1, 2, 64)])},
    },
    'fwd-tm6-cout161': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 6, 1, 0, 512, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(5, 1, 0, 0, 160, 1, 4, 1, 1, 1, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 6, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(6, 1, 0, 0, 161, 0, 8, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 6, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(6, 1, 0, 0, 161, 0, 8, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 6, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(6, 1, 0, 0, 161, 0, 8, 1, 1, 1, 128)])},
    },
    'fwd-tm7x2-cout417': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 7, 2, 0, 128, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 128, 3, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 2),
                           [(7, 1, 0, 0, 224, 1, 4, 1, 1, 1, 32), (6, 1, 0, 224, 416, 0, 4, 1, 1, 1, 32)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 7, 2, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 128, 3, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(7, 2, 0, 0, 417, 0, 8, 1, 1, 1, 32)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 7, 2, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 128, 3, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(7, 2, 0, 0, 417, 0, 8, 1, 1, 1, 32)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 7, 2, 0, 128, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 128, 3, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 2, 0, 0, 320, 0, 8, 1, 1, 1, 32), (4, 1, 0, 320, 417, 0, 8, 1, 1, 1, 32)])},
    },
    'fwd-tm3x4-rest1-cout388+wgrad-xrows-b128-frag+wgrad-nw8-b128-tm7-tm6+wgrad-rec-two-parts-nw8': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 3, 4, 1, 128, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(6, 2, 0, 0, 384, 4, 4, 1, 1, 2, 32)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 3, 4, 1, 128, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 8, 1, 1, 1, 32), (6, 1, 0, 224, 388, 0, 8, 1, 1, 1, 32)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 3, 4, 1, 128, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 8, 1, 1, 1, 32), (6, 1, 0, 224, 388, 0, 8, 1, 1, 1, 32)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 3, 4, 1, 128, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 2, 0, 0, 320, 0, 8, 1, 1, 2, 32), (3, 1, 0, 320, 388, 0, 8, 1, 1, 2, 32)])},
    },
    'fwd-tm2x4-rest1-cout257': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 2, 4, 1, 192, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 192, 2, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(4, 2, 0, 0, 256, 1, 4, 1, 1, 1, 48)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 2, 4, 1, 192, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 192, 2, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 48), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 48)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 2, 4, 1, 192, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 192, 2, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 48), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 48)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 2, 4, 1, 192, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 192, 2, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 48), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 48)])},
    },
    'fwd-tm5-rest4-cout257-bias-lrelu+fwd-nw8-rest': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 5, 1, 4, 512, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 512, 2, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(4, 2, 0, 0, 256, 1, 4, 1, 1, 1, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 8, 1, 5, 1, 4, 256, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 512, 2, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 128), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 8, 1, 5, 1, 4, 256, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 512, 2, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 128), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 8, 1, 5, 1, 4, 256, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 512, 2, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 1, 0, 0, 160, 0, 8, 1, 1, 1, 128), (4, 1, 0, 160, 257, 0, 8, 1, 1, 1, 128)])},
    },
    'fwd-tm7-rest6-cout385-last-group-1-row-3x3+fwd-nw8-rest': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 7, 1, 6, 512, 1, 1, 0)),
                 'dgrad': [('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(6, 2, 0, 0, 384, 1, 4, 1, 1, 2, 64)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 8, 1, 7, 1, 6, 256, 1, 1, 0)),
                   'dgrad': [('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 8, 1, 1, 1, 128), (6, 1, 0, 224, 385, 0, 8, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 8, 1, 7, 1, 6, 256, 1, 1, 0)),
                   'dgrad': [('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 8, 1, 1, 1, 128), (6, 1, 0, 224, 385, 0, 8, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 8, 1, 7, 1, 6, 256, 1, 1, 0)),
                       'dgrad': [('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 2, 0, 0, 320, 0, 8, 1, 1, 2, 64), (3, 1, 0, 320, 385, 0, 8, 1, 1, 2, 128)])},
    },
    'fwd-tm7-cout194-last-group-2-rows+wgrad-xrows-b128-frag+wgrad-rec-two-parts-nw8': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 7, 1, 0, 512, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(6, 1, 0, 0, 192, 2, 4, 1, 1, 1, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 7, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(7, 1, 0, 0, 194, 0, 8, 1, 1, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 7, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(7, 1, 0, 0, 194, 0, 8, 1, 1, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 7, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 512, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(4, 1, 0, 0, 128, 0, 8, 1, 1, 1, 128), (3, 1, 0, 128, 194, 0, 8, 1, 1, 1, 128)])},
    },
    'fwd-nw8-tm4-cout97': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 4, 1, 0, 1024, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(3, 1, 0, 0, 96, 1, 4, 1, 1, 1, 256)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 8, 1, 4, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 256)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 8, 1, 4, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 256)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 8, 1, 4, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(4, 1, 0, 0, 97, 0, 8, 1, 1, 1, 256)])},
    },
    'fwd-nw8-tm7-cout193': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 7, 1, 0, 1024, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(6, 1, 0, 0, 192, 1, 4, 1, 1, 1, 256)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 8, 1, 7, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(7, 1, 0, 0, 193, 0, 8, 1, 1, 1, 256)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 8, 1, 7, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(7, 1, 0, 0, 193, 0, 8, 1, 1, 1, 256)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 8, 1, 7, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 1024, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(4, 1, 0, 0, 128, 0, 8, 1, 1, 1, 256), (3, 1, 0, 128, 193, 0, 8, 1, 1, 1, 256)])},
    },
    'fwd-s2-4x4-tm5-cout160-lrelu+wgrad-s2-4x4': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 5, 1, 0, 512, 1, 1, 0)),
                 'dgrad': [('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                           ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 160, 0, 4, 0, 0, 2, 128)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 5, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                             ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 160, 0, 8, 1, 0, 1, 128)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 5, 1, 0, 512, 1, 1, 0)),
                   'dgrad': [('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                             ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(5, 1, 0, 0, 160, 0, 8, 1, 0, 1, 128)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 5, 1, 0, 512, 1, 1, 0)),
                       'dgrad': [('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                                 ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), ('partial', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 160, 0, 8, 1, 0, 2, 128)])},
    },
    'ring-tm3-cin65': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 192, 5, 1, 1)),
                 'dgrad': [('ring', (1, 0, 4, 1, 3, 1, 0, 205, 1, 1, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 48)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 192, 5, 1, 1)),
                   'dgrad': [('ring', (4, 2, 4, 1, 3, 1, 0, 205, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 48)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 192, 5, 1, 1)),
                   'dgrad': [('ring', (5, 4, 4, 1, 3, 1, 0, 205, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 48)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 192, 5, 1, 1)),
                       'dgrad': [('ring', (5, 5, 4, 1, 3, 1, 0, 205, 1, 1, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 1, 4, 48)])},
    },
    'ring-rest-cin385+ring-nw8-rest': {
        'fp32': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                 'dgrad': [('ring', (1, 0, 4, 1, 6, 2, 1, 529, 1, 1, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 28, 54)])},
        'bf16x3': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                   'dgrad': [('ring', (4, 2, 8, 1, 7, 1, 6, 265, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 28, 54)])},
        'fp16x2': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                   'dgrad': [('ring', (5, 4, 8, 1, 7, 1, 6, 265, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 28, 54)])},
        'fp16x2-rec': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                       'dgrad': [('ring', (5, 5, 8, 1, 7, 1, 6, 265, 1, 1, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 1, 15, 17)])},
    },
    'ring-rec-ng2-tm1-cin65': {
        'fp32': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                 'dgrad': [('ring', (1, 0, 4, 1, 3, 1, 0, 1057, 1, 1, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 256)])},
        'bf16x3': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                   'dgrad': [('ring', (4, 2, 4, 1, 3, 1, 0, 1057, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 256)])},
        'fp16x2': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                   'dgrad': [('ring', (5, 4, 4, 1, 3, 1, 0, 1057, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 5, 256)])},
        'fp16x2-rec': {'fwd': ('cover', (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
                       'dgrad': [('ring', (5, 5, 4, 2, 1, 3, 0, 529, 1, 1, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 1, 4, 64)])},
    },
    'ring-rec-ng2-tm2-rest-cin321': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 384, 3, 1, 1)),
                 'dgrad': [('ring', (1, 0, 4, 1, 3, 3, 2, 397, 1, 1, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 23, 66)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 384, 3, 1, 1)),
                   'dgrad': [('ring', (4, 2, 4, 1, 3, 3, 2, 397, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 23, 66)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 384, 3, 1, 1)),
                   'dgrad': [('ring', (5, 4, 4, 1, 3, 3, 2, 397, 1, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 1, 23, 66)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 384, 3, 1, 1)),
                       'dgrad': [('ring', (5, 5, 4, 2, 2, 5, 1, 199, 1, 1, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 1, 13, 19)])},
    },
    'ph4-tm3-rest-cin385': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 3, 4, 1, 32, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 49, 5)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 3, 4, 1, 32, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 49, 5)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 3, 4, 1, 32, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 49, 5)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 1, 3, 4, 1, 32, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 52, 4)])},
    },
    'ph4-tm5-cin129': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 5, 1, 0, 64, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 17, 15)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 5, 1, 0, 64, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 17, 15)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 5, 1, 0, 64, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 17, 15)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 1, 5, 1, 0, 64, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 20, 12)])},
    },
    'ph4-tm6-cin161': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 128, 8, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 6, 1, 0, 128, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 21, 12)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 128, 8, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 6, 1, 0, 128, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 21, 12)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 128, 8, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 6, 1, 0, 128, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 21, 12)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 128, 8, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 1, 6, 1, 0, 128, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 0, 12, 21)])},
    },
    'ph4-tm7x2-cin417': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 7, 2, 0, 32, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 53, 4)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 7, 2, 0, 32, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 53, 4)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 7, 2, 0, 32, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 53, 4)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 32, 16, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 1, 7, 2, 0, 32, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 56, 4)])},
    },
    'ph4-nw8-tm4-cin97': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 256, 4, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 4, 1, 0, 256, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 13, 59)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 256, 4, 1, 1)),
                   'dgrad': [('phases', (4, 2, 8, 1, 4, 1, 0, 128, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 13, 59)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 256, 4, 1, 1)),
                   'dgrad': [('phases', (5, 4, 8, 1, 4, 1, 0, 128, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 13, 59)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 256, 4, 1, 1)),
                       'dgrad': [('phases', (5, 5, 8, 1, 4, 1, 0, 128, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 0, 8, 32)])},
    },
    'ph4-rec-ng2-tm1-cin257': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 3, 3, 0, 64, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 33, 15)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 3, 3, 0, 64, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 33, 15)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 3, 3, 0, 64, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 33, 15)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 64, 8, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 2, 1, 9, 0, 32, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 36, 7)])},
    },
    'ph4-rec-ng2-tm3-cin65': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 512, 2, 1, 1)),
                 'dgrad': [('phases', (1, 0, 4, 1, 3, 1, 0, 512, 1, 0, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 9, 111)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 512, 2, 1, 1)),
                   'dgrad': [('phases', (4, 2, 4, 1, 3, 1, 0, 512, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 9, 111)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 512, 2, 1, 1)),
                   'dgrad': [('phases', (5, 4, 4, 1, 3, 1, 0, 512, 1, 0, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(1, 1, 0, 0, 16, 0, 4, 1, 0, 9, 111)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 512, 2, 1, 1)),
                       'dgrad': [('phases', (5, 5, 4, 2, 3, 1, 0, 256, 1, 0, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(1, 1, 0, 0, 16, 0, 8, 1, 0, 6, 42)])},
    },
    'perphase-s2-3x3-odd-sizes-tm3-cin65': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 1, 0, 195, 5, 1, 1)),
                 'dgrad': [('partial', (1, 0, 4, 1, 3, 1, 0, 195, 1, 0, 0)), ('partial', (1, 0, 4, 1, 3, 1, 0, 192, 1, 0, 0)),
                           ('partial', (1, 0, 4, 1, 3, 1, 0, 192, 1, 0, 0)), ('partial', (1, 0, 4, 1, 3, 1, 0, 189, 1, 0, 0))],
                 'wgrad': ((1, 0, 0, 0, 0, 0, 0, 0, 0, 1), [(0, 1, 2, 0, 16, 0, 4, 0, 0, 3, 98)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 1, 0, 195, 5, 1, 1)),
                   'dgrad': [('partial', (4, 2, 4, 1, 3, 1, 0, 195, 1, 0, 0)), ('partial', (4, 2, 4, 1, 3, 1, 0, 192, 1, 0, 0)),
                             ('partial', (4, 2, 4, 1, 3, 1, 0, 192, 1, 0, 0)), ('partial', (4, 2, 4, 1, 3, 1, 0, 189, 1, 0, 0))],
                   'wgrad': ((1, 2, 0, 0, 0, 0, 0, 0, 0, 1), [(0, 1, 2, 0, 16, 0, 4, 0, 0, 3, 98)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 1, 0, 195, 5, 1, 1)),
                   'dgrad': [('partial', (5, 4, 4, 1, 3, 1, 0, 195, 1, 0, 0)), ('partial', (5, 4, 4, 1, 3, 1, 0, 192, 1, 0, 0)),
                             ('partial', (5, 4, 4, 1, 3, 1, 0, 192, 1, 0, 0)), ('partial', (5, 4, 4, 1, 3, 1, 0, 189, 1, 0, 0))],
                   'wgrad': ((1, 2, 0, 0, 0, 0, 0, 1, 0, 1), [(0, 1, 2, 0, 16, 0, 4, 0, 0, 3, 98)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 1, 0, 195, 5, 1, 1)),
                       'dgrad': [('partial', (5, 5, 4, 1, 3, 1, 0, 195, 1, 0, 0)), ('partial', (5, 5, 4, 1, 3, 1, 0, 192, 1, 0, 0)),
                                 ('partial', (5, 5, 4, 1, 3, 1, 0, 192, 1, 0, 0)), ('partial', (5, 5, 4, 1, 3, 1, 0, 189, 1, 0, 0))],
                       'wgrad': ((1, 2, 0, 0, 0, 0, 0, 1, 0, 1), [(0, 1, 2, 0, 16, 0, 4, 0, 0, 3, 98)])},
    },
    'up-phased-fwd-tm3-cout65': {
        'fp32': {'fwd': ('phases', (1, 0, 4, 1, 3, 1, 0, 48, 1, 0, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 2, 0, 48, 6, 1, 0))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 48, 0, 4, 1, 0, 9, 12)])},
        'bf16x3': {'fwd': ('phases', (4, 2, 4, 1, 3, 1, 0, 48, 1, 0, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 2, 0, 48, 6, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 48, 0, 4, 1, 0, 9, 12)])},
        'fp16x2': {'fwd': ('phases', (5, 4, 4, 1, 3, 1, 0, 48, 1, 0, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 2, 0, 48, 6, 1, 0))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(2, 1, 0, 0, 48, 0, 4, 1, 0, 9, 12)])},
        'fp16x2-rec': {'fwd': ('phases', (5, 5, 4, 1, 3, 1, 0, 48, 1, 0, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 2, 0, 48, 6, 1, 0))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(2, 1, 0, 0, 48, 0, 4, 1, 0, 12, 12)])},
    },
    'wgrad-xrows-b128-frag-1x1-cout130-cin32+wgrad-nw8-tm5-1x1': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 5, 0, 128, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 128, 1, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(4, 1, 0, 0, 128, 2, 4, 1, 1, 1, 32)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 5, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 128, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 130, 0, 8, 1, 1, 1, 32)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 5, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 128, 1, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 1), [(5, 1, 0, 0, 130, 0, 8, 1, 1, 1, 32)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 5, 0, 128, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 128, 1, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 1), [(5, 1, 0, 0, 130, 0, 8, 1, 1, 1, 32)])},
    },
    'wgrad-xrows-lds-upsample-cout260+wgrad-rec-upsample-nw8': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 9, 0, 128, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(4, 2, 0, 0, 256, 4, 4, 0, 0, 2, 32)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 9, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 4, 0, 0, 2, 32), (4, 1, 0, 160, 260, 0, 4, 0, 0, 2, 32)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 9, 0, 128, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(5, 1, 0, 0, 160, 0, 4, 0, 0, 2, 32), (4, 1, 0, 160, 260, 0, 4, 0, 0, 2, 32)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 9, 0, 128, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 128, 8, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 1, 0, 0, 160, 0, 8, 0, 0, 2, 32), (4, 1, 0, 160, 260, 0, 8, 0, 0, 2, 32)])},
    },
    'wgrad-two-parts-both-split-cout388+wgrad-rec-two-parts-nw4': {
        'fp32': {'fwd': ('cover', (1, 0, 4, 1, 1, 13, 0, 32, 1, 1, 0)),
                 'dgrad': [('cover', (1, 0, 4, 1, 1, 1, 0, 32, 15, 1, 1))],
                 'wgrad': ((1, 0, 1, 0, 0, 0, 0, 0, 1, 1), [(6, 2, 0, 0, 384, 4, 4, 1, 1, 2, 8)])},
        'bf16x3': {'fwd': ('cover', (4, 2, 4, 1, 1, 13, 0, 32, 1, 1, 0)),
                   'dgrad': [('cover', (4, 2, 4, 1, 1, 1, 0, 32, 15, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 0, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 4, 1, 1, 2, 8), (6, 1, 0, 224, 388, 0, 4, 1, 1, 2, 8)])},
        'fp16x2': {'fwd': ('cover', (5, 4, 4, 1, 1, 13, 0, 32, 1, 1, 0)),
                   'dgrad': [('cover', (5, 4, 4, 1, 1, 1, 0, 32, 15, 1, 1))],
                   'wgrad': ((1, 2, 1, 0, 0, 0, 0, 1, 0, 2),
                             [(7, 1, 0, 0, 224, 0, 4, 1, 1, 2, 8), (6, 1, 0, 224, 388, 0, 4, 1, 1, 2, 8)])},
        'fp16x2-rec': {'fwd': ('cover', (5, 5, 4, 1, 1, 13, 0, 32, 1, 1, 0)),
                       'dgrad': [('cover', (5, 5, 4, 1, 1, 1, 0, 32, 15, 1, 1))],
                       'wgrad': ((1, 2, 1, 0, 1, 0, 0, 0, 0, 2),
                                 [(5, 2, 0, 0, 320, 0, 4, 1, 1, 3, 8), (3, 1, 0, 320, 388, 0, 4, 1, 1, 3, 8)])},
    },
}
