"""The edge-case tables of tests/kernel_edge_cases.py, checked without a GPU:

  * branch proof -- the host-only size functions of the built library (and the constants of the sources) say that every
    case reaches the branch its id names; retuning OG_NORM_CHUNK, OG_IN_FUSED_MAX, OG_SM_PER, MM_RMAX, og_stream_grid,
    attn_bwd_chunks, the ROI_* limits of the ordered ROIAlign backward or LIFT_MAXE fails here instead of silently moving a
    GPU case off its branch;
  * reference sanity -- for every tensor of every case the fp32 oracle agrees with the fp64 reference to better than
    1e-3 in the maximum metric (a worse case is badly conditioned) and stays within the rel_l2 bound its family asserts;
  * the explicit first-arg-max masked_max reference equals autograd's on data without non-zero ties;
  * plumbing -- the body of the GPU test runs on the CPU definitions of the ops API (tests/cpu_ops_shim.py).
"""
import os
import re

import pytest
import torch

import cpu_ops_shim
import kernel_edge_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "obj-gan_amd", "csrc")
ALL = K.all_cases()


def _lib():
    from objgan_hip import _lib
    return _lib.load()


def _cdiv(a, b):
    return (a + b - 1) // b


def _define(fname, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, open(os.path.join(CSRC, fname)).read(), re.M)
    assert m, "%s: no #define %s" % (fname, name)
    return int(m.group(1))


def test_the_constants_the_tables_rely_on_are_those_of_the_sources():
    assert _define("norm.hip", "OG_NORM_CHUNK") == K.NORM_CHUNK
    assert _define("norm.hip", "OG_IN_FUSED_MAX") == K.IN_FUSED_MAX
    assert 64 * _define("attention.hip", "OG_SM_PER") == K.SM_ROWS_MAX
    assert _define("attention.hip", "MM_RMAX") == K.MM_RMAX
    m = re.search(r"og_stream_grid\(long work_items, int block\)\s*\{.*?if \(g > (\d+) \* (\d+)\) g = \1 \* \2;",
                  open(os.path.join(CSRC, "common.h")).read(), re.S)
    assert m, "og_stream_grid: cap not found"
    assert int(m.group(1)) * int(m.group(2)) * 256 == K.STREAM_ITEMS
    for name in ("ROI_MAX_SAMPLES", "ROI_TAB_MAX", "ROI_LDS_SMP", "ROI_LDS_G", "ROI_LDS_START", "ROI_SEQ", "ROI_SUB"):
        assert _define("roi_align.hip", name) == getattr(K, name), name
    assert _define("lift_stem.hip", "LIFT_MAXE") == K.LIFT_MAXE
    m = re.search(r"const int cpb = channels >= (\d+) \? (\d+) : (\d+);", open(os.path.join(CSRC, "roi_align.hip")).read())
    assert m, "roi_align.hip: the cpb rule of the ordered backward was not found"
    lo, big, small = (int(v) for v in m.groups())
    assert [K.roi_cpb(c) for c in (1, lo - 1, lo, lo + 1)] == [small, small, big, big]
    # (the host guard of ops._lift_axis_tables against LIFT_MAXE: test_lift_tables_* below)


def test_every_branch_of_the_issue_is_named_by_a_case():
    ids = " ".join(K.case_ids(ALL) + K.case_ids([("attn_general", c) for c in K.ATTN_GENERAL_REJECTED] +
                                                [("masked_max", c) for c in K.MASKED_MAX_REJECTED] +
                                                [("roi", c) for c in K.ROI_REJECTED] +
                                                [("lift_taps", c) for c in K.LIFT_TAPS_REJECTED]))
    for word in ("2splits", "3splits", "in-generic-2splits", "unfused", "fused-at-limit", "hw8196", "hw8192", "mode-none-residual",
                 "eval-plane", "eval-generic", "data-b", "data-c0", "data-c8", "count1", "count2",
                 "idf32-L1", "idf64-L16", "Q1", "Q63", "Q257", "chunks2", "chunks8", "L17-rejected", "idf40-rejected",
                 "mask5d-per-channel", "R16-P257", "R1-P1", "R17-rejected", "nonzero-ties",
                 "rows-dim1-", "rows-dim64-", "rows-dim65-", "rows-dim289-", "rows-dim1024-", "strided-fallback-dim1025", "outer5",
                 "lens-0-1-dim-dim+3", "rows-dim65-rowvalid", "strided-inner11-rowvalid",
                 "R1-L1", "raw-scores", "zero-label-vector", "K0", "K16", "M64-N65", "stride0", "n20000", "n1-",
                 "avgpool2s1-6x6-backward", "max-k2-s2", "max-k3-s1", "avg-k3-s2-p1", "nan-and-minus-inf",
                 "downscale", "to-1x1", "IH1", "sum2x2-3x3", "reflect_fold-3x3", "max_len8-Lout-above-L",
                 "adam-n600001", "ema-n600001", "max-k3-s2-second-grid-stride-trip", "second-grid-stride-trip-400-to-750",
                 "bn-generic-apply-second-grid-stride-trip", "strided-second-grid-stride-trip",
                 "roi:unstaged-n_e-above-1024", "roi:staged-n_e-exactly-1024", "roi:unstaged-n_e-1040",
                 "unstaged-gradient-slab-C68-last-slab-nc4-staged", "unstaged-many-taps", "start-in-lds-at-limit-hw4607",
                 "start-global-hw4608", "C70-cpb8-last-slab-nc6", "C63-cpb1", "roi:C64", "images-0-and-1-own-no-roi",
                 "rois-interleaved-2-0-1-2-0", "unstaged-rois-interleaved-1-0-1-0", "AH2xAW7", "AH7xAW2", "AH2xAW2", "S256-16x16", "H2xW2-smallest-map",
                 "last-row-and-column-exact", "every-sample-outside", "scatter-fallback-513-rois",
                 "scatter-fallback-hw9216-lds", "table-path-320-rois-second-compaction-pass",
                 "17x16-S272-rejected", "AH1-rejected", "roi_cols4-rejected", "map-1x8-rejected", "map-8x1-rejected",
                 "lift_taps:rows-3-to-8-longest-8", "cols-4-to-11-longest-8", "h1-rows-1-to-4-longest-8", "identity-5-to-5",
                 "downscale-9x12-to-4x5", "S2-smallest", "lift_taps:second-grid-stride-trip",
                 "lift_stem:3x3-to-8-C7-Mo5", "lift_stem:5x9-to-12-C3-Mo2", "lift_stem:1x3-to-4",
                 "rows-3-to-9-longest-9-rejected", "rows-1-to-5-longest-10-rejected", "S1-rejected"):
        assert word in ids, word
    assert len(set(K.case_ids(ALL))) == len(ALL), "duplicate case ids"


@pytest.mark.parametrize("case", K.NORM_CASES, ids=[c["id"] for c in K.NORM_CASES])
def test_norm_case_takes_the_branch_it_names(case):
    lib = _lib()
    N, C, H, W = case["shape"]
    HW, pc = H * W, int(case["pc"])
    G = C if pc else N * C
    ws = lib.objgan_norm_ws_floats(N, C, HW, pc)
    assert ws % (2 * G) == 0
    P = ws // (2 * G) - 1                                   # partial slots per group
    sup = lib.objgan_norm_amax_supported(N, C, HW, pc, int(case["affine"]))
    assert P == case["P"], (P, case["P"])
    assert (sup == 2) == case["fused"], sup
    assert (sup != 0) == case["plane"], sup                 # (every plane case here is fused or has P > 1)
    assert case["plane"] == (HW % 4 == 0 and HW >= 256)
    cid = case["id"]
    if "boundary-inside-plane" in cid:
        assert _cdiv(N * HW, P) % HW != 0                   # a split ends in the middle of a plane
    if "one-float4" in cid:
        assert HW % K.NORM_CHUNK == 4 and P == (N if pc else 1) * _cdiv(HW, K.NORM_CHUNK)
    if "at-limit" in cid:
        assert HW == K.IN_FUSED_MAX and lib.objgan_norm_amax_supported(N, C, HW + 4, 0, 0) == 1
    if "unfused" in cid:
        assert HW > K.IN_FUSED_MAX and not pc
    if "generic" in cid and "splits" in cid:
        assert not case["plane"] and P > 1 and (pc or HW > 1024)
    if "second-grid-stride-trip" in cid:
        assert not case["plane"] and K.work_items("norm", case) > K.STREAM_ITEMS


@pytest.mark.parametrize("case", K.NORM_EVAL_CASES, ids=[c["id"] for c in K.NORM_EVAL_CASES])
def test_norm_eval_case_takes_the_path_it_names(case):
    N, C, H, W = case["shape"]
    assert (_lib().objgan_norm_amax_supported(N, C, H * W, 1, 1) != 0) == case["plane"]
    assert case["plane"] == ((H * W) % 4 == 0 and H * W >= 256)


@pytest.mark.parametrize("case", K.ATTN_GENERAL_CASES, ids=[c["id"] for c in K.ATTN_GENERAL_CASES])
def test_attn_general_case_runs_the_wave_count_it_names(case):
    B, idf, Q, L, chunks = case["B"], case["idf"], case["ih"] * case["iw"], case["L"], case["chunks"]
    ws = _lib().objgan_attn_general_backward_ws_floats(B, idf, Q, L)
    assert ws % (B * idf * 16 * 4) == 0
    blocks = ws // (B * idf * 16 * 4)                       # workgroups of four waves per sample
    assert blocks == _cdiv(Q, 256 * chunks), (blocks, chunks)
    if chunks > 1:
        assert [c for c in range(1, 9) if _cdiv(Q, 256 * c) == blocks] == [chunks]
        assert Q % 64 != 0 and _cdiv(Q, 64) % chunks != 0   # the last wave stops inside its walk, on a ragged chunk
    if "Q257" in case["id"]:
        assert blocks == 2
    assert idf in (32, 48, 64) and 1 <= L <= 16


@pytest.mark.parametrize("case", K.MASKED_MAX_CASES, ids=[c["id"] for c in K.MASKED_MAX_CASES])
def test_masked_max_case_fills_the_workgroups_it_names(case):
    B, num, R, P = case["B"], case["num"], case["R"], case["ih"] * case["iw"]
    ws = _lib().objgan_masked_max_backward_ws_floats(B, num, R, P)
    assert ws == B * _cdiv(P, 256) * num * R
    assert R <= K.MM_RMAX and (P != 257 or ws == B * 2 * num * R)
    assert all(c["R"] == K.MM_RMAX + 1 for c in K.MASKED_MAX_REJECTED)


def test_streaming_cases_need_a_second_trip_and_softmax_cases_sit_on_their_kernel():
    n = 0
    for fam, case in ALL:
        if "second-grid-stride-trip" in case["id"]:
            n += 1
            items = K.work_items(fam, case)
            assert K.STREAM_ITEMS < items < 1.2 * K.STREAM_ITEMS, (case["id"], items)
    assert n == 7
    for case in K.SOFTMAX_CASES:
        inner = 1
        for s in case["shape"][case["dim"] + 1:]:
            inner *= s
        assert case["rows"] == (inner == 1 and case["shape"][case["dim"]] <= K.SM_ROWS_MAX), case["id"]
        if case["lens"] is not None:
            assert len(case["lens"]) < K.work_items("softmax", case) // inner


def _roi_ws(case):
    return _lib().objgan_roi_align_backward_ws_floats(case["B"], len(K.roi_inputs(case)[1]), case["C"], case["H"], case["W"],
                                                      case["AH"], case["AW"])


@pytest.mark.parametrize("case", K.ROI_CASES, ids=[c["id"] for c in K.ROI_CASES])
def test_roi_case_takes_the_branches_it_names(case):
    """roi_align_bwd_gather_kernel's decisions, restated from the geometry of the reference definition: per image and
    slab `staged`, per map `st_lds`, per pixel `total > ROI_SEQ`; and the entry point's choice of the scatter."""
    cid, S, HW = case["id"], case["AH"] * case["AW"], case["H"] * case["W"]
    feat, rois, gtop = K.roi_inputs(case)
    assert case["H"] >= 2 and case["W"] >= 2 and 2 <= case["AH"] and 2 <= case["AW"] and S <= K.ROI_MAX_SAMPLES
    assert rois.shape[1] == 5 and bool(torch.isfinite(rois).all())
    assert bool((rois[:, 0] == rois[:, 0].round()).all()) and 0 <= float(rois[:, 0].min()) and float(rois[:, 0].max()) < case["B"]
    ws = _roi_ws(case)
    assert (ws > 0) == case["table"], ws
    assert ("scatter-fallback" in cid) == (not case["table"])
    if not case["table"]:
        table_lds = 2 * HW * 4 + len(rois) * S * 2 + (K.ROI_TAB_MAX + 4 + 2 * 256) * 4    # roi_tap_table_kernel: dynamic + static
        assert (len(rois) > K.ROI_TAB_MAX and table_lds <= 64 * 1024) if "513" in cid else \
            (len(rois) <= K.ROI_TAB_MAX and table_lds > 64 * 1024 and "lds" in cid)           # one reason each
        return
    assert len(rois) <= K.ROI_TAB_MAX
    facts, slabs = K.roi_facts(case), K.roi_slabs(case)
    staged = [[K.roi_slab_is_staged(case, f, nc) for nc in slabs] for f in facts if f["nlist"]]
    flat = [v for row in staged for v in row]
    if case["staged"] == "all":
        assert all(flat)
    elif case["staged"] == "none":
        assert not any(flat)
    else:                                                   # only the short last slab fits
        assert all(row[-1] and not any(row[:-1]) for row in staged) and slabs[-1] < slabs[0]
    assert ("unstaged" in cid) == (case["staged"] != "all")
    assert case["start_lds"] == (HW + 1 <= K.ROI_LDS_START)
    n_seq, n_many = sum(f["n_seq"] for f in facts), sum(f["n_many"] for f in facts)
    assert case["taps"] == ("both" if n_seq and n_many else "many" if n_many else "seq"), (n_seq, n_many)
    assert case["at_seq"] == any(f["n_at_seq"] for f in facts)
    n_e = [f["n_e"] for f in facts]
    if "n_e-above-1024" in cid or "n_e-1040" in cid or "many-taps" in cid:
        assert n_e[0] == len(rois) * S > K.ROI_LDS_SMP and len(rois) * slabs[0] * S <= K.ROI_LDS_G     # the samples alone decide
    if "n_e-exactly-1024" in cid:
        assert n_e[0] == K.ROI_LDS_SMP
    if "gradient-slab" in cid:
        assert n_e[0] <= K.ROI_LDS_SMP and slabs[-1] == 4 and len(rois) * 8 * S > K.ROI_LDS_G >= len(rois) * 4 * S
    if "hw4607" in cid:
        assert HW + 1 == K.ROI_LDS_START
    if "hw4608" in cid:
        assert HW + 1 == K.ROI_LDS_START + 1
    if "hw460" in cid or "last-row-and-column" in cid:      # a valid sample in the last row and the last column
        geo = K.roi_geometry_np(rois.numpy(), case["H"], case["W"], case["AH"], case["AW"], case["scale"])
        last = geo["valid"] & (geo["hstart"] == case["H"] - 2) & (geo["h_ratio"] >= 1) & (geo["wstart"] == case["W"] - 2) & (geo["w_ratio"] >= 1)
        assert bool(last.any())
        if "exact" in cid:
            assert bool((last & (geo["h_ratio"] == 1) & (geo["w_ratio"] == 1)).any())
            assert bool((geo["valid"] & (geo["off"] == 0) & (geo["h_ratio"] == 0) & (geo["w_ratio"] == 0)).any())
            assert bool((~geo["valid"][3]).any()) and bool(geo["valid"][3].any())          # the box from -2
            assert len(set(geo["wstart"][4].tolist())) == 1                                 # width clamped to 0
    if "last-slab-nc6" in cid:
        assert slabs[-1] == 6 < slabs[0] == 8
    if "cpb1" in cid:
        assert set(slabs) == {1} and case["C"] == 63
    if cid == "C64":
        assert set(slabs) == {8}
    if "own-no-roi" in cid:
        assert [f["nlist"] for f in facts] == [0, 0, 5]
    if "interleaved-2-0-1-2-0" in cid:
        assert rois[:, 0].tolist() == [2, 0, 1, 2, 0]
    if "unstaged-rois-interleaved" in cid:                  # in both images a roi's list position differs from its index
        assert all(f["n_e"] > K.ROI_LDS_SMP for f in facts) and rois[:4, 0].tolist() == [1, 0, 1, 0]
    if "S256" in cid:
        assert S == K.ROI_MAX_SAMPLES
    if "H2xW2" in cid:
        assert all(0 < f["n_e"] < f["nlist"] * S for f in facts)
    if "every-sample-outside" in cid:
        assert facts[1]["nlist"] == 3 and facts[1]["n_e"] == 0 and facts[0]["n_e"] > 0
        assert float(K.reference("roi", case)["dfeat"][1].abs().sum()) == 0.0
    if "second-compaction-pass" in cid:
        assert len(rois) > 256 and len(set(rois[256:, 0].tolist())) == case["B"]


def test_roi_cases_sit_on_both_sides_of_every_decision():
    t = [c for c in K.ROI_CASES if c["table"]]
    assert {c["staged"] for c in t} == {"all", "none", "last"}
    assert {c["start_lds"] for c in t} == {True, False} and {c["taps"] for c in t} == {"seq", "both", "many"}
    assert {c["table"] for c in K.ROI_CASES} == {True, False}
    for staged in ("all", "none"):                          # both summation regimes, and a pixel with exactly ROI_SEQ
        assert any(c["taps"] == "both" and c["at_seq"] for c in t if c["staged"] == staged), staged      # taps, on both forms of the tap
    short = [K.roi_slabs(c)[-1] < K.roi_cpb(c["C"]) for c in t]
    assert any(short) and not all(short)


@pytest.mark.parametrize("fam,case", [(f, c) for f, c in ALL if f in ("lift_taps", "lift_stem")] +
                         [("lift_taps", c) for c in K.LIFT_TAPS_REJECTED],
                         ids=lambda v: v["id"] if isinstance(v, dict) else v)
def test_lift_tables_have_the_longest_row_the_case_names(fam, case):
    from objgan_hip import ops
    for n_in, n_out, longest in ((case["h"], case["SH"], case["longest"][0]), (case["w"], case["SW"], case["longest"][1])):
        if longest > K.LIFT_MAXE:
            with pytest.raises(_error()):
                ops._lift_axis_tables(n_in, n_out, "cpu")
            continue
        off = ops._lift_axis_tables(n_in, n_out, "cpu")[3]
        rows = off[:, 1:] - off[:, :-1]
        assert int(rows.max()) == longest, (n_in, n_out, int(rows.max()))
        if "downscale" in case["id"]:
            assert int(rows.min()) == 0                     # source indices no lifted position reads
        if "identity" in case["id"]:
            assert float(ops._lift_axis_tables(n_in, n_out, "cpu")[2].abs().max()) == 0.0
    if "longest-8" in case["id"]:
        assert max(case["longest"]) == K.LIFT_MAXE
    if "second-grid-stride-trip" in case["id"]:
        assert all(n > K.STREAM_ITEMS for n in K.lift_launch_items(case))
    if case["id"] == "S1-rejected":
        assert case["SH"] < 2 and max(case["longest"]) <= K.LIFT_MAXE     # refused by the C entry point (SH < 2), not by the tables


@pytest.mark.parametrize("case", [c for c in K.ROI_CASES if c["table"]], ids=[c["id"] for c in K.ROI_CASES if c["table"]])
def test_roi_backward_path_check_runs_on_the_cpu_definitions(case):
    from oracle import roi as oroi
    seen = []

    def scatter(gtop, rois, case):
        shape = (case["B"], case["C"], case["H"], case["W"])
        return torch.from_numpy(oroi.backward(gtop.numpy(), rois.numpy(), shape, case["scale"]))

    assert K.check_roi_backward_paths(_CpuOps(case), torch.device("cpu"), case, scatter, lambda k, v: seen.append(k)) is not None
    assert len(seen) == 2 and all("scatter" in k for k in seen)


@pytest.mark.parametrize("fam,case", ALL, ids=K.case_ids(ALL))
def test_fp32_oracle_agrees_with_the_fp64_reference(fam, case):
    ref, o32 = K.reference(fam, case), K.oracle32(fam, case)
    assert set(ref) == set(o32) and ref
    for name in ref:
        assert ref[name].dtype == torch.float64, name
        e_o = K.max_err(o32[name], ref[name])
        assert e_o == e_o and e_o < 1e-3, (name, e_o)              # finite, and the case is well conditioned
        bound = K.rl2_bound(fam, case, name)
        assert K.rel_l2(o32[name], ref[name]) <= bound, (name, K.rel_l2(o32[name], ref[name]), bound)


@pytest.mark.parametrize("case", [c for c in K.MASKED_MAX_CASES if not c["tie"]],
                         ids=[c["id"] for c in K.MASKED_MAX_CASES if not c["tie"]])
def test_explicit_masked_max_reference_equals_autograd_without_ties(case):
    f, m, go = K.masked_max_inputs(case)
    f, m, go = f.double(), m.double(), go.double()
    B, num, R, P = case["B"], case["num"], case["R"], case["ih"] * case["iw"]
    fa = f.clone().requires_grad_()
    m4 = m.reshape(B, 1, R, P) if m.dim() == 4 else m.reshape(B, R, num, P).permute(0, 2, 1, 3)
    out_a = (fa.reshape(B, num, R, 1) * m4).max(dim=2)[0].reshape(go.shape)
    (out_a * go).sum().backward()
    fe = f.clone().requires_grad_()
    out_e = K.REF.masked_max(fe, m, case["ih"], case["iw"])
    (out_e * go).sum().backward()
    assert torch.equal(out_e, out_a)
    assert torch.allclose(fe.grad, fa.grad, rtol=1e-12, atol=1e-14)


def test_explicit_masked_max_reference_gives_ties_to_the_first_slot():
    case = [c for c in K.MASKED_MAX_CASES if c["tie"]][0]
    f, m, go = K.masked_max_inputs(case)
    assert torch.equal(f[:, :, 1], f[:, :, 3]) and bool((f[:, :, 1] > 0).any()) and bool((f[:, :, 1] < 0).any())
    prod = f.reshape(case["B"], case["num"], case["R"], 1, 1) * m.unsqueeze(1)
    best = prod.max(dim=2)[0]
    rect = (slice(None), slice(None)) + K.TIE_RECT
    tied = (prod[:, :, 1] == best) & (prod[:, :, 3] == best) & (best != 0)
    assert int(tied[rect].sum()) > 50                       # non-zero ties that ARE the maximum
    ref = K.reference("masked_max", case)
    assert float(ref["df"][:, :, 3].abs().sum()) == 0.0 and float(ref["df"][:, :, 1].abs().sum()) > 0.0


class _CpuOps(object):
    """tests/cpu_ops_shim.py where its contract covers the case, the fp32 definitions of kernel_edge_cases elsewhere.
    Which of the two is decided by the CASE: the shim has no sum2x2 / reflect_fold, its masked_max takes 4-D masks
    with autograd's tie rule, its norm_act is torch's (no group of one value), and its LSTM expects valid token ids and
    lengths (the kernel's clamps are applied in front of it).  The sizes the library rejects raise its error here too,
    by the limits the C entry points state."""

    def __init__(self, case):
        self.case = case

    def __getattr__(self, name):
        return getattr(cpu_ops_shim, name) if hasattr(cpu_ops_shim, name) else getattr(K.REF, name)

    def norm_act(self, x, *args):
        return (K.REF if "count1" in self.case["id"] else cpu_ops_shim).norm_act(x, *args)

    def masked_max(self, f, m, ih, iw):
        if f.shape[2] > K.MM_RMAX:
            raise _error()("masked_max: R > MM_RMAX")
        shim = self.case["mask"] == "shared" and not self.case["tie"]
        return (cpu_ops_shim if shim else K.REF).masked_max(f, m, ih, iw)

    def attn_general(self, x, src, mask=None):
        if x.shape[1] not in (32, 48, 64) or src.shape[2] > 16:
            raise _error()("attn_general: no kernel for this idf / L")
        return cpu_ops_shim.attn_general(x, src, mask)

    @staticmethod
    def roi_align(features, rois, ah, aw, scale):
        if (rois.dim() != 2 or rois.shape[1] != 5 or ah * aw > K.ROI_MAX_SAMPLES or ah < 2 or aw < 2
                or features.shape[2] < 2 or features.shape[3] < 2):
            raise _error()("roi_align: BAD_ARGS")
        return cpu_ops_shim.roi_align(features, rois, ah, aw, scale)

    class _LiftTapsFn(object):
        @staticmethod
        def apply(z, bias, SH, SW):
            from objgan_hip import ops
            if SH < 2 or SW < 2:
                raise _error()("lift_taps: BAD_ARGS")
            ops._lift_axis_tables(z.shape[2], SH, "cpu")            # (the host guard: raises beyond LIFT_MAXE)
            ops._lift_axis_tables(z.shape[3], SW, "cpu")
            return cpu_ops_shim._LiftTapsFn.apply(z, bias, SH, SW)

    @staticmethod
    def lstm_bidir_forward(table, captions, lens, wt_ih, wt_hh, b_ih, b_hh, max_len):
        return cpu_ops_shim.lstm_bidir_forward(table, captions.clamp(0, table.shape[0] - 1), lens.clamp(0, captions.shape[1]),
                                               wt_ih, wt_hh, b_ih, b_hh, max_len)


def _error():
    from objgan_hip import _lib
    return _lib.ObjganHipError


@pytest.mark.parametrize("fam,case", ALL, ids=K.case_ids(ALL))
def test_gpu_test_body_runs_on_the_cpu_definitions(fam, case):
    seen = []
    worst = K.check_case(_CpuOps(case), torch.device("cpu"), fam, case, note=lambda k, v: seen.append((k, v)))
    assert worst is not None                                # (compare() has asserted every bound by now)
    assert len(seen) == len(K.reference(fam, case)) + 1


class _Accepting(object):
    """an operator that takes whatever size it is given (the plain definitions have no value for a 1 x 8 map, four roi
    columns or S = 1)"""

    @staticmethod
    def roi_align(features, rois, ah, aw, scale):
        return features.sum() * torch.ones(rois.shape[0], features.shape[1], ah, aw)

    class _LiftTapsFn(object):
        @staticmethod
        def apply(z, bias, SH, SW):
            return z.sum() * torch.ones(z.shape[0], z.shape[1] // 9, SH, SW)


REJECTED = ([("attn_general", c) for c in K.ATTN_GENERAL_REJECTED] + [("masked_max", c) for c in K.MASKED_MAX_REJECTED] +
            [("roi", c) for c in K.ROI_REJECTED] + [("lift_taps", c) for c in K.LIFT_TAPS_REJECTED])


@pytest.mark.parametrize("fam,case", REJECTED, ids=K.case_ids(REJECTED))
def test_rejection_body_runs_on_the_cpu_definitions(fam, case):
    K.check_rejected(_CpuOps(case), torch.device("cpu"), (fam, case), _error())
    with pytest.raises(AssertionError):             # ... and notices an operator that accepts the size
        K.check_rejected(_Accepting if fam in ("roi", "lift_taps") else K.REF, torch.device("cpu"), (fam, case), _error())
