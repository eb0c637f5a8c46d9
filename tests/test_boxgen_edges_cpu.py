"""Host-side proof for the box generator's edge cases (tests/boxgen_edge_cases.py), no GPU: which branch of
csrc/box_train.hip / csrc/box_decode.hip every case reaches, derived from its shape and the launch arithmetic restated
from the sources (the LDS formula checked against the library's own refusal); a case on either side of every decision;
the fp32 restatement of every case inside the operator bound, with the margins each case requires; the decode margin
cap; and the `dtrace` / `pad` extensions of the restatement against a finite-difference probe and the repository's own
loss classes."""
import numpy as np
import pytest
import torch

import boxgen_edge_cases as E
import boxgen_oracle as BO
import boxgen_train_oracle as TO

TRAIN = {c["id"]: c for c in E.TRAIN_CASES}
WITH_REF = [c for c in E.TRAIN_CASES if not c.get("no_reference")]


def _facts(c, cpw=None):
    return E.launch_facts(c["H"], c["L"], c["K"], c["A"], c["cpw"] if cpw is None else cpw, c["lens"], c["T"])


def test_every_case_reaches_the_branch_it_names():
    f = {k: _facts(c) for k, c in TRAIN.items()}
    # the loss kernel's `t = lane, lane + 64, ...`: second trip, and four trips at the limit with lengths on both
    # sides of a trip boundary
    assert f["T70-second-lane-trip"]["loss_trips"] == 2 and TRAIN["T70-second-lane-trip"]["lens"] == [70, 1, 65, 3, 0]
    assert f["T70-second-lane-trip"]["tiles"] == 2 and f["T70-second-lane-trip"]["tile_maxlen"] == [70, 0]
    t256 = TRAIN["T256-limit-lens-256-64-65-1"]
    assert t256["T"] == E.BT_MAX["T"] and f[t256["id"]]["loss_trips"] == 4 and sorted(t256["lens"]) == [1, 64, 65, 256]
    # cpw = 8 on two waves: four trips of the per-caption softmax loop; a partly filled second tile; zero lengths inside
    b11 = f["cpw8-B11-partial-tile-zero-lens"]
    assert (b11["waves"], b11["caption_trips"], b11["tiles"], b11["last_tile_captions"]) == (2, 4, 2, 3)
    assert b11["gate_rows_masked"] and 0 in b11["clamped"][:8] and min(b11["tile_maxlen"]) > 0
    b17 = f["cpw8-B17-last-tile-all-zero"]
    assert (b17["waves"], b17["caption_trips"], b17["tiles"]) == (1, 8, 3) and b17["tile_maxlen"][-1] == 0
    assert not b17["gate_rows_masked"] and min(b17["tile_maxlen"][:2]) > 0
    # lens outside [0, T]
    lc = TRAIN["lens-clamped"]
    assert max(lc["lens"]) > lc["T"] and min(lc["lens"]) < 0 and f["lens-clamped"]["clamped"] == [6, 0, 6, 0, 3]
    assert f["all-lens-zero-N0"]["N"] == 0 and f["all-lens-zero-N0"]["tile_maxlen"] == [0]
    # the limits
    assert TRAIN["K8-limit"]["K"] == E.BT_MAX["K"] and f["K8-limit"]["head_threads"] == 80
    assert f["L65"]["softmax_trips"] == 2 and TRAIN["L65"]["L"] - 64 == 1
    assert TRAIN["L256-limit"]["L"] == E.BT_MAX["L"] and f["L256-limit"]["softmax_trips"] == 4
    assert TRAIN["A64-limit"]["A"] == E.BT_MAX["A"] and TRAIN["A1"]["A"] == 1
    assert f["H2"]["threads"] == 64 and 4 * TRAIN["H2"]["H"] == 8
    assert f["H16-one-full-wave"]["threads"] == 64 and not f["H16-one-full-wave"]["gate_rows_masked"]
    # one-hot rows up to L - 1 are reachable: the targets of the L cases use labels of the last lane trip
    for k in ("L65", "L256-limit"):
        assert E.build_train(TRAIN[k])["labels"].max() == TRAIN[k]["L"] - 1
    # a pad label before the end of a caption, under both pad ids
    for k in ("pad-inside-caption", "pad2"):
        b = E.build_train(TRAIN[k])
        assert b["labels"][0, 3] == 0 and b["clamped"][0] == 6 and b["labels"][0, 6] == E.EOS
    assert TRAIN["pad2"]["pad"] == 2 and TRAIN["pad-inside-caption"]["pad"] == 0


def test_both_sides_of_every_decision_have_a_case():
    f = [_facts(c) for c in E.TRAIN_CASES]
    assert {x["loss_trips"] for x in f} >= {1, 2, 4}
    assert {x["softmax_trips"] for x in f} >= {1, 2, 4}
    assert {x["caption_trips"] for x in f} >= {2, 4, 8}                   # two waves, four captions ... one wave, eight
    assert _facts(TRAIN[E.CPW_INVARIANT], cpw=1)["caption_trips"] == 1    # a single trip: the invariance test's cpw 1, 2
    assert {x["gate_rows_masked"] for x in f} == {True, False}
    assert any(0 in x["tile_maxlen"] for x in f) and any(0 not in x["tile_maxlen"] and 0 in x["clamped"] for x in f)
    assert any(x["N"] == 0 for x in f) and any(x["N"] > 0 for x in f)
    assert {c["K"] for c in E.TRAIN_CASES} >= {1, 2, 8} and {c["A"] for c in E.TRAIN_CASES} >= {1, 10, 64}
    assert {c["cpw"] for c in E.TRAIN_CASES} >= {4, 8} and E.CPW_INVARIANT in TRAIN   # 1 and 2: the invariance test
    assert {c["pad"] for c in E.TRAIN_CASES} == {0, 2}
    assert sum(bool(c.get("norm_clamp")) for c in E.TRAIN_CASES) == 1
    # the clip: n below, at and above the 256 blocks; empty blocks; a short last block
    cf = {n: E.clip_facts(n) for n in E.CLIP_NS}
    assert cf[1] == {"chunk": 1, "busy_blocks": 1, "empty_blocks": 255, "last_block_short": False}
    assert cf[255]["empty_blocks"] == 1 and cf[256]["empty_blocks"] == 0 and cf[256]["chunk"] == 1
    assert cf[257]["chunk"] == 2 and cf[257]["busy_blocks"] == 129 and cf[257]["last_block_short"]
    assert cf[65537]["chunk"] == 257 and cf[65537]["chunk"] > 256 and cf[65537]["last_block_short"]
    assert any(c["kind"] == "zero" for c in E.CLIP_CASES)
    for c in E.CLIP_CASES:
        if c["kind"] != "zero":       # far enough from zero for the 1e-6 of the divisor to stay below the factor 2^-10
            assert float(E.clip_gradient(c).double().norm()) > 0.01, c["id"]
    # decode
    d = {c["id"]: c for c in E.DECODE_CASES}
    assert d["T32-limit"]["T"] == E.BD_MAX["T"] and d["K8-limit"]["K"] == E.BD_MAX["K"]
    assert -(-d["L130"]["L"] // 64) == 3
    lo, hi = d["tie-same-lane-3-67"]["tie"]
    assert lo % 64 == hi % 64 and lo < hi
    for k in ("tie-across-lanes-5-70", "tie-across-lanes-4-69"):
        lo, hi = d[k]["tie"]
        assert lo % 64 != hi % 64 and lo < hi
    lo, hi = d["tie-across-lanes-4-69"]["tie"]
    assert lo % 2 == 0 and hi % 64 % 2 == 1           # lane 0 meets the odd lanes in the butterfly's last exchange
    c8 = d["cpw8-B11-H20"]
    assert c8["cpw"] == 8 and (4 * c8["H"] + 63) // 64 == 2 and c8["B"] == 11


def test_lds_formula_matches_the_library_refusal():
    """the tile's LDS bytes as restated here against objgan_box_train_forward, which checks them before an empty batch
    returns: the same answer for every case under every cpw, and at the real shape, where cpw = 8 is the first refused"""
    from objgan_hip import _lib
    lib = _lib.load()

    def accepted(H, L, K, A, cpw, T=4):
        return lib.objgan_box_train_forward(*([None] * 22), 0.0, 0.0, 0.0, 0.0, None, None, 1 << 40, 0, T, H, L, K, A,
                                            cpw, None) == 1
    shapes = {(c["H"], c["L"], c["K"], c["A"]) for c in E.TRAIN_CASES} | {(256, 83, 5, 50), (256, 256, 8, 64), (128, 83, 5, 50)}
    refused = []
    for H, L, K, A in sorted(shapes):
        for cpw in (1, 2, 4, 8):
            fits = E.train_lds_bytes(H, L, K, A, cpw) <= E.LDS_BYTES
            assert accepted(H, L, K, A, cpw) == fits, (H, L, K, A, cpw)
            if not fits:
                refused.append((H, L, K, A, cpw))
    assert (256, 83, 5, 50, 8) in refused and (256, 83, 5, 50, 4) not in refused
    assert (256, 256, 8, 64, 8) in refused and (256, 256, 8, 64, 4) not in refused
    # every case fits under every cpw it is launched with (the invariance batch under all four), in both kernels
    for c in E.TRAIN_CASES:
        for cpw in ((1, 2, 4, 8) if c["id"] == E.CPW_INVARIANT else (c["cpw"],)):
            assert E.train_lds_bytes(c["H"], c["L"], c["K"], c["A"], cpw) <= E.LDS_BYTES
            assert E.bptt_lds_bytes(c["H"], cpw) <= E.LDS_BYTES
    # bd_launch: the same tile with a 4-float state record; its entry point returns for B = 0 before the check, so the
    # refusal itself is exercised on the device (test_boxgen_edges_gpu.py)
    for c in E.DECODE_CASES:
        assert E.decode_lds_bytes(c["H"], c["L"], c["K"], c["A"], c["cpw"]) <= E.LDS_BYTES
        assert E.train_lds_bytes(c["H"], c["L"], c["K"], c["A"], 1) - E.decode_lds_bytes(c["H"], c["L"], c["K"], c["A"], 1) == 16
    assert E.decode_lds_bytes(256, 83, 5, 50, 8) > E.LDS_BYTES >= E.decode_lds_bytes(256, 83, 5, 50, 4)


@pytest.mark.parametrize("case", WITH_REF, ids=[c["id"] for c in WITH_REF])
def test_fp32_restatement_within_bounds_and_margins(case):
    ref, o32 = E.train_reference(case["id"]), E.train_reference(case["id"], torch.float32)
    clamped = E.build_train(case)["clamped"]
    l2 = E.rel_l2_tensors(o32, ref)
    assert max(l2.values()) <= TO.BOUND, l2
    worst = E.compare(E.train_blocks(case, o32, clamped), E.train_blocks(case, o32, clamped),
                      E.train_blocks(case, ref, clamped))
    for fam, (_, name, e_o, _) in worst.items():
        assert e_o <= TO.BOUND, (fam, name, e_o)
    assert ref["label_margin"] >= 2 and o32["label_margin"] >= 2
    if case.get("norm_clamp"):
        assert ref["norm_margin"] < 1 and o32["norm_margin"] < 1          # the gn = 0 branch is taken
        o = case["L"] + 6 * case["K"]
        wh = torch.stack([ref["trace"][b, t, o:] for b, n in enumerate(clamped) for t in range(n)])
        nraw = 2 * np.pi * wh[:, 3] * wh[:, 4] * torch.sqrt(1 - wh[:, 5] ** 2)
        assert float(nraw.max()) <= 0.5e-5                               # at EVERY step, none within a factor 2 of the edge
        for b, n in enumerate(clamped):                                  # and z is O(1) at each caption's tuned step
            row, box = ref["trace"][b, n - 1], E.build_train(case)["boxes"][b, n]
            za = (float(box[2]) - float(row[o + 1])) / float(row[o + 3])
            zb = (float(box[3]) - float(row[o + 2])) / float(row[o + 4])
            assert abs(za - 0.5) < 1e-3 and abs(zb + 0.25) < 1e-3, (b, za, zb)
    else:
        assert ref["norm_margin"] >= 2 and o32["norm_margin"] >= 2
    assert o32["matches"] == ref["matches"]
    assert [int(v) for v in ref["sums"][:, 2]] == [sum(1 for t in range(n) if E.build_train(case)["labels"][b, t + 1] != case["pad"])
                                                   for b, n in enumerate(clamped)]
    # rows past a clamped length are zero in the reference too
    for b, n in enumerate(clamped):
        assert not ref["trace"][b, n:].any() and not ref["dtrace"][b, n:].any()


def test_defaults_of_the_extended_restatement_are_unchanged():
    """pad = 0, dtrace off: the keys and the values existing callers and goldens see"""
    case = TRAIN["lens-clamped"]
    b = E.build_train(case)
    args = (b["sd"], b["h0"], b["c0"], b["labels"], b["boxes"], b["clamped"], E.FIRST, b["weight"], 1.0, 1.0, case["K"])
    plain, ext = TO.step_ref(*args), E.train_reference(case["id"])
    assert sorted(plain) == ["grads", "label_margin", "loss", "matches", "norm_margin", "sums", "trace"]
    assert plain["loss"] == ext["loss"] and torch.equal(plain["trace"], ext["trace"])
    assert all(torch.equal(plain["grads"][k], ext["grads"][k]) for k in plain["grads"])


def test_pad_restatement_matches_the_loss_classes():
    """`pad=2` against seq2seq.loss.Perplexity / BBLoss fed the restatement's own trace: label term, box term, counts"""
    from seq2seq.loss import Perplexity, BBLoss
    case = TRAIN["pad2"]
    b, ref = E.build_train(case), E.train_reference("pad2")
    L, K = case["L"], case["K"]
    lsum = bsum = 0.0
    n_all = 0
    for i, n in enumerate(b["clamped"]):
        lloss, bloss = Perplexity(b["weight"].double().clone(), case["pad"], 1.0), BBLoss(1, K, 1.0)
        lloss.reset()
        bloss.reset()
        tr = ref["trace"][i]
        for t in range(n):
            tl = torch.tensor([int(b["labels"][i, t + 1])])
            box = [torch.tensor([float(v)], dtype=torch.float64) for v in b["boxes"][i, t + 1]]
            xy = tuple(tr[t:t + 1, L + j * K:L + (j + 1) * K] for j in range(6))
            wh = tuple(tr[t:t + 1, L + 6 * K + j * K:L + 6 * K + (j + 1) * K] for j in range(6))
            lloss.eval_batch(tr[t:t + 1, :L], tl)
            bloss.eval_batch(xy, wh, box[0], box[1], box[2], box[3], tl)
        assert abs(float(lloss.acc_loss) - float(ref["sums"][i, 0])) <= 1e-12 * abs(float(ref["sums"][i, 0]))
        assert abs(float(bloss.acc_loss) - float(ref["sums"][i, 1])) <= 1e-12 * abs(float(ref["sums"][i, 1]))
        assert int(lloss.norm_term) == int(ref["sums"][i, 2]) == n - 1          # <eos> is the pad: not counted
        assert int(bloss.norm_term) == int((b["labels"][i, 1:n + 1] != 0).sum())   # the box mask stays label != 0
        lsum, bsum, n_all = lsum + float(lloss.acc_loss), bsum + float(bloss.acc_loss), n_all + int(lloss.norm_term)
    assert abs((lsum + bsum) / n_all - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    # under pad = 0 the same targets count the mid-caption pad out and <eos> in
    assert [int(v) for v in E.train_reference("pad-inside-caption")["sums"][:, 2]] == [5, 4]


PROBES = [("lens-clamped", 0, 2), ("lens-clamped", 4, 0), ("pad-inside-caption", 0, 2), ("pad-inside-caption", 0, 3),
          ("pad2", 0, 5), ("pad2", 1, 3), ("norm-clamp-K1-tuned", 0, 6), ("norm-clamp-K1-tuned", 2, 1),
          ("norm-clamp-K1-tuned", 1, 0), ("K8-limit", 2, 5)]


@pytest.mark.parametrize("cid,b,t", PROBES, ids=["%s-b%d-t%d" % p for p in PROBES])
def test_dtrace_extension_matches_finite_differences(cid, b, t):
    """step_ref(dtrace=True) against central differences of the fp64 loss of one (b, t) as a function of its row (every
    entry of the row; the tuned rows of the clamp case sit on the flat side of the normaliser clamp)"""
    case, ref = TRAIN[cid], E.train_reference(cid)
    bt = E.build_train(case)
    L, K = case["L"], case["K"]
    N = float(ref["sums"][:, 2].sum())
    row = ref["trace"][b, t].clone()
    assert float(row[:L].min()) > 2e-5                                   # unclamped: the trace row IS the softmax
    nl, box = int(bt["labels"][b, t + 1]), torch.as_tensor(bt["boxes"][b, t + 1]).double()
    f = lambda r: float(E.row_loss(r, nl, box, bt["weight"], N, L, K, case["pad"]))
    got = ref["dtrace"][b, t]
    fd = torch.zeros_like(got)
    for e in range(row.numel()):
        h = 1e-6 * max(abs(float(row[e])), 1e-3)
        up, dn = row.clone(), row.clone()
        up[e] += h
        dn[e] -= h
        fd[e] = (f(up) - f(dn)) / (2 * h)
    scale = float(fd.abs().max())
    if nl == 0:
        assert not got[L:].any() and not fd[L:].any()                   # mask = 0: no box gradient at all
        if case["pad"] == 0:
            assert scale == 0 and not got.any()                         # and weight[<pad>] = 0: nothing at all
            return
    assert scale > 0 and float((got - fd).abs().max()) <= 1e-5 * scale, (float((got - fd).abs().max()), scale)
    if case.get("norm_clamp"):
        # with the normaliser clamped, sigma and rho get gradient through z alone
        o = L + 6 * K
        assert 2 * np.pi * float(row[o + 3]) * float(row[o + 4]) * np.sqrt(1 - float(row[o + 5]) ** 2) < 0.5e-5
        assert abs(float(got[o + 3])) > 0 and abs(float(got[o + 5])) > 0


@pytest.mark.parametrize("cid", ["pad2", "norm-clamp-K1-tuned", "K8-limit", "lens-clamped"])
def test_loss_reference_on_the_restatements_own_trace(cid):
    """the loss as a function of a given trace (the reference of the loss entry point alone), fed the restatement's own
    fp64 trace: the restatement's sums and dtrace"""
    case, ref = TRAIN[cid], E.train_reference(cid)
    sums, dtrace = E.loss_reference(case, E.build_train(case), ref["trace"])
    assert E.max_err(sums, ref["sums"][:, :2]) <= 1e-13
    for b in range(dtrace.shape[0]):
        for t in range(dtrace.shape[1]):
            assert E.max_err(dtrace[b, t], ref["dtrace"][b, t]) <= 1e-12, (b, t)


def test_label_clamp_rows_have_zero_dtrace():
    """where the clamp is active the extension returns zero, which is what the kernel documents"""
    case = TRAIN["lens-clamped"]
    b = E.build_train(case)
    sd = {k: v.clone() for k, v in b["sd"].items()}
    sd["l_out.bias"][2] += 14.0                           # <eos> takes everything: the other labels fall below 1e-5
    r = TO.step_ref(sd, b["h0"], b["c0"], b["labels"], b["boxes"], b["clamped"], E.FIRST, b["weight"], 1.0, 1.0,
                    case["K"], dtrace=True)
    L = case["L"]
    clamped_rows = 0
    for i, n in enumerate(b["clamped"]):
        for t in range(n):
            nl = int(b["labels"][i, t + 1])
            if float(r["trace"][i, t, nl]) == 1e-5:
                clamped_rows += 1
                assert not r["dtrace"][i, t, :L].any()
    assert clamped_rows >= 3


@pytest.mark.parametrize("case", E.DECODE_CASES, ids=[c["id"] for c in E.DECODE_CASES])
def test_decode_margin_cap_and_restatements_agree(case):
    """the restatement alone leaves out at most 1 caption in 4; fp32 and fp64 restatement take the same decisions on
    the kept captions and stay inside the operator bound; each case ends where its id says"""
    r64, r32 = E.decode_reference(case["id"]), E.decode_reference(case["id"], torch.float32)
    keep = E.decode_keep(case)
    assert len(keep) >= case["B"] - case["B"] // 4, "pick another seed"
    for b in keep:
        assert int(r32[1][b]) == int(r64[1][b]) and np.array_equal(r32[0][b], r64[0][b])
        for i in (2, 3):
            assert BO.trajectory_error(r32[i][b], r64[i][b]) <= TO.BOUND
    lens = r32[1].tolist()
    if case["id"] == "cpw8-B11-H20":
        assert 1 in lens[:8] and case["T"] in lens[:8] and len(set(lens)) >= 3      # frozen captions beside live ones
    if case["id"] == "T32-limit":
        assert lens.count(32) >= case["B"] - 1
    if case["id"] == "all-end-at-step-1":
        assert lens == [1] * case["B"]
    if case["id"] == "L130":
        assert r32[0].max() >= 128                                          # a label of the third lane trip wins
    if case["tie"]:
        lo, hi = case["tie"]
        sd = E.build_decode(case)["sd"]
        assert torch.equal(sd["l_out.weight"][lo], sd["l_out.weight"][hi]) and sd["l_out.bias"][lo] == sd["l_out.bias"][hi]
        L = case["L"]
        assert (r64[3][:, 0, lo] == r64[3][:, 0, hi]).all() and (r64[3][:, 0, :L].argmax(1) == lo).all()
        others = np.delete(r64[3][:, 0, :L], [lo, hi], axis=1)
        assert (others.max(1) < 0.5 * r64[3][:, 0, lo]).all()               # the tied pair IS the maximum
