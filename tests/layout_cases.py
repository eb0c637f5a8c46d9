"""TEST INFRASTRUCTURE shared by tests/test_layout_cpu.py and tests/test_layout_gpu.py: crafted decoder outputs for the
layout stage (csrc/layout.hip), the FILE ROUTE that is its oracle -- Evaluator.postprocess -> write_layouts ->
load_gen_insanns -> get_gen_rois through a temporary directory --, and the list of branches the cases must reach.

Small shapes: B <= 6, T from 2 to 17, L = 8 labels, R = 10, imsize (64, 128, 256), fmsize 16.  The crafted cases use the
trivial de-normalisation (mean 0, std 1), so that a sample IS the box value and every edge can be placed exactly; the
`random` case has ordinary means and stds and exercises the rounding of the fp64 chain.  `gaussian_dict` has sigma = 0:
np.random.normal(mu, 0) == mu, the file route's thresholds are deterministic."""
import contextlib
import os
from fractions import Fraction

import numpy as np

IMSIZE, FMSIZE, R, MIN_SIZE = (64, 128, 256), 16, 10, 10
WORDS = ["<pad>", "<sos>", "<eos>", "<unk>", "1", "3", "17", "44"]          # decoder label -> word
EOS = 2
LAB = {1: 4, 3: 5, 17: 6, 44: 7}                                            # category id -> decoder label
CATS_INDEX = {1: 0, 3: 1, 17: 2, 44: 3}                                     # category id -> row of categories.txt
GAUSS = {1: (3.0, 0.0), 3: (2.9, 0.0), 17: (1.2, 0.0), 44: (20.5, 0.0)}     # caps 3, 2, 2 (the floor of 2), 20
TRIVIAL = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)

BRANCHES = ("nonpositive_x", "nonpositive_y", "nonpositive_w", "nonpositive_h", "zero_survivors", "one_survivor",
            "over_cap_interleaved", "clip_low", "clip_high", "w_cut", "h_cut",
            "frac_below_995", "frac_above_995", "frac_below_995_k0", "frac_above_995_k0",
            "both_sides_small", "one_side_small", "more_than_R_tied", "half_even", "half_odd",
            "clamp_63", "clamp_15", "empty_slice", "short_length")


class LabelLang(object):
    index2word = dict(enumerate(WORDS))
    word2index = {w: i for i, w in enumerate(WORDS)}


def around_995(k):
    """the two neighbouring doubles whose exact values lie below and above k + 0.995"""
    target = Fraction(k) + Fraction(199, 200)
    v = np.float64(k + 0.995)
    while Fraction(float(v)) > target:
        v = np.nextafter(v, -np.inf)
    while Fraction(float(np.nextafter(v, np.inf))) < target:
        v = np.nextafter(v, np.inf)
    lo, hi = float(v), float(np.nextafter(v, np.inf))
    assert Fraction(lo) < target < Fraction(hi)
    assert '%.2f' % lo == '%.2f' % (k + 0.99) and '%.2f' % hi == '%.2f' % (k + 1)
    return lo, hi


def entry(x0, y0, w, h, cat):
    """a decoder step (label, centre x, centre y, w, ratio) whose post-processed box is EXACTLY corner (x0, y0), size
    (w, h) before clipping -- the arithmetic of postprocess is checked to reproduce the four values"""
    r = h / w
    for cand in (r, float(np.nextafter(r, np.inf)), float(np.nextafter(r, -np.inf))):
        if w * cand == h:
            r = cand
            break
    cx, cy = x0 + w / 2.0, y0 + h / 2.0
    assert w * r == h and cx - w / 2.0 == x0 and cy - h / 2.0 == y0, (x0, y0, w, h)
    return (LAB[cat], cx, cy, w, r)


def raw(label, cx, cy, w, r):
    return (label, cx, cy, w, r)


END = (EOS, 50.0, 50.0, 20.0, 1.0)              # the <eos> step: valid values, dropped as the last surviving entry


def _pack(name, captions, T, mean_std=TRIVIAL, lengths=None):
    B = len(captions)
    labels = np.zeros((B, T), np.int32)
    samples = np.zeros((B, T, 4), np.float64)
    lens = np.zeros((B,), np.int32)
    for b, cap in enumerate(captions):
        assert len(cap) <= T
        for t, (l, cx, cy, w, r) in enumerate(cap):
            labels[b, t] = l
            samples[b, t] = (cx, cy, w, r)
        lens[b] = len(cap) if lengths is None or lengths[b] is None else lengths[b]
    return {"name": name, "labels": labels, "lengths": lens, "samples": samples,
            "mean_std": np.array(mean_std, np.float64)}


def cases():
    out = []
    # ---- the positivity filter, the survivor counts, lengths shorter than T ----
    ok = lambda i, cat=1: entry(20.0 + 8 * i, 30.0 + 4 * i, 32.0, 16.0, cat)
    out.append(_pack("filter", [
        [ok(0), raw(LAB[3], -3.0, 40.0, 32.0, 1.0), ok(1, 3), raw(LAB[1], 40.0, -2.5, 32.0, 1.0),
         raw(LAB[17], 40.0, 40.0, -32.0, -1.0), raw(LAB[17], 40.0, 40.0, 32.0, -0.5), ok(2, 17), END],
        [raw(LAB[1], -1.0, 5.0, 5.0, 1.0), raw(EOS, 5.0, -1.0, 5.0, 1.0)],                      # nothing survives
        [raw(LAB[1], -1.0, 5.0, 5.0, 1.0), END],                                                # one survivor: no boxes
        [ok(3, 44), END],                                                                       # two survivors: one box
        # `lengths` 3 of T = 8: what follows looks valid and must not be read
        [ok(4), ok(5, 3), END, ok(6, 17), ok(7, 44)],
        [END],
    ], T=8, lengths=[None, None, None, None, 3, None]))
    # ---- a category over its cap, labels interleaved (caps: 1 -> 3, 3 -> 2, 17 -> 2) ----
    seq = [1, 3, 1, 17, 1, 3, 1, 3, 17, 17, 44]
    out.append(_pack("caps", [[ok(i, c) for i, c in enumerate(seq)] + [END],
                              [ok(i, c) for i, c in enumerate(seq[:5])] + [END]], T=12))
    # ---- clipping at 1 and 255, w / h cut by 256 - x ----
    out.append(_pack("clip", [
        [raw(LAB[1], 5.0, 100.0, 64.0, 0.5),            # x0 = -27 -> 1
         raw(LAB[3], 100.0, 3.0, 32.0, 2.0),            # y0 = -29 -> 1
         raw(LAB[17], 300.0, 100.0, 20.0, 1.0),         # x0 = 290 -> 255, w -> 1
         raw(LAB[44], 100.0, 310.0, 20.0, 2.0),         # y0 = 290 -> 255, h -> 1
         entry(200.0, 50.0, 100.0, 50.0, 1),            # w -> 56: x + w = 256, bound clamped to 63 and to 15
         entry(50.0, 180.0, 32.0, 128.0, 3),            # h -> 76
         END]], T=7))
    # ---- fractional parts next to .995 (k = 0 included), minimum size with one or both sides below 10 ----
    lo0, hi0 = around_995(0)
    lo20, hi20 = around_995(20)
    lo100, hi100 = around_995(100)
    lo37, hi37 = around_995(37)
    lo9, hi9 = around_995(9)
    out.append(_pack("frac", [
        [raw(LAB[1], 60.0, 60.0, lo0, 64.0), raw(LAB[3], 60.0, 60.0, hi0, 64.0),     # w 0.99.. -> 0 / 1, h = 64 w
         raw(LAB[17], 60.0, 60.0, 64.0, lo0 / 64.0), raw(LAB[44], 60.0, 60.0, 64.0, hi0 / 64.0), END],
        [entry(lo100, lo37, 32.0, 32.0, 1), entry(hi100, hi37, 32.0, 32.0, 3),
         raw(LAB[17], 90.0, 90.0, lo20, 1.0), raw(LAB[44], 90.0, 90.0, hi20, 1.0), END],
        [entry(30.0, 30.0, 9.5, 9.5 * 1.0, 1),                       # 9 x 9: dropped
         entry(30.0, 30.0, 8.0, 32.0, 3),                            # 8 x 32: kept
         entry(30.0, 30.0, 32.0, 4.0, 17),                           # 32 x 4: kept
         raw(LAB[44], 90.0, 90.0, lo9, 0.5),                         # 9.99.. -> 9, h 4: dropped
         raw(LAB[44], 90.0, 90.0, hi9, 0.5),                         # -> '10.00': kept
         END]], T=6))
    # ---- more than R boxes, tied areas on both sides of the cut; exactly R after the size filter; T = 17 ----
    sides = [(20, 30), (30, 20), (24, 25), (20, 20), (16, 25), (30, 30), (10, 10), (15, 40), (50, 50), (40, 10),
             (40, 40), (12, 50), (25, 16), (15, 15), (10, 40), (60, 10)]
    # areas: 2500, 1600, 900, six of 600, five of 400 (only the LAST of them is within the ten), 225, 100
    many = [entry(10.0 + 3 * i, 12.0 + 5 * i, float(w), float(h), 1 if i in (0, 5) else 44) for i, (w, h) in enumerate(sides)]
    eleven = [entry(10.0 + 3 * i, 12.0, 16.0, 32.0, 44) for i in range(10)] + [entry(9.0, 9.0, 8.0, 8.0, 44)]
    twelve = [entry(10.0 + 3 * i, 12.0, 16.0 + 2 * i, 32.0, 44) for i in range(12)]
    perm = [5, 12, 0, 9, 3, 15, 7, 1, 11, 14, 2, 8, 13, 4, 10, 6]
    sixteen = [entry(10.0 + 3 * i, 12.0, 16.0 + 2 * p, 32.0, 44) for i, p in enumerate(perm)]     # distinct areas
    out.append(_pack("many", [sixteen + [END], eleven + [END], twelve + [END]], T=17))
    out.append(_pack("tied", [many + [END]], T=17))
    # 11 .. 16 boxes with sides of 10 or 20: every cut falls into a run of equal areas
    rs = np.random.RandomState(3)
    caps = []
    for n in (11, 12, 13, 14, 15, 16):
        wh = rs.choice([10.0, 20.0], size=(n, 2))
        caps.append([entry(10.0 + 3 * i, 12.0 + 2 * i, wh[i, 0], wh[i, 1], 44) for i in range(n)] + [END])
    out.append(_pack("tied_random", caps, T=17))
    # ---- 64-scale coordinates ending in .5 with an even and an odd integer part; empty slices ----
    out.append(_pack("round", [
        [entry(2.0, 6.0, 40.0, 40.0, 1),                # 0.5 -> 0, 1.5 -> 2; 10.5 -> 10, 11.5 -> 12
         entry(10.0, 14.0, 16.0, 16.0, 3),              # 2.5 -> 2, 3.5 -> 4
         entry(8.0, 24.0, 48.0, 32.0, 17),              # feature map: 0.5 -> 0, 1.5 -> 2; 3.5 -> 4
         entry(255.0, 40.0, 1.0, 64.0, 44),             # x 63.75 -> 64 -> 63, x + w 64 -> 63: empty
         entry(40.0, 40.0, 0.5, 32.0, 44),              # w 0.5 -> '0.50' -> 0: x0 == x1, empty
         END]], T=6))
    # ---- ordinary means and stds, normal samples: the fp64 chain as the decoder feeds it ----
    rs = np.random.RandomState(7)
    B, T = 6, 10
    c = _pack("random", [[] for _ in range(B)], T=T,
              mean_std=(120.53, 60.31, 130.27, 55.13, 80.71, 50.93, 1.13, 0.61))
    c["samples"][:] = rs.standard_normal((B, T, 4))
    c["labels"][:] = rs.randint(4, 8, size=(B, T))
    c["lengths"][:] = [10, 7, 10, 4, 9, 2]
    for b in range(B):
        c["labels"][b, c["lengths"][b] - 1] = EOS
        c["samples"][b, c["lengths"][b] - 1] = (0.1, 0.1, 0.1, 0.1)
    out.append(c)
    return out


def thresholds(B):
    """[B, L] int32: max(int(mu), 2) for the category labels (sigma = 0), a large cap for the others"""
    th = np.full((B, len(WORDS)), 1 << 30, np.int32)
    for cat, l in LAB.items():
        th[:, l] = max(int(GAUSS[cat][0]), 2)
    return th


def label_to_cat():
    return np.array([int(w) if w.isdigit() else -1 for w in WORDS], np.int32)


def cat_to_rel():
    t = np.full((max(CATS_INDEX) + 1,), -1, np.int32)
    for cat, rel in CATS_INDEX.items():
        t[cat] = rel
    return t


@contextlib.contextmanager
def layout_cfg():
    """the configuration values the file route reads, set to this module's and put back afterwards"""
    from miscc.config import cfg
    saved = (cfg.TREE.BRANCH_NUM, cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM, cfg.ROI.ROI_MIN_SIZE, cfg.ROI.FM_SIZE)
    cfg.TREE.BRANCH_NUM, cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM, cfg.ROI.ROI_MIN_SIZE, cfg.ROI.FM_SIZE = \
        len(IMSIZE), R, 6, MIN_SIZE, FMSIZE
    try:
        yield cfg
    finally:
        cfg.TREE.BRANCH_NUM, cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM, cfg.ROI.ROI_MIN_SIZE, cfg.ROI.FM_SIZE = saved


def make_evaluator(mean_std, data_dir, label_lang=LabelLang, gaussian_dict=GAUSS):
    from seq2seq.evaluator import Evaluator
    ms = [float(v) for v in mean_std]
    return Evaluator(4, None, data_dir, None, label_lang, ms[0:2], ms[2:4], ms[4:6], ms[6:8], gaussian_dict,
                     os.path.join(data_dir, "gen_masks") + "/", 0)


def decoded_of(case):
    """per caption (sequence, xy, wh), as DecoderRNN.forward hands them to the evaluator"""
    out = []
    for b in range(case["labels"].shape[0]):
        n = int(case["lengths"][b])
        s = case["samples"][b, :n]
        out.append((case["labels"][b, :n].astype(np.int64), [(r[0], r[1]) for r in s], [(r[2], r[3]) for r in s]))
    return out


def file_route(case, data_dir, cats_index=CATS_INDEX, evaluator=None):
    """The oracle: the case through the files.  -> dict of numpy arrays shaped like the outputs of
    ops.layout_from_decode, plus the dataset's one-hot stacks (bbox_maps_fwd / bwd [B, R, C, S, S], bbox_fmaps)."""
    from miscc import load
    B, T = case["labels"].shape
    keys = ["cap%02d" % b for b in range(B)]
    ev = evaluator if evaluator is not None else make_evaluator(case["mean_std"], data_dir)
    with layout_cfg():
        layouts = ev.write_layouts(decoded_of(case), keys)
        anns = load.load_gen_insanns(data_dir, keys, "test", list(IMSIZE), FMSIZE, cats_index)
        S, C = IMSIZE[0], len(cats_index)
        res = {"boxes": np.zeros((B, T, 5)), "nbox": np.zeros((B,), np.int32),
               "rois": [np.zeros((B, R, 6)) for _ in IMSIZE], "fm_rois": np.zeros((B, R, 6)),
               "num_rois": np.zeros((B,), np.int32), "cats": np.zeros((B, R), np.int32),
               "raw_maps": np.zeros((B, R, S, S), np.float32), "raw_fmaps": np.zeros((B, R, FMSIZE, FMSIZE), np.float32),
               "bbox_maps_fwd": np.zeros((B, R, C, S, S)), "bbox_maps_bwd": np.zeros((B, R, C, S, S)),
               "bbox_fmaps": np.zeros((B, R, FMSIZE, FMSIZE)), "files": []}
        for b, key in enumerate(keys):
            res["nbox"][b] = len(layouts[b])
            for i, (x, y, w, h, l) in enumerate(layouts[b]):
                res["boxes"][b, i] = (x, y, w, h, int(l))
            with open(os.path.join(data_dir, "gen_masks", key, "0", "boxes.txt"), "rb") as f:
                res["files"].append(f.read())
            fwd, bwd, fmaps, rois, fm_rois, n = load.get_gen_rois(anns[key], list(IMSIZE), FMSIZE, cats_index, 0)
            for i in range(len(IMSIZE)):
                res["rois"][i][b] = rois[i]
            res["fm_rois"][b] = fm_rois
            res["num_rois"][b] = n
            res["cats"][b] = rois[0][:, 4].astype(np.int32)
            if n > 0:
                res["raw_maps"][b, :n] = anns[key][0]["bbox maps"]
                res["raw_fmaps"][b, :n] = anns[key][0]["bbox fmaps"]
            res["bbox_maps_fwd"][b], res["bbox_maps_bwd"][b], res["bbox_fmaps"][b] = fwd, bwd, fmaps
    return res


def _denormalised(case):
    ms = case["mean_std"]
    s = case["samples"]
    x, y, w = (s[..., i] * ms[2 * i + 1] + ms[2 * i] for i in range(3))
    r = s[..., 3] * ms[7] + ms[6]
    return x, y, w, np.multiply(w, r), r


def positivity_margin_ok(case):
    """no de-normalised value of a decoded step within 2 ulp (of the larger term of its sum) of the `> 0` decision"""
    ms, s = case["mean_std"], case["samples"]
    x, y, w, h, r = _denormalised(case)
    ok = True
    for b in range(s.shape[0]):
        n = int(case["lengths"][b])
        for i, v in enumerate((x, y, w, r)):
            scale = np.maximum(np.abs(s[b, :n, i] * ms[2 * i + 1]), abs(ms[2 * i]))
            ok = ok and bool(np.all(np.abs(v[b, :n]) > 2 * np.spacing(scale)))
        ok = ok and bool(np.all(np.abs(h[b, :n]) > 2 * np.spacing(np.abs(h[b, :n]))))
    return ok


def branches_hit(case, res):
    """which of BRANCHES this case reaches -- read off the inputs and the file route's own results"""
    hit = set()
    x, y, w, h, _ = _denormalised(case)
    B, T = case["labels"].shape
    lo_hi = {k: around_995(k) for k in (0, 9, 20, 37, 100)}
    for b in range(B):
        n = int(case["lengths"][b])
        if n < T and np.any(case["samples"][b, n:] != 0):
            hit.add("short_length")
        xs, ys, ws, hs = x[b, :n], y[b, :n], w[b, :n], h[b, :n]
        for name, v in (("x", xs), ("y", ys), ("w", ws), ("h", hs)):
            if np.any(v <= 0):
                hit.add("nonpositive_" + name)
        valid = (xs > 0) & (ys > 0) & (ws > 0) & (hs > 0)
        if valid.sum() == 0:
            hit.add("zero_survivors")
        if valid.sum() == 1:
            hit.add("one_survivor")
        if valid.sum() <= 1:
            continue
        idx = np.where(valid)[0][:-1]
        cats = [int(WORDS[case["labels"][b, i]]) for i in idx]
        caps = {c: max(int(GAUSS[c][0]), 2) for c in set(cats)}
        for c in set(cats):
            pos = [k for k, cc in enumerate(cats) if cc == c]
            if len(pos) > caps[c] and any(cats[k] != c for k in range(pos[0], pos[-1])):
                hit.add("over_cap_interleaved")
        nb = int(res["nbox"][b])
        bx = res["boxes"][b, :nb]
        kept, seen = [], {}
        for k, c in enumerate(cats):
            seen[c] = seen.get(c, 0) + 1
            if seen[c] <= caps[c]:
                kept.append(idx[k])
        for row, i in zip(bx, kept):
            x0, y0 = xs[i] - ws[i] / 2.0, ys[i] - hs[i] / 2.0
            if x0 < 1 or y0 < 1:
                hit.add("clip_low")
            if x0 > 255 or y0 > 255:
                hit.add("clip_high")
            if row[2] < ws[i]:
                hit.add("w_cut")
            if row[3] < hs[i]:
                hit.add("h_cut")
            for v in row[:4]:
                for k, (lo, hi) in lo_hi.items():
                    if v == lo:
                        hit.add("frac_below_995" + ("_k0" if k == 0 else ""))
                    if v == hi:
                        hit.add("frac_above_995" + ("_k0" if k == 0 else ""))
        ints = np.array([[int(float('%.2f' % v)) for v in row[:4]] for row in bx]).reshape(-1, 4)
        small = ints[:, 2:] < MIN_SIZE
        if np.any(small.all(1)):
            hit.add("both_sides_small")
        if np.any(small.any(1) & ~small.all(1)):
            hit.add("one_side_small")
        keep = ints[~small.all(1)]
        if len(keep) > R:
            areas = np.sort(keep[:, 2] * keep[:, 3])[::-1]
            if areas[R - 1] == areas[R] and len(set(areas[:R].tolist())) < R:
                hit.add("more_than_R_tied")
        nr = int(res["num_rois"][b])
        for row in res["rois"][0][b, :nr]:
            for v in (row[0], row[1], row[0] + row[2], row[1] + row[3]):
                if v % 1 == 0.5:
                    hit.add("half_even" if int(v) % 2 == 0 else "half_odd")
                if round(v) > IMSIZE[0] - 1:
                    hit.add("clamp_63")
        for row in res["fm_rois"][b, :nr]:
            for v in (row[0] / 2.0 + row[2] / 2.0, row[1] / 2.0 + row[3] / 2.0):
                if round(v) > FMSIZE - 1:
                    hit.add("clamp_15")
        for r_ in range(nr):
            if not res["raw_maps"][b, r_].any():
                hit.add("empty_slice")
    return hit
