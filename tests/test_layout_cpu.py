"""Host side of the caption-to-image pipeline: the crafted cases of tests/layout_cases.py through the FILE ROUTE alone
(that they reach every branch the device layout stage has is a property of the inputs, shown here without the kernel),
Evaluator.draw_thresholds / layout_tables, the tokeniser and its refusals, generate.py's answers to missing files and
the boxes.txt writer."""
import os

import numpy as np
import pytest

import layout_cases as LC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    out = []
    for case in LC.cases():
        out.append((case, LC.file_route(case, str(tmp_path_factory.mktemp(case["name"])))))
    return out


def test_cases_stay_within_the_small_shapes():
    for case in LC.cases():
        B, T = case["labels"].shape
        assert B <= 6 and 2 <= T <= 17 and case["samples"].shape == (B, T, 4)
        assert np.all(case["lengths"] >= 1) and np.all(case["lengths"] <= T)
    assert {c["labels"].shape[1] for c in LC.cases()} >= {6, 17}


def test_every_branch_is_reached_by_the_file_route(routed):
    hit = {}
    for case, res in routed:
        for name in LC.branches_hit(case, res):
            hit.setdefault(name, []).append(case["name"])
    missing = [b for b in LC.BRANCHES if b not in hit]
    assert not missing, missing


def test_no_value_sits_on_a_positivity_decision(routed):
    """2 ulp around `> 0`; the .995 neighbours are the intended exception ('%.2f' decides them, exactly)"""
    for case, _ in routed:
        assert LC.positivity_margin_ok(case), case["name"]


def test_file_route_shapes_and_counts(routed):
    by_name = {case["name"]: res for case, res in routed}
    assert by_name["filter"]["nbox"].tolist() == [3, 0, 0, 1, 2, 0]
    assert by_name["caps"]["nbox"].tolist() == [3 + 2 + 2 + 1, 5]
    assert by_name["many"]["nbox"].tolist() == [16, 11, 12] and by_name["many"]["num_rois"].tolist() == [10, 10, 10]
    assert by_name["tied"]["nbox"].tolist() == [16] and by_name["tied"]["num_rois"].tolist() == [10]
    assert by_name["tied_random"]["nbox"].tolist() == [11, 12, 13, 14, 15, 16]
    for res in by_name.values():
        assert np.all(res["num_rois"] <= res["nbox"]) and np.all(res["num_rois"] <= LC.R)


def test_boxes_txt_writer_matches_write_layouts(routed):
    import pipeline
    for case, res in routed:
        for b in range(case["labels"].shape[0]):
            rows = res["boxes"][b, :int(res["nbox"][b])]
            assert pipeline.boxes_txt(rows).encode() == res["files"][b], (case["name"], b)
    assert any(len(f) == 0 for _, res in routed for f in res["files"])          # a caption without boxes: empty file


def test_argsort_tie_rule_describes_this_host():
    """the probe behind ops.layout_from_decode's default says what np.argsort does here with equal keys: 0 the stable
    order, 1 the AVX-512 network's, None neither (then a cut among equal areas is refused, not guessed)"""
    from objgan_hip import ops
    rule = ops.argsort_tie_rule()
    assert rule in (0, 1, None)
    for keys, network in ops._ARGSORT_PROBES:
        a = np.array(keys, np.float64)
        got, stable = np.argsort(a).tolist(), np.argsort(a, kind="stable").tolist()
        assert list(network) != stable and sorted(network) == list(range(len(keys)))
        assert a[list(network)].tolist() == sorted(keys)                  # the recorded order is an ascending one
        if rule is not None:
            assert got == (stable if rule == 0 else list(network))


def _evaluator(gauss):
    from seq2seq.evaluator import Evaluator
    return Evaluator(4, 10, '', None, LC.LabelLang, (1.0, 2.0), (3.0, 4.0), (5.0, 6.0), (7.0, 8.0), gauss, '', 0)


def test_draw_thresholds():
    ev = _evaluator({1: (3.4, 1.5), 3: (2.0, 1.0), 17: (1.2, 0.5), 44: (6.0, 3.0)})
    a = ev.draw_thresholds(np.random.RandomState(3), 5)
    assert a.shape == (5, len(LC.WORDS)) and a.dtype == np.int32
    assert np.all(a >= 2)
    assert np.all(a[:, :4] == ev.UNCAPPED) and np.all(a[:, 4:] < 100)
    assert np.array_equal(a, ev.draw_thresholds(np.random.RandomState(3), 5))            # seeded: repeatable
    assert not np.array_equal(a, ev.draw_thresholds(np.random.RandomState(4), 5))
    assert len(set(a[:, 7].tolist())) > 1                                                # drawn per caption
    # sigma = 0: max(int(mu), 2), which is what the file route draws (np.random.normal(mu, 0) == mu)
    z = _evaluator(LC.GAUSS).draw_thresholds(np.random.RandomState(0), 3)
    assert np.array_equal(z, LC.thresholds(3))
    assert z[0, 4:].tolist() == [3, 2, 2, 20]
    # a category the dictionary does not hold is not capped
    assert np.all(_evaluator({1: (3.0, 0.0)}).draw_thresholds(None, 2)[:, 5:] == ev.UNCAPPED)


def test_layout_tables():
    ms, l2c, c2r = _evaluator(LC.GAUSS).layout_tables(LC.CATS_INDEX)
    assert ms.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0] and str(ms.dtype) == "torch.float64"
    assert np.array_equal(l2c.numpy(), LC.label_to_cat()) and np.array_equal(c2r.numpy(), LC.cat_to_rel())
    assert l2c.tolist() == [-1, -1, -1, -1, 1, 3, 17, 44] and c2r[44] == 3 and c2r[2] == -1 and len(c2r) == 45


def test_tokeniser_and_refusals():
    import pipeline
    assert pipeline.tokenize("A man, riding a WAVE -- on top of a surf-board!") == \
        ["a", "man", "riding", "a", "wave", "on", "top", "of", "a", "surf", "board"]
    small = {"a": 1, "man": 2, "wave": 3}
    other = {"man": 7, "riding": 8, "zebra": 9}
    dropped = set()
    ids = pipeline.encode_caption("A man riding a wave", 4, (small, other), 3, dropped)
    assert ids == [[1, 2, 1], [7, 8]]                          # the first words; each vocabulary on its own
    assert dropped == {"riding", "a", "wave"}
    with pytest.raises(ValueError, match="caption 12 "):
        pipeline.encode_caption("Two zebras graze", 12, (small, other), 12)
    with pytest.raises(ValueError, match="caption 3 "):
        pipeline.encode_caption("  ...  ", 3, (small,), 12)


def _argv(tmp_path, **over):
    ckpt = os.path.join(GOLD, "boxgen_tiny", "checkpoints", "tiny")
    data = os.path.join(GOLD, "data_tiny_eval")
    caps = tmp_path / "captions.txt"
    caps.write_text("a person rides a bicycle\n")
    present = tmp_path / "present.pth"
    present.write_bytes(b"x")
    a = {"--captions": str(caps), "--data_dir": data, "--NET_G": str(present), "--box_ckpt": ckpt,
         "--output_dir": str(tmp_path / "out"), "--NET_E": str(present), "--NET_SHP_G": str(present),
         "--mean_std": os.path.join(GOLD, "boxgen_tiny", "mean_std_test.txt"),
         "--gaussian_dict": os.path.join(GOLD, "boxgen_tiny", "gaussian_dict.npy")}
    a.update(over)
    return [v for kv in a.items() for v in kv]


@pytest.mark.parametrize("flag,role", [("--NET_G", "NET_G"), ("--box_ckpt", "box checkpoint model.pt"),
                                       ("--NET_SHP_G", "NET_SHP_G"), ("--captions", "captions file"),
                                       ("--data_dir", "captions.pickle"), ("--gaussian_dict", "gaussian_dict.npy")])
def test_generate_py_answers_a_missing_file_with_status_2(tmp_path, capsys, flag, role):
    import generate
    missing = str(tmp_path / "not_there")
    rc = generate.main(_argv(tmp_path, **{flag: missing}))
    err = capsys.readouterr().err.strip().splitlines()
    assert rc == 2 and len(err) == 1
    assert err[0].startswith("generate.py: %s not found: " % role) and missing in err[0]
    assert not os.path.exists(str(tmp_path / "out"))
