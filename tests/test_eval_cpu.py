"""Evaluation mode, host side: the test-split data path, the FID arithmetic and the R-precision pool against what the
UNMODIFIED reference returned (tests/golden/eval_ref.pt, written by tests/golden/make_golden_eval.py over
tests/golden/data_tiny_eval/), the pool bookkeeping, the activation file format, the CLI wiring and the C-ABI surface."""
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from eval_helpers import check_fp, record_similarities, compare_pool, cfg_snapshot, cfg_restore

DATA = os.path.join(ROOT, "tests", "golden", "data_tiny_eval")
GOLD = os.path.join(ROOT, "tests", "golden", "eval_ref.pt")
NEW_SYMBOLS = ("objgan_bilinear_halfpixel_forward", "objgan_moments_accumulate", "objgan_moments_finalize")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


@pytest.fixture
def cfg():
    """the global configuration, put back exactly as it was after the test"""
    from miscc.config import cfg as c
    saved = cfg_snapshot(c)
    c.TREE.BRANCH_NUM = 3
    c.TEST.SAMPLE_VAL = False
    yield c
    cfg_restore(c, saved)


def _dataset(cfg, mode, data_dir=DATA):
    import testDataset
    cfg.TEST.USE_GT_BOX_SEG = mode
    return testDataset.TestDataset(data_dir, "test", base_size=64)


# ---- (a) data path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_items_match_reference(cfg, gold, mode):
    ds = _dataset(cfg, mode)
    assert len(ds) == 6 and ds.acts_dict is not None and ds.num_classes == 5
    np.random.seed(gold["seeds"]["items"])
    for i, g in enumerate(gold["data"][mode]["items"]):
        it = ds[i]
        assert len(it) == g["len"] == (17 if mode == 0 else 14)
        if mode == 0:
            (imgs, acts, caps, gcaps, cap_len, hmaps, fwd, bwd, fmaps, rois, fm_rois, num_rois, bt, fm_bt, cls_id, key,
             sent) = it
        else:
            imgs, acts, caps, gcaps, cap_len, fwd, bwd, fmaps, rois, fm_rois, num_rois, cls_id, key, sent = it
        assert key == g["key"] and int(sent) == g["sent"] and int(cls_id) == g["cls_id"]      # same caption drawn
        assert int(num_rois) == g["num_rois"] and int(cap_len) == g["cap_len"]
        assert np.array_equal(caps, g["caps"].numpy()) and np.array_equal(gcaps, g["glove_caps"].numpy())
        assert acts.shape == (2048,) and acts.dtype == np.float64
        assert abs(float(np.sum(acts)) - g["acts_sum"]) <= 1e-9 * abs(g["acts_sum"])
        check_fp(imgs[0], g["img64"])
        check_fp(imgs[2], g["img256"])
        check_fp(fwd, g["fwd"])
        check_fp(bwd, g["bwd"])
        assert torch.allclose(torch.as_tensor(fmaps).float(), g["fmaps"], atol=1e-6)
        for r, gr in zip(rois, g["rois"]):
            assert np.array_equal(r, gr.numpy())
        assert np.array_equal(fm_rois, g["fm_rois"].numpy())
        if mode == 0:
            check_fp(hmaps[0], g["hmap64"])
            check_fp(hmaps[2], g["hmap256"])
            check_fp(bt[0], g["bt_mask64"])
            check_fp(bt[2], g["bt_mask256"])
            check_fp(fm_bt, g["fm_bt_masks"])


@pytest.mark.parametrize("mode", [0, 2])
def test_prepare_functions_match_reference(cfg, gold, mode):
    from torch.utils.data.dataloader import default_collate
    import testDataset
    ds = _dataset(cfg, mode)
    np.random.seed(gold["seeds"]["items"])
    batch = default_collate([ds[i] for i in range(len(ds))])
    p = (testDataset.prepare_data if mode == 0 else testDataset.prepare_gen_data)(batch)
    g = gold["data"][mode]["prepared"]
    assert len(p) == g["len"] == (17 if mode == 0 else 14)
    if mode == 0:
        imgs, acts, caps, gcaps, lens, hmaps, fwd, bwd, fmaps, rois, fm_rois, num, bt, fm_bt, cls, keys, sents = p
    else:
        imgs, acts, caps, gcaps, lens, fwd, bwd, fmaps, rois, fm_rois, num, cls, keys, sents = p
    assert keys == g["keys"] and [int(s) for s in sents] == g["sent_ids"]
    assert np.array_equal(np.asarray(cls), g["class_ids"])
    assert torch.equal(lens, g["cap_lens"]) and (lens[:-1] >= lens[1:]).all()
    assert torch.equal(caps, g["captions"]) and torch.equal(gcaps, g["glove_captions"])
    assert torch.equal(num, g["num_rois"])
    for r, gr in zip(rois, g["rois"]):
        assert torch.equal(r, gr)
    assert torch.equal(fm_rois, g["fm_rois"])
    assert isinstance(acts, np.ndarray) and str(acts.dtype) == g["acts_dtype"]
    check_fp(torch.as_tensor(acts).view(1, len(keys), -1), g["acts"])
    check_fp(imgs[0], g["img64"])
    check_fp(imgs[2], g["img256"])
    assert tuple(fwd.shape) == g["fwd_shape"] and fwd.shape[1] == int(num.max())      # cut to the largest box count
    check_fp(fwd, g["fwd"])
    check_fp(bwd, g["bwd"])
    assert torch.allclose(fmaps, g["fmaps"], atol=1e-6)
    assert str(fwd.dtype) == g["dtypes"]["fwd"] and str(rois[0].dtype) == g["dtypes"]["rois"]
    assert str(caps.dtype) == g["dtypes"]["captions"]
    if mode == 0:
        check_fp(hmaps[0], g["hmap64"])
        check_fp(hmaps[2], g["hmap256"])
        check_fp(bt[0], g["bt_mask64"])
        check_fp(fm_bt, g["fm_bt_masks"])
        assert str(hmaps[0].dtype) == g["dtypes"]["hmaps"] and str(bt[0].dtype) == g["dtypes"]["bt_masks"]


def test_activation_pass_items_without_the_activation_file(cfg, gold, tmp_path):
    """no <split>_acts_tf0.pickle: items are (imgs, key), whatever cfg.TEST.USE_TF says (there is no TensorFlow route)"""
    from torch.utils.data.dataloader import default_collate
    import testDataset
    from miscc import load
    d = str(tmp_path / "data")
    shutil.copytree(DATA, d)
    os.remove(os.path.join(d, "test_acts_tf0.pickle"))
    cfg.TEST.USE_TF = 1
    assert load.load_acts_data(d, "test") is None and load.acts_filename("test") == "test_acts_tf0.pickle"
    ds = _dataset(cfg, 0, d)
    g = gold["acts_pass"]
    assert ds.acts_dict is None
    it = ds[0]
    assert len(it) == g["item_len"] == 2 and it[1] == g["key"]
    check_fp(it[0][0], g["img64"])
    p = testDataset.prepare_acts_data(default_collate([ds[0], ds[1]]))
    assert len(p) == g["prepared_len"] and list(p[1]) == g["keys"]
    check_fp(p[0][2], g["img256"])


def test_sample_filenames_reader(tmp_path):
    from miscc import load
    (tmp_path / "sample").mkdir()
    (tmp_path / "sample" / "filenames.txt").write_text("COCO_val2014_000000000042,3\r\nCOCO_val2014_000000000073,11\n")
    assert load.load_sample_filenames(str(tmp_path)) == (["COCO_val2014_000000000042", "COCO_val2014_000000000073"], [3, 11])
    assert load.load_sample_filenames(str(tmp_path / "nothing")) == ([], [])
    assert "NOT pinned" in load.load_sample_filenames.__doc__


# ---- (b) Frechet distance --------------------------------------------------------------------------------------------
def _fid_inputs(gold):
    out = []
    for seed, shift in zip(gold["seeds"]["acts"], (0.3, 0.35)):
        g = torch.Generator().manual_seed(seed)
        out.append(torch.clamp(shift + 0.4 * torch.randn(256, 64, generator=g), min=0).double().numpy())
    return out


def test_frechet_distance_matches_reference(gold):
    """same scipy / numpy call sequence in fp64 on both sides: relative 1e-9"""
    from miscc.utils import calculate_activation_statistics, calculate_frechet_distance
    a, b = _fid_inputs(gold)
    g = gold["fid"]
    mu1, s1 = calculate_activation_statistics(a)
    mu2, s2 = calculate_activation_statistics(b)
    for got, want in ((mu1, g["mu1"]), (s1, g["sigma1"]), (mu2, g["mu2"]), (s2, g["sigma2"])):
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    fid = calculate_frechet_distance(mu1, s1, mu2, s2)
    assert abs(fid - g["fid"]) <= 1e-9 * abs(g["fid"])
    assert abs(calculate_frechet_distance(mu1, s1, mu1, s1)) < 1e-6
    with pytest.raises(ValueError):
        calculate_frechet_distance(mu1, s1, mu2[:-1], s2)


def test_frechet_distance_singular_product_takes_the_eps_route(capsys, monkeypatch):
    """a non-finite first square root is announced and redone on (sigma1 + eps I)(sigma2 + eps I); the first sqrtm is
    made non-finite here, because scipy may well return finite values for a rank-deficient product"""
    from scipy import linalg
    from miscc.utils import calculate_activation_statistics, calculate_frechet_distance
    g = torch.Generator().manual_seed(1)
    a = torch.randn(6, 32, generator=g).double().numpy()
    b = torch.randn(6, 32, generator=g).double().numpy() + 0.5
    (mu1, s1), (mu2, s2) = calculate_activation_statistics(a), calculate_activation_statistics(b)
    real_sqrtm, seen = linalg.sqrtm, []

    def sqrtm(m, **kw):
        seen.append(np.array(m))
        if len(seen) == 1:
            return np.full_like(m, np.nan), np.inf
        return real_sqrtm(m, **kw)

    monkeypatch.setattr(linalg, "sqrtm", sqrtm)
    eps = 1e-3
    d = calculate_frechet_distance(mu1, s1, mu2, s2, eps=eps)
    assert len(seen) == 2 and "0.001" in capsys.readouterr().out
    eye = np.eye(32) * eps
    assert np.array_equal(seen[0], s1.dot(s2)) and np.array_equal(seen[1], (s1 + eye).dot(s2 + eye))
    root = real_sqrtm(seen[1])
    want = (mu1 - mu2).dot(mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root.real)
    assert np.isfinite(d) and d > 0 and abs(d - want) <= 1e-9 * abs(want)


def test_frechet_distance_rejects_a_complex_root(monkeypatch):
    from scipy import linalg
    from miscc.utils import calculate_frechet_distance
    monkeypatch.setattr(linalg, "sqrtm", lambda m, **kw: (np.eye(4) * (1 + 0.5j), 0.0))
    with pytest.raises(ValueError):
        calculate_frechet_distance(np.zeros(4), np.eye(4), np.zeros(4), np.eye(4))
    monkeypatch.setattr(linalg, "sqrtm", lambda m, **kw: (np.eye(4) * (1 + 1e-5j), 0.0))
    assert abs(calculate_frechet_distance(np.zeros(4), np.eye(4), np.zeros(4), np.eye(4))) < 1e-12


# ---- (c) R-precision pool --------------------------------------------------------------------------------------------
def _pool_inputs(gold, P=100, nef=256, L=12):
    g = torch.Generator().manual_seed(gold["seeds"]["pool"])
    base = torch.randn(P, nef, generator=g)
    regions = 0.5 * torch.randn(P, nef, 17, 17, generator=g) + base.view(P, nef, 1, 1) * \
        (torch.rand(P, 1, 17, 17, generator=g) < 0.3).float()
    words = 0.7 * torch.randn(P, nef, L, generator=g) + base.view(P, nef, 1)
    cap_lens = torch.sort(torch.randint(3, L + 1, (P,), generator=g), descending=True)[0]
    cap_lens[0] = L
    codes = base + 0.8 * torch.randn(P, nef, generator=g)
    sents = base + 0.8 * torch.randn(P, nef, generator=g)
    class_ids = torch.randint(0, 60, (P,), generator=g).numpy()
    return regions, codes, words, sents, class_ids, cap_lens


def test_rprecision_pool_matches_reference(cfg, gold, monkeypatch):
    import cpu_ops_shim
    cpu_ops_shim.install(monkeypatch)
    import evaluator as E
    sink = record_similarities(monkeypatch)
    regions, codes, words, sents, class_ids, cap_lens = _pool_inputs(gold)
    pool = E.RPrecisionPool(100)
    for r in range(0, 100, 20):                                              # five batches of 20 fill the pool ...
        assert pool.step(regions[r:r + 20], codes[r:r + 20], words[r:r + 20, :, :int(cap_lens[r])], sents[r:r + 20],
                         class_ids[r:r + 20], cap_lens[r:r + 20]) is None
    w_accu, s_accu = pool.step(regions[:20], codes[:20], words[:20], sents[:20], class_ids[:20], cap_lens[:20])
    g = gold["pool"]
    assert len(sink) == 4
    compare_pool(sink[0], g["w_sims"], w_accu, g["w_accu"], what="words")
    compare_pool(sink[2], g["s_sims"], s_accu, g["s_accu"], what="sentences")
    assert pool.w_accuracy == [w_accu] and pool.s_accuracy == [s_accu] and pool.rp_count == 0


# ---- pool bookkeeping ------------------------------------------------------------------------------------------------
def test_pool_bookkeeping_counts(cfg, monkeypatch):
    """batches of 3 into a pool of 4: two batches are collected (6 >= 4), the third triggers the evaluation over the
    first 4 rows and is added to no pool, the fourth opens the next pool"""
    import evaluator as E
    calls = []

    def words_stub(regions, words, labels, cap_lens, class_ids, P, **kw):
        calls.append(("w", regions.clone(), words.clone(), labels.clone(), cap_lens.clone(), np.array(class_ids), P, kw))
        return None, None, None, 50.0

    def sent_stub(codes, sents, labels, class_ids, P, **kw):
        calls.append(("s", codes.clone(), sents.clone(), labels.clone(), np.array(class_ids), P, kw))
        return None, None, 25.0
    monkeypatch.setattr(E, "words_loss", words_stub)
    monkeypatch.setattr(E, "sent_loss", sent_stub)
    nef = 8
    lens = [[5, 3, 2], [9, 4, 4], [12, 12, 1], [7, 6, 5]]

    def batch(b):
        ln = torch.tensor(lens[b])
        tag = float(b + 1)
        return (torch.full((3, nef, 17, 17), tag), torch.full((3, nef), tag), torch.full((3, nef, lens[b][0]), tag),
                torch.full((3, nef), tag), np.array([10 * b, 10 * b + 1, 10 * b + 2]), ln)
    pool = E.RPrecisionPool(4)
    assert pool.step(*batch(0)) is None and pool.rp_count == 3
    assert pool.step(*batch(1)) is None and pool.rp_count == 6
    assert pool.step(*batch(2)) == (50.0, 25.0)
    assert pool.rp_count == 0 and pool.regions == [] and len(calls) == 2
    _, regions, words, labels, cap_lens, class_ids, P, kw = calls[0]
    assert P == 4 and regions.shape == (4, nef, 17, 17) and labels.tolist() == [0, 1, 2, 3]
    assert cap_lens.tolist() == [5, 3, 2, 9] and class_ids.tolist() == [0, 1, 2, 10]
    assert regions[:, 0, 0, 0].tolist() == [1.0, 1.0, 1.0, 2.0]                 # truncated: one row of the second batch
    assert words.shape == (4, nef, 9)                                           # padded to the pool's longest caption
    assert float(words[:3, :, :5].min()) == 1.0 and float(words[:3, :, 5:].abs().max()) == 0.0
    assert float(words[3].min()) == 2.0
    assert kw == {"is_training": False, "need_att_maps": False}
    _, codes, sents, labels, class_ids, P, kw = calls[1]
    assert codes.shape == (4, nef) and sents[:, 0].tolist() == [1.0, 1.0, 1.0, 2.0] and kw == {"is_training": False}
    assert not any(float(c[1].max()) == 3.0 for c in calls)                     # the triggering batch is in no pool
    assert pool.step(*batch(3)) is None and pool.rp_count == 3
    assert float(pool.regions[0].max()) == 4.0
    assert pool.w_accuracy == [50.0] and pool.s_accuracy == [25.0]


def test_pool_uses_the_labels_it_is_given(cfg, monkeypatch):
    """the evaluator builds the match labels once (`prepare_labels`) and the pool hands that tensor to both losses"""
    import evaluator as E
    seen = []
    monkeypatch.setattr(E, "words_loss", lambda r, w, labels, *a, **kw: (seen.append(labels), (None, None, None, 1.0))[1])
    monkeypatch.setattr(E, "sent_loss", lambda c, s, labels, *a, **kw: (seen.append(labels), (None, None, 1.0))[1])
    cfg.TEST.RP_POOL_SIZE = 2
    ev = E.condGANEvaluator('', None, type("DS", (), {"cats_index_dict": {}})(), device=torch.device("cpu"))
    labels = ev.prepare_labels()
    assert labels.tolist() == [0, 1]
    pool = E.RPrecisionPool(2, labels)
    one = (torch.ones(2, 4, 17, 17), torch.ones(2, 4), torch.ones(2, 4, 3), torch.ones(2, 4), np.array([0, 1]),
           torch.tensor([3, 2]))
    assert pool.step(*one) is None and pool.step(*one) == (1.0, 1.0)
    assert len(seen) == 2 and seen[0] is labels and seen[1] is labels


# ---- activation file -------------------------------------------------------------------------------------------------
class _StubFid(torch.nn.Module):
    def forward(self, x):
        b = x.size(0)
        feat = x.mean(dim=(2, 3))                                               # [B, 3]: depends on the image
        return [feat.repeat(1, 683)[:, :2048].reshape(b, 2048, 1, 1)]


def test_dump_fid_acts_file_format(cfg, tmp_path):
    import evaluator as E
    from miscc import load
    d = str(tmp_path / "data")
    shutil.copytree(DATA, d)
    os.remove(os.path.join(d, "test_acts_tf0.pickle"))
    cfg.TEST.USE_TF = 0
    ds = _dataset(cfg, 0, d)
    ds.inception_model, ds.inception_model_fid = torch.nn.Identity(), _StubFid()
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    ev = E.condGANEvaluator("", loader, ds, device=torch.device("cpu"))
    ev.dump_fid_acts(d, "test")
    path = os.path.join(d, "test_acts_tf0.pickle")
    raw = open(path, "rb").read()
    assert raw[:2] == b"\x80\x02"                                               # pickle protocol 2
    x = pickle.loads(raw)
    assert isinstance(x, list) and len(x) == 1 and isinstance(x[0], dict)
    assert list(x[0].keys()) == list(ds.filenames)
    for key, v in x[0].items():
        assert isinstance(v, np.ndarray) and v.shape == (2048,) and v.dtype == np.float64
    want = ds[0][0][2].mean(dim=(1, 2)).double().numpy()
    assert np.allclose(x[0][ds.filenames[0]][:3], want, atol=1e-6)
    assert set(load.load_acts_data(d, "test").keys()) == set(ds.filenames)
    before = os.path.getmtime(path)
    ev.dump_fid_acts(d, "test")                                                 # an existing file is left alone
    assert os.path.getmtime(path) == before


def test_reference_activation_file_reads_back(cfg):
    """the file the REFERENCE wrote (committed with the tiny data set) through the product reader"""
    from miscc import load
    acts = load.load_acts_data(DATA, "test")
    names = load.load_filenames(DATA, "test")
    assert list(acts.keys()) == list(names)
    assert all(v.shape == (2048,) and v.dtype == np.float64 and np.isfinite(v).all() for v in acts.values())


# ---- CLI -------------------------------------------------------------------------------------------------------------
def test_build_evaluation_and_main(cfg, tmp_path):
    import main
    import testDataset
    import evaluator as E
    args = main.parse_args(["--gpu", "0", "--data_dir", DATA, "--BATCH_SIZE", "2", "--output_dir", str(tmp_path),
                            "--USE_GT_BOX_SEG", "0", "--TEST_IMG_NUM", "7", "--NET_G", "g.pth"])
    main.apply_args(args)
    assert cfg.TEST.USE_GT_BOX_SEG == 0 and cfg.TEST.TEST_IMG_NUM == 7 and not cfg.TRAIN.FLAG
    dataset, loader, algo = main.build_evaluation(args, 0, 1, torch.device("cpu"))
    assert isinstance(dataset, testDataset.TestDataset) and isinstance(algo, E.condGANEvaluator)
    assert list(dataset.filenames) == ["COCO_val2014_%012d" % i for i in (42, 73, 74, 133, 136, 139)]   # split 'test'
    assert loader.drop_last and loader.batch_size == 2
    assert isinstance(loader.sampler, torch.utils.data.SequentialSampler)                                # shuffle=False
    assert algo.num_batches == 3 and os.path.isdir(algo.score_dir) and os.path.isdir(algo.image_dir)
    assert hasattr(algo, "evaluate") and hasattr(algo, "dump_fid_acts") and algo.prepare_labels is not None
    with pytest.raises(SystemExit) as e:
        main.build_evaluation(args, 0, 2, torch.device("cpu"))
    assert "single GPU" in str(e.value)
    # defaults leave the configuration alone
    assert main.parse_args([]).USE_GT_BOX_SEG is None and main.parse_args([]).TEST_IMG_NUM is None
    # without --FLAG main() heads for the evaluation: on a box without a GPU it stops at the device check, not at the
    # old "outside the hot path" exit
    with pytest.raises(SystemExit) as e:
        main.main(["--gpu", "-1", "--data_dir", DATA])
    assert "outside the hot path" not in str(e.value) and "no CPU path" in str(e.value)


# ---- C-ABI -----------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_listed_and_exported():
    from objgan_hip import _lib
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["objgan_bilinear_halfpixel_forward"]) == 11
    path = _lib.lib_path()
    assert os.path.exists(path), "build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= exported
