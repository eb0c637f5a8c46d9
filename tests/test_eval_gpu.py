"""Evaluation mode on the MI355X: the two kernels of csrc/eval_stats.hip (half-pixel bilinear resize + affine, fp64
moment accumulation), the FID feature network built on them, and `condGANEvaluator.evaluate` end to end over the tiny
evaluation data set against what the unmodified reference computed on the CPU (tests/golden/eval_ref.pt)."""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2, note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

FID_SCALE = [0.5 * s / 0.5 for s in (0.229, 0.224, 0.225)]
FID_SHIFT = [0.5 * s / 0.5 + (m - 0.5) / 0.5 for s, m in zip((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))]


# ---- bilinear_resize_halfpixel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("S", [64, 128, 256, 512])
def test_bilinear_halfpixel_matches_torch(dev, S, N, affine):
    """F.interpolate(align_corners=False) + per-channel affine on the CPU in fp32.  Inputs in [-1, 1] keep |y| < 4;
    three linear interpolations and one affine are at most eight fp32 roundings, 8 * ulp(4) / 2 = 1.9e-6, doubled for the
    rounding of the source coordinate: 4e-6 absolute."""
    from objgan_hip import ops
    g = torch.Generator().manual_seed(S * 100 + N)
    x = torch.rand(N, 3, S, S, generator=g) * 2 - 1
    want = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    scale = shift = None
    if affine:
        scale, shift = torch.tensor(FID_SCALE), torch.tensor(FID_SHIFT)
        want = want * scale.view(1, 3, 1, 1) + shift.view(1, 3, 1, 1)
    got = ops.bilinear_resize_halfpixel(x.to(dev), 299, 299, None if scale is None else scale.to(dev),
                                        None if shift is None else shift.to(dev)).cpu()
    assert got.shape == want.shape and float(want.abs().max()) < 4
    err = float((got - want).abs().max())
    note("bilinear_resize_halfpixel %d->299 N=%d affine=%d max abs err" % (S, N, affine), "%.3e" % err)
    assert err <= 4e-6, err


def test_bilinear_halfpixel_rectangular_and_downscale_edges(dev):
    """non-square sizes, down- and upscaling, odd sizes: the clamps at both borders"""
    from objgan_hip import ops
    g = torch.Generator().manual_seed(3)
    for (h, w, oh, ow) in [(5, 9, 13, 4), (37, 21, 8, 50), (1, 7, 3, 3), (300, 299, 299, 299)]:
        x = torch.rand(2, 3, h, w, generator=g) * 2 - 1
        want = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
        got = ops.bilinear_resize_halfpixel(x.to(dev), oh, ow).cpu()
        assert float((got - want).abs().max()) <= 4e-6, (h, w, oh, ow)
    with pytest.raises(Exception):
        ops.bilinear_resize_halfpixel(torch.zeros(1, 3, 4, 4), 8, 8)            # CPU tensor: no fallback
    with pytest.raises(Exception):
        ops.bilinear_resize_halfpixel(torch.zeros(1, 3, 4, 4, device=dev), 8, 8, scale=torch.ones(3, device=dev))


# ---- MomentAccumulator -----------------------------------------------------------------------------------------------
def _acts(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.clamp(0.3 + 0.4 * torch.randn(N, D, generator=g), min=0)       # pool3 activations are non-negative


def _accumulate(dev, x, chunk):
    from objgan_hip import ops
    acc = ops.MomentAccumulator(x.shape[1], dev)
    xd = x.to(dev)
    for r in range(0, x.shape[0], chunk):
        acc.add(xd[r:r + chunk])
    assert acc.count == x.shape[0]
    mu, sigma = acc.finalize()
    torch.cuda.synchronize()
    return mu.cpu(), sigma.cpu(), acc


@pytest.mark.parametrize("N,D", [(64, 96), (4096, 128), (512, 2048)])
def test_moment_accumulator_matches_numpy(dev, N, D):
    """np.mean / np.cov in fp64.  Bound per element: one-pass recursive summation of N exactly representable products,
    |d sigma_ij| <= 4 N 2^-53 (mean_r |x_ri x_rj| + |mu_i mu_j|) N / (N - 1)."""
    x = _acts(N, D, 5 + N)
    mu, sigma, _ = _accumulate(dev, x, 128)
    x64 = x.double().numpy()
    mu_ref, sigma_ref = np.mean(x64, axis=0), np.cov(x64, rowvar=False)
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64 and sigma.shape == (D, D)
    e_mu = np.abs(mu.numpy() - mu_ref).max()
    assert e_mu <= 4 * N * 2.0 ** -53 * np.abs(x64).mean(0).max()
    bound = 4 * N * 2.0 ** -53 * ((np.abs(x64).T @ np.abs(x64)) / N + np.abs(np.outer(mu_ref, mu_ref))) * N / (N - 1)
    ratio = float((np.abs(sigma.numpy() - sigma_ref) / bound).max())
    note("MomentAccumulator N=%d D=%d: worst |d sigma| / bound, |d mu|" % (N, D), "%.3e, %.3e" % (ratio, e_mu))
    assert ratio <= 1.0, ratio
    assert torch.equal(sigma, sigma.t())                                         # exactly symmetric


def test_moment_accumulator_is_reproducible_and_split_independent(dev):
    x = _acts(128, 2048, 77)
    mu_a, sig_a, acc_a = _accumulate(dev, x, 128)
    mu_b, sig_b, acc_b = _accumulate(dev, x, 128)
    assert torch.equal(mu_a, mu_b) and torch.equal(sig_a, sig_b)                 # two runs: bit-identical
    mu_c, sig_c, acc_c = _accumulate(dev, x, 16)                                 # one 128-row call == eight 16-row calls
    assert torch.equal(acc_a.sum, acc_c.sum) and torch.equal(acc_a.outer, acc_c.outer)
    assert torch.equal(mu_a, mu_c) and torch.equal(sig_a, sig_c)
    mu_d, sig_d, acc_d = _accumulate(dev, x, 50)                                 # ragged cuts (50 + 50 + 28) as well
    assert torch.equal(acc_a.outer, acc_d.outer) and torch.equal(sig_a, sig_d)
    assert float(torch.tril(acc_a.outer, -1).abs().max()) == 0.0                # only the upper triangle is touched


def test_moment_accumulator_rejects_bad_input(dev):
    from objgan_hip import ops
    acc = ops.MomentAccumulator(96, dev)
    with pytest.raises(Exception):
        acc.add(torch.zeros(4, 96))                                              # CPU tensor
    with pytest.raises(Exception):
        acc.add(torch.zeros(4, 64, device=dev))
    acc.add(torch.ones(1, 96, device=dev))
    with pytest.raises(Exception):
        acc.finalize()                                                           # one row: no covariance


# ---- INCEPTION_V3_FID ------------------------------------------------------------------------------------------------
def test_inception_v3_fid_matches_fp64_restatement(dev):
    """The FID network on the kernels against an fp64 restatement on the CPU: oracle.torch_encoders blocks, half-pixel
    F.interpolate, the reference's two affines unfolded (reference model.py:433-441).  One trunk serves INCEPTION_V3,
    CNN_ENCODER and INCEPTION_V3_FID.  Bound: the forward bound of test_kernels_gpu.py::test_inception_encoder_gpu_matches_cpu
    for the same trunk (1e-4 relative L2)."""
    import encoders
    from oracle import torch_encoders as te
    net = encoders.seeded_init_(encoders.inception_v3(), 3)
    mon = encoders.INCEPTION_V3(net).eval()
    enc = encoders.CNN_ENCODER(256, net).eval()
    fid = encoders.INCEPTION_V3_FID([encoders.INCEPTION_V3_FID.BLOCK_INDEX_BY_DIM[2048]], trunk=net).eval()
    assert fid.blocks[3][2] is net.Mixed_7c and enc.Mixed_7c is net.Mixed_7c and mon.model is net
    want_keys = {"blocks.%d.%d.%s" % (b, i, k[len(n) + 1:]) for b, names in enumerate(encoders.FID_BLOCKS)
                 for i, n in enumerate(names) for k in net.state_dict() if k.startswith(n + ".")}
    assert set(fid.state_dict().keys()) == want_keys                              # the reference's key set
    twin = te.cpu_twin(net).double()
    g = torch.Generator().manual_seed(41)
    x = torch.tanh(torch.randn(2, 3, 256, 256, generator=g))
    with torch.no_grad():
        r = F.interpolate(x.double(), size=(299, 299), mode="bilinear", align_corners=False)
        r = r * 0.5 + 0.5
        for c, (s, m) in enumerate(zip((0.229, 0.224, 0.225), (0.485, 0.456, 0.406))):
            r[:, c] = r[:, c] * (s / 0.5) + (m - 0.5) / 0.5
        want = te.inception_trunk(twin, r)
        got = fid.to(dev)(x.to(dev))
    assert isinstance(got, list) and len(got) == 1 and got[0].shape == (2, 2048, 1, 1)
    e = rel_l2(got[0].flatten(1), want)
    note("INCEPTION_V3_FID gfx950 vs fp64 restatement: pool3 rel-L2", "%.3e" % e)
    assert e < 1e-4, e
    from miscc.utils import get_activations
    acts = get_activations(torch.cat([x, x, x[:1]]).to(dev), fid, 2)             # whole batches only: 5 -> 4 rows
    assert acts.is_cuda and acts.shape == (4, 2048) and torch.equal(acts[:2], acts[2:])
    for dims in (64, 192, 768):
        with pytest.raises(NotImplementedError):
            encoders.INCEPTION_V3_FID([encoders.INCEPTION_V3_FID.BLOCK_INDEX_BY_DIM[dims]], trunk=net)


# ---- evaluate() end to end -------------------------------------------------------------------------------------------
# Relative L2 of the continuous intermediates against the reference's CPU run (golden (d)): four times the value of the
# first green run on the MI355X (LAB.md section "evaluation"), never above the project's 1e-3 bound for outputs.
E2E_OBSERVED = {"fake_acts": 7.492e-07, "pred": 1.507e-06, "w_sims": 9.532e-08, "s_sims": 8.784e-07, "real_acts": 4.117e-07}
E2E_BOUNDS = {k: min(4.0 * v, 1e-3) for k, v in E2E_OBSERVED.items()}


@pytest.fixture
def eval_cfg():
    from miscc.config import cfg
    from eval_helpers import cfg_snapshot, cfg_restore
    saved = cfg_snapshot(cfg)
    yield cfg
    cfg_restore(cfg, saved)


def test_evaluate_end_to_end_matches_reference(dev, eval_cfg, tmp_path, monkeypatch):
    """`evaluate` over tests/golden/data_tiny_eval with the seeded checkpoints and the recorded noise of the reference run:
    scores.txt, six images, the activation pickle, the continuous intermediates and the nine scores."""
    import encoders
    import evaluator as E
    import model as M
    import testDataset
    from miscc import load
    from oracle import ref_harness as rh
    from eval_helpers import seeded_emb_, record_similarities, compare_pool
    gold = torch.load(os.path.join(GOLD, "eval_ref.pt"), weights_only=False)
    g, seeds = gold["e2e"], gold["seeds"]
    cfg = eval_cfg
    cfg.TREE.BRANCH_NUM = 3
    cfg.TEST.USE_GT_BOX_SEG, cfg.TEST.USE_TF, cfg.TEST.SAMPLE_VAL, cfg.TEST.SAVE_OPTIONS = 0, 0, False, 'IMAGE'
    cfg.TRAIN.BATCH_SIZE, cfg.TEST.RP_POOL_SIZE, cfg.TRAIN.DISPLAY_INTERVAL = 2, 4, 1
    cfg.TEST.TEST_IMG_NUM = 1000000
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(GOLD, "data_tiny_eval"), data)
    ref_acts = load.load_acts_data(data, "test")                       # written by the reference's dump_fid_acts
    os.remove(os.path.join(data, "test_acts_tf0.pickle"))
    ds = testDataset.TestDataset(data, "test", base_size=64)
    assert ds.acts_dict is None
    trunk = encoders.seeded_init_(encoders.inception_v3(), seeds["inception"])
    ds.text_encoder = rh.seeded_state_(M.RNN_ENCODER(ds.n_words, nhidden=256), seeds["text"])
    ds.image_encoder = seeded_emb_(encoders.CNN_ENCODER(256, trunk), seeds["emb"])
    ds.inception_model = encoders.INCEPTION_V3(trunk)
    ds.inception_model_fid = encoders.INCEPTION_V3_FID([3], trunk=trunk)
    cfg.TRAIN.NET_G = str(tmp_path / "netG.pth")
    torch.save(rh.seeded_state_(M.G_NET(ds.num_classes), seeds["G"]).state_dict(), cfg.TRAIN.NET_G)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)

    def run(tag):
        ev = E.condGANEvaluator(str(tmp_path / tag), loader, ds, device=dev)
        if ds.acts_dict is None:
            ev.dump_fid_acts(data, "test")
            ds.acts_dict = load.load_acts_data(data, "test")
        step = [0]

        def noise_fn(kind, shape):
            assert kind == 'img' and tuple(shape) == (2, cfg.GAN.Z_DIM)
            ev.netG.ca_net.fixed_eps = g["ca_eps"][step[0]].to(dev)
            z = g["noise_img"][step[0]].to(dev)
            step[0] += 1
            return z
        trace = []
        np.random.seed(seeds["items"])
        scores = ev.evaluate("test", ds.imsize, noise_fn=noise_fn, trace=trace)
        torch.cuda.synchronize()
        return ev, scores, trace

    sink = record_similarities(monkeypatch)
    ev, scores, trace = run("first")
    # files
    text = open(os.path.join(ev.score_dir, "scores.txt")).read()
    header, values = text.split("\n")
    assert header + "\n" == g["header"] == E.SCORES_HEADER
    vals = [float(v) for v in values.split(",")]
    assert len(vals) == 9 and all(np.isfinite(v) for v in vals)
    assert sorted(os.listdir(ev.image_dir)) == g["images_written"] and len(g["images_written"]) == 6
    raw = open(os.path.join(data, "test_acts_tf0.pickle"), "rb").read()
    x = pickle.loads(raw)
    assert raw[:2] == b"\x80\x02" and list(x[0].keys()) == list(ds.filenames)
    assert all(v.shape == (2048,) and v.dtype == np.float64 for v in x[0].values())
    got_real = torch.from_numpy(np.stack([x[0][k] for k in ds.filenames]))
    want_real = torch.from_numpy(np.stack([ref_acts[k] for k in ds.filenames]))
    obs = {"real_acts": rel_l2(got_real, want_real)}
    # continuous intermediates
    assert len(trace) == 3 and len(sink) == 4
    e_img = []
    for t, fp in zip(trace, g["fake_img"]):
        sample = t["fake_img"][..., ::fp["step"], ::fp["step"]]
        assert tuple(t["fake_img"].shape) == tuple(fp["shape"])
        e_img.append(rel_l2(sample, fp["sample"]))
    obs["fake_acts"] = rel_l2(torch.cat([t["fake_acts"] for t in trace]), torch.cat(g["fake_acts"]))
    obs["pred"] = rel_l2(torch.cat([torch.as_tensor(t["pred"]) for t in trace]), torch.cat(g["pred"]))
    fin = torch.isfinite(g["w_sims"])
    obs["w_sims"] = rel_l2(sink[0].cpu()[fin], g["w_sims"][fin])
    fin = torch.isfinite(g["s_sims"])
    obs["s_sims"] = rel_l2(sink[2].cpu()[fin], g["s_sims"][fin])
    note("evaluate() e2e vs reference: fake_imgs[-1] sample rel-L2 per batch", " ".join("%.3e" % e for e in e_img))
    for k in sorted(obs):
        note("evaluate() e2e vs reference: %s rel-L2 (asserted at %.1e)" % (k, E2E_BOUNDS[k]), "%.3e" % obs[k])
    note("evaluate() e2e scores got / reference", "%s / %s" % (vals, g["scores"]))
    assert max(e_img) < 1e-3, e_img                       # the generator bound of tests/test_modules_gpu.py (TOL)
    for k, e in obs.items():
        assert e <= E2E_BOUNDS[k], (k, e)
    # the nine scores: IS, NLPP and FID always, R-precision where the reference's rows have a clear best match
    want = g["scores"]
    for i in (0, 1, 2, 3, 8):
        assert abs(vals[i] - want[i]) <= 1e-2 * abs(want[i]), (i, vals[i], want[i])
    compare_pool(sink[0], g["w_sims"], vals[4], want[4], what="words", max_left_out=1.0)
    compare_pool(sink[2], g["s_sims"], vals[6], want[6], what="sentences", max_left_out=1.0)
    assert vals[5] == want[5] == 0.0 and vals[7] == want[7] == 0.0          # one pool: no spread
    # a second evaluation: bit-identical scores
    ev2, scores2, _ = run("second")
    assert open(os.path.join(ev2.score_dir, "scores.txt")).read() == text
    assert scores2 == scores
