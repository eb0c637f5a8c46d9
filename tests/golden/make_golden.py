"""Generate tests/golden/*.pt from the UNMODIFIED reference (run in the build container only):

    python tests/golden/make_golden.py [--shp | --rnn | --standalone]

Inputs are NOT stored: they come from obj-gan_amd/synth_batch.py (seeded, identical everywhere);
weights are NOT stored: they come from oracle.ref_harness.seeded_state_ (filled by state-dict key).
Only reference OUTPUTS (images, losses, gradient summaries) are stored, sub-sampled where large.
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "obj-gan_amd")]

from oracle import ref_harness as rh          # noqa: E402
import synth_batch                            # noqa: E402
from oracle import torch_encoders as encoders  # noqa: E402  (plain-PyTorch Inception-v3)

B = 2
SEEDS = dict(batch=1234, G=11, pat=21, shp=31, objss=41, objls=42, inception=51, enc_proj=52)


def grad_summary(module):
    return {k: (p.grad.norm().item() if p.grad is not None else 0.0) for k, p in module.named_parameters()}


def make_rnn_golden():
    """Reference RNN_ENCODER (model.py:85-179) on the synthetic captions -> tests/golden/rnn_encoder_ref.pt"""
    ref = rh.load_reference(branch_num=3, batch_size=4)
    b = synth_batch.make_batch(4, seed=SEEDS["batch"])
    enc = rh.seeded_state_(ref.model.RNN_ENCODER(1000, nhidden=256), 61, scale=None).eval()
    with torch.no_grad():
        words, sent = enc(b["captions"], b["cap_lens"], 12)
    torch.save({"seed": 61, "B": 4, "ntoken": 1000, "words_emb": words.clone(), "sent_emb": sent.clone()},
               os.path.join(HERE, "rnn_encoder_ref.pt"))
    print("rnn golden", tuple(words.shape), tuple(sent.shape), float(words.abs().mean()))


def make_shp_golden():
    """Reference SHP_G_NET (model.py:898-985) and form_hmaps (utils.py:524-584) on CPU ->
    tests/golden/shp_g_ref.pt.  The reference hard-codes .cuda() for the initial ConvLSTM state and
    cfg.CUDA in form_hmaps: both are neutralised for the run (Tensor.cuda -> identity, cfg.CUDA False)."""
    ref = rh.load_reference(branch_num=3, batch_size=2)
    nbf = 8
    net = rh.seeded_state_(ref.model.SHP_G_NET(nbf), 72).eval()
    z, fwd, bwd, fmaps, rois, num = synth_batch.make_shape_inputs(nbf=nbf)
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            fake = net(z, fwd, bwd, fmaps)
            ref.cfg.CUDA = False
            hm, bt, fmbt = ref.utils.form_hmaps(fake.squeeze(2).clone(), num, rois, [64, 128, 256], nbf)
    finally:
        torch.Tensor.cuda = orig_cuda

    def fp(t):
        t = t.double()
        return {"shape": tuple(t.shape), "sum": float(t.sum()), "sq": float((t * t).sum()),
                "sample": t[..., ::8, ::8].float().clone()}
    torch.save({"seed_inputs": 71, "seed_weights": 72, "nbf": nbf, "fake_hmaps": fake.clone(),
                "state_keys": {k: tuple(v.shape) for k, v in net.state_dict().items()},
                "gen_hmaps": [fp(t) for t in hm], "gen_bt_masks": [fp(t) for t in bt], "gen_fm_bt_masks": fmbt.clone()},
               os.path.join(HERE, "shp_g_ref.pt"))
    print("shp golden", tuple(fake.shape), float(fake.mean()), [tuple(t.shape) for t in hm])


def main():
    torch.set_num_threads(8)
    ref = rh.load_reference(branch_num=3, batch_size=B)
    b = synth_batch.make_batch(B, seed=SEEDS["batch"])
    M, Ls, U = ref.model, ref.losses, ref.utils
    G = rh.seeded_state_(M.G_NET(80), SEEDS["G"]).train()
    pats = [rh.seeded_state_(c(), SEEDS["pat"] + i).train() for i, c in enumerate((M.PAT_D_NET64, M.PAT_D_NET128, M.PAT_D_NET256))]
    shps = [rh.seeded_state_(c(80), SEEDS["shp"] + i).train() for i, c in enumerate((M.SHP_D_NET64, M.SHP_D_NET128, M.SHP_D_NET256))]
    objss = rh.seeded_state_(M.OBJ_SS_D_NET(80), SEEDS["objss"]).train()
    objls = rh.seeded_state_(M.OBJ_LS_D_NET(80), SEEDS["objls"]).train()
    enc = encoders.CNN_ENCODER(256, encoders.seeded_init_(encoders.inception_v3(), SEEDS["inception"]))
    rh.seeded_state_(enc.emb_features, SEEDS["enc_proj"]); rh.seeded_state_(enc.emb_cnn_code, SEEDS["enc_proj"] + 1)
    enc.eval()

    out = {"seeds": SEEDS, "B": B}
    cl = U.form_clabels_feat(b["clabels_emb"], b["rois"][0], b["num_rois"])
    glb = int(b["num_rois"].max())
    # CA_NET draws eps from the global generator (model.py:472-478): inject the batch's ca_eps
    orig = M.CA_NET.reparametrize
    M.CA_NET.reparametrize = lambda self, mu, logvar: b["ca_eps"] * (logvar * 0.5).exp() + mu
    fake, bt_codes, atts, bt_atts, mu, logvar = G(b["noise"], b["sent_emb"], b["words_embs"],
                                                 b["glove_words_embs"], cl, b["mask"], b["hmaps"], b["rois"],
                                                 b["fm_rois"], b["num_rois"], b["bt_masks"], b["fm_bt_masks"], glb)
    M.CA_NET.reparametrize = orig
    out["fake64"] = fake[0].detach().clone()
    out["fake128"] = fake[1].detach().clone()
    out["fake256_s2"] = fake[2].detach()[:, :, ::2, ::2].clone()
    out["bt_c_codes"] = [c.detach().clone() for c in bt_codes]
    out["att128_s4"] = atts[1].detach()[:, :, ::4, ::4].clone()
    out["bt_att64_s2"] = bt_atts[0].detach()[:, :, ::2, ::2].clone()
    out["mu"], out["logvar"] = mu.detach().clone(), logvar.detach().clone()

    bt = [c.detach() for c in bt_codes]
    # discriminator losses + gradient summaries (python `random` seeded before each permute_seg user)
    for i in range(3):
        e = Ls.patD_loss(pats[i], b["imgs"][i], fake[i], b["sent_emb"])
        e.backward()
        out["errPatD%d" % i] = e.item()
        out["gradPatD%d" % i] = grad_summary(pats[i])
    for i in range(3):
        random.seed(100 + i)
        e = Ls.shpD_loss(shps[i], b["imgs"][i], fake[i], b["hmaps"][i], b["rois"][i], b["num_rois"])
        e.backward()
        out["errShpD%d" % i] = e.item()
        out["gradShpD%d" % i] = grad_summary(shps[i])
    random.seed(200)
    e = Ls.objD_loss(objss, b["imgs"][-1], fake[-1], b["hmaps"][-1], b["clabels_emb"], bt[-1], b["rois"][0], b["num_rois"])
    e.backward(); out["errObjSSD"] = e.item(); out["gradObjSSD"] = grad_summary(objss)
    random.seed(201)
    e = Ls.objD_loss(objls, b["imgs"][-1], fake[-1], b["hmaps"][-1], b["clabels_emb"], bt[-1], b["fm_rois"], b["num_rois"], is_large_scale=True)
    e.backward(); out["errObjLSD"] = e.item(); out["gradObjLSD"] = grad_summary(objls)

    # generator loss (+KL) and its gradient through everything
    for net in pats + shps + [objss, objls]:
        net.zero_grad()
    labels = torch.arange(B)
    total, logs = Ls.G_loss(pats, shps, objss, objls, enc, fake, b["hmaps"], b["words_embs"], b["sent_emb"],
                            b["clabels_emb"], bt[-1], labels, b["cap_lens"], b["class_ids"], b["rois"][0],
                            b["fm_rois"], b["num_rois"])
    kl = Ls.KL_loss(mu, logvar)
    (total + kl).backward(retain_graph=True)
    out["errG"] = (total + kl).item(); out["kl"] = kl.item(); out["G_logs"] = logs
    out["gradG"] = grad_summary(G)
    out["gradG_ca_fc_w"] = G.ca_net.fc.weight.grad.clone()
    out["gradG_att_ctx_w"] = G.h_net3_main.att.conv_context.weight.grad.clone()
    out["gradG_img3_w"] = G.img_net3.img[0].weight.grad.clone()
    # The same with a CONSTANT image encoder (no gradient through Inception).  In fp32 the DAMSM
    # input-gradient is ill-conditioned (a 1e-7 relative perturbation of the fake image moves it by
    # 1.6e-3 on the reference's own CPU path), so gradient parity of the generator is pinned on this
    # variant; the DAMSM branch is pinned separately from fixed region features.
    G.zero_grad()
    regions_c, code_c = enc(fake[2].detach())
    const_enc = lambda x: (regions_c.detach(), code_c.detach())     # noqa: E731
    total2, _ = Ls.G_loss(pats, shps, objss, objls, const_enc, fake, b["hmaps"], b["words_embs"], b["sent_emb"],
                          b["clabels_emb"], bt[-1], labels, b["cap_lens"], b["class_ids"], b["rois"][0],
                          b["fm_rois"], b["num_rois"])
    (total2 + Ls.KL_loss(mu, logvar)).backward()
    out["errG_constenc"] = (total2 + kl).item()
    out["gradG_constenc"] = grad_summary(G)
    out["gradG_constenc_img3_w"] = G.img_net3.img[0].weight.grad.clone()
    out["gradG_constenc_att_ctx_w"] = G.h_net3_main.att.conv_context.weight.grad.clone()
    out["gradG_constenc_ca_fc_w"] = G.ca_net.fc.weight.grad.clone()
    out["gradG_constenc_res_w"] = G.h_net2_main.residual[1].block[1].weight.grad[::8, ::8].clone()
    out["regions_s"] = regions_c.detach()[:, ::8].clone()
    # DAMSM pieces on their own
    regions, code = enc(fake[2].detach())
    w0, w1, _, _ = Ls.words_loss(regions, b["words_embs"], labels, b["cap_lens"], b["class_ids"], B)
    s0, s1, _ = Ls.sent_loss(code, b["sent_emb"], labels, b["class_ids"], B)
    out["w_loss"], out["s_loss"] = (w0 + w1).item(), (s0 + s1).item()
    torch.save(out, os.path.join(HERE, "step_b2.pt"))
    print({k: v for k, v in out.items() if isinstance(v, float)})
    print("saved", os.path.getsize(os.path.join(HERE, "step_b2.pt")) / 1e6, "MB")

    # ROIAlign golden vectors from the reference's own C loop
    from oracle import roi
    rng = np.random.RandomState(5)
    feat = rng.randn(2, 6, 32, 32).astype(np.float32)
    rois = np.zeros((20, 5), np.float32)
    rois[:, 0] = np.repeat([0, 1], 10)
    xy = rng.uniform(-8, 300, (20, 2)); wh = rng.uniform(0, 300, (20, 2))
    rois[:, 1:3] = xy; rois[:, 3:5] = xy + wh
    rois[::4, 1:] = np.round(rois[::4, 1:])
    np.savez_compressed(os.path.join(HERE, "roi_align_ref.npz"), feat=feat, rois=rois,
                        out=roi.reference_forward(feat, rois, 6, 6, 1 / 16.0))


def make_standalone_golden():
    """What the CPU tests compared against the reference tree itself -> tests/golden/roi_align_ref_trials.npz (the
    reference's ROIAlignForwardCpu on twelve seeded trials, inputs included) and tests/golden/reference_host_ref.json
    (state-dict key -> shape of the five trained networks; the Inception-score helpers on seeded class posteriors)."""
    import json
    from oracle import roi
    roi.build()
    rng = np.random.RandomState(3)
    arrs = {}
    for trial in range(12):
        H, W = rng.randint(4, 40), rng.randint(4, 40)
        feat = rng.randn(3, 4, H, W).astype(np.float32)
        rois = np.zeros((24, 5), np.float32)
        rois[:, 0] = rng.randint(0, 3, 24)
        sc = [1 / 16., 1.0, 0.5][trial % 3]
        xy = rng.uniform(-5, W / sc, (24, 2)); wh = rng.uniform(0, W / sc, (24, 2))
        rois[:, 1:3] = xy; rois[:, 3:5] = xy + wh
        if trial % 2 == 0:
            rois[:, 1:] = np.round(rois[:, 1:])
        ah, aw = [(6, 6), (2, 2), (7, 5)][trial % 3]
        arrs.update({"feat%d" % trial: feat, "rois%d" % trial: rois, "pooled%d" % trial: np.array([ah, aw]),
                     "scale%d" % trial: np.float32(sc), "out%d" % trial: roi.reference_forward(feat, rois, ah, aw, sc)})
    np.savez_compressed(os.path.join(HERE, "roi_align_ref_trials.npz"), **arrs)

    ref = rh.load_reference(3, 2)
    M = ref.model
    nets = {"G_NET": M.G_NET(80), "PAT_D_NET64": M.PAT_D_NET64(), "SHP_D_NET256": M.SHP_D_NET256(80),
            "OBJ_SS_D_NET": M.OBJ_SS_D_NET(80), "OBJ_LS_D_NET": M.OBJ_LS_D_NET(80)}
    logits = np.random.RandomState(0).randn(37, 11)
    p = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    out = {"state_dict_shapes": {n: {k: list(v.shape) for k, v in m.state_dict().items()} for n, m in nets.items()},
           "inception_score": {"posteriors": "softmax(RandomState(0).randn(37, 11)), 4 splits",
                               "compute_inception_score": [float(v) for v in ref.utils.compute_inception_score(p, 4)],
                               "negative_log_posterior_probability":
                                   [float(v) for v in ref.utils.negative_log_posterior_probability(p, 4)]}}
    with open(os.path.join(HERE, "reference_host_ref.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--shp" in sys.argv:
        make_shp_golden()
    elif "--rnn" in sys.argv:
        make_rnn_golden()
    elif "--standalone" in sys.argv:
        make_standalone_golden()
    else:
        main()
        make_rnn_golden()
        make_standalone_golden()
