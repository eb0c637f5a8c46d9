"""Adversarial losses of the shape generator's training (reference shape_generation/miscc/losses.py:11-164).

Same three entry points.  Differences, all results-preserving: the mask and the one-hot box maps go into the
discriminators as the two parts of their first convolution's input (no concatenated tensor), BCE against constant labels
is one fused kernel (torch's log clamp at -100), the maxima over the box axis are `ops.box_max`.  Padded box slots are
NOT masked, as in the reference: an image with fewer boxes than the batch maximum still contributes its slots to the
instance loss and to the maxima.  The perceptual term runs the frozen VGG-19-bn (`model.VGG.perceptual`) on the pooled fake
and real masks in one batch and adds PCP_LAMBDA times the sum of the 19 per-tap L1 means; a non-zero PCP_LAMBDA
without the network, and a network with PCP_LAMBDA = 0, are refused.
"""
from miscc.config import cfg
from objgan_hip import ops
from objgan_hip._lib import ObjganHipError


def _smooth(name, default):
    return float(cfg.TRAIN.SMOOTH.get(name, default))


def check_pcp_lambda(value, weights_path=None):
    """A non-zero PCP_LAMBDA needs the frozen VGG-19-bn: `weights_path` (the torchvision file) must exist.  Called before
    any work, so that a run never silently trains on a loss without the term."""
    import os
    if float(value) != 0.0 and (weights_path is None or not os.path.isfile(weights_path)):
        raise ObjganHipError("the perceptual (VGG-19-bn) term of the shape generator's loss is not built without its "
                             "weights file %s: PCP_LAMBDA = %g is refused; put torchvision's vgg19_bn-c79401a0.pth there "
                             "or run with --PCP_LAMBDA 0" % (weights_path if weights_path is not None else
                                                             "<DATA_DIR>/pretrained/vgg19_bn-c79401a0.pth", float(value)))


def _ins_probs(netINSD, hmaps, bbox_maps):
    B, R, S = hmaps.size(0), hmaps.size(1), hmaps.size(3)
    feats = netINSD(hmaps.reshape(B * R, 1, S, S), bbox_maps.reshape(B * R, -1, S, S))
    return netINSD.get_logits(feats).reshape(-1)


def _glb_probs(netGLBD, pooled_hmaps, pooled_maps):
    return netGLBD.get_logits(netGLBD(pooled_hmaps, pooled_maps)).reshape(-1)


def ins_discriminator_loss(netINSD, real_hmaps, fake_hmaps, bbox_maps):
    """real_hmaps, fake_hmaps [B, R, 1, S, S]; bbox_maps [B, R, nbf, S, S]"""
    real_errD = ops.bce_const(_ins_probs(netINSD, real_hmaps, bbox_maps), 1.0)
    fake_errD = ops.bce_const(_ins_probs(netINSD, fake_hmaps.detach(), bbox_maps), 0.0)
    return real_errD + fake_errD


def glb_discriminator_loss(netGLBD, real_hmaps, fake_hmaps, bbox_maps, pooled_maps=None):
    """real_hmaps [B, 1, S, S] (the pooled real masks); fake_hmaps [B, R, 1, S, S]; bbox_maps [B, R, nbf, S, S]
    (pooled_maps: their maximum over the boxes when the caller already has it)"""
    if pooled_maps is None:
        pooled_maps = ops.box_max(bbox_maps.detach())
    fake_pooled = ops.box_max(fake_hmaps.detach())
    real_errD = ops.bce_const(_glb_probs(netGLBD, real_hmaps, pooled_maps), 1.0)
    fake_errD = ops.bce_const(_glb_probs(netGLBD, fake_pooled, pooled_maps), 0.0)
    return real_errD + fake_errD


def generator_loss(netINSD, netGLBD, vgg_model, real_hmaps, fake_hmaps, bbox_maps, pooled_maps=None):
    """vgg_model None and PCP_LAMBDA == 0 -> (errG_total, (insg_loss, glbg_loss)); with the frozen network (model.VGG)
    and PCP_LAMBDA != 0 -> (errG_total, (insg_loss, glbg_loss, gpcp_loss), pcp_score) where gpcp_loss = PCP_LAMBDA *
    sum_i mean |fake_i - real_i| over the 19 taps and pcp_score is the unweighted sum (the reference's item_pcp_score).
    Device scalars, formatted by the caller only when it prints.  real_hmaps [B, R, 1, S, S]."""
    lam = _smooth("PCP_LAMBDA", 0.0)
    if lam != 0.0 and vgg_model is None:
        raise ObjganHipError("generator_loss: PCP_LAMBDA = %g needs the frozen VGG-19-bn (vgg_model is None); there is no "
                             "silent loss without the term" % lam)
    if lam == 0.0 and vgg_model is not None:
        raise ObjganHipError("generator_loss: a perceptual network was passed but PCP_LAMBDA is 0: pass vgg_model=None")
    insg_loss = ops.bce_const(_ins_probs(netINSD, fake_hmaps, bbox_maps), 1.0) * _smooth("INS_LAMBDA", 1.0)
    if pooled_maps is None:
        pooled_maps = ops.box_max(bbox_maps.detach())
    fake_pooled = ops.box_max(fake_hmaps)
    glbg_loss = ops.bce_const(_glb_probs(netGLBD, fake_pooled, pooled_maps), 1.0) * _smooth("GLB_LAMBDA", 1.0)
    if vgg_model is None:
        return insg_loss + glbg_loss, (insg_loss, glbg_loss)
    taps = vgg_model.perceptual(fake_pooled, ops.box_max(real_hmaps.detach()))
    pcp_score = taps.sum()
    gpcp_loss = pcp_score * lam
    return insg_loss + glbg_loss + gpcp_loss, (insg_loss, glbg_loss, gpcp_loss), pcp_score.detach()
