"""The box generator's two losses in plain torch, under the reference's class names and its eval_batch / get_loss /
reset interface (reference box_generation/seq2seq/loss/loss.py).  They serve a trainer loop kept from the reference
(the lists DecoderRNN returns with is_training=1 are connected to autograd) and restate on the CPU what
objgan_box_train_loss computes on the device.  The fused training step (SupervisedTrainer._train_batch) does not call
them; it reads `lamda`, `mask` and the label weights from them.

Both accumulate a sum over the steps handed to eval_batch and a count of the steps that are not padding;
get_loss() = lamda * sum / count.  What the sums are:

  Perplexity   sum of -weight[label] * p[label] over the batch: nn.NLLLoss applied to the clamped PROBABILITIES the
               decoder returns, not to their logs, with weight[mask] = 0
  BBLoss       sum of -[label != 0] * (pdf_xy + pdf_wh), pdf = log(sum_k pi_k exp(a_k - a_max) / max(norm_k, 1e-5) + 1e-5)
               + a_max, a_k the exponent of the bivariate normal and norm_k = 2 pi sigma sigma sqrt(1 - rho^2); a_max is
               not detached, so the gradient runs through it"""
import math

import torch
import torch.nn as nn


class _StepSum(object):
    """a running sum over steps and the number of non-pad steps behind it"""

    def __init__(self, name, lamda):
        self.name = name
        self.lamda = lamda
        self.reset()

    def reset(self):
        self.acc_loss = 0
        self.norm_term = 0

    def get_loss(self):
        count = self.norm_term
        return self.lamda * self.acc_loss / (count.float() if torch.is_tensor(count) else float(count))


class Perplexity(_StepSum):
    def __init__(self, weight=None, mask=None, lamda=1.0):
        if mask is not None and weight is None:
            raise ValueError("a masked label needs the weight vector its entry is zeroed in")
        if mask is not None:
            weight[mask] = 0            # in place, as the reference does: the caller's tensor is the criterion's
        self.mask = mask
        self.criterion = nn.NLLLoss(weight=weight, reduction='sum')
        super(Perplexity, self).__init__("Perplexity", lamda)

    def cuda(self):
        self.criterion.cuda()

    def eval_batch(self, outputs, target):
        """outputs [batch, labels]: the step's clamped label probabilities; target [batch]"""
        self.acc_loss = self.acc_loss + self.criterion(outputs, target)
        self.norm_term = self.norm_term + (target.numel() if self.mask is None else (target.detach() != self.mask).sum())


class BBLoss(_StepSum):
    def __init__(self, batch_size, gmm_comp_num, lamda):
        self.batch_size = batch_size
        self.gmm_comp_num = gmm_comp_num
        super(BBLoss, self).__init__("Bbox Loss", lamda)

    def cuda(self):
        pass

    @staticmethod
    def pdf(pi, u_x, u_y, sigma_x, sigma_y, rho, x, y):
        """log-density of the mixture at (x, y), [batch]; the parameters are [batch, K], x and y [batch, 1]"""
        dx, dy = (x - u_x) / sigma_x, (y - u_y) / sigma_y
        # the cross term keeps the reference's grouping (product of the differences over the product of the sigmas)
        z = dx ** 2 + dy ** 2 - 2 * rho * ((x - u_x) * (y - u_y) / (sigma_x * sigma_y))
        a = -z / (2 * (1 - rho ** 2))
        a_max = a.max(dim=1, keepdim=True)[0]
        norm = (2 * math.pi * sigma_x * sigma_y * torch.sqrt(1 - rho ** 2)).clamp(min=1e-5)
        return torch.log((pi * torch.exp(a - a_max) / norm).sum(dim=1) + 1e-5) + a_max.squeeze(1)

    def eval_batch(self, xy_gmm_params, wh_gmm_params, gt_x, gt_y, gt_w, gt_h, gt_l):
        """the two parameter tuples (pi, u, u, sigma, sigma, rho) hold [batch, K] tensors, the targets are [batch]"""
        keep = (gt_l != 0).to(xy_gmm_params[0].dtype)
        xy = self.pdf(*xy_gmm_params, gt_x.unsqueeze(1), gt_y.unsqueeze(1))
        wh = self.pdf(*wh_gmm_params, gt_w.unsqueeze(1), gt_h.unsqueeze(1))
        self.acc_loss = self.acc_loss - (keep * xy).sum() - (keep * wh).sum()
        self.norm_term = self.norm_term + keep.sum()
