"""DAMSM pretraining: the text encoder (RNN_ENCODER) and the image encoder's two projections learn to match captions and
images (AttnGAN's pretrain_DAMSM.py, the program the reference's `pretrained/text_encoder100.pth` and
`image_encoder100.pth` come from).  The step minimises w_loss0 + w_loss1 + s_loss0 + s_loss1 of miscc.losses over a batch
of (largest image, caption) pairs; the Inception trunk stays frozen.

The parameters, their gradients and the Adam moments live in one flat arena owned by this trainer, text encoder first:
the global-norm clip (ops.box_train_clip) runs over the text slice only, the update is the gated fused Adam
(ops.adam_step_gated_) -- the text slice divided by the clip's device scalar, the projections as they are.  A step
reads nothing back to the host unless it prints.
"""
import os
import re
import sys
import time

import torch

from miscc.config import cfg
from miscc.losses import words_loss, sent_loss
from miscc.utils import mkdir_p, _host
from objgan_hip import ops

BETAS = (0.5, 0.999)
EPS = 1e-8
INCEPTION_FILE = 'inception_v3_google-1a9a5a14.pth'
PROJECTION_KEYS = ("emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias")


class Refusal(Exception):
    """what pretrain_DAMSM.py answers with one line on stderr and exit status 2"""


def next_lr(lr, base_lr):
    """the learning rate after an epoch: lr * 0.98 while lr > base_lr / 10"""
    return lr * 0.98 if lr > base_lr / 10.0 else lr


def resume_epoch(path):
    """text_encoder<N>.pth -> N (0 when the name carries no number)"""
    m = re.search(r'text_encoder(\d+)\.pth$', os.path.basename(path))
    return int(m.group(1)) if m else 0


def image_encoder_path(net_e):
    d, name = os.path.split(net_e)
    return os.path.join(d, name.replace('text_encoder', 'image_encoder'))


def check_files(data_dir, net_e, net_inception):
    """The refusals that need no device: a missing data directory, a missing resume pair, a missing Inception file."""
    if not os.path.isdir(data_dir) or not os.path.isfile(os.path.join(data_dir, 'captions.pickle')):
        raise Refusal("no prepared data directory at %s (captions.pickle, train/filenames.pickle, train_imgs.bigfile; "
                      "prepare_data.py builds one)" % data_dir)
    if net_e:
        pair = (net_e, image_encoder_path(net_e))
        missing = [p for p in pair if not os.path.isfile(p)]
        if missing or 'text_encoder' not in os.path.basename(net_e):
            raise Refusal("--NET_E resumes from a text_encoder*.pth / image_encoder*.pth pair; missing: %s"
                          % ", ".join(missing or pair[:1]))
    elif not os.path.isfile(net_inception):
        raise Refusal("no Inception-v3 ImageNet weights at %s (torchvision's %s; --NET_INCEPTION names the file)"
                      % (net_inception, INCEPTION_FILE))


def build_encoders(n_words, net_e, net_inception, device):
    """-> (text_encoder, image_encoder, first epoch): fresh encoders on the ImageNet trunk, or the pair --NET_E names"""
    import encoders
    from model import RNN_ENCODER
    text = RNN_ENCODER(n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)
    if net_e:
        image = encoders.CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
        text.load_state_dict(torch.load(net_e, map_location="cpu"))
        image.load_state_dict(torch.load(image_encoder_path(net_e), map_location="cpu"))
        print('Load', net_e, 'and', image_encoder_path(net_e))
        start = resume_epoch(net_e)
    else:
        net = encoders.inception_v3()
        net.load_state_dict(torch.load(net_inception, map_location="cpu"))
        print('Load pretrained model from', net_inception)
        image = encoders.CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM, net)
        start = 0
    for k, p in image.named_parameters():
        p.requires_grad_(k in PROJECTION_KEYS)
    image.train_projections = True
    return text.to(device), image.to(device).eval(), start


class EncoderArena(object):
    """text encoder parameters, then the image encoder's projections, re-homed into one flat buffer; .grad of each is
    its view of the flat gradient buffer, so that backward accumulates in place"""

    def __init__(self, text_encoder, image_encoder):
        named = dict(image_encoder.named_parameters())
        self.text_params = list(text_encoder.parameters())
        self.params = self.text_params + [named[k] for k in PROJECTION_KEYS]
        self.n_text = sum(p.numel() for p in self.text_params)
        self.n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.n, dtype=torch.float32, device=dev)
        # per slice: steps, beta1^steps, beta2^steps (advanced by the gated kernel) and its 3 floats of scratch
        self.state = [torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev) for _ in range(2)]
        self.coef = [torch.zeros(3, dtype=torch.float32, device=dev) for _ in range(2)]
        self.partials = torch.empty(256, dtype=torch.float64, device=dev)
        self.clip_out = torch.ones(2, dtype=torch.float32, device=dev)
        self.one = torch.ones(1, dtype=torch.float32, device=dev)
        self._views = []
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            self._views.append(self.grad[off:off + k].view_as(p))
            off += k
        self.zero_grad()

    def zero_grad(self):
        self.grad.zero_()
        for p, gv in zip(self.params, self._views):
            p.grad = gv

    def sync_grads(self):
        for p, gv in zip(self.params, self._views):
            if p.grad is None:
                gv.zero_()
            elif p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad)
            p.grad = gv

    def step(self, lr, max_norm):
        """clip_grad_norm_(text parameters, max_norm), then Adam over everything; nothing is read back"""
        self.sync_grads()
        nt = self.n_text
        ops.box_train_clip(self.grad[:nt], max_norm, self.partials, self.clip_out)
        for i, (a, b, flag, scale) in enumerate(((0, nt, self.clip_out, -1.0), (nt, self.n, self.one, 1.0))):
            ops.adam_step_gated_(self.flat[a:b], self.grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b], lr, BETAS[0],
                                 BETAS[1], EPS, self.state[i], flag, self.coef[i], grad_scale=scale)


class DAMSMTrainer(object):
    def __init__(self, output_dir, dataloader, dataset, device, text_encoder, image_encoder, start_epoch=0,
                 encoder_lr=0.002, rnn_grad_clip=0.25, max_epoch=600, snapshot_interval=5, print_interval=200,
                 val_loader=None):
        self.model_dir = os.path.join(output_dir, 'Model') if output_dir else ''
        if self.model_dir:
            mkdir_p(self.model_dir)
        self.dataloader, self.dataset, self.device = dataloader, dataset, device
        self.val_loader = val_loader
        self.text_encoder, self.image_encoder = text_encoder, image_encoder
        self.start_epoch = start_epoch
        self.base_lr, self.clip = float(encoder_lr), float(rnn_grad_clip)
        self.max_epoch, self.snapshot_interval = int(max_epoch), int(snapshot_interval)
        self.print_interval = int(print_interval)
        self.arena = EncoderArena(text_encoder, image_encoder)
        self.lr = self.base_lr
        for _ in range(start_epoch):
            self.lr = next_lr(self.lr, self.base_lr)
        self.epoch_losses = []          # per finished epoch: the summed (w0, w1, s0, s1) of its steps
        self._labels = {}

    def labels(self, B):
        if B not in self._labels:
            self._labels[B] = torch.arange(B, device=self.device)
        return self._labels[B]

    def losses(self, imgs, captions, cap_lens, class_ids):
        """-> the four losses (device scalars) of a batch sorted by caption length"""
        B = captions.shape[0]
        max_len = int(_host(cap_lens).max())
        words_emb, sent_emb = self.text_encoder(captions, cap_lens, max_len)
        feats, code = self.image_encoder(imgs)
        labels = self.labels(B)
        w0, w1, _, _ = words_loss(feats, words_emb, labels, cap_lens, class_ids, B, top1=False, need_att_maps=False)
        s0, s1, _ = sent_loss(code, sent_emb, labels, class_ids, B, top1=False)
        return torch.stack((w0, w1, s0, s1))

    def train_step(self, imgs, captions, cap_lens, class_ids):
        self.arena.zero_grad()
        four = self.losses(imgs, captions, cap_lens, class_ids)
        four.sum().backward()
        self.arena.step(self.lr, self.clip)
        return four.detach()

    def prepare(self, data):
        from trainDataset import prepare_data
        p = prepare_data(data, self.device, self.dataset.num_classes)
        captions = p[1].reshape(len(p[11]), -1)
        return p[0][-1], captions, p[3], p[10]

    def train_epoch(self, epoch):
        self.text_encoder.train()
        total = torch.zeros(4, device=self.device)
        window = torch.zeros(4, device=self.device)
        start = time.time()
        for step, data in enumerate(self.dataloader, 1):
            four = self.train_step(*self.prepare(data))
            total += four
            window += four
            if self.print_interval > 0 and step % self.print_interval == 0:
                w = (window / self.print_interval).tolist()
                print('| epoch {:3d} | {:5d}/{:5d} batches | ms/batch {:5.2f} | s_loss {:5.2f} {:5.2f} | w_loss {:5.2f} '
                      '{:5.2f}'.format(epoch, step, len(self.dataloader), (time.time() - start) * 1000. / self.print_interval,
                                       w[2], w[3], w[0], w[1]))
                window.zero_()
                start = time.time()
        return total.tolist()

    @torch.no_grad()
    def evaluate(self):
        """-> (mean sentence loss, mean word loss) over the validation loader, eval mode, forward only"""
        self.text_encoder.eval()
        total = torch.zeros(4, device=self.device)
        n = 0
        for data in self.val_loader:
            total += self.losses(*self.prepare(data))
            n += 1
        self.text_encoder.train()
        t = (total / max(n, 1)).tolist()
        return t[2] + t[3], t[0] + t[1]

    def save(self, epoch):
        text = {k: v.detach().clone().cpu() for k, v in self.text_encoder.state_dict().items()}
        image = {k: v.detach().clone().cpu() for k, v in self.image_encoder.state_dict().items()}
        torch.save(text, os.path.join(self.model_dir, 'text_encoder%d.pth' % epoch))
        torch.save(image, os.path.join(self.model_dir, 'image_encoder%d.pth' % epoch))
        print('Save encoders of epoch %d to %s' % (epoch, self.model_dir))

    def train(self):
        epoch = self.start_epoch
        if self.val_loader is None:
            print('no test split in the data directory: validation skipped')
        for epoch in range(self.start_epoch + 1, self.max_epoch + 1):
            t0 = time.time()
            four = self.train_epoch(epoch)
            self.epoch_losses.append(four)
            print('| end epoch {:3d} | {:6.1f} s | lr {:.5f} | summed loss {:.4f} (w {:.4f} {:.4f} s {:.4f} {:.4f})'.format(
                epoch, time.time() - t0, self.lr, sum(four), *four))
            if self.val_loader is not None:
                s, w = self.evaluate()
                print('| end epoch {:3d} | valid loss {:5.2f} {:5.2f}'.format(epoch, s, w))
            self.lr = next_lr(self.lr, self.base_lr)
            if self.model_dir and (epoch % self.snapshot_interval == 0 or epoch == self.max_epoch):
                self.save(epoch)
        sys.stdout.flush()
        return epoch
