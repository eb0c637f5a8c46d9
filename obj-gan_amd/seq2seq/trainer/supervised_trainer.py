"""Box-generator training (reference box_generation/seq2seq/trainer/supervised_trainer.py).

The reference's step is one caption: ten LSTM-cell launches of batch 1, two mixture heads, a Python loop of loss
calls, autograd, clip_grad_norm and Adam.  Here a step of B captions is the frozen encoder (csrc/lstm.hip), three entry
points of csrc/box_train.hip (forward, loss, backward), the norm / clip kernel and the fused Adam
(objgan_adam_step_gated), all on flat device arenas; nothing is read back unless the step prints or checkpoints.

Batch semantics: loss = (lamda1 sum_b label_b + lamda2 sum_b box_b) / sum_b n_b with n_b the non-pad steps of caption
b -- what the reference's loss classes compute when handed a batch; at B = 1 it is the reference's step."""
from __future__ import division

import logging
import os
import random

import torch
from torch import optim

from objgan_hip import ops
from seq2seq.dataset.prepare_dataset import random_batch
from seq2seq.models.DecoderRNN import DecoderRNN, _TRANSPOSED
from seq2seq.optim import Optimizer
from seq2seq.util.checkpoint import Checkpoint


class FusedBoxStep(object):
    """Parameters, gradients and Adam moments of a DecoderRNN as flat arenas in the kernels' layout.  The arena is the
    master copy while training: `step` updates it in place, `sync_to_module` writes it back to the nn.Parameters
    (before state_dict() / a checkpoint), `load_optimizer` / `store_optimizer` exchange the moments and the step
    count with a torch.optim.Adam."""

    def __init__(self, decoder, weight, lamda1=1.0, lamda2=1.0, max_grad_norm=5, lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, pad=0):
        params = decoder._params()
        dev = params[0].device
        if dev.type != 'cuda':
            raise ops._lib.ObjganHipError("training the box generator runs on the GPU kernels (got a %s module); "
                                          "there is no CPU path" % dev)
        self.decoder = decoder
        H, L, K, A = decoder.hidden_size, decoder.l_output_size, decoder.gmm_comp_num, decoder.aug_size
        self.K, self.pad = K, pad
        shapes = ops.box_weight_shapes(H, L, K, A)
        with torch.no_grad():
            self.flat_p, self.p = ops.box_arena(shapes, dev, [(t.t() if i in _TRANSPOSED else t).detach()
                                                              for i, t in enumerate(params)])
        self.flat_g, self.g = ops.box_arena(shapes, dev)
        self.flat_m, self.m = ops.box_arena(shapes, dev)
        self.flat_v, self.v = ops.box_arena(shapes, dev)
        weight = weight.detach().to(device=dev, dtype=torch.float32).clone()
        weight[pad] = 0
        self.weight = weight
        self.lamda1, self.lamda2 = float(lamda1), float(lamda2)
        self.max_grad_norm = float(max_grad_norm)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)
        self.clip = torch.ones(2, dtype=torch.float32, device=dev)
        self.coef = torch.zeros(3, dtype=torch.float32, device=dev)
        self.partials = torch.zeros(256, dtype=torch.float64, device=dev)
        self.first = (decoder.x_mean, decoder.y_mean, decoder.w_mean, decoder.r_mean)

    def gradients(self, h0, c0, labels, boxes, lens, cpw=None):
        """forward, loss, backward -> (sums, trace, dtrace); the gradients are in self.g"""
        trace, ws = ops.box_train_forward(h0, c0, labels, boxes, lens, self.p, self.first, cpw=cpw)
        sums, dtrace = ops.box_train_loss(trace, labels, boxes, lens, self.weight, self.lamda1, self.lamda2, self.K,
                                          pad=self.pad)
        ops.box_train_backward(dtrace, trace, c0, labels, lens, self.p, ws, grads=self.g, cpw=cpw)
        return sums, trace, dtrace

    def update(self):
        """clip_grad_norm_(max_grad_norm) and Adam on the arenas, coefficient and step count on the device"""
        if self.max_grad_norm > 0:
            ops.box_train_clip(self.flat_g, self.max_grad_norm, self.partials, self.clip)
        ops.adam_step_gated_(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.lr, self.betas[0],
                             self.betas[1], self.eps, self.state, self.clip, self.coef, grad_scale=-1.0)

    def step(self, h0, c0, labels, boxes, lens):
        sums = self.gradients(h0, c0, labels, boxes, lens)[0]
        self.update()
        return sums

    def sync_to_module(self):
        with torch.no_grad():
            for i, (t, p) in enumerate(zip(self.decoder._params(), self.p)):
                t.copy_(p.t() if i in _TRANSPOSED else p)

    def load_optimizer(self, adam):
        """moments and step count of a torch.optim.Adam over decoder.parameters() -> the arenas"""
        steps = 0
        with torch.no_grad():
            for i, t in enumerate(self.decoder._params()):
                st = adam.state.get(t)
                if not st:
                    continue
                self.m[i].copy_(st['exp_avg'].t() if i in _TRANSPOSED else st['exp_avg'])
                self.v[i].copy_(st['exp_avg_sq'].t() if i in _TRANSPOSED else st['exp_avg_sq'])
                steps = int(st['step'])
        self.state.copy_(torch.tensor([float(steps), self.betas[0] ** steps, self.betas[1] ** steps],
                                      dtype=torch.float64))

    def store_optimizer(self, adam):
        """the arenas' moments and step count -> the state of a torch.optim.Adam over decoder.parameters()"""
        steps = float(self.state[0])
        for i, t in enumerate(self.decoder._params()):
            adam.state[t] = {'step': torch.tensor(steps),
                             'exp_avg': (self.m[i].t() if i in _TRANSPOSED else self.m[i]).clone().contiguous(),
                             'exp_avg_sq': (self.v[i].t() if i in _TRANSPOSED else self.v[i]).clone().contiguous()}


class _Window(object):
    """label / box losses of the print steps since the last log line"""

    def __init__(self):
        self.label = self.box = 0.0
        self.count = 0

    def add(self, label, box):
        self.label, self.box, self.count = self.label + label, self.box + box, self.count + 1

    def line(self, step, steps_per_epoch, total_steps, names):
        n = self.count
        text = '%d/%d Progress: %d%%, Train Total: %.4f, %s: %.4f, %s: %.4f' % (
            step, steps_per_epoch, 100 * step / total_steps, (self.label + self.box) / n, names[0], self.label / n,
            names[1], self.box / n)
        self.__init__()
        return text


class SupervisedTrainer(object):
    """The reference's trainer object: same constructor arguments, `train(encoder, decoder, data, num_epochs, resume,
    dev_data, optimizer, is_training)`, its console lines (`epoch: `, `step: `, `l_accuracy: `) and its checkpoint
    rhythm (every `checkpoint_every` steps and at the last step), around the fused device step."""

    def __init__(self, expt_dir='experiment', lloss=None, bloss=None, batch_size=64, random_seed=None,
                 checkpoint_every=100, print_every=1, train_cap_lang=None, train_label_lang=None, x_mean_std=None,
                 y_mean_std=None, w_mean_std=None, r_mean_std=None):
        self.logger = logging.getLogger(__name__)
        self.lloss, self.bloss = lloss, bloss
        self.batch_size = batch_size
        self.print_every, self.checkpoint_every = print_every, checkpoint_every
        self.train_cap_lang, self.train_label_lang = train_cap_lang, train_label_lang
        self.x_mean_std, self.y_mean_std, self.w_mean_std, self.r_mean_std = x_mean_std, y_mean_std, w_mean_std, r_mean_std
        self.expt_dir = os.path.abspath(expt_dir)
        os.makedirs(self.expt_dir, exist_ok=True)
        self.random_seed = random_seed
        if random_seed is not None:                    # Python's generator draws the batches, torch's the init
            random.seed(random_seed)
            torch.manual_seed(random_seed)
        self.optimizer = None
        self.fused = None
        self.history = []                 # (step, label loss, box loss) of the print steps

    def _fused(self, decoder):
        if self.fused is None or self.fused.decoder is not decoder:
            inner = self.optimizer.optimizer
            g = inner.param_groups[0]
            self.fused = FusedBoxStep(decoder, self.lloss.criterion.weight, self.lloss.lamda, self.bloss.lamda,
                                      max_grad_norm=self.optimizer.max_grad_norm, lr=g['lr'], betas=g['betas'],
                                      eps=g['eps'], pad=self.lloss.mask if self.lloss.mask is not None else 0)
            self.fused.load_optimizer(inner)
        return self.fused

    def _train_batch(self, input_variable, input_lengths, target_l_variables, target_x_variables, target_y_variables,
                     target_w_variables, target_h_variables, encoder, decoder, is_training, batch_step):
        """one fused step; the losses and the accuracy are read from the device on print steps only (None otherwise)"""
        fused = self._fused(decoder)
        with torch.no_grad():
            _, encoder_hidden = encoder(input_variable, input_lengths)
            h0, c0 = (s[0].contiguous() for s in decoder._init_state(encoder_hidden))
            labels, boxes, lens = DecoderRNN.pack_targets(target_l_variables, target_x_variables, target_y_variables,
                                                          target_w_variables, target_h_variables)
            sums = fused.step(h0, c0, labels, boxes, lens)
        if batch_step % self.print_every != 0:
            return None, None
        s = sums.cpu()
        n = float(s[-1])
        per = s[:-1].view(-1, 4).sum(dim=0)
        l_accuracy = float(per[3]) / n if n > 0 else float('nan')
        print('l_accuracy: {}'.format(l_accuracy))
        return fused.lamda1 * float(per[0]) / n, fused.lamda2 * float(per[1]) / n

    def _checkpoint(self, decoder, epoch, step):
        self.fused.sync_to_module()
        self.fused.store_optimizer(self.optimizer.optimizer)
        return Checkpoint(model=decoder, optimizer=self.optimizer, epoch=epoch, step=step,
                          cap_word2index=self.train_cap_lang.word2index, cap_index2word=self.train_cap_lang.index2word,
                          label_word2index=self.train_label_lang.word2index,
                          label_index2word=self.train_label_lang.index2word).save(self.expt_dir)

    def _train_epoches(self, data, encoder, decoder, n_epochs, start_epoch, start_step, dev_data=None, is_training=0,
                       rng=None):
        """epochs start_epoch .. n_epochs of round(len(data) / batch_size) steps each, counting on from start_step.
        The averages of a log line are over the steps whose losses were read, i.e. the print steps."""
        steps_per_epoch = int(round(len(data) / self.batch_size))
        total_steps = steps_per_epoch * n_epochs
        means = (self.x_mean_std, self.y_mean_std, self.w_mean_std, self.r_mean_std)
        names = (self.lloss.name, self.bloss.name)
        window, last_line = _Window(), ''
        step = saved_at = start_step
        epoch = start_epoch
        decoder.train(True)
        for epoch in range(start_epoch, n_epochs + 1):
            self.logger.debug("Epoch: %d, Step: %d" % (epoch, step))
            print('epoch: ', epoch)
            for step in range(step + 1, step + steps_per_epoch + 1):
                caps, cap_lens, tl, _, tx, ty, tw, tr = random_batch(self.batch_size, data, self.train_cap_lang,
                                                                     self.train_label_lang, *means, is_training=1, rng=rng)
                losses = self._train_batch(caps, cap_lens, tl, tx, ty, tw, tr, encoder, decoder, is_training, step)
                if losses[0] is not None:
                    window.add(*losses)
                    self.history.append((step,) + tuple(losses))
                    print('step: ', step)
                    last_line = window.line(step, steps_per_epoch, total_steps, names)
                    self.logger.info(last_line)
                if step % self.checkpoint_every == 0 or step == total_steps:
                    self._checkpoint(decoder, epoch, step)
                    saved_at = step
            self.logger.info(last_line)
        if self.fused is not None:
            # a resumed run repeats its checkpoint's epoch and so counts past total_steps: whatever the rhythm above
            # left unsaved is saved here, and the module holds the trained weights afterwards
            if step != saved_at:
                self._checkpoint(decoder, epoch, step)
            self.fused.sync_to_module()
            self.fused.store_optimizer(self.optimizer.optimizer)

    def train(self, encoder, decoder, data, num_epochs=5, resume=False, dev_data=None, optimizer=None, is_training=0,
              rng=None):
        """-> the trained decoder.  resume: decoder, optimizer state, epoch and step come from the newest checkpoint
        under expt_dir (the `decoder` argument is ignored, as in the reference)."""
        start_epoch, start_step = 1, 0
        if resume:
            path = Checkpoint.get_latest_checkpoint(self.expt_dir)
            ck = Checkpoint.load(path)
            if ck.optimizer is None:
                raise ValueError("%s holds no optimizer state to resume from" % path)
            decoder = ck.model.to(next(encoder.parameters()).device)
            # the loaded Adam state sits on the CPU: an optimizer over the moved parameters takes it over
            adam = type(ck.optimizer.optimizer)(decoder.parameters())
            adam.load_state_dict(ck.optimizer.optimizer.state_dict())
            ck.optimizer.optimizer = adam
            self.optimizer, start_epoch, start_step = ck.optimizer, ck.epoch, ck.step
        else:
            self.optimizer = optimizer if optimizer is not None else Optimizer(optim.Adam(decoder.parameters()),
                                                                               max_grad_norm=5)
        if not isinstance(self.optimizer.optimizer, optim.Adam):
            raise NotImplementedError("the fused step implements torch.optim.Adam")
        self.logger.info("Optimizer: %s, Scheduler: %s" % (self.optimizer.optimizer, self.optimizer.scheduler))
        self._train_epoches(data, encoder, decoder, num_epochs, start_epoch, start_step, dev_data=dev_data,
                            is_training=is_training, rng=rng)
        return decoder


