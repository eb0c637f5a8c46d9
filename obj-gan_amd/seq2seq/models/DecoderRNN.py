import numpy as np
import torch
import torch.nn as nn

from objgan_hip import ops


def draw_noise(rng, n, steps):
    """The decoder's noise rows for n captions, [n, steps, 6] float64: per step a uniform and two standard normals for
    the (x, y) draw, then the same for (w, h).  Drawn caption by caption (steps x 2 uniforms, then steps x 4 normals),
    so a caption's row depends on its index in the stream and not on how the captions are batched."""
    rng = np.random if rng is None else rng
    noise = np.empty((n, steps, 6), dtype=np.float64)
    for i in range(n):
        u = rng.random_sample((steps, 2))
        z = rng.standard_normal((steps, 4))
        noise[i, :, 0], noise[i, :, 1:3] = u[:, 0], z[:, 0:2]
        noise[i, :, 3], noise[i, :, 4:6] = u[:, 1], z[:, 2:4]
    return noise


_TRANSPOSED = (7, 8, 11, 13, 15)


class _TeacherForced(torch.autograd.Function):
    """trace = objgan_box_train_forward(...); backward = objgan_box_train_backward, gradients handed back in the nn
    layout.  The transposed copies the kernels stream are made per call here (the autograd route serves a trainer loop
    kept from the reference; the fused step keeps its master copy in the kernel's layout instead)."""

    @staticmethod
    def forward(ctx, h0, c0, labels, boxes, lens, first, *params):
        with torch.no_grad():
            W = [(p.t() if i in _TRANSPOSED else p).detach().contiguous() for i, p in enumerate(params)]
        trace, ws = ops.box_train_forward(h0, c0, labels, boxes, lens, W, first)
        ctx.saved = (trace, ws, c0, labels, lens, W)
        return trace

    @staticmethod
    def backward(ctx, dtrace):
        trace, ws, c0, labels, lens, W = ctx.saved
        grads = ops.box_train_backward(dtrace.contiguous(), trace, c0, labels, lens, W, ws)
        out = [(g.t() if i in _TRANSPOSED else g) for i, g in enumerate(grads)]
        return (None,) * 6 + tuple(out)


class DecoderRNN(nn.Module):
    """The box generator's decoder, sampling path (reference box_generation/seq2seq/models/DecoderRNN.py): same
    constructor arguments and the same 17 state-dict tensors (`l_embedding.weight`, `xy_embedding.*`, `wh_embedding.*`,
    `next_xy_embedding.*`, `rnn.{weight,bias}_{ih,hh}_l0`, `l_out.*`, `xy_out.*`, `wh_out.*`).  The nn modules hold the
    parameters; a whole decode of B captions is ONE launch of objgan_box_decode, and every row of the result is what
    the reference computes for that caption alone (its batch size is 1).

    The kernel draws no random numbers: `noise` [B, T, 6] (see draw_noise) makes a layout a pure function of weights,
    caption and noise row.  The component choice follows np.random.choice on the temperature-adjusted weights; the
    point is the Cholesky factor of the reference's covariance applied to two normals (numpy's multivariate_normal
    factors the same matrix by SVD: same law, other sample for the same normals).

    Training: forward(..., target_*_variables, is_training=1) is the teacher-forced pass of B captions in ONE launch of
    objgan_box_train_forward, connected to autograd by _TeacherForced (its backward is objgan_box_train_backward), so
    the reference's loop of loss calls and loss.backward() works on the returned lists for one caption or a batch of
    equal lengths (rows past a caption's length are zero, where the reference's BBLoss divides 0 by 0: for captions of
    unequal lengths use SupervisedTrainer, whose fused step masks by length).  The fused step of
    seq2seq.trainer does not go through autograd.  input_dropout_p must be 0; dropout_p is accepted and does nothing,
    as in torch (nn.LSTM applies dropout between layers only, and there is one layer).  Free-running training
    (is_training=1 without targets) and the attention variant are not built here."""
    KEY_ATTN_SCORE = 'attention_score'
    KEY_LENGTH = 'length'
    KEY_SEQUENCE = 'sequence'
    KEY_XYS = 'xy'
    KEY_WHS = 'wh'

    def __init__(self, l_word2index, x_mean, y_mean, w_mean, r_mean, batch_size, max_len, hidden_size, gmm_comp_num,
                 n_layers=1, rnn_cell='lstm', bidirectional=False, input_dropout_p=0, dropout_p=0,
                 use_attention=False):
        super(DecoderRNN, self).__init__()
        if use_attention:
            raise NotImplementedError("use_attention=True: the reference's sample.py and every checkpoint it writes "
                                      "use the plain decoder; the attention variant has no kernel here")
        if rnn_cell.lower() != 'lstm' or n_layers != 1:
            raise NotImplementedError("the kernel evaluates the reference default: one LSTM cell")
        self.vocab_size = self.l_output_size = len(l_word2index)
        self.max_len = self.max_length = max_len
        self.hidden_size = hidden_size
        self.n_layers = n_layers
        self.input_dropout_p = input_dropout_p
        self.dropout_p = dropout_p
        self.bidirectional_encoder = bidirectional
        self.aug_size = 50
        self.batch_size = batch_size
        self.gmm_comp_num = gmm_comp_num
        self.gmm_param_num = 6           # pi, u_x, u_y, sigma_x, sigma_y, rho_xy
        self.use_attention = use_attention
        self.l_eos_id = l_word2index["<eos>"]
        self.l_sos_id = l_word2index["<sos>"]
        self.x_mean, self.y_mean, self.w_mean, self.r_mean = x_mean, y_mean, w_mean, r_mean
        self.temperature = 0.4

        self.l_embedding = nn.Embedding(self.l_output_size, hidden_size)
        self.xy_embedding = nn.Linear(2, self.aug_size)
        self.wh_embedding = nn.Linear(2, self.aug_size)
        self.next_xy_embedding = nn.Linear(2, self.aug_size)
        self.rnn = nn.LSTM(hidden_size + 2 * self.aug_size, hidden_size, n_layers, batch_first=True)
        self.l_out = nn.Linear(hidden_size, self.l_output_size)
        self.xy_out = nn.Linear(hidden_size + self.l_output_size, gmm_comp_num * self.gmm_param_num)
        self.wh_out = nn.Linear(hidden_size + self.l_output_size + self.aug_size, gmm_comp_num * self.gmm_param_num)
        self._packed = None

    def _weights(self):
        """the 17 tensors in the kernel's order, the matrices it streams transposed (consecutive threads read
        consecutive floats); rebuilt when a parameter was replaced or edited"""
        srcs = (self.l_embedding.weight, self.xy_embedding.weight, self.xy_embedding.bias,
                self.wh_embedding.weight, self.wh_embedding.bias,
                self.next_xy_embedding.weight, self.next_xy_embedding.bias,
                self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0, self.rnn.bias_hh_l0,
                self.l_out.weight, self.l_out.bias, self.xy_out.weight, self.xy_out.bias,
                self.wh_out.weight, self.wh_out.bias)
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        if self._packed is None or self._packed[0] != key:
            transposed = (7, 8, 11, 13, 15)
            with torch.no_grad():
                packed = [(t.t() if i in transposed else t).detach().contiguous() for i, t in enumerate(srcs)]
            self._packed = (key, packed)
        return self._packed[1]

    def _params(self):
        """the 17 parameters in the kernel's order (nn layout)"""
        return (self.l_embedding.weight, self.xy_embedding.weight, self.xy_embedding.bias,
                self.wh_embedding.weight, self.wh_embedding.bias,
                self.next_xy_embedding.weight, self.next_xy_embedding.bias,
                self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0, self.rnn.bias_hh_l0,
                self.l_out.weight, self.l_out.bias, self.xy_out.weight, self.xy_out.bias,
                self.wh_out.weight, self.wh_out.bias)

    @staticmethod
    def pack_targets(target_l, target_x, target_y, target_w, target_h, pad=0):
        """[B, T + 1] targets -> labels int32, boxes [B, T + 1, 4] fp32, lens [B] int32 (steps up to the last non-pad
        label) on the targets' device, without a host read"""
        labels = target_l.to(torch.int32).contiguous()
        boxes = torch.stack((target_x, target_y, target_w, target_h), dim=2).to(torch.float32).contiguous()
        T = labels.shape[1] - 1
        steps = torch.arange(1, T + 1, device=labels.device, dtype=torch.int32)
        lens = ((labels[:, 1:] != pad).to(torch.int32) * steps).amax(dim=1).to(torch.int32).contiguous()
        return labels, boxes, lens

    def _forward_train(self, encoder_hidden, target_l, target_x, target_y, target_w, target_h):
        if self.input_dropout_p != 0:
            raise NotImplementedError("input_dropout_p != 0: the training kernels apply no input dropout (the "
                                      "reference's sample.py never sets it)")
        if encoder_hidden is None:
            raise ValueError("the training path needs the encoder's (h_n, c_n)")
        h0, c0 = (s[0] for s in self._init_state(encoder_hidden))
        labels, boxes, lens = self.pack_targets(target_l, target_x, target_y, target_w, target_h)
        T = labels.shape[1] - 1
        first = (self.x_mean, self.y_mean, self.w_mean, self.r_mean)
        trace = _TeacherForced.apply(h0.detach(), c0.detach(), labels, boxes, lens, first, *self._params())
        L, K = self.l_output_size, self.gmm_comp_num
        Q = K * self.gmm_param_num
        l_outputs = [trace[:, t, :L] for t in range(T)]
        xy = [tuple(trace[:, t, L + i * K:L + (i + 1) * K] for i in range(6)) for t in range(T)]
        wh = [tuple(trace[:, t, L + Q + i * K:L + Q + (i + 1) * K] for i in range(6)) for t in range(T)]
        sequence = [o.detach().topk(1)[1].squeeze(1) for o in l_outputs]
        # 'length': the decode steps of each caption's targets (one host read; this route is not the fused one)
        ret_dict = {DecoderRNN.KEY_SEQUENCE: sequence, DecoderRNN.KEY_LENGTH: lens.tolist(),
                    DecoderRNN.KEY_XYS: [], DecoderRNN.KEY_WHS: []}
        return l_outputs, xy, wh, None, ret_dict

    def _init_state(self, encoder_hidden):
        return tuple(self._cat_directions(h) for h in encoder_hidden)

    def _cat_directions(self, h):
        """(#directions, B, H) -> (1, B, #directions * H) for a bidirectional encoder"""
        if self.bidirectional_encoder:
            h = torch.cat([h[0:h.size(0):2], h[1:h.size(0):2]], 2)
        return h

    def forward(self, encoder_hidden=None, encoder_outputs=None, target_l_variables=None, target_x_variables=None,
                target_y_variables=None, target_w_variables=None, target_h_variables=None, is_training=0,
                early_stop_len=None, noise=None, rng=None, trace=False):
        """encoder_hidden: (h_n, c_n) of the encoder for B captions.  Returns the reference's five values; the first
        three (label softmax [B, T, L], xy and wh mixture parameters [B, T, 6K]) only with trace=True, the decoder's
        final state never (None).  ret_dict holds, per caption, 'sequence' (label indices, the <eos> step included),
        'length' (steps taken), 'xy' and 'wh' (lists of float64 pairs)."""
        if is_training:
            if target_l_variables is None or target_x_variables is None:
                raise NotImplementedError("is_training=1 without targets: free-running training of the box generator "
                                          "is out of scope here; pass the target sequences (teacher forcing)")
            return self._forward_train(encoder_hidden, target_l_variables, target_x_variables, target_y_variables,
                                       target_w_variables, target_h_variables)
        if encoder_hidden is None or early_stop_len is None:
            raise ValueError("the sampling path needs the encoder's (h_n, c_n) and early_stop_len")
        h0, c0 = (s[0] for s in self._init_state(encoder_hidden))
        B, T = h0.shape[0], int(early_stop_len)
        if noise is None:
            noise = draw_noise(rng, B, T)
        noise = torch.as_tensor(noise, dtype=torch.float64).to(h0.device)
        if tuple(noise.shape) != (B, T, 6):
            raise ValueError("noise must be [B, early_stop_len, 6]")
        out = ops.box_decode(h0, c0, noise, self._weights(), (self.x_mean, self.y_mean, self.w_mean, self.r_mean),
                             self.l_sos_id, self.l_eos_id, trace=trace)
        labels, lengths, samples = (t.cpu().numpy() for t in out[:3])
        ret_dict = {DecoderRNN.KEY_SEQUENCE: [labels[b, :lengths[b]].astype(np.int64) for b in range(B)],
                    DecoderRNN.KEY_LENGTH: lengths.tolist(),
                    DecoderRNN.KEY_XYS: [[(s[0], s[1]) for s in samples[b, :lengths[b]]] for b in range(B)],
                    DecoderRNN.KEY_WHS: [[(s[2], s[3]) for s in samples[b, :lengths[b]]] for b in range(B)]}
        if not trace:
            return None, None, None, None, ret_dict
        L, Q = self.l_output_size, self.gmm_comp_num * self.gmm_param_num
        tr = out[3]
        return tr[:, :, :L], tr[:, :, L:L + Q], tr[:, :, L + Q:], None, ret_dict
