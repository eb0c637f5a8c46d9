import torch
import torch.nn as nn

from objgan_hip import ops


class PreEncoderRNN(nn.Module):
    """The box generator's caption encoder (reference box_generation/seq2seq/models/PreEncoderRNN.py): the network of
    model.RNN_ENCODER with the reference's batch-first return values.  Same constructor arguments and state-dict keys
    (`encoder.weight`, `rnn.weight_ih_l0`, ..., `rnn.bias_hh_l0_reverse`); nn.Embedding / nn.LSTM hold the parameters,
    the pass is one launch of objgan_lstm_bidir_forward_state.  Forward only, eval-mode dropout (identity).

    forward(captions [B, L] int64, cap_lens) -> output [B, L, nhidden], (h_n, c_n) each [2, B, nhidden / 2].
    Captions need not be sorted by length (the kernel walks every caption on its own)."""

    def __init__(self, ntoken, ninput=300, drop_prob=0.5, nhidden=128, nlayers=1, bidirectional=True):
        super(PreEncoderRNN, self).__init__()
        if nlayers != 1 or not bidirectional:
            raise NotImplementedError("the kernel evaluates the reference default: a 1-layer bidirectional LSTM")
        self.ntoken = ntoken
        self.ninput = ninput
        self.drop_prob = drop_prob
        self.nlayers = nlayers
        self.bidirectional = bidirectional
        self.rnn_type = 'LSTM'
        self.num_directions = 2
        self.nhidden = nhidden // self.num_directions
        self.encoder = nn.Embedding(self.ntoken, self.ninput)
        self.drop = nn.Dropout(self.drop_prob)
        self.rnn = nn.LSTM(self.ninput, self.nhidden, self.nlayers, batch_first=True,
                           dropout=self.drop_prob, bidirectional=self.bidirectional)
        self.encoder.weight.data.uniform_(-0.1, 0.1)
        self._packed = None

    def _weights(self):
        """[2][I][4H] / [2][H][4H] transposed copies, rebuilt when a weight tensor was replaced or edited"""
        r = self.rnn
        srcs = (r.weight_ih_l0, r.weight_ih_l0_reverse, r.weight_hh_l0, r.weight_hh_l0_reverse,
                r.bias_ih_l0, r.bias_ih_l0_reverse, r.bias_hh_l0, r.bias_hh_l0_reverse)
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                wt_ih = torch.stack((srcs[0].t(), srcs[1].t())).contiguous()
                wt_hh = torch.stack((srcs[2].t(), srcs[3].t())).contiguous()
                b_ih = torch.stack((srcs[4], srcs[5])).contiguous()
                b_hh = torch.stack((srcs[6], srcs[7])).contiguous()
            self._packed = (key, wt_ih, wt_hh, b_ih, b_hh)
        return self._packed[1:]

    def forward(self, captions, cap_lens):
        if self.training and self.drop_prob > 0:
            raise NotImplementedError("PreEncoderRNN is frozen (the reference never trains it): call .eval()")
        wt_ih, wt_hh, b_ih, b_hh = self._weights()
        lens = torch.as_tensor(cap_lens, dtype=torch.int32)
        out, hn, cn = ops.lstm_bidir_forward(self.encoder.weight.detach(), captions, lens, wt_ih, wt_hh, b_ih, b_hh,
                                             captions.shape[1], return_cn=True)
        B, H = captions.shape[0], self.nhidden
        return out.transpose(1, 2), (hn.view(B, 2, H).transpose(0, 1), cn.view(B, 2, H).transpose(0, 1))
