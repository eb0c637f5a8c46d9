"""Box generator (reference box_generation/seq2seq): caption -> label and box sequence on the gfx950 kernels.
Sampling: csrc/lstm.hip, csrc/box_decode.hip.  Training: csrc/box_train.hip, seq2seq/{loss,optim,trainer}."""
