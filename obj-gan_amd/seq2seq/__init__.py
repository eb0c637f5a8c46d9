"""Box generator, sampling path (reference box_generation/seq2seq): caption -> label and box sequence on the gfx950
kernels (csrc/lstm.hip, csrc/box_decode.hip).  Training the box generator is out of scope."""
