"""TEST INFRASTRUCTURE: CPU definitions of the shape-generator operators (`convlstm_sequence`, `box_max`,
`boxmaps_onehot`, `box_train_clip`) on top of tests/cpu_ops_shim.py, so that the host side of the feature -- model.py's
training path, miscc/shape_losses.py, shapeDataset.py, shape_trainer.py with its arenas -- runs on CPU tensors.  The
product never imports this module."""
import torch
import torch.nn.functional as F

import cpu_ops_shim


def convlstm_sequence(x, w, bias=None, reverse=False):
    """definition: the reference's cell (one convolution over [input, hidden]) step by step, autograd does the rest"""
    B, R = x.shape[0], x.shape[1]
    Ch = w.shape[0] // 4
    h = c = x.new_zeros((B, Ch) + tuple(x.shape[3:]))
    out = [None] * R
    for t in range(R):
        i, f, o, g = F.conv2d(torch.cat((x[:, t], h), 1), w, bias, 1, w.shape[2] // 2).chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[R - 1 - t if reverse else t] = h
    return torch.stack(out, 1)


def box_max(x, return_arg=False):
    y, arg = torch.max(x, 1)           # (CPU: the gradient goes to the first maximal box)
    return (y, arg.to(torch.uint8)) if return_arg else y


def boxmaps_onehot(raw, cats, num_rois, R, C):
    B, NB, S, _ = raw.shape
    full = raw.new_zeros((B, NB, C, S, S))
    for b in range(B):
        for r in range(int(num_rois[b])):
            full[b, r, int(cats[b, r])] = raw[b, r]
    return full[:, :R].contiguous(), full.flip(1)[:, :R].contiguous()


def box_train_clip(flat_grads, max_norm, partials=None, out=None):
    if out is None:
        out = torch.empty(2, dtype=torch.float32)
    norm = float(flat_grads.double().square().sum().sqrt())
    out[0] = max(1.0, (norm + 1e-6) / float(max_norm))
    out[1] = norm
    return out


def install(monkeypatch):
    """cpu_ops_shim.install, extended by the definitions above and pointed at the feature's modules too"""
    shim = cpu_ops_shim.install(monkeypatch)
    for f in (convlstm_sequence, box_max, boxmaps_onehot, box_train_clip):
        setattr(shim, f.__name__, f)
    import shape_trainer
    import shapeDataset
    from miscc import shape_losses
    for mod in (shape_trainer, shapeDataset, shape_losses):
        monkeypatch.setattr(mod, "ops", shim)
    return shim
