import torch


class Optimizer(object):
    """A torch optimizer behind the reference's `Optimizer(optim, max_grad_norm)` / `step()` (reference
    box_generation/seq2seq/optim/optim.py): `step()` clips the global gradient norm of every parameter the optimizer
    holds to max_grad_norm (0 = no clipping), then steps.  That is the host route, on the parameters' .grad.  The fused
    training step keeps parameters, gradients and Adam moments in flat device arenas and exchanges moments and step
    count with `self.optimizer` through seq2seq.trainer.FusedBoxStep (load_optimizer / store_optimizer), so a
    checkpoint holds an ordinary torch.optim.Adam state.  The reference never sets a learning-rate scheduler on the
    box generator; `scheduler` stays None and exists for its log line."""

    def __init__(self, optim, max_grad_norm=0):
        self.optimizer = optim
        self.max_grad_norm = max_grad_norm
        self.scheduler = None

    def step(self):
        if self.max_grad_norm > 0:
            params = [p for group in self.optimizer.param_groups for p in group['params']]
            torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        self.optimizer.step()
