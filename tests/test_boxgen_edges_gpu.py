"""fp64 edge-shape parity of the box generator kernels on the MI355X: csrc/box_train.hip (forward, loss, BPTT, reduce,
clip) and csrc/box_decode.hip.

Parametrised over the tables of tests/boxgen_edge_cases.py (which branch every case reaches is proven on the host in
tests/test_boxgen_edges_cpu.py).  Every training case compares the trace, the per-caption sums, every row of dtrace and
all 17 gradients with the float64 restatement: e_k = max |kernel - ref64| / max |ref64| per block must stay within
M[family] * max(e_o, 2^-23), e_o being the same figure of the fp32 restatement, and every tensor within TO.BOUND in
rel_l2; each observed figure goes to the parity log of conftest.note().  Counts, zeros past a (clamped) length, the
N = 0 batch, bit-equality under cpw 1, 2, 4 and 8 and from run to run, the clip's divisor of its own norm and the first
maximum of a tie are asserted as equalities.  The allocator is NaN-poisoned before every test (conftest) and the
gradient buffers are NaN-filled by the runner, so an unwritten element fails here.

What the cases are there to catch, tried as one-line changes of the kernels on a scratch copy (first catching case each):
    bt_loss_kernel's step loop reduced to one trip             train:T70-second-lane-trip (rows 64.. of dtrace stay NaN; also T256)
    the `nraw >= 1e-5f` test of gn dropped in bt_pdf           train:norm-clamp-K1-tuned, the ONLY case, and only through its
                                                                 tuned rows of dtrace (dtrace[0,6].wh is 0.66 off in both families; the 17 summed
                                                                 gradients stay inside their bound, 12.9 as without the change)
    `64 + 2 * K` -> `64 + K` in bt_heads_bwd_kernel            train:T70-second-lane-trip (every case: d2 is never written)
    zero fill of the trace started at max(len, 1)              train:T70-second-lane-trip (row 0 of its zero-length caption stays
                                                                 NaN; every case with a zero length)
    `hi` unclamped in bt_sumsq_kernel                          clip:n257 (the norm is NaN: the element past the arena is poison; run
                                                                 against n257 alone, the other n would read further past it)
    `oi < bi` dropped from the decode butterfly                decode:tie-across-lanes-4-69, the ONLY case: tie-across-lanes-5-70 of
                                                                 the issue passes, lane 0 meets the lane that holds 5 in the last
                                                                 exchange and takes the smaller index either way; 4-69 was added
    `v > bv` -> `v >= bv` in the decode's lane loop            decode:tie-same-lane-3-67
    the `t < len[c]` guard on the dh write of bt_bptt_kernel   no case, and none can: dg of a caption is all zero until its own
      dropped                                                    last step (the kernel clears it and writes it only under
                                                                 `t < len[c]`), so the unguarded write stores the +0 that dh holds
dtrace is compared twice, row by row and segment by segment: the chain's own against the restatement's (family
box_loss), and that of the loss entry point alone, fed the restatement's trace rounded to fp32, against the fp64 loss of
that rounded trace (family box_loss_alone; why the first needs M = 32 is written beside M in tests/boxgen_edge_cases.py).
"""
import pytest
import torch

import boxgen_edge_cases as E
from conftest import note

pytestmark = pytest.mark.gpu


def _ops():
    from objgan_hip import ops
    return ops


@pytest.mark.parametrize("case", E.TRAIN_CASES, ids=[c["id"] for c in E.TRAIN_CASES])
def test_train_edge_case_matches_fp64(dev, case):
    E.check_train_case(_ops(), dev, case, note=note)


def test_bits_do_not_depend_on_cpw(dev):
    """B = 11 with zero lengths: trace, dtrace, sums and all 17 gradients under cpw 1, 2, 4 and 8, bit for bit (every
    caption's chain and the reduce order are independent of CPW in the code)"""
    E.check_cpw_invariance(_ops(), dev, E.train_case(E.CPW_INVARIANT))


def test_empty_batch_through_ops(dev):
    """B = 0: an empty trace, sums == 0, gradients of zeros, no error and no launch"""
    ops = _ops()
    case = E.train_case("H16-one-full-wave")
    H, L, K, A, T = case["H"], case["L"], case["K"], case["A"], 3
    W = [w.to(dev) for w in E.to_kernel_layout(E.random_state(H, L, K, A, 1))]
    lab = torch.zeros((0, T + 1), dtype=torch.int32, device=dev)
    box = torch.zeros((0, T + 1, 4), device=dev)
    ln = torch.zeros((0,), dtype=torch.int32, device=dev)
    h0 = torch.zeros((0, H), device=dev)
    trace, ws = ops.box_train_forward(h0, h0, lab, box, ln, W, E.FIRST, cpw=4)
    assert tuple(trace.shape) == (0, T, L + 12 * K)
    sums, dtrace = ops.box_train_loss(trace, lab, box, ln, torch.ones(L, device=dev), 1.0, 1.0, K)
    assert tuple(sums.shape) == (1,) and float(sums[0]) == 0.0 and tuple(dtrace.shape) == tuple(trace.shape)
    grads = ops.box_train_backward(dtrace, trace, h0, lab, ln, W, ws, cpw=4)
    torch.cuda.synchronize()
    assert len(grads) == 17 and all(not g.any() for g in grads)
    out = ops.box_decode(h0, h0, torch.zeros((0, T, 6), dtype=torch.float64, device=dev), W, E.FIRST, E.SOS, E.EOS,
                         trace=True, cpw=8)
    assert [tuple(t.shape) for t in out] == [(0, T), (0,), (0, T, 4), (0, T, L + 12 * K)]


@pytest.mark.parametrize("case", E.CLIP_CASES, ids=[c["id"] for c in E.CLIP_CASES])
def test_clip_edge_case(dev, case):
    E.check_clip_case(_ops(), dev, case, note=note)


@pytest.mark.parametrize("case", E.DECODE_CASES, ids=[c["id"] for c in E.DECODE_CASES])
def test_decode_edge_case(dev, case):
    E.check_decode_case(_ops(), dev, case, note=note)


def test_decode_refuses_the_first_tile_beyond_the_lds(dev):
    """bd_launch's own LDS check (the entry point returns for B = 0 before it): the real shape under cpw = 8 is refused
    before any launch, cpw = 4 runs; the restated formula of boxgen_edge_cases says the same"""
    from objgan_hip import _lib
    ops = _ops()
    H, L, K, A = 256, 83, 5, 50
    assert E.decode_lds_bytes(H, L, K, A, 8) > E.LDS_BYTES >= E.decode_lds_bytes(H, L, K, A, 4)
    W = [w.to(dev) for w in E.to_kernel_layout(E.random_state(H, L, K, A, 2, 0.05))]
    h0 = torch.zeros((1, H), device=dev)
    noise = torch.full((1, 1, 6), 0.5, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.ObjganHipError):
        ops.box_decode(h0, h0, noise, W, E.FIRST, E.SOS, E.EOS, cpw=8)
    labels, lens, samples = ops.box_decode(h0, h0, noise, W, E.FIRST, E.SOS, E.EOS, cpw=4)
    torch.cuda.synchronize()
    assert int(lens[0]) == 1 and bool(torch.isfinite(samples).all())
