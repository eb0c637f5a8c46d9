"""fp64 edge-shape parity of the norm, attention, pooling, resize, optimiser and LSTM kernels on the MI355X.

Parametrised over the tables of tests/kernel_edge_cases.py (which branch every case reaches is proven on the host in
tests/test_kernel_edges_cpu.py).  Every case compares EVERY output and gradient of its operator with the float64
reference: e_k = max |kernel - ref64| / max |ref64| must stay within M[family] * max(e_o, 2^-23), e_o being the same
figure of the fp32 oracle, and within the family's rel_l2 bound; each observed figure goes to
the parity log of conftest.note().  Equalities (zeros past `lens`, cleared rows, LSTM padding, bit-equal maxima, ties) are
asserted as equalities.  The allocator is NaN-poisoned before every test (conftest), so an unwritten tail fails here.

What the cases are there to catch, tried as one-line changes of the kernels on a scratch copy (first catching case each):
    last partial slot dropped in norm_partials_sum_kernel     norm:bn-generic-2splits-boundary-inside-plane (17 norm cases)
    i1 one float4 short in norm_stats_plane_kernel            norm:in-plane-unfused-hw65540-last-chunk-one-float4 (7 cases)
    (1 - momentum) replaced by 1 on running_mean              norm:bn-generic-2splits-boundary-inside-plane (all 14 BatchNorm cases)
    `v >= best` in masked_max_bwd_kernel                      masked_max:nonzero-ties-first-max-wins
    m_stride_c ignored                                        masked_max:mask5d-per-channel-R3, -R16
    softmax_rows_fwd_kernel stores under `d < n`              softmax:rows-dim*-lens-0-1-dim-dim+3, rows-dim289-lens-and-rowvalid
"""
import ctypes

import pytest
import torch

import kernel_edge_cases as K
from conftest import note

pytestmark = pytest.mark.gpu

ALL = K.all_cases()
REJECTED = ([("attn_general", c) for c in K.ATTN_GENERAL_REJECTED] + [("masked_max", c) for c in K.MASKED_MAX_REJECTED])


class _DevOps(object):
    """objgan_hip.ops, plus the two fold kernels that only have a C entry point (called as ops.py calls them)"""

    def __getattr__(self, name):
        from objgan_hip import ops
        return getattr(ops, name)

    @staticmethod
    def _fold(entry, src, h, w):
        from objgan_hip import _lib
        src = src.contiguous()
        out = torch.empty((src.shape[0], h, w), dtype=torch.float32, device=src.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.call(entry, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), src.shape[0], h, w, stream)
        return out

    def sum2x2(self, dy, h, w):
        return self._fold("objgan_sum2x2", dy, h, w)

    def reflect_fold(self, dxp, h, w):
        return self._fold("objgan_reflect_fold", dxp, h, w)


@pytest.mark.parametrize("fam,case", ALL, ids=K.case_ids(ALL))
def test_edge_case_matches_fp64(dev, fam, case):
    K.check_case(_DevOps(), dev, fam, case, note=note)


@pytest.mark.parametrize("fam,case", REJECTED, ids=K.case_ids(REJECTED))
def test_unsupported_sizes_are_rejected(dev, fam, case):
    """L > 16, an idf without a kernel and R > MM_RMAX return BAD_ARGS from the C entry point before any launch"""
    from objgan_hip import _lib
    K.check_rejected(_DevOps(), dev, (fam, case), _lib.ObjganHipError)
