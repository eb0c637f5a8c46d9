"""fp64 edge-shape parity of the norm, attention, pooling, resize, optimiser, LSTM, ROIAlign and lift-stem kernels on the
MI355X.

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
    `total <= ROI_SEQ` -> `<` in the butterfly loop of        roi:unstaged-n_e-above-1024 (dfeat 0.26 off: a pixel with exactly
      roi_align_bwd_gather_kernel (a pixel summed twice)        24 taps; every case with at_seq in its table entry has one)
    `g.w >> 8` -> `g.x` in the global-memory tap              roi:unstaged-rois-interleaved-1-0-1-0 (the ONLY case: the other
                                                                unstaged cases have one image, where list position = roi index)
    `nc` -> `cpb` in the s_g index                            roi:C70-cpb8-last-slab-nc6 (run without the C68 case, where the
                                                                changed index leaves the 4096 floats of s_g)
    `p >= W + 1` term dropped from `touched`                  roi:unstaged-n_e-above-1024 (dfeat 0.09 off)
    LIFT_MAXE 7                                               lift_taps:rows-3-to-8-longest-8 (dz only: the eighth entry dropped)
    `r >= n_out` reflection dropped in _lift_axis_tables      lift_taps:rows-3-to-8-longest-8 (y and dz)
ROIAlign besides: the forward bit-equal to the C oracle; the atomic scatter (objgan_roi_align_backward, which the ordered
entry point falls back to) against fp64 on the inputs of every table-path case, not only against the ordered kernel; the
ordered backward twice with equal bits; exact zeros wherever the fp64 reference has one.
"""
import ctypes

import pytest
import torch

import kernel_edge_cases as K
from conftest import note

pytestmark = pytest.mark.gpu

ALL = K.all_cases()
REJECTED = ([("attn_general", c) for c in K.ATTN_GENERAL_REJECTED] + [("masked_max", c) for c in K.MASKED_MAX_REJECTED] +
            [("roi", c) for c in K.ROI_REJECTED] + [("lift_taps", c) for c in K.LIFT_TAPS_REJECTED])
ROI_TABLE = [c for c in K.ROI_CASES if c["table"]]


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
    """L > 16, an idf without a kernel, R > MM_RMAX, AH * AW > 256, AH < 2, four roi columns, a map with one row or one
    column and SH < 2 return BAD_ARGS from the C entry point before any launch; a lift whose table has a row longer than
    LIFT_MAXE is refused by the host before the call"""
    from objgan_hip import _lib
    K.check_rejected(_DevOps(), dev, (fam, case), _lib.ObjganHipError)


def _roi_scatter(gtop, rois, case):
    """objgan_roi_align_backward, the atomic scatter, called as test_roi_align_backward_is_bit_reproducible calls it"""
    from objgan_hip import _lib
    B, C, H, W = case["B"], case["C"], case["H"], case["W"]
    gtop, rois = gtop.contiguous(), rois.contiguous()
    out = torch.zeros(B, C, H, W, device=gtop.device)
    _lib.call("objgan_roi_align_backward", gtop.data_ptr(), rois.data_ptr(), out.data_ptr(), B, rois.shape[0], 5, C, H, W,
              case["AH"], case["AW"], float(case["scale"]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ROI_TABLE, ids=[c["id"] for c in ROI_TABLE])
def test_roi_scatter_matches_fp64_and_the_ordered_backward_repeats_its_bits(dev, case):
    K.check_roi_backward_paths(_DevOps(), dev, case, _roi_scatter, note=note)
