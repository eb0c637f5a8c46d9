"""fp64 parity of the convolution launch plans the small shapes never reach, on the MI355X: tall forward tiles, the rest
launch, 8-wave workgroups, two pixel groups per wave, the four-phase and ring data gradients, the multi-part weight
gradient -- the cases of tests/conv_plan_cases.py (which plan every case reaches is proven on the host in
tests/test_conv_plans_cpu.py), one (case, arithmetic) per test.

Every test records the arguments of the size queries objgan_hip.ops makes during the call and requires them to be the
tuples the plans were proven for (the plan that ran is the plan that was proven), then compares y, dx, dw (db) of one
ops.conv2d forward + backward with the float64 reference: e_k = max |kernel - ref64| / max |ref64| within
M[tensor, arithmetic] * max(e_o, 2^-23), e_o being the same figure of the fp32 oracle, and rel_l2 < 1e-4; each observed
figure goes to the parity log of conftest.note().  The allocator is NaN-poisoned before every test (conftest), so an
unwritten row group fails here.

What the cases are there to catch, tried as value-only changes on a scratch copy, each run once (first failing case;
which of the older convolution tests of test_kernels_gpu.py / test_fullsize_gpu.py fail as well):
    the rest launch (m_begin > 0) drops its last K step          fwd-tm3x4-rest1-cout388 [fp32]; 28 tests, every case with
        a rest launch (older: only the adjoint identity of test_fullsize_gpu.py case0; CONV_CASES, X3_CASES, REC_CASES pass)
    conv_igemm3_kernel<5> scales its fifth row group by 1 + 2^-10   fwd-tm5-cout129-reflect-3x3 [fp32]; 16 tests, the four
        cases with a TM 5 launch (older: none fails)
    the second pixel group of an ng = 2 wave stores the first group's accumulator   ring-rec-ng2-tm1-cin65 [fp16x2-rec]; the
        four ng 2 cases (older: three REC_CASES bit-identity cases and three adjoint cases; CONV_CASES, X3_CASES pass)
    the combine of a weight gradient's second part reads from slot offset 0   fwd-tm7x2-cout417 [fp32]; 22 tests, every
        two-part weight gradient (older: CONV_CASES case19, X3_CASES case1, REC_CASES and the reproducibility test fail too)
"""
import pytest
import torch

import conv_plan_cases as P
from conftest import note

pytestmark = pytest.mark.gpu

PAIRS = [(c, a) for c in P.CASES for a in P.ARITHS]
PAIR_IDS = ["%s-%s" % (c["id"][:60], a) for c, a in PAIRS]


@pytest.fixture(scope="module", autouse=True)
def _references_do_not_outlive_the_module():
    yield
    P.release()


def _ops():
    from objgan_hip import ops
    return ops


@pytest.fixture
def arithmetic(request):
    """The arithmetic of a test, set up as the fp32_math fixture of test_kernels_gpu.py does: fp32, bf16x3, fp16x2 with
    the FLOP threshold at zero and records off, fp16x2 with every launch (and every eligible weight gradient) on records."""
    ops = _ops()
    arith = request.param
    prev, prev_min, prev_rec = ops.get_conv_math(), ops._H2_MIN_FLOP, dict(ops._REC)
    ops.set_conv_math({"fp16x2-rec": "fp16x2"}.get(arith, arith))
    ops._H2_MIN_FLOP = 0.0
    ops._REC["min_i"] = ops._REC["min_i_short"] = 0.0
    ops._REC["wgrad"] = "all"
    ops._REC["wgrad_math"] = 5
    ops.set_h2_records(arith == "fp16x2-rec")
    yield arith
    ops.set_conv_math(prev)
    ops._H2_MIN_FLOP = prev_min
    ops._REC.update(prev_rec)


@pytest.mark.parametrize("case,arithmetic", PAIRS, ids=PAIR_IDS, indirect=["arithmetic"])
def test_conv_plan_case_matches_fp64(dev, case, arithmetic):
    ops = _ops()
    from objgan_hip import _lib
    lib, q = _lib.load(), ops._q
    # the library this test runs plans what the table states (host-only, as in the CPU file) ...
    assert P.plans_of(lib, case, arithmetic, q) == P.PLANS[case["id"]][arithmetic]
    want = P.expected_queries(case, arithmetic, q)
    asked = []

    def recording(name, *args):
        if name in (P.IGEMM_Q, P.PHASES_Q, P.WGRAD_Q):
            asked.append((name,) + tuple(args))
        return q(name, *args)

    ops._q = recording
    failed, had_max = None, None
    try:
        _, had_max = P.check_case(ops, dev, case, arithmetic, note=note)
    except AssertionError as e:
        failed = e
    finally:
        ops._q = q
    # ... and the call asked for exactly the launches those plans were proven for
    assert asked == want, (asked, want)
    if failed is not None:
        raise failed
    if case["geo"][11] == "lrelu" and arithmetic.startswith("fp16x2"):
        assert had_max, "the LeakyReLU epilogue left no partial maxima on y"
