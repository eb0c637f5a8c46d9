"""The convolution plan cases of tests/conv_plan_cases.py, checked without a GPU on the built library:

  * coverage -- every launch-plan feature the table is there for is named by a case id and holds in the plan the table
    states for that case (per arithmetic);
  * branch proof -- for every (case, arithmetic) the host-only plan queries (objgan_conv_igemm_plan,
    objgan_conv_dgrad_s2_phases_plan, objgan_conv_wgrad_plan) return exactly the stated plan for the argument tuples
    `launches` derives: retuning the `pen` table of og_row_plan, og_rec_ng2_min, og_nw8_min or the 16384-pixel threshold of
    the 8-wave weight gradient fails here instead of silently moving a GPU case off its launch;
  * the queries are tied to the run: the workspace sizes objgan_conv_igemm_ws_floats / objgan_conv_wgrad_ws_floats report
    (what ops allocates, from the same plan functions the run follows) are the ones the returned plans imply;
  * reference sanity -- the fp32 oracle agrees with the fp64 reference on every case;
  * plumbing -- the body of the GPU test runs on the CPU definitions of the ops API (tests/cpu_ops_shim.py).
"""
import pytest
import torch

import conv_plan_cases as P
import cpu_ops_shim

IDS = [c["id"][:60] for c in P.CASES]
PAIRS = [(c, a) for c in P.CASES for a in P.ARITHS]
PAIR_IDS = ["%s-%s" % (c["id"][:60], a) for c, a in PAIRS]


@pytest.fixture(scope="module", autouse=True)
def _references_do_not_outlive_the_module():
    yield
    P.release()


def _lib():
    from objgan_hip import _lib
    return _lib.load()


def _q(name, *args):
    return getattr(_lib(), name)(*args)


def test_case_ids_are_unique_and_every_case_has_a_stated_plan():
    assert len(set(IDS)) == len(P.CASES) == len(P.BY_ID)
    assert set(P.PLANS) == set(P.BY_ID)
    for plan in P.PLANS.values():
        assert set(plan) == set(P.ARITHS)


@pytest.mark.parametrize("row", P.COVERAGE, ids=[r[0] for r in P.COVERAGE])
def test_every_coverage_row_is_named_by_a_case_whose_stated_plan_has_it(row):
    name, word, ariths, pred = row
    named = [c for c in P.CASES if word in c["id"]]
    assert named, "no case id names %r" % word
    for arith in ariths:
        assert any(pred(c, P.PLANS[c["id"]][arith]) for c in named), (name, arith, [c["id"] for c in named])


@pytest.mark.parametrize("case,arith", PAIRS, ids=PAIR_IDS)
def test_the_library_plans_what_the_table_states(case, arith):
    got, want = P.plans_of(_lib(), case, arith, _q), P.PLANS[case["id"]][arith]
    for launch in ("fwd", "dgrad", "wgrad"):
        assert got[launch] == want[launch], (launch, got[launch], want[launch])


@pytest.mark.parametrize("case,arith", PAIRS, ids=PAIR_IDS)
def test_workspace_queries_equal_what_the_plans_imply(case, arith):
    """one weight-gradient part or more (every case), and every forward / data-gradient launch, split or not"""
    L, plan = P.launches(case, arith, _q), P.PLANS[case["id"]][arith]
    for launch, (_, fields) in zip([L["fwd"]] + L["dgrad"], [plan["fwd"]] + plan["dgrad"]):
        if launch[0] == "phases":
            assert _q(*launch[1]) == 0                   # (four phases in one launch: never split, no operand copy)
            assert P.fields(fields)["splits"] == 1
        else:
            assert _q(*launch[1]) == P.implied_igemm_ws(launch[1], fields), launch[1]
    assert plan["wgrad"][0][9] >= 1
    assert _q(*L["wgrad"]) == P.implied_wgrad_ws(L["wgrad"], plan["wgrad"]), L["wgrad"]


def test_split_launches_are_among_the_cases():
    """the tie above is not vacuous: forward / data-gradient launches with several splits, and weight gradients whose
    second part starts behind the slots of the first"""
    nsplit = sum(1 for c, a in PAIRS for _, f in [P.PLANS[c["id"]][a]["fwd"]] + P.PLANS[c["id"]][a]["dgrad"] if P.fields(f)["splits"] > 1)
    two = sum(1 for c, a in PAIRS if len(P.PLANS[c["id"]][a]["wgrad"][1]) == 2)
    assert nsplit >= 20 and two >= 20, (nsplit, two)


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_fp32_oracle_agrees_with_the_fp64_reference_and_the_gpu_body_runs_on_the_cpu_definitions(case):
    """(one test per case, so that its references are computed once)  The conditioning check: e_o finite and below
    1e-3, rel_l2 within the bound the GPU test asserts.  Then the GPU test's body on tests/cpu_ops_shim.py."""
    ref, o32 = P.reference(case), P.oracle32(case)
    assert set(ref) == set(o32) == {"y", "dx", "dw"} | ({"db"} if case["geo"][10] else set())
    for name in ref:
        assert ref[name].dtype == torch.float64, name
        e_o = P.max_err(o32[name], ref[name])
        assert e_o == e_o and e_o < 1e-3, (name, e_o)
        assert P.rel_l2(o32[name], ref[name]) < P.RL2, (name, P.rel_l2(o32[name], ref[name]))
    seen = []
    ratios, had_max = P.check_case(cpu_ops_shim, torch.device("cpu"), case, "fp32", note=lambda k, v: seen.append((k, v)))
    assert set(ratios) == set(ref) and not had_max
    assert all(r <= 1.0 for r in ratios.values()), ratios      # (the shim IS the fp32 oracle)
    assert len(seen) == 2 * len(ref)


def test_a_wrong_row_group_fails_the_comparison_and_names_its_place():
    """the comparison notices one 32-row group of one pixel tile scaled by 1 + 2^-10, which the whole-tensor rel_l2 does
    not, and reports the row group and the tile"""
    case = P.BY_ID["fwd-tm3-cout65-last-group-1-row-3x3"]
    got = {k: v.clone() for k, v in P.oracle32(case).items()}
    got["y"][2, 32:64, 5, 0:64] *= 1.0 + 2.0 ** -10
    assert P.rel_l2(got["y"], P.reference(case)["y"]) < P.RL2
    with pytest.raises(AssertionError) as err:
        P.compare(case, "fp32", got)
    assert "row group 1" in str(err.value) and "128-pixel tile %d" % ((2 * 64 + 5) * 64 // 128) in str(err.value)
