"""CPU: every case of ``conv_loop_refs.py`` against the library's planner (``hf_conv2d_nhwc_plan_info``).  The cases are
named for the steps one workgroup walks in the K loop of the 64 x 64 kernels; the planner, not the case, decides that
number -- a retuned planner fails HERE, without a GPU, instead of silently moving a case of
``test_conv_loop_gpu.py`` to another branch of the loop."""

import numpy as np
import pytest

import conv_loop_refs as lr
import conv_refs as cr
from pytorchhessianfree_amd import _lib

_IDS = [c.name for c in lr.CASES]


@pytest.fixture(scope="module")
def infos():
    return {c.name: cr.plan_infos(c, _lib.conv_plan_info) for c in lr.CASES}


@pytest.mark.parametrize("case", lr.CASES, ids=_IDS)
def test_planner_gives_the_share_the_case_is_named_for(case, infos):
    assert not case.tickets and all(p.splits == 0 for p in case.problems)  # the planner's own split count
    for p, want, got in zip(case.problems, case.expect, infos[case.name]):
        have = cr.Expect(got["config"], got["scalar"], got["cls_taps"], got["live_taps"], got["splits"],
                         -(-got["steps"] // got["splits"]))
        assert have == want, (p, have, want)
        assert want.config == 0 and not want.scalar  # the Small configuration's vector bodies
        assert got["live_taps"] == len(cr.live_taps(p))
        if want.cls_taps:
            assert want.cls_taps == cr.class_taps(p)
        assert -(-got["steps"] // got["splits"]) * (got["splits"] - 1) < got["steps"]  # no share without a step


def test_the_table_reaches_every_branch_of_the_loop(infos):
    """Forward / data gradient: 6, 7, 8 and 12 steps (every residue modulo the plain ring's 3), the last share shorter
    than the others; weight gradient: odd and even step counts in the first round of the pipelined ring and after
    several; a ragged last channel step and ragged rows; dead taps; residue classes with different share lengths; the
    merged forms with mixed share lengths; the BNSUM epilogue."""
    shares = {"nt0": set(), "nt1": set(), "tn": set()}
    short_last = set()
    for case in lr.CASES:
        for p, i in zip(case.problems, infos[case.name]):
            body = "tn" if p.d == 2 else "nt%d" % p.d
            shares[body] |= set(lr.share_lengths(i))
            per = -(-i["steps"] // i["splits"])
            if not i["ncls"] and i["steps"] - per * (i["splits"] - 1) < per:
                short_last.add((body, per))
    for body in ("nt0", "nt1"):
        assert {6, 7, 8, 12} <= shares[body], (body, shares[body])
        assert (body, 6) in short_last and (body, 12) in short_last
    assert {1, 3, 5, 6, 7} <= shares["tn"], shares["tn"]
    assert {s % lr.RING for s in shares["tn"] if s > lr.RING} == set(range(lr.RING))  # every exit of the unrolled ring
    by_name = {c.name: c for c in lr.CASES}
    # ragged last channel step: the gathered channel count a multiple of 4 but not of 32; rows not a multiple of 64
    for name in ("loop_nt_forward_6_steps_last_share_5", "loop_nt_dgrad_7_steps", "loop_nt_forward_12_steps"):
        (p,) = by_name[name].problems
        cs, rows = (p.c, p.k)[p.d], p.n * (p.h * p.w if p.d else int(np.prod(cr.out_hw(p))))
        assert cs % 4 == 0 and cs % 32 and rows % 64
    for name in ("loop_tn_5_steps_ragged_rows", "loop_tn_6_steps_ragged_rows", "loop_tn_7_steps_ragged_rows"):
        (p,) = by_name[name].problems
        assert (p.n * int(np.prod(cr.out_hw(p)))) % 32
    # a 3 x 3 window on a 2 x 2 map, with and without taps the host drops
    assert infos["loop_nt_forward_2x2_map"][0]["live_taps"] == 9
    assert infos["loop_nt_forward_2x2_map_dead_taps"][0]["live_taps"] == 4
    assert infos["loop_nt_dgrad_2x2_map_dead_taps"][0]["live_taps"] == 4
    # residue classes with different share lengths
    cls = lr.share_lengths(infos["loop_nt_dgrad_residue_classes"][0])
    assert len(set(cls)) >= 3 and max(cls) == 6, cls
    assert infos["loop_nt_dgrad_strided_plain"][0]["ncls"] == 0
    # merged forms: share lengths differ inside one launch
    for name in ("loop_pair_6_and_3_steps", "loop_pair_12_and_7_steps", "loop_group_of_four_mixed",
                 "loop_group_cls_with_plain", "loop_bnsum_group_mixed"):
        lens = [lr.share_lengths(i) for i in infos[name]]
        assert len({max(s) for s in lens}) >= 2, (name, lens)
    assert len(by_name["loop_group_of_four_mixed"].problems) == 4
    assert {c.form for c in lr.CASES} == {"slabs", "dw_slabs", "group_slabs", "group_slabs_bnsum"}


def test_the_scatter_carrying_case_and_the_product_geometries_plan_small():
    p, want = lr.UNPACK
    got = _lib.conv_plan_info(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad)
    have = cr.Expect(got["config"], got["scalar"], got["cls_taps"], got["live_taps"], got["splits"],
                     -(-got["steps"] // got["splits"]))
    assert have == want and got["steps"] - want.per * (want.splits - 1) < want.per  # (a shorter last share)
    for p in lr.PRODUCT_GEOMETRIES:
        got = _lib.conv_plan_info(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad)
        assert got["config"] == 0 and not got["scalar"] and not got["ncls"], p


@pytest.mark.parametrize("case", lr.CASES, ids=_IDS)
def test_inputs_are_exact(case):
    for idx, p in enumerate(case.problems):
        assert cr.exact(p), p
        if case.sums and case.sums[idx]:
            assert cr.bn_exact(p), p
    assert cr.exact(lr.UNPACK[0])
