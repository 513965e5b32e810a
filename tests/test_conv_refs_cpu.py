"""CPU: the case table of ``conv_refs.py`` against the library's own planner (``hf_conv2d_nhwc_plan_info``: host
arithmetic through ``plan_problem``, the function every launching entry point of ``hf_conv.hip`` runs), the exactness
condition of its inputs, and -- as an assertion -- that the table reaches every kernel instantiation the launchers can
dispatch.  A planner tuning that moves a case to another instantiation fails HERE, without a GPU, and the message names
the instantiation that lost its test.  ``test_conv_kernels_gpu.py`` runs the same table on the kernels."""

import numpy as np
import pytest
import torch

import conv_refs as cr
from pytorchhessianfree_amd import _lib

_IDS = [c.name for c in cr.CASES]

# Every instantiation that launch_one / launch_dw / launch_group of hf_conv.hip can dispatch (launch_unpack's two are
# covered by test_conv_gpu's test of hf_conv2d_nhwc_slabs_unpack), written out: the table must hit each.
INSTANTIATIONS = [
    # launch_one, forward / data gradient
    "k_conv_nt<scalar,Small>", "k_conv_nt<Small>", "k_conv_nt<Big>", "k_conv_nt<Big96>",
    "k_conv_nt<Small,CLS>", "k_conv_nt<Big,CLS>", "k_conv_nt<Big96,CLS>",
    # launch_one, weight gradient
    "k_conv_tn<scalar,Small>", "k_conv_tn<Small>", "k_conv_tn<Big>", "k_conv_tn<Big96>", "k_conv_tn<Flat96>",
    # launch_dw
    "k_conv_dw<ANYBIG=0,CLS=0>", "k_conv_dw<ANYBIG=0,CLS=1>", "k_conv_dw<ANYBIG=1,CLS=0>", "k_conv_dw<ANYBIG=1,CLS=1>",
    # launch_group
    "k_conv_group<ANYBIG=0,CLS=0>", "k_conv_group<ANYBIG=0,CLS=1>", "k_conv_group<ANYBIG=1,CLS=0>",
    "k_conv_group<ANYBIG=1,CLS=1>", "k_conv_group<BNSUM>", "k_conv_nt<Small,BNSUM>",
]
# ... and the bodies inside the merged kernels that only one side or one problem of a launch selects
BODIES = [
    "k_conv_dw<ANYBIG=0,CLS=0>/nt<Small>", "k_conv_dw<ANYBIG=0,CLS=0>/tn<Small>",
    "k_conv_dw<ANYBIG=0,CLS=1>/nt<Small,CLS>",
    "k_conv_dw<ANYBIG=1,CLS=0>/nt<Small>", "k_conv_dw<ANYBIG=1,CLS=0>/tn<Flat96>",      # only the w side is 128-wide
    "k_conv_dw<ANYBIG=1,CLS=1>/nt<Big,CLS>", "k_conv_dw<ANYBIG=1,CLS=1>/tn<Small>",      # only the d side is
    "k_conv_group<ANYBIG=0,CLS=0>/1 problems", "k_conv_group<ANYBIG=0,CLS=0>/4 problems",
    "k_conv_group<ANYBIG=0,CLS=1>/2 problems", "k_conv_group<ANYBIG=1,CLS=0>/3 problems",
    "k_conv_group<ANYBIG=0,CLS=1>/nt<Small,CLS>", "k_conv_group<ANYBIG=0,CLS=1>/tn<Small>",
    "k_conv_group<ANYBIG=0,CLS=1>/nt<Small,CLS>:plain",                                   # a problem with ncls == 0
    "k_conv_group<ANYBIG=1,CLS=0>/nt<Big>", "k_conv_group<ANYBIG=1,CLS=0>/nt<Small>",    # a Small problem under ANYBIG
    "k_conv_group<ANYBIG=1,CLS=0>/tn<Flat96>",
    "k_conv_group<ANYBIG=1,CLS=1>/nt<Big,CLS>", "k_conv_group<ANYBIG=1,CLS=1>/tn<Small>",
    "k_conv_group<ANYBIG=1,CLS=1>/nt<Small,CLS>:plain",
    "k_conv_group<BNSUM>/nt<Small,BNSUM>", "k_conv_group<BNSUM>/nt<Small>",
    # every argument slot of k_conv_group, the weight-gradient body and the forward / data-gradient body in each of
    # the first three
    "k_conv_group/slot 0 nt", "k_conv_group/slot 0 tn", "k_conv_group/slot 1 nt", "k_conv_group/slot 1 tn",
    "k_conv_group/slot 2 nt", "k_conv_group/slot 2 tn", "k_conv_group/slot 3 tn",
]
# ring phases: steps of one workgroup on the hand-counted prefetch ring
PHASES = [(body, "Small", steps) for body in ("nt", "tn") for steps in (1, 2, 3, 4, 5)] + \
         [("nt", "Big", 50), ("nt", "Big", 15), ("nt", "Big", 20), ("nt", "Big", 11), ("nt", "Big96", 17),
          ("tn", "Big", 18), ("tn", "Big96", 18), ("tn", "Flat96", 8), ("tn", "Flat96", 16)]


@pytest.fixture(scope="module")
def infos():
    return {c.name: cr.plan_infos(c, _lib.conv_plan_info) for c in cr.CASES}


@pytest.mark.parametrize("case", cr.CASES, ids=_IDS)
def test_table_matches_the_planner(case, infos):
    """Configuration, scalar gathers, residue classes with their tap counts, live taps, splits and steps per split of
    every problem are what the table says; the class tap counts and the live taps also equal a brute-force count."""
    for p, want, got in zip(case.problems, case.expect, infos[case.name]):
        have = cr.Expect(got["config"], got["scalar"], got["cls_taps"], got["live_taps"], got["splits"],
                         -(-got["steps"] // got["splits"]))
        assert have == want, (p, have, want)
        assert got["ncls"] == len(want.cls_taps)
        assert got["live_taps"] == len(cr.live_taps(p))
        if want.cls_taps:
            assert want.cls_taps == cr.class_taps(p)
            assert got["steps"] == max(want.cls_taps) * -(-p.k // cr.BK[want.config]) or max(want.cls_taps) == 0
        bm, bn = cr.TILE[want.config]
        oh, ow = cr.out_hw(p)
        if p.d == 2:
            cols = (-(-got["live_taps"] * p.c // bn) if want.config == 3 else got["live_taps"] * -(-p.c // bn))
            assert (got["tiles_m"], got["tiles_n"]) == (-(-p.k // bm), cols)
            assert got["steps"] == -(-p.n * oh * ow // cr.BK[want.config])
        elif not want.cls_taps:
            rows, nout = (p.n * oh * ow, p.k) if p.d == 0 else (p.n * p.h * p.w, p.c)
            assert (got["tiles_m"], got["tiles_n"]) == (-(-rows // bm), -(-nout // bn))
        assert got["blocks"] == got["tiles_m"] * got["tiles_n"] * got["splits"]
        # (no split without a step: what a slab-mode launch demands of the caller's count)
        assert -(-got["steps"] // got["splits"]) * (got["splits"] - 1) < got["steps"]


def test_plan_info_agrees_with_the_plan_and_refuses_like_it():
    """The new query and ``hf_conv2d_nhwc_plan`` are one planner: same split count for every slab-mode problem of the
    table, the same refusal codes for geometries neither can plan, HF_ERR_ARG for null arguments."""
    lib = _lib.load()
    for case in cr.CASES:
        for p in case.problems:
            if case.tickets or p.splits or p.act_ld or p.mat_ld:
                continue
            sp = lib.hf_conv2d_nhwc_plan(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, *p.stride, *p.pad, 0)
            assert sp == _lib.conv_plan_info(p.d, p.n, p.h, p.w, p.c, p.k, p.r, p.s, p.stride, p.pad)["splits"], p
    info, q = _lib.ConvPlanInfo(), _lib.ConvProblem()
    byref = _lib.ctypes.byref
    for geom in ((0, 2, 9, 9, 8, 8, 9, 8, 1, 1, 4, 4), (1, 2, 2, 2, 8, 8, 5, 5, 1, 1, 0, 0), (3, 32, 7, 7, 64, 64, 3, 3, 1, 1, 1, 1),
                 (0, 0, 7, 7, 64, 64, 3, 3, 1, 1, 1, 1), (2, 32, 7, 7, 64, 64, 3, 3, 0, 1, 1, 1)):
        (q.direction, q.n, q.h, q.w, q.c, q.k, q.r, q.s, q.stride_h, q.stride_w, q.pad_h, q.pad_w) = geom
        want = lib.hf_conv2d_nhwc_plan(*geom, 0)
        assert want < 0
        for ticket_mode in (0, 1):
            assert lib.hf_conv2d_nhwc_plan_info(byref(q), ticket_mode, 1 << 20, 64, 0, byref(info)) == want
    (q.direction, q.n, q.h, q.w, q.c, q.k, q.r, q.s, q.stride_h, q.stride_w, q.pad_h, q.pad_w) = (0, 2, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1)
    assert lib.hf_conv2d_nhwc_plan_info(byref(q), 0, 0, 0, 0, byref(info)) == 0
    assert lib.hf_conv2d_nhwc_plan_info(None, 0, 0, 0, 0, byref(info)) == _lib.HF_ERR_ARG
    assert lib.hf_conv2d_nhwc_plan_info(byref(q), 0, 0, 0, 0, None) == _lib.HF_ERR_ARG
    assert lib.hf_conv2d_nhwc_plan_info(byref(q), 1, -1, 64, 0, byref(info)) == _lib.HF_ERR_ARG
    # a mat_ld on a weight gradient, an out_c on a forward problem: refused as by the launches
    q.direction, q.mat_ld = 2, 8
    assert lib.hf_conv2d_nhwc_plan_info(byref(q), 0, 0, 0, 0, byref(info)) == _lib.HF_ERR_ARG
    q.direction, q.mat_ld, q.out_c = 0, 0, 4
    assert lib.hf_conv2d_nhwc_plan_info(byref(q), 0, 0, 0, 0, byref(info)) == _lib.HF_ERR_ARG


def test_every_dispatchable_instantiation_has_a_case(infos):
    hit, phases = {}, {}
    for case in cr.CASES:
        for key in cr.instantiations(case, infos[case.name]):
            hit.setdefault(key, []).append(case.name)
        for key in cr.ring_phases(case, infos[case.name]):
            phases.setdefault(key, []).append(case.name)
    lost = [key for key in INSTANTIATIONS + BODIES if key not in hit]
    assert not lost, "no case of conv_refs.CASES runs %s any more" % lost
    lost = [key for key in PHASES if key not in phases]
    assert not lost, "no case of conv_refs.CASES runs a workgroup of (body, configuration, steps) %s any more" % lost
    # each residue of the step count modulo 3 above the short forms, per vector body and tile width
    for body in ("nt", "tn"):
        for wide in (False, True):
            residues = {steps % 3 for b, cfg, steps in phases if b == body and (cfg != "Small") == wide and steps > 3}
            assert len(residues) >= 2, (body, wide, residues)
    # ticket mode: the split counts of the last arriver's four-slab unroll, remainders 0 .. 3
    splits = {infos[c.name][0]["splits"] for c in cr.CASES if c.form == "tickets"}
    assert {2, 3, 4, 5, 6, 9} <= splits
    assert {(s - 1) % 4 for s in splits if s > 4} == {0, 1, 2, 3}
    # forms
    assert {c.form for c in cr.CASES} == {"slabs", "tickets", "backward", "backward_slabs", "dw_slabs", "group_slabs",
                                          "group_slabs_bnsum"}


@pytest.mark.parametrize("case", cr.CASES, ids=_IDS)
def test_inputs_are_exact(case):
    """The exactness condition holds for every problem; operands are integers in [-3, 3] in the layouts the entry points
    take; the float64 reference (computed here where it is small) is integer-valued, below 2**24, and zero at the dead
    taps of a weight gradient; the BatchNorm sums stay exact as well."""
    for idx, p in enumerate(case.problems):
        assert cr.exact(p), p
        ops = cr.operands(p)
        for t in ops.values():
            assert t.dtype == np.float32 and np.array_equal(t, np.rint(t)) and np.abs(t).max() <= cr.VMAX
        oh, ow = cr.out_hw(p)
        cs = (p.c, p.k, p.c)[p.d]
        assert ops["act"].shape[-1] == (p.act_ld or cs)
        assert ops["mat"].shape == ((p.k, p.r, p.s, p.mat_ld or p.c), (p.c, p.r, p.s, p.mat_ld or p.k),
                                    (p.n, oh, ow, p.k))[p.d]
        assert np.array_equal(ops["act"][..., :cs], (ops["x"], ops["gy"], ops["x"])[p.d])
        if p.d == 1:
            assert np.array_equal(ops["mat"][..., :p.k], ops["wt"].transpose(3, 1, 2, 0))
        if case.sums and case.sums[idx]:
            assert cr.bn_exact(p)
            bn = cr.bn_operands(p)
            assert set(np.unique(bn["rstd"])) <= {0.5, 1.0, 2.0} and np.array_equal(bn["mean"], np.rint(bn["mean"]))
        if np.prod(cr.out_shape(p)) * cr.reduction_length(p) > 2e8:
            continue  # (the large problems: their reference is computed on the device by the GPU test)
        ref = cr.reference(p, ops)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == cr.out_shape(p)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < cr.EXACT_LIMIT
        assert float(ref.abs().max()) > 0
        if p.d == 2:
            dead = torch.from_numpy(cr.dead_mask(p))
            assert int(dead.sum()) == (p.r * p.s - len(cr.live_taps(p))) * p.k * p.c
            assert not ref[dead].any()
        if case.sums and case.sums[idx]:
            s1, sx = cr.bn_partial_ref(ref.reshape(-1, p.k).numpy(), bn)
            for s in (s1, sx):
                assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
