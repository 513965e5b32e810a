"""GPU: every instantiation of the implicit-GEMM convolution kernels (``hf_conv.hip``) that the launchers can dispatch,
through the C ABI, against the float64 references of ``conv_refs.py`` -- EXACTLY.  The operands are small integers, so
every partial sum of every split in any order is an exactly representable integer (``conv_refs`` states the
condition): the result must equal the reference at every element, whatever kernel, split count or summation order the
planner chose.  ``test_conv_refs_cpu.py`` asserts on the CPU that the table reaches every instantiation.

Every output lies between GUARD NaN sentinels; slabs are GAP floats apart (``slab_stride`` larger than the tensor) and
the gaps are NaN too.  After a launch: guards and gaps untouched; every slab completely written (a residue class without
taps and a split without steps write zeros) except the entries of a weight gradient's dead taps, which the kernels leave
to the caller -- those, and only those, keep the sentinel, and the reference is zero there; the sum of the slabs IS the
reference; a second launch on the same buffers (recycled tickets and workspace) gives the same bits.  In ticket mode
the workspace beyond ``ws_bytes`` and the counters beyond ``n_tickets`` are sentinels that survive, and the counters
are back at zero.  The merged launches write bitwise what the single launches of their problems write."""

import pytest
import torch

import conv_harness as ch
import conv_refs as cr
from conv_harness import PTR, Out, _bits, _expect_plan, _geo, _info, _ops, _st, _twice
from guarded import DEV, GUARD, NAN
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
_BY_FORM = {form: [c for c in cr.CASES if c.form == form] for form in {c.form for c in cr.CASES}}


def _ids(cases):
    return [c.name for c in cases]


class Scratch:
    """Workspace of ``ws_bytes`` and ``n_tickets`` zeroed counters, each between sentinels."""

    def __init__(self, ws_bytes, n_tickets):
        self.ws_bytes, self.n_tickets = ws_bytes, n_tickets
        self.floats = -(-ws_bytes // 4)
        self.ws = torch.full((2 * GUARD + self.floats,), NAN, device=DEV)
        self.tk = torch.full((2 * GUARD + n_tickets,), -7, dtype=torch.int32, device=DEV)
        self.tk[GUARD:GUARD + n_tickets] = 0
        self.ws_ptr, self.tk_ptr = self.ws.data_ptr() + 4 * GUARD, self.tk.data_ptr() + 4 * GUARD
        assert self.ws_ptr % 16 == 0

    def check(self, what):
        assert bool(torch.isnan(self.ws[:GUARD]).all()) and bool(torch.isnan(self.ws[GUARD + self.ws_bytes // 4:]).all()), \
            "%s: the workspace was written outside its ws_bytes" % what
        assert bool((self.tk[:GUARD] == -7).all()) and bool((self.tk[GUARD + self.n_tickets:] == -7).all()), \
            "%s: a ticket counter outside n_tickets was written" % what
        assert not bool(self.tk[GUARD:GUARD + self.n_tickets].any()), "%s: the ticket counters are not back at zero" % what


def _launch_tickets(p, out, sc, target):
    ops = _ops(p)[1]
    assert not p.mat_ld
    _lib.check(_lib.load().hf_conv2d_nhwc(
        p.d, PTR(out.ptr), PTR(ops["act"].data_ptr()), PTR(ops["mat"].data_ptr()), *_geo(p), p.act_ld,
        PTR(sc.ws_ptr), sc.ws_bytes, PTR(sc.tk_ptr), sc.n_tickets, target, _lib.HF_F32, _st()), "hf_conv2d_nhwc")


@pytest.mark.parametrize("case", _BY_FORM["slabs"], ids=_ids(_BY_FORM["slabs"]))
def test_slab_launch_equals_float64_exactly(case):
    ch.slab_launch_equals_float64_exactly(case)


@pytest.mark.parametrize("case", _BY_FORM["tickets"], ids=_ids(_BY_FORM["tickets"]))
def test_ticket_launch_equals_float64_exactly(case):
    """``hf_conv2d_nhwc``: the last workgroup to arrive at a tile sums the splits' partial tiles from the workspace."""
    _expect_plan(case)
    (p,), (ws_bytes, n_tickets, target) = case.problems, case.tickets
    out, sc = Out(p, 1), Scratch(ws_bytes, n_tickets)
    _twice(lambda: _launch_tickets(p, out, sc, target), [out], case.name, [sc])
    info = _info(p, case.tickets)
    if info["splits"] > 1:  # (the partial tiles really went through the workspace)
        bm, bn = cr.TILE[info["config"]]
        used = info["splits"] * info["tiles_m"] * info["tiles_n"] * bm * bn
        assert used * 4 <= ws_bytes
        assert not bool(torch.isnan(sc.ws[GUARD:GUARD + used]).any())
        assert bool(torch.isnan(sc.ws[GUARD + used:]).all())


@pytest.mark.parametrize("case", _BY_FORM["backward"], ids=_ids(_BY_FORM["backward"]))
def test_ticket_pair_equals_the_single_launches_and_float64(case):
    """``hf_conv2d_nhwc_backward``: each half plans with half of the workspace and half of the counters."""
    _expect_plan(case)
    d, w = case.problems
    ws_bytes, n_tickets, target = case.tickets
    outs, sc = [Out(d, 1), Out(w, 1)], Scratch(ws_bytes, n_tickets)
    od, ow = _ops(d)[1], _ops(w)[1]
    assert torch.equal(od["act"], ow["mat"].view_as(od["act"]))  # one dY

    def launch():
        _lib.check(_lib.load().hf_conv2d_nhwc_backward(
            PTR(outs[0].ptr), PTR(outs[1].ptr), PTR(od["act"].data_ptr()), PTR(ow["act"].data_ptr()),
            PTR(od["mat"].data_ptr()), *_geo(d), PTR(sc.ws_ptr), sc.ws_bytes, PTR(sc.tk_ptr), sc.n_tickets, target,
            _lib.HF_F32, _st()), "hf_conv2d_nhwc_backward")

    merged = _twice(launch, outs, case.name, [sc])
    for idx, (p, m) in enumerate(zip(case.problems, merged)):
        half = cr.scratch_of(case, idx)
        out, sc1 = Out(p, 1), Scratch(half[0], half[1])
        (single,) = _twice(lambda: _launch_tickets(p, out, sc1, target), [out], "%s, single %d" % (case.name, idx), [sc1])
        assert torch.equal(_bits(m), _bits(single))


_PAIRS = _BY_FORM["backward_slabs"] + _BY_FORM["dw_slabs"]


@pytest.mark.parametrize("case", _PAIRS, ids=_ids(_PAIRS))
def test_slab_pair_equals_the_single_launches_and_float64(case):
    ch.slab_pair_equals_the_single_launches_and_float64(case)


@pytest.mark.parametrize("case", _BY_FORM["group_slabs"], ids=_ids(_BY_FORM["group_slabs"]))
def test_grouped_launch_equals_the_single_launches_and_float64(case):
    ch.grouped_launch_equals_the_single_launches_and_float64(case)


@pytest.mark.parametrize("case", _BY_FORM["group_slabs_bnsum"], ids=_ids(_BY_FORM["group_slabs_bnsum"]))
def test_bnsum_launch_equals_the_single_launches_and_exact_partial_sums(case):
    ch.bnsum_launch_equals_the_single_launches_and_exact_partial_sums(case)
