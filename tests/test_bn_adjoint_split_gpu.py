"""GPU: the eval-mode BatchNorm adjoint split into its elementwise launch (``hf_bn_adjoint_v4`` / ``_pair``) and the
multi-problem sums launch (``hf_bn_sums_multi``), through the C ABI.

Both halves must reproduce the BITS of the fused row-major launch (``hf_chan_affine_bwd_ex`` with row shares) on the same
operands -- gres / gx resp. every partial row of gw / gb -- and the elementwise half also lies inside the float64 bound of
``layer_refs.bn_adjoint_pre`` (``r_bwd_g`` / ``r_bwd_gx``: no tolerance of its own).  Every output sits in a NaN-filled
buffer with guard words on both sides, slabs are ``GAP`` NaN words apart, and every case is launched twice."""

import ctypes

import pytest
import torch
from tol import within

import layer_refs as L
from guarded import DEV, ERR_ARG, GAP, GUARD, P, FlatOut, _ids, bits_equal, optr, ptr, slabs_dev, st, twice
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu


def rb_for(rows, c, i):
    ch = [rb for rb in L.row_block_choices(rows, c) if rb >= 2 and L.share_ok(rows, rb)]
    return ch[i % len(ch)]


# ---------------------------------------------------------------------------------------------------------------
# the elementwise launch
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [sh for sh in L.EVAL_SHAPES if sh[1] % 4 == 0 and sh != (3, 20)]
assert SHAPES == [(1568, 64), (32, 512), (200, 96), (37, 12), (5, 4), (130, 260), (64, 1024)]
EW_CASES = [(sh, sl, i) for i, (sh, sl) in enumerate((sh, sl) for sh in SHAPES for sl in L.SLAB_COUNTS)]


class Problem:
    """One elementwise problem on the device, its float64 reference and the fused launch's arguments."""

    def __init__(self, shape, slab_counts, use_mask, use_w, rb):
        (self.rows, self.c), (self.s1, self.s2) = shape, slab_counts
        o = L.eval_inputs(self.rows, self.c, self.s1, self.s2)
        mask, w = (o.mask if use_mask else None), (o.w if use_w else None)
        self.ref = L.bn_adjoint_pre(o.a, o.b, mask, w, o.rstd)
        self.mask_host = mask
        self.la, self.lb = self.rows * self.c + GAP, (self.rows * self.c + GAP if o.b is not None else 0)
        self.a, self.b = slabs_dev(o.a, self.la), slabs_dev(o.b, self.lb)
        self.mask, self.w, self.rstd = (t.to(DEV) if t is not None else None for t in (mask, w, o.rstd))
        self.rb = rb

    def outs(self):
        return tuple(FlatOut(self.rows * self.c, front=GUARD, shape=(self.rows, self.c)) for _ in range(2))

    def fused(self, lib):
        gx, gres, gb = *self.outs(), FlatOut(self.rb * self.c, front=GUARD)
        _lib.check(lib.hf_chan_affine_bwd_ex(
            gx.ptr, None, gb.ptr, gres.ptr, ptr(self.a), self.s1, self.la, ptr(self.b), self.s2 or 1, self.lb, None, None,
            ptr(self.rstd), ptr(self.w), ptr(self.mask), self.rows, self.c, 1, 1, self.rb, _lib.HF_F32, st()),
            "hf_chan_affine_bwd_ex")
        return gres, gx

    def check(self, g, ga, gres, gx):
        note = (self.rows, self.c, self.s1, self.s2)
        assert bits_equal(g.val, gres.val), f"g differs from the fused launch's gres {note}"
        assert bits_equal(ga.val, gx.val), f"ga differs from the fused launch's gx {note}"
        within(L.ratio(g.val, self.ref.g, self.ref.Mg, L.r_bwd_g(self.s1, self.s2)), 1.0, strict=False, note=note)
        within(L.ratio(ga.val, self.ref.ga, self.ref.Mga, L.r_bwd_gx(self.s1, self.s2)), 1.0, strict=False, note=note)
        if self.mask_host is not None:
            off = ~(self.mask_host > 0).to(DEV)
            assert bool((g.val[off] == 0).all()) and bool((ga.val[off] == 0).all())


@pytest.mark.parametrize("shape,slab_counts,i", EW_CASES, ids=_ids)
def test_elementwise_launch_equals_the_fused_launch_bit_for_bit(shape, slab_counts, i):
    """Every shape x every slab-count pair; each case with one (mask, w) choice and with its complement, so that every
    operand is present and absent at every shape and count.  That is two of the four (mask, w) combinations per case, not
    the full cross product: which two a (shape, count) pair gets rotates with the case number ``i``."""
    lib = _lib.load()
    for variant in (i % 4, 3 - i % 4):
        k = Problem(shape, slab_counts, bool(variant & 1), bool(variant & 2), rb_for(*shape, i))

        def launch():
            g, ga = k.outs()
            _lib.check(lib.hf_bn_adjoint_v4(g.ptr, ga.ptr, ptr(k.a), k.s1, k.la, ptr(k.b), k.s2 or 1, k.lb, ptr(k.mask),
                                            ptr(k.w), ptr(k.rstd), k.rows, k.c, _lib.HF_F32, st()), "hf_bn_adjoint_v4")
            return g, ga

        g, ga = twice(launch)
        k.check(g, ga, *k.fused(lib))


def test_elementwise_launch_with_one_output():
    lib = _lib.load()
    k = Problem((200, 96), (9, 2), True, True, 7)
    gres, gx = k.fused(lib)
    for which in (0, 1):

        def launch():
            o = k.outs()[0]
            args = (o.ptr, None) if which == 0 else (None, o.ptr)
            _lib.check(lib.hf_bn_adjoint_v4(*args, ptr(k.a), k.s1, k.la, ptr(k.b), k.s2, k.lb, ptr(k.mask), ptr(k.w),
                                            ptr(k.rstd), k.rows, k.c, _lib.HF_F32, st()), "hf_bn_adjoint_v4")
            return (o,)

        (o,) = twice(launch)
        assert bits_equal(o.val, (gres, gx)[which].val)


EW_PAIRS = [(((200, 96), (3, 1), 3), ((37, 12), (9, 2), 1)), (((130, 260), (2, 17), 2), ((5, 4), (1, None), 0)),
            (((1568, 64), (18, 1), 3), ((64, 1024), (1, 9), 3))]


@pytest.mark.parametrize("pair", EW_PAIRS, ids=_ids)
def test_elementwise_pair_equals_the_fused_launch_bit_for_bit(pair):
    """Two problems of different shapes, slab counts and operands in one launch."""
    lib = _lib.load()
    ks = [Problem(sh, sl, bool(v & 1), bool(v & 2), rb_for(*sh, 0)) for sh, sl, v in pair]

    def launch():
        arr, outs = (_lib.BnAdjointProblem * 2)(), [k.outs() for k in ks]
        for q, k, (g, ga) in zip(arr, ks, outs):
            q.gres, q.gx, q.gy, q.gy_splits, q.gy_slab = g.ptr, ga.ptr, ptr(k.a), k.s1, k.la
            q.gy2, q.gy2_splits, q.gy2_slab = ptr(k.b), k.s2 or 1, k.lb
            q.mask_src, q.w, q.rstd, q.n, q.c, q.hw = ptr(k.mask), ptr(k.w), ptr(k.rstd), k.rows, k.c, 1
        _lib.check(lib.hf_bn_adjoint_v4_pair(ctypes.cast(arr, P), _lib.HF_F32, st()), "hf_bn_adjoint_v4_pair")
        return [o for pair_ in outs for o in pair_]

    outs = twice(launch)
    for j, k in enumerate(ks):
        k.check(outs[2 * j], outs[2 * j + 1], *k.fused(lib))


# ---------------------------------------------------------------------------------------------------------------
# the multi-problem sums
# ---------------------------------------------------------------------------------------------------------------
# (rows, c, which row-block choice, form): channel counts 4 / 64 / 260 / 1024 mixed; form "b": bias only (x = NULL),
# "w": gw only, "wb": both.  Choice "small": the first accepted count whose shares are smaller than the BLOCK / (c/4) rows
# a workgroup takes per pass; "short": the first one that leaves the last share short.
SUMS_PROBLEMS = [(37, 4, "short", "wb"), (200, 64, "small", "wb"), (130, 260, "short", "b"), (64, 1024, "short", "w"),
                 (1568, 64, "small", "wb")]


class SumsProblem:
    def __init__(self, rows, c, choice, form, j):
        gen = L.gen_of("sums", rows, c, j)
        self.rows, self.c, self.form = rows, c, form
        ch = [rb for rb in L.row_block_choices(rows, c) if rb >= 2 and L.share_ok(rows, rb)]
        rp = max(256 // (c // 4), 1)
        self.rb = next(rb for rb in ch if (-(-rows // rb) < rp if choice == "small" else rows % rb))
        self.g = L.mask_like(gen, rows, c).to(DEV) * 3  # (a masked cotangent: exact zeros of both signs)
        self.x = (L.randn(gen, rows, c) * 2 + 0.5).to(DEV)
        self.mean, self.rstd = L.randn(gen, c).to(DEV), L.rstd_like(gen, c).to(DEV)
        self.bias_only = form == "b"

    def outs(self):
        n = self.rb * self.c
        return tuple(FlatOut(n, front=GUARD) if k in self.form else None for k in "wb")

    def fused(self, lib):
        gw, gb = self.outs()
        x = None if self.bias_only else self.x
        _lib.check(lib.hf_chan_affine_bwd_ex(
            None, optr(gw), optr(gb), None, ptr(self.g), 1, 0, None, 1, 0, ptr(x), ptr(self.mean), ptr(self.rstd), None,
            None, self.rows, self.c, 1, 1, self.rb, _lib.HF_F32, st()), "hf_chan_affine_bwd_ex")
        return gw, gb

    def entry(self, q, gw, gb):
        q.gw, q.gb, q.g = optr(gw), optr(gb), ptr(self.g)
        q.x = None if self.bias_only else ptr(self.x)
        q.mean, q.rstd = ptr(self.mean), ptr(self.rstd)
        q.rows, q.c, q.row_blocks = self.rows, self.c, self.rb


def build_table(lib, probs, outs):
    tab = (_lib.BnSumsProblem * len(probs))()
    for q, k, (gw, gb) in zip(tab, probs, outs):
        k.entry(q, gw, gb)
    blocks = lib.hf_bn_sums_table(ctypes.cast(tab, P), len(probs))
    assert blocks == sum(k.rb for k in probs)
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    return tab, dev


@pytest.mark.parametrize("count,first,launched", [(1, 0, 1), (2, 0, 2), (5, 0, 5), (5, 1, 3), (5, 4, 1)], ids=_ids)
def test_sums_multi_equals_the_fused_launch_bit_for_bit(count, first, launched):
    """Tables of 1, 2 and 5 problems; whole-table launches and sub-ranges (the middle of a table, its last entry).
    Every partial row equals the fused launch's at the same row_blocks; rows of problems outside the range stay NaN."""
    lib = _lib.load()
    probs = [SumsProblem(*spec, j) for j, spec in enumerate(SUMS_PROBLEMS[:count] if count > 1 else SUMS_PROBLEMS[1:2])]
    assert {k.c for k in probs} == {4, 64, 260, 1024} or count < 5
    if count == 5:  # the row-block choices named above are what they claim to be
        assert any(-(-k.rows // k.rb) < max(256 // (k.c // 4), 1) for k in probs), "no share smaller than one pass"
        assert any(k.rows % k.rb for k in probs), "no short last share"

    def launch():
        outs = [k.outs() for k in probs]
        tab, dev = build_table(lib, probs, outs)
        _lib.check(lib.hf_bn_sums_multi(dev.data_ptr(), ctypes.cast(tab, P), count, first, launched, _lib.HF_F32, st()),
                   "hf_bn_sums_multi")
        return [o for pair in outs for o in pair]

    outs = twice(launch)
    for j, k in enumerate(probs):
        gw, gb = outs[2 * j], outs[2 * j + 1]
        if first <= j < first + launched:
            fw, fb = k.fused(lib)
            torch.cuda.synchronize()
            for got, want in ((gw, fw), (gb, fb)):
                assert (got is None) == (want is None)
                assert got is None or got.same(want), f"problem {j}: partial rows differ from the fused launch's"
        else:
            assert all(o is None or o.pristine() for o in (gw, gb)), f"problem {j} is outside the range but was written"


# ---------------------------------------------------------------------------------------------------------------
# refusals: HF_ERR_ARG, nothing written
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    lib = _lib.load()
    rows = 8
    src = torch.ones(rows * 12 + 8, device=DEV)
    vec = torch.ones(16, device=DEV)
    g, ga = FlatOut(rows * 12, front=GUARD), FlatOut(rows * 12, front=GUARD)

    def v4(gp, gap, gy, c, slab=0, s1=1, rstd=vec.data_ptr()):
        return lib.hf_bn_adjoint_v4(gp, gap, gy, s1, slab, None, 1, 0, None, None, rstd, rows, c, _lib.HF_F32, st())

    assert v4(g.ptr, ga.ptr, src.data_ptr(), 6) == ERR_ARG               # c % 4 != 0
    assert v4(g.ptr, ga.ptr, src.data_ptr() + 4, 12) == ERR_ARG          # a misaligned cotangent
    assert v4(P(g.ptr.value + 4), ga.ptr, src.data_ptr(), 12) == ERR_ARG          # a misaligned output
    assert v4(g.ptr, ga.ptr, src.data_ptr(), 12, rstd=vec.data_ptr() + 4) == ERR_ARG
    assert v4(g.ptr, ga.ptr, src.data_ptr(), 12, slab=rows * 12 + 2, s1=2) == ERR_ARG  # a slab stride off the quads
    assert v4(None, None, src.data_ptr(), 12) == ERR_ARG
    arr = (_lib.BnAdjointProblem * 2)()
    for q, c in zip(arr, (12, 6)):
        q.gres, q.gx, q.gy, q.gy_splits, q.gy2_splits, q.rstd = g.ptr, ga.ptr, src.data_ptr(), 1, 1, vec.data_ptr()
        q.n, q.c, q.hw = rows, c, 1
    assert lib.hf_bn_adjoint_v4_pair(ctypes.cast(arr, P), _lib.HF_F32, st()) == ERR_ARG

    def one(rows_, c, rb, g_off=0):
        q = _lib.BnSumsProblem()
        q.gw, q.gb, q.g, q.x = g.ptr, ga.ptr, src.data_ptr() + g_off, src.data_ptr()
        q.mean, q.rstd, q.rows, q.c, q.row_blocks = vec.data_ptr(), vec.data_ptr(), rows_, c, rb
        return q

    def table(*qs):
        tab = (_lib.BnSumsProblem * len(qs))(*qs)
        return tab, lib.hf_bn_sums_table(ctypes.cast(tab, P), len(qs))

    assert table(one(8, 6, 2))[1] == ERR_ARG                              # c % 4 != 0
    assert table(one(8, 12, 2, g_off=4))[1] == ERR_ARG                    # a misaligned operand
    assert not L.share_ok(8, 7) and table(one(8, 12, 7))[1] == ERR_ARG    # an empty share
    assert table(one(8, 12, 2), one(8, 6, 2))[1] == ERR_ARG               # ... in any entry
    good, blocks = table(*(one(8, 12, 2) for _ in range(_lib.BN_SUMS_MAX + 1)))
    assert blocks == 2 * (_lib.BN_SUMS_MAX + 1)
    dev = torch.frombuffer(bytearray(bytes(good)), dtype=torch.uint8).to(DEV)
    n = len(good)

    def multi(tab, first, count, table_count=n):
        return lib.hf_bn_sums_multi(dev.data_ptr(), ctypes.cast(tab, P), table_count, first, count, _lib.HF_F32, st())

    assert multi(good, 0, n) == ERR_ARG                                   # more problems than the cap
    assert multi(good, 2, _lib.BN_SUMS_MAX) == ERR_ARG                    # count past the table
    assert multi(good, 0, 2, table_count=1) == ERR_ARG
    assert multi(good, -1, 1) == ERR_ARG and multi(good, 0, 0) == ERR_ARG
    bad = (_lib.BnSumsProblem * n)()
    ctypes.memmove(bad, good, ctypes.sizeof(bad))
    bad[1].row_blocks = 7                                                 # an entry the builder would have refused
    assert multi(bad, 0, 3) == ERR_ARG
    ctypes.memmove(bad, good, ctypes.sizeof(bad))
    bad[2].block0 += 1                                                    # derived fields that are not the builder's
    assert multi(bad, 0, 4) == ERR_ARG
    torch.cuda.synchronize()
    assert g.pristine() and ga.pristine(), "a refused call wrote something"
