"""CPU: the buffer layouts of ``guarded.py`` themselves.  A wrong size in a shared helper would be an out-of-bounds write
on the GPU in every kernel test at once, so the total words, the offset of ``ptr`` and the stride of every class are held
to literals worked out by hand from the constructors each class replaced (cited as file:line of commit 1640cf6); then
``untouched()`` must see one word written into each region outside the payload, ``same()`` must be bitwise, and
``twice`` must refuse what it exists to refuse -- on a Python stand-in for the launch."""

import inspect

import numpy as np
import pytest
import torch

from guarded import DEV, GAP, GUARD, SLAB_GAP, FlatOut, Payload, RowOut, SlabOut, twice

CPU = "cpu"
F64, I32 = torch.float64, torch.int32


def _addr(o):
    return o.ptr if isinstance(o.ptr, int) else o.ptr.value


def test_sizes_of_guard_and_gaps_and_the_default_device():
    assert (GUARD, GAP, SLAB_GAP, DEV) == (64, 8, 96, "cuda")
    for cls in (RowOut, FlatOut, SlabOut, Payload):
        assert inspect.signature(cls).parameters["device"].default == "cuda"


# (constructor arguments, total words, byte offset of ptr, stride in words)
ROW = [
    (dict(rows=2, c=3, ld=5, extra=1), 79, 0, 5),             # test_layer_kernels_gpu.py:46  (2 + 1) * 5 + 64;  :50 ptr = buf
    (dict(rows=2, c=3), 70, 0, 3),                            # test_pool_act_kernels_gpu.py:41  2 * 3 + 64;  :45
    (dict(rows=4, c=3, extra=2, dtype=F64), 82, 0, 3),        # test_layer_kernels_gpu.py:46  (4 + 2) * 3 + 64, any float dtype
]
FLAT = [
    (dict(numel=5, off=3, slabs=2, stride=7), 81, 12, 7),     # dense_guarded.py:49  3 + 7 * 2 + 64;  :50 ptr = buf + 4 * 3
    (dict(numel=5, off=3), 72, 12, 5),                        # dense_guarded.py:48-50  stride = numel:  3 + 5 + 64
    (dict(numel=5, off=1, front=GUARD), 134, 260, 5),         # test_dense_diag_kernels_gpu.py:28  64 + 1 + 5 + 64;  :29 4 * (64 + 1)
    (dict(numel=5, front=GUARD), 133, 256, 5),                # test_bn_adjoint_split_gpu.py:36  5 + 2 * 64;  :40 4 * 64
    (dict(numel=5, off=1, dtype=I32), 70, 4, 5),              # test_dense_session_kernels_gpu.py:56-58  1 + 5 + 64;  4 * 1
    (dict(numel=5, off=1, dtype=F64), 70, 8, 5),              # test_dense_session_kernels_gpu.py:58  element_size * off
]
SLAB = [
    (dict(numel=6, splits=2), 336, 256, 104),                 # test_conv_kernels_gpu.py:88  8 + 96;  :89 2 * 64 + 2 * 104;  :90
    (dict(numel=8, splits=1), 232, 256, 104),                 # test_diag_sq_kernels_gpu.py:51-53  8 + 96;  128 + 104
    (dict(numel=9, splits=3), 452, 256, 108),                 # test_conv_kernels_gpu.py:88-90  12 + 96;  128 + 3 * 108
]


@pytest.mark.parametrize("cls, table", [(RowOut, ROW), (FlatOut, FLAT), (SlabOut, SLAB)], ids=lambda v: getattr(v, "__name__", ""))
def test_words_ptr_offset_and_stride_are_the_replaced_constructors(cls, table):
    for kw, words, ptr_off, stride in table:
        o = cls(device=CPU, **kw)
        assert o.buf.numel() == words, kw
        assert _addr(o) - o.buf.data_ptr() == ptr_off, kw
        assert (o.w if cls is RowOut else o.stride) == stride, kw
        assert o.buf.dtype == kw.get("dtype", torch.float32) and o.pristine() and o.untouched(), kw
    if cls is SlabOut:
        assert isinstance(o.ptr, int) and o.ptr % 16 == 0 and int(o.inside.sum()) == 3 * 9 and o.inside.numel() == 452


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_payload_layout(dtype):
    g = Payload(np.arange(5, dtype=dtype), device=CPU)   # test_pcg_kernels_gpu.py:53-58  64 + 5 + 64; t = buf[64:69], aligned
    assert g.buf.numel() == 133 and g.before.size == 133 and g.size == 5
    assert g.t.data_ptr() - g.buf.data_ptr() == 64 * np.dtype(dtype).itemsize and g.t.data_ptr() % 16 == 0
    assert np.array_equal(g.before[64:69], np.arange(5)) and np.isnan(g.before[:64]).all() and np.isnan(g.before[69:]).all()
    e = g.expect(np.array([[9, 8, 7, 6, 5]]))            # test_pcg_kernels_gpu.py:63-66  payload at [64, 69), the rest kept
    assert np.array_equal(e[64:69], [9, 8, 7, 6, 5]) and np.isnan(e[:64]).all() and np.isnan(e[69:]).all() and e.dtype == dtype


def _regions(o, payload, outside, value=1.0):
    """Writing the payload keeps ``untouched()``; one word at each index of ``outside``, one at a time, does not."""
    payload(o)
    assert o.untouched() and not o.pristine()
    for k in outside:
        keep = o.buf[k].clone()
        o.buf[k] = value
        assert not o.untouched(), k
        o.buf[k] = keep
        assert o.untouched(), k


def test_row_form_sees_the_ld_gap_an_extra_row_and_the_guard():
    o = RowOut(2, 3, ld=5, extra=1, device=CPU)
    assert o.val.shape == (2, 3)
    # [r0: 0 1 2 | 3 4] [r1: 5 6 7 | 8 9] [extra row 10..14] [guard 15..78]
    _regions(o, lambda o: o.val.fill_(1.0), (3, 4, 8, 9, 10, 14, 15, 78))
    o = RowOut(2, 3, dtype=F64, device=CPU)
    _regions(o, lambda o: o.val.fill_(1.0), (6, 69))


def test_flat_form_sees_the_words_before_off_the_gap_between_slabs_and_both_guards():
    o = FlatOut(5, 3, 2, 7, device=CPU)
    assert o.body.shape == (2, 5) and o.val.shape == (5,)
    # [0 1 2] [slab 0: 3..7 | 8 9] [slab 1: 10..14 | 15 16] [guard 17..80]
    _regions(o, lambda o: o.body.fill_(1.0), (0, 2, 8, 9, 15, 16, 17, 80))
    o = FlatOut(6, 1, front=GUARD, shape=(2, 3), device=CPU)
    assert o.val.shape == (2, 3)
    # [front guard 0..63] [64] [65..70] [guard 71..134]
    _regions(o, lambda o: o.val.fill_(1.0), (0, 63, 64, 71, 134))


def test_flat_form_of_an_integer_dtype_keeps_minus_seven():
    o = FlatOut(2, 1, dtype=I32, device=CPU)
    assert bool((o.buf == -7).all()) and o.pristine()
    _regions(o, lambda o: o.val.fill_(0), (0, 3, 66), value=0)
    o.val.fill_(-7)
    assert o.pristine()


def test_slab_form_sees_the_round_up_the_gap_and_both_guards():
    o = SlabOut(6, 2, device=CPU)
    assert o.slabs().shape == (2, 6)
    # [guard 0..63] [slab 0: 64..69 | 70 71 | gap 72..167] [slab 1: 168..173 | 174..271] [guard 272..335]
    _regions(o, lambda o: o.slabs().fill_(1.0), (0, 63, 70, 71, 72, 167, 174, 271, 272, 335))
    assert bool(o.inside[64:70].all()) and bool(o.inside[168:174].all()) and int(o.inside.sum()) == 12


def test_payload_form_sees_both_guards():
    g = Payload(np.zeros(5, np.float32), device=CPU)
    assert g.untouched() and g.pristine()
    g.t.fill_(2.0)
    assert g.untouched() and not g.pristine()
    assert np.array_equal(g.after(), g.expect(np.full(5, 2.0, np.float32)), equal_nan=True)
    for k in (0, 63, 69, 132):
        g.buf[k] = 1.0
        assert not g.untouched(), k
        g.buf[k] = float("nan")
        assert g.untouched(), k


@pytest.mark.parametrize("make", [lambda: RowOut(1, 2, device=CPU), lambda: FlatOut(2, 1, device=CPU),
                                  lambda: SlabOut(2, 1, device=CPU), lambda: RowOut(1, 2, dtype=F64, device=CPU)],
                         ids=["row", "flat", "slab", "row-float64"])
def test_same_is_bitwise(make):
    a, b = make(), make()
    assert a.same(b)
    lo = 64 if isinstance(a, SlabOut) else 1 if isinstance(a, FlatOut) else 0   # (a payload word)
    a.buf[lo], b.buf[lo] = 0.0, -0.0
    assert a.buf[lo] == b.buf[lo] and not a.same(b)
    b.buf[lo] = 0.0
    assert a.same(b)
    bits = a.buf.view(torch.int32 if a.buf.element_size() == 4 else torch.int64)
    bits[-1] += 1                                                               # (a guard NaN with another payload)
    assert bool(torch.isnan(a.buf[-1])) and a.untouched() and not a.same(b)


def test_twice_on_a_stand_in_launch():
    def launch(step=iter(range(100)), drift=0, spill=False, pair=False):
        o = FlatOut(4, 1, device=CPU)
        o.val.copy_(torch.arange(4.0) + drift * next(step))
        if spill:
            o.buf[-1] = 0.0
        return (o, None) if pair else o

    assert torch.equal(twice(launch).val, torch.arange(4.0))
    first, none = twice(lambda: launch(pair=True))
    assert none is None and torch.equal(first.val, torch.arange(4.0))
    with pytest.raises(AssertionError, match="differ"):
        twice(lambda: launch(drift=1))
    with pytest.raises(AssertionError, match="differ"):
        twice(lambda: launch(drift=1, pair=True))
    with pytest.raises(AssertionError, match="guard"):
        twice(lambda: launch(spill=True))
    with pytest.raises(AssertionError, match="guard"):
        twice(lambda: launch(spill=True, pair=True))
