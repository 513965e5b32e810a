"""GPU: every branch of the gather / scatter kernels between per-layer buffers and the flat CG vector -- ``k_pack``
(``hf_pack_ex``), ``k_unpack_tangent`` (``hf_unpack_weights``) and ``k_live_copy`` (``hf_live_copy``) -- against the
bitwise numpy references of ``pack_refs.py``, and the refusals of the three entry points.

Nothing here has a tolerance: mode 0 is one rounded multiply, mode 1 three roundings, a split source is summed in split
order in its own type, the library is built without contraction, and unpack / live-copy only move values.  Every
destination lies between GUARD NaN sentinels on each side that must survive; every entry a kernel must not read (dead
taps, the gaps between slabs, one whole slab behind the last) is NaN, so reading it shows.  ``test_pack_refs_cpu.py``
checks with a mirror of the kernels' predicates that the case tables reach every branch."""

import zlib

import numpy as np
import pytest

import pack_refs as pr
from guarded import ERR_ARG, GUARD, NAN, P, Payload, dev, st
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
_CODE = {np.float32: _lib.HF_F32, np.float64: _lib.HF_F64}
_DT_IDS = [np.dtype(d).name for d in pr.DTYPES]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _i64(vals):
    return (_lib.c_int64 * len(vals))(*vals)


def _diff(got, want):
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    if bad.size == 0:
        return "equal"
    k = int(bad[0])
    return f"{bad.size} of {got.size} entries differ, first at {k - GUARD} (payload index): {got[k]!r} != {want[k]!r}"


# ---- k_pack ------------------------------------------------------------------------------------------------------------
def _params(cases):
    return [pytest.param(c, dt, id=f"{c.name}-{np.dtype(dt).name}") for c in cases for dt in c.dtypes]


def _check_pack(case, dtype, mode):
    bufs, sources = pr.make_sources(case, dtype, _seed(case.name))
    size = np.dtype(dtype).itemsize
    tensors, perms, splits, live = [], {}, {}, {}
    for i, (buf, s) in enumerate(zip(bufs, case.srcs)):
        t = dev(buf)[s.src_off:s.src_off + s.numel]
        assert s.numel == 0 or t.data_ptr() % 16 == s.src_off * size % 16
        tensors.append(t)
        if s.perm:
            perms[i] = s.perm
        if s.nsplit > 1:
            splits[i] = (s.nsplit, s.stride or s.numel)
        if s.live:
            live[i] = s.live
    n = sum(s.numel for s in case.srcs)
    rng = np.random.RandomState(_seed(case.name, "dst"))
    for scale in pr.SCALES:
        # mode 0 overwrites every entry (NaN shows one that it left), mode 1 adds to random values
        before = rng.standard_normal(n).astype(dtype) if mode == 1 else np.full(n, NAN, dtype)
        dst = Payload(before)
        _lib.pack_ex(dst.t, tensors, perms, splits, scale=scale, live=live, mode=mode)
        want = pr.pack_ref(before, sources, scale, mode)
        assert not np.isnan(want).any()
        got = dst.after()
        assert pr.same(got, dst.expect(want)), (scale, _diff(got, dst.expect(want)))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,dtype", _params(pr.SPLIT_CASES))
def test_pack_of_split_sources_is_the_scaled_sum_in_split_order(case, dtype, mode):
    """Staged, unstaged and plain 16-byte paths and the generic path of ``nsplit > 1``: every batch depth of the slab
    loops, both chunk rules, the swizzle of the staging tile, a live mask with NaN in the dead taps of every slab."""
    _check_pack(case, dtype, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,dtype", _params(pr.SINGLE_CASES))
def test_pack_of_single_slabs_is_the_scaled_unpermuted_source(case, dtype, mode):
    """The zero stream and the fallback walk of the live-mask path, the tiled and the direct un-permuting path, the
    plain copies; aligned and odd destination offsets."""
    _check_pack(case, dtype, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,dtype", _params(pr.TABLE_CASES))
def test_pack_across_the_table_boundary(case, dtype, mode):
    """64 non-empty tensors fill one argument table exactly; the 65th, a split tensor, goes into a second launch.  Empty
    tensors between them take no table entry but keep their place in the offsets."""
    assert sum(s.numel > 0 for s in case.srcs) == (65 if case.name == "table_65" else 64)
    _check_pack(case, dtype, mode)


# ---- k_unpack_tangent --------------------------------------------------------------------------------------------------
def _unpack(v, slots, halves, dtype):
    """Launches ``hf_unpack_weights`` for ``slots`` (pack_refs.Slot) with one half per slot; returns per slot the
    guarded buffer and its logical view."""
    guarded, views, tables = [], [], []
    for s, h in zip(slots, halves):
        O, I, H, W = s.shape
        g = Payload(np.full(O * I * H * W * (1 if h == 2 else 2), NAN, dtype))
        if h == 2:
            view = g.t.view(I, H, W, O)
        elif s.nhwc:
            view = g.t.view(O, H, W, 2 * I).permute(0, 3, 1, 2)
        else:
            view = g.t.view(O, 2 * I, H, W)
        tab = _lib.unpack_table(v, [(s.off, view, I, s.live)], h)
        if h != 2:
            tab[4][0] = I if s.nhwc else 0  # (a 1x1 kernel's buffer is NCHW- and NHWC-contiguous at once)
        assert view.data_ptr() % 16 == 0
        guarded.append(g)
        views.append(view)
        tables.append(tab)
    n = len(slots)
    dsts = (P * n)(*[tab[0][0] for tab in tables])
    cols = [_i64([tab[c][0] for tab in tables]) for c in range(1, 7)]
    _lib.check(_lib.load().hf_unpack_weights(P(v.data_ptr()), dsts, *cols, n, _CODE[dtype], st()), "hf_unpack_weights")
    return guarded, views


def _check_unpack(v_host, slots, halves, dtype):
    v = dev(v_host)
    guarded, views = _unpack(v, slots, halves, dtype)
    for s, h, g, view, want in zip(slots, halves, guarded, views, pr.unpack_ref(v_host, slots, halves)):
        got = view.cpu().numpy()
        assert pr.same(got, want), (s, h, _diff(got.reshape(-1), want.reshape(-1)))
        after = g.after()
        assert np.isnan(after[:GUARD]).all() and np.isnan(after[after.size - GUARD:]).all(), (s, h)
    assert pr.same(v.cpu().numpy(), v_host)


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=_DT_IDS)
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_centre", "nhwc_corner"])
def test_unpack_moves_the_slices_into_the_halves(layout, shift, half, dtype):
    """``shift`` 0: slices at 16-byte aligned places of the vector, the 16-byte loops of ``unpack_block`` (and the
    scalar ones for the 3-channel shape); ``shift`` 1: the scalar loops for every shape.  Dead slices keep the NaN."""
    live = {"nhwc_centre": pr.CENTRE, "nhwc_corner": pr.CORNER}.get(layout, 0)
    slots, n = pr.unpack_slots(shift, layout != "nchw", live)
    v_host = np.random.RandomState(_seed(layout, shift)).standard_normal(n).astype(dtype)
    _check_unpack(v_host, slots, [half] * len(slots), dtype)


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=_DT_IDS)
def test_unpack_of_halves_0_1_and_2_in_one_launch(dtype):
    """A ``halves`` array: W halves, v_W halves and a ragged transposed copy (70 x 45: no multiple of the 64 x 64 tile)
    side by side in one launch."""
    shapes = [((24, 16, 3, 3), True, 0), (pr.UNPACK_RAGGED_SHAPE, False, 2), ((5, 8, 2, 3), False, 1),
              ((8, 3, 3, 3), True, 1), ((5, 8, 2, 3), True, 0), (pr.UNPACK_RAGGED_SHAPE, False, 2)]
    slots, halves, off = [], [], 4
    for k, (sh, nhwc, h) in enumerate(shapes):
        slots.append(pr.Slot(off, sh, nhwc, pr.CORNER if k == 0 else 0))
        halves.append(h)
        off += int(np.prod(sh)) + (k % 2)
    v_host = np.random.RandomState(_seed("halves")).standard_normal(off + 3).astype(dtype)
    _check_unpack(v_host, slots, halves, dtype)


# ---- k_live_copy -------------------------------------------------------------------------------------------------------
def _live_copy(full, comp, scatter, segs, dtype, n_segments=None):
    cols = [_i64([s[c] for s in segs]) for c in range(4)]
    return _lib.load().hf_live_copy(P(full.data_ptr()), P(comp.data_ptr()), scatter, *cols,
                                    len(segs) if n_segments is None else n_segments, _CODE[dtype], st())


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=_DT_IDS)
@pytest.mark.parametrize("name", list(pr.LIVE_LAYOUTS))
def test_live_copy_gathers_and_scatters_exactly_the_live_entries(name, dtype):
    """Dense segments through the 16-byte branch with its tail and through the scalar one, one-tap and many-tap
    periodic segments, 24 segments (the limit): gather equals indexing, scatter into a NaN-filled vector restores
    exactly the gathered entries and nothing else."""
    segs, n = pr.LIVE_LAYOUTS[name]
    full_host = np.random.RandomState(_seed(name)).standard_normal(n).astype(dtype)
    idx = pr.live_index(segs)
    full, comp = Payload(full_host), Payload(np.full(idx.size, NAN, dtype))
    assert _live_copy(full.t, comp.t, 0, segs, dtype) == 0
    got, want = comp.after(), comp.expect(pr.live_copy_ref(full_host, segs))
    assert pr.same(got, want), _diff(got, want)
    assert full.pristine()
    target = Payload(np.full(n, NAN, dtype))
    assert _live_copy(target.t, comp.t, 1, segs, dtype) == 0
    restored = np.full(n, NAN, dtype)
    restored[idx] = full_host[idx]
    got, want = target.after(), target.expect(restored)
    assert pr.same(got, want), _diff(got, want)
    assert pr.same(comp.after(), comp.expect(full_host[idx]))


# ---- refusals ----------------------------------------------------------------------------------------------------------
_PACK_OK = dict(numel=72, I=4, HW=9, count=1, stride=0, mode=0, dtype=_lib.HF_F32, null_src=False)
_PACK_REFUSED = {
    "split_count_0": dict(count=0),
    "stride_below_numel": dict(count=2, stride=71),
    "numel_no_multiple_of_the_slab": dict(I=5),
    "hw_0": dict(HW=0),
    "mode_2": dict(mode=2),
    "dtype_7": dict(dtype=7),
    "negative_numel": dict(numel=-1),
    "null_source": dict(null_src=True),
}


def _pack_call(dst, src, a):
    srcs = (P * 1)(None if a["null_src"] else src.data_ptr())
    return _lib.load().hf_pack_ex(P(dst.data_ptr()), srcs, _i64([a["numel"]]), _i64([a["I"], a["HW"]]),
                                  _i64([a["count"], a["stride"]]), _i64([0]), 1, 0.5, a["mode"], a["dtype"], st())


@pytest.mark.parametrize("fault", list(_PACK_REFUSED))
def test_pack_ex_refuses(fault):
    src = dev(np.ones(2 * 72, np.float32))
    ok = Payload(np.full(72, NAN, np.float32))
    assert _pack_call(ok.t, src, _PACK_OK) == 0  # (the call every row differs from in one argument)
    assert pr.same(ok.after(), ok.expect(np.full(72, 0.5, np.float32)))
    dst = Payload(np.full(72, NAN, np.float32))
    assert _pack_call(dst.t, src, {**_PACK_OK, **_PACK_REFUSED[fault]}) == ERR_ARG
    assert dst.pristine()


_UNPACK_OK = dict(null_dst=False, off=4, numel=72, slab=18, inner=0, half=1)
_UNPACK_REFUSED = {
    "null_dst": dict(null_dst=True),
    "negative_offset": dict(off=-1),
    "slab_0": dict(slab=0),
    "numel_no_multiple_of_the_slab": dict(slab=7),
    "slab_no_multiple_of_the_inner_count": dict(inner=4),
    "half_2_without_inner_count": dict(half=2),
}


def _unpack_call(v, dst, a):
    dsts = (P * 1)(None if a["null_dst"] else dst.data_ptr())
    return _lib.load().hf_unpack_weights(P(v.data_ptr()), dsts, _i64([a["off"]]), _i64([a["numel"]]), _i64([a["slab"]]),
                                         _i64([a["inner"]]), _i64([0]), _i64([a["half"]]), 1, _lib.HF_F32, st())


@pytest.mark.parametrize("fault", list(_UNPACK_REFUSED))
def test_unpack_weights_refuses(fault):
    v_host = np.arange(80, dtype=np.float32)
    v = dev(v_host)
    ok = Payload(np.full(144, NAN, np.float32))
    assert _unpack_call(v, ok.t, _UNPACK_OK) == 0
    want = np.full((4, 2, 18), NAN, np.float32)
    want[:, 1] = v_host[4:76].reshape(4, 18)
    assert pr.same(ok.after(), ok.expect(want.reshape(-1)))
    dst = Payload(np.full(144, NAN, np.float32))
    assert _unpack_call(v, dst.t, {**_UNPACK_OK, **_UNPACK_REFUSED[fault]}) == ERR_ARG
    assert dst.pristine()


_DENSE25 = [(4 * k, 4, 0, 0) for k in range(25)]
_LIVE_REFUSED = {  # segments, n_segments
    "segments_0": ([(0, 36, 9, pr.CENTRE)], 0),
    "segments_25": (_DENSE25, 25),
    "period_17": ([(0, 34, 17, 1)], 1),
    "count_no_multiple_of_the_period": ([(0, 35, 9, pr.CENTRE)], 1),
    "mask_outside_the_period": ([(0, 36, 9, 1 << 9)], 1),
    "count_0": ([(0, 0, 0, 0)], 1),
}


@pytest.mark.parametrize("scatter", [0, 1])
@pytest.mark.parametrize("fault", list(_LIVE_REFUSED))
def test_live_copy_refuses(fault, scatter):
    full_host = np.arange(100, dtype=np.float32)
    ok_full, ok_comp = Payload(full_host), Payload(np.full(100, NAN, np.float32))
    assert _live_copy(ok_full.t, ok_comp.t, 0, [(0, 36, 9, pr.CENTRE)], np.float32) == 0
    assert _live_copy(ok_full.t, ok_comp.t, 0, _DENSE25[:24], np.float32) == 0  # (24 segments are the limit)
    assert pr.same(ok_comp.after()[GUARD:GUARD + 96], full_host[:96])
    full, comp = Payload(full_host), Payload(np.full(100, NAN, np.float32))
    segs, n_segments = _LIVE_REFUSED[fault]
    assert _live_copy(full.t, comp.t, scatter, segs, np.float32, n_segments) == ERR_ARG
    assert full.pristine() and comp.pristine()
