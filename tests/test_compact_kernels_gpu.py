"""GPU: the gather into, the scatter from and the dead-entry check of the COMPACT layout of the flat CG vector
(``hf_pack_compact``, ``hf_unpack_weights_compact`` / ``hf_conv2d_nhwc_slabs_unpack_compact``, ``hf_live_copy_rows``,
``hf_live_dead_check``) -- bit for bit against the references of ``pack_refs`` indexed by the compact map of
``compact_refs``.  Every comparison is exact; the shapes are the smallest that reach each branch (``compact_refs.CASES``)."""

import zlib

import numpy as np
import pack_refs as pr
import pytest
import torch

import compact_refs as cr
from guarded import DEV, GUARD, NAN, P, Payload, dev
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
_CODE = {np.float32: _lib.HF_F32, np.float64: _lib.HF_F64}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _i64(vals):
    return (_lib.c_int64 * len(vals))(*[int(v) for v in vals])


# ---- gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case,dtype", [pytest.param(c, dt, id=f"{c.name}-{np.dtype(dt).name}") for c in cr.CASES
                                        for dt in c.dtypes])
def test_gather_into_the_compact_layout_is_the_compact_image_of_the_flat_gather(case, dtype, mode):
    """``hf_pack_compact`` == ``pack_ref`` (the flat gather) indexed by the compact map: every branch a masked tensor can
    take (staged, straight and direct 16-byte paths of split sources, the generic split path, the one-tap vector copy and
    the walk of single slabs), and every branch of the tensors around it at their compact offsets.  Dead taps' sources are
    NaN in every slab and are never read; the NaN guards around the compact vector stay untouched."""
    bufs, sources = cr.make_sources(case, dtype, _seed(case.name))
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
    compact = {i: nl for i, nl in enumerate(cr.periods(case.srcs)) if nl}
    assert compact
    idx = cr.compact_index(case.srcs)
    n = sum(s.numel for s in case.srcs)
    rng = np.random.RandomState(_seed(case.name, "dst"))
    for scale in (1.0, 0.3):
        # mode 0 overwrites every entry (NaN shows one that it left), mode 1 adds to what is there
        before = rng.randint(-4, 5, size=idx.size).astype(dtype) if mode == 1 else np.full(idx.size, NAN, dtype)
        flat_before = np.zeros(n, dtype)
        flat_before[idx] = before
        dst = Payload(before)
        _lib.pack_ex(dst.t, tensors, perms, splits, scale=scale, live=live, mode=mode, compact=compact)
        want = pr.pack_ref(flat_before, sources, scale, mode)[idx]
        assert not np.isnan(want).any()
        got, host = dst.after(), dst.expect(want)
        bad = np.nonzero(~((got == host) | (np.isnan(got) & np.isnan(host))))[0]
        assert bad.size == 0, (scale, bad.size, int(bad[0]) - GUARD, got[bad[0]], host[bad[0]])


def test_gather_refuses_a_period_that_is_not_the_masks():
    t = torch.zeros(3 * 8 * 9, device=DEV)
    dst = torch.zeros(3 * 8 * 9, device=DEV)
    lib = _lib.load()
    for live, period in ((pr.CENTRE, 4), (0, 1), (pr.CORNER, 9)):
        rc = lib.hf_pack_compact(P(dst.data_ptr()), (P * 1)(t.data_ptr()), _i64([t.numel()]), _i64([8, 9]), _i64([1, 0]),
                                 _i64([live]), _i64([period]), 1, 1.0, 0, _lib.HF_F32, None)
        assert rc == _lib.HF_ERR_ARG


# ---- scatter -----------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _scatter_setup(I, front, dtype):
    """A flat vector of [front | centre-masked | corner-masked | all taps | 1x1] weights [3, I, ., .] and its slots."""
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    srcs = ([pr.Src(front)] if front else []) + [pr.Src(27 * I, (I, 9), live=pr.CENTRE), pr.Src(27 * I, (I, 9), live=pr.CORNER),
                                                  pr.Src(27 * I, (I, 9)), pr.Src(3 * I)]
    shapes = [(3, I, 3, 3)] * 3 + [(3, I, 1, 1)]
    offs_c, n_live = cr.compact_offsets(srcs)
    offs_f = np.cumsum([0] + [s.numel for s in srcs])[:-1]
    k0 = 1 if front else 0
    n = int(sum(s.numel for s in srcs))
    v = np.random.RandomState(_seed("scatter", I, front)).standard_normal(n).astype(dtype)
    vc = cr.gather(v, srcs)
    assert vc.size == n_live

    def slots(compact):
        out = []
        for k, sh in enumerate(shapes):
            s = srcs[k0 + k]
            buf = _cl(torch.full((sh[0], 2 * sh[1], sh[2], sh[3]), NAN, dtype=tdt, device=DEV))
            if compact:
                out.append((int(offs_c[k0 + k]), buf, I, s.live, cr.periods(srcs)[k0 + k]))
            else:
                out.append((int(offs_f[k0 + k]), buf, I, s.live))
        return out

    return dev(v), dev(vc), slots


def _same_buffers(a, b):
    for sa, sb in zip(a, b):
        x, y = sa[1].cpu().numpy(), sb[1].cpu().numpy()
        assert pr.same(x, y), (sa[0], sb[0])
    assert any(np.isfinite(s[1].cpu().numpy()).any() for s in a)  # (the scatter really ran)


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=[np.dtype(d).name for d in pr.DTYPES])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("front", [0, 7])
@pytest.mark.parametrize("I", [8, 5])
def test_scatter_from_the_compact_layout_equals_the_flat_scatter(I, front, half, dtype):
    """``hf_unpack_weights_compact`` on ``gather(v)`` writes what ``hf_unpack_weights`` writes from ``v``: the 16-byte
    loop (I = 8, aligned offsets; one contiguous load for the one-tap mask) and the scalar loop (I = 5, or a dense tensor
    of odd length in front), both halves; dead slices keep their NaN on both sides.  Transposed copies (half 2) have no
    compact form: refused."""
    v, vc, slots = _scatter_setup(I, front, dtype)
    flat, comp = slots(False), slots(True)
    _lib.unpack_tangent(v, flat, half=half)
    _lib.unpack_tangent(vc, comp, half=half)
    _same_buffers(flat, comp)
    # half 2 with a compact period: HF_ERR_ARG
    wt = torch.empty((I, 3, 3, 3), dtype=v.dtype, device=DEV)
    tab = _lib.unpack_table(v, [(0, wt, I)], 2)
    tab[5][0] = pr.CENTRE
    rc = _lib.load().hf_unpack_weights_compact(P(vc.data_ptr()), *tab[:-1], _i64([1]), 1, _CODE[dtype], None)
    assert rc == _lib.HF_ERR_ARG


@pytest.mark.parametrize("front", [0, 7])
@pytest.mark.parametrize("I", [8, 5])
def test_stem_convolution_carrying_the_compact_scatter_equals_the_flat_one(I, front):
    """``hf_conv2d_nhwc_slabs_unpack_compact``: one tiny convolution whose launch carries the scatter from the compact
    vector -- same convolution output and same destination buffers as the launch that carries the flat scatter."""
    v, vc, slots = _scatter_setup(I, front, np.float32)
    rows, c, k = 64, 52, 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    cols = torch.randint(-3, 4, (rows, c), device=DEV, generator=gen).float()
    w = torch.randint(-3, 4, (k, c), device=DEV, generator=gen).float()
    sp = _lib.conv_plan(0, rows, 1, 1, c, k, 1, 1, (1, 1), (0, 0))
    lib, st = _lib.load(), _lib.current_stream_ptr(torch.device(DEV))
    flat, comp = slots(False), slots(True)
    out_f = torch.full((sp, rows * k), -1.0, device=DEV)
    out_c = torch.full((sp, rows * k), -1.0, device=DEV)
    geo = (rows, 1, 1, c, k, 1, 1, 1, 1, 0, 0, 0, 0, sp)
    assert lib.hf_conv2d_nhwc_slabs_unpack(P(out_f.data_ptr()), P(cols.data_ptr()), P(w.data_ptr()), *geo, out_f.shape[1],
                                           P(v.data_ptr()), *_lib.unpack_table(v, flat), _lib.HF_F32, st) == 0
    tab = _lib.unpack_table(vc, comp)
    assert lib.hf_conv2d_nhwc_slabs_unpack_compact(P(out_c.data_ptr()), P(cols.data_ptr()), P(w.data_ptr()), *geo,
                                                   out_c.shape[1], P(vc.data_ptr()), *tab[:-1], _lib.compact_periods(comp),
                                                   tab[-1], _lib.HF_F32, st) == 0
    assert torch.equal(out_f, out_c)
    assert torch.equal(out_c.sum(0).view(rows, k), cols @ w.t())  # (small integers: exact)
    _same_buffers(flat, comp)


# ---- live copy of rows, dead-entry check -------------------------------------------------------------------------------
def _segs(I=8, front=7):
    srcs = [pr.Src(front), pr.Src(27 * I, (I, 9), live=pr.CENTRE), pr.Src(11), pr.Src(27 * I, (I, 9), live=pr.CORNER),
            pr.Src(5)]
    segs, n = cr.segments(srcs)
    cols = [_i64([sg[c] for sg in segs]) for c in range(4)]
    return srcs, segs, n, cols


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=[np.dtype(d).name for d in pr.DTYPES])
def test_live_copy_of_rows_moves_every_row_in_one_launch(dtype):
    srcs, segs, n, cols = _segs()
    idx = cr.compact_index(srcs)
    rows, fs, cs = 3, n + 3, idx.size + 5
    full = np.random.RandomState(2).standard_normal((rows, fs)).astype(dtype)
    comp = np.full((rows, cs), NAN, dtype)
    dfull, dcomp = dev(full), dev(comp)
    lib = _lib.load()
    assert lib.hf_live_copy_rows(P(dfull.data_ptr()), P(dcomp.data_ptr()), 0, rows, fs, cs, *cols, len(segs), _CODE[dtype],
                                 None) == 0
    want = comp.copy()
    want[:, :idx.size] = full[:, idx]
    assert pr.same(dcomp.cpu().numpy(), want)
    back = dev(np.zeros((rows, fs), dtype))
    assert lib.hf_live_copy_rows(P(back.data_ptr()), P(dcomp.data_ptr()), 1, rows, fs, cs, *cols, len(segs), _CODE[dtype],
                                 None) == 0
    wantb = np.zeros((rows, fs), dtype)
    wantb[:, idx] = full[:, idx]
    assert pr.same(back.cpu().numpy(), wantb)


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=[np.dtype(d).name for d in pr.DTYPES])
@pytest.mark.parametrize("front", [0, 7])
def test_dead_entry_check(front, dtype):
    """Clean: zero or -0.0 on every dead entry (the live entries are not looked at: NaN there is fine).  Dirty: a single 1.0 or NaN at the first / the last dead entry of a segment, at a dead tap between two
    live ones, in either of the two vectors."""
    srcs, segs, n, cols = _segs(front=front)
    idx = cr.compact_index(srcs)
    dead = np.ones(n, bool)
    dead[idx] = False
    lib = _lib.load()
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)

    def check(a, b):
        da, db = dev(a), (None if b is None else dev(b))
        rc = lib.hf_live_dead_check(P(da.data_ptr()), None if db is None else P(db.data_ptr()), P(flag.data_ptr()), *cols,
                                    len(segs), _CODE[dtype], None)
        assert rc == 0
        return int(flag.item())

    clean = np.random.RandomState(4).standard_normal(n).astype(dtype)
    clean[dead] = 0.0
    clean[np.nonzero(dead)[0][::2]] = -0.0
    assert check(clean, None) == 0 and check(clean, clean) == 0
    places = []
    for off, cnt, per, mask in segs:
        if per:
            d = off + np.nonzero(dead[off:off + cnt])[0]
            places += [int(d[0]), int(d[-1])]
            if mask == pr.CORNER:  # taps 4, 5, 7, 8 live: tap 6 lies between live ones
                places.append(off + 9 * 3 + 6)
    assert len(places) == 5 and all(dead[p] for p in places)
    for p in places:
        for bad in (1.0, NAN):
            dirty = clean.copy()
            dirty[p] = bad
            assert check(dirty, None) == 1, (p, bad)
            assert check(clean, dirty) == 1, (p, bad)
            assert check(dirty, clean) == 1, (p, bad)
    live_nan = clean.copy()
    live_nan[idx[::3]] = NAN  # (live entries are not the check's business)
    assert check(live_nan, None) == 0
