"""CPU: the bitwise references of the gather / scatter kernels (``pack_refs.py``) are the constructions the older tests
compare with (``torch.cat`` of the un-permuted tensors, ``copy_`` into the halves, ``permute(1, 2, 3, 0)``, boolean-mask
indexing); the split sum is pinned to split order; and the case tables reach every branch of ``k_pack`` and the 16-byte
loops of ``unpack_block`` -- checked with a mirror of the kernels' predicates, not asserted."""

import numpy as np
import pytest
import torch

import pack_refs as pr

_IDS = [c.name for c in pr.PACK_CASES]
_TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def _logical(slab, perm):
    """One stored slab as the flat tensor in vector order (O, I, HW)."""
    if perm is None:
        return torch.from_numpy(slab.copy())
    I, HW = perm
    return torch.from_numpy(slab.copy()).view(-1, HW, I).permute(0, 2, 1).reshape(-1)


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_pack_ref_of_single_slabs_equals_cat_times_scale(dtype):
    cases = [c for c in pr.SINGLE_CASES if not any(s.live for s in c.srcs)]
    assert len(cases) >= 8
    for c in cases:
        _, sources = pr.make_sources(c, dtype, 1)
        cat = torch.cat([_logical(slabs[0], perm) for slabs, perm, _ in sources])
        for scale in pr.SCALES:
            got = pr.pack_ref(np.full(cat.numel(), pr.NAN, dtype), sources, scale, 0)
            want = torch.tensor(scale, dtype=_TORCH[dtype]) * cat
            assert got.dtype == dtype and torch.equal(torch.from_numpy(got), want), (c.name, scale)
            d = np.random.RandomState(2).standard_normal(cat.numel()).astype(dtype)
            g = want.numpy()
            assert pr.same(pr.pack_ref(d, sources, scale, 1), d + g * g), (c.name, scale)


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_pack_ref_sums_split_sources_left_to_right(dtype):
    # 1 + 2^-p is a tie for p = the mantissa width: left to right every small term is rounded away one by one, while
    # the pairwise np.sum first adds small terms to each other
    tiny = dtype(np.finfo(dtype).eps / 2)
    slabs = np.full((33, 40), tiny, dtype)
    slabs[0] = 1
    ref = pr.pack_ref(np.zeros(40, dtype), [(slabs, None, 0)], 1.0, 0)
    pairwise = np.sum(np.ascontiguousarray(slabs.T), axis=1)  # (numpy sums pairwise along a contiguous axis)
    assert pairwise.dtype == dtype and np.all(ref == 1) and np.all(pairwise > 1)
    rng = np.random.RandomState(3)
    for case in (c for c in pr.SPLIT_CASES if dtype in c.dtypes):
        _, sources = pr.make_sources(case, dtype, 4)
        d = rng.standard_normal(sum(s[0].shape[1] for s in sources)).astype(dtype)
        for mode in (0, 1):
            got = pr.pack_ref(d, sources, 0.3, mode)
            assert not np.isnan(got).any(), case.name  # (the NaN of the dead taps was not read)
            want = []
            for slabs, perm, live in sources:
                s = slabs[0]
                for k in range(1, len(slabs)):
                    s = s + slabs[k]
                g = _logical(dtype(0.3) * s, perm).numpy()
                want.append(np.where(np.isnan(g), dtype(0), g))  # dead taps: 0, resp. d unchanged
            want = np.concatenate(want)
            assert pr.same(got, want if mode == 0 else d + want * want), (case.name, mode)


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_pack_ref_of_live_masks_zeroes_the_dead_taps_without_reading_them(dtype):
    cases = [c for c in pr.SINGLE_CASES + pr.TABLE_CASES if any(s.live for s in c.srcs)]
    assert cases
    for c in cases:
        _, sources = pr.make_sources(c, dtype, 5)
        n = sum(s[0].shape[1] for s in sources)
        d = np.random.RandomState(6).standard_normal(n).astype(dtype)
        zeroed = [(np.nan_to_num(slabs, nan=0.0), perm, 0) for slabs, perm, _ in sources]  # ... as the older test does
        for mode in (0, 1):
            got = pr.pack_ref(d, sources, -0.5, mode)
            assert not np.isnan(got).any()
            assert pr.same(got, pr.pack_ref(d, zeroed, -0.5, mode)), (c.name, mode)


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_unpack_ref_equals_copy_and_permute(dtype):
    for nhwc in (False, True):
        for shift in (0, 1):
            slots, n = pr.unpack_slots(shift, nhwc, pr.CORNER)
            v = np.random.RandomState(7).standard_normal(n).astype(dtype)
            tv = torch.from_numpy(v)
            for half in (0, 1):
                for s, got in zip(slots, pr.unpack_ref(v, slots, half)):
                    O, I, H, W = s.shape
                    want = torch.full((O, 2 * I, H, W), pr.NAN, dtype=_TORCH[dtype])
                    want[:, half * I:(half + 1) * I].copy_(tv[s.off:s.off + O * I * H * W].view(s.shape))
                    if nhwc and s.live:
                        dead = torch.tensor([not (s.live >> t) & 1 for t in range(H * W)]).view(H, W)
                        want[:, :, dead] = pr.NAN
                    assert pr.same(got, want.numpy()), (s, half)
            for s, got in zip(slots, pr.unpack_ref(v, slots, 2)):
                want = tv[s.off:s.off + int(np.prod(s.shape))].view(s.shape).permute(1, 2, 3, 0).contiguous()
                assert pr.same(got, want.numpy())


@pytest.mark.parametrize("name", list(pr.LIVE_LAYOUTS))
def test_live_copy_ref_equals_boolean_mask_indexing(name):
    segs, n = pr.LIVE_LAYOUTS[name]
    keep = np.zeros(n, bool)
    for off, cnt, per, mask in segs:
        assert not keep[off:off + cnt].any() and off + cnt <= n  # (segments in order, no overlap)
        keep[off:off + cnt] = True if per == 0 else np.tile([bool((mask >> t) & 1) for t in range(per)], cnt // per)
    full = np.random.RandomState(8).standard_normal(n)
    assert pr.same(pr.live_copy_ref(full, segs), full[keep])
    assert len(pr.LIVE_LAYOUTS["limit_24"][0]) == 24
    assert not keep.all()  # some entries belong to no segment or to a dead position


def test_the_case_table_names_the_path_each_case_takes():
    for c in pr.PACK_CASES:
        if c.path is None:
            continue
        for dtype in c.dtypes:
            for mode in (0, 1):
                assert pr.case_path(c, dtype, mode) == pr.expected_path(c, dtype, mode), (c.name, dtype, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_the_case_table_reaches_every_path_of_k_pack(mode):
    reached = {dt: set() for dt in pr.DTYPES}
    for c in pr.PACK_CASES:
        for dt in c.dtypes:
            off = 0
            for s in c.srcs:
                if s.numel:
                    p = pr.pack_path(dt, s.numel, s.perm, s.nsplit, s.stride or s.numel, s.live,
                                     s.src_off * np.dtype(dt).itemsize % 16, off, mode)
                    assert p == "split_generic" or not (dt == np.float64 and s.nsplit > 1)
                    reached[dt].add(p)
                off += s.numel
    every = set(pr.PACK_PATHS)
    if mode == 1:  # the zero stream and the vector store of plain split sources exist for mode 0 only
        every -= {"live_zero_stream", "split_quad_plain_vec"}
    assert reached[np.float32] == every
    assert reached[np.float64] == {p for p in every if not p.startswith("split_quad")}


def test_pack_path_at_the_thresholds_of_the_chunk_rule():
    f32, f64 = np.float32, np.float64
    path = lambda dt, I, HW, O, nsplit=1, live=0, off=0, mode=0: pr.pack_path(dt, O * I * HW, (I, HW), nsplit,
                                                                              O * I * HW, live, 0, off, mode)
    # slab + HW against the tile of 8192 fp32 / 4096 fp64 elements
    assert path(f32, 909, 9, 2) == "perm_tiled" and path(f32, 910, 9, 2) == "perm_direct"   # 8190, 8199
    assert path(f64, 454, 9, 2) == "perm_tiled" and path(f64, 455, 9, 2) == "perm_direct"   # 4095, 4104
    # staged stores: I*HW <= the tile
    assert path(f32, 908, 9, 2, nsplit=2) == "split_quad_staged"       # 8172
    assert path(f32, 912, 9, 2, nsplit=2) == "split_quad_direct"       # 8208
    # zero stream: slab <= 2 * PACK_CHUNK
    assert path(f32, 908, 9, 4, live=pr.CENTRE) == "live_zero_stream"  # 8172
    assert path(f32, 912, 9, 4, live=pr.CENTRE) == "live_walk"         # 8208
    # a mask wider than the period, or a period above 16 taps, is no mask
    assert path(f32, 16, 25, 4, live=pr.CENTRE) == "perm_tiled"
    assert path(f32, 16, 9, 4, live=1 << 9) == "perm_tiled"


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_the_unpack_slots_reach_both_16_byte_loops_and_both_scalar_loops(dtype):
    for nhwc in (False, True):
        aligned, _ = pr.unpack_slots(0, nhwc, pr.CENTRE)
        shifted, _ = pr.unpack_slots(1, nhwc, pr.CENTRE)
        vec = [s for s in aligned if pr.unpack_vector_loop(dtype, s.off, s.shape, s.nhwc)]
        assert [s.shape for s in vec] == list(pr.UNPACK_VEC_SHAPES)
        assert not any(pr.unpack_vector_loop(dtype, s.off, s.shape, s.nhwc) for s in shifted)
        if nhwc:  # the live skip in both loops
            assert any(s.live for s in vec) and any(s.live for s in aligned if s not in vec)
