"""Bitwise references of the gather / scatter kernels between per-layer buffers and the flat CG vector (``hf_pack.hip``,
``hf_unpack.h``: ``k_pack``, ``k_unpack_tangent``, ``k_live_copy``), a mirror of the rules by which ``k_pack`` chooses
its code path, and the case tables the CPU tests of the references (``test_pack_refs_cpu.py``) and the GPU tests of the
kernels (``test_pack_kernels_gpu.py``) share.  Plain module, numpy only, no GPU.

Every result of these kernels is determined to the bit: the library is built with ``-ffp-contract=off``, mode 0 is ONE
rounded multiply ``scale * s``, mode 1 is ``d + g*g`` with ``g = scale * s`` (three roundings), a split source is summed
in split order ``((s0 + s1) + s2) + ...`` in the tensor's own type before the scale, and unpack / live-copy only move
values.  The references below compute in the tensor's dtype with one numpy operation per rounding."""

from collections import namedtuple

import numpy as np

NAN = float("nan")
SCALES = (1.0, -0.5, 0.3)  # (0.3 is no power of two: the multiply really rounds)
DTYPES = (np.float32, np.float64)


def same(a, b):
    """Exact equality of two arrays; NaN sentinels are compared by position."""
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- k_pack ------------------------------------------------------------------------------------------------------------
def _dest_order(numel, perm, live):
    """Per DESTINATION entry of one tensor: its source index, and whether its kernel tap is live."""
    if perm is None:
        return np.arange(numel), np.ones(numel, bool)
    I, HW = perm
    src = np.arange(numel).reshape(-1, HW, I).transpose(0, 2, 1)  # stored (o, hw, i) -> vector order (o, i, hw)
    taps = np.array([(live >> t) & 1 if live else 1 for t in range(HW)], bool)
    return src.reshape(-1), np.broadcast_to(taps, src.shape).reshape(-1)


def pack_ref(dst_before, sources, scale, mode):
    """The flat vector after ``hf_pack_ex``.  ``sources``: per tensor ``(slabs[nsplit, numel] in storage order,
    (I, HW) or None, live mask)``.  Entries of dead taps are exactly 0 (mode 0) resp. keep ``d`` (mode 1: ``d + 0*0``);
    their source entries are never looked at."""
    out = dst_before.copy()
    sc = out.dtype.type(scale)
    off = 0
    for slabs, perm, live in sources:
        nsplit, numel = slabs.shape
        assert slabs.dtype == out.dtype
        idx, alive = _dest_order(numel, perm, live)
        idx = idx[alive]
        s = slabs[0, idx]
        for k in range(1, nsplit):
            s = s + slabs[k, idx]  # split order, one rounding per slab
        g = sc * s
        seg = out[off:off + numel]
        if mode == 0:
            seg[:] = 0
            seg[alive] = g
        else:
            sq = g * g
            seg[alive] = seg[alive] + sq
        off += numel
    assert off == out.size
    return out


# Constants of the source: BLOCK (hf_unpack.h:13), PACK_CHUNK = BLOCK * 16 (hf_unpack.h:15), the split chunk BLOCK * 4
# (hf_pack.hip:434), TILE_BYTES (hf_pack.hip:40).
BLOCK, PACK_CHUNK, SPLIT_CHUNK, TILE_BYTES = 256, 4096, 1024, 32768
PACK_PATHS = ("split_quad_staged", "split_quad_direct", "split_quad_plain_vec", "split_quad_plain_scalar", "split_generic",
              "live_zero_stream", "live_walk", "perm_tiled", "perm_direct", "plain_vec", "plain_scalar")


def pack_path(dtype, numel, perm, nsplit, stride, live, src_align, dst_off, mode=0):
    """The branch of ``k_pack`` that one tensor takes: the host's chunk rule (hf_pack.hip:428-455) and the kernel's
    predicates.  ``src_align``: source address modulo 16 (bytes); ``dst_off``: the tensor's offset (elements) in a
    16-byte aligned vector.  Every block of the tensor must take the same branch (asserted)."""
    size = np.dtype(dtype).itemsize
    W, TILE = 16 // size, TILE_BYTES // size
    I, HW = perm or (0, 0)
    slab = I * HW
    lv = live & ((1 << HW) - 1) if I and HW <= 16 else 0
    chunk = SPLIT_CHUNK if nsplit > 1 else PACK_CHUNK
    if I:
        up = lambda least: -(-least // slab) * slab  # whole slabs
        if TILE // (slab + HW) >= 1 and nsplit == 1 and not lv:
            chunk = TILE // (slab + HW) * slab
        elif nsplit > 1 and size == 4 and I % 4 == 0 and slab <= TILE:
            chunk = up(512 if nsplit >= 24 else 2048)
        elif lv and nsplit == 1 and slab <= 2 * PACK_CHUNK:
            chunk = up(PACK_CHUNK)

    def block(j0):
        al = (dst_off + j0) * size % 16 == 0
        if nsplit > 1:
            if not (size == 4 and src_align == 0 and stride % 4 == 0 and j0 % 4 == 0 and numel % 4 == 0 and I % 4 == 0):
                return "split_generic"
            if I:
                return "split_quad_staged" if chunk % slab == 0 and chunk <= TILE and al else "split_quad_direct"
            return "split_quad_plain_vec" if mode == 0 and al else "split_quad_plain_scalar"
        if lv:
            whole = chunk % slab == 0 and (min(j0 + chunk, numel) - j0) % W == 0
            return "live_zero_stream" if mode == 0 and al and whole else "live_walk"
        if I:
            return "perm_tiled" if chunk % slab == 0 and chunk // slab * (slab + HW) <= TILE else "perm_direct"
        return "plain_vec" if src_align == 0 and dst_off * size % 16 == 0 else "plain_scalar"

    names = {block(j0) for j0 in range(0, numel, chunk)}
    assert len(names) == 1, names
    return names.pop()


# One source tensor of a pack case.  ``perm``: (I, HW) of a tensor stored (O, HW, I), None = plain; ``stride``: elements
# between split slabs (None = numel); ``src_off``: elements between a 16-byte aligned address and the first slab.
Src = namedtuple("Src", "numel perm nsplit stride live src_off", defaults=(None, 1, None, 0, 0))
# ``path``: the branch the case is there for, taken by its LAST tensor (the ones before it only move the destination
# offset): a name, ``(mode 0 name, mode 1 name)``, or a dict of those by dtype name; None where no single one is meant.
PackCase = namedtuple("PackCase", "name srcs dtypes path")
F32, BOTH = (np.float32,), DTYPES
CENTRE, CORNER = 1 << 4, 0b110110000  # a 3x3 kernel on a 1x1 map, and on a 2x2 map with stride 2 (engine._live_taps)


def _perm(I, HW, O, **kw):
    return Src(O * I * HW, (I, HW), **kw)


def _by_dtype(f32, f64="split_generic"):
    return {"float32": f32, "float64": f64}


def _split_cases():
    c = []
    for n in (2, 9, 16, 17, 24, 33):  # one predicated batch | one 8-batch | 8 + 7 | one 16-batch | 16 + 7 | two 16-batches
        c.append(PackCase(f"staged_n{n}", [_perm(16, 9, 24, nsplit=n)], F32, "split_quad_staged"))
    c.append(PackCase("staged_live_n24", [_perm(16, 9, 24, nsplit=24, live=CENTRE)], F32, "split_quad_staged"))
    c.append(PackCase("staged_swizzle", [_perm(64, 9, 16, nsplit=3)], F32, "split_quad_staged"))
    c.append(PackCase("direct_dst_misaligned", [Src(3), _perm(16, 9, 24, nsplit=2)], F32, "split_quad_direct"))
    c.append(PackCase("direct_slab_above_tile", [_perm(1028, 9, 2, nsplit=3)], F32, "split_quad_direct"))
    c.append(PackCase("plain_split_aligned", [Src(4100, nsplit=5)], F32,
                      ("split_quad_plain_vec", "split_quad_plain_scalar")))
    c.append(PackCase("plain_split_odd_dst", [Src(1), Src(4100, nsplit=5)], F32, "split_quad_plain_scalar"))
    for n in (8, 9, 10):  # only the predicated batch | exactly one full batch | a full batch + 1
        for name, src in (("perm6", _perm(6, 9, 40, nsplit=n)),
                          ("perm6_live", _perm(6, 9, 40, nsplit=n, live=CORNER)),
                          ("numel4099", Src(4099, nsplit=n)),
                          ("stride_plus1", _perm(16, 9, 24, nsplit=n, stride=3457)),
                          ("src_plus1", _perm(16, 9, 24, nsplit=n, src_off=1))):
            c.append(PackCase(f"generic_{name}_n{n}", [src], BOTH, "split_generic"))
    return c


def _single_cases():
    c = []
    for tag, m in (("centre", CENTRE), ("corner", CORNER)):
        c.append(PackCase(f"live_{tag}", [_perm(16, 9, 64, live=m)], BOTH, ("live_zero_stream", "live_walk")))
        c.append(PackCase(f"live_{tag}_odd_dst", [Src(1), _perm(16, 9, 64, live=m)], BOTH, "live_walk"))
        c.append(PackCase(f"live_{tag}_big_slab", [_perm(1028, 9, 2, live=m)], BOTH, "live_walk"))
    for O, I, HW in ((9, 6, 6), (5, 3, 1), (64, 2, 49), (70, 64, 9)):  # (the last: more slabs than one tile holds)
        c.append(PackCase(f"perm_{O}x{I}x{HW}", [_perm(I, HW, O)], BOTH, "perm_tiled"))
    # slab + HW = 6309: inside the fp32 tile of 8192 elements, not inside the fp64 tile of 4096
    c.append(PackCase("perm_3x700x9", [_perm(700, 9, 3)], BOTH, _by_dtype("perm_tiled", "perm_direct")))
    c.append(PackCase("perm_3x700x9_odd_dst", [Src(3), _perm(700, 9, 3)], BOTH, _by_dtype("perm_tiled", "perm_direct")))
    c.append(PackCase("perm_2x1028x9", [_perm(1028, 9, 2)], BOTH, "perm_direct"))
    c.append(PackCase("perm_2x1028x9_odd_dst", [Src(1), _perm(1028, 9, 2)], BOTH, "perm_direct"))
    c.append(PackCase("plain_aligned", [Src(4099)], BOTH, "plain_vec"))
    c.append(PackCase("plain_odd_dst", [Src(1), Src(4099)], BOTH, "plain_scalar"))
    c.append(PackCase("plain_src_plus1", [Src(4099, src_off=1)], BOTH, "plain_scalar"))
    return c


def _table_cases():
    """64 and 65 non-empty tensors (PACK_MAXT = 64 per launch) of mixed kinds with empty ones between them; the 65th --
    alone in the second launch -- is a split tensor."""
    kinds = (Src(7), _perm(3, 4, 2), _perm(4, 9, 3, live=CENTRE), Src(13, nsplit=3), _perm(4, 9, 1, nsplit=2), Src(0))
    srcs = []
    while sum(s.numel > 0 for s in srcs) < 64:
        srcs.append(kinds[len(srcs) % len(kinds)])
    return [PackCase("table_64", srcs + [Src(0)], BOTH, None),
            PackCase("table_65", srcs + [Src(0), _perm(16, 9, 24, nsplit=9)], BOTH, _by_dtype("split_quad_staged"))]


SPLIT_CASES, SINGLE_CASES, TABLE_CASES = _split_cases(), _single_cases(), _table_cases()
PACK_CASES = SPLIT_CASES + SINGLE_CASES + TABLE_CASES


def expected_path(case, dtype, mode):
    p = case.path
    if isinstance(p, dict):
        p = p[np.dtype(dtype).name]
    return p[mode] if isinstance(p, tuple) else p


def case_path(case, dtype, mode):
    """``pack_path`` of the case's last tensor, placed behind the tensors before it."""
    s = case.srcs[-1]
    size = np.dtype(dtype).itemsize
    return pack_path(dtype, s.numel, s.perm, s.nsplit, s.stride or s.numel, s.live, s.src_off * size % 16,
                     sum(q.numel for q in case.srcs[:-1]), mode)


def make_sources(case, dtype, seed):
    """Random normal data of a case: per tensor the whole buffer as it lies in memory (``src_off`` NaN entries, the
    slabs ``stride`` apart, NaN between them and in ONE MORE slab behind the last, so that a read past the split count
    meets NaN), and the ``pack_ref`` description of it.  The source entries of dead taps are NaN in every slab."""
    rng = np.random.RandomState(seed)
    bufs, sources = [], []
    for s in case.srcs:
        stride = s.stride or s.numel
        buf = np.full(s.src_off + (s.nsplit + 1) * stride, NAN, dtype)
        slabs = rng.standard_normal((s.nsplit, s.numel)).astype(dtype)
        if s.perm and s.live:
            dead = [t for t in range(s.perm[1]) if not (s.live >> t) & 1]
            slabs.reshape(s.nsplit, -1, s.perm[1], s.perm[0])[:, :, dead, :] = NAN
        for k in range(s.nsplit):
            buf[s.src_off + k * stride:s.src_off + k * stride + s.numel] = slabs[k]
        bufs.append(buf)
        sources.append((slabs, s.perm, s.live))
    return bufs, sources


# ---- k_unpack_tangent --------------------------------------------------------------------------------------------------
# One destination of an unpack launch: the [O, I, H, W] slice of the vector at ``off`` goes into half 0 / 1 of a
# [O, 2I, H, W] buffer stored NCHW or NHWC, or (half 2) into a dense (I, H, W, O) buffer.  ``live`` counts for NHWC only.
Slot = namedtuple("Slot", "off shape nhwc live", defaults=(False, 0))
UNPACK_VEC_SHAPES = ((24, 16, 3, 3), (8, 4, 1, 1), (5, 8, 2, 3))
UNPACK_SCALAR_SHAPE = (8, 3, 3, 3)
UNPACK_RAGGED_SHAPE = (70, 5, 3, 3)  # half 2: neither O nor I*H*W a multiple of the 64 x 64 transpose tile


def unpack_ref(v, slots, half):
    """The destination buffers after ``hf_unpack_weights``, as logical [O, 2I, H, W] arrays (half 2: (I, H, W, O)) that
    start NaN-filled.  ``half``: one value or one per slot.  The slices of dead taps keep the NaN."""
    halves = [half] * len(slots) if np.isscalar(half) else list(half)
    out = []
    for s, h in zip(slots, halves):
        O, I, H, Wd = s.shape
        w = v[s.off:s.off + O * I * H * Wd].reshape(s.shape)
        if h == 2:
            out.append(np.ascontiguousarray(w.transpose(1, 2, 3, 0)))
            continue
        buf = np.full((O, 2 * I, H, Wd), NAN, v.dtype)
        taps = np.array([(s.live >> t) & 1 if s.nhwc and s.live else 1 for t in range(H * Wd)], bool).reshape(H, Wd)
        buf[:, h * I:(h + 1) * I][:, :, taps] = w[:, :, taps]
        out.append(buf)
    return out


def unpack_vector_loop(dtype, off, shape, nhwc):
    """Whether ``unpack_block`` takes its 16-byte loop for a slice at ``off`` of an aligned vector (hf_unpack.h:63, :77;
    the destination buffers are aligned)."""
    size = np.dtype(dtype).itemsize
    W = 16 // size
    aligned = off * size % 16 == 0
    O, I, H, Wd = shape
    return aligned and (I % W == 0 if nhwc else (I * H * Wd) % W == 0)


def unpack_slots(shift, nhwc, live=0):
    """The shapes of the vector loops, 4-element aligned slices moved by ``shift``, and the scalar shape behind them;
    ``live`` on the 3x3 shapes.  Returns the slots and the length of the vector."""
    slots, off = [], 8 + shift
    for sh in UNPACK_VEC_SHAPES + (UNPACK_SCALAR_SHAPE,):
        slots.append(Slot(off, sh, nhwc, live if sh[2] * sh[3] == 9 else 0))
        off += -(-int(np.prod(sh)) // 4) * 4 + 4
    return slots, off + 3


# ---- k_live_copy -------------------------------------------------------------------------------------------------------
# A segment: (offset in the full vector, elements in the full vector, period (0 = dense), mask of the live positions).
def live_index(segs):
    idx = []
    for off, cnt, per, mask in segs:
        keep = np.ones(cnt, bool) if per == 0 else np.tile([bool((mask >> t) & 1) for t in range(per)], cnt // per)
        idx.append(off + np.nonzero(keep)[0])
    return np.concatenate(idx)


def live_copy_ref(full, segs):
    """The compact vector of ``hf_live_copy`` (gather): segment after segment, the live entries in order."""
    return full[live_index(segs)]


def _chain(items, off=3):
    segs = []
    for cnt, per, mask in items:
        segs.append((off, cnt, per, mask))
        off += cnt + (5 if per == 0 else 0)  # (gaps: entries that belong to no segment)
    return segs, off + 2


def _live_layouts():
    lay = {}
    lay["small"] = ([(0, 37, 0, 0), (37, 270, 9, CENTRE), (307, 11, 0, 0), (318, 108, 9, CORNER), (426, 5, 0, 0)], 431)
    lay["big"] = _chain([(70001, 0, 0), (300 * 40 * 9, 9, CENTRE), (4099, 0, 0), (128 * 64 * 9, 9, 0b110110110),
                         (96 * 48 * 9, 9, CORNER), (8192, 0, 0)])
    # dense, full and compact offsets both multiples of 4, two whole blocks of 2048 and a block of 203 (a tail of 3
    # resp. 1 behind the 16-byte copies); then the same length at an odd compact offset and an odd full offset
    lay["dense_aligned"] = ([(8, 4299, 0, 0), (4308, 4299, 0, 0), (8609, 4299, 0, 0)], 12912)
    lay["limit_24"] = _chain([((5, 0, 0), (36, 9, CENTRE), (90, 9, CORNER), (32, 16, 0x8001), (8, 4, 0b0110),
                               (2051, 0, 0))[k % 6] for k in range(24)], off=4)
    return lay


LIVE_LAYOUTS = _live_layouts()
