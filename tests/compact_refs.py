"""The COMPACT layout of the flat CG vector -- the flat vector with the entries of kernel taps that never meet data removed
 -- as a numpy index map built on ``pack_refs.live_index``, a mirror of the branch of ``k_pack`` a tensor
takes when the gather writes that layout (``hf_pack_compact``), and the case table the CPU test of these definitions
(``test_compact_refs_cpu.py``) and the GPU test of the kernels (``test_compact_kernels_gpu.py``) share.  Plain module, numpy
only, no GPU.

Layout (one definition, the order ``hf_live_copy`` gives): tensor after tensor; a tensor without dead taps as it is; a conv
weight ``[O, I, HW]`` with tap mask ``m`` as ``[O, I, popcount(m)]``, taps in increasing order; no padding."""

from collections import namedtuple

import numpy as np
from pack_refs import (BLOCK, CENTRE, CORNER, DTYPES, NAN, PACK_CHUNK, PACK_PATHS, SPLIT_CHUNK, TILE_BYTES, Src, live_index,
                       pack_path)

MASKS = {"centre": CENTRE, "corner": CORNER}  # nl = 1 (3x3 on a 1x1 map), nl = 4 (3x3 stride 2 on a 2x2 map)


def popcount(m):
    return bin(m).count("1")


def masked(s):
    """Whether tensor ``s`` (pack_refs.Src) loses entries in the compact layout."""
    return bool(s.perm and s.live and popcount(s.live) < s.perm[1])


def segments(srcs):
    """The ``hf_live_copy`` segment table of a vector made of ``srcs``: (full offset, count, period, mask) per tensor."""
    segs, off = [], 0
    for s in srcs:
        if s.numel:
            segs.append((off, s.numel, s.perm[1], s.live) if masked(s) else (off, s.numel, 0, 0))
        off += s.numel
    return segs, off


def compact_index(srcs):
    """Flat index of every compact entry, in compact order."""
    return live_index(segments(srcs)[0])


def periods(srcs):
    """The ``compact`` array of ``hf_pack_compact`` / ``hf_unpack_weights_compact``: live taps of a masked tensor, else 0."""
    return [popcount(s.live) if masked(s) else 0 for s in srcs]


def compact_offsets(srcs):
    off, out = 0, []
    for s in srcs:
        out.append(off)
        off += s.numel // s.perm[1] * popcount(s.live) if masked(s) else s.numel
    return out, off


def gather(v, srcs):
    return v[compact_index(srcs)]


def scatter(c, srcs):
    """Compact vector -> flat vector, dead entries zero."""
    out = np.zeros(segments(srcs)[1], c.dtype)
    out[compact_index(srcs)] = c
    return out


# ---- the branch of k_pack a tensor takes in a compact launch -------------------------------------------------------------
# masked tensors (hf_pack.hip: the `cnl` branches); every other tensor takes its pack_refs.pack_path at its COMPACT offset
COMPACT_PATHS = ("split_quad_staged", "split_quad_straight", "split_quad_direct", "split_generic", "live_compact_vec",
                 "live_compact_walk")
# a compact launch gives every masked tensor its compact period (the engine's rule), so the two flat live-mask paths -- a
# zero stream over the dead taps, and its fallback walk -- are not reachable in it; everything else is, by the other tensors
REACHABLE = tuple(p for p in PACK_PATHS if p not in ("live_zero_stream", "live_walk"))


def masked_path(dtype, numel, perm, nsplit, stride, live, src_align, dst_off_c, mode=0):
    size = np.dtype(dtype).itemsize
    W, TILE = 16 // size, TILE_BYTES // size
    I, HW = perm
    slab, nl = I * HW, popcount(live)
    up = lambda least: -(-least // slab) * slab  # noqa: E731
    chunk = SPLIT_CHUNK if nsplit > 1 else PACK_CHUNK
    if nsplit > 1 and size == 4 and I % 4 == 0 and slab <= TILE:
        chunk = up(512 if nsplit >= 24 else 2048)
    elif nsplit == 1 and slab <= 2 * PACK_CHUNK:
        chunk = up(PACK_CHUNK)

    def block(j0):
        j1 = min(j0 + chunk, numel)
        if nsplit > 1:
            if not (size == 4 and src_align == 0 and stride % 4 == 0 and j0 % 4 == 0 and numel % 4 == 0 and I % 4 == 0):
                return "split_generic"
            al = (dst_off_c + j0 // slab * I * nl) * size % 16 == 0
            if chunk % slab == 0 and chunk <= TILE and al and nl != 1:
                return "split_quad_staged"
            return "split_quad_straight" if nl == 1 and dst_off_c * size % 16 == 0 else "split_quad_direct"
        whole = j0 % slab == 0 and (j1 - j0) % slab == 0
        if nl == 1 and I % W == 0 and whole and (dst_off_c + j0 // HW) * size % 16 == 0 and src_align == 0:
            return "live_compact_vec"
        return "live_compact_walk"

    names = {block(j0) for j0 in range(0, numel, chunk)}
    assert len(names) == 1, names
    return names.pop(), -(-numel // chunk)


def case_paths(case, dtype, mode):
    """Per non-empty tensor of the case: (branch name, masked?, workgroups)."""
    size = np.dtype(dtype).itemsize
    offs, _ = compact_offsets(case.srcs)
    out = []
    for s, off in zip(case.srcs, offs):
        if not s.numel:
            continue
        args = (dtype, s.numel, s.perm, s.nsplit, s.stride or s.numel, s.live, s.src_off * size % 16, off, mode)
        if masked(s):
            out.append(masked_path(*args) + (True,))
        else:
            out.append((pack_path(*args), None, False))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------
CompactCase = namedtuple("CompactCase", "name srcs dtypes")


def _perm(I, HW, O, **kw):
    return Src(O * I * HW, (I, HW), **kw)


def _cases():
    """The smallest shapes that reach each branch: masks centre / corner / all nine live / HW = 1, I = 8 (16-byte paths) and
    5 (scalar paths), O = 3, every depth class of the slab loops (1 | one predicated batch | one 8-batch + 1 | one 16-batch
    + 1), with and without a dense tensor of odd length in front (compact offsets behind it are unaligned)."""
    c = []
    for I in (8, 5):
        for n in (1, 2, 9, 17):
            for front in (0, 7):
                srcs = [Src(front)] if front else []
                srcs += [_perm(I, 9, 3, nsplit=n, live=CENTRE), _perm(I, 9, 3, nsplit=n, live=CORNER),
                         _perm(I, 9, 3, nsplit=n), Src(3 * I, nsplit=n)]
                c.append(CompactCase(f"i{I}_n{n}_front{front}", srcs, DTYPES))
    # more than one workgroup per tensor: 120 slabs of 72 (single slabs: 57 per workgroup; split: 29)
    for n in (1, 2):
        for front in (0, 7):
            srcs = ([Src(front)] if front else []) + [_perm(8, 9, 120, nsplit=n, live=CENTRE),
                                                       _perm(8, 9, 120, nsplit=n, live=CORNER), Src(5)]
            c.append(CompactCase(f"blocks_n{n}_front{front}", srcs, DTYPES))
    # slabs above the staging tile (split, 16-byte loads, no staging) and the direct un-permuting path of an unmasked tensor
    c.append(CompactCase("big_slab", [_perm(1028, 9, 2, nsplit=3, live=CORNER), _perm(1028, 9, 2)], DTYPES))
    return c


CASES = _cases()


def make_sources(case, dtype, seed):
    """As ``pack_refs.make_sources`` -- whole buffers with NaN in front, between and behind the slabs and in the source
    entries of dead taps -- with small-integer data: every sum is exact in every order."""
    rng = np.random.RandomState(seed)
    bufs, sources = [], []
    for s in case.srcs:
        stride = s.stride or s.numel
        buf = np.full(s.src_off + (s.nsplit + 1) * stride, NAN, dtype)
        slabs = rng.randint(-4, 5, size=(s.nsplit, s.numel)).astype(dtype)
        if s.perm and s.live:
            dead = [t for t in range(s.perm[1]) if not (s.live >> t) & 1]
            slabs.reshape(s.nsplit, -1, s.perm[1], s.perm[0])[:, :, dead, :] = NAN
        for k in range(s.nsplit):
            buf[s.src_off + k * stride:s.src_off + k * stride + s.numel] = slabs[k]
        bufs.append(buf)
        sources.append((slabs, s.perm, s.live))
    return bufs, sources


__all__ = ["BLOCK", "CASES", "COMPACT_PATHS", "REACHABLE", "MASKS"]
