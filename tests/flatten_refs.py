"""TEST INFRASTRUCTURE ONLY -- references of the two boundary kernels between a conv stack and a classifier tail
(``hf_flatten_nhwc_rows`` / ``hf_unflatten_slabs_nhwc`` of ``csrc/hf_head.hip``), written from the index maps in
``include/hf_pcg.h`` with explicit loops, and the shapes the kernel tests run.  Plain module, no GPU.

    flatten:    out[r*out_ld + ch*hw + p] = in[(r*hw + p)*in_ld + ch]
    unflatten:  out[(r*hw + p)*c + ch]    = ((s0 + s1) + s2) ...   of   slabs[s*slab_stride + r*c*hw + ch*hw + p]

``test_flatten_refs_cpu.py`` anchors both to ``torch.flatten`` of a ``channels_last`` tensor and its autograd adjoint."""

import numpy as np
import torch

# (n, hw, c): one pixel; one tile; hw not a multiple of 4, odd, square; two channel tiles; the dense kernels' row limit
# at one pixel; more than one pixel tile with a ragged end
SHAPES = [(1, 1, 4), (2, 4, 8), (3, 30, 8), (5, 9, 12), (2, 49, 64), (256, 1, 4), (4, 130, 4)]
SPLITS = (1, 2, 5)


def operand(n, hw, c, in_ld, half):
    """A flat NHWC operand of ``n*hw`` pixels at pitch ``in_ld`` whose every element is distinct (its own index + 1:
    a misplaced element cannot pass), and the offset of the half the kernel reads."""
    assert in_ld >= c * (half + 1)
    buf = torch.arange(1, n * hw * in_ld + 1, dtype=torch.float32)
    return buf, half * c


def flatten(buf, off, in_ld, n, hw, c, out_ld, fill):
    """The index map, one element at a time; the padding of a row keeps ``fill``."""
    src, out = buf.numpy(), np.full(n * out_ld, fill, dtype=np.float32)
    for r in range(n):
        for p in range(hw):
            for ch in range(c):
                out[r * out_ld + ch * hw + p] = src[off + (r * hw + p) * in_ld + ch]
    return torch.from_numpy(out)


def slabs(n, hw, c, splits, seed):
    """``splits`` standard-normal [n, c*hw] slabs: their fp32 sum depends on the order of the additions."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(splits, n * c * hw, generator=g, dtype=torch.float32)


def slab_sum(s):
    """slab 0, then slabs 1 .. n-1 in split order, one fp32 rounding each."""
    acc = s[0].numpy().copy()
    for k in range(1, s.shape[0]):
        acc = (acc + s[k].numpy()).astype(np.float32)
    return acc


def unflatten(s, n, hw, c):
    """The index map on the ordered slab sum -> a dense NHWC map [n*hw*c]."""
    acc, out = slab_sum(s), np.empty(n * hw * c, dtype=np.float32)
    for r in range(n):
        for p in range(hw):
            for ch in range(c):
                out[(r * hw + p) * c + ch] = acc[r * c * hw + ch * hw + p]
    return torch.from_numpy(out)
