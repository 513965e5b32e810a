"""CPU: the references of ``flatten_refs`` against torch itself -- ``torch.flatten`` of a ``channels_last`` tensor (what
``nn.Flatten`` computes on a prepared model's last map) and its autograd adjoint."""

import numpy as np
import pytest
import torch

import flatten_refs as R


@pytest.mark.parametrize("n,hw,c", R.SHAPES)
@pytest.mark.parametrize("wide,half", [(0, 0), (1, 0), (1, 1)])
def test_flatten_is_torch_flatten_of_a_channels_last_tensor(n, hw, c, wide, half):
    in_ld = 2 * c if wide else c
    buf, off = R.operand(n, hw, c, in_ld, half)
    h, w = (hw // 7, 7) if hw % 7 == 0 else (hw, 1)
    # the half as the model sees it: a logically-NCHW tensor whose memory is NHWC
    nhwc = buf.view(n, h, w, in_ld)[..., off:off + c]
    x = nhwc.permute(0, 3, 1, 2)
    assert x.shape == (n, c, h, w) and x.stride(1) == 1
    want = torch.flatten(x, 1)
    for out_ld in (c * hw, c * hw + 4):
        got = R.flatten(buf, off, in_ld, n, hw, c, out_ld, -1.0).view(n, out_ld)
        assert torch.equal(got[:, :c * hw], want)
        assert bool((got[:, c * hw:] == -1.0).all())
    assert want.unique().numel() == want.numel()  # (every element distinct: a permutation error cannot hide)


@pytest.mark.parametrize("n,hw,c", R.SHAPES)
def test_unflatten_of_one_slab_is_the_adjoint_of_flatten(n, hw, c):
    h, w = (hw // 7, 7) if hw % 7 == 0 else (hw, 1)
    s = R.slabs(n, hw, c, 1, seed=3)
    x = torch.zeros(n, c, h, w).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    torch.flatten(x, 1).backward(s[0].view(n, c * hw))
    want = x.grad.permute(0, 2, 3, 1).contiguous().view(-1)  # the cotangent of the map, NHWC
    assert torch.equal(R.unflatten(s, n, hw, c), want)


@pytest.mark.parametrize("splits", R.SPLITS)
def test_slab_sum_is_the_ordered_fp32_sum(splits):
    n, hw, c = 3, 30, 8
    s = R.slabs(n, hw, c, splits, seed=5)
    acc = s[0].clone()
    for k in range(1, splits):
        acc = acc + s[k]  # ((s0 + s1) + s2) ... in fp32
    assert torch.equal(torch.from_numpy(R.slab_sum(s)), acc)
    if splits == 5:  # the order matters on these operands: the reversed sum differs somewhere
        rev = s[4].clone()
        for k in (3, 2, 1, 0):
            rev = rev + s[k]
        assert not torch.equal(rev, acc)
    got = R.unflatten(s, n, hw, c).view(n, hw, c)
    assert torch.equal(got, acc.view(n, c, hw).permute(0, 2, 1))


def test_shapes_cover_the_kernel_paths():
    tile = 32  # FT of csrc/hf_head.hip
    assert any(hw == 1 for _, hw, _ in R.SHAPES) and any(hw % 2 and hw > 1 for _, hw, _ in R.SHAPES)
    assert any(hw > tile and hw % tile for _, hw, _ in R.SHAPES) and any(c > tile for _, _, c in R.SHAPES)
    assert any(n == 256 for n, _, _ in R.SHAPES) and all(c % 4 == 0 for _, _, c in R.SHAPES)
    assert np.float32(1.0) + np.float32(2.0 ** -24) == np.float32(1.0)  # (numpy float32 additions round to fp32)
