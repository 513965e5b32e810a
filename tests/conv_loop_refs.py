"""Cases for the K loops of the 64 x 64 convolution kernels (``hf_conv.hip``) at share lengths that ``conv_refs.py``'s
table (1 .. 5 steps per workgroup) does not reach.

The weight-gradient body (``conv_tn_body``, Small configuration) runs the software-pipelined loop ``pipelined_share``: a
register ring of ``RING`` = 2 steps, refilled as soon as a slot is stashed, with the ring's slot, the LDS buffer and the
fragment registers of a step compile-time in a loop unrolled ``RING`` times.  A share leaves that loop after an odd or
an even number of steps, in its first round or after several: 1, 3, 5, 6 and 7 steps here.  The forward / data-gradient
body keeps its three-deep ring; its cases here walk it at 6, 7, 8 and 12 steps (every residue modulo 3, two to four
rounds), with a last share shorter than the others, ragged channel steps, dead taps and residue classes -- the cases a
pipelined form of that body has to pass as well (one, six deep, was measured and not kept: DESIGN.md section 6.1; these
cases were written against it).

Every case is found through the planner (slab mode, the planner's own split count -- no case passes one): the share
length a case is named for is what ``hf_conv2d_nhwc_plan_info`` answers, asserted on the CPU by
``test_conv_loop_refs_cpu.py``; ``test_conv_loop_gpu.py`` runs the kernels.  Operands, references and the exactness
condition are ``conv_refs``' (integers in [-3, 3]: every partial sum is an exact integer).

Sizes: batch 2 .. 4, maps up to 7 x 7, channels up to 160 -- the planner splits until 256 workgroups exist, so a share of
6 steps on so few tiles needs a long reduction: a 7 x 7 window (49 taps) over 100 .. 132 channels (4 or 5 steps per tap,
the last one ragged: 100 = 3 * 32 + 4, 132 = 4 * 32 + 4).  Two exceptions, each the smallest the planner admits: the
residue-class enumeration of a strided data gradient starts at 2048 pixels (8 x 16 x 16), and the scatter-carrying
launch takes an im2col'd operand (196 rows of a 1 x 1 map, as many as 4 x 7 x 7)."""

from conv_refs import Case, E, P

RING = 2  # hf_conv.hip: depth of the register ring of pipelined_share

_K7 = (7, 7, 1, 3)  # 7 x 7 window, stride 1, pad 3


def _named(name, shares, form, problems, expect, sums=None):
    """``shares``: per problem, the steps of one workgroup's share the case is named for (residue classes: of the
    longest class)."""
    assert tuple(e.per for e in expect) == tuple(shares), name
    return Case(name, form, tuple(problems), tuple(expect), None, sums)


# problems that several cases share (a data gradient and a weight gradient of one layer read the same dY)
F_6, D_6, W_OF_6 = P(0, 2, 5, 7, 132, 132, *_K7), P(1, 2, 5, 7, 132, 132, *_K7), P(2, 2, 5, 7, 132, 132, *_K7)
F_7, D_7, W_OF_7 = P(0, 4, 5, 7, 100, 132, *_K7), P(1, 4, 5, 7, 132, 100, *_K7), P(2, 4, 5, 7, 132, 100, *_K7)
F_8, D_8 = P(0, 4, 7, 7, 132, 68, *_K7), P(1, 4, 7, 7, 68, 132, *_K7)
F_12, D_12, W_OF_12 = P(0, 4, 7, 7, 132, 132, *_K7), P(1, 4, 7, 7, 132, 132, *_K7), P(2, 4, 7, 7, 132, 132, *_K7)
W_5, W_6, W_7 = P(2, 4, 5, 7, 68, 132, *_K7), P(2, 4, 7, 6, 68, 132, *_K7), P(2, 4, 7, 7, 68, 132, *_K7)
F_ONE, F_3 = P(0, 2, 4, 4, 32, 8, 1, 1), P(0, 4, 6, 6, 16, 24, 3, 3, 1, 1)
D_CLS = P(1, 8, 16, 16, 4, 132, 5, 5, 2, 2)
F_BN = P(0, 4, 7, 7, 36, 100, 3, 3, 1, 1)
F_BN49 = P(0, 3, 7, 7, 28, 68, *_K7)
F_UNPACK = P(0, 196, 1, 1, 132, 68, 1, 1)

# 70 / 140 / 196 rows: none a multiple of 64;  245 steps in shares of 6 or 12: the last share has 5
E_F_6, E_F_7, E_F_8, E_F_12 = E(0, 41, 6, 49), E(0, 28, 7, 49), E(0, 31, 8, 49), E(0, 21, 12, 49)
E_W_5, E_W_6, E_W_7 = E(0, 1, 5, 49), E(0, 1, 6, 49), E(0, 1, 7, 49)
E_W_OF_6, E_W_OF_7, E_W_OF_12 = E(0, 1, 3, 49), E(0, 1, 5, 49), E(0, 1, 7, 49)
E_F_ONE, E_F_3 = E(0, 1, 1, 1), E(0, 3, 3, 9)
E_D_CLS = E(0, 8, 6, 25, (9, 6, 6, 4))   # 45 / 30 / 30 / 20 steps per class in 8 shares: 6 / 4 / 4 / 3
E_F_BN, E_F_BN49 = E(0, 9, 2, 9), E(0, 17, 3, 49)
E_F_UNPACK = E(0, 2, 3, 1)


def _cases():
    one = lambda name, steps, p, e: _named(name, (steps,), "slabs", (p,), (e,))  # noqa: E731
    return [
        # -- shares beyond conv_refs' 1 .. 5 steps: forward, data gradient (6 / 7 / 8 / 12), weight gradient (5 / 6 / 7)
        one("loop_nt_forward_6_steps_last_share_5", 6, F_6, E_F_6),
        one("loop_nt_forward_7_steps", 7, F_7, E_F_7),
        one("loop_nt_forward_8_steps", 8, F_8, E_F_8),
        one("loop_nt_forward_12_steps", 12, F_12, E_F_12),
        one("loop_nt_dgrad_6_steps_last_share_5", 6, D_6, E_F_6),
        one("loop_nt_dgrad_7_steps", 7, D_7, E_F_7),
        one("loop_nt_dgrad_8_steps", 8, D_8, E_F_8),
        one("loop_nt_dgrad_12_steps", 12, D_12, E_F_12),
        one("loop_tn_5_steps_ragged_rows", 5, W_5, E_W_5),      # 140 rows: the last step has 12
        one("loop_tn_6_steps_ragged_rows", 6, W_6, E_W_6),      # 168 rows: the last step has 8
        one("loop_tn_7_steps_ragged_rows", 7, W_7, E_W_7),      # 196 rows: the last step has 4
        # -- a 3 x 3 window on a 2 x 2 map: stride 1 keeps all nine taps (five of them miss per pixel), stride 2 has one
        #    output pixel and four live taps; 160 channels = 5 steps per tap
        one("loop_nt_forward_2x2_map", 3, P(0, 4, 2, 2, 160, 64, 3, 3, 1, 1), E(0, 15, 3, 9)),
        one("loop_nt_dgrad_2x2_map", 2, P(1, 4, 2, 2, 160, 64, 3, 3, 1, 1), E(0, 9, 2, 9)),
        one("loop_nt_forward_2x2_map_dead_taps", 2, P(0, 4, 2, 2, 160, 160, 3, 3, 2, 1), E(0, 10, 2, 4)),
        one("loop_nt_dgrad_2x2_map_dead_taps", 2, P(1, 4, 2, 2, 160, 160, 3, 3, 2, 1), E(0, 10, 2, 4)),
        one("loop_tn_2x2_map", 1, P(2, 4, 2, 2, 160, 160, 3, 3, 1, 1), E(0, 1, 1, 9)),
        # -- strided data gradients: plain enumeration (below 2048 pixels) and by residue class, the classes' shares
        #    6 / 4 / 4 / 3 steps
        one("loop_nt_dgrad_strided_plain", 2, P(1, 4, 7, 7, 36, 36, 3, 3, 2, 1), E(0, 9, 2, 9)),
        one("loop_nt_dgrad_residue_classes", 6, D_CLS, E_D_CLS),
        # -- merged launches with mixed share lengths
        _named("loop_pair_6_and_3_steps", (6, 3), "dw_slabs", (D_6, W_OF_6), (E_F_6, E_W_OF_6)),
        _named("loop_pair_12_and_7_steps", (12, 7), "dw_slabs", (D_12, W_OF_12), (E_F_12, E_W_OF_12)),
        _named("loop_group_of_four_mixed", (7, 1, 6, 12), "group_slabs", (F_7, F_ONE, W_6, D_12),
               (E_F_7, E_F_ONE, E_W_6, E_F_12)),
        _named("loop_group_cls_with_plain", (6, 5, 3), "group_slabs", (D_CLS, W_OF_7, F_3), (E_D_CLS, E_W_OF_7, E_F_3)),
        # -- the BNSUM epilogue behind the loop (36 channels: a full step and a ragged one per tap; 196 rows)
        _named("loop_bnsum_single", (2,), "group_slabs_bnsum", (F_BN,), (E_F_BN,), (True,)),
        _named("loop_bnsum_group_mixed", (3, 2, 3), "group_slabs_bnsum", (F_BN49, F_BN, F_3), (E_F_BN49, E_F_BN, E_F_3),
               (True, True, False)),
    ]


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)

# the launch that carries the weight scatter (hf_conv2d_nhwc_slabs_unpack): its own test, no Case form
UNPACK = (F_UNPACK, E_F_UNPACK)

# Repeatability on N(0, 1) operands: three geometries of the ResNet-18 product (28 x 28 inputs) scaled to batch 2 --
# layer1's tangent convolution (2 * 64 channels), layer2's first data gradient (stride 2), layer3's weight gradient
PRODUCT_GEOMETRIES = [P(0, 2, 7, 7, 128, 64, 3, 3, 1, 1), P(1, 2, 7, 7, 64, 128, 3, 3, 2, 1), P(2, 2, 2, 2, 256, 256, 3, 3, 1, 1)]


def share_lengths(info):
    """Steps of one workgroup's share per residue class (plain enumeration: one entry), from a plan info."""
    if info["ncls"]:
        csteps = info["steps"] // max(info["cls_taps"])
        return tuple(-(-(t * csteps) // info["splits"]) for t in info["cls_taps"])
    return (-(-info["steps"] // info["splits"]),)
