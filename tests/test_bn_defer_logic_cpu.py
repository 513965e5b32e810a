"""CPU: the host logic of the deferred BatchNorm sums -- which unit defers (``defer_sums_ok``), the sums table's block
prefix as the library's own host function fills it (``hf_bn_sums_table``: no device is touched), and the contiguous
sub-ranges a set of pending table entries is launched as (``sums_runs``)."""

import ctypes

import pytest

import layer_refs as L
from pytorchhessianfree_amd import _lib
from pytorchhessianfree_amd.engine.buffers import _Buffers, adjoint_split_ok, defer_sums_ok, sums_runs, sums_table

MAX = _Buffers.DEFER_MAX_BYTES
BASE = dict(train=False, rb=64, hessian=False, has_gw=True, has_gb=True, map_bytes=MAX, max_bytes=MAX, enabled=True)

# one case per clause of the rule: (what changes against BASE, defers?)
CASES = [({}, True),
         ({"train": True}, False),                      # train mode: the elementwise pass needs the sums first
         ({"rb": 1}, False),                            # not the row-major kernel
         ({"rb": 2}, True),
         ({"hessian": True}, False),                    # _swap_first_order swaps the buffers a static table points to
         ({"has_gw": False, "has_gb": False}, False),   # frozen scale and shift: no sums at all
         ({"has_gw": False}, True),                     # ... one of the two is enough
         ({"has_gb": False}, True),
         ({"map_bytes": MAX + 4}, False),               # above the threshold the fused launch stays
         ({"map_bytes": 4}, True),
         ({"enabled": False}, False)]                   # HF_BN_SUMS_DEFER=0


@pytest.mark.parametrize("change,want", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_defer_sums_ok_clause_by_clause(change, want):
    assert defer_sums_ok(**{**BASE, **change}) is want


def test_a_unit_without_sums_still_takes_the_elementwise_launch():
    kw = {k: v for k, v in BASE.items() if k not in ("has_gw", "has_gb")}
    assert adjoint_split_ok(**kw) and not defer_sums_ok(**kw, has_gw=False, has_gb=False)
    for change in ({"train": True}, {"rb": 1}, {"hessian": True}, {"map_bytes": MAX + 4}, {"enabled": False}):
        assert not adjoint_split_ok(**{**kw, **change})


def test_elementwise_launch_is_decided_at_call_time_by_the_scales_alignment():
    """A scale bound at an unpadded offset of a flat vector (``utils.ParameterArena``) can sit on any 4-byte boundary."""
    import torch
    from types import SimpleNamespace as NS

    flat = torch.zeros(64)
    base = (-flat.data_ptr() // 4) % 4  # the first 16-byte aligned entry
    eng = _Buffers()
    eng.split_fallbacks = 0
    unit = NS(split=True, scale=flat[base:base + 8])
    assert eng._split_now(unit) and eng.split_fallbacks == 0
    for off in (1, 2, 3):
        unit.scale = flat[base + off:base + off + 8]
        assert not eng._split_now(unit)
    assert eng.split_fallbacks == 3
    unit.scale = flat[base + 4:base + 12]  # re-bound to an aligned place: elementwise again
    assert eng._split_now(unit)
    assert eng._split_now(NS(split=True, scale=None))  # a bias unit has no scale to load
    assert not eng._split_now(NS(split=False, scale=flat[base:base + 8])) and eng.split_fallbacks == 3


def test_threshold_covers_every_resnet18_map_and_not_the_largest_allcnnc_ones():
    assert MAX == 4 * 6272 * 64 * 4          # four times the stem's map (32 x 14 x 14 x 64 floats)
    assert 32 * 16 * 16 * 192 * 4 <= MAX     # All-CNN-C's 16 x 16 maps defer ...
    assert 32 * 32 * 32 * 96 * 4 > MAX       # ... its 32 x 32 maps keep the fused launch


def _problem(rows, c, rb, addr=0x10000, gw=True, gb=True):
    return dict(gw=addr if gw else None, gb=addr + 0x100 if gb else None, g=addr + 0x1000, x=addr + 0x2000 if gw else None,
                mean=addr + 0x3000, rstd=addr + 0x4000, rows=rows, c=c, row_blocks=rb)


SPECS = [(37, 4, 3), (200, 64, 14), (130, 260, 7), (64, 1024, 64), (1568, 64, 63)]


@pytest.mark.parametrize("count", [1, 2, 5])
def test_table_builder_block_prefix(count):
    tab, blocks = sums_table([_problem(*spec) for spec in SPECS[:count]])
    assert len(tab) == count and ctypes.sizeof(tab) == 72 * count
    prefix = 0
    for q, (rows, c, rb) in zip(tab, SPECS):
        assert (q.rows, q.c, q.row_blocks) == (rows, c, rb)
        assert q.block0 == prefix and q.rows_per_block == -(-rows // rb)
        assert L.row_shares(rows, rb)[-1][0] < rows  # (the shares the kernel walks: none empty)
        prefix += rb
    assert blocks == prefix


def test_table_builder_refuses_what_the_kernel_does_not_take():
    for bad in (_problem(8, 6, 2), _problem(8, 1028, 2), _problem(8, 12, 7), _problem(8, 12, 2, addr=0x10004),
                _problem(8, 12, 2, gw=False, gb=False), _problem(8, 12, 0)):
        with pytest.raises(_lib.Refused):
            sums_table([_problem(8, 12, 2), bad])
    assert not L.share_ok(8, 7)
    # a bias-only problem: x is dropped, nothing else changes
    tab, blocks = sums_table([_problem(8, 12, 2, gw=False)])
    assert blocks == 2 and tab[0].x is None and tab[0].gw is None


def test_sub_range_arithmetic():
    cap = _lib.BN_SUMS_MAX
    assert sums_runs(set(), cap) == []
    assert sums_runs({0, 1, 2, 3}, cap) == [(0, 4)]
    assert sums_runs({3, 1, 2}, cap) == [(1, 3)]                       # the middle of a table
    assert sums_runs({0, 1, 4, 5, 6, 9}, cap) == [(0, 2), (4, 3), (9, 1)]
    assert sums_runs(range(cap), cap) == [(0, cap)]
    assert sums_runs(range(cap + 1), cap) == [(0, cap), (cap, 1)]      # a second launch beyond the cap
    assert sums_runs(range(2, 2 * cap + 5), cap) == [(2, cap), (2 + cap, cap), (2 + 2 * cap, 3)]
    for pending in ({0}, {5, 6}, set(range(70))):
        runs = sums_runs(pending, cap)
        assert sorted(i for f, n in runs for i in range(f, f + n)) == sorted(pending)
        assert all(1 <= n <= cap for _, n in runs)
