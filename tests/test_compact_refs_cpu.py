"""CPU: the numpy definition of the compact layout (``compact_refs``) and the coverage of its case table -- every branch
of ``k_pack`` that a launch into the compact layout can take has a case, in the dtype and mode that reach it."""

import numpy as np
import pack_refs as pr
import pytest

import compact_refs as cr


def test_every_branch_reachable_in_compact_mode_has_a_case():
    seen_masked, seen_other, blocks = set(), set(), 0
    for case in cr.CASES:
        for dtype in case.dtypes:
            for mode in (0, 1):
                for name, nblk, is_masked in cr.case_paths(case, dtype, mode):
                    (seen_masked if is_masked else seen_other).add(name)
                    blocks = max(blocks, nblk or 0)
    assert seen_masked == set(cr.COMPACT_PATHS), sorted(set(cr.COMPACT_PATHS) ^ seen_masked)
    assert set(cr.REACHABLE) <= seen_other | seen_masked, sorted(set(cr.REACHABLE) - seen_other - seen_masked)
    assert set(cr.REACHABLE) | {"live_zero_stream", "live_walk"} == set(pr.PACK_PATHS)
    assert blocks > 1  # (a masked tensor shared among several workgroups)


@pytest.mark.parametrize("case", cr.CASES, ids=[c.name for c in cr.CASES])
def test_scatter_of_gather_zeroes_the_dead_entries_only(case):
    segs, n = cr.segments(case.srcs)
    idx = cr.compact_index(case.srcs)
    offs, n_live = cr.compact_offsets(case.srcs)
    assert idx.size == n_live and np.all(np.diff(idx) > 0) and sum(s.numel for s in case.srcs) == n
    v = np.random.RandomState(1).standard_normal(n)
    back = cr.scatter(cr.gather(v, case.srcs), case.srcs)
    dead = np.ones(n, bool)
    dead[idx] = False
    assert np.array_equal(back[~dead], v[~dead]) and not back[dead].any()
    # dead entries: exactly the taps outside the mask of the masked tensors
    off = 0
    for s, c0, nl in zip(case.srcs, offs, cr.periods(case.srcs)):
        d = dead[off:off + s.numel]
        if nl:
            taps = np.array([not (s.live >> t) & 1 for t in range(s.perm[1])])
            assert np.array_equal(d.reshape(-1, s.perm[1]), np.broadcast_to(taps, (s.numel // s.perm[1], s.perm[1])))
            # compact position of (o, i, tap): (o*I + i)*nl + rank(tap)
            g = 5 % (s.numel // s.perm[1])
            live_taps = [t for t in range(s.perm[1]) if (s.live >> t) & 1]
            assert [int(i) for i in idx[c0 + g * nl:c0 + (g + 1) * nl]] == [off + g * s.perm[1] + t for t in live_taps]
        else:
            assert not d.any()
        off += s.numel


def test_compact_gather_of_the_reference_pack_ignores_dead_sources():
    """``pack_ref`` never looks at the NaN source entries of dead taps, so its compact image is finite."""
    case = cr.CASES[0]
    _, sources = cr.make_sources(case, np.float32, 3)
    n = sum(s.numel for s in case.srcs)
    flat = pr.pack_ref(np.zeros(n, np.float32), sources, 1.0, 0)
    assert np.isfinite(cr.gather(flat, case.srcs)).all()
