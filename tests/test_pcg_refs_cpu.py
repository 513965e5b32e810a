"""CPU: the phase-level reference of the PCG kernels (``pcg_refs.py``) against the oracle, the decidability of every
fp32 scalar of the GPU case tables, the tables' coverage of instantiations and tile shapes, and hand-made checks of the
scalar block's bookkeeping."""

import numpy as np
import pytest
import torch

import pcg_refs as pr
from oracle import pcg as oracle_pcg

REASON_TEXT = {pr.MARTENS: oracle_pcg.REASON_MARTENS, pr.MAXITER: oracle_pcg.REASON_MAXITER,
               pr.DIVERGED: oracle_pcg.REASON_DIVERGED, pr.TOL: oracle_pcg.REASON_TOL}

# (name, n, mode, lam, warm, martens, max_iter, tol, atol, store)
WHOLE = [
    ("plain", 1000, pr.M_NONE, 0.0, False, False, 30, 1e-4, None, []),
    ("martens", 2049, pr.M_NONE, 0.3, False, True, 60, 0.0, None, [1, 4, 5, 99]),
    ("warm_diag", 777, pr.M_DIAG, 0.3, True, True, 25, 1e-6, None, [0, 1, 2]),
    ("diag_grid", 4100, pr.M_DIAG, 0.0, False, False, 12, 0.0, None, None),
    ("external", 515, pr.M_EXTERNAL, 0.3, True, True, 40, 1e-5, 1e-3, [0]),
    ("maxiter1", 5, pr.M_NONE, 0.0, True, False, 1, 1e-5, None, [0, 1]),
]


def _whole(case, dtype):
    name, n, mode, lam, warm, martens, max_iter, tol, atol, store = case
    d, b, minv, x0 = pr.make_inputs(dtype, n, ("whole", name), warm=warm)
    keep = oracle_pcg.snapshot_grid(max_iter) if store is None else store
    ref = pr.Ref(dtype, mode, x0, b, minv if mode == pr.M_DIAG else None, max_iter, tol, -1.0 if atol is None else atol,
                 martens, keep, bool(keep) and keep[0] == 0)
    pr.solve(ref, lambda p: d * p, lam, d * x0 + (dtype(lam) * x0 if lam else 0), lambda r: minv * r)
    td, tb, tm = torch.from_numpy(d), torch.from_numpy(b), torch.from_numpy(minv)
    A = (lambda v: td * v + lam * v) if lam else (lambda v: td * v)
    xs, ms, reason = oracle_pcg.pcg(A, tb, torch.from_numpy(x0) if warm else None, None if mode == pr.M_NONE else (lambda r: tm * r),
                                    max_iter, tol, atol, martens, keep, accumulate="fp64")
    return ref, xs, ms, reason


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_whole_solve_equals_the_oracle_bitwise_in_fp32(case):
    ref, xs, ms, reason = _whole(case, np.float32)
    assert ref.undecidable == []
    assert REASON_TEXT[ref.done] == reason
    mine = ref.x_iters()
    assert [x is None for x in mine] == [x is None for x in xs]
    for k, (a, o) in enumerate(zip(mine, xs)):
        if a is not None:
            assert pr.same(a, o.numpy()), (k, pr.diff(a, o.numpy()))
    if ms is None:
        assert ref.m_hist is None
    else:
        got = ref.m_hist[:ref.n_iters + 1]
        want = np.array([float(m) for m in ms], np.float32)
        assert pr.same(got, want), pr.diff(got, want)
        assert np.isnan(ref.m_hist[ref.n_iters + 1:]).all()


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_whole_solve_float64_has_the_oracles_reason_and_pattern(case):
    ref, xs, ms, reason = _whole(case, np.float64)
    assert REASON_TEXT[ref.done] == reason
    mine = ref.x_iters()
    assert [x is None for x in mine] == [x is None for x in xs]
    scale = float(np.abs(mine[-1]).max())
    assert float(np.abs(mine[-1] - xs[-1].numpy()).max()) <= 1e-9 * scale


def test_one_iteration_table_is_decidable_and_reaches_every_instantiation_and_tile_shape():
    scalars, seen, rows = 0, set(), set()
    for case in pr.one_iter_cases():
        for nt in (0, 1):
            seen |= pr.instantiations_of(case.dtype, case.mode, nt, nt)
        rows.add((np.dtype(case.dtype).name, case.name))
        if case.dtype is np.float32:
            ref = pr.run_one_iter_ref(case)
            assert ref.undecidable == [], case.id  # a condition on the table, not a tolerance: change SEED_SALT
            scalars += ref.scalars
            assert ref.iter_next == 2 and not ref.done, case.id
    assert scalars > 1000
    assert len(seen) == pr.N_INSTANTIATIONS == 40
    assert rows == {(np.dtype(dt).name, row[0]) for dt in pr.DTYPES for row in pr.lengths(dt)}
    assert len(pr.lengths(np.float32)) == 14 and len(pr.lengths(np.float64)) == 13  # (fp64: W - 1 == 1)


def test_length_table_grids_follow_the_tile_arithmetic():
    for dt in pr.DTYPES:
        W = pr.width(dt)
        for name, n, mb, g_init, g_k in pr.lengths(dt):
            nvec = n // W
            tiles = lambda u: max(1, -(-nvec // (pr.BLOCK * u)))  # noqa: E731
            cap = lambda t: min(t, mb) if mb else t  # noqa: E731
            assert (cap(tiles(1)), cap(tiles(pr.UNROLL))) == (g_init, g_k), (name, dt)
    assert pr.length_row(np.float32, "257T+W+3")[4] == 258 > pr.BLOCK  # second trip of reduce_partials' loop
    assert pr.length_row(np.float32, "257T+W+3")[1] < 530000


def test_trajectory_table_is_decidable_and_reaches_every_reason():
    reasons, combos = set(), set()
    for case in pr.traj_cases():
        ref = pr.run_traj_ref(case)
        sc = case.sc
        if case.dtype is np.float32:
            assert ref.undecidable == [], case.id
        assert ref.done == sc.reason, (case.id, ref.done, ref.n_iters)
        if sc.n_iters is not None:
            assert ref.n_iters == sc.n_iters, case.id
        if sc.name == "martens":
            assert ref.n_iters >= 11, case.id
        if sc.nonpos is not None:
            assert [i for i, _ in ref.nonpos] == sc.nonpos[:pr.NP_CAP] and ref.nonpos_count == len(sc.nonpos), case.id
        reasons.add(ref.done)
        combos.add((case.dtype, case.mode, case.name, case.nt))
    assert reasons == {pr.MARTENS, pr.MAXITER, pr.DIVERGED, pr.TOL}
    assert {c[:3] for c in combos} == {(dt, m, n) for dt in pr.DTYPES for m in pr.MODES for n in pr.TRAJ_LENGTHS}
    assert {c[3] for c in combos} == {0, 1}


# ---- bookkeeping, by hand ----------------------------------------------------------------------------------------------
def _small(store, max_iter, **kw):
    n = 300
    d, b, minv, x0 = pr.make_inputs(np.float32, n, ("hand", tuple(store), max_iter))
    ref = pr.Ref(np.float32, pr.M_NONE, x0, b, None, max_iter, 0.0, -1.0, False, store, bool(store) and store[0] == 0, **kw)
    return pr.solve(ref, lambda p: d * p, 0.0, d * x0), d


def test_slot_advance_with_zero_gaps_and_entries_past_max_iter():
    ref, _ = _small([0, 2, 5, 99, 99], 7, slab_stride=304)
    assert ref.done == pr.MAXITER and ref.n_iters == 7
    assert ref.slot_next == 3                                   # 0, 2 and 5 were stored; 99 never comes
    assert not np.isnan(ref.slab[:3, :300]).any() and np.isnan(ref.slab[3:]).all() and np.isnan(ref.slab[:, 300:]).all()
    assert np.all(ref.slab[0, :300] == 0)
    assert [x is not None for x in ref.x_iters()] == [True, False, True, False, False, True, False, True]
    ref, _ = _small([1, 3], 4)
    assert ref.slot_next == 2
    ref, _ = _small([1, 1, 2], 4)                               # a repeat is never reached: the cursor waits at it
    assert ref.slot_next == 1 and np.isnan(ref.slab[1:]).all()
    ref, _ = _small([], 3)
    assert ref.slot_next == 0 and ref.slab.shape[0] == 0


def _fabricated(max_iter, martens=True):
    ref = pr.Ref(np.float32, pr.M_NONE, np.zeros(4, np.float32), np.ones(4, np.float32), None, max_iter, 0.1, -1.0, martens)
    ref.init(np.zeros(4, np.float32))
    assert ref.res_bound == 0.1 * 2.0 and (not martens or ref.m_hist[0] == 0)
    return ref


def _k3(ref, it, m, rr=100.0):
    ref.iter_cur, ref.ry_cur, ref.slot_cur, ref.stored_cur = it, pr._point(np.float32(1)), 0, 0
    ref._sums.update(ry2=pr.Sum(1.0, 0.0, 1), rr=pr.Sum(rr, 0.0, 1), m=pr.Sum(2.0 * m, 0.0, 1))
    ref.update_p()


def test_martens_window_is_max_of_ten_and_a_tenth_of_the_iteration():
    ref = _fabricated(300)
    for it in range(1, 300):                                    # no progress at all: fires as soon as 10 < iter
        _k3(ref, it, -1.0)
        if ref.done:
            break
    assert (ref.done, ref.n_iters) == (pr.MARTENS, 11)
    ref = _fabricated(300)
    for it in range(1, 300):                                    # progress until 100, none afterwards
        _k3(ref, it, -float(it) if it <= 100 else -200.0)
        if ref.done:
            break
    assert (ref.done, ref.n_iters) == (pr.MARTENS, 112)        # window 11 at iteration 111 still sees m_100
    assert ref.m_hist[112] == -200 and np.isnan(ref.m_hist[113])


def test_order_of_the_four_termination_tests():
    ref = _fabricated(11)
    for it in range(1, 11):
        _k3(ref, it, -1.0)
    assert not ref.done
    _k3(ref, 11, -1.0, rr=pr.NAN)                               # Martens, max_iter and NaN at once
    assert ref.done == pr.MARTENS
    ref = _fabricated(3, martens=False)
    _k3(ref, 3, 0.0, rr=pr.NAN)
    assert ref.done == pr.MAXITER                               # max_iter before NaN
    ref = _fabricated(3, martens=False)
    _k3(ref, 3, 0.0, rr=1e-6)
    assert ref.done == pr.MAXITER                               # ... and before the tolerance
    ref = _fabricated(3, martens=False)
    _k3(ref, 2, 0.0, rr=pr.NAN)
    assert ref.done == pr.DIVERGED
    ref = _fabricated(3, martens=False)
    _k3(ref, 2, 0.0, rr=0.2 * 0.2 * 0.999)
    assert ref.done == pr.TOL and ref.last_res_norm < 0.2
    ref = _fabricated(3, martens=False)
    _k3(ref, 2, 0.0, rr=0.2 * 0.2 * 1.001)
    assert not ref.done and ref.iter_next == 3 and ref.last_beta == 1.0
    _k3(ref, 3, 0.0)
    before = ref.status()
    _k3(ref, 4, 0.0)                                            # after termination every phase is a no-op
    assert ref.status() == before and ref.flag == (pr.MAXITER, 3)


def test_nonpositive_curvature_log_overflows_at_its_capacity():
    case = next(c for c in pr.traj_cases() if c.sc.name == "negative40" and c.dtype is np.float32)
    ref = pr.run_traj_ref(case)
    assert ref.nonpos_count == 40 and len(ref.nonpos) == pr.NP_CAP == 32
    assert [i for i, _ in ref.nonpos] == list(range(1, 33)) and all(v < 0 for _, v in ref.nonpos)
    assert ref.done == pr.MAXITER and ref.n_iters == 40         # the solve goes on past them
