"""GPU: every instantiation and every grid shape of the PCG kernels of ``csrc/hf_pcg.hip`` -- ``k_init*``, K1
``k_curvature``, K2 ``k_update_xr``, ``k_dot_ry``, K3 ``k_update_p`` -- phase by phase on the raw C ABI against the
numpy reference of ``pcg_refs.py`` (its docstring states the rules), plus ``hf_axpy_out`` and ``hf_precond_build``.

Elementwise results (x, r, p, the snapshot slab) are compared BITWISE, in fp32 and fp64.  fp32 scalars are bitwise too
(the tables have no undecidable scalar: ``test_pcg_refs_cpu.py``); fp64 scalars must lie within the derived bound of the
exact sum and are then adopted, so every phase is still exact.  The operator is diagonal and applied on the host in T,
so ``Bp`` is the same bits on both sides.  Every vector a kernel writes lies between NaN guards (and the slab's padding
and the unwritten part of ``m_hist`` are NaN) that must survive; every input must come back unchanged.  Streaming
(non-temporal) on and off, set through ``hf_pcg_set_streaming``, must give identical bits everywhere.  Only
``hf_precond_build`` has a tolerance: the device's ``pow`` is not correctly rounded (measured, in ulps)."""

import ctypes
import math

import numpy as np
import pytest
import torch

import pcg_refs as pr
import tol
from guarded import DEV, GUARD, P, Payload, dev, p as _ptr, st as _st  # (p, st: names of locals here)
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
_CODE = {np.float32: _lib.HF_F32, np.float64: _lib.HF_F64}
ERR_ARG, ERR_ALIGN, ERR_STATE = -1, -2, -3
# hf_precond_build: worst distance seen on the MI355X from (diag + lambda)^(-a) evaluated in float64 and rounded to T was
# 1 ulp (fp32) / 1 ulp (fp64); asserted at 3x that (profiles/r15_pcg_tolerance_sites.jsonl)
POW_ULPS = {np.float32: 3.0, np.float64: 3.0}


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


class Handle:
    """One ``hf_pcg_create`` ... ``hf_pcg_destroy`` with the streaming flags set and the plan read back."""

    def __init__(self, dtype, n, max_blocks, nt):
        self.lib = _lib.load()
        self.dtype, self.n = dtype, n
        self.h = P()
        assert self.lib.hf_pcg_create(ctypes.byref(self.h), n, _CODE[dtype], max_blocks) == 0
        assert self.lib.hf_pcg_set_streaming(self.h, nt, nt) == 0
        self.plan = _lib.PcgPlan()
        assert self.lib.hf_pcg_plan_info(self.h, ctypes.byref(self.plan)) == 0
        assert (self.plan.nt_k12, self.plan.nt_k3) == (nt, nt)
        assert self.plan.width == pr.width(dtype)
        assert (self.plan.unroll_k1, self.plan.unroll_k2, self.plan.unroll_k3) == (pr.UNROLL,) * 3

    def grids(self):
        p = self.plan
        return (p.grid_init, p.grid_k1, p.grid_k2, p.grid_k3)

    def describe(self, mode):
        p = self.plan
        return (f"{np.dtype(self.dtype).name}/{pr.MODE_NAMES[mode]}/NT({p.nt_k12},{p.nt_k3})/n={self.n}/"
                f"grid init {p.grid_init} K1 {p.grid_k1} K2 {p.grid_k2} K3 {p.grid_k3} cap {p.grid_cap}")

    def close(self):
        assert self.lib.hf_pcg_destroy(self.h) == 0


class Solve:
    """One ``hf_pcg_begin`` on a handle with guarded outputs, and the phase calls of the raw ABI."""

    def __init__(self, handle, mode, b, minv, x0, max_iter, tol_, atol, martens, store_iters, store_x0, slab_stride):
        self.hd, self.lib, self.h, self.mode = handle, handle.lib, handle.h, mode
        T = self.T = np.dtype(handle.dtype).type
        n = self.n = handle.n
        self.x = Payload(x0.astype(T))
        self.r, self.p = Payload(np.full(n, pr.NAN, T)), Payload(np.full(n, pr.NAN, T))
        self.n_store = len(store_iters)
        self.slab = Payload(np.full(self.n_store * slab_stride, pr.NAN, T)) if self.n_store else None
        self.m_hist = Payload(np.full(max_iter + 1, pr.NAN, T)) if martens else None
        self.inputs = {"b": [b.astype(T), None]}
        if mode == pr.M_DIAG:
            self.inputs["minv"] = [minv.astype(T), None]
        if self.n_store:
            self.inputs["store_iters"] = [np.asarray(store_iters, np.int64), None]
        for rec in self.inputs.values():
            rec[1] = dev(rec[0])
        for name in ("Ax0", "Bp", "y"):
            self.inputs[name] = [np.zeros(n, T), torch.zeros(n, dtype=torch.from_numpy(np.zeros(1, T)).dtype, device=DEV)]
        dv = lambda name: _ptr(self.inputs[name][1]) if name in self.inputs else None  # noqa: E731
        rc = self.lib.hf_pcg_begin(self.h, _ptr(self.x.t), _ptr(self.r.t), _ptr(self.p.t), dv("b"), dv("minv"), mode,
                                   max_iter, tol_, atol, int(martens), dv("store_iters"), self.n_store, int(store_x0),
                                   _ptr(self.slab.t) if self.slab else None, slab_stride if self.n_store else 0,
                                   _ptr(self.m_hist.t) if self.m_hist else None)
        assert rc == 0, rc

    def _put(self, name, a):
        a = np.ascontiguousarray(a, self.T)
        self.inputs[name][0] = a
        self.inputs[name][1].copy_(torch.from_numpy(a))
        return _ptr(self.inputs[name][1])

    def init(self, Ax0):
        assert self.lib.hf_pcg_init(self.h, self._put("Ax0", Ax0), _st()) == 0

    def init_external(self, y):
        assert self.lib.hf_pcg_init_external(self.h, self._put("y", y), _st()) == 0

    def curvature(self, bp, lam):
        assert self.lib.hf_pcg_curvature(self.h, self._put("Bp", bp), lam, _st()) == 0

    def update_xr(self, lam):
        assert self.lib.hf_pcg_update_xr(self.h, _ptr(self.inputs["Bp"][1]), lam, _st()) == 0

    def update_p(self, y=None):
        assert self.lib.hf_pcg_update_p(self.h, self._put("y", y) if y is not None else None, _st()) == 0

    def iterate(self, bp, lam):
        assert self.lib.hf_pcg_iterate(self.h, self._put("Bp", bp), lam, _st()) == 0

    def finish(self):
        st = _lib.Status()
        assert self.lib.hf_pcg_finish(self.h, ctypes.byref(st), _st()) == 0
        return {name: getattr(st, name) for name, _ in _lib.Status._fields_}

    def poll(self):
        st = _lib.Status()
        assert self.lib.hf_pcg_poll(self.h, ctypes.byref(st)) == 0
        return st.reason, st.n_iters

    def nonpos(self):
        iters, vals = (_lib.c_int64 * 64)(), (_lib.c_double * 64)()
        c = self.lib.hf_pcg_read_nonpos(self.h, iters, vals, 64)
        assert c >= 0
        return [(iters[i], vals[i]) for i in range(c)]

    def outputs(self):
        return [("x", self.x), ("r", self.r), ("p", self.p)] + ([("slab", self.slab)] if self.slab else []) + \
            ([("m_hist", self.m_hist)] if self.m_hist else [])

    def snapshot(self):
        torch.cuda.synchronize()
        return {name: g.after() for name, g in self.outputs()}

    def scalars(self, st, it):
        """What the device reports of its scalars (float64 feedback for the reference)."""
        d = {"res_bound": st["res_bound"], "pAp": st["last_pAp"], "alpha": st["last_alpha"], "beta": st["last_beta"],
             "res_norm": st["last_res_norm"]}
        if self.m_hist:
            d["m_i"] = self.m_hist.t[it].item()
        return d

    def assert_matches(self, ref, where):
        """Everything the kernels may write equals the reference bitwise; guards and padding are still NaN."""
        snap = self.snapshot()
        want = {"x": ref.x, "r": ref.r, "p": ref.p, "slab": ref.slab, "m_hist": ref.m_hist}
        for name, g in self.outputs():
            exp = g.expect(want[name])
            assert pr.same(snap[name], exp), (where, name, pr.diff(snap[name][GUARD:-GUARD], exp[GUARD:-GUARD]),
                                              "guards: " + pr.diff(np.r_[snap[name][:GUARD], snap[name][-GUARD:]],
                                                                   np.r_[exp[:GUARD], exp[-GUARD:]]))
        return snap

    def assert_inputs_unchanged(self):
        torch.cuda.synchronize()
        for name, (host, dev) in self.inputs.items():
            got = dev.cpu().numpy()
            assert pr.same(got, host), (name, "an input was written")


def _assert_status(st, want, where):
    for key, w in want.items():
        g = st[key]
        assert g == w or (g != g and w != w), (where, key, g, w)


# ---- one full iteration, phase by phase, every instantiation over every tile shape -----------------------------------------
def _one_iteration(hd, case, d, b, minv, x0, ref):
    """Runs ``case`` on handle ``hd``; with ``ref`` every phase is compared with the reference.  Returns the snapshot and
    status after every phase."""
    T, lam, mode = np.dtype(case.dtype).type, case.lam, case.mode
    fb = case.dtype is np.float64
    sv = Solve(hd, mode, b, minv, x0, case.max_iter, case.tol, case.atol, case.martens, case.store_iters, case.store_x0,
               case.slab_stride)
    trail = []

    def step(where, apply_ref, it=None, finish=True):
        st = sv.finish() if finish else None
        if ref is not None:
            apply_ref(sv.scalars(st, it) if (fb and st is not None and it is not None) else None)
            snap = sv.assert_matches(ref, (case.id, where))
            if st is not None:
                _assert_status(st, ref.status(), (case.id, where))
        else:
            snap = sv.snapshot()
        trail.append((where, snap, st))

    with np.errstate(all="ignore"):
        ax0 = d * x0
    sv.init(ax0)
    if mode == pr.M_EXTERNAL:
        step("k_init", lambda dev: ref.init(ax0), finish=False)
        y0 = minv * (ref.r if ref is not None else trail[-1][1]["r"][GUARD:-GUARD])
        sv.init_external(y0)
        step("k_init_external", lambda dev: ref.init_external(y0, dev), it=0)
    else:
        step("k_init", lambda dev: ref.init(ax0, dev), it=0)
    p_now = trail[-1][1]["p"][GUARD:-GUARD]
    bp = (d * p_now).astype(T)
    sv.curvature(bp, lam)
    step("K1", lambda dev: ref.curvature(bp, lam))
    sv.update_xr(lam)
    step("K2", lambda dev: ref.update_xr(bp, lam, dev), it=1)
    y = (minv * trail[-1][1]["r"][GUARD:-GUARD]).astype(T) if mode == pr.M_EXTERNAL else None
    sv.update_p(y)
    step("K3", lambda dev: ref.update_p(y, dev), it=1)
    sv.assert_inputs_unchanged()
    st = trail[-1][2]
    assert st["done"] == 0 and st["iter_next"] == 2 and st["n_stored"] == len(case.store_iters)
    return trail


_ONE = [(dt, mode, lam, row) for dt in pr.DTYPES for mode in pr.MODES for lam in (0.0, 0.3) for row in pr.lengths(dt)]


@pytest.mark.parametrize("dtype,mode,lam,row", _ONE,
                         ids=[f"{np.dtype(dt).name}-{pr.MODE_NAMES[m]}-lam{lam}-n={row[0]}" for dt, m, lam, row in _ONE])
def test_one_iteration_phase_by_phase_bitwise_and_streaming_on_equals_off(dtype, mode, lam, row):
    trails = {}
    for nt in (0, 1):
        hd = Handle(dtype, row[1], row[2], nt)
        assert hd.grids() == (row[3], row[4], row[4], row[4]), (hd.grids(), row)  # the grids the table's row is about
        print("ran:", hd.describe(mode), sorted(pr.instantiations_of(dtype, mode, nt, nt)))
        for variant in "ab":
            case = pr.OneIter(dtype, mode, lam, row, variant)
            d, b, minv, x0 = case.inputs()
            ref = case.ref(b, minv, x0) if nt == 0 else None
            trails[nt, variant] = _one_iteration(hd, case, d, b, minv, x0, ref)
            if ref is not None and dtype is np.float32:
                assert ref.undecidable == []
        hd.close()
    for variant in "ab":  # streaming on == streaming off: every buffer, guard and status field, bit for bit
        for (where, s0, st0), (_, s1, st1) in zip(trails[0, variant], trails[1, variant]):
            for name in s0:
                assert np.array_equal(_bits(s0[name]), _bits(s1[name])), (variant, where, name, pr.diff(s1[name], s0[name]))
            if st0 is not None:
                _assert_status(st1, st0, (variant, where))


def test_streaming_policy_thresholds_and_refusals():
    lib = _lib.load()
    for n, flags in ((15999999, (0, 0)), (16000000, (1, 0)), (63999999, (1, 0)), (64000000, (1, 1))):
        h, plan = P(), _lib.PcgPlan()
        assert lib.hf_pcg_create(ctypes.byref(h), n, _lib.HF_F32, 0) == 0
        assert lib.hf_pcg_plan_info(h, ctypes.byref(plan)) == 0
        assert (plan.nt_k12, plan.nt_k3) == flags, n
        assert plan.grid_cap >= max(plan.grid_init, plan.grid_k1, plan.grid_k2, plan.grid_k3)
        assert lib.hf_pcg_destroy(h) == 0
    h, plan = P(), _lib.PcgPlan()
    assert lib.hf_pcg_create(ctypes.byref(h), 1000, _lib.HF_F64, 0) == 0
    assert lib.hf_pcg_plan_info(None, ctypes.byref(plan)) == ERR_ARG and lib.hf_pcg_plan_info(h, None) == ERR_ARG
    for bad in ((2, 0), (0, 2), (-2, 0), (0, -2)):
        assert lib.hf_pcg_set_streaming(h, *bad) == ERR_ARG
    assert lib.hf_pcg_set_streaming(None, 0, 0) == ERR_ARG
    for k12, k3 in ((1, 0), (0, 1), (1, 1), (-1, -1)):
        assert lib.hf_pcg_set_streaming(h, k12, k3) == 0
        assert lib.hf_pcg_plan_info(h, ctypes.byref(plan)) == 0
        assert (plan.nt_k12, plan.nt_k3) == (max(k12, 0), max(k3, 0))
    buf = torch.zeros(4 * 1000, dtype=torch.float64, device=DEV)
    x, r, p, b = (buf[i * 1000:(i + 1) * 1000] for i in range(4))
    assert lib.hf_pcg_begin(h, _ptr(x), _ptr(r), _ptr(p), _ptr(b), None, 0, 3, 0.0, -1.0, 0, None, 0, 0, None, 0, None) == 0
    assert lib.hf_pcg_set_streaming(h, 1, 1) == ERR_STATE          # a graph built since begin must not go stale
    assert lib.hf_pcg_plan_info(h, ctypes.byref(plan)) == 0 and (plan.nt_k12, plan.nt_k3) == (0, 0)
    assert lib.hf_pcg_begin(h, _ptr(buf[1:1001]), _ptr(r), _ptr(p), _ptr(b), None, 0, 3, 0.0, -1.0, 0, None, 0, 0, None, 0,
                            None) == ERR_ALIGN                      # refused before any launch
    assert lib.hf_pcg_destroy(h) == 0


# ---- whole trajectories -----------------------------------------------------------------------------------------------------
_TRAJ = pr.traj_cases()


def _device_iteration(sv, ref, case, d, minv, fb):
    """One iteration on the device and in the reference (hf_pcg_iterate, or the three phase calls for EXTERNAL)."""
    it = ref.iter_next
    bp = case.Bp(d, ref.p, it)
    if case.mode == pr.M_EXTERNAL:
        sv.curvature(bp, case.lam)
        sv.update_xr(case.lam)
        st = sv.finish()
        ref.curvature(bp, case.lam)
        ref.update_xr(bp, case.lam, sv.scalars(st, it) if fb else None)
        with np.errstate(all="ignore"):
            y = minv * ref.r
        sv.update_p(y)
        st = sv.finish()
        ref.update_p(y, sv.scalars(st, it) if fb else None)
    else:
        sv.iterate(bp, case.lam)
        st = sv.finish()
        ref.iterate(bp, case.lam, None, sv.scalars(st, it) if fb else None)
    _assert_status(st, ref.status(), (case.id, "iteration", it))
    return bp


@pytest.mark.parametrize("case", _TRAJ, ids=[c.id for c in _TRAJ])
def test_trajectory_bitwise_to_termination_and_no_ops_afterwards(case):
    sc, fb = case.sc, case.dtype is np.float64
    d, b, minv, x0 = case.inputs()
    hd = Handle(case.dtype, case.n, case.max_blocks, case.nt)
    assert hd.grids() == (case.grid_init, case.grid_k, case.grid_k, case.grid_k)
    print("ran:", hd.describe(case.mode), sc.name)
    sv = Solve(hd, case.mode, b, minv, x0, sc.max_iter, sc.tol, case.atol, sc.martens, case.store_iters, case.store_x0,
               case.slab_stride)
    ref = case.ref(b, minv, x0)
    with np.errstate(all="ignore"):
        ax0 = d * x0
    sv.init(ax0)
    if case.mode == pr.M_EXTERNAL:
        ref.init(ax0)
        y0 = minv * ref.r
        sv.init_external(y0)
        ref.init_external(y0, sv.scalars(sv.finish(), 0) if fb else None)
    else:
        ref.init(ax0, sv.scalars(sv.finish(), 0) if fb else None)
    assert sv.poll() == (0, 0)
    bp = None
    while not ref.done:
        assert ref.iter_next <= sc.max_iter
        bp = _device_iteration(sv, ref, case, d, minv, fb)
    final = sv.assert_matches(ref, (case.id, "final"))
    st = sv.finish()
    _assert_status(st, ref.status(), (case.id, "final"))
    if case.dtype is np.float32:
        assert ref.undecidable == []
    # the scenario is what the table says it is
    assert st["done"] == sc.reason and (sc.n_iters is None or st["n_iters"] == sc.n_iters)
    if sc.name == "martens":
        assert st["n_iters"] >= 11
    if sc.name == "atol_dominates":
        assert st["res_bound"] == case.atol
    if ref.m_hist is not None:  # exactly n_iters + 1 entries of m_hist are written
        m = final["m_hist"][GUARD:-GUARD]
        assert not np.isnan(m[:st["n_iters"] + 1]).any() or sc.reason == pr.DIVERGED
        assert np.isnan(m[st["n_iters"] + 1:]).all()
    if sc.store:
        assert st["n_stored"] == sum(1 for s in sc.store if s <= st["n_iters"])
    got = sv.nonpos()
    assert st["nonpos_count"] == ref.nonpos_count and len(got) == min(ref.nonpos_count, pr.NP_CAP)
    for (gi, gv), (wi, wv) in zip(got, ref.nonpos):
        assert gi == wi and (gv == wv or (gv != gv and wv != wv)), (gi, gv, wi, wv)
    if sc.nonpos is not None:
        assert [i for i, _ in got] == sc.nonpos[:pr.NP_CAP] and st["nonpos_count"] == len(sc.nonpos)
    # after termination: three more full iterations change nothing, and the host mirror agrees with finish
    assert sv.poll() == (st["reason"], st["n_iters"])
    for _ in range(3):
        if case.mode == pr.M_EXTERNAL:
            sv.curvature(bp, case.lam)
            sv.update_xr(case.lam)
            sv.update_p(minv * ref.r)
        else:
            sv.iterate(bp, case.lam)
    again = sv.snapshot()
    for name in final:
        assert np.array_equal(_bits(final[name]), _bits(again[name])), (case.id, "after termination", name)
    _assert_status(sv.finish(), st, (case.id, "after termination"))
    assert sv.poll() == (st["reason"], st["n_iters"])
    sv.assert_inputs_unchanged()
    hd.close()


# ---- the per-iteration graph -----------------------------------------------------------------------------------------------
def _graph_problem(dtype, mode, key, lam, store, martens):
    name, n, mb, _, _ = pr.length_row(dtype, "7T+2W+3,mb3")
    d, b, minv, x0 = pr.make_inputs(dtype, n, ("graph", key, mode), warm=True)
    W = pr.width(dtype)
    return dict(n=n, mb=mb, d=d, b=b, minv=minv, x0=x0, lam=lam, store=store, martens=martens, max_iter=6,
                stride=(n + W - 1) // W * W + 4 * W)


def _run_problem(hd, mode, pb, launch):
    """``launch(sv, it)`` enqueues one iteration whose product is already in the solve's Bp buffer."""
    T = np.dtype(hd.dtype).type
    sv = Solve(hd, mode, pb["b"], pb["minv"], pb["x0"], pb["max_iter"], 0.0, -1.0, pb["martens"], pb["store"],
               bool(pb["store"]) and pb["store"][0] == 0, pb["stride"])
    yield sv          # (the caller builds / refreshes its graph between begin and init)
    sv.init(pb["d"] * pb["x0"])
    trail = []
    for it in range(1, pb["max_iter"] + 1):
        p_now = sv.snapshot()["p"][GUARD:-GUARD]
        sv._put("Bp", (pb["d"] * p_now).astype(T))
        launch(sv, it)
        trail.append((sv.snapshot(), sv.finish()))
    sv.assert_inputs_unchanged()
    yield trail


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mode", (pr.M_NONE, pr.M_DIAG), ids=lambda m: pr.MODE_NAMES[m])
def test_iteration_graph_is_bitwise_iterate_also_after_update_and_timed(dtype, mode):
    lib = _lib.load()
    first = _graph_problem(dtype, mode, 1, 0.0, [0, 1, 2], True)
    second = _graph_problem(dtype, mode, 2, 0.3, [1, 4, 5, 99], True)   # other x / b / slab / m_hist, damping 0 -> 0.3
    n, mb = first["n"], first["mb"]

    def direct(pb):
        hd = Handle(dtype, n, mb, 0)
        def iterate(sv, it):
            assert lib.hf_pcg_iterate(sv.h, _ptr(sv.inputs["Bp"][1]), pb["lam"], _st()) == 0

        run = _run_problem(hd, mode, pb, iterate)
        next(run)
        trail = next(run)
        hd.close()
        return trail

    want = [direct(first), direct(second)]
    hd = Handle(dtype, n, mb, 0)
    print("ran:", hd.describe(mode), "hf_pcg_graph")
    g = P()
    timed = []

    def launch(sv, it):
        t = int(len(solves) == 2 and it % 2 == 0)  # second solve: every other launch through the timed executable
        assert lib.hf_pcg_graph_launch(g, t, _st()) == 0
        if t:
            assert lib.hf_pcg_graph_collect_timing(g) == 0
            timed.append(it)

    solves = []
    run = _run_problem(hd, mode, first, launch)
    solves.append(next(run))
    bp_ptr = _ptr(solves[0].inputs["Bp"][1])
    assert lib.hf_pcg_graph_create(ctypes.byref(g), hd.h, None, bp_ptr, first["lam"], 1) == 0
    got = [next(run)]
    run = _run_problem(hd, mode, second, launch)
    solves.append(next(run))                                               # a second hf_pcg_begin on the same handle
    assert lib.hf_pcg_graph_update(g, _ptr(solves[1].inputs["Bp"][1]), second["lam"]) == 0
    got.append(next(run))
    for k, (w, gt) in enumerate(zip(want, got)):
        for it, ((ws, wst), (gs, gst)) in enumerate(zip(w, gt), 1):
            for name in ws:
                assert np.array_equal(_bits(ws[name]), _bits(gs[name])), (k, it, name, pr.diff(gs[name], ws[name]))
            _assert_status(gst, wst, (k, it))
    assert timed == [2, 4, 6]                                              # the timed executable ran, same bits
    ms = [_lib.c_double() for _ in range(3)]
    cnt = _lib.c_int64()
    assert lib.hf_pcg_timing_read(hd.h, *[ctypes.byref(m) for m in ms], ctypes.byref(cnt)) == 0
    assert cnt.value == len(timed) and all(m.value >= 0 for m in ms)
    assert lib.hf_pcg_graph_destroy(g) == 0
    hd.close()


# ---- vector helpers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pr.DTYPES, ids=lambda d: np.dtype(d).name)
def test_axpy_out_bitwise_aligned_offset_and_in_place(dtype):
    lib, T = _lib.load(), np.dtype(dtype).type
    alpha = 0.37
    for name, n, _, _, _ in pr.lengths(dtype):
        g = np.random.default_rng(pr.seed_of("axpy", name, np.dtype(dtype).name))
        a, s = g.standard_normal(n + 1).astype(T), g.standard_normal(n + 1).astype(T)
        for off, in_place in ((0, False), (1, False), (0, True), (1, True)):
            want = a[off:off + n] + (T(alpha) * s[off:off + n])
            da, ds = Payload(a), dev(s)
            out = da if in_place else Payload(np.full(n + 1, pr.NAN, T))
            rc = lib.hf_axpy_out(_ptr(out.t[off:off + n]), _ptr(da.t[off:off + n]), _ptr(ds[off:off + n]), alpha, n,
                                 _CODE[dtype], _st())
            assert rc == 0
            exp = out.before.copy()
            exp[GUARD + off:GUARD + off + n] = want
            got = out.after()
            assert pr.same(got, exp), (name, off, in_place, pr.diff(got, exp))
            assert pr.same(ds.cpu().numpy(), s) and (in_place or pr.same(da.after(), da.before))


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=lambda d: np.dtype(d).name)
def test_precond_build_against_float64_power_in_ulps(dtype):
    lib, T = _lib.load(), np.dtype(dtype).type
    n, lam = 10007, 0.3
    g = np.random.default_rng(pr.seed_of("precond", np.dtype(dtype).name))
    diag = (g.random(n) * 3).astype(T)
    diag[:4] = T(0), T(1) - T(lam), T(1e-6), T(1e4)
    for exponent in (0.75, 1.0, 0.5):
        out, dd = Payload(np.full(n, pr.NAN, T)), dev(diag)
        assert lib.hf_precond_build(_ptr(out.t), _ptr(dd), lam, exponent, n, _CODE[dtype], _st()) == 0
        base = (diag + T(lam)).astype(np.float64)                    # the kernel's own base, exact in float64
        want = np.array([math.pow(v, float(T(-exponent))) for v in base.tolist()]).astype(T)
        got = out.after()
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[-GUARD:]).all() and pr.same(dd.cpu().numpy(), diag)
        ulps = float(np.max(np.abs(got[GUARD:-GUARD].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))))
        print(f"hf_precond_build {np.dtype(dtype).name} exponent {exponent}: worst {ulps} ulp")
        tol.within(ulps, POW_ULPS[dtype], strict=False, note=(np.dtype(dtype).name, exponent))
