"""TEST INFRASTRUCTURE ONLY -- a phase-level numpy reference of the PCG kernels of ``csrc/hf_pcg.hip`` in the kernels'
own arithmetic, and the case tables of ``test_pcg_refs_cpu.py`` / ``test_pcg_kernels_gpu.py``.

One method of :class:`Ref` per device phase (``init``, ``init_external``, ``curvature`` = K1, ``update_xr`` = K2,
``dot_ry``, ``update_p`` = K3); the object keeps what the device keeps: x, r, p, the snapshot slab, ``m_hist`` and the
scalar block (ry, iter, slot, stored, res_bound, done, n_iters, the non-positive-curvature log).

Rules
  * ELEMENTWISE values are computed in the vector's dtype T with numpy ufuncs, one rounding per operation, written as
    the kernel writes them: ``bp + (lam * p)`` when damped else ``bp`` (lam cast to T); ``x + (alpha * p)``;
    ``r + (alpha * ap)``; ``minv * r``; ``(-y) + (beta * p)``; ``(r - b)`` rounded to T before its product with x.
    The library is built without contraction, so these are compared BITWISE.
  * REDUCTIONS: the terms are ``(double)a * (double)b`` -- exact for fp32, rounded once for fp64, as in the kernel --
    and are summed exactly (``math.fsum``): S.  The device adds the same terms in fp64 in some order, which moves the
    sum by at most ``e = n_terms * 2^-53 * sum|term|`` (derived, not measured; plus the half ulp of S itself).  An
    all-zero sum is exact (e = 0, and +0 as on the device, whose accumulators start at +0).
  * SCALARS are intervals in T: a dot product is ``[T(S-e), T(S+e)]``, a norm ``[T(sqrt(S-e) - ulp64),
    T(sqrt(S+e) + ulp64)]`` (one fp64 ulp for the device's sqrt); float64 intervals with e > 0 are widened by one ulp of
    T.  A NaN sum is the exact scalar NaN.
      - fp32: a scalar is DECIDABLE when both ends are the same float; then it is known bitwise.  A case whose scalars
        are all decidable has a bitwise trajectory with no feedback from the device.  ``Ref.undecidable`` lists the
        others (the tables below are chosen to have none: change a seed, never skip a case).
      - fp64 (``dev=`` given): the device's scalar must lie inside the interval and is then ADOPTED, so the elementwise
        output of every phase is predicted bitwise from the device's own ``alpha`` / ``beta`` even though two float64
        trajectories separate.  ``ry`` is not reported by ``hf_pcg_status``; it stays an interval, and ``alpha = ry/pAp``
        / ``beta = ry_new/ry_old`` must lie between the IEEE quotients of the interval ends (in fp32: be that quotient).
  * Without ``dev`` and for float64 every scalar is ``T(S)`` (a whole solve on the CPU, ``solve``).
"""

import math
import zlib

import numpy as np

M_NONE, M_DIAG, M_EXTERNAL = 0, 1, 2
RUNNING, MARTENS, MAXITER, DIVERGED, TOL = 0, 1, 2, 3, 4
NP_CAP = 32
BLOCK = 256
UNROLL = 2  # HF_U1 = HF_U2 = HF_U3
NAN = float("nan")
DTYPES = (np.float32, np.float64)
MODES = (M_NONE, M_DIAG, M_EXTERNAL)
MODE_NAMES = {M_NONE: "none", M_DIAG: "diag", M_EXTERNAL: "ext"}


def width(dtype):
    return 16 // np.dtype(dtype).itemsize


def same(a, b):
    """Bitwise equality of two arrays / scalars, any NaN equal to any NaN (x86 and gfx950 sign their NaNs differently)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    iv = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))))


def diff(got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    iv = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    bad = np.nonzero(~((got.view(iv) == want.view(iv)) | (np.isnan(got) & np.isnan(want))))[0]
    if bad.size == 0:
        return "equal"
    k = int(bad[0])
    return f"{bad.size} of {got.size} entries differ, first at {k}: {got[k]!r} != {want[k]!r}"


# ---- reductions --------------------------------------------------------------------------------------------------------
class Sum:
    """Exact sum S of the fp64 terms and the bound e on what any fp64 summation order can move it by."""

    def __init__(self, S, e, n):
        self.S, self.e, self.n = S, e, n


def exact_sum(a, b):
    with np.errstate(all="ignore"):
        t = a.astype(np.float64) * b.astype(np.float64)
    n = t.size
    if n == 0:
        return Sum(0.0, 0.0, 0)
    if not np.isfinite(t).all():
        with np.errstate(all="ignore"):
            s = float(np.sum(t))
        return Sum(s, 0.0 if s != s else math.inf, n)
    mag = float(np.abs(t).sum()) * (1.0 + 2.0 ** -20)  # (numpy's own summation error of the magnitudes)
    if mag == 0.0:
        return Sum(0.0, 0.0, n)
    S = math.fsum(t.tolist())
    if S == 0.0:
        S = 0.0
    return Sum(S, n * 2.0 ** -53 * mag + float(np.spacing(abs(S))), n)


class Iv:
    """A scalar of type T known to lie in [lo, hi]; ``mid`` = T(S) resp. the quotient of the mids."""

    def __init__(self, lo, hi, mid, free=False):
        self.lo, self.hi, self.mid, self.free = lo, hi, mid, free  # free: no statement (a quotient by an interval with 0)

    @property
    def exact(self):
        return not self.free and same(self.lo, self.hi)

    def holds(self, v):
        if self.free:
            return True
        if self.lo != self.lo:
            return bool(v != v)
        if self.exact:
            return bool(v == self.lo)  # (-0 == +0)
        return bool(self.lo <= v <= self.hi)

    def __repr__(self):
        return f"[{self.lo!r}, {self.hi!r}]"


def _point(v):
    return Iv(v, v, v)


def iv_dot(s, T):
    with np.errstate(all="ignore"):
        if s.S != s.S:
            return _point(T(NAN))
        lo, hi, mid = T(s.S - s.e), T(s.S + s.e), T(s.S)
        if T is np.float64 and s.e > 0:
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return Iv(lo, hi, mid)


def iv_norm(s, T):
    with np.errstate(all="ignore"):
        if s.S != s.S:
            return _point(T(NAN))
        mid = T(math.sqrt(s.S)) if s.S >= 0 else T(NAN)
        if s.e == 0:
            return _point(mid)
        lo = np.nextafter(np.float64(math.sqrt(max(s.S - s.e, 0.0))), -np.inf)
        hi = np.nextafter(np.float64(math.sqrt(s.S + s.e)), np.inf)
        lo, hi = T(max(lo, 0.0)), T(hi)
        if T is np.float64:
            lo, hi = T(max(np.nextafter(lo, -np.inf), 0.0)), np.nextafter(hi, np.inf)
    return Iv(lo, hi, mid)


def iv_half(iv, T):
    with np.errstate(all="ignore"):
        return Iv(T(0.5) * iv.lo, T(0.5) * iv.hi, T(0.5) * iv.mid)


def iv_div(num, den):
    """IEEE quotients in T of the interval ends (division is monotone in each operand on a sign-definite interval)."""
    with np.errstate(all="ignore"):
        mid = num.mid / den.mid
        if num.exact and den.exact:
            return _point(num.lo / den.lo)
        if den.lo != den.lo or num.lo != num.lo:
            return _point(type(mid)(NAN))
        if den.lo <= 0 <= den.hi:
            return Iv(mid, mid, mid, free=True)
        q = [a / b for a in (num.lo, num.hi) for b in (den.lo, den.hi)]
    return Iv(min(q), max(q), mid)


# ---- the phases --------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, dtype, mode, x0, b, minv=None, max_iter=10, tol=1e-5, atol=-1.0, martens=False, store_iters=(),
                 store_x0=False, slab_stride=None):
        T = self.T = np.dtype(dtype).type
        self.mode, self.n = mode, b.size
        self.x, self.b, self.minv = x0.astype(T).copy(), b.astype(T), None if minv is None else minv.astype(T)
        self.r, self.p = np.full(self.n, NAN, T), np.full(self.n, NAN, T)
        self.max_iter, self.tol, self.atol = int(max_iter), float(tol), float(atol)
        self.store_iters = [int(s) for s in store_iters]
        self.n_store, self.store_x0 = len(self.store_iters), bool(store_x0)
        assert not (self.store_x0 and self.n_store == 0)
        self.slab_stride = self.n if slab_stride is None else int(slab_stride)
        self.slab = np.full((self.n_store, self.slab_stride), NAN, T)
        self.m_hist = np.full(self.max_iter + 1, NAN, T) if martens else None
        self.inited = False
        self.scalars, self.undecidable = 0, []
        self._sums = {}
        self.flag = (0, 0)  # the pinned host mirror hf_pcg_poll reads: (reason, terminating iteration)

    # -- scalar bookkeeping
    def _take(self, name, iv, dev):
        """The value of a scalar the device reports: the device's (checked against the interval) or the reference's."""
        self.scalars += 1
        if dev is not None:
            v = self.T(dev[name])
            assert iv.holds(v), f"{name} at iteration {getattr(self, 'iter_next', 0)}: device {v!r} outside {iv!r}"
            return v
        if self.T is np.float32 and not iv.exact:
            self.undecidable.append((name, getattr(self, "iter_next", 0), repr(iv)))
        return iv.mid

    def _keep(self, name, iv, dev):
        """A scalar the device does not report (ry): an interval under feedback, else a point."""
        self.scalars += 1
        if dev is not None:
            return iv
        if self.T is np.float32 and not iv.exact:
            self.undecidable.append((name, getattr(self, "iter_next", 0), repr(iv)))
        return _point(iv.mid)

    def _ap(self, Bp, lam):
        T = self.T
        Bp = Bp.astype(T)
        with np.errstate(all="ignore"):
            return Bp + (T(lam) * self.p) if lam != 0.0 else Bp

    # -- init
    def init(self, Ax0, dev=None):
        T = self.T
        with np.errstate(all="ignore"):
            self.r = Ax0.astype(T) - self.b
            self._sums = {"bb": exact_sum(self.b, self.b), "m0": exact_sum(self.r - self.b, self.x)}
            if self.mode != M_EXTERNAL:
                y = self.minv * self.r if self.mode == M_DIAG else self.r
                self._sums["ry"] = exact_sum(self.r, y)
                self.p = -y
        if self.store_x0:
            self.slab[0, :self.n] = self.x
        if self.mode != M_EXTERNAL:
            self._finalize(dev)

    def init_external(self, y, dev=None):
        assert self.mode == M_EXTERNAL
        y = y.astype(self.T)
        self._sums["ry"] = exact_sum(self.r, y)
        self.p = -y
        self._finalize(dev)

    def _finalize(self, dev):
        T = self.T
        self.iter_next = 0
        ry = self._keep("ry", iv_dot(self._sums["ry"], T), dev)
        bn = iv_norm(self._sums["bb"], T)

        def bound(v):
            bd = self.tol * float(v)
            return max(bd, self.atol) if self.atol >= 0.0 else bd

        bd = Iv(np.float64(bound(bn.lo)), np.float64(bound(bn.hi)), np.float64(bound(bn.mid)))
        self.res_bound = float(self._take_bound(bd, dev))
        if self.m_hist is not None:
            self.m_hist[0] = self._take("m_i", iv_half(iv_dot(self._sums["m0"], T), T), dev)
        self.ry_next, self.iter_next = ry, 1
        self.slot_next = 1 if (self.n_store > 0 and self.store_iters[0] == 0) else 0
        self.ry_cur, self.iter_cur, self.slot_cur, self.stored_cur = _point(T(0)), 0, 0, 0
        self.n_iters, self.done = 0, 0
        self.last_alpha = self.last_beta = self.last_pAp = self.last_res_norm = 0.0
        self.nonpos_count, self.nonpos = 0, []
        self.flag = (0, 0)
        self.inited = True

    def _take_bound(self, iv, dev):
        """res_bound: a double on the device whatever T is."""
        self.scalars += 1
        if dev is not None:
            v = np.float64(dev["res_bound"])
            assert iv.holds(v), f"res_bound: device {v!r} outside {iv!r}"
            return v
        if self.T is np.float32 and not iv.exact:
            self.undecidable.append(("res_bound", 0, repr(iv)))
        return iv.mid

    # -- K1
    def curvature(self, Bp, lam):
        if self.done:
            return
        self._sums["pAp"] = exact_sum(self.p, self._ap(Bp, lam))

    # -- K2
    def update_xr(self, Bp, lam, dev=None):
        if self.done:
            return
        T = self.T
        pAp = self._take("pAp", iv_dot(self._sums["pAp"], T), dev)
        alpha = self._take("alpha", iv_div(self.ry_next, _point(pAp)), dev)
        it, slot = self.iter_next, self.slot_next
        store = slot < self.n_store and self.store_iters[slot] == it
        self.ry_cur, self.iter_cur, self.slot_cur, self.stored_cur = self.ry_next, it, slot, int(store)
        self.last_pAp, self.last_alpha = float(pAp), float(alpha)
        if not (pAp > 0):
            if self.nonpos_count < NP_CAP:
                self.nonpos.append((it, float(pAp)))
            self.nonpos_count += 1
        with np.errstate(all="ignore"):
            ap = self._ap(Bp, lam)
            self.x = self.x + (alpha * self.p)
            self.r = self.r + (alpha * ap)
            if store:
                self.slab[slot, :self.n] = self.x
            rr = exact_sum(self.r, self.r)
            self._sums["rr"] = rr
            self._sums["m"] = exact_sum(self.r - self.b, self.x)
            if self.mode == M_NONE:
                self._sums["ry2"] = rr
            elif self.mode == M_DIAG:
                self._sums["ry2"] = exact_sum(self.r, self.minv * self.r)

    # -- k_dot_ry (launched by hf_pcg_update_p in front of K3)
    def dot_ry(self, y):
        if self.done:
            return
        self._sums["ry2"] = exact_sum(self.r, y.astype(self.T))

    # -- K3
    def update_p(self, y=None, dev=None):
        if self.done:
            return
        T = self.T
        it = self.iter_cur
        if self.mode == M_EXTERNAL:
            self.dot_ry(y)
        ry_old = self.ry_cur
        ry_new = self._keep("ry", iv_dot(self._sums["ry2"], T), dev)
        res_norm = self._take("res_norm", iv_norm(self._sums["rr"], T), dev)
        reason = RUNNING
        with np.errstate(all="ignore"):
            if self.m_hist is not None:
                m_i = self._take("m_i", iv_half(iv_dot(self._sums["m"], T), T), dev)
                k = max(it // 10, 10)
                if k < it:
                    num = m_i - self.m_hist[it - k]
                    den = m_i - self.m_hist[0]
                    if T(num / den) < T(5e-4):
                        reason = MARTENS
            if reason == RUNNING:
                if it >= self.max_iter:
                    reason = MAXITER
                elif res_norm != res_norm:
                    reason = DIVERGED
                elif res_norm < T(self.res_bound):
                    reason = TOL
        if self.m_hist is not None:
            self.m_hist[it] = m_i
        self.last_res_norm = float(res_norm)
        self.slot_next = self.slot_cur + self.stored_cur
        if reason != RUNNING:
            self.n_iters, self.done = it, reason
            self.flag = (reason, min(it, 0x7fffffff))
            return
        beta = self._take("beta", iv_div(ry_new, ry_old), dev)
        self.ry_next, self.iter_next, self.last_beta = ry_new, it + 1, float(beta)
        with np.errstate(all="ignore"):
            yv = y.astype(T) if self.mode == M_EXTERNAL else (self.minv * self.r if self.mode == M_DIAG else self.r)
            self.p = (-yv) + (beta * self.p)

    def iterate(self, Bp, lam, y_of_r=None, dev=None):
        self.curvature(Bp, lam)
        self.update_xr(Bp, lam, dev)
        self.update_p(y_of_r(self.r) if self.mode == M_EXTERNAL and not self.done else None, dev)

    def status(self):
        """The fields of ``hf_pcg_status`` as ``hf_pcg_finish`` fills them."""
        return {"done": self.done, "reason": self.done, "n_iters": self.n_iters, "iter_next": self.iter_next,
                "nonpos_count": self.nonpos_count, "last_alpha": self.last_alpha, "last_beta": self.last_beta,
                "last_pAp": self.last_pAp, "last_res_norm": self.last_res_norm, "res_bound": self.res_bound,
                "n_stored": self.slot_next}

    def x_iters(self):
        """The reference's ``x_iters`` list: the stored iterates, ``None`` elsewhere, the final iterate always."""
        xs = [None] * (self.n_iters + 1)
        for j in range(self.slot_next):
            if 0 <= self.store_iters[j] <= self.n_iters:
                xs[self.store_iters[j]] = self.slab[j, :self.n].copy()
        xs[-1] = self.x.copy()
        return xs


def solve(ref, A, lam, Ax0, M=None, limit=10000):
    """A whole solve on the CPU: ``A`` is the UNDAMPED operator on numpy vectors, ``M`` the external preconditioner."""
    ref.init(Ax0)
    if ref.mode == M_EXTERNAL:
        ref.init_external(M(ref.r))
    for _ in range(limit):
        if ref.done:
            break
        ref.iterate(A(ref.p), lam, M)
    assert ref.done
    return ref


# ---- case tables ---------------------------------------------------------------------------------------------------------
SEED_SALT = 0  # (part of every seed: the one to change should a table ever meet an undecidable fp32 scalar)


def seed_of(*key):
    return zlib.crc32(repr((SEED_SALT,) + key).encode()) & 0x7fffffff


def lengths(dtype):
    """(name, n, max_blocks, grid of k_init*, grid of K1-K3 / k_dot_ry): the smallest lengths that reach each branch.
    T1 = 256 W is one unrolled row, T = 512 W one K1-K3 tile."""
    W = width(dtype)
    T1, T = BLOCK * W, BLOCK * UNROLL * W
    rows = [("1", 1, 0, 1, 1), ("W-1", W - 1, 0, 1, 1), ("W", W, 0, 1, 1), ("W+1", W + 1, 0, 1, 1),
            ("T1-1", T1 - 1, 0, 1, 1), ("T1", T1, 0, 1, 1), ("T1+1", T1 + 1, 0, 1, 1),
            ("T-1", T - 1, 0, 2, 1), ("T", T, 0, 2, 1), ("T+1", T + 1, 0, 2, 1),
            ("3T+W+1", 3 * T + W + 1, 0, 7, 4), ("7T+2W+3,mb3", 7 * T + 2 * W + 3, 3, 3, 3),
            ("5T+1,mb1", 5 * T + 1, 1, 1, 1), ("257T+W+3", 257 * T + W + 3, 0, 515, 258)]
    seen, out = set(), []
    for row in rows:  # (fp64: W-1 == 1)
        if row[1] not in seen:
            seen.add(row[1])
            out.append(row)
    return out


def length_row(dtype, name):
    return next(row for row in lengths(dtype) if row[0] == name)


def make_inputs(dtype, n, key, operator="rand", warm=False):
    """The input family: diagonal operator ``rand*3 + 0.5``, ``b = randn``, diagonal ``minv = rand + 0.5``."""
    T = np.dtype(dtype).type
    g = np.random.default_rng(seed_of(key))
    d = (g.random(n) * 3 + 0.5).astype(T)
    b = g.standard_normal(n).astype(T)
    minv = (g.random(n) + 0.5).astype(T)
    x0 = (g.standard_normal(n) * 0.25).astype(T) if warm else np.zeros(n, T)
    if operator == "identity_int":      # converges exactly in one iteration; then pAp = 0
        d = np.ones(n, T)
        minv = np.ones(n, T)
        b = g.integers(-3, 4, n).astype(T)
        b[0] = 1
    elif operator == "indefinite":      # four distinct eigenvalues, three of them negative: a Krylov space of dimension
        d = np.full(n, 2.0, T)          # 4 whose tridiagonal matrix has the pivots (+, -, -, -): iterations 2, 3, 4
        d[[0, n // 2, n - 1]] = T(-40.0), T(-55.0), T(-70.0)
        minv = np.full(n, 0.5, T)
    elif operator == "negative":        # negative definite: pAp <= 0 in every iteration
        d = -d
    else:
        assert operator == "rand", operator
    return d, b, minv, x0


class OneIter:
    """One full iteration phase by phase; ``variant`` a: warm x0, snapshots [0, 1] in a padded slab, m_hist;
    b: x0 = 0, snapshot [1] only (store_x0 off), no m_hist."""

    def __init__(self, dtype, mode, lam, row, variant):
        self.dtype, self.mode, self.lam, self.row, self.variant = dtype, mode, lam, row, variant
        self.name, self.n, self.max_blocks, self.grid_init, self.grid_k = row
        W = width(dtype)
        up = (self.n + W - 1) // W * W
        if variant == "a":
            self.warm, self.store_iters, self.store_x0, self.martens, self.slab_stride = True, [0, 1], True, True, up + 4 * W
        else:
            self.warm, self.store_iters, self.store_x0, self.martens, self.slab_stride = False, [1], False, False, up
        self.max_iter, self.tol, self.atol = 5, 0.0, -1.0  # (tol 0: K3 always goes on to update p)
        self.id = f"{np.dtype(dtype).name}-{MODE_NAMES[mode]}-lam{lam}-n={self.name}-{variant}"

    def inputs(self):
        return make_inputs(self.dtype, self.n, ("one", self.name, self.mode, self.lam, self.variant), warm=self.warm)

    def ref(self, b, minv, x0):
        return Ref(self.dtype, self.mode, x0, b, minv if self.mode == M_DIAG else None, self.max_iter, self.tol,
                   self.atol, self.martens, self.store_iters, self.store_x0, self.slab_stride)


def one_iter_cases(dtypes=DTYPES):
    return [OneIter(dt, mode, lam, row, v) for dt in dtypes for mode in MODES for lam in (0.0, 0.3)
            for row in lengths(dt) for v in "ab"]


def run_one_iter_ref(case, dev=None):
    """The reference alone (CPU): one iteration with the host-side diagonal operator."""
    d, b, minv, x0 = case.inputs()
    ref = case.ref(b, minv, x0)
    ref.init(d * x0)
    if case.mode == M_EXTERNAL:
        ref.init_external(minv * ref.r)
    ref.iterate(d * ref.p, case.lam, (lambda r: minv * r))
    return ref


class Scenario:
    def __init__(self, name, reason, max_iter, tol=0.0, atol=-1.0, martens=False, store=(), operator="rand", warm=False,
                 pad=False, nan_at=None, n_iters=None, nonpos=None, lam=None, n_nonpos=None):
        self.name, self.reason, self.max_iter, self.tol, self.atol, self.martens = name, reason, max_iter, tol, atol, martens
        self.store, self.operator, self.warm, self.pad, self.nan_at = list(store), operator, warm, pad, nan_at
        self.n_iters, self.nonpos, self.lam, self.n_nonpos = n_iters, nonpos, lam, n_nonpos


# atol of "atol_dominates" is a multiple of sqrt(n): ||b|| of a standard normal b is about sqrt(n)
SCENARIOS = [
    Scenario("maxiter1", MAXITER, 1, n_iters=1),
    Scenario("maxiter7", MAXITER, 7, store=[0, 1, 2], warm=True, martens=True, n_iters=7),
    Scenario("tol", TOL, 60, tol=1e-3, store=[1, 4, 5, 99], pad=True),
    Scenario("atol_dominates", TOL, 60, tol=1e-6, atol=0.02, store=[0], warm=True),
    Scenario("martens", MARTENS, 60, martens=True, store=[1, 4, 5, 99]),
    Scenario("exact_then_zero_curvature", DIVERGED, 9, operator="identity_int", martens=True, store=[0, 1, 2], pad=True,
             n_iters=2, nonpos=[2], lam=0.0),
    Scenario("nan_body", DIVERGED, 9, nan_at=("body", 2), store=[1, 4, 5, 99], n_iters=2, nonpos=[2]),
    Scenario("nan_tail", DIVERGED, 9, nan_at=("tail", 3), martens=True, n_iters=3, nonpos=[3]),
    Scenario("indefinite", MAXITER, 4, operator="indefinite", store=[0, 1, 2], n_iters=4, nonpos=[2, 3, 4], n_nonpos=3),
    Scenario("negative40", MAXITER, 40, operator="negative", n_iters=40, nonpos=list(range(1, 41))),
]
TRAJ_LENGTHS = ("T+1", "7T+2W+3,mb3", "3T+W+1")


class Traj:
    def __init__(self, dtype, mode, length, sc, index):
        self.dtype, self.mode, self.sc = dtype, mode, sc
        self.row = length_row(dtype, length)
        self.name, self.n, self.max_blocks, self.grid_init, self.grid_k = self.row
        self.nt = index % 2                       # streaming on for half of the runs
        self.lam = sc.lam if sc.lam is not None else (0.3 if (index // 2) % 2 else 0.0)
        W = width(dtype)
        up = (self.n + W - 1) // W * W
        self.slab_stride = up + 4 * W if sc.pad else up
        self.store_iters = sc.store
        self.store_x0 = bool(sc.store) and sc.store[0] == 0
        self.id = f"{sc.name}-{np.dtype(dtype).name}-{MODE_NAMES[mode]}-n={self.name}-nt{self.nt}-lam{self.lam}"

    def inputs(self):
        d, b, minv, x0 = make_inputs(self.dtype, self.n, ("traj", self.sc.name, self.name, self.mode), self.sc.operator,
                                     self.sc.warm)
        return d, b, minv, x0

    @property
    def atol(self):
        return self.sc.atol * math.sqrt(self.n) if self.sc.atol >= 0 else -1.0

    def ref(self, b, minv, x0):
        return Ref(self.dtype, self.mode, x0, b, minv if self.mode == M_DIAG else None, self.sc.max_iter, self.sc.tol,
                   self.atol, self.sc.martens, self.store_iters, self.store_x0, self.slab_stride)

    def Bp(self, d, p, it):
        """The host-side curvature product of iteration ``it``, with the scenario's NaN put in."""
        with np.errstate(all="ignore"):
            bp = d * p
        if self.sc.nan_at is not None and it == self.sc.nan_at[1]:
            W = width(self.dtype)
            assert self.n % W != 0
            bp[5 if self.sc.nan_at[0] == "body" else self.n - 1] = NAN
        return bp


def traj_cases(dtypes=DTYPES):
    out = []
    for sc in SCENARIOS:
        for dt in dtypes:
            for mode in MODES:
                for length in TRAJ_LENGTHS:
                    out.append(Traj(dt, mode, length, sc, len(out)))
    return out


def run_traj_ref(case):
    d, b, minv, x0 = case.inputs()
    ref = case.ref(b, minv, x0)
    ref.init(d * x0)
    if case.mode == M_EXTERNAL:
        ref.init_external(minv * ref.r)
    while not ref.done:
        bp = case.Bp(d, ref.p, ref.iter_next)
        ref.iterate(bp, case.lam, (lambda r: minv * r))
    return ref


# the 40 instantiations of the seven kernels (k_init_finalize has no mode, k_dot_ry / k_init_external only EXTERNAL)
def instantiations_of(dtype, mode, nt12, nt3):
    dn = np.dtype(dtype).name
    out = {("k_init", dn, mode), ("k_init_finalize", dn), ("k_curvature", dn, nt12), ("k_update_xr", dn, mode, nt12),
           ("k_update_p", dn, mode, nt3)}
    if mode == M_EXTERNAL:
        out |= {("k_init_external", dn), ("k_dot_ry", dn)}
    return out


N_INSTANTIATIONS = 2 * 3 + 2 + 2 + 2 * 2 + 2 * 3 * 2 + 2 + 2 * 3 * 2  # = 40
