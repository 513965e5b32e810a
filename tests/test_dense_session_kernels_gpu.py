"""GPU: the two kernels of the dense-stack session (``hf_dense_act_forward``, ``hf_dense_loss_head`` of ``hf_dense.hip``)
through the C ABI -- no engine, no ``modelprep``.

Exact where the header promises it: the slab sum, the bias, identity and relu against the numpy reference of
``dense_session_refs``; ``dl`` / ``dl_ps`` against ``(p - onehot) * scale`` / ``(out - t) * scale`` evaluated by torch; two
calls on the same operands.  Where a transcendental function or a long sum is in the way, the project's rule: the
distance to float64 is at most 3 x the distance other fp32 evaluations of the same quantity keep from float64 (``torch``
in fp32 on the GPU; for tanh also numpy's float32 ``tanh``), measured here, nothing taken from the kernel; every such
comparison asserts that the reference distance is not zero.  A case is a handful of operand draws (the slab / bias
variants of the forward pass, DRAWS seeds of the loss head).  Loss values, and ``p`` / ``dl`` of at most POOL_BELOW numbers,
are compared as one vector over the draws: one draw of a 1 x 1 or 1 x 2 problem, or of a loss value of any shape, is a
single number that an fp32 evaluation rounds correctly as often as not; larger ``p`` / ``dl`` are held to the bound of
their own draw (with two draws of the 256 x 4097 ``mean`` MSE, torch's values sat 0.5 u from float64 and the kernel's 1.5 u -- the
three roundings its stated order has: the sum, ``coef``, their product).

Operands sit in NaN-filled buffers 4 bytes off the 16-byte grid, outputs in NaN-filled buffers with guard words."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from tol import within

import dense_session_refs as sr
from guarded import DEV, ERR_ARG, F32, NAN, FlatOut, P, st
from pytorchhessianfree_amd import _lib

pytestmark = pytest.mark.gpu
DRAWS = 8
POOL_BELOW = 64  # results of at most this many numbers are pooled over the draws (see above); larger ones: per draw


def put(arr, off=1):
    """``arr`` inside a NaN-filled buffer (int64: a zero-filled one), ``off`` elements behind its start."""
    t = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.full((t.numel() + off + 8,), NAN, device=DEV) if t.dtype.is_floating_point else \
        torch.zeros(t.numel() + off + 8, dtype=t.dtype, device=DEV)
    buf[off:off + t.numel()].copy_(t)
    return buf, P(buf.data_ptr() + buf.element_size() * off)


def dist(a, b):
    """max-norm distance relative to max |b| (b: float64)."""
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- hf_dense_act_forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("rows", [1, 3, 64, 256])
def test_act_forward_is_exact_and_tanh_is_within_three_times_other_fp32_tanh_of_float64(rows, c):
    lib = _lib.load()
    got_t, torch_t, numpy_t, want_t = [], [], [], []
    for splits in (1, 2, 5, 32):
        for with_b in (True, False):
            g = np.random.default_rng(7 * splits + int(with_b) + 100 * rows + c)
            slabs = g.standard_normal((splits, rows, c)).astype(np.float32)
            b = g.standard_normal(c).astype(np.float32) if with_b else None
            stride = rows * c + (9 if splits > 1 else 0)  # (> rows * c: the gaps between the slabs are NaN)
            padded = np.full((splits, stride), np.nan, np.float32)
            padded[:, :rows * c] = slabs.reshape(splits, -1)
            s_buf, s_ptr = put(padded)
            b_buf, b_ptr = put(b) if with_b else (None, None)
            outs = {}
            for act in (sr.IDENTITY, sr.RELU, sr.TANH):
                y, y2 = FlatOut(rows * c, 1), FlatOut(rows * c, 1)
                for o in (y, y2):
                    rc = lib.hf_dense_act_forward(o.ptr, s_ptr, splits, stride, b_ptr, act, rows, c, F32, st())
                    assert rc == 0, rc
                torch.cuda.synchronize()
                assert torch.equal(bits(y.buf), bits(y2.buf)), "two launches on the same inputs differ"
                assert y.untouched(), "a guard word was written"
                outs[act] = y.val.clone()
            pre = sr.act_forward(slabs, b, sr.IDENTITY)
            note = (rows, c, splits, with_b)
            assert np.array_equal(outs[sr.IDENTITY].cpu().numpy().reshape(rows, c), pre), note
            assert np.array_equal(outs[sr.RELU].cpu().numpy().reshape(rows, c), sr.act_forward(slabs, b, sr.RELU)), note
            assert not bool(torch.signbit(outs[sr.RELU]).any()), note
            # tanh of the kernel's exact pre-activation: float64, torch on the GPU, numpy in float32
            got_t.append(outs[sr.TANH].cpu().double())
            torch_t.append(torch.tanh(outs[sr.IDENTITY]).cpu().double())
            numpy_t.append(torch.from_numpy(np.tanh(pre).reshape(-1)).double())
            want_t.append(torch.from_numpy(np.tanh(pre.astype(np.float64)).reshape(-1)))
    want = torch.cat(want_t)
    d_ref = max(dist(torch.cat(torch_t), want), dist(torch.cat(numpy_t), want))
    d_got = dist(torch.cat(got_t), want)
    print(f"act_forward tanh {rows}x{c}: kernel {d_got:.3e}  other fp32 {d_ref:.3e}")
    assert d_ref > 0.0
    within(d_got, 3.0 * d_ref, strict=False, note=(rows, c))


def test_act_forward_relu_keeps_a_nan_and_turns_minus_zero_into_plus_zero():
    """A NaN pre-activation stays a NaN (as ``torch.relu``: a trial point with a NaN hidden layer must not report a finite
    loss); ``-0`` becomes ``+0``."""
    pre = np.array([[NAN, -0.0, 0.0, -1.5, 2.5]], np.float32)
    s_buf, s_ptr = put(pre)
    y = FlatOut(5, 1)
    assert _lib.load().hf_dense_act_forward(y.ptr, s_ptr, 1, 0, None, sr.RELU, 1, 5, F32, st()) == 0
    torch.cuda.synchronize()
    want = torch.relu(torch.from_numpy(pre).to(DEV)).reshape(-1)
    assert bool(torch.isnan(y.val[0])) and torch.equal(bits(y.val[1:]), bits(want[1:])) and y.untouched()
    assert np.isnan(sr.act_forward(pre[None], None, sr.RELU)[0, 0])


# ---- hf_dense_loss_head, cross-entropy ---------------------------------------------------------------------------------
def _ce_call(x, t, reduction, ps=True, off=1):
    """One call on fp32 logits / int64 targets (numpy).  Returns the outputs ``(p, dl, dl_ps, loss, flag)``."""
    lib = _lib.load()
    rows, c = x.shape
    sg, sps, coef = sr.loss_scales(sr.CE, rows, c, reduction)
    xb, xp = put(x, off)
    tb, tp = put(t, off)
    work = torch.full((512,), NAN, dtype=torch.float64, device=DEV)
    outs = [FlatOut(rows * c, off), FlatOut(rows * c, off), FlatOut(rows * c, off) if ps else None, FlatOut(1, 1),
            FlatOut(1, 1, dtype=torch.int32)]
    rc = lib.hf_dense_loss_head(sr.CE, xp, tp, *[None if o is None else o.ptr for o in outs], P(work.data_ptr()), sg, sps,
                                coef, rows, c, F32, st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(o is None or o.untouched() for o in outs), "a guard word was written"
    return outs


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("c", [2, 10, 100, 1000, 1024])
@pytest.mark.parametrize("rows", [1, 2, 65, 256])
def test_ce_head_against_float64_and_torch(rows, c, reduction):
    sg, sps, _ = sr.loss_scales(sr.CE, rows, c, reduction)
    draws = DRAWS
    got, ref, want = {k: [] for k in "pgl"}, {k: [] for k in "pgl"}, {k: [] for k in "pgl"}
    for seed in range(draws):
        x, t = sr.logits_case(rows, c, seed=seed)
        p, dl, dl_ps, loss, flag = _ce_call(x, t, reduction)
        again = _ce_call(x, t, reduction)
        for a, b in zip((p, dl, dl_ps, loss, flag), again):
            assert torch.equal(bits(a.buf), bits(b.buf)), "two calls on the same inputs differ"
        assert int(flag.val) == 0
        xg, tg = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        onehot = F.one_hot(tg, c).float()
        pv = p.val.view(rows, c)
        # dl, dl_ps: two roundings from the kernel's OWN p, as core._dlogits
        assert torch.equal(bits(dl.val.view(rows, c)), bits((pv - onehot) * sg))
        assert torch.equal(bits(dl_ps.val.view(rows, c)), bits((pv - onehot) * sps))
        x32 = xg.clone().requires_grad_(True)
        l32 = F.cross_entropy(x32, tg, reduction=reduction)
        (g32,) = torch.autograd.grad(l32, x32)
        x64 = xg.double().requires_grad_(True)
        l64 = F.cross_entropy(x64, tg, reduction=reduction)
        (g64,) = torch.autograd.grad(l64, x64)
        for k, a, r, w in (("p", pv, torch.softmax(xg, 1), torch.softmax(x64.detach(), 1)), ("g", dl.val, g32, g64),
                           ("l", loss.val, l32.detach(), l64.detach())):
            if k != "l" and rows * c > POOL_BELOW:  # a matrix with enough entries: held to its own draw's bound
                d_got, d_ref = dist(a, w), dist(r, w)
                assert d_ref > 0.0, (k, seed)
                within(d_got, 3.0 * d_ref, strict=False, note=(rows, c, reduction, k, seed))
                continue
            got[k].append(a.double().reshape(-1).cpu())
            ref[k].append(r.double().reshape(-1).cpu())
            want[k].append(w.reshape(-1).cpu())
        # without the per-sample output: the same bits elsewhere
        q = _ce_call(x, t, reduction, ps=False)
        assert torch.equal(bits(q[1].buf), bits(dl.buf)) and torch.equal(bits(q[3].buf), bits(loss.buf))
    for k, name in (("p", "p"), ("g", "dl"), ("l", "loss")):
        if not want[k]:
            continue
        w = torch.cat(want[k])
        d_got, d_ref = dist(torch.cat(got[k]), w), dist(torch.cat(ref[k]), w)
        print(f"ce {rows}x{c} {reduction} {name}: kernel {d_got:.3e}  torch fp32 {d_ref:.3e}")
        assert d_ref > 0.0, name
        within(d_got, 3.0 * d_ref, strict=False, note=(rows, c, reduction, name))


@pytest.mark.parametrize("bad", [-100, "c"])
def test_ce_head_flags_a_target_outside_the_classes(bad):
    """The flagged row has no one in its one-hot and adds nothing to the loss: the loss is the sum over the OTHER rows
    times ``coef`` -- against float64 by the 3 x rule, the other fp32 evaluation being ``F.cross_entropy`` of those rows
    in fp32 on the GPU (the losses of the draws as one vector)."""
    rows, c = 65, 10
    coef = 1.0 / rows
    got, ref, want = [], [], []
    for seed in range(DRAWS):
        x, t = sr.logits_case(rows, c, seed=seed)
        t = t.copy()
        t[33] = c if bad == "c" else bad
        p, dl, dl_ps, loss, flag = _ce_call(x, t, "mean")
        assert int(flag.val) != 0
        assert all(bool(torch.isfinite(o.val).all()) for o in (p, dl, dl_ps, loss))
        assert sr.ce_head(x, t, *sr.loss_scales(sr.CE, rows, c, "mean")[:2], "mean")[4] == 1
        assert torch.equal(bits(dl.val.view(rows, c)[33]), bits(p.val.view(rows, c)[33] * coef))  # no one
        keep = [r for r in range(rows) if r != 33]
        xk, tk = torch.from_numpy(x[keep]).to(DEV), torch.from_numpy(t[keep]).to(DEV)
        got.append(loss.val.double().cpu())
        ref.append((F.cross_entropy(xk, tk, reduction="sum") * coef).double().reshape(1).cpu())
        want.append((F.cross_entropy(xk.double(), tk, reduction="sum") * coef).reshape(1).cpu())
    w = torch.cat(want)
    d_got, d_ref = dist(torch.cat(got), w), dist(torch.cat(ref), w)
    print(f"ce bad target {bad}: kernel {d_got:.3e}  torch fp32 {d_ref:.3e}")
    assert d_ref > 0.0
    within(d_got, 3.0 * d_ref, strict=False, note=bad)


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_ce_head_on_logits_of_magnitude_1e4(reduction):
    rows, c = 65, 100
    got, ref, want = [], [], []
    for seed in range(2):
        x, t = sr.logits_case(rows, c, seed=seed, offset=1e4)
        p, dl, dl_ps, loss, flag = _ce_call(x, t, reduction)
        assert all(bool(torch.isfinite(o.val).all()) for o in (p, dl, dl_ps, loss)) and int(flag.val) == 0
        xg, tg = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        got.append(torch.cat([p.val.double().cpu(), loss.val.double().cpu()]))
        ref.append(torch.cat([torch.softmax(xg, 1).double().reshape(-1).cpu(),
                              F.cross_entropy(xg, tg, reduction=reduction).double().reshape(1).cpu()]))
        want.append(torch.cat([torch.softmax(xg.double(), 1).reshape(-1).cpu(),
                               F.cross_entropy(xg.double(), tg, reduction=reduction).reshape(1).cpu()]))
    # (p and the loss as one vector would let the loss's magnitude hide p: compared part by part)
    n = rows * c
    for name, sl in (("p", slice(0, n)), ("loss", slice(n, n + 1))):
        w = torch.cat([v[sl] for v in want])
        d_got, d_ref = dist(torch.cat([v[sl] for v in got]), w), dist(torch.cat([v[sl] for v in ref]), w)
        print(f"ce 1e4 {reduction} {name}: kernel {d_got:.3e}  torch fp32 {d_ref:.3e}")
        assert d_ref > 0.0, name
        within(d_got, 3.0 * d_ref, strict=False, note=(reduction, name))


# ---- hf_dense_loss_head, mean-squared error --------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("c", [1, 3, 100, 4097])
@pytest.mark.parametrize("rows", [1, 17, 256])
def test_mse_head_against_float64_and_torch(rows, c, reduction):
    lib = _lib.load()
    sg, sps, coef = sr.loss_scales(sr.MSE, rows, c, reduction)
    draws = DRAWS
    got, ref, want = [], [], []
    for seed in range(draws):
        x, t = sr.mse_case(rows, c, seed=seed)
        xb, xp = put(x)
        tb, tp = put(t)
        runs = []
        for _ in range(2):
            work = torch.full((512,), NAN, dtype=torch.float64, device=DEV)
            p = FlatOut(rows * c, 1)  # (not touched by this kind)
            dl, dl_ps = FlatOut(rows * c, 1), FlatOut(rows * c, 1)
            loss, flag = FlatOut(1, 1), FlatOut(1, 1, dtype=torch.int32)
            rc = lib.hf_dense_loss_head(sr.MSE, xp, tp, p.ptr, dl.ptr, dl_ps.ptr, loss.ptr, flag.ptr, P(work.data_ptr()),
                                        sg, sps, coef, rows, c, F32, st())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert p.pristine() and all(o.untouched() for o in (dl, dl_ps, loss, flag))
            runs.append((dl, dl_ps, loss, flag))
        for a, b in zip(*runs):
            assert torch.equal(bits(a.buf), bits(b.buf)), "two calls on the same inputs differ"
        dl, dl_ps, loss, flag = runs[0]
        xg, tg = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        assert int(flag.val) == 0
        assert torch.equal(bits(dl.val.view(rows, c)), bits((xg - tg) * sg))
        assert torch.equal(bits(dl_ps.val.view(rows, c)), bits((xg - tg) * sps))
        got.append(loss.val.double().cpu())
        ref.append(F.mse_loss(xg, tg, reduction=reduction).double().reshape(1).cpu())
        want.append(F.mse_loss(xg.double(), tg.double(), reduction=reduction).reshape(1).cpu())
    w = torch.cat(want)
    d_got, d_ref = dist(torch.cat(got), w), dist(torch.cat(ref), w)
    print(f"mse {rows}x{c} {reduction} loss: kernel {d_got:.3e}  torch fp32 {d_ref:.3e}")
    assert d_ref > 0.0
    within(d_got, 3.0 * d_ref, strict=False, note=(rows, c, reduction))


# ---- refusals: HF_ERR_ARG before any launch, the outputs stay as they were ---------------------------------------------
def test_session_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    work = torch.zeros(512, dtype=torch.float64, device=DEV)
    tg = torch.zeros(8, dtype=torch.int64, device=DEV)
    b, w, t, s = P(buf.data_ptr()), P(work.data_ptr()), P(tg.data_ptr()), st()
    AF, LH = lib.hf_dense_act_forward, lib.hf_dense_loss_head
    assert AF(None, b, 1, 0, b, 1, 4, 4, F32, s) == ERR_ARG        # no output
    assert AF(b, None, 1, 0, b, 1, 4, 4, F32, s) == ERR_ARG        # no slabs
    assert AF(b, b, 0, 0, b, 1, 4, 4, F32, s) == ERR_ARG and AF(b, b, 33, 16, b, 1, 4, 4, F32, s) == ERR_ARG
    assert AF(b, b, 2, 15, b, 1, 4, 4, F32, s) == ERR_ARG          # slabs would overlap
    assert AF(b, b, 1, 0, b, 3, 4, 4, F32, s) == ERR_ARG and AF(b, b, 1, 0, b, -1, 4, 4, F32, s) == ERR_ARG
    assert AF(b, b, 1, 0, b, 1, 0, 4, F32, s) == ERR_ARG and AF(b, b, 1, 0, b, 1, 257, 4, F32, s) == ERR_ARG
    assert AF(b, b, 1, 0, b, 1, 4, 0, F32, s) == ERR_ARG
    assert AF(b, b, 1, 0, b, 1, 4, 4, _lib.HF_F64, s) == ERR_ARG
    for kind in (sr.CE, sr.MSE):
        tt = t if kind == sr.CE else b
        ok = [kind, b, tt, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, F32, s]
        for i in (1, 2, 4, 6, 7, 8):  # logits, targets, dl, loss, flag, work
            args = list(ok)
            args[i] = None
            assert LH(*args) == ERR_ARG, (kind, i)
        for i in (9, 10, 11):         # a NaN scale
            args = list(ok)
            args[i] = NAN
            assert LH(*args) == ERR_ARG, (kind, i)
        for rows, c in ((0, 4), (257, 4), (1, 0), (1, (1 << 20) + 1)):
            args = list(ok)
            args[12], args[13] = rows, c
            assert LH(*args) == ERR_ARG, (kind, rows, c)
        args = list(ok)
        args[14] = _lib.HF_F64
        assert LH(*args) == ERR_ARG
        args = list(ok)
        args[8] = P(work.data_ptr() + 4)  # a workspace off the 8-byte grid
        assert LH(*args) == ERR_ARG
    assert LH(sr.CE, b, t, None, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, F32, s) == ERR_ARG      # cross-entropy without p
    assert LH(sr.CE, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 1025, F32, s) == ERR_ARG      # more than 1024 classes
    assert LH(2, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, F32, s) == ERR_ARG             # an unknown kind
    assert LH(-1, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, F32, s) == ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(work.abs().sum()) == 0.0  # nothing ran
