"""The accumulated engine session behind ``HessianFree.acc_step()`` (``optimizer_acc``): loss, gradient and every
curvature product over lists of data chunks as graph replays over fused curvature engines -- the counterpart of
``session.EngineSession`` for ``step()``."""

import os

import torch

from . import _lib
from .engine import FusedGGNEngine, loss_spec_of
from .session import _loss_decline, _NoEngine, _Session


class AccumulatedSession(_Session):
    """``HessianFree.acc_step()`` on the fused engine (reference optimizer.py:519-606, :608-684, :767-814): loss,
    gradient and every curvature product accumulated over lists of data chunks, without building a forward
    graph per chunk and product as the reference does (it says so itself, optimizer.py:537-540).

    One fused curvature engine per DISTINCT chunk of the three data lists (chunks that the lists share -- the
    default: one list for everything -- share their engine), every buffer static, and FOUR hipGraphs for the
    whole lists, kept across ``acc_step`` calls while the lists keep their shapes:

        G_wT    the (I, H, W, O) weight copies of every engine                              (per step)
        G_fwd   forward pass + loss of every chunk of the LOSS list (and of the chunks whose activations the
                gradient / curvature lists need), loss = sum_k N_k loss_k / sum_k N_k        (per step, per trial point)
        G_grad  one adjoint sweep per chunk of the GRADIENT list, summed                   (per step)
        G_prod  one product per chunk of the CURVATURE list, each already weighted N_k / sum N (mean) or 1
                (sum), summed by one gather launch -- cloned into ``cg()``'s one-launch-per-iteration graph

    The chunks' sweeps are independent until the final sum: they are captured on parallel branches of the
    graph (fork / join by events during capture), so that two latency-bound sweeps of half the batch overlap
    instead of queueing (measured: 1 288 matvecs/s against 855 one after the other; train-mode BatchNorm always runs the
    chunks in sequence -- they all move the same running statistics).  Everything is the package's own
    deterministic kernels: two ``acc_step`` calls on the same data are bitwise equal.

    Under data parallelism (``process_group``) every rank holds ITS lists; the counts are totals over all ranks
    and the summed product / gradient / losses are all-reduced once more (compact layout of the engine)."""

    @property
    def mode(self):
        if len(self.engines) == 1 and self.merged:
            return ("accumulated engine session: the chunks carry one per-sample weight and the model does not couple "
                    "samples, so they run as ONE batch on one fused curvature engine (" + FusedGGNEngine.mode + "); engine, "
                    "graphs and PCG iteration graph kept across acc_step calls")
        return ("accumulated engine session: one fused curvature engine per data chunk"
                + (" (chunks of equal per-sample weight merged)" if self.merged else "")
                + (" on parallel graph branches" if self.parallel else ", in sequence")
                + ", weighted sum by one gather launch; engine, graphs and PCG iteration graph kept across acc_step calls")

    # ------------------------------------------------------------------------------------
    @classmethod
    def try_create(cls, model, loss_func, lists, params, reduction, counts, hessian=False, group=None, why=None):
        """``lists = (loss_datalist, grad_datalist, mvp_datalist)`` on the device; ``counts`` their total sample
        counts (over all ranks).  ``None`` when the engine does not cover the model / loss (``why``, a list, then
        receives the reason)."""
        why = [] if why is None else why
        if os.environ.get("HF_ACC_SESSION", "1") == "0":
            why.append("the accumulated session is switched off (HF_ACC_SESSION=0)")
            return None
        if not torch.cuda.is_available():
            why.append("no GPU")
            return None
        if not getattr(model, "_hf_engine_hooks", False):
            why.append("the model is not a prepared one (modelprep.prepare_model(model, channels_last=True) installs "
                       "the layers the fused engine reads)")
            return None
        sess = cls.__new__(cls)
        sess._why = why
        try:
            sess._build(model, loss_func, lists, list(params), reduction, counts, hessian, group)
        except _NoEngine as exc:
            if not why:
                why.append(exc.reason)
            return None
        return sess

    @staticmethod
    def _plan(lists):
        """Distinct chunks (by identity of their tensors) and the slots each list uses."""
        slots, index, roles = [], {}, []
        for dl in lists:
            idx = []
            for inputs, targets in dl:
                key = (id(inputs), id(targets))
                if key not in index:
                    index[key] = len(slots)
                    slots.append((inputs, targets))
                idx.append(index[key])
            roles.append(tuple(idx))
        return slots, roles

    @staticmethod
    def _merge_groups(model, slots, roles):
        """Which distinct chunks may run as ONE batch on ONE engine.  The accumulated quantities are
        ``sum_k w_k q_k`` with ``q_k`` a mean / sum over the samples of chunk k (optimizer.py:677-684): chunks that
        appear in the same lists the same number of times carry the same weight PER SAMPLE (``1 / sum N`` resp. 1), so
        for a model that does not couple the samples of a batch their concatenation IS the accumulation -- the
        reference's own test states it (tests/test_optimizer_acc.py:116-175: [7, 8] chunks == one batch of 15).  Not
        merged: a model with a train-mode BatchNorm or an active dropout layer (per-chunk statistics / masks are part
        of the reference's result), chunks that differ in more than the batch size.  What the loss function adds per
        CALL rather than per sample -- a tagged quadratic regulariser -- is not the concatenation's: the reference adds
        it once per chunk occurrence, which under ``mean`` comes to the merged engine's one term (the weights sum to the
        group's) and under ``sum`` to as many terms as the group has chunks; ``_build`` gives a merged engine's
        quadratic term that factor.  Returns lists of slot indices, in order of first appearance."""
        coupled = any((isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training)
                      or (isinstance(m, torch.nn.modules.dropout._DropoutNd) and m.training and m.p > 0)
                      for m in model.modules())
        groups, index = [], {}
        for k, (x, t) in enumerate(slots):
            key = (tuple(sum(1 for j in r if j == k) for r in roles), tuple(x.shape[1:]), x.dtype, tuple(t.shape[1:]),
                   t.dtype) if not coupled else k
            if key not in index:
                index[key] = len(groups)
                groups.append([])
            groups[index[key]].append(k)
        return groups

    def _merged(self, slots):
        """The data of the engines: per group of chunks their concatenation (a group of one: the chunk itself)."""
        return [slots[g[0]] if len(g) == 1 else
                (torch.cat([slots[k][0] for k in g]), torch.cat([slots[k][1] for k in g])) for g in self.groups]

    def _build(self, model, loss_func, lists, params, reduction, counts, hessian, group):
        slots, roles = self._plan(lists)
        if not slots or any(len(r) == 0 for r in roles):
            raise _NoEngine("an empty data list")
        self.model, self.loss_func, self.reduction, self.hessian = model, loss_func, reduction, bool(hessian)
        self.chunk_roles, self.chunk_shapes = roles, [tuple(x.shape) for x, _ in slots]
        for x, t in slots:
            if not (isinstance(x, torch.Tensor) and isinstance(t, torch.Tensor) and x.dim() >= 1 and t.dim() in (1, 2)
                    and t.shape[0] == x.shape[0]):
                raise _NoEngine("a data chunk is not (float32 inputs, class-index or [batch, outputs] targets)")
        # chunks that carry the same per-sample weight in every list run as ONE batch on ONE engine (round 6: the
        # default call -- one list for loss, gradient and curvature -- is then a single engine on the whole batch:
        # 1 450+ instead of 1 280 matvecs/s for chunks [16, 16], no graph branches)
        self.groups = self._merge_groups(model, slots, roles)
        self.merged = any(len(g) > 1 for g in self.groups)
        roles = [tuple(gi for gi, g in enumerate(self.groups) for _ in range(sum(1 for j in r if j == g[0])))
                 for r in roles]
        slots = self._merged(slots)
        self.roles, self.counts = roles, tuple(float(c) for c in counts)
        self.shapes = [tuple(x.shape) for x, _ in slots]
        self.group, self.params = group, params
        cur = self._enter_capture()
        engines = []
        with torch.cuda.stream(self.stream), torch.no_grad():
            for x, t in slots:
                if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and t.dim() in (1, 2)):
                    cur.wait_stream(self.stream)
                    raise _NoEngine("a data chunk is not (float32 inputs, class-index or [batch, outputs] targets)")
                with torch.enable_grad():
                    out = model(x)
                    loss = loss_func(out, t)
                    spec = loss_spec_of(loss, out) if isinstance(out, torch.Tensor) and out.dim() == 2 else None
                    eng = None
                    if spec is None:
                        self._why.append(_loss_decline(loss, out))
                    elif spec["reduction"] != reduction:
                        self._why.append(f"the loss function reduces by '{spec['reduction']}', acc_step was asked for "
                                         f"reduction='{reduction}'")
                    else:
                        # (group=None: the ranks' sum is taken once, after the chunks' sum)
                        eng = FusedGGNEngine.try_build(loss, out, params, weight=1.0, group=None, hessian=hessian,
                                                       why=self._why, need_session=True, for_acc=True)
                if eng is None or eng.loss_spec is None:
                    cur.wait_stream(self.stream)
                    raise _NoEngine("the fused engine does not cover this model / loss")
                engines.append(eng)
                del out, loss
            # What is per CHUNK rather than per sample does not merge by concatenation: a tagged quadratic term
            # (testproblems.l2_regularized) is part of the user's loss function, which the reference calls once per chunk
            # occurrence (optimizer.py:641, :678-684: ``result += eval_mb``).  Under ``mean`` the occurrences' weights sum to
            # the merged engine's; under ``sum`` every occurrence weighs 1, so an engine that stands for a group of m
            # chunks carries the term m times -- in its loss head, its gradient and its Hessian product, which all read
            # ``_l2`` (the engine's weight per list then counts how often the GROUP is listed).
            if reduction == "sum":
                for eng, g in zip(engines, self.groups):
                    if len(g) > 1 and eng._l2 is not None:
                        eng._l2 = eng._l2 * float(len(g))
            self.engines = engines
            self._layers = [e.layer_signature() for e in engines]
            # (the compact all-reduce layout -- which kernel taps can meet data -- is engine[0]'s: it depends on the
            # chunks' spatial shape, so all chunks must share everything but the batch size)
            if any(tuple(sh[1:]) != tuple(self.shapes[0][1:]) for sh in self.shapes):
                cur.wait_stream(self.stream)
                raise _NoEngine("the data chunks differ in more than their batch size: "
                                + ", ".join(str(sh) for sh in self.shapes))
            e0 = engines[0]
            self.op = self.engine = e0
            self.dev = e0.dev
            self.train_bn = any(e.train_bn for e in engines)
            self.parallel = len(engines) > 1 and not self.train_bn
            if self.parallel:  # (one level of graph branches: the chunks'; no fork inside a forked branch)
                for e in engines:
                    e._extras_allowed = False
            f32 = dict(dtype=torch.float32, device=self.dev)
            k_all = len(engines)
            self._allocate(e0.n, torch.float32, self.dev)
            self._parts = torch.empty((k_all, self.n), **f32)   # per-chunk partial products / gradients
            self._loss_ks = list(dict.fromkeys(roles[0]))  # (trial points: only these engines run)
            self._lossvec = torch.zeros(len(self._loss_ks), **f32)
            w = torch.zeros(len(self._loss_ks), **f32)
            for k in roles[0]:
                w[self._loss_ks.index(k)] += float(self.shapes[k][0]) if reduction == "mean" else 1.0
            self._loss_w = w
            self.loss_buf = torch.zeros((), **f32)
            self._side = [torch.cuda.Stream() for _ in range(k_all - 1)] if self.parallel else []
            self._events = [torch.cuda.Event() for _ in range(2 * k_all)]
            # which engines each graph touches
            grad_set = list(dict.fromkeys(roles[1]))
            if hessian:  # (a Hessian engine's products read the first-order cotangents its gradient sweep keeps)
                grad_set += [k for k in dict.fromkeys(roles[2]) if k not in grad_set]
            self._grad_set, self._mvp_set = grad_set, list(dict.fromkeys(roles[2]))
            self._fwd_set = list(range(k_all))

            def role_weights(role):  # (a chunk listed twice in one list counts twice)
                out = {}
                for k in roles[role]:
                    wk = float(self.shapes[k][0]) / self.counts[role] if reduction == "mean" else 1.0
                    out[k] = out.get(k, 0.0) + wk
                return out

            self._w_grad, self._w_mvp = role_weights(1), role_weights(2)
            # warm-up of everything that will be captured
            self._refresh()
            self._forward(self._fwd_set, update_running=False)
            self._gradient()
            self._product()
        self.stream.synchronize()
        with torch.no_grad():
            self.g_wT = self._capture(self._refresh)
            # every engine (a step's linearisation point) / the loss list's engines only (trial points)
            self.g_fwd_all = self._capture(lambda: self._forward(self._fwd_set, update_running=True))
            self.g_fwd = (self.g_fwd_all if len(self._loss_ks) == k_all
                          else self._capture(lambda: self._forward(self._loss_ks, update_running=True)))
            self.g_fwd_still = (self._capture(lambda: self._forward(self._fwd_set, update_running=False))
                                if self.train_bn else self.g_fwd_all)
            self.g_grad = self._capture(self._gradient)
            self.graph = self._capture(self._product, keep=True)
        cur.wait_stream(self.stream)
        torch.cuda.synchronize()
        self.steps = 0
        self.base_loss = None
        self._fresh = True  # (the model's own forward passes of the creating step have moved the running statistics)

    # ---- the four bodies ---------------------------------------------------------------------
    def _fork_join(self, ks, fn):
        """``fn(k)`` for every engine index of ``ks``: on parallel branches (the current stream + side streams,
        forked and joined by events -- inside a capture these become the graph's branches) or in sequence."""
        ks = list(ks)
        if not self.parallel or len(ks) < 2:
            for k in ks:
                fn(k)
            return
        cur = torch.cuda.current_stream()
        fork = self._events[0]
        fork.record(cur)
        for j, k in enumerate(ks[1:]):
            st = self._side[j]
            st.wait_event(fork)
            with torch.cuda.stream(st):
                fn(k)
                self._events[1 + j].record(st)
        fn(ks[0])
        for j in range(len(ks) - 1):
            cur.wait_event(self._events[1 + j])

    def _refresh(self):
        self._fork_join(self._fwd_set, lambda k: self.engines[k].refresh_weights(transposed=True))

    def _forward(self, ks, update_running=True):
        self._fork_join(ks, lambda k: self.engines[k].forward_own(refresh=True, update_running=update_running))
        torch.stack([self.engines[k].loss_buf for k in self._loss_ks], out=self._lossvec)
        val = torch.dot(self._lossvec, self._loss_w)
        if self.reduction == "mean":
            val = val / self.counts[0]
        self.loss_buf.copy_(val)

    def _sum_parts(self, ks, out):
        """``out = sum of the leading rows of the parts``: one gather launch (fixed order: repeatable)."""
        _lib.pack_ex(out, [self._parts[0]], {}, {0: (len(list(ks)), self.n)}, scale=1.0)

    def _gradient(self):
        order = self._grad_set  # (gradient-list chunks first: their parts are the leading rows)

        def one(j):
            eng = self.engines[order[j]]
            eng.weight = self._w_grad.get(order[j], 1.0)
            eng.gradient(self._parts[j])

        n_sum = len(dict.fromkeys(self.roles[1]))
        if n_sum == 1:  # (one chunk: straight into the result)
            eng = self.engines[order[0]]
            eng.weight = self._w_grad.get(order[0], 1.0)
            eng.gradient(self.grad_buffer)
            for j in range(1, len(order)):
                one(j)
            return
        self._fork_join(range(len(order)), one)
        self._sum_parts(range(n_sum), self.grad_buffer)

    def _product(self):
        order = self._mvp_set

        def one(j):
            eng = self.engines[order[j]]
            eng.weight = self._w_mvp[order[j]]
            eng.local(self.input_buffer, out=self._parts[j])

        if len(order) == 1:
            eng = self.engines[order[0]]
            eng.weight = self._w_mvp[order[0]]
            eng.local(self.input_buffer, out=self.output_buffer)
            return
        self._fork_join(range(len(order)), one)
        self._sum_parts(range(len(order)), self.output_buffer)

    # ---- validity ------------------------------------------------------------------------------
    def accepts(self, model, loss_func, lists, params, reduction, counts, hessian, group):
        slots, roles = self._plan(lists)
        if (model is not self.model or loss_func is not self.loss_func or reduction != self.reduction
                or bool(hessian) != self.hessian or group is not self.group or roles != self.chunk_roles
                or tuple(float(c) for c in counts) != self.counts):
            return None
        # (what the captured graphs bake in about the layers -- module identities, every BatchNorm's mode / eps /
        # momentum, the model's mode where it matters -- as EngineSession compares it; not model.training itself: an
        # eval() model with one train-mode BatchNorm is a train_bn session)
        if any(eng.layer_signature() != sig for eng, sig in zip(self.engines, self._layers)):
            return None
        if [tuple(x.shape) for x, _ in slots] != self.chunk_shapes:
            return None
        if self._merge_groups(model, slots, roles) != self.groups:
            return None  # (a dropout / BatchNorm layer changed mode: the chunks must no longer / may now be merged)
        if len(params) != len(self.params) or any(a is not b for a, b in zip(params, self.params)):
            return None
        e0 = self.engines[0]
        if e0._flat_params is None or e0._flat_params.data_ptr() != e0.params[0].data_ptr():
            return None
        for x, t in slots:
            if not x.is_cuda or x.dtype != torch.float32 or t.dim() not in (1, 2) or t.shape[0] != x.shape[0]:
                return None
        return slots

    # ---- per step ----------------------------------------------------------------------------
    def begin_step(self, slots, verify=False, reduce=True):
        """New data + current parameters into every engine; returns the accumulated loss (``reduce``: summed over
        the ranks here; else the caller does it -- after the ranks have agreed to use the session at all)."""
        with torch.no_grad():
            for (x, t), eng in zip(self._merged(slots), self.engines):
                eng.set_batch(x.detach(), t)
            self.g_wT.replay()
            (self.g_fwd_still if self._fresh else self.g_fwd_all).replay()
            self._fresh = False
            bad = torch.stack([eng.bad_targets.float().reshape(()) for eng in self.engines]).sum()
            vals = torch.stack([self.loss_buf.float().reshape(()), bad]).tolist()
        if vals[1]:
            raise _NoEngine("a target is outside the classes")
        if verify:
            self._verify(slots)
        self.steps += 1
        self._first_order_fresh = False
        self.base_loss = self.reduce_losses(self.loss_buf.reshape(1)).tolist()[0] if reduce else vals[0]
        return self.base_loss

    def _verify(self, slots):
        """The captured graphs still describe the model: its STOCK forward pass on the first chunk against the
        engine's logits (1e-4); raises ``_NoEngine`` otherwise."""
        x, _ = slots[0]
        with torch.no_grad():
            want = self.model._hf_stock_model_forward(x)
        got = self.engines[0].logits[: want.shape[0]]  # (chunk 0 leads the first engine's batch)
        err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
        if not err < 1e-4:
            raise _NoEngine(f"the captured graphs no longer reproduce the model's own forward pass (logits differ by "
                            f"{err:.1e})")

    def reduce_losses(self, vals):
        """Sum over ranks of (already count-weighted) loss values, as float64."""
        vals = vals.double()
        if self.group is not None:
            torch.distributed.all_reduce(vals, group=self.group)
        return vals

    def gradient(self):
        self.g_grad.replay()
        self._first_order_fresh = True
        if self.group is not None:
            self.engine.reduce(self.grad_buffer, self.group)
        return self.grad_buffer
