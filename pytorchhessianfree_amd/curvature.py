"""Curvature-vector products ``v -> B v`` on flat parameter vectors (the ``mvp`` of
the reference's ``optimizer.py:237-247, :450-462``) and their data-parallel sum.

The reference delegates to BackPACK, which re-derives everything on every call:
``R_op`` builds a double-backward graph through a dummy cotangent, runs it, and
``parameters_to_vector`` concatenates the result (optimizer.py:457-462).  Here

* the linear map ``u -> J^T u`` (``J = d outputs / d params``) is recorded ONCE per
  step as an autograd graph; ``J v`` is then one backward sweep through that
  recorded graph per matvec (MIOpen/rocBLAS kernels on PyTorch-ROCm -- this is
  not a dense contraction, so no custom MFMA kernel);
* the loss Hessian ``H_L`` is likewise recorded once (``d loss / d outputs`` with
  graph) and applied with one tiny backward sweep;
* ``J^T (H_L J v)`` is one ordinary reverse pass through the step's forward graph;
* the per-parameter results are gathered into ONE contiguous HBM vector by the
  multi-tensor ``hf_pack`` kernel (8 N bytes instead of ``torch.cat``), with the
  data-parallel weight ``N_k / sum N`` folded into the same pass;
* across ranks the partial products are summed with ONE all-reduce per matvec
  (the ``result += N * mb_result`` of optimizer.py:677-684 turned sideways).

On CPU tensors (host-logic tests, gloo tests) the gather is ``torch.cat``; on a
GPU the HIP kernel is mandatory (``_lib`` raises if the library is missing).
"""

import gc

import torch

from . import _lib
from .modelprep import consumed_at_once, first_order_only, tangent_owner
from .utils import vector_to_parameter_list


def flatten_into(tensors, like_params, out=None, scale=1.0):
    """``parameters_to_vector`` replacement: gather ``tensors`` (``None`` -> zeros
    shaped like the matching parameter) into one flat vector, times ``scale``."""
    ref = like_params[0]
    n = sum(p.numel() for p in like_params)
    if out is None:
        out = torch.empty(n, dtype=ref.dtype, device=ref.device)
    dense = [
        torch.zeros_like(p) if t is None else t.detach() for t, p in zip(tensors, like_params)
    ]
    if out.is_cuda:
        _lib.pack(out, dense, scale=scale, mode=0)
    else:
        torch.cat([t.reshape(-1) for t in dense], out=out)
        if scale != 1.0:
            out.mul_(scale)
    return out


def _all_reduce_sum(t, group):
    from .distributed import all_reduce_sum

    return all_reduce_sum(t, group)


class _Operator:
    """Common part: flat-vector in, flat-vector out, optional rank weight and
    process group.  ``group=None`` means single process (reference behaviour)."""

    def __init__(self, params, weight=1.0, group=None):
        self.params = list(params)
        self.weight = float(weight)
        self.group = group
        self.n = sum(p.numel() for p in self.params)
        self.calls = 0

    mode = "eager autograd"

    def _finish(self, per_param, out):
        return flatten_into(per_param, self.params, out=out, scale=self.weight)

    def local(self, v, out=None):
        """This rank's weighted partial product (no communication)."""
        raise NotImplementedError

    def reduce(self, t, group=None):
        """In-place sum of a local product over the ranks (``group`` defaults to the operator's
        own); operators that know more about the vector may move fewer bytes (the engine)."""
        return _all_reduce_sum(t, self.group if group is None else group)

    def __call__(self, v, out=None):
        self.calls += 1
        return self.reduce(self.local(v, out))


class GGNOperator(_Operator):
    """``v -> J^T H_L J v`` for the mini-batch behind ``(loss, outputs)``
    (math contract of BackPACK's ``ggn_vector_product_from_plist``,
    optimizer.py:457-462)."""

    def __init__(self, loss, outputs, params, weight=1.0, group=None):
        super().__init__(params, weight, group)
        self.outputs = outputs
        # u -> J^T u, recorded once (u is a dummy cotangent)
        self._u = torch.zeros_like(outputs, requires_grad=True)
        with first_order_only():  # only d/du of this map is ever taken
            JTu = torch.autograd.grad(
                outputs, self.params, grad_outputs=self._u, create_graph=True,
                retain_graph=True, allow_unused=True,
            )
        self._used = [i for i, g in enumerate(JTu) if g is not None]
        self._JTu = [JTu[i] for i in self._used]
        # d loss / d outputs with graph -> H_L by one more sweep
        (self._dl,) = torch.autograd.grad(loss, outputs, create_graph=True, retain_graph=True)
        self._ce = self._closed_form_loss_hessian(loss, outputs)

    def _closed_form_loss_hessian(self, loss, outputs):
        """``(p, scale)`` if the loss is a softmax cross-entropy of ``outputs`` whose
        Hessian ``scale * (diag(p) - p p^T)`` (per row) reproduces the autograd sweep
        through ``d loss / d outputs`` on a random vector, else ``None``.  The structural
        test only nominates; the numerical check decides (class weights, ignored targets,
        label smoothing etc. fail it and keep the generic sweep).  GPU tensors only."""
        fn = loss.grad_fn
        try:
            if not outputs.is_cuda or outputs.dim() != 2 or fn is None or fn.name() != "NllLossBackward0":
                return None
            lsm = fn.next_functions[0][0]
            if lsm is None or lsm.name() != "LogSoftmaxBackward0" or lsm._saved_dim not in (1, -1):
                return None
            if lsm.next_functions[0][0] is not outputs.grad_fn or not self._dl.requires_grad:
                return None
            scale = {1: 1.0 / outputs.shape[0], 2: 1.0}.get(fn._saved_reduction)
        except AttributeError:
            return None
        if scale is None:
            return None
        p = torch.softmax(outputs.detach(), dim=1)
        gen = torch.Generator(device=outputs.device).manual_seed(99)
        probe = torch.randn(outputs.shape, dtype=outputs.dtype, device=outputs.device, generator=gen)
        (want,) = torch.autograd.grad(self._dl, outputs, grad_outputs=probe, retain_graph=True)
        got = _lib.softmax_ce_hvp(p, probe, scale)
        if not float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()):
            return None
        return p, scale

    def _loss_hessian(self, Jv):
        if self._ce is not None:
            return _lib.softmax_ce_hvp(self._ce[0], Jv, self._ce[1])
        if not self._dl.requires_grad:  # loss linear in the outputs: H_L = 0
            return torch.zeros_like(Jv)
        (HJv,) = torch.autograd.grad(
            self._dl, self.outputs, grad_outputs=Jv, retain_graph=True, allow_unused=True
        )
        return torch.zeros_like(Jv) if HJv is None else HJv

    def local(self, v, out=None):
        vs = vector_to_parameter_list(v, self.params)
        with tangent_owner(self, v):  # conv layers' v_W operands: one scatter launch
            (Jv,) = torch.autograd.grad(
                self._JTu, self._u, grad_outputs=[vs[i] for i in self._used], retain_graph=True
            )
        HJv = self._loss_hessian(Jv)
        with consumed_at_once():  # gathered by hf_pack right below
            JTHJv = torch.autograd.grad(
                self.outputs, self.params, grad_outputs=HJv, retain_graph=True, allow_unused=True
            )
            return self._finish(JTHJv, out)

    # -- the same product in two phases, for overlapping the all-reduce with compute --
    def split_point(self, tail_fraction=0.75):
        """Index ``c`` such that ``params[c:]`` (the LAST layers, whose gradients the
        adjoint sweep produces FIRST) hold at most ``tail_fraction`` of the entries;
        returns ``(c, flat offset of params[c])``."""
        total, acc, c = self.n, 0, len(self.params)
        while c > 1 and acc + self.params[c - 1].numel() <= tail_fraction * total:
            c -= 1
            acc += self.params[c].numel()
        return c, total - acc

    def _H_J(self, v):
        vs = vector_to_parameter_list(v, self.params)
        with tangent_owner(self, v):
            (Jv,) = torch.autograd.grad(
                self._JTu, self._u, grad_outputs=[vs[i] for i in self._used], retain_graph=True
            )
        return self._loss_hessian(Jv)

    def phase_tail(self, v, out, cut, offset):
        """``out[offset:] = weight * (J^T H_L J v)[offset:]`` -- tangent sweep, loss
        Hessian, and the adjoint sweep only as far back as ``params[cut]``."""
        self._hjv = self._H_J(v)
        tail = self.params[cut:]
        with consumed_at_once():
            g = torch.autograd.grad(self.outputs, tail, grad_outputs=self._hjv, retain_graph=True,
                                    allow_unused=True)
            flatten_into(g, tail, out=out[offset:], scale=self.weight)

    def phase_head(self, out, cut, offset):
        """``out[:offset]``: the rest of the adjoint sweep (re-walks the tail's data
        gradients, which is cheap next to the all-reduce it hides)."""
        head = self.params[:cut]
        with consumed_at_once():
            g = torch.autograd.grad(self.outputs, head, grad_outputs=self._hjv, retain_graph=True,
                                    allow_unused=True)
            flatten_into(g, head, out=out[:offset], scale=self.weight)


def ggn_operator(loss, outputs, params, weight=1.0, group=None, why=None):
    """The GGN operator for ``(loss, outputs)``: the fused curvature engine (engine.py) when
    ``outputs`` comes from a prepared model of a family it knows (conv - eval-BatchNorm - ReLU
    units with residual connections, NHWC fp32), else the autograd operator above."""
    if isinstance(outputs, torch.Tensor) and getattr(outputs, "_hf_model", None) is not None:
        from .engine import FusedGGNEngine

        eng = FusedGGNEngine.try_build(loss, outputs, list(params), weight=weight, group=group, why=why)
        if eng is not None:
            return eng
    elif why is not None:
        why.append("the model is not a prepared one (modelprep.prepare_model(model, channels_last=True) installs the "
                   "layers the fused engine reads)")
    return GGNOperator(loss, outputs, params, weight=weight, group=group)


def hessian_operator(loss, outputs, params, grad_with_graph=None, weight=1.0, group=None, why=None):
    """The Hessian operator for ``loss``: the fused curvature engine in Hessian mode (engine.py:
    forward-over-reverse on the package's own kernels) when ``outputs`` comes from a prepared model of
    a family it covers (plain conv-ReLU stacks with a softmax cross-entropy, optionally plus a tagged
    L2 term), else the autograd operator below."""
    if isinstance(outputs, torch.Tensor) and getattr(outputs, "_hf_model", None) is not None:
        from .engine import FusedGGNEngine

        eng = FusedGGNEngine.try_build(loss, outputs, list(params), weight=weight, group=group, hessian=True,
                                       why=why)
        if eng is not None:
            return eng
    elif why is not None:
        why.append("the model is not a prepared one (modelprep.prepare_model(model, channels_last=True) installs the "
                   "layers the fused engine reads)")
    return HessianOperator(loss, params, grad_with_graph=grad_with_graph, weight=weight, group=group)


class HessianOperator(_Operator):
    """``v -> (d^2 loss / d params^2) v`` (BackPACK's ``hessian_vector_product``,
    optimizer.py:450-455).  ``grad_with_graph`` are the per-parameter gradients
    computed with ``create_graph=True`` (the step needs them anyway,
    optimizer.py:231-233); H is symmetric, so one reverse sweep through that
    graph with cotangent ``v`` is ``H v``."""

    def __init__(self, loss, params, grad_with_graph=None, weight=1.0, group=None):
        super().__init__(params, weight, group)
        if grad_with_graph is None:
            grad_with_graph = torch.autograd.grad(
                loss, self.params, create_graph=True, retain_graph=True
            )
        self._used = [i for i, g in enumerate(grad_with_graph) if g.requires_grad]
        self._g = [grad_with_graph[i] for i in self._used]

    def local(self, v, out=None):
        vs = vector_to_parameter_list(v, self.params)
        if self._g:
            Hv = torch.autograd.grad(
                self._g, self.params, grad_outputs=[vs[i] for i in self._used],
                retain_graph=True, allow_unused=True,
            )
        else:  # loss linear in the parameters
            Hv = [None] * len(self.params)
        return self._finish(Hv, out)


_capture_streams = {}  # one capture stream per device, shared by every captured operator


class CapturedOperator:
    """A curvature operator whose local product is captured once as hipGraph(s) and replayed per matvec.  The
    contract :func:`~pytorchhessianfree_amd.cg.cg` relies on, for every subclass:

    * ``input_buffer`` / ``output_buffer``: the captured product reads the one and writes the other.  ``cg()``
      adopts ``input_buffer`` as its search direction ``p`` (its update kernel writes the next direction straight
      into the graph's input: no copy); ``local`` / ``__call__`` copy any other input vector in first.  A returned
      ``output_buffer`` is overwritten by the next product.
    * ``replay_local()``: this rank's product, ``input_buffer -> output_buffer``.  ``reduce(t)``: the in-place sum
      of a local product over ``group`` (the wrapped engine's compact all-reduce when it has one).
      ``replay_and_reduce()``: one product summed over the ranks -- ``replay_local()`` then
      ``reduce(output_buffer)`` unless a subclass overlaps the two.
    * ``raw_graph``: ``None`` as a class attribute means ``cg()`` calls the operator in every iteration.  As a
      method it lets ``cg()`` fuse K1-K3 into one graph launch per iteration; the product joins that graph only
      when ``raw_graph()`` returns a handle (the single product graph, owned by the operator) and there is no
      group.  ``raw_graph()`` returning ``None`` means the product has no single graph: without a group ``cg()``
      then takes its unfused loop.  Under a group ``cg()`` calls ``replay_and_reduce()`` before every K1-K3 launch.
    * ``calls``: products taken, counted by ``cg()`` also for those it replays itself.  ``group``: the process
      group, ``None`` for a single process.  ``op``: the captured eager operator or engine.
    * ``compact``: ``None``, or an object with this same contract over the ``n_live`` entries of the vector that can
      be non-zero (:class:`CompactFacet`: its own ``input_buffer`` / ``output_buffer`` / product graph, products
      counted on this operator) plus ``n_live``, ``gather(full, out)``, ``scatter(compact, out)`` and
      ``dead_entries_zero(b, x0)``.  ``cg()`` runs its whole solve there when the dead entries of ``b`` and ``x0``
      are zero (they then stay zero in ``r``, ``p``, ``x``); ``compact_decline`` says why there is none.

    The data-parallel all-reduce stays outside the graphs.  Subclasses build on the device's capture stream
    (``_enter_capture``), allocate the two buffers with ``_allocate`` and capture with ``_capture``."""

    calls = 0
    group = None
    compact = None          # (the same product between compact vectors: CompactFacet)
    compact_decline = None  # (why not)
    _side = None            # (two-phase products: the probed side stream of distributed.two_phase_all_reduce ...)
    side_runs_beside = None  # (... and the probe's verdict)

    def _enter_capture(self):
        """Point ``self.stream`` at the device's capture stream, ordered after the current stream; returns the
        current stream (the caller makes it wait for the capture stream when done)."""
        cur = torch.cuda.current_stream()
        dev = torch.cuda.current_device()
        stream = _capture_streams.get(dev)
        if stream is None:
            stream = _capture_streams[dev] = torch.cuda.Stream()
        self.stream = stream
        stream.wait_stream(cur)
        return cur

    def _allocate(self, n, dtype, device):
        self.n = n
        self.input_buffer = torch.zeros(n, dtype=dtype, device=device)
        self.output_buffer = torch.zeros(n, dtype=dtype, device=device)

    def _capture(self, fn, keep=False, pool=None):
        """``fn`` captured on ``self.stream``.  ``keep``: the raw ``hipGraph_t`` stays available (``cg()`` clones
        it into its one-launch-per-iteration graph, product -> K1 -> K2 -> K3, hf_pcg_graph_*)."""
        g = torch.cuda.CUDAGraph(keep_graph=True) if keep else torch.cuda.CUDAGraph()
        # No cycle collection while the stream captures: a dead ``CUDAGraph`` that only the collector frees (an earlier
        # session's, held in a reference cycle) synchronises the device in its destructor, which a capture in progress
        # forbids -- the destructor throws and the process aborts.  ``torch.cuda.graph`` no longer collects on entry, so
        # which allocation inside ``fn`` starts a collection is a matter of the process's history.
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, stream=self.stream, pool=pool):
                fn()
        finally:
            if collecting:
                gc.enable()
        if keep:
            g.instantiate()
        return g

    def raw_graph(self):
        """The captured product as a raw ``hipGraph_t`` (an int), owned by ``self.graph``."""
        return self.graph.raw_cuda_graph()

    def replay_local(self):
        self.graph.replay()

    def reduce(self, t):
        inner = getattr(self.op, "reduce", None)  # (the captured operator's own rule, if it has one)
        if inner is not None:
            return inner(t, self.group)
        return _all_reduce_sum(t, self.group)

    @property
    def reduce_bytes(self):
        return getattr(self.op, "reduce_bytes", self.output_buffer.nbytes)

    def replay_and_reduce(self):
        self.replay_local()
        self.reduce(self.output_buffer)

    def _load(self, v):
        if v.data_ptr() != self.input_buffer.data_ptr():
            self.input_buffer.copy_(v)

    def _result(self, out):
        if out is not None:
            out.copy_(self.output_buffer)
            return out
        return self.output_buffer

    def local(self, v, out=None):
        """This rank's product of ``v`` (no communication)."""
        self._load(v)
        self.replay_local()
        return self._result(out)

    def __call__(self, v, out=None):
        self.calls += 1
        self._load(v)
        if self.group is None:
            self.replay_local()
        else:
            self.replay_and_reduce()
        return self._result(out)


class CompactFacet(CapturedOperator):
    """The product of a :class:`CapturedOperator` (``parent``) between vectors in the COMPACT layout -- the flat vector
    with the structurally-zero entries removed (``engine.compact_layout``; the order of ``hf_live_copy``).  A second
    product graph over the parent's engine: only the scatter that reads ``input_buffer`` and the gather that writes
    ``output_buffer`` differ from the parent's graph; every launch between them, and every buffer, is shared.

    ``cg()`` solves on a facet exactly as on any captured operator (adopts ``input_buffer`` as ``p``, fuses the
    product into its iteration graph); products are counted on the parent, and the iteration graphs are kept in the
    parent's ``_iteration_graphs``."""

    def __init__(self, parent, layout, capture):
        """``capture(fn, pool)``: the parent's capture on its stream; called inside the parent's build."""
        eng = parent.engine
        self.parent, self.op, self.engine, self.layout = parent, eng, eng, layout
        self.n_live, self.n_full = layout["n_live"], eng.n
        self.stream = parent.stream
        self._allocate(self.n_live, torch.float32, eng.dev)
        self.n = self.n_live
        self._flag = torch.zeros(1, dtype=torch.int32, device=eng.dev)
        self.__dict__["_iteration_graphs"] = parent.__dict__.setdefault("_iteration_graphs", {})
        product = lambda: eng.local_compact(self.input_buffer, self.output_buffer)  # noqa: E731
        with torch.cuda.stream(self.stream), torch.no_grad():
            product()  # warm-up (the argument tables of the compact launches)
        self.stream.synchronize()
        with torch.no_grad():
            self.graph = capture(product, parent.graph.pool())

    @property
    def calls(self):
        return self.parent.calls

    @calls.setter
    def calls(self, value):
        self.parent.calls = value

    def _live_copy(self, full, comp, scatter, rows=1, full_stride=0, comp_stride=0):
        offs, counts, periods, masks, ns = self.layout["segs"]
        _lib.check(_lib.load().hf_live_copy_rows(
            _lib.c_void_p(full.data_ptr()), _lib.c_void_p(comp.data_ptr()), int(scatter), rows, full_stride, comp_stride,
            offs, counts, periods, masks, ns, _lib.dtype_code(full.dtype), _lib.current_stream_ptr(full.device)),
            "hf_live_copy_rows")

    def gather(self, full, out=None):
        """The live entries of the flat vector ``full``, in the compact layout."""
        if out is None:
            out = torch.empty(self.n_live, dtype=full.dtype, device=full.device)
        self._live_copy(full, out, False)
        return out

    def scatter(self, compact, out):
        """``compact`` into the live entries of ``out`` (a flat vector, or the rows of a [rows, stride] pair:
        all rows in one launch); the dead entries of ``out`` are left as they are."""
        if compact.dim() == 2:
            self._live_copy(out, compact, True, compact.shape[0], out.stride(0), compact.stride(0))
        else:
            self._live_copy(out, compact, True)
        return out

    def dead_entries_zero(self, b, x0=None):
        """Whether every dead entry of ``b`` (and ``x0``) is zero: one launch, one host wait."""
        offs, counts, periods, masks, ns = self.layout["segs"]
        _lib.check(_lib.load().hf_live_dead_check(
            _lib.c_void_p(b.data_ptr()), _lib.c_void_p(x0.data_ptr()) if x0 is not None else None,
            _lib.c_void_p(self._flag.data_ptr()), offs, counts, periods, masks, ns, _lib.dtype_code(b.dtype),
            _lib.current_stream_ptr(b.device)), "hf_live_dead_check")
        return int(self._flag.item()) == 0


class GraphedOperator(CapturedOperator):
    """The local part of a curvature operator (autograd sweeps + ``hf_pack``)
    captured ONCE into a hipGraph and replayed per matvec.

    On a ResNet-18 one GGN matvec is ~700 small kernels; issued eagerly the host
    needs longer to launch them than the MI355X needs to run them.  A graph
    replay costs one launch.

    ``builder()`` must run the forward pass and return the eager operator; it is
    executed on the capture stream because autograd issues backward kernels on
    the stream their forward ran on.

    Precondition (PyTorch-ROCm 2.10 / HIP 7.0 crash the process otherwise, measured
    in scripts/experiments/graph_repro*.py): while capturing, no autograd state that ties the
    parameters to ANOTHER stream may be alive -- i.e. no ``.grad`` on them (stashed
    and restored here when ``params`` is given) and no live autograd graph built
    on another stream that reaches them (their ``AccumulateGrad`` nodes remember
    that stream and the engine then touches it during capture).
    """

    @property
    def mode(self):
        inner = getattr(getattr(self, "op", None), "mode", "")
        if "engine" in inner:
            return "hipGraph replay of the " + inner
        return "hipGraph replay of autograd sweeps + hf_pack"

    _captured_before = False  # later captures in a process need a single warm-up run

    def __init__(self, builder, warmup=None, params=None):
        if warmup is None:
            warmup = 1 if GraphedOperator._captured_before else 3
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedOperator needs a GPU")

        first = not GraphedOperator._captured_before
        GraphedOperator._captured_before = True
        stash = [(p, p.grad) for p in (params or []) if p.grad is not None]
        for p, _ in stash:
            p.grad = None
        if first or stash:
            # let dead graphs (and their AccumulateGrad nodes) go.  Later captures
            # skip this 40 ms sweep: every instance records on the SAME stream, so
            # a lingering earlier graph of ours ties the parameters to that stream only
            gc.collect()
        try:
            self._build(builder, warmup)
        finally:
            for p, g in stash:
                p.grad = g

    def _build(self, builder, warmup):
        cur = self._enter_capture()
        with torch.cuda.stream(self.stream):
            self.op = builder()
            self.group, self.params = self.op.group, self.op.params
            self._allocate(self.op.n, self.params[0].dtype, self.params[0].device)
            self._plan()
            for _ in range(warmup):
                self._product()
        self.stream.synchronize()
        self._capture_product()
        cur.wait_stream(self.stream)
        torch.cuda.synchronize()
        self._verify_replay()

    def _plan(self):
        pass

    def _product(self):
        self.op.local(self.input_buffer, out=self.output_buffer)

    def _capture_product(self):
        self.graph = self._capture(self._product, keep=True)

    _verified = set()  # signatures whose first capture in this process was checked

    def _verify_replay(self):
        """Replay twice on a random vector and compare with the eager product.

        Not paranoia: on this stack (PyTorch-ROCm 2.10, HIP 7.0, MIOpen 3.5) library
        routines that zero a scratch buffer and then accumulate into it (MIOpen's CK
        split-K weight gradient, its backward-bias, PyTorch's multi-block reductions of
        NHWC tensors) were measured to be right when issued eagerly and wrong when
        replayed from a hipGraph, the second replay differently from the first.  The
        package routes around the instances it met; a model that brings a new one
        must fail here, loudly, instead of producing wrong Newton steps.  By default
        the first capture of every signature in the process -- vector size, parameter
        shapes, shape of the network output (batch size!), operator type, device: a
        different batch or input shape selects different library kernels -- is checked
        (~2 products); ``HF_GRAPH_VERIFY=always|never`` overrides."""
        import os

        policy = os.environ.get("HF_GRAPH_VERIFY", "first")
        outputs = getattr(self.op, "outputs", None)
        key = (self.n, tuple(tuple(p.shape) for p in self.params), str(self.input_buffer.device),
               self.input_buffer.dtype, type(self.op).__name__,
               None if outputs is None else tuple(outputs.shape),
               getattr(self.op, "input_signature", None))
        if policy == "never" or (policy != "always" and key in GraphedOperator._verified):
            return
        gen = torch.Generator(device=self.input_buffer.device).manual_seed(1234)
        with torch.cuda.stream(self.stream):
            self.input_buffer.copy_(torch.randn(self.n, dtype=self.input_buffer.dtype,
                                                device=self.input_buffer.device, generator=gen))
            want = torch.empty_like(self.output_buffer)
            self.op.local(self.input_buffer, out=want)
            errs = []
            for _ in range(2):
                self.replay_local()
                errs.append(float((self.output_buffer - want).abs().max() / want.abs().max().clamp_min(1e-30)))
            self.input_buffer.zero_()
        self.stream.synchronize()
        torch.cuda.current_stream().wait_stream(self.stream)
        if not all(e < 1e-3 for e in errs):
            raise RuntimeError(
                "hipGraph replay of the curvature product does not reproduce the eager product "
                f"(relative max-norm error of two replays: {errs[0]:.2e}, {errs[1]:.2e}). A library "
                "routine inside the product is not capture-safe on this stack; run with "
                "graph_matvec=False (eager) or prepare the model with modelprep.prepare_model.")
        GraphedOperator._verified.add(key)


class OverlappedGraphedOperator(GraphedOperator):
    """Data-parallel variant: the local product is captured as TWO hipGraphs so that
    the all-reduce of the last layers' part of the vector (the adjoint sweep
    produces it first; on conv nets it is most of the bytes) runs while the rest
    of the sweep is still computing -- the schedule of
    :func:`~pytorchhessianfree_amd.distributed.two_phase_all_reduce`:

        replay G1 (tangent sweep, H_L, adjoint of the tail, pack tail)
        all-reduce(out[offset:])   -- on a side stream
        replay G2 (adjoint of the head, pack head)          <- overlaps
        all-reduce(out[:offset])
        wait for both

    The collectives stay outside the graphs.  Results are those of the unsplit
    product up to fp32 summation order.

    EXPERIMENTAL, off by default.  Measured on one MI355X (ResNet-18, batch 32):
    the split costs +0.19 ms per product (the head's sweep re-walks the tail's
    data gradients; second graph launch), and two asynchronous collectives cost
    a further ~0.4 ms of stream hand-offs even on a 1-rank RCCL group -- more than
    the ~0.3 ms of all-reduce it can hide on 44.7 MB.  It pays only where the
    all-reduce is slow (many ranks over few links, much larger vectors)."""

    mode = "2 hipGraphs per product, all-reduce of the tail overlapped with the head's adjoint sweep"
    raw_graph = None  # two graphs: cg() keeps its separate K1-K3 launches

    def __init__(self, builder, params=None, tail_fraction=0.75):
        self._tail_fraction = tail_fraction
        super().__init__(builder, params=params)

    def _plan(self):
        if not isinstance(self.op, GGNOperator):
            raise TypeError("OverlappedGraphedOperator needs a GGNOperator")
        self.cut, self.offset = self.op.split_point(self._tail_fraction)

    def _phase_tail(self):
        self.op.phase_tail(self.input_buffer, self.output_buffer, self.cut, self.offset)

    def _phase_head(self):
        self.op.phase_head(self.output_buffer, self.cut, self.offset)

    def _product(self):
        self._phase_tail()
        self._phase_head()

    def _capture_product(self):
        self.graph = self._capture(self._phase_tail)
        self.graph_head = self._capture(self._phase_head, pool=self.graph.pool())

    def replay_local(self):
        self.graph.replay()
        self.graph_head.replay()

    def replay_and_reduce(self):
        from .distributed import two_phase_all_reduce

        buf = self.output_buffer
        two_phase_all_reduce(self.graph.replay, self.graph_head.replay, [buf[: self.offset]],
                             [buf[self.offset:]], self.group, self)


def maybe_graphed(builder, enable=True, params=None):
    """``GraphedOperator(builder)`` if capture works on this stack, else the eager
    operator (still HIP: only the launch mechanism differs)."""
    if enable and torch.cuda.is_available():
        try:
            return GraphedOperator(builder, params=params)
        except Exception as exc:  # capture not supported for some op on this stack
            import warnings

            warnings.warn(f"hipGraph capture of the matvec failed ({exc!r}); running it eagerly")
            torch.cuda.synchronize()
    return builder()
