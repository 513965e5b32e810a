"""GPU: the launch sequence of the engines (``FusedGGNEngine``, ``PlainStackEngine``, ``DenseStackEngine``) WITH ARGUMENTS
-- every ``hf_*`` call that ``forward_own()``, ``local(v)``, ``gradient(out)`` (on a dense stack also ``gradient()``) and
``diag_ef("mean")`` issue, eagerly, on small nets -- against
``tests/golden/engine_launch_sequence.json.gz`` (one call per line; gzip, since most of its 2 500 lines are the per-sample
launches of ``diag_ef``, equal but for the addresses' ranks).

The golden file is a recording of the commit BEFORE the launcher and the problem builders (``engine/common._Launcher``,
``engine/problems.py``) replaced the raw ctypes calls; the ``dense_*`` cases of the commit BEFORE the chain of ``Linear``
layers (``engine/linear.py``) replaced the dense-stack engine's own loops: the code under test is never the source of its
own expectation.  It is rewritten only from a checkout that is trusted to launch correctly, put first on
``PYTHONPATH``::

    PYTHONPATH=<trusted checkout> python tests/test_engine_launch_sequence_gpu.py tests/golden/engine_launch_sequence.json.gz

Recording (as ``test_dense_launch_order_gpu.py``: ``_lib.load`` returns a proxy around the library): name and arguments of
every call of an entry point of ``_lib.SIGNATURES``; the stream is dropped; every distinct non-null address is replaced by
``"@k"``, k its rank of first appearance within the recording of one operation; struct arguments (the two-problem forms,
the grouped convolutions, the sums table) are decoded field by field, pointer arrays (pack / unpack) entry by entry.
While an operation is recorded every tensor it creates is kept alive (``KeepAlive``): a temporary freed in the middle of
it could otherwise hand its address to a later one, and whether it does depends on the allocator's state, not on the
engine."""

import ctypes
import gzip
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from engine_nets import DEV, build, build_plain, net_and_loss
from pytorchhessianfree_amd import _lib, curvature, modelprep
from pytorchhessianfree_amd import testproblems as tp
from pytorchhessianfree_amd.engine import FusedGGNEngine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_sequence.json.gz")

# case -> how the engine is built.  ``wide``: batch 16, 32 / 64 channels -- the stem, an identity block, a downsample block
# with rb > 1 on both of its first units (the two-problem forms), a third block on a 1x1 map (rb == 1)
CASES = {
    "plain": lambda: build("wide"),
    "frozen": lambda: build("wide", "scale_shift"),
    "fused": lambda: build("wide"),  # (HF_BN_SUMS_DEFER=0, see ENV: the fused adjoint launches, single and pair)
    "train": lambda: build("wide", train=True),
    "hessian": lambda: build("wide", hessian=True),
    "hessian_train": lambda: build("wide", train=True, hessian=True),
    "stack": lambda: build_plain(),
    "stack_hessian": lambda: build_plain(hessian=True),
    # ``testproblems.convpool_small`` as ``test_pooled_stack_engine_gpu.py`` builds it, batch 2: two pooled units
    "stack_pooled": lambda: build_pooled(),
    "stack_pooled_hessian": lambda: build_pooled(hessian=True),
    "stack_frozen": lambda: build_pooled(freeze_first=True),  # (the pooled first layer dead for both sweeps)
    # the Hessian extras in sequence (``acc_session.AccumulatedSession``'s parallel chunks: no side branch)
    "hessian_seq": lambda: sequential_extras(build("wide", hessian=True)),
    "stack_hessian_seq": lambda: sequential_extras(build_plain(hessian=True)),
    "diag_batched": lambda: build("wide"),  # (HF_DIAG_EF_BATCHED=1, see ENV: one squared-sum launch per layer)
    "stack_diag_batched": lambda: build_plain(),
    # the dense stack: nets A and D of ``test_dense_launch_order_gpu.py`` (D: only a bias tangent enters the first layer)
    "dense_ggn": lambda: build_dense("A", "ggn"),
    "dense_hessian": lambda: build_dense("A", "hessian"),
    "dense_session": lambda: build_dense("A", "session"),
    "dense_bias_only": lambda: build_dense("D", "ggn"),
}
DENSE = {"ggn": {"HF_DENSE_ENGINE": "1", "HF_DENSE_HESSIAN": "0", "HF_DENSE_SESSION": "0"},
         "hessian": {"HF_DENSE_ENGINE": "1", "HF_DENSE_HESSIAN": "1", "HF_DENSE_SESSION": "0"},
         "session": {"HF_DENSE_ENGINE": "1", "HF_DENSE_HESSIAN": "0", "HF_DENSE_SESSION": "1"}}
ENV = {"fused": {"HF_BN_SUMS_DEFER": "0"}, "diag_batched": {"HF_DIAG_EF_BATCHED": "1"},
       "stack_diag_batched": {"HF_DIAG_EF_BATCHED": "1"}, "dense_ggn": DENSE["ggn"], "dense_hessian": DENSE["hessian"],
       "dense_session": DENSE["session"], "dense_bias_only": DENSE["ggn"]}
# the operations recorded per case: all four unless listed here, the diagonal only where it is the case's subject (most
# of the file's lines are ``diag_ef``'s per-sample launches)
ALL_OPS = ("forward_own", "local", "gradient", "diag_ef")
OPS = {case: ALL_OPS[:3] for case in
       ("stack_pooled", "stack_pooled_hessian", "stack_frozen", "hessian_seq", "stack_hessian_seq")}
OPS.update(diag_batched=("diag_ef",), stack_diag_batched=("diag_ef",))
# the dense stack: what ``test_dense_launch_order_gpu.py`` runs per kind (``gradient(out)`` of a GGN engine outside session
# mode raises before anything is launched)
OPS.update(dense_hessian=ALL_OPS + ("gradient_kept",), dense_session=ALL_OPS + ("gradient_kept",))


def build_pooled(hessian=False, freeze_first=False):
    model, (x, t), lossf = tp.convpool_small(batch_size=2, device="cpu")
    if freeze_first:
        for p in next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d)).parameters():
            p.requires_grad_(False)
    model, x, t = model.to(DEV), x.to(DEV), t.to(DEV)
    modelprep.prepare_model(model, channels_last=True)
    out = model(x)
    make_op = curvature.hessian_operator if hessian else curvature.ggn_operator
    op = make_op(lossf(out, t), out, [p for p in model.parameters() if p.requires_grad])
    assert type(op).__name__ == "PlainStackEngine" and op.hessian == hessian
    return op


def build_dense(net, kind):
    model, out, loss = net_and_loss(net)
    why = []
    op = FusedGGNEngine.try_build(loss, out, [p for p in model.parameters() if p.requires_grad], hessian=kind == "hessian",
                                  why=why, need_session=kind == "session")
    assert type(op).__name__ == "DenseStackEngine" and (op.loss_spec is not None) == (kind == "session"), why
    return op


def sequential_extras(op):
    op._extras_allowed = False
    return op


# every BatchNorm / affine / adjoint / sums / statistics / pooling / head / pack / convolution entry point the engine
# mixins call in these four operations: the cases together must reach each of them
REQUIRED = [
    "hf_bn_forward", "hf_bn_stats_rows", "hf_bn_forward_train", "hf_maxpool_forward_nhwc", "hf_maxpool_tangent_nhwc",
    "hf_maxpool_adjoint_nhwc", "hf_chan_affine_ex", "hf_chan_affine_pair", "hf_chan_affine_train",
    "hf_chan_affine_train_pair", "hf_chan_affine_bwd_ex", "hf_chan_affine_bwd_pair", "hf_bn_adjoint_v4",
    "hf_bn_adjoint_v4_pair", "hf_bn_sums_multi", "hf_bn_train_hessian_coeffs", "hf_bn_train_hessian_apply",
    "hf_linear_ce_head", "hf_pool_ce_head", "hf_pack_ex", "hf_unpack_weights", "hf_conv2d_nhwc_slabs",
    "hf_conv2d_nhwc_slabs_unpack", "hf_conv2d_nhwc_backward_slabs", "hf_conv2d_nhwc_group_slabs",
    "hf_conv2d_nhwc_group_slabs_bnsum", "hf_conv2d_nhwc_dw_slabs", "hf_pool_act_tangent_nhwc",
    "hf_pool_act_adjoint_nhwc", "hf_conv2d_nhwc_sqsum_slabs", "hf_chan_sqsum",
    # the chain of ``Linear`` layers (the dense stack)
    "hf_softmax_ce_hvp", "hf_dense_tangent_slabs", "hf_dense_act_forward", "hf_dense_act_tangent", "hf_dense_act_adjoint",
    "hf_dense_act_adjoint2", "hf_dense_wgrad", "hf_dense_wgrad2", "hf_dense_dgrad_slabs", "hf_dense_dgrad2_slabs",
    "hf_dense_sq_wgrad", "hf_dense_sq_colsum", "hf_dense_loss_head",
]

# struct arguments: entry point -> {argument index: (struct, count or the index of the argument that holds it)}
STRUCTS = {
    "hf_chan_affine_pair": {0: (_lib.AffineProblem, 2)},
    "hf_chan_affine_bwd_pair": {0: (_lib.BnAdjointProblem, 2)},
    "hf_bn_adjoint_v4_pair": {0: (_lib.BnAdjointProblem, 2)},
    "hf_chan_affine_train_pair": {0: (_lib.AffineTrainProblem, 2)},
    "hf_conv2d_nhwc_group_slabs": {0: (_lib.ConvProblem, "1")},
    "hf_conv2d_nhwc_group_slabs_bnsum": {0: (_lib.ConvProblem, "1"), 2: (_lib.ConvBnSum, "1")},
    "hf_conv2d_nhwc_dw_slabs": {0: (_lib.ConvProblem, 1), 1: (_lib.ConvProblem, 1)},
    "hf_bn_sums_multi": {1: (_lib.BnSumsProblem, "2")},
}


class Recorder:
    """Forwards every attribute to the real library; a call of an entry point of ``_lib.SIGNATURES`` is appended to
    ``calls`` as ``[name, argument, ...]`` in the normal form of the module's docstring."""

    def __init__(self, lib):
        self._lib, self.calls, self._ranks = lib, [], {}

    def restart(self):
        self.calls, self._ranks = [], {}

    def _rank(self, address):
        if isinstance(address, ctypes.c_void_p):
            address = address.value
        if not address:
            return None
        return "@%d" % self._ranks.setdefault(int(address), len(self._ranks))

    def _struct(self, kind, pointer, count):
        arr = ctypes.cast(pointer, ctypes.POINTER(kind * count)).contents
        return [{name: (self._rank(getattr(q, name)) if ctype is ctypes.c_void_p else getattr(q, name))
                 for name, ctype in kind._fields_} for q in arr]

    def _normal(self, name, args):
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        if len(argtypes) >= 3 and argtypes[-1] is ctypes.c_void_p and argtypes[-2] is ctypes.c_int:
            args, argtypes = args[:-1], argtypes[:-1]  # (int dtype, void* stream): the stream is dropped
        out = [name]
        for i, (a, ctype) in enumerate(zip(args, argtypes)):
            if i in STRUCTS.get(name, {}):
                kind, count = STRUCTS[name][i]
                out.append(self._struct(kind, a, args[int(count)] if isinstance(count, str) else count))
            elif ctype is ctypes.c_void_p:
                out.append(self._rank(a))
            elif isinstance(a, ctypes.Array):
                out.append([self._rank(e) for e in a] if a._type_ is ctypes.c_void_p else list(a))
            else:
                out.append(getattr(a, "value", a))
        return out

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _lib.SIGNATURES:
            return fn

        def call(*args):
            self.calls.append(self._normal(name, args))
            return fn(*args)

        return call


class KeepAlive(TorchDispatchMode):
    """Holds the result of every torch operation until the mode is left: no address is used twice inside it."""

    def __init__(self):
        super().__init__()
        self.kept = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.kept.append(out)
        return out


def record(case, setenv, patch_load):
    """{operation: recorded calls, or what it raised} of one case; ``setenv(name, value)`` and ``patch_load(fn)`` are the
    caller's way to change the environment and ``_lib.load``."""
    setenv("HF_ENGINE_VERIFY", "never")  # (the first-use check against autograd is not what is recorded)
    for name, value in ENV.get(case, {}).items():
        setenv(name, value)
    rec = Recorder(_lib.load())
    patch_load(lambda: rec)
    op = CASES[case]()
    v = torch.randn(op.n, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = torch.empty(op.n, device=DEV)
    got = {}
    for what, call in (("forward_own", op.forward_own), ("local", lambda: op.local(v)),
                       ("gradient", lambda: op.gradient(out)), ("gradient_kept", lambda: op.gradient()),
                       ("diag_ef", lambda: op.diag_ef("mean"))):
        if what not in OPS.get(case, ALL_OPS):
            continue
        rec.restart()
        with KeepAlive():
            try:
                call()
                got[what] = rec.calls
            except RuntimeError as exc:  # (diag_ef of a train-mode engine: refused before anything is launched)
                got[what] = {"raises": type(exc).__name__, "after": rec.calls}
            torch.cuda.synchronize()
    return json.loads(json.dumps(got))


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_launches_and_their_arguments_equal_the_recorded_ones(case, recorded, monkeypatch):
    got = record(case, monkeypatch.setenv, lambda fn: monkeypatch.setattr(_lib, "load", fn))
    want = recorded[case]
    assert list(got) == list(want)
    for what in want:
        if isinstance(want[what], dict):
            assert got[what] == want[what], what
            continue
        assert [c[0] for c in got[what]] == [c[0] for c in want[what]], f"{what}: another sequence of entry points"
        for k, (g, w) in enumerate(zip(got[what], want[what])):
            assert g == w, f"{what}: call {k} ({w[0]})"


def test_the_recording_reaches_every_entry_point_of_the_layer_launches(recorded):
    assert sorted(recorded) == sorted(CASES)
    reached = {c[0] for ops in recorded.values() for calls in ops.values()
               for c in (calls["after"] if isinstance(calls, dict) else calls)}
    assert not [name for name in REQUIRED if name not in reached]


if __name__ == "__main__":
    real, cases = _lib.load, {}
    for case_ in CASES:
        before = dict(os.environ)
        try:
            cases[case_] = record(case_, os.environ.__setitem__, lambda fn: setattr(_lib, "load", fn))
        except Exception:  # noqa: BLE001  (the other cases still say what they reach; the exit status is the failure)
            import traceback

            traceback.print_exc()
        _lib.load = real
        os.environ.clear()
        os.environ.update(before)
    text = ",\n".join(
        json.dumps(c) + ": {\n" + ",\n".join(
            json.dumps(w) + ": " + (json.dumps(calls, separators=(",", ":")) if isinstance(calls, dict) else
                                    "[\n" + ",\n".join(json.dumps(call, separators=(",", ":")) for call in calls) + "\n]")
            for w, calls in ops.items()) + "\n}" for c, ops in cases.items())
    with open(sys.argv[1], "wb") as f, gzip.GzipFile("", "wb", 9, f, mtime=0) as z:  # (no name, no time: same bytes again)
        z.write(("{\n" + text + "\n}\n").encode())
    names = {c[0] for ops in cases.values() for calls in ops.values()
             for c in (calls["after"] if isinstance(calls, dict) else calls)}
    print("package:", os.path.dirname(_lib.__file__))
    print("calls:", {c: {w: len(x["after"] if isinstance(x, dict) else x) for w, x in ops.items()} for c, ops in cases.items()})
    print("not reached:", [name for name in REQUIRED if name not in names])
    print("raised:", {c: {w: x["raises"] for w, x in ops.items() if isinstance(x, dict)} for c, ops in cases.items()})
    sys.exit(0 if len(cases) == len(CASES) else 1)
