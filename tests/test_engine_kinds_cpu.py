"""The three engine kinds and the contract they share (engine/base.py): who inherits what, what each kind declares, what
the kinds answer before anything is built, the two layout helpers, and that the callers read the contract instead of
probing for it.  Import only: no GPU."""

import ast
import itertools
import os
import weakref

import pytest
import torch
from torch import nn

from pytorchhessianfree_amd.engine import DenseStackEngine, FusedGGNEngine, PlainStackEngine, _Engine, _Unsupported
from pytorchhessianfree_amd.engine.adjoint import _AdjointSweep
from pytorchhessianfree_amd.engine.buffers import _Buffers
from pytorchhessianfree_amd.engine.common import mark_dead_prefix, records_of
from pytorchhessianfree_amd.engine.conv import _ConvEngine
from pytorchhessianfree_amd.engine.dataparallel import _DataParallel
from pytorchhessianfree_amd.engine.diag_ef import _DiagEF
from pytorchhessianfree_amd.engine.forward import _Forward
from pytorchhessianfree_amd.engine.hessian import _HessianExtras
from pytorchhessianfree_amd.engine.tangent import _TangentSweep
from pytorchhessianfree_amd.engine.topology import _Topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (FusedGGNEngine, PlainStackEngine, DenseStackEngine)
CONTRACT = {"mode", "supports_hessian", "supports_session", "supports_two_phase", "supports_compact", "acc_decline",
            "session_decline", "has_weight_copies", "verify_tol", "hessian", "train_bn", "frozen_any", "_l2"}
ACC_ONLY = "the dense-stack engine serves step() sessions only"
OPT_IN = "the dense-stack engine is opt-in (set HF_DENSE_ENGINE=1)"
NO_HESSIAN = "no Hessian products unless HF_DENSE_HESSIAN=1 (opt-in on top of HF_DENSE_ENGINE=1)"
NO_SESSION = "the dense-stack engine has no session yet (opt-in: set HF_DENSE_SESSION=1)"


def _contract_of_base():
    """The plain class attributes ``_Engine`` itself declares: the contract (methods, properties and dunders are not)."""
    return {k for k, v in vars(_Engine).items()
            if not k.startswith("__") and not callable(v) and not isinstance(v, (classmethod, staticmethod, property))}


RESIDUAL_ONLY = ("phase_split", "local_phase_a", "local_phase_b", "local_compact", "_tangent_stem", "_tangent_blocks",
                 "_adjoint_blocks", "_adjoint_stem", "_grouping", "_head_fused")
RESIDUAL_ATTRIBUTES = ("stem", "blocks", "fc", "pool_args", "pfw", "pfb")


def test_who_inherits_what():
    unit_mixins = (_Buffers, _Forward, _TangentSweep, _AdjointSweep, _HessianExtras, _DiagEF, _DataParallel)
    conv_mixins = (_Topology,) + unit_mixins
    assert _Engine in DenseStackEngine.__mro__
    assert not set(conv_mixins + (_ConvEngine,)) & set(DenseStackEngine.__mro__)
    assert FusedGGNEngine not in DenseStackEngine.__mro__
    for name in ("phase_split", "local_phase_a", "local_phase_b", "compact_layout", "local_compact"):
        assert not hasattr(DenseStackEngine, name), name
        assert hasattr(FusedGGNEngine, name), name
    # the two conv kinds: siblings on the conv base, the residual walks on the residual kind alone
    assert _ConvEngine in FusedGGNEngine.__mro__ and _ConvEngine in PlainStackEngine.__mro__
    assert not issubclass(PlainStackEngine, FusedGGNEngine) and _Topology not in PlainStackEngine.__mro__
    assert issubclass(FusedGGNEngine, _Engine) and issubclass(PlainStackEngine, _Engine)
    assert set(conv_mixins) <= set(FusedGGNEngine.__mro__) and set(unit_mixins) <= set(PlainStackEngine.__mro__)
    for kind in (FusedGGNEngine, PlainStackEngine):
        for name in ("local", "gradient", "_gather", "forward_own", "diag_ef"):  # ONE skeleton
            assert getattr(kind, name) is getattr(_ConvEngine, name), (kind.__name__, name)
        assert hasattr(kind, "compact_layout")
    for name in RESIDUAL_ONLY:
        assert not hasattr(PlainStackEngine, name), name
        assert hasattr(FusedGGNEngine, name), name
    # one process on the base, the compact all-reduce on the conv kinds
    assert DenseStackEngine.reduce is _Engine.reduce and DenseStackEngine.reduce_bytes is _Engine.reduce_bytes
    assert FusedGGNEngine.reduce is _DataParallel.reduce and FusedGGNEngine.reduce_bytes is _DataParallel.reduce_bytes
    assert PlainStackEngine.reduce is _DataParallel.reduce


def test_contract_values_per_kind():
    assert _contract_of_base() == CONTRACT
    for kind in KINDS:
        for name in CONTRACT:
            getattr(kind, name)  # readable on the class
    #          hessian session two_phase compact acc_decline has_weight_copies
    table = {FusedGGNEngine: (True, True, True, True, None, True),
             PlainStackEngine: (True, True, False, False, None, True),
             DenseStackEngine: (True, False, False, False, ACC_ONLY, False)}
    for kind, want in table.items():
        got = (kind.supports_hessian, kind.supports_session, kind.supports_two_phase, kind.supports_compact,
               kind.acc_decline, kind.has_weight_copies)
        assert got == want, (kind.__name__, got)
        assert kind.session_decline is None and kind.verify_tol == 1e-5
        assert (kind.hessian, kind.train_bn, kind.frozen_any, kind._l2) == (False, False, False, None)
        assert "fused curvature engine" in kind.mode
    assert len({kind.mode for kind in KINDS}) == 3


@pytest.mark.parametrize("engine,hess,sess", list(itertools.product(("0", "1", None), ("1", None), ("1", None))))
def test_unavailable(monkeypatch, engine, hess, sess):
    for name, value in (("HF_DENSE_ENGINE", engine), ("HF_DENSE_HESSIAN", hess), ("HF_DENSE_SESSION", sess)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    for hessian, need_session in itertools.product((False, True), (False, True)):
        assert FusedGGNEngine.unavailable(hessian, need_session) is None
        assert PlainStackEngine.unavailable(hessian, need_session) is None
        if engine != "1":
            want = OPT_IN
        elif hessian and hess != "1":
            want = NO_HESSIAN
        elif need_session and sess != "1":
            want = NO_SESSION
        else:
            want = None
        assert DenseStackEngine.unavailable(hessian, need_session) == want, (hessian, need_session)


def test_base_unavailable_reads_the_flags():
    class GGNOnly(_Engine):
        supports_hessian = False
        supports_session = False

    assert GGNOnly.unavailable(False, False) is None
    assert GGNOnly.unavailable(True, True) == "no Hessian products (GGN only)"
    assert GGNOnly.unavailable(False, True) == "no persistent session on this engine yet"


def test_try_build_declines_without_a_gpu(monkeypatch):
    monkeypatch.delenv("HF_ENGINE", raising=False)
    model = nn.Linear(3, 2)
    outputs = model(torch.zeros(4, 3))
    loss = outputs.sum()
    why = []
    assert FusedGGNEngine.try_build(loss, outputs, list(model.parameters()), why=why) is None
    assert len(why) == 1 and why[0].startswith("the model is not a prepared one (modelprep.prepare_model("), why
    outputs._hf_model = weakref.ref(model)
    for kind in KINDS:
        why = []
        assert kind.try_build(loss, outputs, list(model.parameters()), why=why) is None
        assert why == ["the model output is not a CUDA float32 [batch, classes] tensor (got torch.float32, (4, 2), cpu)"]
    monkeypatch.setenv("HF_ENGINE", "0")
    why = []
    assert FusedGGNEngine.try_build(loss, outputs, list(model.parameters()), why=why) is None
    assert why == ["the fused engine is switched off (HF_ENGINE=0)"]


class _L:
    def __init__(self, pw, pb):
        self.pw, self.pb, self.dead = pw, pb, False


def test_mark_dead_prefix():
    layers = [_L(0, 1), _L(None, None), _L(2, None)]
    assert mark_dead_prefix(layers) == 0 and [u.dead for u in layers] == [False, False, False]
    layers = [_L(None, None), _L(None, None), _L(None, 0)]  # (a trainable bias alone keeps a layer alive)
    assert mark_dead_prefix(layers) == 2 and [u.dead for u in layers] == [True, True, False]
    layers = [_L(None, None), _L(0, 1), _L(None, None)]  # (frozen BEHIND a live layer: not dead)
    assert mark_dead_prefix(layers) == 1 and [u.dead for u in layers] == [True, False, False]
    with pytest.raises(_Unsupported, match="^every layer is frozen$"):
        mark_dead_prefix([_L(None, None), _L(None, None), _L(None, None)])


def test_records_of():
    m = nn.ReLU()
    with pytest.raises(_Unsupported, match="^ReLU has no record of this forward pass$"):
        records_of(m)
    a, b = torch.zeros(1), torch.ones(1)
    m._hf_io = (a, b)
    assert records_of(m) == (a, b) and records_of(m, with_input=True) == (a, b)
    with pytest.raises(_Unsupported, match="^ReLU has no record"):
        records_of(m, 5)
    m._hf_io = (a,)
    with pytest.raises(_Unsupported, match="^ReLU has no record"):
        records_of(m)
    m._hf_io = (None, b)
    assert records_of(m)[1] is b
    with pytest.raises(_Unsupported, match="^ReLU has no record"):
        records_of(m, with_input=True)
    bn = nn.BatchNorm2d(2)
    bn._hf_io = (a, None, b, True, a)
    assert len(records_of(bn, 5)) == 5
    with pytest.raises(_Unsupported, match="^BatchNorm2d has no record"):
        records_of(bn)


def test_callers_read_the_contract():
    """No ``getattr(x, "<contract attribute>", default)`` on a name or an attribute in the engines' callers: every
    engine has the attribute, and a default would say again who the odd kind is.  (``GraphedOperator.mode`` asks an
    operator that may not be there yet, ``getattr(getattr(self, "op", None), "mode", "")``: no engine probe.)"""
    contract = _contract_of_base()
    for name in ("session.py", "acc_session.py", "curvature.py"):
        path = os.path.join(ROOT, "pytorchhessianfree_amd", name)
        for node in ast.walk(ast.parse(open(path).read())):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr"
                    and len(node.args) >= 2 and isinstance(node.args[0], (ast.Name, ast.Attribute))
                    and isinstance(node.args[1], ast.Constant)):
                assert node.args[1].value not in contract, (name, node.lineno, node.args[1].value)


def test_unit_level_code_reads_nothing_residual():
    """The conv base and the unit-level mixins know a list of conv units and nothing about how a residual net wires
    them: no ``self.stem`` / ``blocks`` / ``fc`` / ``pool_args`` / ``pfw`` / ``pfb`` in any of these files (the residual
    kind's walks, its max-pool and its linear head stand in engine/core.py and engine/topology.py)."""
    for name in ("conv.py", "buffers.py", "diag_ef.py", "hessian.py", "forward.py", "tangent.py", "adjoint.py",
                 "dataparallel.py", "plain.py"):
        path = os.path.join(ROOT, "pytorchhessianfree_amd", "engine", name)
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self":
                assert node.attr not in RESIDUAL_ATTRIBUTES, (name, node.lineno, node.attr)
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ("getattr", "hasattr")
                    and len(node.args) >= 2 and isinstance(node.args[1], ast.Constant)):
                assert node.args[1].value not in RESIDUAL_ATTRIBUTES, (name, node.lineno, node.args[1].value)


REMOVED_FROM_LIB = ("conv_group_slabs", "conv_group_slabs_bnsum", "conv_dw_slabs", "_fill_problem")
# what the engines ask the library without launching anything: the planners and the table-size queries
PLANNERS = {"hf_conv2d_nhwc_plan", "hf_conv2d_nhwc_sqsum_plan", "hf_dense_plan", "hf_linear_ce_head_slabs",
            "hf_bn_sums_table"}


def _engine_sources():
    folder = os.path.join(ROOT, "pytorchhessianfree_amd", "engine")
    return {name: open(os.path.join(folder, name)).read() for name in sorted(os.listdir(folder)) if name.endswith(".py")}


def test_one_path_to_the_launching_entry_points():
    """The binding holds no engine code for the grouped / paired convolutions, and outside ``common.py`` (the launcher)
    no engine file calls an ``hf_*`` attribute of the loaded library itself -- but the planners, which launch nothing."""
    from pytorchhessianfree_amd import _lib

    for name in REMOVED_FROM_LIB:
        assert not hasattr(_lib, name), name
    sources = _engine_sources()
    assert "common.py" in sources and len(sources) > 10
    for name, text in sources.items():
        if name == "common.py":
            continue
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("hf_"):
                assert node.func.attr in PLANNERS, (name, node.lineno, node.func.attr)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name):
                assert node.func.id != "getattr" or not any(  # (nor fetches one by name)
                    isinstance(a, ast.Call) and isinstance(a.func, ast.Attribute) and a.func.attr == "load"
                    for a in node.args[:1]), (name, node.lineno)


def test_geometries_are_read_by_field():
    """No engine file indexes or slices a geometry (``geo[``) or unpacks one into nine names."""
    for name, text in _engine_sources().items():
        assert "geo[" not in text and "geo1[" not in text and "geo_w[" not in text, name
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, (ast.Assign, ast.For)):
                targets = node.targets if isinstance(node, ast.Assign) else [node.target]
                for t in targets:
                    assert not (isinstance(t, ast.Tuple) and len(t.elts) == 9), (name, node.lineno)
