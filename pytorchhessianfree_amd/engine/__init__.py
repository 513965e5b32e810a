"""The fused curvature engines: GGN and Hessian products of a prepared model by explicit tangent and adjoint sweeps over
its layers, issued as direct kernel launches.  Three kinds on one base (``_Engine``, engine/base.py: the contract callers
read, ``try_build``): ``FusedGGNEngine`` for ResNet families and ``PlainStackEngine`` for conv-ReLU(-MaxPool) stacks, both
on ``_ConvEngine`` (engine/conv.py: one product and gradient skeleton over a list of conv units), ``DenseStackEngine`` for
MLPs.  Why and how the sweeps are built: engine/core.py."""

from .base import _Engine  # noqa: F401
from .common import _Unsupported, _live_taps, ce_loss_spec, loss_spec_of, mse_loss_spec  # noqa: F401
from .core import FusedGGNEngine  # noqa: F401
from .dense import DenseStackEngine  # noqa: F401
from .plain import PlainStackEngine  # noqa: F401
