"""dhts -- MI355X-native differentiable traffic stepper (ARZ cell stencil + IDM ODE, forward + adjoint).

Host-side Python over libdhts.so (hand-written HIP for gfx950, C ABI in include/dhts.h).
"""
from . import _lib, dist, ops  # noqa: F401
from ._lib import DhtsError  # noqa: F401
from .ops import (MacroRollout, MacroRolloutRamp, MacroRolloutRing, MacroRolloutRingTarget, MacroRolloutTarget, MicroRollout, MicroRolloutLead, MicroRolloutRing, MicroRolloutRingTarget,  # noqa: F401
                  MicroRolloutSamples, MicroRolloutTarget, macro_rollout, micro_rollout)
from .jvp import macro_rollout_jvp, micro_rollout_jvp  # noqa: F401
