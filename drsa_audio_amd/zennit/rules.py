"""LRP rule descriptors with zennit 0.5.1 names and constructor signatures.

Semantics (reference name maps ``constants.py:27-51``):
  Epsilon(ε)   R_in = x ⊙ Jᵀ_W(R / stab_ε(z))
  Gamma(γ, ε)  W± = W + γ·W.clamp(min/max=0) (bias likewise); positive/negative output split;
               den± = f(x+; W±, b±) + f(x-; W∓, 0) (zennit 0.5.1 zero_bias on the x- terms)
  WSquare(ε)   R_in = Jᵀ_{W²}(R / stab_ε(conv(1; W², b²)))
  Flat(ε)      as WSquare with W -> 1, b -> 0
  Pass()       R_in = R_out (activation layers only)
  ZPlus(ε)     z = f(x+; W+, b+) + f(x-; W-, 0);  R_in = x+ ⊙ Jᵀ_{W+} g + x- ⊙ Jᵀ_{W-} g,
               g = R / stab_ε(z)   (conv layers; runs on the Gamma kernels with these sets)
  AlphaBeta(α, β, ε)  positive set (x+, W+, b+) + (x-, W-, 0), negative set (x+, W-, b-) + (x-, W+, 0),
               one denominator per set; R_in = α·pos − β·neg (HIP engine: convs with a non-negative
               input; elsewhere compiling the composite raises ``EngineError``)
  Norm(ε)      ≡ Epsilon(ε) on conv/dense layers
  ZBox(low, high, ε)  for an input in the box low ≤ x ≤ high, l / h = low[:1] / high[:1] spread over x:
               den = (f(x; W, b) − f(l; W+, b+)) − f(h; W−, b−),  g = R / stab_ε(den),
               R_in = x ⊙ Jᵀ_W g − l ⊙ Jᵀ_{W+} g − h ⊙ Jᵀ_{W−} g   (b = b+ + b−: the bias cancels in den, so the
               rule conserves with or without a bias; den ≥ 0 inside the box.  HIP engine: the first conv,
               one input channel; elsewhere compiling the composite raises ``EngineError``)
Every rule but AlphaBeta, ZBox and Pass also compiles on the dense head (``classifier.*``), with the same
semantics on ``f = Linear`` and a signed or non-negative input:

  rule      conv trunk                      dense head
  Epsilon   yes                             yes
  Norm      yes (≡ Epsilon)                 yes (≡ Epsilon)
  Gamma     yes                             yes (den- too where no ReLU follows the layer)
  ZPlus     yes                             yes
  WSquare   yes                             yes (den = f(1; W², b²), one constant per output neuron);
                                            on ``classifier.0`` only with the last conv's ReLU unmapped
  Flat      yes                             as WSquare
  AlphaBeta non-negative input only         ``EngineError``
  ZBox      first conv, Cin = 1, only       ``EngineError``
  Pass     activations only                activations only
``zero_params`` on a dense layer raises ``EngineError``.
WSquare / Flat do not multiply by the layer's input, so under a Pass on the ReLU below them relevance
reaches units with z <= 0.  Inside the head the plan runs that case (the layer below takes unmasked
relevance).  On ``classifier.0`` above a Pass on the last conv block's ReLU it raises ``EngineError``:
the conv kernels have no [z < 0] branch.  ``PixelFlipping`` maps Pass to every activation, so its
``'dense'`` key cannot name ``wsquare`` or ``flat``.
A ``Hook`` subclass with its own ``backward`` (not a descriptor) runs on the autograd slow path
(``engine/hooks.py``).
"""
from __future__ import annotations

from .core import BasicHook, Stabilizer


class Epsilon(BasicHook):
    kind = "epsilon"

    def __init__(self, epsilon=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.epsilon = Stabilizer.ensure(epsilon).epsilon


class Gamma(BasicHook):
    kind = "gamma"

    def __init__(self, gamma=0.25, stabilizer=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.gamma = float(gamma)
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon


class WSquare(BasicHook):
    kind = "wsquare"

    def __init__(self, stabilizer=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon


class Flat(BasicHook):
    kind = "flat"

    def __init__(self, stabilizer=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon


class Pass(BasicHook):
    kind = "pass"

    def __init__(self):
        super().__init__()


class ZPlus(BasicHook):
    kind = "zplus"

    def __init__(self, stabilizer=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon


class AlphaBeta(BasicHook):
    kind = "alphabeta"

    def __init__(self, alpha=2.0, beta=1.0, stabilizer=1e-6, zero_params=None):
        # zennit 0.5.1 refuses these configurations (conservation needs alpha - beta = 1)
        if alpha < 0 or beta < 0:
            raise ValueError("Both alpha and beta parameters must be non-negative!")
        if (alpha - beta) != 1.0:
            raise ValueError("The difference of parameters alpha - beta must equal 1!")
        super().__init__(zero_params)
        self.alpha, self.beta = float(alpha), float(beta)
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon


class ZBox(BasicHook):
    """zennit ZBox: the first-layer rule for an input bounded by ``low <= x <= high``.

    ``low`` / ``high``: Python floats, or tensors broadcastable to one sample ``[1, 1, H, W]``; a tensor
    with a batch dimension greater than 1 contributes its first row (zennit's ``low[:1]``).  Inputs
    outside the box are NOT checked (zennit does not check them either): there the denominator can
    change sign and the heatmap loses its meaning, silently."""
    kind = "zbox"

    def __init__(self, low, high, stabilizer=1e-6, zero_params=None):
        super().__init__(zero_params)
        self.low, self.high = low, high
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon

    def bounds(self, x):
        """(l, h): both bounds spread over ``x`` (``low[:1].expand_as(x)``), in x's dtype on x's device."""
        return tuple(_bound(v, x) for v in (self.low, self.high))


def _bound(v, x):
    import torch
    t = torch.as_tensor(v).detach().to(device=x.device, dtype=x.dtype)
    if t.dim() == x.dim() and t.size(0) > 1:
        t = t[:1]
    return t.expand_as(x)


class Norm(BasicHook):
    kind = "norm"

    def __init__(self, stabilizer=1e-6):
        super().__init__()
        self.stabilizer = Stabilizer.ensure(stabilizer).epsilon
