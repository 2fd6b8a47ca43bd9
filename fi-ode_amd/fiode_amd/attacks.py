"""The two validation attacks of the reference (pl_modules.py:189-195), restated from their published
algorithm: projected gradient descent (Madry et al., "Towards Deep Learning Models Resistant to
Adversarial Attacks", 2018) in the L-infinity ball (``PGD``) and in the L2 ball (``PGDL2``), with the
conventions of the torchattacks classes the reference calls (torchattacks is not a dependency):

  * the cost is ``nn.CrossEntropyLoss()`` on the model's outputs, applied as it stands even when the
    outputs are simplex probabilities (the reference's model under ``simplex=True``);
  * the gradient is taken with respect to the image only (``torch.autograd.grad``); parameters are
    left alone -- run the attack inside ``fiode_amd.lyapunov.no_param_grad(model)`` so that the
    native ODE solve takes its input-gradient route;
  * images live in [0, 1]: the start point and every iterate are clamped to it;
  * ``random_start=True`` is the default: Linf starts at x + U(-eps, eps); L2 at x + eps * d with
    d a normal draw scaled to unit L2 norm per image times r ~ U(0, 1), as torchattacks does;
  * L2 step ``alpha * grad / (||grad||_2 + 1e-10)`` per image and projection
    ``delta * min(1, eps / ||delta||_2)``; Linf step ``alpha * sign(grad)`` and a clamp of delta.

``generator`` (optional ``torch.Generator`` on the images' device) fixes the random start.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn


class _PGDBase:
    def __init__(self, model, eps: float, alpha: float, steps: int, random_start: bool = True,
                 generator: Optional[torch.Generator] = None):
        self.model = model
        self.eps, self.alpha, self.steps = float(eps), float(alpha), int(steps)
        self.random_start = bool(random_start)
        self.generator = generator
        self.loss = nn.CrossEntropyLoss()

    def _start(self, images: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _step(self, adv: torch.Tensor, grad: torch.Tensor, images: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def __call__(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        images = images.clone().detach()
        labels = labels.clone().detach()
        adv = images.clone()
        if self.random_start:
            adv = torch.clamp(self._start(images), min=0.0, max=1.0).detach()
        with torch.enable_grad():
            for _ in range(self.steps):
                adv.requires_grad_(True)
                cost = self.loss(self.model(adv), labels)
                grad, = torch.autograd.grad(cost, adv, retain_graph=False, create_graph=False)
                adv = self._step(adv.detach(), grad.detach(), images)
        return adv.detach()


class PGD(_PGDBase):
    """Linf PGD: ``torchattacks.PGD(model, eps, alpha, steps, random_start=True)``."""

    def __init__(self, model, eps: float = 8 / 255, alpha: float = 2 / 255, steps: int = 10,
                 random_start: bool = True, generator: Optional[torch.Generator] = None):
        super().__init__(model, eps, alpha, steps, random_start, generator)

    def _start(self, images):
        u = torch.rand(images.shape, dtype=images.dtype, device=images.device, generator=self.generator)
        return images + (2.0 * u - 1.0) * self.eps

    def _step(self, adv, grad, images):
        adv = adv + self.alpha * grad.sign()
        delta = torch.clamp(adv - images, min=-self.eps, max=self.eps)
        return torch.clamp(images + delta, min=0.0, max=1.0)


class PGDL2(_PGDBase):
    """L2 PGD: ``torchattacks.PGDL2(model, eps, alpha, steps, random_start=True, eps_for_division=1e-10)``."""

    def __init__(self, model, eps: float = 1.0, alpha: float = 0.2, steps: int = 10, random_start: bool = True,
                 eps_for_division: float = 1e-10, generator: Optional[torch.Generator] = None):
        super().__init__(model, eps, alpha, steps, random_start, generator)
        self.eps_for_division = float(eps_for_division)

    @staticmethod
    def _norms(t: torch.Tensor) -> torch.Tensor:
        return t.flatten(1).norm(p=2, dim=1).view(-1, *([1] * (t.dim() - 1)))

    def _start(self, images):
        d = torch.randn(images.shape, dtype=images.dtype, device=images.device, generator=self.generator)
        r = torch.rand((images.shape[0],) + (1,) * (images.dim() - 1), dtype=images.dtype, device=images.device,
                       generator=self.generator)
        return images + d / (self._norms(d) + self.eps_for_division) * r * self.eps

    def _step(self, adv, grad, images):
        grad = grad / (self._norms(grad) + self.eps_for_division)
        adv = adv + self.alpha * grad
        delta = adv - images
        # delta * min(1, eps / ||delta||_2); a zero delta stays zero
        factor = torch.clamp(self.eps / self._norms(delta).clamp_min(1e-30), max=1.0)
        return torch.clamp(images + delta * factor, min=0.0, max=1.0)
