"""Feature standardisation (MLlib StandardScaler, and the useFeatureScaling
step of GeneralizedLinearAlgorithm built on it).

``StandardScaler(with_mean, with_std).fit(stats)`` turns an ``ops.ColStats``
into a ``ScalerModel``; the model rescales dense or CSR data in place with
the scale kernels (ops.scale_ / ops.scale_csr_) and maps weights trained on
the scaled features back to the raw ones."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops


@dataclass
class ScalerModel:
    """``mean`` and ``factor`` are fp32 [d]; x -> (x - mean) * factor.
    ``mean`` is zeros unless ``with_mean``."""
    mean: torch.Tensor
    factor: torch.Tensor
    with_mean: bool = False
    with_std: bool = True

    def _on(self, device):
        return self.mean.to(device), self.factor.to(device)

    def transform_(self, X: torch.Tensor) -> None:
        """Rescale the dense rows X [n, d] in place."""
        if X.shape[1] != self.factor.numel():
            raise ValueError(f"X must be [n, {self.factor.numel()}], got "
                             f"{tuple(X.shape)}")
        mean, factor = self._on(X.device)
        ops.scale_(X, mean, factor, with_mean=self.with_mean)

    def transform_csr_(self, indices: torch.Tensor, values: torch.Tensor
                       ) -> None:
        """Rescale CSR values in place. Centring would fill the matrix, so
        ``with_mean`` raises, as MLlib's StandardScalerModel does."""
        if self.with_mean:
            raise ValueError("cannot centre sparse data: with_mean needs a "
                             "dense matrix")
        ops.scale_csr_(indices, values, self._on(values.device)[1])

    def unscale_weights(self, W: torch.Tensor) -> torch.Tensor:
        """The model for RAW features of weights W [..., d] trained on the
        scaled ones: x_scaled . w == x_raw . (w * factor). fp64 product,
        returned in fp32."""
        if self.with_mean:
            raise ValueError("with_mean shifts the score by -mean . (w * "
                             "factor): that needs an intercept, which this "
                             "model family does not have")
        return (W.double() * self.factor.to(W.device).double()).float()


class StandardScaler:
    """fit(stats) -> ScalerModel. factor = fp32(1 / std) with the unbiased
    std, and 0 where the column is constant (variance == 0 or min == max,
    MLlib's rule); all ones without ``with_std``. The defaults are MLlib's:
    unit variance, no centring."""

    def __init__(self, with_mean: bool = False, with_std: bool = True):
        self.with_mean = bool(with_mean)
        self.with_std = bool(with_std)

    def fit(self, stats: "ops.ColStats") -> ScalerModel:
        if self.with_std:
            var = stats.variance
            const = (var == 0) | (stats.min == stats.max)
            safe = torch.where(const, torch.ones_like(var), var)
            factor = torch.where(const, torch.zeros_like(var),
                                 1.0 / safe.sqrt()).float()
        else:
            factor = torch.ones_like(stats.mean, dtype=torch.float32)
        mean = (stats.mean.float() if self.with_mean
                else torch.zeros_like(factor))
        return ScalerModel(mean, factor, self.with_mean, self.with_std)
