"""
`Noise`: smooth random field initialiser (reference: phi/field/_noise.py:9-60), e.g. `CenteredGrid(Noise(vector='x,y'), PERIODIC, x=64, y=64)`
in Burgers.ipynb. Set-up work, not a kernel: the spectrum is shaped with `torch.fft` on the field's device, seeded by torch's generator
(`torch.manual_seed`). The random stream is torch's, so values never match PhiML's for the same seed; the statistics do.
"""
from typing import Optional, Sequence

import torch


class Noise:
    """ Random fluctuations of physical size `scale` whose spectrum falls off like (1/k^2)^smoothness. Each sampling draws a new field.

    Args:
        scale: size of the fluctuations in physical units
        smoothness: how quickly high frequencies die out
        vector: item names of a vector axis, e.g. 'x,y' (a centred vector field); None for a scalar
        batch: number of independent batch entries (None: not batched)
    """

    def __init__(self, scale: float = 10., smoothness: float = 1.0, vector: Optional[str] = None, batch: Optional[int] = None):
        self.scale = float(scale)
        self.smoothness = float(smoothness)
        self.vector = [n.strip() for n in vector.split(',')] if isinstance(vector, str) else (list(vector) if vector is not None else None)
        self.batch = batch

    def grid_sample(self, shape: Sequence[int], size: Sequence[float], channels: int, device, dtype, batch: int = 1) -> torch.Tensor:
        """ (batch, channels, *shape) noise on a grid of `shape` cells spanning `size` (phi/field/_noise.py:37-60):
        complex normal noise times (1/k^2)^smoothness with k = fftfreq(n, size) * n * scale, frequencies with k^2 <= 0.1 removed,
        real part of the inverse FFT, divided by its std and made zero-mean over all non-batch dims (the vector axis included). """
        shape = tuple(int(n) for n in shape)
        full = (batch, channels) + shape
        re = torch.randn(full, dtype=torch.float64, device=device)
        rnd = torch.complex(re, torch.randn(full, dtype=torch.float64, device=device))     # normal + 1j * normal
        k2 = torch.zeros(shape, dtype=torch.float64, device=device)
        for a, (n, sz) in enumerate(zip(shape, size)):
            k = torch.fft.fftfreq(n, d=float(sz), dtype=torch.float64, device=device) * n * self.scale
            k2 = k2 + (k ** 2).reshape([n if b == a else 1 for b in range(len(shape))])
        weight_mask = (k2 > 0.1).to(torch.float64)
        inv_k2 = torch.where(k2 == 0, torch.zeros_like(k2), 1.0 / torch.where(k2 == 0, torch.ones_like(k2), k2))   # divide_no_nan
        fft = rnd * (inv_k2 ** self.smoothness * weight_mask)
        array = torch.fft.ifftn(fft, dim=tuple(range(2, 2 + len(shape)))).real
        flat = array.reshape(batch, -1)
        array = array / flat.std(dim=1, unbiased=False).reshape(batch, *([1] * (array.dim() - 1)))
        array = array - array.reshape(batch, -1).mean(dim=1).reshape(batch, *([1] * (array.dim() - 1)))
        return array.to(dtype)

    def __repr__(self):
        return f"Noise(scale={self.scale}, smoothness={self.smoothness}, vector={self.vector}, batch={self.batch})"
