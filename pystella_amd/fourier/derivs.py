"""Spectral-collocation derivatives: FFT → ik-multiply → iFFT.

Analogue of reference pystella/fourier/derivs.py:28-205.  On the GPU
the k-space work of a call is one fused HIP kernel per slice
(backend/hip.py ``kspace_derivs`` / ``kspace_div_accum``); on the CPU,
for float32 transforms and with ``PYSTELLA_KSPACE=0`` it is a chain of
torch ops.  The FFTs are rocFFT (GPU) / FFTW-class (CPU) through
torch.fft.
"""

from __future__ import annotations

import os

import numpy as np
import torch

__all__ = ["SpectralCollocator"]


class SpectralCollocator:
    """Exact spectral derivatives with the same call interface as
    :class:`~pystella_amd.FiniteDifferencer`.

    On the fused GPU path the k-space outputs live in scratch buffers
    owned by the collocator: allocated on first use, one per output of
    the largest subset of ``lap``/``pdx``/``pdy``/``pdz`` ever requested
    in one call, and reused across calls and slices.  That is at most
    4 × 16 B × k-volume of device memory held for the collocator's
    lifetime (4 GiB at 512³).
    """

    def __init__(self, fft, dk):
        self.fft = fft
        self.grid_size = int(np.prod(fft.grid_shape))

        self.k1 = []   # Nyquist- and zero-zeroed (first derivatives)
        self.k2 = []   # full magnitudes (Laplacian)
        for mu, name in enumerate(("momenta_x", "momenta_y", "momenta_z")):
            kk = fft.sub_k[name].cpu().numpy().astype(int)
            kk_mu = dk[mu] * kk.astype(np.float64)
            self.k2.append(torch.as_tensor(
                kk_mu.copy(), device=fft.fk.device))
            kk_mu = kk_mu.copy()
            kk_mu[np.abs(kk) == fft.grid_shape[mu] // 2] = 0.
            kk_mu[kk == 0] = 0.
            self.k1.append(torch.as_tensor(kk_mu, device=fft.fk.device))

        # flat per-axis tables for the fused kernels, and the scratch
        # buffers their outputs go to
        self._k1_flat = [k.contiguous() for k in self.k1]
        self._k2_flat = [k.contiguous() for k in self.k2]
        self._scratch = []

        shape = (-1, 1, 1), (1, -1, 1), (1, 1, -1)
        self.k1 = [k.view(s) for k, s in zip(self.k1, shape)]
        self.k2 = [k.view(s) for k, s in zip(self.k2, shape)]

    def _fused(self):
        """The fused kernels take complex128 on the GPU; everything else
        (CPU, float32 transforms, ``PYSTELLA_KSPACE=0``) runs the torch
        chain."""
        fk = self.fft.fk
        return (isinstance(fk, torch.Tensor) and fk.is_cuda
                and fk.dtype == torch.complex128 and fk.is_contiguous()
                and os.environ.get("PYSTELLA_KSPACE") != "0")

    def _get_scratch(self, n):
        while len(self._scratch) < n:
            self._scratch.append(torch.empty_like(self.fft.fk))
        return self._scratch[:n]

    def _pd(self, fk, mu):
        return 1j * self.k1[mu] * fk

    def _lap(self, fk):
        kmag_sq = (self.k2[0]**2 + self.k2[1]**2 + self.k2[2]**2)
        return -kmag_sq * fk

    def __call__(self, queue=None, fx=None, *, lap=None, pdx=None, pdy=None,
                 pdz=None, grd=None, allocator=None):
        if fx is None and isinstance(queue, torch.Tensor):
            fx = queue
            queue = None
        if grd is not None:
            if isinstance(grd, (tuple, list)):
                pdx, pdy, pdz = grd
            else:
                pdx = grd[..., 0, :, :, :]
                pdy = grd[..., 1, :, :, :]
                pdz = grd[..., 2, :, :, :]

        from itertools import product
        slices = list(product(*[range(n) for n in fx.shape[:-3]]))
        inv_n = 1.0 / self.grid_size

        if self._fused():
            from pystella_amd.backend import hip
            outs = {name: out for name, out in (
                ("lap", lap), ("pdx", pdx), ("pdy", pdy), ("pdz", pdz))
                if out is not None}
            if not outs:
                return
            bufs = dict(zip(outs, self._get_scratch(len(outs))))
            for s in slices:
                fk = self.fft.dft(fx[s])
                hip.kspace_derivs(fk, bufs, self._k1_flat, self._k2_flat,
                                  inv_n)
                for name, out in outs.items():
                    self.fft.idft(bufs[name], out[s])
            return

        for s in slices:
            fk = self.fft.dft(fx[s]).clone() * inv_n
            if lap is not None:
                self.fft.idft(self._lap(fk), lap[s])
            if pdx is not None:
                self.fft.idft(self._pd(fk, 0), pdx[s])
            if pdy is not None:
                self.fft.idft(self._pd(fk, 1), pdy[s])
            if pdz is not None:
                self.fft.idft(self._pd(fk, 2), pdz[s])

    def divergence(self, queue=None, vec=None, div=None, allocator=None):
        if vec is None and isinstance(queue, torch.Tensor):
            vec = queue
            queue = None
        from itertools import product
        slices = list(product(*[range(n) for n in vec.shape[:-4]]))
        inv_n = 1.0 / self.grid_size

        if self._fused():
            from pystella_amd.backend import hip
            div_k, = self._get_scratch(1)
            for s in slices:
                for mu in range(3):
                    fk = self.fft.dft(vec[s][mu])
                    hip.kspace_div_accum(fk, div_k, self._k1_flat[mu], mu,
                                         inv_n, accumulate=mu > 0)
                self.fft.idft(div_k, div[s])
            return

        for s in slices:
            div_k = None
            for mu in range(3):
                fk = self.fft.dft(vec[s][mu])
                term = self._pd(fk, mu) * inv_n
                div_k = term if div_k is None else div_k + term
            self.fft.idft(div_k, div[s])
