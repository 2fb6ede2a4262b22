"""Spectral-collocation derivatives: FFT → ik-multiply → iFFT.

Analogue of reference pystella/fourier/derivs.py:28-205.  On the GPU
the k-space work of a call is one fused HIP kernel per slice
(backend/hip.py ``kspace_derivs`` / ``kspace_div_accum``); on the CPU,
for float32 transforms and with ``PYSTELLA_KSPACE=0`` it is a chain of
torch ops.  The FFTs are rocFFT (GPU) / FFTW-class (CPU) through
torch.fft.

Float32 transforms (complex64 modes) have two forms.  The default,
``precision="promote"``, is the torch chain: the float64 tables promote
the modes to complex128 and every inverse transform runs in complex128.
``precision="native"`` keeps the modes complex64 from ``fft.dft`` to
``fft.idft``: each stored mode is widened once to double, the same
formulas are evaluated in double in the same order with the float64
tables, and each real component of a result is rounded once to float32
where it is stored, so a stored derivative or Laplacian mode is within
one float32 rounding of the double result computed from the stored
input.  The divergence keeps its three accumulating steps: after each,
the stored ``div_k`` is one float32 rounding of the previously stored
``div_k``, widened, plus the double term.  The inverse transform is the
complex64 one.  On the GPU that is the ``kspace_derivs_c64`` /
``kspace_div_accum_c64`` kernels; on the CPU, for a non-contiguous
``fk`` and with ``PYSTELLA_KSPACE=0`` it is the same definition in torch
ops.
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
    lifetime (4 GiB at 512³); 4 × 8 B × k-volume for complex64 modes
    under ``precision="native"``.

    :arg precision: ``"promote"`` (default) or ``"native"``; they differ
        only on a float32 transform, as the module docstring defines.
    """

    def __init__(self, fft, dk, *, precision="promote"):
        if precision not in ("promote", "native"):
            raise ValueError('precision must be "promote" or "native", '
                             f"got {precision!r}")
        self.precision = precision
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
        """The fused kernels take complex128 on the GPU, and complex64
        under ``precision="native"``; everything else (CPU, float32
        transforms otherwise, ``PYSTELLA_KSPACE=0``) runs torch ops."""
        fk = self.fft.fk
        return (isinstance(fk, torch.Tensor) and fk.is_cuda
                and (fk.dtype == torch.complex128 or self._native())
                and fk.is_contiguous()
                and os.environ.get("PYSTELLA_KSPACE") != "0")

    def _native(self):
        """complex64 modes that stay complex64."""
        return (self.precision == "native"
                and self.fft.fk.dtype == torch.complex64)

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
            kernel = (hip.kspace_derivs_c64 if self._native()
                      else hip.kspace_derivs)
            bufs = dict(zip(outs, self._get_scratch(len(outs))))
            for s in slices:
                fk = self.fft.dft(fx[s])
                kernel(fk, bufs, self._k1_flat, self._k2_flat, inv_n)
                for name, out in outs.items():
                    self.fft.idft(bufs[name], out[s])
            return

        if self._native():
            def c64(x):
                return x.to(torch.complex64)
            for s in slices:
                fk = self.fft.dft(fx[s]).to(torch.complex128) * inv_n
                if lap is not None:
                    self.fft.idft(c64(self._lap(fk)), lap[s])
                if pdx is not None:
                    self.fft.idft(c64(self._pd(fk, 0)), pdx[s])
                if pdy is not None:
                    self.fft.idft(c64(self._pd(fk, 1)), pdy[s])
                if pdz is not None:
                    self.fft.idft(c64(self._pd(fk, 2)), pdz[s])
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
            kernel = (hip.kspace_div_accum_c64 if self._native()
                      else hip.kspace_div_accum)
            div_k, = self._get_scratch(1)
            for s in slices:
                for mu in range(3):
                    fk = self.fft.dft(vec[s][mu])
                    kernel(fk, div_k, self._k1_flat[mu], mu, inv_n,
                           accumulate=mu > 0)
                self.fft.idft(div_k, div[s])
            return

        if self._native():
            # rounded after each term, as the stored div_k of the kernels
            for s in slices:
                div_k = None
                for mu in range(3):
                    fk = self.fft.dft(vec[s][mu]).to(torch.complex128)
                    term = self._pd(fk, mu) * inv_n
                    if div_k is not None:
                        term = div_k.to(torch.complex128) + term
                    div_k = term.to(torch.complex64)
                self.fft.idft(div_k, div[s])
            return

        for s in slices:
            div_k = None
            for mu in range(3):
                fk = self.fft.dft(vec[s][mu])
                term = self._pd(fk, mu) * inv_n
                div_k = term if div_k is None else div_k + term
            self.fft.idft(div_k, div[s])
