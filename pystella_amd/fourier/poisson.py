"""Fourier-space Poisson solver: ∇²f − m²f = ρ.

Analogue of reference pystella/fourier/poisson.py:33-125.  The solve is
implemented relative to the eigenvalues of a chosen second-difference
stencil (``effective_k(k, dx)``), so solutions are consistent with the
finite-difference Laplacian of the same order.

On the GPU the k-space solve is one fused HIP kernel, in place on the
transform's k-space array (backend/hip.py ``kspace_poisson``); on the
CPU, for float32 transforms and with ``PYSTELLA_KSPACE=0`` it is a chain
of torch ops.

Float32 transforms (complex64 modes) have two forms.  The default,
``precision="promote"``, is the torch chain: the float64 tables promote
the modes to complex128 and the inverse transform runs in complex128.
``precision="native"`` keeps the modes complex64: each stored mode is
widened once to double, the same formula is evaluated in double with the
float64 tables, and each real component of the solution is rounded once
to float32 where it is stored, so a stored mode is within one float32
rounding of the double result computed from the stored input; the
inverse transform is the complex64 one.  On the GPU that is the
``kspace_poisson_c64`` kernel, in place; on the CPU, for a
non-contiguous ``fk`` and with ``PYSTELLA_KSPACE=0`` it is the same
definition in torch ops.
"""

from __future__ import annotations

import os

import numpy as np
import torch

__all__ = ["SpectralPoissonSolver"]


class SpectralPoissonSolver:
    """:arg precision: ``"promote"`` (default) or ``"native"``; they
    differ only on a float32 transform, as the module docstring defines.
    """

    def __init__(self, fft, dk, dx, effective_k, *, precision="promote"):
        if precision not in ("promote", "native"):
            raise ValueError('precision must be "promote" or "native", '
                             f"got {precision!r}")
        self.precision = precision
        self.fft = fft
        self.grid_size = int(np.prod(fft.grid_shape))
        dev = fft.fk.device

        ks = []
        for mu, name in enumerate(("momenta_x", "momenta_y", "momenta_z")):
            kk = fft.sub_k[name].cpu().numpy().astype(int)
            kk_mu = effective_k(dk[mu] * kk.astype(np.float64), dx[mu])
            ks.append(torch.as_tensor(np.asarray(kk_mu, dtype=np.float64),
                                      device=dev))
        # flat per-axis tables for the fused kernel
        self._eig_flat = [k.contiguous() for k in ks]
        shape = (-1, 1, 1), (1, -1, 1), (1, 1, -1)
        # eigenvalues of the per-axis second difference (≤ 0); their sum
        # is −k²_eff
        self.minus_k_squared = sum(k.view(s) for k, s in zip(ks, shape))

    def __call__(self, queue=None, fx=None, rho=None, m_squared=0,
                 allocator=None):
        if fx is None and isinstance(queue, torch.Tensor):
            fx = queue
            queue = None
        rhok = self.fft.dft(rho)
        native = (self.precision == "native"
                  and rhok.dtype == torch.complex64)
        if (rhok.is_cuda and (rhok.dtype == torch.complex128 or native)
                and rhok.is_contiguous()
                and os.environ.get("PYSTELLA_KSPACE") != "0"):
            from pystella_amd.backend import hip
            kernel = hip.kspace_poisson_c64 if native else hip.kspace_poisson
            kernel(rhok, rhok, *self._eig_flat, 1.0 / self.grid_size,
                   m_squared)
            self.fft.idft(rhok, fx)
            return fx
        if native:
            rhok = rhok.to(torch.complex128)
        denom = self.minus_k_squared - m_squared
        sol = torch.where(
            self.minus_k_squared < 0,
            rhok * (1.0 / self.grid_size) / denom,
            torch.zeros((), dtype=rhok.dtype, device=rhok.device))
        if native:
            sol = sol.to(torch.complex64)
        self.fft.idft(sol, fx)
        return fx
