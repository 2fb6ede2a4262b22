"""Counter-based random modes for :class:`RayleighGenerator`
(``rng="philox"``): the definition that the HIP kernel
``backend/hip.py:rayleigh_modes`` implements, here in vectorised numpy
for CPU transforms and as the kernel's oracle.

A mode's random numbers depend only on (seed, draw, global mode index):
Philox4x32-10 (Salmon et al., SC'11) with key
``(seed & 0xffffffff, seed >> 32)`` and counter
``(cx, cy, gz, 2*draw + j)``, where ``(cx, cy)`` is the canonical
x/y index.  On the self-conjugate planes of a real transform
(``gz == 0`` and, for even Nz, ``gz == Nz/2``) a mode and its partner
``((Nx-gx) % Nx, (Ny-gy) % Ny)`` share one canonical index, chosen by
the ``keep`` rule of :func:`~pystella_amd.fourier.rayleigh.make_hermitian`;
the other of the two stores the complex conjugate, and a mode that is
its own partner stores a zero imaginary part.  Every layout therefore
draws the same, exactly Hermitian, realisation.
"""

from __future__ import annotations

import numpy as np

__all__ = ["philox4x32", "philox_uniforms", "global_indices",
           "canonical_indices", "mode_values", "modes", "modes_WKB",
           "check_seed", "check_draw"]

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = 0x9E3779B9
_W1 = 0xBB67AE85
_MASK = np.uint64(0xffffffff)
_S32 = np.uint64(32)
RSQRT2 = float(np.sqrt(0.5))


def check_seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2**64:
        raise ValueError(f"seed must lie in [0, 2**64), got {seed}")
    return seed


def check_draw(draw):
    draw = int(draw)
    if not 0 <= draw < 2**30:
        raise ValueError(f"draw must lie in [0, 2**30), got {draw}")
    return draw


def philox4x32(counter, key):
    """Philox4x32-10.  ``counter`` is four and ``key`` two arrays (or
    scalars) of 32-bit words, broadcast against each other; returns the
    four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(
        *[np.asarray(c, dtype=np.uint64) & _MASK for c in counter])
    k0, k1 = (int(k) & 0xffffffff for k in key)
    for rnd in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK,
                          (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0 = (k0 + _W0) & 0xffffffff
        k1 = (k1 + _W1) & 0xffffffff
    return c0, c1, c2, c3


def philox_uniforms(seed, draw, j, cx, cy, gz):
    """``(u_amp, u_phs)`` of the modes with canonical index ``(cx, cy)``
    and global z index ``gz``: exact doubles in (0, 1]."""
    seed = check_seed(seed)
    draw = check_draw(draw)
    w0, w1, w2, w3 = philox4x32(
        (cx, cy, gz, 2 * draw + int(j)), (seed & 0xffffffff, seed >> 32))
    sh = np.uint64(11)
    one = np.uint64(1)
    u_amp = ((((w0 >> sh) << _S32) | w1) + one).astype(np.float64) * 2.0**-53
    u_phs = ((((w2 >> sh) << _S32) | w3) + one).astype(np.float64) * 2.0**-53
    return u_amp, u_phs


def global_indices(fft):
    """This rank's global mode indices along each axis: ``fft.sub_k``
    mod ``grid_shape`` (the Nyquist mode, stored as +N/2, is itself)."""
    return tuple(
        np.asarray(fft.sub_k[name].cpu()).astype(np.int64) % int(n)
        for name, n in zip(("momenta_x", "momenta_y", "momenta_z"),
                           fft.grid_shape))


def canonical_indices(gidx, grid_shape, is_real):
    """``(cx, cy, gz, conj, self_conj)`` broadcast to the k-shape."""
    gx = gidx[0][:, None, None]
    gy = gidx[1][None, :, None]
    gz = gidx[2][None, None, :]
    shape = (len(gidx[0]), len(gidx[1]), len(gidx[2]))
    gx, gy, gz = (np.broadcast_to(g, shape) for g in (gx, gy, gz))
    if not is_real:
        no = np.zeros(shape, dtype=bool)
        return gx, gy, gz, no, no
    Nx, Ny, Nz = grid_shape
    plane = gz == 0
    if Nz % 2 == 0:
        plane = plane | (gz == Nz // 2)
    px = (Nx - gx) % Nx
    py = (Ny - gy) % Ny
    keep = (gx < px) | ((gx == px) & (gy <= py))
    conj = plane & ~keep
    self_conj = plane & (px == gx) & (py == gy)
    return (np.where(conj, px, gx), np.where(conj, py, gy), gz, conj,
            self_conj)


def _sincos_2pi(u):
    """``(cos 2πu, sin 2πu)`` for u in (0, 1], reduced exactly to
    |angle| <= π/4 first (as ``sincospi`` does on the device)."""
    v = 2.0 * u
    q = np.rint(2.0 * v)
    r = np.pi * (v - 0.5 * q)
    c, s = np.cos(r), np.sin(r)
    q = q.astype(np.int64) % 4
    cos = np.choose(q, [c, -s, -c, s])
    sin = np.choose(q, [s, c, -s, -c])
    return cos, sin


def mode_values(seed, draw, j, cx, cy, gz, sqrt_power, random=True):
    """``z = amp · sqrt_power · exp(2πi u_phs)`` as (real, imag)."""
    u_amp, u_phs = philox_uniforms(seed, draw, j, cx, cy, gz)
    cos, sin = _sincos_2pi(u_phs)
    a = (np.sqrt(-np.log(u_amp)) * sqrt_power) if random \
        else 1.0 * sqrt_power
    return a * cos, a * sin


def _finish(re, im, conj, self_conj):
    out = np.empty(re.shape, dtype=np.complex128)
    out.real = re
    out.imag = np.where(self_conj, 0.0, np.where(conj, -im, im))
    return out


def modes(seed, draw, gidx, grid_shape, is_real, sqrt_power, random=True):
    """The ``generate`` modes of one rank, complex128."""
    cx, cy, gz, conj, self_conj = canonical_indices(gidx, grid_shape,
                                                    is_real)
    re, im = mode_values(seed, draw, 0, cx, cy, gz, sqrt_power, random)
    return _finish(re, im, conj, self_conj)


def modes_WKB(seed, draw, gidx, grid_shape, is_real, sqrt_power, omega,
              hubble, random=True):
    """The ``generate_WKB`` pair ``(fk, dfk)`` of one rank, complex128:
    ``fk = (L + R)/√2``, ``dfk = iω(L − R)/√2 − H·fk``."""
    cx, cy, gz, conj, self_conj = canonical_indices(gidx, grid_shape,
                                                    is_real)
    lr, li = mode_values(seed, draw, 0, cx, cy, gz, sqrt_power, random)
    rr, ri = mode_values(seed, draw, 1, cx, cy, gz, sqrt_power, random)
    fr, fi = (lr + rr) * RSQRT2, (li + ri) * RSQRT2
    dr, di = (lr - rr) * RSQRT2, (li - ri) * RSQRT2
    hubble = float(hubble)
    gr = -(omega * di) - hubble * fr
    gi = omega * dr - hubble * fi
    return (_finish(fr, fi, conj, self_conj),
            _finish(gr, gi, conj, self_conj))
