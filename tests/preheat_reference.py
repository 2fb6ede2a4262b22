"""Independent numpy reference for the GPU kernel tests.

Plain numpy, float64 throughout, sharing no code with the framework's
stepper, stencil, reduction or expansion machinery: the finite-
difference coefficients and the RK tableau are written out literally
from the published tables (standard centred-difference tables of
truncation order 2h; Carpenter & Kennedy 1994 for the 2N-storage
RK54), and the physics is the conformal-FLRW Klein-Gordon + Friedmann
system of ``tests/test_crosscheck.py`` with the same potential and
constants.

``tests/test_preheat_reference.py`` pins this module against the CPU
host loop for every halo order; the GPU matrices
(``tests/test_stage_variants.py``, ``tests/test_derivs_edges.py``)
compare the HIP kernels against it.
"""

import numpy as np

MPHI, MPL, GSQ = 1.2e-6, 1.0, 2.5e-7

# centred second-difference coefficients, offset 0..h
LAP_COEFS = {
    1: (-2., 1.),
    2: (-30. / 12, 16. / 12, -1. / 12),
    3: (-490. / 180, 270. / 180, -27. / 180, 2. / 180),
    4: (-14350. / 5040, 8064. / 5040, -1008. / 5040, 128. / 5040,
        -9. / 5040),
}

# centred first-difference coefficients, offset 1..h
GRAD_COEFS = {
    1: (1. / 2,),
    2: (8. / 12, -1. / 12),
    3: (45. / 60, -9. / 60, 1. / 60),
    4: (672. / 840, -168. / 840, 32. / 840, -3. / 840),
}

# Carpenter & Kennedy (1994) five-stage fourth-order 2N-storage scheme
RK54_A = (
    0.,
    -567301805773. / 1357537059087.,
    -2404267990393. / 2016746695238.,
    -3550918686646. / 2091501179385.,
    -1275806237668. / 842570457699.,
)
RK54_B = (
    1432997174477. / 9575080441755.,
    5161836677717. / 13612068292357.,
    1720146321549. / 2090206949498.,
    3134564353537. / 4481467310338.,
    2277821191437. / 14882151754819.,
)


def potential(f):
    """The two-field potential of tests/test_crosscheck.py (works on
    numpy arrays and on the framework's symbolic fields alike)."""
    phi, chi = f[0], f[1]
    return (MPHI**2 / 2 * phi**2 + GSQ / 2 * phi**2 * chi**2) / MPHI**2


def _dpotential(f):
    phi, chi = f[0], f[1]
    return np.stack([
        (MPHI**2 * phi + GSQ * phi * chi**2) / MPHI**2,
        (GSQ * phi**2 * chi) / MPHI**2,
    ])


def initial_data(grid):
    """The rng(42) initial realization of
    test_crosscheck.test_independent_numpy_integration on ``grid``."""
    rng = np.random.default_rng(42)
    f0 = np.stack([0.193 + 1e-3 * rng.standard_normal(grid),
                   1e-3 * rng.standard_normal(grid)])
    df0 = np.stack([-0.142 + 1e-3 * rng.standard_normal(grid),
                    1e-3 * rng.standard_normal(grid)])
    return f0, df0


def periodic_laplacian(u, h, dx):
    """Order-2h centred Laplacian of the periodic array ``u`` (last
    three axes are the grid)."""
    c = LAP_COEFS[h]
    out = np.zeros(u.shape, dtype=np.float64)
    for mu in range(3):
        axis = u.ndim - 3 + mu
        acc = c[0] * u
        for s in range(1, h + 1):
            acc = acc + c[s] * (np.roll(u, s, axis) + np.roll(u, -s, axis))
        out += acc / dx[mu] / dx[mu]
    return out


def preheat_reference(f0, df0, dx, dt, steps, h, mpl=MPL):
    """Integrate ``steps`` RK54 steps of two-field preheating from the
    unpadded periodic initial data ``f0``, ``df0`` (shape (2, nx, ny,
    nz)) with the order-2h Laplacian.

    Returns ``(f, dfdt, a, adot, energies)`` where ``energies`` is the
    list of ``(E, P)`` pairs fed to the Friedmann update at every
    stage: entry 0 is the energy of the initial state (a=1), entry
    ``5*n + s`` that of the input state of stage ``s`` of step ``n``,
    and the last entry that of the final state.
    """
    f = np.array(f0, dtype=np.float64)
    dfdt = np.array(df0, dtype=np.float64)

    def energy(f, dfdt, lap_f, a):
        kin = sum(np.mean(dfdt[i]**2) / 2 / a**2 for i in range(2))
        pot = np.mean(potential(f))
        grad = sum(np.mean(-f[i] * lap_f[i]) / 2 / a**2 for i in range(2))
        return kin + pot + grad, kin - grad / 3 - pot

    lap_f = periodic_laplacian(f, h, dx)
    a = 1.0
    E, P = energy(f, dfdt, lap_f, a)
    adot = np.sqrt(8 * np.pi * a**2 / 3 / mpl**2 * E) * a
    energies = [(E, P)]

    k_f = np.zeros_like(f)
    k_df = np.zeros_like(dfdt)
    k_a = 0.0
    k_ad = 0.0
    for _ in range(steps):
        for s in range(5):
            hubble = adot / a
            rhs_df = lap_f - 2 * hubble * dfdt - a**2 * _dpotential(f)
            k_f = RK54_A[s] * k_f + dt * dfdt
            k_df = RK54_A[s] * k_df + dt * rhs_df
            f = f + RK54_B[s] * k_f
            dfdt = dfdt + RK54_B[s] * k_df
            # Friedmann update with the energy of the stage's input state
            rhs_ad = 4 * np.pi * a**2 / 3 / mpl**2 * (E - 3 * P) * a
            k_a = RK54_A[s] * k_a + dt * adot
            k_ad = RK54_A[s] * k_ad + dt * rhs_ad
            a = a + RK54_B[s] * k_a
            adot = adot + RK54_B[s] * k_ad
            lap_f = periodic_laplacian(f, h, dx)
            E, P = energy(f, dfdt, lap_f, a)
            energies.append((E, P))
    return f, dfdt, a, adot, energies


def fd_reference(fpad, h, dx):
    """``(lap, pdx, pdy, pdz)`` of the halo-padded array ``fpad`` (last
    three axes padded by ``h``) by direct slicing; float64 accumulation
    whatever the input dtype."""
    fp = np.asarray(fpad).astype(np.float64)
    n = [fp.shape[fp.ndim - 3 + mu] - 2 * h for mu in range(3)]

    def shifted(mu, s):
        sl = [slice(None)] * fp.ndim
        for nu in range(3):
            d = s if nu == mu else 0
            sl[fp.ndim - 3 + nu] = slice(h + d, h + d + n[nu])
        return fp[tuple(sl)]

    lc, gc = LAP_COEFS[h], GRAD_COEFS[h]
    center = shifted(0, 0)
    lap = np.zeros(center.shape, dtype=np.float64)
    pds = []
    for mu in range(3):
        acc = lc[0] * center
        pd = np.zeros(center.shape, dtype=np.float64)
        for s in range(1, h + 1):
            up, dn = shifted(mu, s), shifted(mu, -s)
            acc = acc + lc[s] * (up + dn)
            pd = pd + gc[s - 1] * (up - dn)
        lap += acc / dx[mu] / dx[mu]
        pds.append(pd / dx[mu])
    return lap, pds[0], pds[1], pds[2]
