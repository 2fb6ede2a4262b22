"""Independent numpy reference for the GPU kernel tests.

Plain numpy, float64 throughout, sharing no code with the framework's
stepper, stencil, reduction or expansion machinery: the finite-
difference coefficients and the RK tableau are written out literally
from the published tables (standard centred-difference tables of
truncation order 2h; Carpenter & Kennedy 1994 for the 2N-storage
RK54), and the physics is the conformal-FLRW Klein-Gordon + Friedmann
system of ``tests/test_crosscheck.py`` with the same potential and
constants.  ``gw_reference`` adds the six tensor-perturbation
components sourced by the scalar gradients, with the index pairs
written out literally.

``tests/test_preheat_reference.py`` pins this module against the CPU
host loop for every halo order; the GPU matrices
(``tests/test_stage_variants.py``, ``tests/test_stage_gw_variants.py``,
``tests/test_derivs_edges.py``) compare the HIP kernels against it.
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


def periodic_gradient(u, h, dx):
    """Order-2h centred first differences ``(d/dx, d/dy, d/dz)`` of the
    periodic array ``u`` (last three axes are the grid)."""
    c = GRAD_COEFS[h]
    out = []
    for mu in range(3):
        axis = u.ndim - 3 + mu
        acc = np.zeros(u.shape, dtype=np.float64)
        for s in range(1, h + 1):
            acc = acc + c[s - 1] * (np.roll(u, -s, axis) - np.roll(u, s, axis))
        out.append(acc / dx[mu])
    return out


def initial_tensor_data(grid):
    """Seeded nonzero ``h_ij`` and ``dh_ij/dt`` (shape (6,) + grid), so
    that the Laplacian and friction terms of the tensor equation are
    exercised and not only its source."""
    rng = np.random.default_rng(4242)
    h0 = 1e-3 * rng.standard_normal((6,) + tuple(grid))
    dh0 = 1e-3 * rng.standard_normal((6,) + tuple(grid))
    return h0, dh0


def gw_reference(f0, df0, h0, dh0, dx, dt, steps, h, A=RK54_A, B=RK54_B,
                 mpl=MPL, _mutant=None):
    """:func:`preheat_reference` for any 2N-storage tableau ``(A, B)``,
    plus six tensor-perturbation components

        h_ij'' = lap h_ij - 2 H h_ij' + 16 pi sum_fld d_i f d_j f

    stored in the order (xx, xy, xz, yy, yz, zz), with order-2h
    periodic gradients and the source evaluated on each stage's input
    state.  The tensor sector does not back-react: the scalar and
    Friedmann arithmetic is that of :func:`preheat_reference`,
    operation for operation.  ``h0 = dh0 = None`` integrates the scalar
    system alone and returns ``None`` for the tensor arrays.

    Returns ``(f, dfdt, hij, dhijdt, a, adot, energies)``; ``energies``
    is indexed as in :func:`preheat_reference` with ``len(A)`` stages
    per step (entry ``len(A)*n + s`` is the input of stage ``s`` of
    step ``n``).

    RK54 keeps the literal table above.  For the other tableaus the
    tests pass the framework's ``Stepper._A`` and ``Stepper._B``: the
    *values* of those tables are covered by the convergence test in
    ``tests/test_step.py``; this comparison covers their *use* by the
    stage kernels.

    ``_mutant`` is private to the sensitivity test of
    ``tests/test_preheat_reference.py``, which checks that each
    deliberately wrong variant of this integration lies far outside the
    tolerances the GPU matrix holds the kernels to.
    """
    assert _mutant in (None, "no_source", "swap_source", "grad_z_off",
                       "no_friction", "stale_k", "skip_site")
    ns = len(A)
    f = np.array(f0, dtype=np.float64)
    dfdt = np.array(df0, dtype=np.float64)
    gw = h0 is not None
    if gw:
        hij = np.array(h0, dtype=np.float64)
        dhij = np.array(dh0, dtype=np.float64)
        k_h = np.zeros_like(hij)
        k_dh = np.zeros_like(dhij)
    else:
        hij = dhij = None

    def energy(f, dfdt, lap_f, a):
        kin = sum(np.mean(dfdt[i]**2) / 2 / a**2 for i in range(2))
        pot = np.mean(potential(f))
        grad = sum(np.mean(-f[i] * lap_f[i]) / 2 / a**2 for i in range(2))
        return kin + pot + grad, kin - grad / 3 - pot

    def source(f):
        fx, fy, fz = periodic_gradient(f, h, dx)
        if _mutant == "grad_z_off":
            fz = np.roll(fz, 1, axis=-1)
        s = 16 * np.pi * np.stack([
            fx[0] * fx[0] + fx[1] * fx[1],      # xx
            fx[0] * fy[0] + fx[1] * fy[1],      # xy
            fx[0] * fz[0] + fx[1] * fz[1],      # xz
            fy[0] * fy[0] + fy[1] * fy[1],      # yy
            fy[0] * fz[0] + fy[1] * fz[1],      # yz
            fz[0] * fz[0] + fz[1] * fz[1],      # zz
        ])
        if _mutant == "no_source":
            s = 0 * s
        if _mutant == "swap_source":
            s = s[[0, 2, 1, 3, 4, 5]]
        return s

    lap_f = periodic_laplacian(f, h, dx)
    a = 1.0
    E, P = energy(f, dfdt, lap_f, a)
    adot = np.sqrt(8 * np.pi * a**2 / 3 / mpl**2 * E) * a
    energies = [(E, P)]

    k_f = np.zeros_like(f)
    k_df = np.zeros_like(dfdt)
    k_a = 0.0
    k_ad = 0.0
    for n in range(steps):
        for s in range(ns):
            hubble = adot / a
            if gw:
                friction = 0 if _mutant == "no_friction" else 2 * hubble
                rhs_dh = (periodic_laplacian(hij, h, dx) - friction * dhij
                          + source(f))
                # a stale k survives when the last stage's k store is
                # wrongly elided and stage 0 does not multiply it by zero
                A_h = 1. if (_mutant == "stale_k" and n > 0 and s == 0) \
                    else A[s]
                k_h = A_h * k_h + dt * dhij
                k_dh = A[s] * k_dh + dt * rhs_dh
                h_new = hij + B[s] * k_h
                dh_new = dhij + B[s] * k_dh
                if _mutant == "skip_site" and n == steps - 1 and s == ns - 1:
                    site = (4, 37, 10, 63)
                    h_new[site] = hij[site]
                    dh_new[site] = dhij[site]
                hij, dhij = h_new, dh_new
            rhs_df = lap_f - 2 * hubble * dfdt - a**2 * _dpotential(f)
            k_f = A[s] * k_f + dt * dfdt
            k_df = A[s] * k_df + dt * rhs_df
            f = f + B[s] * k_f
            dfdt = dfdt + B[s] * k_df
            # Friedmann update with the energy of the stage's input state
            rhs_ad = 4 * np.pi * a**2 / 3 / mpl**2 * (E - 3 * P) * a
            k_a = A[s] * k_a + dt * adot
            k_ad = A[s] * k_ad + dt * rhs_ad
            a = a + B[s] * k_a
            adot = adot + B[s] * k_ad
            lap_f = periodic_laplacian(f, h, dx)
            E, P = energy(f, dfdt, lap_f, a)
            energies.append((E, P))
    return f, dfdt, hij, dhij, a, adot, energies


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
