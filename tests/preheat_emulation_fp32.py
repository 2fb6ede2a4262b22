"""float32 emulation of the mixed-precision fused stage kernels, in plain
numpy, sharing no code with the framework.

The precision model is the one the float32 ``JitLapStage`` /
``JitLapReduction`` kernels implement: the fields, their ``.dot``
companions and the RK k-arrays are float32; every per-site expression
(Laplacian, right-hand side, 2N update, the field part of each
reducer's per-site value) is evaluated in float32 with float32
coefficients, and with the scale factor and Hubble rate narrowed to
float32 once per stage; each reducer's per-site value is widened once,
where the float64 scale factor enters it, and summed in float64; the
(a, adot) Friedmann ODE is integrated in float64.  (A scale factor
narrowed to float32 inside the reducers would be off by up to 6e-8
relative, the kinetic and gradient energies by twice that, the same
for every site, so it does not average out: it is the one place where
the run-time scalars must stay float64.)

Two Laplacian forms are provided.  ``"plain"`` is
``c0*f0 + sum_s c_s (f[+s] + f[-s])``; its float32 coefficients do not
sum to zero, so the field's mean leaks into the result.
``"difference"`` is ``sum_s c_s ((f[+s] - f0) + (f[-s] - f0))``, in
which the mean cancels exactly before any coefficient is applied; it
is the form the float32 kernels use.

The deviation of this emulation from ``tests/preheat_reference.py``
(float64) is what float32 storage and arithmetic cost on a given
problem; the float32 GPU tests hold the kernels to four times that
deviation (``tests/test_stage_fp32.py``), and
``tests/test_stage_fp32_cpu.py`` pins the emulation itself to a quarter
of those tolerances.
"""

import numpy as np

from tests.preheat_reference import (
    GSQ, LAP_COEFS, MPHI, MPL, RK54_A, RK54_B)

F32 = np.float32

# What the float32 kernel tests allow against preheat_reference on the
# zero-mean data of ``zero_mean_data`` (grid (72,11,80), two RK54
# steps): four times this emulation's own deviation for h = 1..4
# (f 6.2e-8, dfdt 4.9e-7, a 3.5e-11, adot 7.5e-9, E 2.0e-8, P 2.4e-8;
# the factor covers FMA contraction and another summation order).  f
# and dfdt are max abs; a, adot and E are relative; P is relative to
# max(|P|, |E|).  E and P are compared where the kernel tests compare
# them: the seed energy and the pair fed to each step's last stage.
TOL_FP32 = {"f": 2.5e-7, "dfdt": 2e-6, "a": 1.5e-10, "adot": 3e-8,
            "E": 8e-8, "P": 1e-7}


def zero_mean_data(grid):
    """Zero-mean initial data, rounded to float32 (so that a float64
    integration of the same values differs by arithmetic alone).
    Without the inflaton's 0.193 mean a stencil fault stands out above
    float32 rounding."""
    rng = np.random.default_rng(42)
    f0 = (0.05 * rng.standard_normal((2,) + tuple(grid))).astype(F32)
    df0 = (0.05 * rng.standard_normal((2,) + tuple(grid))).astype(F32)
    return f0, df0


def deviations(got, ref, steps):
    """{quantity: deviation} of ``(f, dfdt, a, adot, energies)`` from
    the reference's, in the measures of ``TOL_FP32``.  ``energies`` of
    ``got`` may be a dict {index: (E, P)} of the entries it has."""
    f, dfdt, a, adot, en = got
    fr, dfr, ar, adr, enr = ref
    if not isinstance(en, dict):
        en = {i: en[i] for i in [0] + [5 * n + 4 for n in range(steps)]}
    return {
        "f": float(np.abs(f - fr).max()),
        "dfdt": float(np.abs(dfdt - dfr).max()),
        "a": abs(a - ar) / abs(ar),
        "adot": abs(adot - adr) / abs(adr),
        "E": max(abs(E - enr[i][0]) / abs(enr[i][0])
                 for i, (E, P) in en.items()),
        "P": max(abs(P - enr[i][1]) / max(abs(enr[i][1]), abs(enr[i][0]))
                 for i, (E, P) in en.items()),
    }


def laplacian_fp32(u, h, dx, form="difference"):
    """Order-2h centred Laplacian of the periodic float32 array ``u``
    (last three axes are the grid), every operation in float32."""
    assert u.dtype == F32
    c = [F32(x) for x in LAP_COEFS[h]]
    inv2 = [F32(1.0 / d / d) for d in dx]
    ax = [u.ndim - 3 + mu for mu in range(3)]
    if form == "plain":
        c0 = F32(LAP_COEFS[h][0] * sum(1.0 / d / d for d in dx))
        la = u * c0
        for s in range(1, h + 1):
            la = la + c[s] * sum(
                (np.roll(u, -s, ax[mu]) + np.roll(u, s, ax[mu])) * inv2[mu]
                for mu in range(3))
    elif form == "difference":
        la = np.zeros_like(u)
        for s in range(1, h + 1):
            la = la + c[s] * sum(
                ((np.roll(u, -s, ax[mu]) - u) + (np.roll(u, s, ax[mu]) - u))
                * inv2[mu] for mu in range(3))
    else:
        raise ValueError(form)
    assert la.dtype == F32
    return la


# the potential and its derivative exactly as preheat_reference writes
# them, with float32 constants and arrays
M2, G = F32(MPHI**2), F32(GSQ)


def _potential32(f):
    phi, chi = f[0], f[1]
    return (M2 / F32(2) * phi**2 + G / F32(2) * phi**2 * chi**2) / M2


def _dpotential32(f):
    phi, chi = f[0], f[1]
    return np.stack([
        (M2 * phi + G * phi * chi**2) / M2,
        (G * phi**2 * chi) / M2,
    ])


def _mean64(x):
    assert x.dtype == F32
    return float(np.mean(x, dtype=np.float64))


def energy_fp32(f, dfdt, lap_f, a):
    """(E, P): the field part of each per-site reducer value in
    float32; the scale factor, the means and their combination in
    float64."""
    half = F32(0.5)
    kin = sum(_mean64(dfdt[i] * dfdt[i] * half) / a**2 for i in range(2))
    pot = _mean64(_potential32(f))
    grad = sum(_mean64(-f[i] * lap_f[i] * half) / a**2 for i in range(2))
    return kin + pot + grad, kin - grad / 3 - pot


def preheat_emulation_fp32(f0, df0, dx, dt, steps, h, form="difference",
                           mpl=MPL):
    """The float32 counterpart of
    ``preheat_reference.preheat_reference``: same arguments and return
    value, ``f`` and ``dfdt`` returned as float32."""
    f = np.array(f0, dtype=F32)
    dfdt = np.array(df0, dtype=F32)
    assert np.array_equal(f, np.asarray(f0)), "feed float32-rounded data"
    assert np.array_equal(dfdt, np.asarray(df0))

    lap_f = laplacian_fp32(f, h, dx, form)
    a = 1.0
    E, P = energy_fp32(f, dfdt, lap_f, a)
    adot = np.sqrt(8 * np.pi * a**2 / 3 / mpl**2 * E) * a
    energies = [(E, P)]

    k_f = np.zeros_like(f)
    k_df = np.zeros_like(dfdt)
    k_a = 0.0
    k_ad = 0.0
    dt32 = F32(dt)
    for _ in range(steps):
        for s in range(5):
            A32, B32 = F32(RK54_A[s]), F32(RK54_B[s])
            a32 = F32(a)
            hub32 = F32(adot / a)
            rhs_df = lap_f - F32(2) * hub32 * dfdt \
                - (a32 * a32) * _dpotential32(f)
            k_f = A32 * k_f + dt32 * dfdt
            k_df = A32 * k_df + dt32 * rhs_df
            f = f + B32 * k_f
            dfdt = dfdt + B32 * k_df
            assert f.dtype == F32 and dfdt.dtype == F32
            rhs_ad = 4 * np.pi * a**2 / 3 / mpl**2 * (E - 3 * P) * a
            k_a = RK54_A[s] * k_a + dt * adot
            k_ad = RK54_A[s] * k_ad + dt * rhs_ad
            a = a + RK54_B[s] * k_a
            adot = adot + RK54_B[s] * k_ad
            lap_f = laplacian_fp32(f, h, dx, form)
            E, P = energy_fp32(f, dfdt, lap_f, a)
            energies.append((E, P))
    return f, dfdt, a, adot, energies
