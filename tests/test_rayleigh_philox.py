"""RayleighGenerator(rng="philox") on the CPU: Philox4x32-10 against its
known answers, the package's vectorised mode definition
(fourier/philox.py) against this file's own scalar transcription, the
exact Hermitian planes, the draw counter, the statistics of one fixed
realisation, and the independence of the realisation from the layout.

Nothing here shares code with the package: ``ref_*`` below are written
from the definition alone, in plain Python integers and ``math``.
"""

import math
import os
import sys

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.fourier import DFT, philox

GRID = (12, 10, 14)
ODD = (9, 6, 7)          # odd extents: no Nyquist plane in x or z
DK = (1.3, 0.9, 0.7)
VOLUME = 8.
NORM = 2.                # NORM / VOLUME = 1/4: an exact scaling
MASS2 = 0.37
HUBBLE = 0.1
SEED = 0xfedcba9876543210
EPS = 2.0**-53

KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# -- this file's transcription of the definition

def ref_philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff,
                          (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff)
        k0 = (k0 + 0x9E3779B9) & 0xffffffff
        k1 = (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def ref_uniforms(seed, draw, j, cx, cy, gz):
    w = ref_philox((cx, cy, gz, 2 * draw + j),
                   (seed & 0xffffffff, seed >> 32))
    u_amp = ((((w[0] >> 11) << 32) | w[1]) + 1) / 2**53
    u_phs = ((((w[2] >> 11) << 32) | w[3]) + 1) / 2**53
    return u_amp, u_phs


def ref_canonical(g, grid, is_real):
    """(cx, cy, conj, self_conj) of global index g."""
    gx, gy, gz = g
    if not is_real or not (gz == 0 or (grid[2] % 2 == 0
                                       and gz == grid[2] // 2)):
        return gx, gy, False, False
    px, py = (grid[0] - gx) % grid[0], (grid[1] - gy) % grid[1]
    if gx < px or (gx == px and gy <= py):
        return gx, gy, False, (px, py) == (gx, gy)
    return px, py, True, False


def ref_cis(u):
    """exp(2 pi i u), the angle reduced exactly to at most pi/4."""
    v = 2 * u
    q = round(2 * v)
    r = math.pi * (v - q / 2)
    z = complex(math.cos(r), math.sin(r))
    return z * (1, 1j, -1, -1j)[q % 4]


def ref_z(seed, draw, j, cx, cy, gz, sp, random):
    u_amp, u_phs = ref_uniforms(seed, draw, j, cx, cy, gz)
    amp = math.sqrt(-math.log(u_amp)) if random else 1.
    return amp * sp * ref_cis(u_phs)


def ref_store(z, conj, self_conj):
    if self_conj:
        return complex(z.real, 0.)
    return z.conjugate() if conj else z


def ref_arrays(gidx, grid, is_real, seed, draw, sqrt_power, omega, random):
    """(z, fk, dfk, T_z, T_fk, T_dfk) at every mode of the rank whose
    global indices are ``gidx``; T are the summed term magnitudes."""
    shape = tuple(len(g) for g in gidx)
    out = [np.zeros(shape, dtype=np.complex128) for _ in range(3)]
    mag = [np.zeros(shape) for _ in range(3)]
    for i, gx in enumerate(gidx[0]):
        for j, gy in enumerate(gidx[1]):
            for k, gz in enumerate(gidx[2]):
                cx, cy, conj, self_conj = ref_canonical(
                    (int(gx), int(gy), int(gz)), grid, is_real)
                sp, w = float(sqrt_power[i, j, k]), float(omega[i, j, k])
                L = ref_z(seed, draw, 0, cx, cy, int(gz), sp, random)
                R = ref_z(seed, draw, 1, cx, cy, int(gz), sp, random)
                fk = (L + R) / math.sqrt(2.)
                dfk = 1j * w * (L - R) / math.sqrt(2.) - HUBBLE * fk
                for n, v in enumerate((L, fk, dfk)):
                    out[n][i, j, k] = ref_store(v, conj, self_conj)
                lr = (abs(L) + abs(R)) / math.sqrt(2.)
                mag[0][i, j, k] = abs(L)
                mag[1][i, j, k] = lr
                mag[2][i, j, k] = w * lr + abs(HUBBLE) * abs(fk)
    return out + mag


# -- the generator under test

def make_fft(grid, dtype=np.float64):
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    return DFT(decomp, grid_shape=grid, dtype=dtype)


def make_gen(grid, seed=SEED, dtype=np.float64, fft=None, **kwargs):
    fft = fft or make_fft(grid, dtype)
    return ps.RayleighGenerator(fft=fft, dk=DK, volume=VOLUME, seed=seed,
                                rng="philox", **kwargs)


def omega_k(k):
    return np.sqrt(k**2 + MASS2)


def inputs(fft):
    """(gidx, sqrt_power, omega) as the generator forms them for the
    default WKB spectrum 1/(2 omega), in numpy."""
    sub_k = [fft.sub_k[n].numpy()
             for n in ("momenta_x", "momenta_y", "momenta_z")]
    gidx = [k.astype(np.int64) % n for k, n in zip(sub_k, fft.grid_shape)]
    kvecs = np.meshgrid(*sub_k, indexing="ij", sparse=False)
    kmags = np.sqrt(sum((dki * ki)**2 for dki, ki in zip(DK, kvecs)))
    omega = omega_k(kmags)
    wk = omega.copy()
    zero = kmags[0, 0, 0] == 0.
    if zero:
        wk[0, 0, 0] = wk[0, 0, 1]
    power = 1 / 2 / wk
    if zero:
        power[0, 0, 0] = 0.
    return gidx, np.sqrt(power * (NORM / VOLUME)), omega


def assert_within(got, want, mag, ulps, what):
    err = np.abs(got - want)
    worst = float((err / np.maximum(mag, 1e-300)).max() / EPS)
    print(f"{what}: max err {worst:.2f} x 2^-53 of the terms "
          f"(bound {ulps})")
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    assert (err <= ulps * EPS * mag).all(), (what, worst)


# -- known answers

def test_philox_known_answers():
    for counter, key, want in KAT:
        assert ref_philox(counter, key) == want
        got = philox.philox4x32(counter, key)
        assert tuple(int(w) for w in got) == want
    # vectorised over arrays of counters
    c = np.array([[k[0][n] for k in KAT] for n in range(4)])
    for n, (counter, key, want) in enumerate(KAT):
        got = philox.philox4x32(tuple(c), key)
        assert tuple(int(w[n]) for w in got) == want


@pytest.mark.parametrize("grid", [GRID, ODD], ids=["12x10x14", "9x6x7"])
def test_uniforms_equal_the_transcription_bit_for_bit(grid):
    fft = make_fft(grid)
    gidx = philox.global_indices(fft)
    cx, cy, gz, conj, self_conj = philox.canonical_indices(
        gidx, grid, True)
    draw = 3
    for j in (0, 1):
        u_amp, u_phs = philox.philox_uniforms(SEED, draw, j, cx, cy, gz)
        assert u_amp.dtype == np.float64 and u_amp.shape == fft.shape(True)
        for idx in np.ndindex(*u_amp.shape):
            g = tuple(int(gidx[n][idx[n]]) for n in range(3))
            rx, ry, rconj, rself = ref_canonical(g, grid, True)
            assert (rx, ry, rconj, rself) == (
                cx[idx], cy[idx], conj[idx], self_conj[idx])
            assert (u_amp[idx], u_phs[idx]) == ref_uniforms(
                SEED, draw, j, rx, ry, g[2])
        assert u_amp.min() > 0 and u_amp.max() <= 1
        assert u_phs.min() > 0 and u_phs.max() <= 1
    # some mode on a symmetric plane takes its partner's numbers
    assert conj.any() and self_conj.any()


@pytest.mark.parametrize("random", [True, False], ids=["random", "unit"])
@pytest.mark.parametrize("grid", [GRID, ODD], ids=["12x10x14", "9x6x7"])
def test_modes_equal_the_transcription(grid, random):
    gen = make_gen(grid)
    gidx, sqrt_power, omega = inputs(gen.fft)
    gen.draw = 5
    z = gen.generate(random=random, norm=NORM,
                     field_ps=lambda k: 1 / 2 / omega_k(k))
    fk, dfk = gen.generate_WKB(random=random, norm=NORM, omega_k=omega_k,
                               hubble=HUBBLE)
    assert gen.draw == 7
    assert z.dtype == fk.dtype == dfk.dtype == torch.complex128
    want5 = ref_arrays(gidx, grid, True, SEED, 5, sqrt_power, omega, random)
    want6 = ref_arrays(gidx, grid, True, SEED, 6, sqrt_power, omega, random)
    assert_within(z.numpy(), want5[0], want5[3], 4, "generate")
    assert_within(fk.numpy(), want6[1], want6[4], 4, "WKB fk")
    assert_within(dfk.numpy(), want6[2], want6[5], 4, "WKB dfk")
    if not random:
        # unit amplitudes: |z| is sqrt_power, but for the real-only modes
        pair = ~philox.canonical_indices(gidx, grid, True)[4]
        assert (np.abs(np.abs(z.numpy()) - sqrt_power)[pair]
                <= 4 * EPS * sqrt_power[pair]).all()


def test_complex64_transform_rounds_once():
    gen = make_gen(GRID, dtype=np.float32)
    wide = make_gen(GRID)
    fk, dfk = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    fk_w, dfk_w = wide.generate_WKB(norm=NORM, omega_k=omega_k,
                                    hubble=HUBBLE)
    assert fk.dtype == dfk.dtype == torch.complex64
    assert torch.equal(fk, fk_w.to(torch.complex64))
    assert torch.equal(dfk, dfk_w.to(torch.complex64))


def test_complex_transform_applies_no_symmetry():
    fft = make_fft(ODD, np.complex128)
    gen = make_gen(ODD, fft=fft)
    gidx, sqrt_power, omega = inputs(fft)
    assert tuple(sqrt_power.shape) == ODD
    fk, dfk = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    want = ref_arrays(gidx, ODD, False, SEED, 0, sqrt_power, omega, True)
    assert_within(fk.numpy(), want[1], want[4], 4, "c2c fk")
    assert_within(dfk.numpy(), want[2], want[5], 4, "c2c dfk")
    assert fk[3, 0, 0].imag != 0 and fk[6, 0, 0] != fk[3, 0, 0].conj()


# -- Hermitian planes

def test_symmetric_planes_are_exactly_hermitian():
    gen = make_gen(GRID)
    z = gen.generate(norm=NORM, field_ps=lambda k: 1 / 2 / omega_k(k))
    fk, dfk = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    Nx, Ny, Nz = GRID
    ni = (-np.arange(Nx)) % Nx
    nj = (-np.arange(Ny)) % Ny
    for name, a in (("z", z), ("fk", fk), ("dfk", dfk)):
        a = a.numpy()
        for kz in (0, Nz // 2):
            plane = a[:, :, kz]
            partner = plane[np.ix_(ni, nj)]
            assert np.array_equal(partner, plane.conj()), (name, kz)
            for i in (0, Nx // 2):
                for j in (0, Ny // 2):
                    assert plane[i, j].imag == 0, (name, kz, i, j)
            assert np.count_nonzero(plane.imag) > plane.size // 2
        # an interior plane is not symmetric
        assert not np.array_equal(a[:, :, 1][np.ix_(ni, nj)],
                                  a[:, :, 1].conj())
        # and the package's own symmetriser finds nothing to change
        sym = ps.fourier.rayleigh.make_hermitian(torch.as_tensor(a).clone())
        assert np.array_equal(sym.numpy(), a)
    for a in (z, fk, dfk):
        fx = gen.fft.idft(a.clone()).clone()
        assert torch.isfinite(fx).all()
        assert fx.std() > 0


# -- draws

def test_draws_number_the_realisations():
    a, b = make_gen(GRID), make_gen(GRID)
    assert a.draw == 0
    first = []
    for n in range(3):
        fa, fb = a.generate(), b.generate()
        assert torch.equal(fa, fb)
        wa, wb = a.generate_WKB(hubble=HUBBLE), b.generate_WKB(hubble=HUBBLE)
        assert torch.equal(wa[0], wb[0]) and torch.equal(wa[1], wb[1])
        assert a.draw == b.draw == 2 * n + 2
        first.append(fa)
    assert not torch.equal(first[0], first[1])
    assert not torch.equal(first[1], first[2])
    a.draw = 2
    assert torch.equal(a.generate(), first[1])
    assert a.draw == 3
    other = make_gen(GRID, seed=SEED ^ 1)
    assert not torch.equal(other.generate(), first[0])
    high = make_gen(GRID, seed=SEED ^ (1 << 63))
    assert not torch.equal(high.generate(), first[0])


def test_init_calls_consume_draws_in_call_order():
    gen = make_gen(GRID)
    fx = torch.zeros(GRID, dtype=torch.float64)
    dfx = torch.zeros(GRID, dtype=torch.float64)
    gen.init_field(fx)
    assert gen.draw == 1
    gen.init_WKB_fields(fx, dfx, hubble=HUBBLE)
    assert gen.draw == 2
    replay = make_gen(GRID)
    replay.draw = 1
    fk, dfk = replay.generate_WKB(hubble=HUBBLE)
    assert torch.equal(replay.fft.idft(fk).clone(), fx)


# -- statistics of one fixed realisation

def test_statistics_of_a_fixed_realisation():
    """5-sigma bounds on a deterministic input: a failure is a bug.  The
    homogeneous mode carries no power and is left out of the ratios."""
    grid = (32, 32, 32)
    M = 32 * 32 * 17
    gen = make_gen(grid, seed=20261021)
    power = NORM / VOLUME
    z0 = gen.generate(norm=NORM, field_ps=lambda k: 1.).numpy()
    z1 = gen.generate(norm=NORM, field_ps=lambda k: 1.).numpy()
    assert z0.size == M and z0[0, 0, 0] == 0
    keep = np.ones(z0.shape, dtype=bool)
    keep[0, 0, 0] = False
    a0 = np.abs(z0[keep])**2 / power
    a1 = np.abs(z1[keep])**2 / power
    bound = 5 / math.sqrt(M)
    mean = abs(a0.mean() - 1)
    phase = abs(np.mean(z0[keep] / np.abs(z0[keep])))
    corr = abs(np.corrcoef(a0, a1)[0, 1])
    print(f"mean amp^2 - 1: {mean:.4f}, |mean phase|: {phase:.4f}, "
          f"draw correlation: {corr:.4f}; bound {bound:.4f}")
    assert mean < bound
    assert phase < bound
    assert corr < bound


# -- layout independence

def _layout_worker(rank, world_size, proc_shape):
    full_fft = make_fft(GRID)
    full = make_gen(GRID, fft=full_fft)
    decomp = ps.DomainDecomposition(proc_shape, 0, grid_shape=GRID)
    fft = DFT(decomp, grid_shape=GRID, dtype=np.float64)
    assert tuple(fft.shape(True)) != tuple(full_fft.shape(True))
    part = make_gen(GRID, fft=fft)
    full.draw = part.draw = 4
    want = full.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    got = part.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)

    full_g = philox.global_indices(full_fft)
    part_g = philox.global_indices(fft)
    where = np.ix_(*[[int(np.flatnonzero(f == g)[0]) for g in p]
                     for f, p in zip(full_g, part_g)])
    # the uniforms, bit for bit
    cf = philox.canonical_indices(full_g, GRID, True)
    cp = philox.canonical_indices(part_g, GRID, True)
    for j in (0, 1):
        uf = philox.philox_uniforms(SEED, 4, j, *cf[:3])
        up = philox.philox_uniforms(SEED, 4, j, *cp[:3])
        for f, p in zip(uf, up):
            assert np.array_equal(f[where], p)
    # the values
    gidx, sqrt_power, omega = inputs(full_fft)
    L = np.sqrt(-np.log(philox.philox_uniforms(SEED, 4, 0, *cf[:3])[0]))
    R = np.sqrt(-np.log(philox.philox_uniforms(SEED, 4, 1, *cf[:3])[0]))
    lr = (L + R) * sqrt_power / math.sqrt(2.)
    mags = (lr, omega * lr + HUBBLE * np.abs(want[0].numpy()))
    for name, g, w, mag in zip(("fk", "dfk"), got, want, mags):
        assert tuple(g.shape) == tuple(fft.shape(True))
        assert np.abs(w.numpy()).max() > 0
        assert_within(g.numpy(), w.numpy()[where], mag[where], 4,
                      f"rank {rank} {proc_shape} {name}")


@pytest.mark.parametrize("proc_shape", [(2, 1, 1), (1, 2, 1)],
                         ids=["2x1x1", "1x2x1"])
def test_realisation_does_not_depend_on_the_layout(proc_shape):
    from tests.conftest import run_distributed
    run_distributed(_layout_worker, 2, args=(proc_shape,))


# -- errors

def test_bad_arguments_are_refused():
    fft = make_fft(GRID)
    with pytest.raises(ValueError, match="rng"):
        ps.RayleighGenerator(fft=fft, dk=DK, volume=VOLUME, rng="threefry")
    for seed in (-1, 2**64):
        with pytest.raises(ValueError, match="seed"):
            make_gen(GRID, seed=seed, fft=fft)
    make_gen(GRID, seed=2**64 - 1, fft=fft).generate()
    gen = make_gen(GRID, fft=fft)
    gen.draw = 2**30
    with pytest.raises(ValueError, match="draw"):
        gen.generate()
    with pytest.raises(ValueError, match="draw"):
        gen.generate_WKB()
    gen.draw = 2**30 - 1
    gen.generate()
    with pytest.raises(ValueError, match="draw"):
        gen.generate()
    gen.draw = -1
    with pytest.raises(ValueError, match="draw"):
        gen.generate()


# -- the default generator never reaches the new code

def _raise(*args, **kwargs):
    raise AssertionError("rng='torch' reached the philox path")


def test_default_path_is_untouched(monkeypatch):
    def run():
        gen = ps.RayleighGenerator(fft=make_fft(GRID), dk=DK,
                                   volume=VOLUME, seed=77)
        assert gen.rng == "torch" and not hasattr(gen, "draw")
        return (gen.generate(),) + gen.generate_WKB(hubble=HUBBLE)
    want = run()
    monkeypatch.setattr(hip, "rayleigh_modes", _raise)
    monkeypatch.setattr(hip, "rayleigh_source", _raise)
    for name in philox.__all__:
        monkeypatch.setattr(philox, name, _raise)
    got = run()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


# -- the example

def test_example_runs_with_philox(tmp_path):
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "examples"))
    import scalar_preheating
    os.chdir(tmp_path)
    expand, energy = scalar_preheating.main(
        ["--grid-shape", "16", "16", "16", "--end-time", "0.07",
         "--device", "cpu", "--no-output", "--rng", "philox"])
    assert np.isfinite(energy["total"])
    assert np.isfinite(expand.constraint(energy["total"]))
