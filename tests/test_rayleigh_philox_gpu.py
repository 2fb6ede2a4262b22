"""The fused Rayleigh mode kernel (backend/hip.py ``rayleigh_modes``)
and RayleighGenerator(rng="philox") on the GPU: the kernel against this
file's own numpy transcription of the mode definition, the device
against the CPU path, index tables that do not start at 0, outputs
between guards, the argument checks, the launch count and the peak
memory of a call.

k-shape (12, 10, 8) of grid (12, 10, 14) is 960 modes, three full
blocks of 256 and a partial one; k-shape (9, 6, 4) of grid (9, 6, 7) is
a single partial block and has no Nyquist plane in x or z; the c2c
transform of (9, 6, 7) has no symmetric plane at all.

Bounds.  float64: |got - want| <= 16 * 2^-53 * T per mode, the
project's k-space tolerance, where T is the sum of the magnitudes of
the terms added (|z|; (|L|+|R|)/sqrt 2; omega (|L|+|R|)/sqrt 2 +
|H| |fk|), because L + R can cancel.  complex64: the same reference
rounded to float32, with 2 * 2^-24 * T.
"""

import functools
import types

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.fourier import DFT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

GRID = (12, 10, 14)
ODD = (9, 6, 7)
DK = (1.3, 0.9, 0.7)
VOLUME = 8.
NORM = 2.
MASS2 = 0.37
HUBBLE = 0.1
SEED = 0xfedcba9876543210      # both key words have their top bit set
DRAW = 5
RTOL = 16 * 2.0**-53
RTOL32 = 2 * 2.0**-24

# name: (grid, is_real)
SHAPES = {"12x10x14-r2c": (GRID, True), "9x6x7-r2c": (ODD, True),
          "9x6x7-c2c": (ODD, False)}


# -- this file's numpy transcription of the definition

def np_philox(counter, key):
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [int(key[0]), int(key[1])]
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & lo32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & lo32]
        k = [(k[0] + 0x9E3779B9) % 2**32, (k[1] + 0xBB67AE85) % 2**32]
    return c


def np_z(seed, draw, j, cx, cy, gz, sp, random):
    w = np_philox((cx, cy, gz, np.full_like(cx, 2 * draw + j)),
                  (seed % 2**32, seed // 2**32))
    u_amp = ((w[0] // 2**11 * 2**32 + w[1]) + 1).astype(np.float64) / 2.**53
    u_phs = ((w[2] // 2**11 * 2**32 + w[3]) + 1).astype(np.float64) / 2.**53
    amp = np.sqrt(-np.log(u_amp)) if random else np.ones_like(u_amp)
    # exp(2 pi i u) with the angle reduced exactly to at most pi/4
    v = 2 * u_phs
    q = np.rint(2 * v)
    r = np.pi * (v - q / 2)
    cis = (np.cos(r) + 1j * np.sin(r)) * np.array(
        [1, 1j, -1, -1j])[q.astype(int) % 4]
    return amp * sp * cis


def np_modes(gidx, grid, is_real, seed, draw, sp, om, hubble, random=True):
    """{"z", "fk", "dfk"}: (values, T) at the modes with global indices
    ``gidx`` (three 1-D arrays)."""
    shape = tuple(len(g) for g in gidx)
    gx, gy, gz = (np.broadcast_to(g, shape).astype(np.uint64) for g in (
        gidx[0][:, None, None], gidx[1][None, :, None],
        gidx[2][None, None, :]))
    Nx, Ny, Nz = (np.uint64(n) for n in grid)
    px, py = (Nx - gx) % Nx, (Ny - gy) % Ny
    plane = (gz == 0) | ((gz * 2 == Nz) if grid[2] % 2 == 0 else False)
    plane = plane & is_real
    keep = (gx < px) | ((gx == px) & (gy <= py))
    conj = plane & ~keep
    self_conj = plane & (gx == px) & (gy == py)
    cx, cy = np.where(conj, px, gx), np.where(conj, py, gy)
    L = np_z(seed, draw, 0, cx, cy, gz, sp, random)
    R = np_z(seed, draw, 1, cx, cy, gz, sp, random)
    fk = (L + R) / np.sqrt(2.)
    dfk = 1j * om * (L - R) / np.sqrt(2.) - hubble * fk
    lr = (np.abs(L) + np.abs(R)) / np.sqrt(2.)
    out = {}
    for name, v, mag in (("z", L, np.abs(L)), ("fk", fk, lr),
                         ("dfk", dfk, om * lr + abs(hubble) * np.abs(fk))):
        v = np.where(conj, v.conj(), v)
        v = np.where(self_conj, v.real + 0j, v)
        out[name] = (v, mag)
    return out


# -- inputs

def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def omega_k(k):
    return np.sqrt(k**2 + MASS2)


def _gidx_full(grid, is_real):
    g = [np.arange(n) for n in grid]
    if is_real:
        g[2] = np.arange(grid[2] // 2 + 1)
    return g


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape):
    """(gidx, sqrt_power, omega) over the whole k-space of ``shape``:
    a power spectrum and a frequency that vary with |k|, as bitwise
    symmetric under k -> -k as the generator's are."""
    grid, is_real = SHAPES[shape]
    gidx = _gidx_full(grid, is_real)
    k = [np.where(g > n // 2, g - n, g).astype(np.float64)
         for g, n in zip(gidx, grid)]
    kmag = np.sqrt((DK[0] * k[0][:, None, None])**2
                   + (DK[1] * k[1][None, :, None])**2
                   + (DK[2] * k[2][None, None, :])**2)
    om = omega_k(kmag)
    sp = np.sqrt(0.25 / 2 / om)
    sp[0, 0, 0] = 0.
    return gidx, sp, om


def launch(shape, wkb, random, ctype=torch.complex128, seed=SEED,
           draw=DRAW, hubble=HUBBLE, out=None):
    grid, is_real = SHAPES[shape]
    gidx, sp, om = kernel_inputs(shape)
    kshape = sp.shape
    if out is None:
        out = [torch.full(kshape, complex("nan+nanj"), dtype=ctype,
                          device="cuda") for _ in range(1 + wkb)]
    hip.rayleigh_modes(
        out[0], out[1] if wkb else None, _dev(sp), _dev(om) if wkb else None,
        [_dev(g.astype(np.int32)) for g in gidx], grid, seed, draw,
        hubble, is_real=is_real, random=random)
    torch.cuda.synchronize()
    return out


def assert_within(got, want, mag, rtol, what):
    got = np.asarray(got)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), what
    err = np.abs(got.astype(np.complex128) - want)
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"{what}: max err {worst:.3e} of the terms (bound {rtol:.3e})")
    assert (err <= rtol * mag).all(), (what, worst)


def assert_planes_hermitian(a, grid, what):
    Nx, Ny, Nz = grid
    ni, nj = (-np.arange(Nx)) % Nx, (-np.arange(Ny)) % Ny
    planes = [0] + ([Nz // 2] if Nz % 2 == 0 else [])
    for kz in planes:
        plane = a[:, :, kz]
        assert np.array_equal(plane[np.ix_(ni, nj)], plane.conj()), \
            (what, kz)
        for i in {0, Nx // 2 if Nx % 2 == 0 else 0}:
            for j in {0, Ny // 2 if Ny % 2 == 0 else 0}:
                assert plane[i, j].imag == 0, (what, kz, i, j)
        assert np.count_nonzero(plane.imag) > plane.size // 2


# -- 1. the kernel against numpy

@pytest.mark.parametrize("random", [True, False], ids=["random", "unit"])
@pytest.mark.parametrize("wkb", [False, True], ids=["generate", "wkb"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_numpy(shape, wkb, random):
    grid, is_real = SHAPES[shape]
    gidx, sp, om = kernel_inputs(shape)
    want = np_modes(gidx, grid, is_real, SEED, DRAW, sp, om, HUBBLE, random)
    out = [o.cpu().numpy() for o in launch(shape, wkb, random)]
    names = ("fk", "dfk") if wkb else ("z",)
    for name, got in zip(names, out):
        assert_within(got, *want[name], RTOL, f"{shape} {name}")
        assert np.abs(got).max() > 0
        if is_real:
            assert_planes_hermitian(got, grid, f"{shape} {name}")
    if not is_real:
        # no symmetry applied: the kz = 0 plane is not Hermitian
        ni, nj = (-np.arange(grid[0])) % grid[0], \
            (-np.arange(grid[1])) % grid[1]
        plane = out[0][:, :, 0]
        assert not np.array_equal(plane[np.ix_(ni, nj)], plane.conj())


@pytest.mark.parametrize("wkb", [False, True], ids=["generate", "wkb"])
def test_complex64_kernel_against_numpy(wkb):
    shape = "12x10x14-r2c"
    grid, is_real = SHAPES[shape]
    gidx, sp, om = kernel_inputs(shape)
    want = np_modes(gidx, grid, is_real, SEED, DRAW, sp, om, HUBBLE)
    out = launch(shape, wkb, True, ctype=torch.complex64)
    names = ("fk", "dfk") if wkb else ("z",)
    for name, got in zip(names, out):
        assert got.dtype == torch.complex64
        got = got.cpu().numpy()
        ref, mag = want[name]
        assert_within(got, ref.astype(np.complex64).astype(np.complex128),
                      mag, RTOL32, f"complex64 {name}")
        assert_planes_hermitian(got, grid, f"complex64 {name}")


def test_draw_and_seed_words_reach_the_counter():
    """A kernel that dropped the high key word, or the draw, would pass
    the comparison above only at the one (seed, draw) it uses."""
    shape = "9x6x7-r2c"
    grid, is_real = SHAPES[shape]
    gidx, sp, om = kernel_inputs(shape)
    for seed, draw in ((0, 0), (1 << 63, 0), (2**64 - 1, 2**30 - 1),
                       (0x7fffffff80000000, 1)):
        want = np_modes(gidx, grid, is_real, seed, draw, sp, om, 0.)
        got = launch(shape, True, True, seed=seed, draw=draw, hubble=0.)
        assert_within(got[0].cpu().numpy(), *want["fk"], RTOL,
                      f"seed {seed:#x} draw {draw}")


# -- 2. the device against the CPU path

def make_gen(grid, device, dtype=np.float64, fft=None):
    if fft is None:
        decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
        fft = DFT(decomp, grid_shape=grid, dtype=dtype, device=device)
    return ps.RayleighGenerator(fft=fft, dk=DK, volume=VOLUME, seed=SEED,
                                rng="philox")


def run_generator(gen, random=True):
    gen.draw = DRAW
    z = gen.generate(random=random, norm=NORM,
                     field_ps=lambda k: 1 / 2 / omega_k(k))
    fk, dfk = gen.generate_WKB(random=random, norm=NORM, omega_k=omega_k,
                               hubble=HUBBLE)
    assert gen.draw == DRAW + 2
    return {"z": z, "fk": fk, "dfk": dfk}


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128],
                         ids=["r2c", "r2c-fp32", "c2c"])
@pytest.mark.parametrize("grid", [GRID, ODD], ids=["12x10x14", "9x6x7"])
def test_device_equals_cpu_path(grid, dtype):
    is_real = np.dtype(dtype).kind == "f"
    want = run_generator(make_gen(grid, "cpu", dtype))
    got = run_generator(make_gen(grid, "cuda", dtype))
    rtol = RTOL32 if dtype == np.float32 else RTOL
    # T from this file's transcription, at the generator's own inputs
    gidx = _gidx_full(grid, is_real)
    k = [np.where(g > n // 2, g - n, g).astype(np.float64)
         for g, n in zip(gidx, grid)]
    kmag = np.sqrt(sum((d * kk)**2 for d, kk in zip(
        DK, np.meshgrid(*k, indexing="ij"))))
    om = omega_k(kmag)
    sp = np.sqrt(NORM / VOLUME / 2 / om)
    sp[0, 0, 0] = 0.
    mags = {}
    for name, draw in (("z", DRAW), ("fk", DRAW + 1), ("dfk", DRAW + 1)):
        mags[name] = np_modes(gidx, grid, is_real, SEED, draw, sp, om,
                              HUBBLE)[name][1]
    for name in want:
        assert got[name].dtype == want[name].dtype
        assert got[name].is_cuda
        assert_within(got[name].cpu().numpy(),
                      want[name].numpy().astype(np.complex128), mags[name],
                      rtol, f"{grid} {np.dtype(dtype).name} {name}")
        if is_real:
            assert_planes_hermitian(got[name].cpu().numpy(), grid, name)


# -- 3. index tables that do not start at 0

def _stub_fft(full, ysl, zsl):
    """A rank's view of ``full``'s k-space: y and z sliced."""
    sub_k = {"momenta_x": full.sub_k["momenta_x"],
             "momenta_y": full.sub_k["momenta_y"][ysl].contiguous(),
             "momenta_z": full.sub_k["momenta_z"][zsl].contiguous()}
    kshape = tuple(len(sub_k[n]) for n in
                   ("momenta_x", "momenta_y", "momenta_z"))
    return types.SimpleNamespace(
        fk=torch.empty(kshape, dtype=full.fk.dtype, device="cuda"),
        sub_k=sub_k, grid_shape=full.grid_shape, is_real=full.is_real,
        shape=lambda forward_output=True: kshape)


def test_slices_of_the_grid_equal_the_full_grid_bit_for_bit():
    """Hermitian partners of a slice's modes lie outside the slice."""
    full = make_gen(GRID, "cuda")
    want = run_generator(full)
    for ysl in (slice(0, 5), slice(5, 10)):
        for zsl in (slice(0, 4), slice(4, 8)):
            part = make_gen(GRID, "cuda",
                            fft=_stub_fft(full.fft, ysl, zsl))
            assert part._gidx[1][0] == ysl.start
            assert part._gidx[2][0] == zsl.start
            got = run_generator(part)
            for name in want:
                assert tuple(got[name].shape) == (12, 5, 4)
                assert torch.equal(got[name], want[name][:, ysl, zsl]), \
                    (name, ysl, zsl)


# -- 4. outputs between guards

@pytest.mark.parametrize("shape", ["12x10x14-r2c", "9x6x7-r2c"])
@pytest.mark.parametrize("ctype", [torch.complex128, torch.complex64],
                         ids=["complex128", "complex64"])
def test_outputs_lie_between_intact_guards(shape, ctype):
    vol = int(np.prod(kernel_inputs(shape)[1].shape))
    kshape = kernel_inputs(shape)[1].shape
    buf = torch.full((2 * vol + 3 * 256,), complex("nan+nanj"), dtype=ctype,
                     device="cuda")
    fk = buf[256:256 + vol].view(kshape)
    dfk = buf[512 + vol:512 + 2 * vol].view(kshape)
    launch(shape, True, True, ctype=ctype, out=[fk, dfk])
    written = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    written[256:256 + vol] = True
    written[512 + vol:512 + 2 * vol] = True
    nan = torch.isnan(buf.real) | torch.isnan(buf.imag)
    assert bool(nan[~written].all()), "a guard was written"
    assert not bool(nan[written].any()), "an output element was not written"


# -- 5. argument checks, before any launch

class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"the native module's {name} was reached")


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(hip, "ext", _NoLaunch)


def _good(wkb=True):
    gidx, sp, om = kernel_inputs("12x10x14-r2c")
    a = {"fk": torch.zeros(sp.shape, dtype=torch.complex128, device="cuda"),
         "dfk": torch.zeros(sp.shape, dtype=torch.complex128,
                            device="cuda") if wkb else None,
         "sqrt_power": _dev(sp), "omega": _dev(om) if wkb else None,
         "tables": [_dev(g.astype(np.int32)) for g in gidx],
         "seed": SEED, "draw": DRAW}
    return a


def _call(a):
    hip.rayleigh_modes(a["fk"], a["dfk"], a["sqrt_power"], a["omega"],
                       a["tables"], GRID, a["seed"], a["draw"], HUBBLE,
                       is_real=True)


def test_wrong_dtypes_are_refused(no_launch):
    for key, bad in (("fk", torch.float64), ("dfk", torch.complex64),
                     ("sqrt_power", torch.float32),
                     ("omega", torch.float32)):
        a = _good()
        a[key] = torch.zeros(a[key].shape, dtype=bad, device="cuda")
        with pytest.raises(TypeError, match=f"{key} has dtype"):
            _call(a)
    a = _good()
    a["tables"][1] = a["tables"][1].long()
    with pytest.raises(TypeError, match="int32"):
        _call(a)
    a = _good()
    a["fk"] = a["fk"].cpu()
    with pytest.raises(TypeError, match="must be a CUDA tensor"):
        _call(a)


def test_wrong_shapes_are_refused(no_launch):
    for key in ("dfk", "sqrt_power", "omega"):
        a = _good()
        a[key] = a[key][:, :, :7].contiguous()
        with pytest.raises(ValueError, match=f"{key} has shape"):
            _call(a)
    a = _good()
    a["tables"][2] = a["tables"][2][:7].contiguous()
    with pytest.raises(ValueError, match=r"tables\[z\] has shape"):
        _call(a)
    a = _good()
    a["fk"] = a["fk"].transpose(0, 1)
    with pytest.raises(ValueError, match="must be contiguous"):
        _call(a)
    a = _good()
    a["omega"] = None
    with pytest.raises(ValueError, match="omega goes with dfk"):
        _call(a)


def test_aliased_outputs_and_bad_counters_are_refused(no_launch):
    a = _good()
    a["dfk"] = a["fk"]
    with pytest.raises(ValueError, match="aliases fk"):
        _call(a)
    for key, bad in (("seed", -1), ("seed", 2**64), ("draw", 2**30),
                     ("draw", -1)):
        a = _good()
        a[key] = bad
        with pytest.raises(ValueError, match=key):
            _call(a)


def test_zero_volume_launches_nothing(no_launch):
    empty = torch.zeros((12, 0, 8), dtype=torch.complex128, device="cuda")
    gidx = kernel_inputs("12x10x14-r2c")[0]
    hip.rayleigh_modes(
        empty, None, torch.zeros((12, 0, 8), dtype=torch.float64,
                                 device="cuda"), None,
        [_dev(gidx[0].astype(np.int32)),
         torch.zeros(0, dtype=torch.int32, device="cuda"),
         _dev(gidx[2].astype(np.int32))], GRID, SEED, DRAW, is_real=True)


# -- 6. one launch per call, no recompilation

def test_one_launch_per_call_and_no_recompilation(monkeypatch):
    real = hip.ext()
    counts = {"jit_launch": 0, "jit_compile": 0}

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in counts:
                return fn

            def counted(*args, **kwargs):
                counts[name] += 1
                return fn(*args, **kwargs)
            return counted

    monkeypatch.setattr(hip, "ext", Spy)
    gen = make_gen(GRID, "cuda")
    first = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    assert counts["jit_launch"] == 1
    entries = set(hip._rayleigh_cache)
    compiled = counts["jit_compile"]
    gen.seed = SEED ^ 0xffff0000ffff
    gen.draw = 77
    second = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=0.3)
    assert counts["jit_launch"] == 2
    assert counts["jit_compile"] == compiled
    assert set(hip._rayleigh_cache) == entries
    assert not torch.equal(first[0], second[0])
    gen.generate(norm=NORM)
    assert counts["jit_launch"] == 3


# -- 7. memory

def _peak_extra(gen):
    """Peak of max_memory_allocated above what was allocated before a
    generate_WKB call (whose outputs are dropped)."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = gen.generate_WKB(norm=NORM, omega_k=omega_k, hubble=HUBBLE)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def test_philox_call_peaks_below_half_of_the_torch_call():
    """A condition on the design, counted from the code: the torch path
    holds at least 21 real k-space arrays at once, the philox path at
    most 9 (4 of outputs, sqrt_power and omega, three transients while
    the power is formed)."""
    grid = (64, 64, 64)
    one = 64 * 64 * 33 * 8
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    fft = DFT(decomp, grid_shape=grid, dtype=np.float64, device="cuda")
    torch_gen = ps.RayleighGenerator(fft=fft, dk=DK, volume=VOLUME, seed=3)
    philox_gen = ps.RayleighGenerator(fft=fft, dk=DK, volume=VOLUME, seed=3,
                                      rng="philox")
    _peak_extra(philox_gen)          # compiles the kernel
    peak_torch = _peak_extra(torch_gen)
    peak_philox = _peak_extra(philox_gen)
    print(f"peak extra memory in real k-space arrays: torch "
          f"{peak_torch / one:.1f}, philox {peak_philox / one:.1f}")
    assert peak_philox < peak_torch / 2
