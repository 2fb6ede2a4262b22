"""The generic hiprtc map kernels on the GPU at the shapes where they
can go wrong: ``JitElementwise`` (through ``ElementWiseMap`` and a
red-black smoother colour map), ``JitStencil`` (through ``Stencil``) and
``wrap_star``, each against the same formula written in numpy on the
inputs exactly as stored.

Shape A = (70, 11, 72).  For the 64z x 4y x 64x elementwise tile this is
x-chunks of 64 and 6, three y-blocks with 3 live rows in the last, and
z-blocks of 64 and 8.  For the 32z x 8y stencil tile with x-chunks of 32
it is x-chunks of 32, 32 and 6 (so the register ring is initialised at
i0 = 32 and 64), y-blocks of 8 and 3 and z-blocks of 32, 32 and 8.

Every output starts NaN-filled.  An unpadded output is the middle slab
``big[1:-1]`` of a sentinel-filled buffer whose guard slabs must come
back unchanged; a padded output's halo must come back unchanged.
"""

import itertools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.elementwise import ElementWiseMap
from pystella_amd.field import Field, shift_fields, var
from pystella_amd.stencil import Stencil

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

A = (70, 11, 72)
DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
NPTYPE = {torch.float64: np.float64, torch.float32: np.float32}
EPS = {torch.float64: 2.0**-53, torch.float32: 2.0**-24}
SENTINEL = -12345.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(rng, shape, tdtype, lo=-0.5):
    return (rng.random(shape) + lo).astype(NPTYPE[tdtype])


def _padded(shape, h):
    return tuple(n + 2 * h for n in shape)


def _interior(a, h, s=(0, 0, 0)):
    """The interior of the padded ``a`` (trailing three axes), shifted
    by ``s`` sites."""
    nx, ny, nz = (n - 2 * h for n in a.shape[-3:])
    return a[..., h + s[0]:h + s[0] + nx, h + s[1]:h + s[1] + ny,
             h + s[2]:h + s[2] + nz]


class Slab:
    """An unpadded NaN-filled device output that is the middle slab of a
    sentinel-filled buffer."""

    def __init__(self, shape, tdtype):
        self.big = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL,
                              dtype=tdtype, device="cuda")
        self.out = self.big[1:-1]
        assert self.out.is_contiguous()
        self.out.fill_(float("nan"))

    def result(self):
        torch.cuda.synchronize()
        big = self.big.cpu().numpy()
        assert np.all(big[0] == SENTINEL) and np.all(big[-1] == SENTINEL), \
            "a guard slab was written"
        return big[1:-1].astype(np.float64)


def _halo_mask(shape, h):
    mask = np.ones(_padded(shape, h), dtype=bool)
    mask[h:-h, h:-h, h:-h] = False
    return mask


def _close(got, ref, bound, what):
    assert not np.isnan(got).any(), f"{what}: sites left unwritten"
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (what, worst, got[worst], ref[worst])


# ---------------------------------------------------------------------------
# ElementWiseMap

@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
def test_map_with_temporary_and_scalar(tdtype):
    h = 2
    rng = np.random.default_rng(201)
    f = _rand(rng, _padded(A, h), tdtype)
    g = _rand(rng, A, tdtype)
    c = 1.375
    F, G = Field("f", offset="h"), Field("g", offset=0)
    out = Field("out", offset=0)
    t = var("t")
    ew = ElementWiseMap({out: t * var("c") + F}, tmp_instructions={t: F * G},
                        halo_shape=h)
    slab = Slab(A, tdtype)
    f_d, g_d = _dev(f), _dev(g)
    ew(f=f_d, g=g_d, out=slab.out, c=c)
    assert isinstance(ew._hip_kernel, hip.JitElementwise)
    assert ew._hip_kernel.grid == (2, 3, 2)
    got = slab.result()
    assert np.array_equal(f_d.cpu().numpy(), f)
    assert np.array_equal(g_d.cpu().numpy(), g)
    fw = _interior(f, h).astype(np.float64)
    gw = g.astype(np.float64)
    ref = fw * gw * c + fw
    # at most four roundings (the scalar's cast among them), doubled
    bound = 8 * EPS[tdtype] * (np.abs(fw * gw * c) + np.abs(fw))
    _close(got, ref, bound, "out")


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
def test_map_in_place_padded_update(tdtype):
    h = 2
    rng = np.random.default_rng(202)
    f = _rand(rng, _padded(A, h), tdtype)
    g = _rand(rng, A, tdtype)
    c = -0.625
    F, G = Field("f", offset="h"), Field("g", offset=0)
    ew = ElementWiseMap({F: F + var("c") * G * F}, halo_shape=h)
    f_d = _dev(f)
    ew(f=f_d, g=_dev(g), c=c)
    torch.cuda.synchronize()
    got = f_d.cpu().numpy()
    halo = _halo_mask(A, h)
    assert np.array_equal(got[halo], f[halo]), "the halo was written"
    fw = _interior(f, h).astype(np.float64)
    gw = g.astype(np.float64)
    ref = fw + c * gw * fw
    bound = 8 * EPS[tdtype] * (np.abs(fw) + np.abs(c * gw * fw))
    _close(_interior(got, h).astype(np.float64), ref, bound, "f")


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
def test_map_store_into_second_component(tdtype):
    h = 2
    rng = np.random.default_rng(203)
    f = _rand(rng, _padded(A, h), tdtype)
    g = _rand(rng, (2,) + _padded(A, h), tdtype)
    F = Field("f", offset="h")
    G = Field("g", offset="h", shape=(2,))
    ew = ElementWiseMap({G[1]: F * 2 + G[0] * var("c")}, halo_shape=h)
    c = 0.3
    _interior(g[1], h)[...] = np.nan
    g_d = _dev(g)
    ew(f=_dev(f), g=g_d, c=c)
    torch.cuda.synchronize()
    got = g_d.cpu().numpy()
    assert np.array_equal(got[0], g[0]), "component 0 was written"
    halo = _halo_mask(A, h)
    assert np.array_equal(got[1][halo], g[1][halo]), "the halo was written"
    fw = _interior(f, h).astype(np.float64)
    g0w = _interior(g[0], h).astype(np.float64)
    ref = fw * 2 + g0w * c
    bound = 8 * EPS[tdtype] * (np.abs(fw * 2) + np.abs(g0w * c))
    _close(_interior(got[1], h).astype(np.float64), ref, bound, "g[1]")


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
def test_red_black_colour_maps(tdtype, n=70):
    """Both colour maps of the red-black smoother, one call each: the
    colour's sites take f - omega (lap f - rho) / D, the other colour's
    sites and the halo keep their bits."""
    from pystella_amd.multigrid import RedBlackIterator
    h = 1
    shape = (n, n, n)
    omega = 0.9
    dx = 2 * np.pi / n
    decomp = ps.DomainDecomposition((1, 1, 1), h, rank_shape=shape)
    f = Field("f", offset="h")
    rho = Field("rho", offset="h")
    lap = sum(
        (shift_fields(f, tuple(int(m == d) for m in range(3)))
         - 2 * f
         + shift_fields(f, tuple(-int(m == d) for m in range(3))))
        for d in range(3)) / var("dx")[0]**2
    solver = RedBlackIterator(decomp, {f: (lap, rho)}, halo_shape=h,
                              fixed_parameters=dict(omega=omega))
    rng = np.random.default_rng(204)
    fv = _rand(rng, _padded(shape, h), tdtype)
    rv = _rand(rng, _padded(shape, h), tdtype)
    fw, rw = fv.astype(np.float64), rv.astype(np.float64)
    nbsum = sum(_interior(fw, h, tuple(s * int(m == d) for m in range(3)))
                for d in range(3) for s in (1, -1))
    nbabs = sum(
        np.abs(_interior(fw, h, tuple(s * int(m == d) for m in range(3))))
        for d in range(3) for s in (1, -1))
    f0, r0 = _interior(fw, h), _interior(rw, h)
    diag = -6 / dx**2
    gs = f0 - omega * ((nbsum - 6 * f0) / dx**2 - r0) / diag
    # about twenty operations on these magnitudes, doubled
    bound = 40 * EPS[tdtype] * (
        np.abs(f0) + omega * ((nbabs + 6 * np.abs(f0)) / 6
                              + np.abs(r0) * dx**2 / 6))
    i, j, k = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    parity = (i + j + k) & 1
    halo = _halo_mask(shape, h)
    for colour, stepper in enumerate(solver.color_steppers):
        f_d = _dev(fv)
        stepper(f=f_d, rho=_dev(rv), dx=np.array((dx,) * 3), rb_off=0.0)
        torch.cuda.synchronize()
        assert isinstance(stepper._hip_kernel, hip.JitElementwise)
        assert stepper._hip_kernel.grid == (2, 18, 2)
        got = f_d.cpu().numpy()
        assert np.array_equal(got[halo], fv[halo]), "the halo was written"
        gi = _interior(got, h)
        mine = parity == colour
        assert np.array_equal(gi[~mine], _interior(fv, h)[~mine]), \
            "the other colour was changed"
        ref = np.where(mine, gs, f0)
        _close(gi.astype(np.float64), ref, bound, f"colour {colour}")
        assert np.abs(gi[mine] - _interior(fv, h)[mine]).max() > 0.1


# ---------------------------------------------------------------------------
# Stencil

def _radii(h):
    """(inner, outer) shift of the two star radii at halo h."""
    return (h + 1) // 2, h


def _sh(a, h, s):
    return _interior(a, h, s).astype(np.float64)


def _run_stencil(statements, arrays, out_shape, tdtype, lds, monkeypatch):
    if lds:
        monkeypatch.delenv("PYSTELLA_STENCIL_LDS", raising=False)
    else:
        monkeypatch.setenv("PYSTELLA_STENCIL_LDS", "0")
    h = arrays.pop("_h")
    st = Stencil(statements, halo_shape=h, rank_shape=A)
    slab = Slab(out_shape, tdtype)
    dev = {k: (_dev(v) if isinstance(v, np.ndarray) else v)
           for k, v in arrays.items()}
    st(out=slab.out, **dev)
    got = slab.result()
    for k, v in arrays.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(dev[k].cpu().numpy(), v), \
                f"input {k} was written"
    if lds:
        assert isinstance(st._hip_kernel, hip.JitStencil), \
            "expected the LDS-staged kernel to be selected"
        assert st._hip_kernel.grid == (3, 2, 3)
    else:
        assert isinstance(st._hip_kernel, hip.JitElementwise)
        assert not isinstance(st._hip_kernel, hip.JitStencil)
    return got, st


def _stencil_tol(tdtype, ref):
    tol = 1e-12 if tdtype == torch.float64 else 1e-5
    return tol * (1 + np.abs(ref).max())


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_stencil_partial_tiles(h, tdtype, monkeypatch):
    """Star reads of f at two radii from the LDS tile, pure-x reads from
    the register ring, a mixed corner read from global memory and a
    second prefetched field."""
    r1, r2 = _radii(h)
    f = Field("f", offset="h")
    g = Field("g", offset="h")
    out = Field("out", offset=0)
    expr = (2.0 * f
            + shift_fields(f, (r1, 0, 0)) + shift_fields(f, (-r2, 0, 0))
            + 0.5 * (shift_fields(f, (0, r1, 0))
                     + shift_fields(f, (0, -r2, 0)))
            + 0.25 * (shift_fields(f, (0, 0, r2))
                      + shift_fields(f, (0, 0, -r1)))
            + 0.125 * shift_fields(f, (r1, r1, 0))
            + shift_fields(g, (0, r2, -r1)) * var("c"))
    rng = np.random.default_rng(205 + h)
    fv = _rand(rng, _padded(A, h), tdtype)
    gv = _rand(rng, _padded(A, h), tdtype)
    c = 1.5
    ref = (2.0 * _sh(fv, h, (0, 0, 0))
           + _sh(fv, h, (r1, 0, 0)) + _sh(fv, h, (-r2, 0, 0))
           + 0.5 * (_sh(fv, h, (0, r1, 0)) + _sh(fv, h, (0, -r2, 0)))
           + 0.25 * (_sh(fv, h, (0, 0, r2)) + _sh(fv, h, (0, 0, -r1)))
           + 0.125 * _sh(fv, h, (r1, r1, 0))
           + _sh(gv, h, (0, r2, -r1)) * c)
    bound = _stencil_tol(tdtype, ref)
    got, st = _run_stencil({out: expr}, dict(_h=h, f=fv, g=gv, c=c), A,
                           tdtype, True, monkeypatch)
    assert "r_f_0[2*H + 1]" in st._hip_kernel.source
    assert "__shared__ real t_f_0" in st._hip_kernel.source
    assert "__shared__ real t_g_0" in st._hip_kernel.source
    _close(got, ref, bound, "LDS form")
    plain, _ = _run_stencil({out: expr}, dict(_h=h, f=fv, g=gv, c=c), A,
                            tdtype, False, monkeypatch)
    _close(plain, ref, bound, "elementwise form")
    _close(plain, got, bound, "elementwise form against LDS form")


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_stencil_reads_second_component(h, tdtype, monkeypatch):
    """Star and pure-x reads of f[1] of a two-component field: the LDS
    tile and the register ring are based at component 1."""
    r1, r2 = _radii(h)
    f = Field("f", offset="h", shape=(2,))
    out = Field("out", offset=0)
    expr = (f[1] * var("c")
            + shift_fields(f[1], (r2, 0, 0)) - shift_fields(f[1], (-r1, 0, 0))
            + 0.5 * (shift_fields(f[1], (0, r2, 0))
                     + shift_fields(f[1], (0, 0, -r2)))
            + 0.25 * shift_fields(f[1], (0, -r1, r1)))
    rng = np.random.default_rng(215 + h)
    fv = _rand(rng, (2,) + _padded(A, h), tdtype)
    # component 0 must not be what is read
    fv[0] += 100
    c = -0.75
    f1 = fv[1]
    ref = (_sh(f1, h, (0, 0, 0)) * c
           + _sh(f1, h, (r2, 0, 0)) - _sh(f1, h, (-r1, 0, 0))
           + 0.5 * (_sh(f1, h, (0, r2, 0)) + _sh(f1, h, (0, 0, -r2)))
           + 0.25 * _sh(f1, h, (0, -r1, r1)))
    bound = _stencil_tol(tdtype, ref)
    got, st = _run_stencil({out: expr}, dict(_h=h, f=fv, c=c), A, tdtype,
                           True, monkeypatch)
    src = st._hip_kernel.source
    assert "t_f_1[t] = (f + 1L * PVOL)[goff];" in src
    assert "r_f_1[2*H] = (f + 1L * PVOL)[" in src
    # component 0 is not read, so it is neither staged nor ringed
    assert "t_f_0" not in src and "r_f_0" not in src
    _close(got, ref, bound, "LDS form")
    plain, _ = _run_stencil({out: expr}, dict(_h=h, f=fv, c=c), A, tdtype,
                            False, monkeypatch)
    _close(plain, ref, bound, "elementwise form")
    _close(plain, got, bound, "elementwise form against LDS form")


# ---------------------------------------------------------------------------
# wrap_star

AXES_SUBSETS = [s for r in (1, 2, 3)
                for s in itertools.combinations(range(3), r)]
OUTER_SHAPES = [(), (3,), (2, 3)]
WRAP_CASES = [((5, 7, 9), 1), ((5, 7, 9), 2), ((5, 7, 9), 3),
              ((5, 7, 9), 4), ((4, 5, 6), 4)]


def _check_wrap(got, base, shape, h, axes):
    """``got`` after wrapping ``axes`` of ``base`` (interior data inside a
    SENTINEL halo)."""
    outer = base.ndim - 3
    inner = tuple(slice(h, h + n) for n in shape)
    lead = (slice(None),) * outer
    assert np.array_equal(got[lead + inner], base[lead + inner]), \
        "the interior was written"
    interior = base[lead + inner]
    for ax in range(3):
        width = [(0, 0)] * outer + [(h, h) if a == ax else (0, 0)
                                    for a in range(3)]
        want = np.pad(interior, width, mode="wrap")
        for side in (slice(0, h), slice(h + shape[ax], None)):
            face = lead + tuple(side if a == ax else inner[a]
                                for a in range(3))
            wface = lead + tuple(side if a == ax else slice(None)
                                 for a in range(3))
            if ax in axes:
                assert np.array_equal(got[face], want[wface]), (ax, side)
            else:
                assert np.all(got[face] == SENTINEL), (ax, side)


def _wrap_input(rng, outer, shape, h, nptype):
    base = np.full(outer + _padded(shape, h), SENTINEL, dtype=nptype)
    _interior(base, h)[...] = rng.random(outer + shape)
    return base


@pytest.mark.parametrize("tdtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,h", WRAP_CASES,
                         ids=[f"{'x'.join(map(str, s))}-h{h}"
                              for s, h in WRAP_CASES])
def test_wrap_star_every_axis_subset(shape, h, tdtype):
    rng = np.random.default_rng(220 + h)
    for outer in OUTER_SHAPES:
        base = _wrap_input(rng, outer, shape, h, NPTYPE[tdtype])
        for axes in AXES_SUBSETS:
            arr = _dev(base)
            hip.wrap_star(arr, h, axes)
            torch.cuda.synchronize()
            try:
                _check_wrap(arr.cpu().numpy(), base, shape, h, axes)
            except AssertionError as e:
                raise AssertionError((outer, axes) + e.args) from e


def test_wrap_star_stride_loop(shape=(8, 150, 150), h=4, nf=6):
    """6 x 8 x 158 x 158 = 1 198 272 x-face cells, more than the 4096
    blocks of 256 threads the launch is capped at."""
    assert nf * 2 * h * (shape[1] + 2 * h) * (shape[2] + 2 * h) \
        == 1198272 > 4096 * 256
    rng = np.random.default_rng(230)
    base = _wrap_input(rng, (nf,), shape, h, np.float64)
    arr = _dev(base)
    hip.wrap_star(arr, h, (0, 1, 2))
    torch.cuda.synchronize()
    _check_wrap(arr.cpu().numpy(), base, shape, h, (0, 1, 2))
