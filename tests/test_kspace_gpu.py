"""The fused k-space kernels (backend/hip.py ``kspace_derivs``,
``kspace_div_accum``, ``kspace_poisson``) on the GPU: each kernel
against a numpy transcription of its formula, SpectralCollocator and
SpectralPoissonSolver against their CPU results, the routing between
the fused path and the torch chain, and the argument checks.

The grid is (12, 10, 14): k-shape (12, 10, 8) is 960 modes, three full
blocks of 256 and a partial one, and its three extents differ, as do
the three box lengths, so no transposed index or table can pass.
"""

import functools

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.derivs import SecondCenteredDifference
from pystella_amd.fourier import DFT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

GRID = (12, 10, 14)
KSHAPE = (12, 10, 8)
LENGTHS = (5., 3., 7.)
VOLK = int(np.prod(KSHAPE))
INV_N = 1.0 / float(np.prod(GRID))
OUTS = ("pdx", "pdy", "pdz", "lap")
GRAD = ("pdx", "pdy", "pdz")
# at most eight rounded operations on same-signed terms, doubled
RTOL = 16 * 2.0**-53
# the bound tests/test_gpu.py holds the rocFFT path to, scaled to the data
CLASS_RTOL = 1e-12


def _dk(lengths=LENGTHS):
    return tuple(2 * np.pi / li for li in lengths)


def _dx(grid=GRID, lengths=LENGTHS):
    return tuple(li / n for li, n in zip(lengths, grid))


@functools.lru_cache(maxsize=None)
def tables():
    """(k1, k2, eig): the per-axis tables of both classes at GRID, as
    numpy arrays."""
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=GRID)
    fft = DFT(decomp, grid_shape=GRID, dtype=np.float64)
    coll = ps.SpectralCollocator(fft, _dk())
    k1 = tuple(k.reshape(-1).numpy().copy() for k in coll.k1)
    k2 = tuple(k.reshape(-1).numpy().copy() for k in coll.k2)
    eig = tuple(
        np.asarray(SecondCenteredDifference(1).get_eigenvalues(
            _dk()[mu] * fft.sub_k[name].numpy().astype(np.float64),
            _dx()[mu]), dtype=np.float64)
        for mu, name in enumerate(("momenta_x", "momenta_y", "momenta_z")))
    assert [len(k) for k in k1] == list(KSHAPE)
    return k1, k2, eig


@functools.lru_cache(maxsize=None)
def mode_data(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(KSHAPE) + 1j * rng.standard_normal(KSHAPE)


def _bcast(tabs):
    return (tabs[0][:, None, None], tabs[1][None, :, None],
            tabs[2][None, None, :])


def _cplx(re, im):
    out = np.empty(KSHAPE, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


class Guarded:
    """A k-space output that ends one block before its allocation does:
    a store past VOLK lands in the NaN-filled tail."""

    def __init__(self):
        self.buf = torch.full((VOLK + 256,), complex("nan+nanj"),
                              dtype=torch.complex128, device="cuda")
        self.out = self.buf[:VOLK].view(KSHAPE)

    def untouched(self):
        return bool(torch.isnan(self.buf.real).all()
                    and torch.isnan(self.buf.imag).all())

    def tail_untouched(self):
        tail = self.buf[VOLK:]
        return bool(torch.isnan(tail.real).all()
                    and torch.isnan(tail.imag).all())


def assert_close(got, want, what):
    """Real and imaginary parts separately; exact zeros stay zero."""
    got = got.cpu().numpy()
    for part in ("real", "imag"):
        g, w = getattr(got, part), getattr(want, part)
        assert np.isfinite(g).all(), (what, part)
        err = np.abs(g - w)
        worst = float((err / np.maximum(np.abs(w), 1e-300)).max())
        print(f"{what}.{part}: max rel err {worst:.3e} (bound {RTOL:.3e})")
        assert (err <= RTOL * np.abs(w)).all(), (what, part, worst)
        assert (g[w == 0] == 0).all(), (what, part)


# -- 1. kernels against numpy

def want_derivs(fk):
    k1, k2, _ = tables()
    tr, ti = fk.real * INV_N, fk.imag * INV_N
    want = {}
    for name, q in zip(GRAD, _bcast(k1)):
        want[name] = _cplx(-q * ti, q * tr)
    kx, ky, kz = _bcast(k2)
    mk2 = -((kx * kx + ky * ky) + kz * kz)
    want["lap"] = _cplx(mk2 * tr, mk2 * ti)
    return want


@pytest.mark.parametrize(
    "mask", [("pdx",), ("pdy",), ("pdz",), ("lap",), GRAD, GRAD + ("lap",)],
    ids="+".join)
def test_derivs_kernel_against_numpy(mask):
    k1, k2, _ = tables()
    fk = mode_data(1)
    fk_d = _dev(fk)
    fk_before = fk_d.clone()
    bufs = {name: Guarded() for name in OUTS}
    hip.kspace_derivs(fk_d, {name: bufs[name].out for name in mask},
                      [_dev(k) for k in k1], [_dev(k) for k in k2], INV_N)
    torch.cuda.synchronize()
    want = want_derivs(fk)
    # the k1 tables hold zeros (k = 0 and Nyquist): those outputs are 0
    assert any((want[name] == 0).any() for name in GRAD)
    for name in OUTS:
        if name in mask:
            assert_close(bufs[name].out, want[name], name)
            assert bufs[name].tail_untouched(), name
        else:
            assert bufs[name].untouched(), name
    assert torch.equal(fk_d, fk_before)


def test_div_accum_kernel_against_numpy():
    k1, _, _ = tables()
    terms = []
    div = Guarded()
    for mu in range(3):
        fk = mode_data(10 + mu)
        q = _bcast(k1)[mu]
        terms.append(_cplx((-q * fk.imag) * INV_N, (q * fk.real) * INV_N))
        hip.kspace_div_accum(_dev(fk), div.out, _dev(k1[mu]), mu, INV_N,
                             accumulate=mu > 0)
        torch.cuda.synchronize()
        if mu == 0:
            assert_close(div.out, terms[0], "div store")
        elif mu == 1:
            assert_close(div.out, terms[0] + terms[1], "div accumulate")
    assert_close(div.out, (terms[0] + terms[1]) + terms[2], "div three")
    assert div.tail_untouched()


def want_poisson(rhok, m2):
    ex, ey, ez = _bcast(tables()[2])
    mk2 = (ex + ey) + ez
    den = np.where(mk2 < 0, mk2 - m2, 1.0)
    re = np.where(mk2 < 0, (rhok.real * INV_N) / den, 0.0)
    im = np.where(mk2 < 0, (rhok.imag * INV_N) / den, 0.0)
    return _cplx(re, im)


@pytest.mark.parametrize("m2", [0.0, 1.7])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in_place"])
def test_poisson_kernel_against_numpy(m2, in_place):
    eig = tables()[2]
    assert all((e <= 0).all() for e in eig) and eig[0][0] == 0
    rhok = mode_data(20)
    rhok_d = _dev(rhok)
    sol = Guarded()
    if in_place:
        sol.out.copy_(rhok_d)
        rhok_d = sol.out
    hip.kspace_poisson(rhok_d, sol.out, *[_dev(e) for e in eig], INV_N, m2)
    torch.cuda.synchronize()
    want = want_poisson(rhok, m2)
    assert want[0, 0, 0] == 0 and rhok[0, 0, 0] != 0
    assert_close(sol.out, want, f"poisson m2={m2}")
    assert sol.tail_untouched()
    if not in_place:
        assert torch.equal(rhok_d, _dev(rhok))


# -- 2. classes, GPU against CPU

CASES = {"12x10x14": ((12, 10, 14), LENGTHS),
         "16x16x16": ((16, 16, 16), (2 * np.pi,) * 3)}
H = 1


@functools.lru_cache(maxsize=None)
def class_inputs(case):
    grid, _ = CASES[case]
    pad = tuple(n + 2 * H for n in grid)
    gen = torch.Generator().manual_seed(31)
    fx = torch.rand((2,) + pad, dtype=torch.float64, generator=gen)
    vec = torch.rand((2, 3) + pad, dtype=torch.float64, generator=gen)
    rho = 0.25 + torch.rand(grid, dtype=torch.float64, generator=gen)
    return fx, vec, rho


def run_collocator(case, device, dtype=np.float64):
    """Every call form of the collocator; returns its outputs on the
    CPU, by name."""
    grid, lengths = CASES[case]
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=grid)
    fft = DFT(decomp, grid_shape=grid, dtype=dtype, device=device)
    coll = ps.SpectralCollocator(fft, _dk(lengths))
    fx, vec, _ = (t.to(device=device, dtype=tdtype)
                  for t in class_inputs(case))
    fx_before = fx.clone()
    pad = fx.shape[1:]

    def zeros(*shape):
        return torch.zeros(shape, dtype=tdtype, device=device)

    out = {"lap": zeros(2, *pad), "grd": zeros(2, 3, *grid)}
    coll(fx=fx, lap=out["lap"], grd=out["grd"])            # two slices
    assert torch.equal(fx, fx_before)
    tup = tuple(zeros(2, *grid) for _ in range(3))
    coll(fx=fx, grd=tup)
    out["grd_tuple"] = torch.stack(tup, dim=1)
    for name in OUTS:
        out[name + "_only"] = zeros(*grid)
        coll(fx[1], **{name: out[name + "_only"]})
    out["div"] = zeros(2, *grid)
    coll.divergence(vec=vec, div=out["div"])
    if device != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(fx, fx_before)
    return {k: v.cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def collocator_cpu(case):
    return run_collocator(case, "cpu")


def assert_outputs_agree(got, want, what):
    assert got.keys() == want.keys()
    for name in want:
        scale = want[name].abs().max().item()
        err = (got[name] - want[name]).abs().max().item()
        print(f"{what} {name}: max err {err:.3e} at magnitude {scale:.3e}")
        assert scale > 0
        assert err <= CLASS_RTOL * scale, (what, name, err, scale)


@pytest.mark.parametrize("case", list(CASES))
def test_collocator_gpu_against_cpu(case):
    want = collocator_cpu(case)
    got = run_collocator(case, "cuda")
    assert_outputs_agree(got, want, case)
    # the array, tuple and single-output forms agree among themselves
    assert torch.equal(got["grd"], got["grd_tuple"])
    for mu, name in enumerate(GRAD):
        assert torch.equal(got[name + "_only"], got["grd"][1, mu])


def run_poisson(device, m2, solver=None):
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=GRID)
    if solver is None:
        fft = DFT(decomp, grid_shape=GRID, dtype=np.float64, device=device)
        solver = ps.SpectralPoissonSolver(
            fft, _dk(), _dx(), SecondCenteredDifference(H).get_eigenvalues)
    rho = class_inputs("12x10x14")[2].to(device)
    rho_before = rho.clone()
    fx = torch.zeros(tuple(n + 2 * H for n in GRID), dtype=torch.float64,
                     device=device)
    solver(fx=fx, rho=rho, m_squared=m2)
    assert torch.equal(rho, rho_before)
    return fx.cpu()


@functools.lru_cache(maxsize=None)
def poisson_cpu(m2):
    return run_poisson("cpu", m2)


@pytest.mark.parametrize("m2", [0, 1.7])
def test_poisson_gpu_against_cpu(m2):
    want = poisson_cpu(m2)
    got = run_poisson("cuda", m2)
    assert_outputs_agree({"f": got}, {"f": want}, f"poisson m2={m2}")
    # the source has a mean; the k = 0 mode is dropped for either mass
    interior = (slice(H, -H),) * 3
    mean = got[interior].mean().abs().item()
    print(f"interior mean {mean:.3e}, max|f| {got.abs().max().item():.3e}")
    assert mean <= 1e-14 * got.abs().max().item()


# -- 3. routing

@pytest.fixture
def launches(monkeypatch):
    """Counts of the fused entry points' calls."""
    counts = dict.fromkeys(
        ("kspace_derivs", "kspace_div_accum", "kspace_poisson"), 0)
    for name in counts:
        def counted(*args, _name=name, _fn=getattr(hip, name), **kwargs):
            counts[_name] += 1
            return _fn(*args, **kwargs)
        monkeypatch.setattr(hip, name, counted)
    return counts


def _collocator(dtype=np.float64):
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=GRID)
    fft = DFT(decomp, grid_shape=GRID, dtype=dtype, device="cuda")
    return ps.SpectralCollocator(fft, _dk())


def test_one_launch_per_operation(launches, monkeypatch):
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    coll = _collocator()
    fx, vec, _ = (t.cuda() for t in class_inputs("12x10x14"))
    lap = torch.zeros_like(fx)
    grd = torch.zeros((2, 3) + GRID, dtype=torch.float64, device="cuda")
    coll(fx=fx, lap=lap, grd=grd)
    assert launches == {"kspace_derivs": 2, "kspace_div_accum": 0,
                        "kspace_poisson": 0}
    div = torch.zeros((2,) + GRID, dtype=torch.float64, device="cuda")
    coll.divergence(vec=vec, div=div)
    assert launches["kspace_div_accum"] == 6
    assert launches["kspace_derivs"] == 2
    # the scratch buffers grow to the largest subset and are reused
    assert len(coll._scratch) == 4
    ptrs = [b.data_ptr() for b in coll._scratch]
    coll(fx=fx, lap=lap)
    coll.divergence(vec=vec, div=div)
    assert [b.data_ptr() for b in coll._scratch] == ptrs


def test_knob_forces_the_torch_chain(launches, monkeypatch):
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    fused = run_collocator("12x10x14", "cuda")
    fused_p = run_poisson("cuda", 1.7)
    assert launches["kspace_derivs"] > 0 and launches["kspace_poisson"] == 1
    before = dict(launches)
    monkeypatch.setenv("PYSTELLA_KSPACE", "0")
    chain = run_collocator("12x10x14", "cuda")
    chain_p = run_poisson("cuda", 1.7)
    assert launches == before
    assert_outputs_agree(chain, fused, "chain against fused")
    assert_outputs_agree({"f": chain_p}, {"f": fused_p},
                         "poisson chain against fused")


def test_float32_transform_keeps_the_torch_chain(launches, monkeypatch):
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    got = run_collocator("12x10x14", "cuda", dtype=np.float32)
    assert not any(launches.values())
    want = collocator_cpu("12x10x14")
    for name, out in got.items():
        assert out.dtype == torch.float32
        # a sanity check only: float32 data (2^-24) through -k^2 <= 207
        scale = want[name].abs().max().item()
        assert (out.double() - want[name]).abs().max().item() < 1e-3 * scale


def test_new_mass_compiles_nothing(launches, monkeypatch):
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=GRID)
    fft = DFT(decomp, grid_shape=GRID, dtype=np.float64, device="cuda")
    solver = ps.SpectralPoissonSolver(
        fft, _dk(), _dx(), SecondCenteredDifference(H).get_eigenvalues)
    first = run_poisson("cuda", 1.7, solver)
    entries = set(hip._kspace_cache)
    assert any(key[0] == "poisson" for key in entries)
    second = run_poisson("cuda", 0.3, solver)
    assert set(hip._kspace_cache) == entries
    assert launches["kspace_poisson"] == 2
    assert not torch.equal(first, second)


# -- 4. errors

class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"the native module's {name} was reached")


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(hip, "ext", _NoLaunch)


def _good():
    k1, k2, eig = tables()
    return {"fk": _dev(mode_data(1)),
            "out": torch.zeros(KSHAPE, dtype=torch.complex128,
                               device="cuda"),
            "k1": [_dev(k) for k in k1], "k2": [_dev(k) for k in k2],
            "eig": [_dev(e) for e in eig]}


def _calls(a):
    return {
        "derivs": lambda: hip.kspace_derivs(
            a["fk"], {"pdx": a["out"]}, a["k1"], a["k2"], INV_N),
        "div_accum": lambda: hip.kspace_div_accum(
            a["fk"], a["out"], a["k1"][0], 0, INV_N, False),
        "poisson": lambda: hip.kspace_poisson(
            a["fk"], a["out"], *a["eig"], INV_N, 0.0),
    }


@pytest.mark.parametrize("op", ["derivs", "div_accum", "poisson"])
def test_wrong_dtypes_are_refused(op, no_launch):
    a = _good()
    a["fk"] = a["fk"].to(torch.complex64)
    with pytest.raises(TypeError,
                       match="(fk|rhok) has dtype torch.complex64"):
        _calls(a)[op]()
    a = _good()
    a["out"] = a["out"].to(torch.complex64)
    with pytest.raises(TypeError, match="has dtype torch.complex64"):
        _calls(a)[op]()
    a = _good()
    for key in ("k1", "k2", "eig"):
        a[key][0] = a[key][0].float()
    with pytest.raises(TypeError, match="has dtype torch.float32"):
        _calls(a)[op]()


@pytest.mark.parametrize("op", ["derivs", "div_accum"])
def test_output_aliasing_fk_is_refused(op, no_launch):
    a = _good()
    a["out"] = a["fk"]
    with pytest.raises(ValueError, match="aliases fk"):
        _calls(a)[op]()


@pytest.mark.parametrize("op", ["derivs", "div_accum", "poisson"])
def test_cpu_tensors_are_refused(op, no_launch):
    a = _good()
    a["fk"] = a["fk"].cpu()
    with pytest.raises(TypeError, match="must be a CUDA tensor"):
        _calls(a)[op]()
    a = _good()
    for key in ("k1", "k2", "eig"):
        a[key][0] = a[key][0].cpu()
    with pytest.raises(TypeError, match="must be a CUDA tensor"):
        _calls(a)[op]()


def test_derivs_refuses_other_outputs(no_launch):
    a = _good()
    for outs in ({}, {"pdw": a["out"]}):
        with pytest.raises(ValueError, match="non-empty subset"):
            hip.kspace_derivs(a["fk"], outs, a["k1"], a["k2"], INV_N)
    with pytest.raises(ValueError, match="alias each other"):
        hip.kspace_derivs(a["fk"], {"pdx": a["out"], "lap": a["out"]},
                          a["k1"], a["k2"], INV_N)
    with pytest.raises(ValueError, match="must be contiguous"):
        hip.kspace_derivs(a["fk"].transpose(0, 1), {"lap": a["out"]},
                          a["k1"], a["k2"], INV_N)
