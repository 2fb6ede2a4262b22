"""The complex64 observable kernels on the GPU: ``spectra_bin_c64``, the
seven ``projector_op_c64`` kernels and ``tt_project_c64``, at the shapes
where they can go wrong, and their routing from ``PowerSpectra`` and
``Projector`` built on a float32 transform.

Every reference is a plain numpy complex128 transcription
(tests/obs_c64_reference.py) applied to the complex64 inputs as stored,
widened.  The kernels widen once, work in double and round once on the
store, so a projected value is within one float32 rounding of the
reference plus the double kernels' own 1e-12, and a binned sum meets the
complex128 kernel's bound.
"""

import functools

import numpy as np
import pytest
import torch

from pystella_amd.backend import hip
from tests import obs_c64_reference as ref
from tests.obs_c64_reference import GRID, KSHAPE, U24, U53

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

GUARD = 4096
SENTINEL = complex(-7.25, 3.5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _c64(rng, shape):
    return (rng.standard_normal(shape)
            + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _wide(a):
    return a.astype(np.complex128)


def _scale(*inputs):
    return max(1.0, max(max(np.abs(a.real).max(), np.abs(a.imag).max())
                        for a in inputs))


class Guarded:
    """A NaN-filled complex64 output between two sentinel regions."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.flat = torch.full((n + 2 * GUARD,), SENTINEL,
                               dtype=torch.complex64, device="cuda")
        self.flat[GUARD:GUARD + n] = complex(np.nan, np.nan)
        self.out = self.flat[GUARD:GUARD + n].view(tuple(shape))
        assert self.out.is_contiguous()

    def result(self):
        flat = self.flat.cpu()
        assert bool((flat[:GUARD] == SENTINEL).all()), "front guard written"
        assert bool((flat[-GUARD:] == SENTINEL).all()), "back guard written"
        return self.out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _objects(grid=GRID, dtype=np.float32):
    fft, spectra, projector = ref.make_objects(grid, dtype, "cuda")
    eff = [projector.eff_mom[n].cpu().numpy().astype(np.float64)
           for n in ("eff_mom_x", "eff_mom_y", "eff_mom_z")]
    return fft, spectra, projector, eff


class Spies:
    """Counts the calls of the fused entry points, old and new."""

    NEW = ("spectra_bin_c64", "projector_op_c64", "tt_project_c64")
    OLD = ("spectra_bin", "projector_op")

    def __init__(self, monkeypatch):
        self.calls = {}
        for name in self.NEW + self.OLD:
            self._spy(monkeypatch, hip, name)
        self._spy(monkeypatch, hip.ext(), "tt_project")

    def _spy(self, monkeypatch, owner, name):
        real = getattr(owner, name)
        self.calls[name] = 0

        def spy(*args, **kwargs):
            self.calls[name] += 1
            return real(*args, **kwargs)

        monkeypatch.setattr(owner, name, spy)

    def only(self, **want):
        assert {k: v for k, v in self.calls.items() if v} == want, self.calls


# ---------------------------------------------------------------------------
# the raw binning kernel

N_SMALL = 1000                      # four blocks, the last one partial
N_STRIDE = 4096 * 256 + 77          # above the 4096-block cap


@functools.lru_cache(maxsize=None)
def _bin_inputs(n):
    rng = np.random.default_rng(207)
    fk = _c64(rng, n)
    kmag = 50 * rng.random(n)
    weights = {"unit": np.ones(n),
               "k3": rng.integers(1, 3, size=n) * kmag**3}
    return fk, weights


@pytest.mark.parametrize("weight", ["unit", "k3"])
@pytest.mark.parametrize("num_bins", [37, 700, 4096])
@pytest.mark.parametrize("n", [N_SMALL, N_STRIDE])
def test_spectra_bin_c64_direct(n, num_bins, weight):
    fk, weights = _bin_inputs(n)
    w = weights[weight]
    rng = np.random.default_rng(208 + num_bins)
    bidx = rng.integers(0, num_bins, size=n).astype(np.int32)
    bidx[0], bidx[n // 2], bidx[n - 1] = 0, num_bins - 1, num_bins - 1
    fk_d = _dev(fk)
    got = hip.spectra_bin_c64(fk_d, _dev(w), _dev(bidx), num_bins)
    assert got.dtype == torch.float64 and got.shape == (num_bins,)
    got = got.cpu().numpy()
    assert np.array_equal(fk_d.cpu().numpy(), fk)

    wide = _wide(fk)
    terms = w * (wide.real**2 + wide.imag**2)
    want = np.bincount(bidx, weights=terms, minlength=num_bins)
    nterm = np.bincount(bidx, minlength=num_bins)
    assert nterm[0] >= 1 and nterm[-1] >= 2
    bound = (nterm + 8) * U53 * want
    err = np.abs(got - want)
    print("spectra_bin_c64", n, num_bins, weight, "worst err/bound",
          np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), int(np.argmax(err - bound))
    assert np.all(got[nterm == 0] == 0)


def test_bin_power_c64_anisotropic_box(monkeypatch):
    fft, spectra, _, _ = _objects()
    assert fft.fk.dtype == torch.complex64
    assert fft.shape(True) == KSHAPE and int(np.prod(KSHAPE)) == 960
    fk = _c64(np.random.default_rng(209), KSHAPE)
    spies = Spies(monkeypatch)
    for k_power in (3, 0):
        want, nterm = ref.bin_power(_wide(fk), k_power)
        assert spectra.num_bins == len(want)
        got = spectra.bin_power(_dev(fk), k_power=k_power)
        bound = (nterm + 8) * U53 * want
        err = np.abs(got - want)
        print("bin_power c64", k_power, "worst err/bound",
              np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), k_power
    spies.only(spectra_bin_c64=2)


# ---------------------------------------------------------------------------
# the projector kernels

@functools.lru_cache(maxsize=None)
def _proj_inputs():
    rng = np.random.default_rng(210)
    return {"vec": _c64(rng, (3,) + KSHAPE), "hij": _c64(rng, (6,) + KSHAPE),
            "plus": _c64(rng, KSHAPE), "minus": _c64(rng, KSHAPE),
            "lng": _c64(rng, KSHAPE)}


def _unwritten(dev, host, what):
    assert np.array_equal(dev.cpu().numpy(), host), f"{what} was written"


def test_transversify_c64(monkeypatch):
    _, _, proj, eff = _objects()
    vec = _proj_inputs()["vec"]
    want = ref.transversify(_wide(vec), eff)
    spies = Spies(monkeypatch)
    src, g = _dev(vec), Guarded((3,) + KSHAPE)
    assert proj.transversify(vector=src, vector_T=g.out) is g.out
    ref.assert_stored(g.result(), want, _scale(vec), "out of place")
    _unwritten(src, vec, "vector")
    assert proj.transversify(src) is src
    ref.assert_stored(src.cpu().numpy(), want, _scale(vec), "in place")
    spies.only(projector_op_c64=2)


def test_vec_to_pol_and_back_c64(monkeypatch):
    _, _, proj, eff = _objects()
    inp = _proj_inputs()
    vec, plus, minus = inp["vec"], inp["plus"], inp["minus"]
    spies = Spies(monkeypatch)
    src, gp, gm = _dev(vec), Guarded(KSHAPE), Guarded(KSHAPE)
    proj.vec_to_pol(plus=gp.out, minus=gm.out, vector=src)
    wp, wm = ref.vec_to_pol(_wide(vec), eff)
    ref.assert_stored(gp.result(), wp, _scale(vec), "plus")
    ref.assert_stored(gm.result(), wm, _scale(vec), "minus")
    _unwritten(src, vec, "vector")
    spies.only(projector_op_c64=1)

    p, m, gv = _dev(plus), _dev(minus), Guarded((3,) + KSHAPE)
    proj.pol_to_vec(plus=p, minus=m, vector=gv.out)
    want = ref.pol_to_vec(_wide(plus), _wide(minus), eff)
    ref.assert_stored(gv.result(), want, _scale(plus, minus), "vector")
    _unwritten(p, plus, "plus")
    _unwritten(m, minus, "minus")
    spies.only(projector_op_c64=2)


@pytest.mark.parametrize("times_abs_k", [False, True])
def test_decompose_vector_c64(monkeypatch, times_abs_k):
    _, _, proj, eff = _objects()
    vec = _proj_inputs()["vec"]
    want = ref.decompose_vector(_wide(vec), eff, times_abs_k)
    # 1/k^2 and 1/|k| amplify lng; the bound's scale is the input's
    scale = _scale(vec)
    spies = Spies(monkeypatch)
    src = _dev(vec)
    outs = [Guarded(KSHAPE) for _ in range(3)]
    proj.decompose_vector(vector=src, plus=outs[0].out, minus=outs[1].out,
                          lng=outs[2].out, times_abs_k=times_abs_k)
    for g, w, name in zip(outs, want, ("plus", "minus", "lng")):
        ref.assert_stored(g.result(), w, scale, name)
    _unwritten(src, vec, "vector")
    # the outputs as views of the input, as PowerSpectra passes them
    proj.decompose_vector(vector=src, plus=src[0], minus=src[1], lng=src[2],
                          times_abs_k=times_abs_k)
    got = src.cpu().numpy()
    for c, name in enumerate(("plus", "minus", "lng")):
        ref.assert_stored(got[c], want[c], scale, name + " aliased")
    spies.only(projector_op_c64=2)


@pytest.mark.parametrize("times_abs_k", [False, True])
def test_decomp_to_vec_c64(monkeypatch, times_abs_k):
    _, _, proj, eff = _objects()
    inp = _proj_inputs()
    parts = [inp[n] for n in ("plus", "minus", "lng")]
    want = ref.decomp_to_vec(*[_wide(a) for a in parts], eff, times_abs_k)
    spies = Spies(monkeypatch)
    dev = [_dev(a) for a in parts]
    g = Guarded((3,) + KSHAPE)
    proj.decomp_to_vec(plus=dev[0], minus=dev[1], lng=dev[2], vector=g.out,
                       times_abs_k=times_abs_k)
    ref.assert_stored(g.result(), want, _scale(*parts), "vector")
    for d, a, name in zip(dev, parts, ("plus", "minus", "lng")):
        _unwritten(d, a, name)
    spies.only(projector_op_c64=1)


def test_tensor_to_pol_and_back_c64(monkeypatch):
    _, _, proj, eff = _objects()
    inp = _proj_inputs()
    hij, plus, minus = inp["hij"], inp["plus"], inp["minus"]
    wp, wm = ref.tensor_to_pol(_wide(hij), eff)
    spies = Spies(monkeypatch)
    src, gp, gm = _dev(hij), Guarded(KSHAPE), Guarded(KSHAPE)
    proj.tensor_to_pol(plus=gp.out, minus=gm.out, hij=src)
    ref.assert_stored(gp.result(), wp, _scale(hij), "plus")
    ref.assert_stored(gm.result(), wm, _scale(hij), "minus")
    _unwritten(src, hij, "hij")
    # plus and minus as views of hij, as PowerSpectra passes them
    proj.tensor_to_pol(plus=src[0], minus=src[1], hij=src)
    got = src.cpu().numpy()
    ref.assert_stored(got[0], wp, _scale(hij), "plus aliased")
    ref.assert_stored(got[1], wm, _scale(hij), "minus aliased")
    assert np.array_equal(got[2:], hij[2:]), "hij[2:] was written"
    spies.only(projector_op_c64=2)

    p, m, gt = _dev(plus), _dev(minus), Guarded((6,) + KSHAPE)
    proj.pol_to_tensor(plus=p, minus=m, hij=gt.out)
    want = ref.pol_to_tensor(_wide(plus), _wide(minus), eff)
    ref.assert_stored(gt.result(), want, _scale(plus, minus), "hij")
    _unwritten(p, plus, "plus")
    _unwritten(m, minus, "minus")
    spies.only(projector_op_c64=3)


# ---------------------------------------------------------------------------
# transverse-traceless projection on the matrix cores

TT_SMALL = (6, 5, 4)        # 90 k-sites: last wave holds two live sites
TT_LARGE = (96, 96, 114)    # 534 528 k-sites = 33 408 blocks: blockIdx.y


@functools.lru_cache(maxsize=None)
def _tt_case(grid):
    _, _, proj, eff = _objects(grid)
    kshape = tuple(len(e) for e in eff)
    hij = _c64(np.random.default_rng(211), (6,) + kshape)
    want = ref.transverse_traceless(_wide(hij), eff)
    return proj, kshape, hij, want


def _check_tt(got, want, hij):
    scale = _scale(hij)
    ref.assert_stored(got, want, scale, "hij_TT")
    tr = _wide(got[0]) + _wide(got[3]) + _wide(got[5])
    assert max(np.abs(tr.real).max(), np.abs(tr.imag).max()) \
        <= 8 * U24 * scale


@pytest.mark.parametrize("grid", [TT_SMALL, TT_LARGE], ids=["90", "534528"])
def test_tt_c64_in_place(monkeypatch, grid):
    proj, kshape, hij, want = _tt_case(grid)
    vol = int(np.prod(kshape))
    assert vol in (90, 534528)
    assert vol % 16 != 0 or -(-vol // 16) > 32768
    spies = Spies(monkeypatch)
    got = _dev(hij)
    assert proj.transverse_traceless(got) is got
    torch.cuda.synchronize()
    _check_tt(got.cpu().numpy(), want, hij)
    spies.only(tt_project_c64=1)


@pytest.mark.parametrize("grid", [TT_SMALL, TT_LARGE], ids=["90", "534528"])
def test_tt_c64_out_of_place_between_guards(monkeypatch, grid):
    proj, kshape, hij, want = _tt_case(grid)
    spies = Spies(monkeypatch)
    src, g = _dev(hij), Guarded((6,) + kshape)
    assert proj.transverse_traceless(hij=src, hij_TT=g.out) is g.out
    torch.cuda.synchronize()
    _check_tt(g.result(), want, hij)
    _unwritten(src, hij, "hij")
    spies.only(tt_project_c64=1)


# ---------------------------------------------------------------------------
# routing

def _gw_fields():
    return torch.from_numpy(ref.end_to_end_fields()["hij"]).cuda()


def test_gw_is_one_tt_launch_and_six_binning_launches(monkeypatch):
    _, spectra, proj, _ = _objects()
    spies = Spies(monkeypatch)
    spectra.gw(_gw_fields(), proj, ref.HUBBLE)
    spies.only(tt_project_c64=1, spectra_bin_c64=6)


def test_the_switch_forces_the_torch_branch(monkeypatch):
    monkeypatch.setenv("PYSTELLA_OBS_C64", "0")
    spies = Spies(monkeypatch)
    got = ref.run_spectra(np.float32, "cuda")
    spies.only()
    ref.assert_end_to_end(got)


def test_any_other_value_of_the_switch_keeps_the_kernels(monkeypatch):
    monkeypatch.setenv("PYSTELLA_OBS_C64", "1")
    _, spectra, proj, _ = _objects()
    spies = Spies(monkeypatch)
    spectra.gw_polarization(_gw_fields(), proj, ref.HUBBLE)
    spies.only(projector_op_c64=1, spectra_bin_c64=2)


def test_complex128_on_a_float32_transform_takes_the_old_kernels(
        monkeypatch):
    _, spectra, proj, eff = _objects()
    inp = _proj_inputs()
    vec, hij = _wide(inp["vec"]), _wide(inp["hij"])
    spies = Spies(monkeypatch)
    v = _dev(vec)
    proj.transversify(v)
    want = ref.transversify(vec, eff)
    assert np.abs(v.cpu().numpy() - want).max() <= 1e-12 * _scale(vec)
    h = _dev(hij)
    proj.transverse_traceless(h)
    want = ref.transverse_traceless(hij, eff)
    assert np.abs(h.cpu().numpy() - want).max() <= 1e-12 * _scale(hij)
    got = spectra.bin_power(_dev(vec[0]), k_power=3)
    want, nterm = ref.bin_power(vec[0], 3)
    assert np.all(np.abs(got - want) <= (nterm + 8) * U53 * want)
    spies.only(projector_op=1, tt_project=1, spectra_bin=1)


def test_mixed_types_take_the_torch_branch(monkeypatch):
    _, _, proj, eff = _objects()
    vec = _proj_inputs()["vec"]
    spies = Spies(monkeypatch)
    out = torch.zeros((3,) + KSHAPE, dtype=torch.complex128, device="cuda")
    proj.transversify(vector=_dev(vec), vector_T=out)
    want = ref.transversify(_wide(vec), eff)
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-5 * _scale(vec)
    spies.only()


def test_complex64_on_a_float64_transform_reaches_no_kernel(monkeypatch):
    _, spectra, proj, eff = _objects(GRID, np.float64)
    assert spectra.fft.fk.dtype == torch.complex128
    inp = _proj_inputs()
    spies = Spies(monkeypatch)
    v = _dev(inp["vec"])
    proj.transversify(v)
    want = ref.transversify(_wide(inp["vec"]), eff)
    assert np.abs(v.cpu().numpy() - want).max() <= 1e-5 * _scale(inp["vec"])
    h = _dev(inp["hij"])
    proj.transverse_traceless(h)
    p, m = _dev(inp["plus"]), _dev(inp["minus"])
    proj.tensor_to_pol(plus=p, minus=m, hij=h)
    proj.decompose_vector(vector=v, plus=v[0], minus=v[1], lng=v[2])
    got = spectra.bin_power(_dev(inp["plus"]), k_power=3)
    want, nterm = ref.bin_power(_wide(inp["plus"]), 3)
    assert np.all(np.abs(got - want)
                  <= ((nterm + 8) * U53 + 8 * U24) * want)
    spies.only()


def test_raw_entry_points_refuse_the_other_complex_type(monkeypatch):
    _, _, proj, _ = _objects()
    launched = []
    real_launch = hip.ext().jit_launch

    def record(*args):
        launched.append(args)
        return real_launch(*args)

    def reached(*args):
        launched.append(args)
        raise AssertionError("a refused tensor reached tt_project_c64")

    monkeypatch.setattr(hip.ext(), "jit_launch", record)
    monkeypatch.setattr(hip.ext(), "tt_project_c64", reached)
    n, nb = 1000, 37
    w = torch.ones(n, dtype=torch.float64, device="cuda")
    b = torch.zeros(n, dtype=torch.int32, device="cuda")
    f64 = torch.zeros(n, dtype=torch.complex64, device="cuda")
    f128 = torch.zeros(n, dtype=torch.complex128, device="cuda")
    with pytest.raises(TypeError):
        hip.spectra_bin_c64(f128, w, b, nb)
    with pytest.raises(TypeError):
        hip.spectra_bin(f64, w, b, nb)
    eff = proj._eff_c
    v128 = torch.zeros((3,) + KSHAPE, dtype=torch.complex128, device="cuda")
    v64 = torch.zeros((3,) + KSHAPE, dtype=torch.complex64, device="cuda")
    with pytest.raises(TypeError):
        hip.projector_op_c64("transversify", KSHAPE, [v128, v128], eff)
    with pytest.raises(TypeError):
        hip.projector_op_c64("transversify", KSHAPE, [v64, v128], eff)
    h128 = torch.zeros((6,) + KSHAPE, dtype=torch.complex128, device="cuda")
    h64 = torch.zeros((6,) + KSHAPE, dtype=torch.complex64, device="cuda")
    with pytest.raises(TypeError):
        hip.tt_project_c64(h128, h128, eff, KSHAPE)
    with pytest.raises(TypeError):
        hip.tt_project_c64(h64, h128, eff, KSHAPE)
    # the wrong shape, a CPU tensor and float32 tables are refused too
    with pytest.raises(ValueError):
        hip.tt_project_c64(h64[:5].contiguous(), h64, eff, KSHAPE)
    with pytest.raises(ValueError):
        hip.projector_op_c64("vec_to_pol", KSHAPE, [v64, v64, v64], eff)
    with pytest.raises(TypeError):
        hip.tt_project_c64(h64.cpu(), h64, eff, KSHAPE)
    with pytest.raises(TypeError):
        hip.projector_op_c64("transversify", KSHAPE, [v64, v64],
                             [e.float() for e in eff])
    assert not launched


# ---------------------------------------------------------------------------
# end to end

def test_float32_spectra_end_to_end(monkeypatch):
    spies = Spies(monkeypatch)
    got = ref.run_spectra(np.float32, "cuda")
    # __call__ 2; polarization 1 + 2; vector_decomposition 1 + 3;
    # gw 1 + 6; gw_polarization 1 + 2
    spies.only(spectra_bin_c64=15, projector_op_c64=3, tt_project_c64=1)
    ref.assert_end_to_end(got)
