"""The observable kernels on the GPU at the shapes where they can go
wrong: ``JitReduction``, ``JitHistogram`` (``Histogrammer`` and
``FieldHistogrammer``), ``spectra_bin`` and the matrix-core
transverse-traceless projection, each against a plain numpy float64
reference computed from the inputs exactly as stored (a float32 input
is widened, not regenerated).  The references share no code with the
expression front-end.

Shape A = (70, 11, 72): for the 64z x 4y x 64x reduction tile this is
x-chunks of 64 and 6, three y-blocks with 3 live rows in the last, and
z-blocks of 64 and 8, twelve blocks in all.  For the 256-thread
histogram it is 217 blocks with the last one partial; (70, 64, 66) is
295 680 sites, above the 1024-block cap, so 33 536 threads take a second
stride.
"""

import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.field import Field, var
from pystella_amd.fourier import DFT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

A = (70, 11, 72)
B = (70, 64, 66)
H = 2
U53 = 2.0**-53
U24 = 2.0**-24
DTYPES = [torch.float64, torch.float32]
NPTYPE = {torch.float64: np.float64, torch.float32: np.float32}
TILE = (64, 4, 64)
HALO_FILL = 3.0e30      # read by no kernel; would spoil every result


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad(interior, h=H, fill=HALO_FILL):
    """``interior`` (trailing three axes) inside a halo of ``fill``."""
    shape = interior.shape[:-3] + tuple(n + 2 * h
                                        for n in interior.shape[-3:])
    out = np.full(shape, fill, dtype=interior.dtype)
    out[..., h:-h, h:-h, h:-h] = interior
    return out


def _nblk(shape, tile=TILE):
    nx, ny, nz = shape
    return (-(-nz // tile[0])) * (-(-ny // tile[1])) * (-(-nx // tile[2]))


def _sum_bound(v, tdtype, shape=A):
    """Error bound of a block-tree sum of the per-site values ``v``:
    XCHUNK sequential adds per thread, eight tree levels, a worst-case
    sequential finish over the block partials and eight per-site
    roundings (the listed expressions make at most three in the kernel
    and three in the reference; the division of an average by N is one
    more).  Float32 fields add at most six float roundings per site,
    scalar casts included, taken as 16."""
    s = math.fsum(np.abs(v).ravel())
    bound = (TILE[2] + 8 + _nblk(shape) + 8) * U53 * s
    if tdtype == torch.float32:
        bound += 16 * U24 * s
    return bound


# ---------------------------------------------------------------------------
# Reduction

@functools.lru_cache(maxsize=None)
def _reduction_inputs(tdtype):
    rng = np.random.default_rng(101)
    f = (rng.random(A) - 0.4).astype(NPTYPE[tdtype])        # signed
    g = (0.5 + rng.random(A)).astype(NPTYPE[tdtype])        # positive
    return f, g


def test_twelve_blocks_at_shape_a():
    assert _nblk(A) == 12 and np.prod(A) == 55440


@pytest.mark.parametrize("tdtype", DTYPES, ids=["f64", "f32"])
def test_reduction_partial_tiles(tdtype):
    f, g = _reduction_inputs(tdtype)
    a = 1.7
    n = float(np.prod(A))
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=A)
    F = Field("f", offset="h")
    G = Field("g", offset=0)
    red = ps.Reduction(decomp, {
        "f": [(F, "avg"), (F, "sum"), (F, "max"), (F, "min")],
        "kin": [(F**2 / 2 / var("a")**2, "avg")],
        "fg": [(F * G / var("a"), "sum")],
    }, halo_shape=H, grid_size=n)
    out = red(f=_dev(_pad(f)), g=_dev(g), a=np.array([a]))
    assert isinstance(red._hip_kernel, hip.JitReduction)
    assert red._hip_kernel.dtype == tdtype
    assert red._hip_kernel.nblk == 12

    fw, gw = f.astype(np.float64), g.astype(np.float64)
    # extrema of a bare field are exact
    assert out["f"][2] == fw.max(), (out["f"][2], fw.max())
    assert out["f"][3] == fw.min(), (out["f"][3], fw.min())

    def check(name, got, v, avg):
        ref = math.fsum(v.ravel())
        bound = _sum_bound(v, tdtype)
        if avg:
            ref, bound = ref / n, bound / n
        print(name, tdtype, "err", abs(got - ref), "bound", bound)
        assert abs(got - ref) <= bound, (name, got, ref, bound)

    check("avg f", out["f"][0], fw, True)
    check("sum f", out["f"][1], fw, False)
    check("avg kin", out["kin"][0], fw**2 / 2 / a**2, True)
    check("sum fg", out["fg"][0], fw * gw / a, False)


def _exact_product(vals):
    """Product of the float64 ``vals``: in extended precision where
    that has at least 60 bits, else exactly."""
    if np.finfo(np.longdouble).eps < 2.0**-60:
        ref = np.longdouble(1)
        for chunk in np.array_split(vals.astype(np.longdouble), 64):
            ref = ref * np.prod(chunk)
        return ref
    items = [Fraction(float(x)) for x in vals]
    while len(items) > 1:
        items = [items[i] * items[i + 1] if i + 1 < len(items)
                 else items[i] for i in range(0, len(items), 2)]
    return items[0]


@pytest.mark.parametrize("tdtype", DTYPES, ids=["f64", "f32"])
def test_reduction_prod(tdtype):
    rng = np.random.default_rng(102)
    f = (1 + 1e-4 * (rng.random(A) - 0.5)).astype(NPTYPE[tdtype])
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=A)
    red = ps.Reduction(decomp, {"p": [(Field("f", offset="h"), "prod")]},
                       halo_shape=H)
    got = red(f=_dev(_pad(f)))["p"][0]
    n = int(np.prod(A))
    ref = _exact_product(f.astype(np.float64).ravel())
    if isinstance(ref, Fraction):
        rel = abs(float((Fraction(float(got)) - ref) / ref))
    else:
        rel = float(abs(np.longdouble(got) - ref) / ref)
    # one rounding per multiply, in the threads, the tree and the finish
    bound = 2 * (n + _nblk(A)) * U53
    if tdtype == torch.float32:
        bound += 16 * U24 * n
    print("prod", tdtype, got, "rel", rel, "bound", bound)
    assert 0.5 < got < 2.0
    assert rel <= bound, (got, ref, rel, bound)


@pytest.mark.parametrize("tdtype", DTYPES, ids=["f64", "f32"])
def test_field_statistics_two_components(tdtype):
    rng = np.random.default_rng(103)
    f = (rng.random((2,) + A) - np.array([0.3, 0.8]).reshape(2, 1, 1, 1)
         ).astype(NPTYPE[tdtype])
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=A)
    stats = ps.FieldStatistics(decomp, H, max_min=True)
    out = stats(_dev(_pad(f)))
    n = float(np.prod(A))
    for c in range(2):
        fw = f[c].astype(np.float64)
        assert out["max"][c] == fw.max()
        assert out["min"][c] == fw.min()
        assert out["abs_max"][c] == np.abs(fw).max()
        assert out["abs_min"][c] == np.abs(fw).min()
        mean = math.fsum(fw.ravel()) / n
        b1 = _sum_bound(fw, tdtype) / n
        assert abs(out["mean"][c] - mean) <= b1, (c, out["mean"][c], mean)
        sq = fw**2
        msq = math.fsum(sq.ravel()) / n
        b2 = _sum_bound(sq, tdtype) / n
        # <f^2> - <f>^2: both averages' bounds and the two roundings of
        # the square and the difference
        bound = b2 + 2 * abs(mean) * b1 + b1**2 + 2 * U53 * (msq + mean**2)
        ref = msq - mean**2
        print("variance", c, tdtype, abs(out["variance"][c] - ref), bound)
        assert abs(out["variance"][c] - ref) <= bound


# ---------------------------------------------------------------------------
# Histogrammer

def _bin_values(rng, shape, num_bins, nptype):
    """(b + u) / num_bins with integer b in [0, num_bins) and u in
    [0.25, 0.75] on a 2^-10 lattice: at most 22 significant bits, so the
    value is the same number in float32 and float64."""
    b = rng.integers(0, num_bins, size=shape)
    u = 0.25 + rng.integers(0, 513, size=shape) / 1024.0
    val = ((b + u) / num_bins).astype(nptype)
    return val


def _checked_bins(values, num_bins):
    """Bin index of ``values * num_bins`` in float64, after asserting
    that each is at least 0.25 away from an integer."""
    t = values.astype(np.float64).ravel() * num_bins
    assert np.all(np.abs(t - np.round(t)) >= 0.25)
    b = np.trunc(t).astype(np.int64)
    assert b.min() >= 0 and b.max() < num_bins
    return b


def _binned_fsum(b, w, num_bins):
    order = np.argsort(b, kind="stable")
    bs, ws = b[order], w[order]
    edges = np.searchsorted(bs, np.arange(num_bins + 1))
    return np.array([math.fsum(ws[edges[i]:edges[i + 1]])
                     for i in range(num_bins)])


HIST_CASES = [(A, 64), (B, 64), (A, 4096)]


@pytest.mark.parametrize("tdtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape,num_bins", HIST_CASES,
                         ids=["A-64", "B-64", "A-3x4096"])
def test_histogrammer_strides_and_templates(shape, num_bins, tdtype):
    assert num_bins & (num_bins - 1) == 0   # value * num_bins is exact
    rng = np.random.default_rng(104)
    p = _bin_values(rng, shape, num_bins, NPTYPE[tdtype])
    u = _bin_values(rng, shape, num_bins, NPTYPE[tdtype])
    P = Field("p", offset="h")
    U = Field("u", offset=0)
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=shape)
    hist = ps.Histogrammer(decomp, {
        "unit_p": (P * num_bins, 1),
        "w_p": (U * num_bins, P),
        "w_uu": (P * num_bins, U * U),
    }, num_bins, halo_shape=H)
    out = hist(p=_dev(_pad(p)), u=_dev(u))

    kern = hist._hip_kernel
    assert kern.dtype == tdtype
    total = int(np.prod(shape))
    assert kern.grid == min(-(-total // 256), 1024)
    if shape == B:
        assert 256 * kern.grid < total          # the stride loop runs
    lds = "__shared__ double lh" in kern.source
    assert lds == (3 * num_bins <= hip._HIST_LDS_DOUBLES)
    assert lds == (num_bins == 64)

    bp = _checked_bins(p, num_bins)
    bu = _checked_bins(u, num_bins)
    pw, uw = p.astype(np.float64).ravel(), u.astype(np.float64).ravel()

    assert out["unit_p"].sum() == total
    assert np.array_equal(out["unit_p"],
                          np.bincount(bp, minlength=num_bins))

    for name, b, w in (("w_p", bu, pw), ("w_uu", bp, uw * uw)):
        ref = _binned_fsum(b, w, num_bins)
        count = np.bincount(b, minlength=num_bins)
        sabs = _binned_fsum(b, np.abs(w), num_bins)
        bound = (count + 4) * U53 * sabs
        if tdtype == torch.float32:
            bound = bound + 8 * U24 * sabs
        err = np.abs(out[name] - ref)
        print(name, shape, num_bins, tdtype, "worst err/bound",
              np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (name, np.argmax(err - bound))
        assert np.all(out[name][count == 0] == 0)


def test_histogram_refuses_another_dtype():
    """The kernel is built for the first field's type; a second field of
    the other type is refused before anything is launched."""
    num_bins = 64
    rng = np.random.default_rng(105)
    p = _bin_values(rng, A, num_bins, np.float64)
    u = _bin_values(rng, A, num_bins, np.float64)
    P = Field("p", offset="h")
    U = Field("u", offset=0)
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=A)
    for first, second in ((torch.float64, torch.float32),
                          (torch.float32, torch.float64)):
        hist = ps.Histogrammer(decomp, {"w": (P * num_bins, U)}, num_bins,
                               halo_shape=H)
        names = [fa.name for fa in hist.field_args if fa.spatial]
        arrays = {"p": _dev(_pad(p)), "u": _dev(u)}
        arrays[names[0]] = arrays[names[0]].to(first)
        arrays[names[1]] = arrays[names[1]].to(second)
        with pytest.raises(TypeError):
            hist(**arrays)
        assert hist._hip_kernel.dtype == first
        # the built kernel, called directly with the other type throughout
        other = {k: v.to(second) for k, v in arrays.items()}
        with pytest.raises(TypeError):
            hist._hip_kernel(other)
        # the front end rebuilds for a consistent set
        out = hist(**other)
        assert hist._hip_kernel.dtype == second
        bp = _checked_bins(p, num_bins)
        assert abs(out["w"].sum() - math.fsum(u.ravel())) \
            < 1e-6 * u.sum()
        assert np.array_equal(out["w"] > 0,
                              np.bincount(bp, minlength=num_bins) > 0)


# ---------------------------------------------------------------------------
# FieldHistogrammer

FH_BINS = 50
FH_RANGES = {"linear": [(0.5, 2.75), (-3.0, -0.75)],
             "log": [(-2.0, 3.0), (0.25, 4.0)]}


def _field_hist_arrays(nptype):
    """Two (2,) + A arrays: one whose linear bin values, one whose log
    bin values are (b + u) with u in [0.25, 0.75], each with one site
    exactly at its minimum and one exactly at its maximum."""
    rng = np.random.default_rng(106)
    lin = np.empty((2,) + A)
    lg = np.empty((2,) + A)
    for c in range(2):
        for arr, (lo, hi) in ((lin, FH_RANGES["linear"][c]),
                              (lg, FH_RANGES["log"][c])):
            b = rng.integers(0, FH_BINS, size=A)
            u = 0.25 + 0.5 * rng.random(A)
            v = lo + (b + u) * (hi - lo) / FH_BINS
            v.flat[1234], v.flat[4321 + c] = lo, hi
            arr[c] = v
        lg[c] = (-1) ** c * np.exp(lg[c])
    return lin.astype(nptype), lg.astype(nptype)


def _edge_safe_bins(t):
    """Bins of the float64 bin values ``t``: the minimum site is exactly
    0 and the maximum site exactly FH_BINS (clipped into the top bin);
    every other value keeps 0.2 from an integer, ten thousand times the
    float32 kernel's worst error (four roundings of 2^-24 on values
    below FH_BINS * max|f| / (max - min) < 200)."""
    t = t.ravel()
    ends = (t == 0.0) | (t == float(FH_BINS))
    assert ends.sum() == 2 and t.min() == 0.0 and t.max() == FH_BINS
    inner = t[~ends]
    assert np.all(np.abs(inner - np.round(inner)) >= 0.2)
    b = np.clip(np.trunc(t), 0, FH_BINS - 1).astype(np.int64)
    hist = np.bincount(b, minlength=FH_BINS)
    assert hist[0] >= 1 and hist[-1] >= 1
    return hist


@pytest.mark.parametrize("tdtype", DTYPES, ids=["f64", "f32"])
def test_field_histogrammer_automatic_bounds(tdtype):
    lin, lg = _field_hist_arrays(NPTYPE[tdtype])
    decomp = ps.DomainDecomposition((1, 1, 1), H, rank_shape=A)
    fh = ps.FieldHistogrammer(decomp, FH_BINS, halo_shape=H)
    n = int(np.prod(A))
    eps = U53 if tdtype == torch.float64 else U24

    for which, arr in (("linear", lin), ("log", lg)):
        # the halo of a log-safe array must stay log-safe to no one: it
        # is never read, so any finite non-zero filler does
        out = fh(_dev(_pad(arr)))
        assert fh._hip_kernel.dtype == tdtype
        other = "log" if which == "linear" else "linear"
        for c in range(2):
            w = arr[c].astype(np.float64)
            mn, mx = w.min(), w.max()
            lw = np.log(np.abs(w))
            lmn, lmx = lw.min(), lw.max()
            if which == "linear":
                t = (w - mn) / (mx - mn) * FH_BINS
            else:
                t = (lw - lmn) / (lmx - lmn) * FH_BINS
            ref = _edge_safe_bins(t)
            assert np.array_equal(out[which][c], ref), (which, c)
            assert out[other][c].sum() == n, (other, c)
            assert np.array_equal(
                out["linear_bins"][c], np.linspace(mn, mx, FH_BINS + 1))
            # the device's log and numpy's are each within an ulp of the
            # fields' type: the edges agree to that, relative
            want = np.exp(np.linspace(lmn, lmx, FH_BINS + 1))
            rtol = 4 * eps * max(abs(lmn), abs(lmx), 1.0) + 4 * U53
            assert np.all(np.abs(out["log_bins"][c] - want)
                          <= rtol * want), (which, c)


# ---------------------------------------------------------------------------
# spectra_bin

N_SMALL = 1000                      # four blocks, the last one partial
N_STRIDE = 4096 * 256 + 77          # above the 4096-block cap


@functools.lru_cache(maxsize=None)
def _spectra_inputs(n):
    rng = np.random.default_rng(107)
    fk = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    w = 0.5 + rng.random(n)
    return fk, w


@pytest.mark.parametrize("num_bins", [37, 700, 4096])
@pytest.mark.parametrize("n", [N_SMALL, N_STRIDE])
def test_spectra_bin_direct(n, num_bins):
    fk, w = _spectra_inputs(n)
    rng = np.random.default_rng(108 + num_bins)
    bidx = rng.integers(0, num_bins, size=n).astype(np.int32)
    bidx[0], bidx[n // 2], bidx[n - 1] = 0, num_bins - 1, num_bins - 1
    got = hip.spectra_bin(_dev(fk), _dev(w), _dev(bidx), num_bins)
    assert got.dtype == torch.float64 and got.shape == (num_bins,)
    got = got.cpu().numpy()

    terms = w * (fk.real**2 + fk.imag**2)
    ref = np.bincount(bidx, weights=terms, minlength=num_bins)
    count = np.bincount(bidx, minlength=num_bins)
    assert count[0] >= 1 and count[-1] >= 2
    # count adds and the term's own roundings; terms are positive
    bound = (count + 4) * U53 * ref
    err = np.abs(got - ref)
    print("spectra_bin", n, num_bins, "worst err/bound",
          np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), int(np.argmax(err - bound))
    assert np.all(got[count == 0] == 0)


SPEC_GRID = (12, 10, 14)
SPEC_LENGTHS = (5., 3., 7.)


def _bin_power_reference(fk, k_power):
    """numpy transcription of the binned |f_k|^2 k^n with r2c weights;
    returns (spectrum, modes per bin)."""
    dk = [2 * np.pi / li for li in SPEC_LENGTHS]
    kx = np.fft.fftfreq(12, 1 / 12)
    ky = np.fft.fftfreq(10, 1 / 10)
    kx[6], ky[5] = 6, 5
    kz = np.arange(8.)
    kmag = np.sqrt((dk[0] * kx[:, None, None])**2
                   + (dk[1] * ky[None, :, None])**2
                   + (dk[2] * kz[None, None, :])**2)
    counts = np.full(kmag.shape, 2.)
    counts[:, :, 0] = 1.
    counts[:, :, 7] = 1.
    bw = min(dk)
    num_bins = int(kmag.max() / bw + .5) + 1
    b = np.round(kmag / bw).astype(np.int64).ravel()
    assert b.max() == num_bins - 1
    bin_counts = np.bincount(b, weights=counts.ravel(), minlength=num_bins)
    terms = (counts * kmag**k_power * np.abs(fk)**2).ravel()
    ref = np.bincount(b, weights=terms, minlength=num_bins)
    nterm = np.bincount(b, minlength=num_bins)
    assert nterm.min() >= 1
    return ref / bin_counts, nterm


def test_bin_power_anisotropic_box(monkeypatch):
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=SPEC_GRID)
    fft = DFT(decomp, grid_shape=SPEC_GRID, dtype=np.float64,
              device="cuda")
    dk = tuple(2 * np.pi / li for li in SPEC_LENGTHS)
    spectra = ps.PowerSpectra(decomp, fft, dk, float(np.prod(SPEC_LENGTHS)))
    kshape = fft.shape(True)
    assert kshape == (12, 10, 8)
    rng = np.random.default_rng(109)
    fk = rng.standard_normal(kshape) + 1j * rng.standard_normal(kshape)

    calls = []
    real_spectra_bin = hip.spectra_bin

    def spy(*args, **kwargs):
        calls.append(1)
        return real_spectra_bin(*args, **kwargs)

    monkeypatch.setattr(hip, "spectra_bin", spy)
    for k_power in (3, 0):
        ref, nterm = _bin_power_reference(fk, k_power)
        assert spectra.num_bins == len(ref)
        got = spectra.bin_power(_dev(fk), k_power=k_power)
        # the kernel's count + 4, and four more roundings for k^n, the
        # mode count and the division by the bin's weight; terms are
        # positive
        bound = (nterm + 8) * U53 * ref
        assert np.all(np.abs(got - ref) <= bound), k_power
    assert len(calls) == 2

    # complex64 modes take the torch branch: |f_k|^2 is then formed in
    # float32 (hypot, square: four roundings, taken as 8)
    fk32 = fk.astype(np.complex64)
    ref, nterm = _bin_power_reference(fk32.astype(np.complex128), 3)
    got = spectra.bin_power(_dev(fk32), k_power=3)
    assert len(calls) == 2, "complex64 reached spectra_bin"
    bound = ((nterm + 8) * U53 + 8 * U24) * ref
    assert np.all(np.abs(got - ref) <= bound)


# ---------------------------------------------------------------------------
# transverse-traceless projection on the matrix cores

TT_SMALL = (6, 5, 4)        # 90 k-sites: last wave holds two live sites
TT_LARGE = (96, 96, 114)    # 534 528 k-sites = 33 408 blocks: gy = 2
GUARD = 4096


def _projector(grid):
    lengths = (5., 3., 7.)
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    fft = DFT(decomp, grid_shape=grid, dtype=np.float64, device="cuda")
    dk = tuple(2 * np.pi / li for li in lengths)
    dx = tuple(li / n for li, n in zip(lengths, grid))
    return ps.Projector(fft, 1, dk, dx), fft.shape(True)


def _tt_reference(hij, eff):
    """(P_ac P_db - P_ab P_cd / 2) h_cd with P = 1 - khat khat^T, zero
    where k = 0; hij is [6, nkx, nky, nkz] in numpy."""
    kshape = hij.shape[1:]
    k = np.stack(np.broadcast_arrays(
        eff[0][:, None, None], eff[1][None, :, None],
        eff[2][None, None, :])).reshape(3, -1)
    ksq = (k**2).sum(axis=0)
    zero = ksq == 0
    khat = k / np.sqrt(np.where(zero, 1.0, ksq))
    P = np.eye(3)[:, :, None] - khat[:, None, :] * khat[None, :, :]
    sym = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    h = hij.reshape(6, -1)
    Hm = np.empty((3, 3, h.shape[1]), dtype=np.complex128)
    for a in range(3):
        for b in range(3):
            Hm[a, b] = h[sym[(min(a, b), max(a, b))]]
    php = np.einsum("acn,cbn->abn", P, np.einsum("cdn,dbn->cbn", Hm, P))
    tr = np.einsum("cdn,cdn->n", P, Hm)
    res = php - 0.5 * P * tr[None, None, :]
    res[:, :, zero] = 0
    out = np.stack([res[a, b] for (a, b) in sorted(sym, key=sym.get)])
    return out.reshape((6,) + tuple(kshape)), int(zero.sum())


@functools.lru_cache(maxsize=None)
def _tt_case(grid):
    proj, kshape = _projector(grid)
    rng = np.random.default_rng(110)
    hij = (rng.standard_normal((6,) + kshape)
           + 1j * rng.standard_normal((6,) + kshape))
    eff = [proj.eff_mom[n].cpu().numpy()
           for n in ("eff_mom_x", "eff_mom_y", "eff_mom_z")]
    want, nzero = _tt_reference(hij, eff)
    assert nzero >= 1
    return proj, kshape, hij, want


def _check_tt(got, want):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err < 1e-12 * max(scale, 1.0), (err, scale)
    tr = got[0] + got[3] + got[5]
    assert np.abs(tr).max() < 1e-11 * max(scale, 1.0)


@pytest.mark.parametrize("grid", [TT_SMALL, TT_LARGE], ids=["90", "534528"])
def test_tt_in_place(grid):
    proj, kshape, hij, want = _tt_case(grid)
    vol = int(np.prod(kshape))
    assert vol % 16 != 0 or -(-vol // 16) > 32768
    got = _dev(hij)
    ret = proj.transverse_traceless(got)
    assert ret is got
    torch.cuda.synchronize()
    _check_tt(got.cpu().numpy(), want)


@pytest.mark.parametrize("grid", [TT_SMALL, TT_LARGE], ids=["90", "534528"])
def test_tt_out_of_place_between_guards(grid):
    proj, kshape, hij, want = _tt_case(grid)
    vol = int(np.prod(kshape))
    src = _dev(hij)
    sentinel = complex(-7.25, 3.5)
    flat = torch.full((6 * vol + 2 * GUARD,), sentinel,
                      dtype=torch.complex128, device="cuda")
    out = flat[GUARD:GUARD + 6 * vol].view((6,) + tuple(kshape))
    assert out.is_contiguous()
    ret = proj.transverse_traceless(hij=src, hij_TT=out)
    assert ret is out
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), hij), "input was written"
    flat_h = flat.cpu()
    assert bool((flat_h[:GUARD] == sentinel).all())
    assert bool((flat_h[-GUARD:] == sentinel).all())
    _check_tt(out.cpu().numpy(), want)


def test_tt_guards_keep_bad_arguments_from_the_kernel(monkeypatch):
    proj, kshape, hij, _ = _tt_case(TT_SMALL)
    reached = []

    def record(*args):
        reached.append(args)
        raise AssertionError("bad arguments reached tt_project")

    monkeypatch.setattr(hip.ext(), "tt_project", record)
    src = _dev(hij)
    # a CPU output for a device input
    with pytest.raises(Exception):
        proj.transverse_traceless(
            hij=src, hij_TT=torch.zeros((6,) + kshape,
                                        dtype=torch.complex128))
    # a complex64 output is filled by the torch path, in its precision
    out32 = torch.zeros((6,) + kshape, dtype=torch.complex64, device="cuda")
    proj.transverse_traceless(hij=src, hij_TT=out32)
    want = _tt_case(TT_SMALL)[3]
    assert np.abs(out32.cpu().numpy() - want).max() \
        < 1e-5 * max(np.abs(want).max(), 1.0)
    # the wrong trailing shape
    wrong = torch.zeros((6, 6, 5, 4), dtype=torch.complex128,
                        device="cuda")
    with pytest.raises(Exception):
        proj.transverse_traceless(wrong)
    # five components
    with pytest.raises(Exception):
        proj.transverse_traceless(src[:5].contiguous())
    assert not reached


# ---------------------------------------------------------------------------
# jit_launch

def test_jit_launch_refuses_an_integer_beyond_int():
    n, num_bins = 1000, 37
    fk, w = _spectra_inputs(n)
    bidx = _dev(np.zeros(n, dtype=np.int32))
    hip.spectra_bin(_dev(fk), _dev(w), bidx, num_bins)
    key = hip._spectra_bin_cache[num_bins]
    fk_d, w_d = _dev(fk), _dev(w)
    hist = torch.zeros(num_bins, dtype=torch.float64, device="cuda")
    ptrs = [fk_d.data_ptr(), w_d.data_ptr(), bidx.data_ptr(),
            hist.data_ptr()]
    stream = torch.cuda.current_stream().cuda_stream
    for bad in (2**31, -2**31 - 1):
        with pytest.raises(OverflowError):
            hip.ext().jit_launch(key, 4, 1, 1, 256, 1, 1, 0, stream, ptrs,
                                 [bad], [])
    torch.cuda.synchronize()
    assert float(hist.sum()) == 0.0, "something was launched"
    assert "int n)" in hip.SPECTRA_BIN_SRC
