"""The ``precision`` keyword of SpectralCollocator and
SpectralPoissonSolver on the CPU, where ``"native"`` is the torch form
of its definition: the default is untouched, a float64 transform does
not see the keyword, complex64 modes stay complex64 up to the inverse
transform, and the results are as close to the float64 classes as the
promoting chain's.
"""

import numpy as np
import pytest
import torch

import pystella_amd as ps
from pystella_amd.backend import hip
from pystella_amd.derivs import SecondCenteredDifference
from tests.kspace_c64_reference import (
    CASES, assert_end_to_end, dk, dx, make_collocator, make_fft,
    make_solver, run_all)


@pytest.fixture(autouse=True)
def no_kernels(monkeypatch):
    def _raise(*args, **kwargs):
        raise AssertionError("the CPU path reached a fused k-space kernel")
    for name in ("kspace_derivs", "kspace_div_accum", "kspace_poisson",
                 "kspace_derivs_c64", "kspace_div_accum_c64",
                 "kspace_poisson_c64"):
        monkeypatch.setattr(hip, name, _raise)


def assert_same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].abs().max() > 0, name
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64],
                         ids=["float32", "float64"])
def test_promote_is_the_default(dtype):
    coll = make_collocator("12x10x14", "cpu", dtype)
    solver = make_solver("12x10x14", "cpu", dtype)
    assert coll.precision == solver.precision == "promote"
    assert_same(run_all("12x10x14", "cpu", dtype),
                run_all("12x10x14", "cpu", dtype, precision="promote"))


def test_native_on_a_float64_transform_is_promote():
    coll = make_collocator("12x10x14", "cpu", np.float64, precision="native")
    solver = make_solver("12x10x14", "cpu", np.float64, precision="native")
    assert coll.precision == solver.precision == "native"
    assert_same(run_all("12x10x14", "cpu", np.float64, precision="native"),
                run_all("12x10x14", "cpu", np.float64))


@pytest.mark.parametrize("make", [make_collocator, make_solver])
def test_other_precisions_are_refused(make):
    for bad in ("fast", None, "Native", torch.float32):
        with pytest.raises(ValueError, match="precision"):
            make("12x10x14", "cpu", np.float32, precision=bad)


def test_precision_is_keyword_only():
    fft = make_fft("12x10x14", "cpu", np.float32)
    with pytest.raises(TypeError):
        ps.SpectralCollocator(fft, dk(), "native")
    with pytest.raises(TypeError):
        ps.SpectralPoissonSolver(
            fft, dk(), dx(), SecondCenteredDifference(1).get_eigenvalues,
            "native")


@pytest.mark.parametrize("precision,cdtype", [
    ("native", torch.complex64), ("promote", torch.complex128)])
def test_the_inverse_transform_sees(precision, cdtype, monkeypatch):
    """Every mode array handed to ``fft.idft`` on a float32 transform."""
    from pystella_amd.fourier.dft import BaseDFT
    seen = []
    idft = BaseDFT.idft

    def spy(self, fk=None, fx=None):
        seen.append(fk.dtype)
        return idft(self, fk, fx)

    monkeypatch.setattr(BaseDFT, "idft", spy)
    out = run_all("12x10x14", "cpu", np.float32, precision=precision)
    # lap + grd on two slices, the tuple gradient on two, four single
    # outputs, two divergences, two solves
    assert len(seen) == 8 + 6 + 4 + 2 + 2
    assert set(seen) == {cdtype}
    assert all(v.dtype == torch.float32 for v in out.values())


@pytest.mark.parametrize("case", list(CASES))
def test_native_is_as_accurate_as_promote(case):
    """Every call form of the collocator and the solve for both masses
    (run_all asserts float32 outputs and unmodified inputs)."""
    native = run_all(case, "cpu", np.float32, precision="native")
    # the default-constructed objects: the unchanged promoting chain
    promote = run_all(case, "cpu", np.float32)
    assert_end_to_end(native, promote, case, "cpu")
    # the call forms agree among themselves
    assert torch.equal(native["grd"], native["grd_tuple"])
    for mu, name in enumerate(("pdx", "pdy", "pdz")):
        assert torch.equal(native[name + "_only"], native["grd"][1, mu])
    assert torch.equal(native["lap_only"],
                       native["lap"][1][1:-1, 1:-1, 1:-1])
