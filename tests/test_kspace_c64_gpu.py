"""The complex64 k-space kernels (backend/hip.py ``kspace_derivs_c64``,
``kspace_div_accum_c64``, ``kspace_poisson_c64``) on the GPU: each
kernel against numpy on the stored modes, widened; both classes under
``precision="native"`` against the promoting chain and the float64 CPU
classes; the routing; and the argument checks.

Shapes are those of tests/test_kspace_gpu.py: k-shape (12, 10, 8) is 960
modes, three full blocks of 256 and a partial one, with all three
extents and box lengths different.
"""

import numpy as np
import pytest
import torch

from pystella_amd.backend import hip
from tests.kspace_c64_reference import (
    CASES, GRAD, GRID, INV_N, KSHAPE, OUTS, VOLK, assert_end_to_end,
    assert_stored, class_inputs, make_collocator, make_solver,
    mode_data_c64, run_all, run_collocator, run_poisson, tables,
    want_derivs, want_div_term, want_poisson)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]

C128 = ("kspace_derivs", "kspace_div_accum", "kspace_poisson")
C64 = tuple(name + "_c64" for name in C128)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


class Guarded:
    """A complex64 k-space output that ends one block before its
    allocation does: a store past VOLK lands in the NaN-filled tail."""

    def __init__(self):
        self.buf = torch.full((VOLK + 256,), complex("nan+nanj"),
                              dtype=torch.complex64, device="cuda")
        self.out = self.buf[:VOLK].view(KSHAPE)

    def untouched(self):
        return bool(torch.isnan(self.buf.real).all()
                    and torch.isnan(self.buf.imag).all())

    def tail_untouched(self):
        tail = self.buf[VOLK:]
        return bool(torch.isnan(tail.real).all()
                    and torch.isnan(tail.imag).all())

    def numpy(self):
        return self.out.cpu().numpy()


# -- 1. kernels against numpy

@pytest.mark.parametrize(
    "mask", [("pdx",), ("pdy",), ("pdz",), ("lap",), GRAD, GRAD + ("lap",)],
    ids="+".join)
def test_derivs_kernel_against_numpy(mask):
    k1, k2, _ = tables()
    fk = mode_data_c64(1)
    fk_d = _dev(fk)
    assert fk_d.dtype == torch.complex64
    fk_before = fk_d.clone()
    bufs = {name: Guarded() for name in OUTS}
    hip.kspace_derivs_c64(fk_d, {name: bufs[name].out for name in mask},
                          [_dev(k) for k in k1], [_dev(k) for k in k2],
                          INV_N)
    torch.cuda.synchronize()
    want = want_derivs(fk)
    # the k1 tables hold zeros (k = 0 and Nyquist): those outputs are 0
    assert any((want[name] == 0).any() for name in GRAD)
    for name in OUTS:
        if name in mask:
            assert_stored(bufs[name].numpy(), want[name], name)
            assert bufs[name].tail_untouched(), name
        else:
            assert bufs[name].untouched(), name
    assert torch.equal(fk_d, fk_before)


def test_div_accum_kernel_against_numpy():
    k1, _, _ = tables()
    div = Guarded()
    for mu in range(3):
        fk = mode_data_c64(10 + mu)
        fk_d = _dev(fk)
        want = want_div_term(fk, mu)
        if mu > 0:
            # what the last launch stored, read back and widened
            want = div.numpy().astype(np.complex128) + want
        hip.kspace_div_accum_c64(fk_d, div.out, _dev(k1[mu]), mu, INV_N,
                                 accumulate=mu > 0)
        torch.cuda.synchronize()
        assert_stored(div.numpy(), want, f"div launch {mu}")
        assert torch.equal(fk_d, _dev(fk))
    assert div.tail_untouched()


@pytest.mark.parametrize("m2", [0.0, 1.7])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in_place"])
def test_poisson_kernel_against_numpy(m2, in_place):
    eig = tables()[2]
    assert all((e <= 0).all() for e in eig) and eig[0][0] == 0
    rhok = mode_data_c64(20)
    rhok_d = _dev(rhok)
    sol = Guarded()
    if in_place:
        sol.out.copy_(rhok_d)
        rhok_d = sol.out
    hip.kspace_poisson_c64(rhok_d, sol.out, *[_dev(e) for e in eig], INV_N,
                           m2)
    torch.cuda.synchronize()
    want = want_poisson(rhok, m2)
    assert want[0, 0, 0] == 0 and rhok[0, 0, 0] != 0
    assert_stored(sol.numpy(), want, f"poisson m2={m2}")
    assert sol.tail_untouched()
    if not in_place:
        assert torch.equal(rhok_d, _dev(rhok))


# -- 2. classes on the GPU

@pytest.mark.parametrize("case", list(CASES))
def test_native_is_as_accurate_as_promote(case, monkeypatch):
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    native = run_all(case, "cuda", np.float32, precision="native")
    # the default-constructed objects: the unchanged promoting chain
    promote = run_all(case, "cuda", np.float32)
    assert_end_to_end(native, promote, case, "cuda")
    # the array, tuple and single-output forms agree among themselves
    assert torch.equal(native["grd"], native["grd_tuple"])
    for mu, name in enumerate(GRAD):
        assert torch.equal(native[name + "_only"], native["grd"][1, mu])
    assert torch.equal(native["lap_only"],
                       native["lap"][1][1:-1, 1:-1, 1:-1])


# -- 3. routing

@pytest.fixture
def launches(monkeypatch):
    """Counts of the six entry points' calls."""
    counts = dict.fromkeys(C128 + C64, 0)
    for name in counts:
        def counted(*args, _name=name, _fn=getattr(hip, name), **kwargs):
            counts[_name] += 1
            return _fn(*args, **kwargs)
        monkeypatch.setattr(hip, name, counted)
    monkeypatch.delenv("PYSTELLA_KSPACE", raising=False)
    return counts


def _zero(names):
    return dict.fromkeys(names, 0)


def test_native_float32_runs_the_c64_kernels(launches):
    coll = make_collocator("12x10x14", "cuda", np.float32,
                           precision="native")
    fx, vec, _ = (t.to("cuda", torch.float32)
                  for t in class_inputs("12x10x14"))
    lap = torch.zeros_like(fx)
    grd = torch.zeros((2, 3) + GRID, dtype=torch.float32, device="cuda")
    coll(fx=fx, lap=lap, grd=grd)
    assert launches == {**_zero(C128 + C64), "kspace_derivs_c64": 2}
    # the scratch is four complex64 buffers, reused from here on
    assert len(coll._scratch) == 4
    assert all(b.dtype == torch.complex64 and b.shape == KSHAPE
               for b in coll._scratch)
    ptrs = [b.data_ptr() for b in coll._scratch]
    div = torch.zeros((2,) + GRID, dtype=torch.float32, device="cuda")
    coll.divergence(vec=vec, div=div)
    assert launches == {**_zero(C128 + C64), "kspace_derivs_c64": 2,
                        "kspace_div_accum_c64": 6}
    coll(fx=fx, lap=lap)
    coll.divergence(vec=vec, div=div)
    assert [b.data_ptr() for b in coll._scratch] == ptrs
    assert len(coll._scratch) == 4

    solver = make_solver("12x10x14", "cuda", np.float32, precision="native")
    first = run_poisson("12x10x14", "cuda", np.float32, solver=solver)
    assert launches["kspace_poisson_c64"] == 2       # one per mass
    assert not any(launches[name] for name in C128)
    # a new mass compiles nothing
    entries = set(hip._kspace_cache)
    assert any(key[0] == "poisson" and "complex64" in key for key in entries)
    rho = class_inputs("12x10x14")[2].to("cuda", torch.float32)
    f = torch.zeros_like(fx[0])
    solver(fx=f, rho=rho, m_squared=0.3)
    assert launches["kspace_poisson_c64"] == 3
    assert set(hip._kspace_cache) == entries
    assert not torch.equal(f.cpu(), first["poisson m2=1.7"])


def test_one_poisson_launch_per_solve(launches):
    solver = make_solver("12x10x14", "cuda", np.float32, precision="native")
    rho = class_inputs("12x10x14")[2].to("cuda", torch.float32)
    f = torch.zeros(tuple(n + 2 for n in GRID), dtype=torch.float32,
                    device="cuda")
    solver(fx=f, rho=rho, m_squared=1.7)
    assert launches == {**_zero(C128 + C64), "kspace_poisson_c64": 1}


def test_default_float32_launches_nothing(launches):
    run_all("12x10x14", "cuda", np.float32)
    run_all("12x10x14", "cuda", np.float32, precision="promote")
    assert launches == _zero(C128 + C64)


def test_native_float64_runs_the_complex128_kernels(launches):
    native = run_all("12x10x14", "cuda", np.float64, precision="native")
    counts = dict(launches)
    assert counts["kspace_derivs"] > 0 and counts["kspace_div_accum"] == 6
    assert counts["kspace_poisson"] == 2
    assert not any(counts[name] for name in C64)
    default = run_all("12x10x14", "cuda", np.float64)
    assert launches == {k: 2 * v for k, v in counts.items()}
    for name in default:
        assert torch.equal(native[name], default[name]), name


def test_knob_forces_the_torch_form(launches, monkeypatch):
    fused = run_all("12x10x14", "cuda", np.float32, precision="native")
    assert launches["kspace_derivs_c64"] > 0
    before = dict(launches)
    monkeypatch.setenv("PYSTELLA_KSPACE", "0")
    chain = run_all("12x10x14", "cuda", np.float32, precision="native")
    assert launches == before
    # the same double expressions and the same inverse transform: a
    # difference is a last-bit difference of a few stored modes
    for name in fused:
        scale = fused[name].abs().max().item()
        diff = (chain[name] - fused[name]).abs().max().item()
        print(f"torch form against kernels, {name}: max diff {diff:.3e} "
              f"at magnitude {scale:.3e}")
        assert diff <= 4 * 2.0**-24 * scale, (name, diff, scale)


def test_a_strided_fk_takes_the_torch_form(launches):
    coll = make_collocator("12x10x14", "cuda", np.float32,
                           precision="native")
    want = run_collocator("12x10x14", "cuda", np.float32, coll=coll)
    before = dict(launches)
    assert before["kspace_derivs_c64"] > 0
    fk = coll.fft.fk
    coll.fft.fk = torch.empty((KSHAPE[0], KSHAPE[1], 2 * KSHAPE[2]),
                              dtype=fk.dtype, device="cuda")[:, :, ::2]
    got = run_collocator("12x10x14", "cuda", np.float32, coll=coll)
    assert launches == before
    for name in want:
        scale = want[name].abs().max().item()
        assert (got[name] - want[name]).abs().max().item() \
            <= 4 * 2.0**-24 * scale, name


# -- 4. refusals

class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"the native module's {name} was reached")


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(hip, "ext", _NoLaunch)


def _good():
    k1, k2, eig = tables()
    return {"fk": _dev(mode_data_c64(1)),
            "out": torch.zeros(KSHAPE, dtype=torch.complex64,
                               device="cuda"),
            "k1": [_dev(k) for k in k1], "k2": [_dev(k) for k in k2],
            "eig": [_dev(e) for e in eig]}


def _calls(a):
    return {
        "derivs": lambda: hip.kspace_derivs_c64(
            a["fk"], {"pdx": a["out"]}, a["k1"], a["k2"], INV_N),
        "div_accum": lambda: hip.kspace_div_accum_c64(
            a["fk"], a["out"], a["k1"][0], 0, INV_N, False),
        "poisson": lambda: hip.kspace_poisson_c64(
            a["fk"], a["out"], *a["eig"], INV_N, 0.0),
    }


OUT_NAMES = {"derivs": "pdx", "div_accum": "div_k", "poisson": "sol"}
TABLE_NAMES = {"derivs": r"k1\[0\]", "div_accum": "k1_mu", "poisson": "ex"}


@pytest.mark.parametrize("op", ["derivs", "div_accum", "poisson"])
def test_wrong_dtypes_are_refused(op, no_launch):
    a = _good()
    a["fk"] = a["fk"].to(torch.complex128)
    with pytest.raises(TypeError,
                       match="(fk|rhok) has dtype torch.complex128"):
        _calls(a)[op]()
    a = _good()
    a["out"] = a["out"].to(torch.complex128)
    with pytest.raises(
            TypeError,
            match=f"{OUT_NAMES[op]} has dtype torch.complex128"):
        _calls(a)[op]()
    a = _good()
    for key in ("k1", "k2", "eig"):
        a[key][0] = a[key][0].float()
    with pytest.raises(
            TypeError,
            match=f"{TABLE_NAMES[op]} has dtype torch.float32"):
        _calls(a)[op]()


@pytest.mark.parametrize("op", ["derivs", "div_accum", "poisson"])
def test_wrong_shapes_are_refused(op, no_launch):
    a = _good()
    a["out"] = torch.zeros(KSHAPE[::-1], dtype=torch.complex64,
                           device="cuda")
    with pytest.raises(ValueError,
                       match=f"{OUT_NAMES[op]} has shape"):
        _calls(a)[op]()
    a = _good()
    a["fk"] = a["fk"].reshape(-1)
    with pytest.raises(ValueError, match="(fk|rhok) has shape"):
        _calls(a)[op]()
    a = _good()
    for key in ("k1", "k2", "eig"):
        a[key][0] = a[key][0][:-1].contiguous()
    with pytest.raises(ValueError, match=f"{TABLE_NAMES[op]} has shape"):
        _calls(a)[op]()


@pytest.mark.parametrize("op", ["derivs", "div_accum"])
def test_output_aliasing_fk_is_refused(op, no_launch):
    a = _good()
    a["out"] = a["fk"]
    with pytest.raises(ValueError, match="aliases fk"):
        _calls(a)[op]()


def test_the_complex128_entry_points_still_refuse_complex64(no_launch):
    a = _good()
    with pytest.raises(TypeError, match="fk has dtype torch.complex64; the "
                                        "k-space kernels take complex128"):
        hip.kspace_derivs(a["fk"], {"pdx": a["out"]}, a["k1"], a["k2"],
                          INV_N)
