"""What the KSpaceMap tests share: the cases (statements, inputs as they
are stored, numpy transcriptions of the wanted values) and the derived
tolerance.

The tolerance per real component of a stored value is

    u_store * |want| + 16 * n * 2^-53 * mag

where ``n`` is the number of operation and call nodes of the expression
tree (a temporary counts where it is used), ``u_store`` is 2^-24 for a
float32 or complex64 target and 0 for a double one, and ``mag`` is the
*magnitude* evaluation of the same tree: every leaf replaced by its
modulus, every subtraction an addition, a quotient mag(num)/|den|,
exp(z) as exp(Re z).  Sixteen roundoffs per node: a complex product is
within sqrt(5) u normwise and the textbook complex quotient within about
7 u, and an exp whose argument has |z| <= 4 amplifies its argument's
error by |z|.  The inputs keep every denominator a leaf of modulus >=
0.5, every exp argument within |z| <= 4 and every modulus far from
overflow.  Nothing is fitted to what the code under test gives.

``evaluate`` walks the expression tree with numpy, independently of the
torch evaluator and of the code generator; each case's ``want`` is a
hand transcription, and the CPU tests hold the two against each other.
"""

import functools

import numpy as np

from pystella_amd.field import (
    Call, Comparison, Field, If, Power, Product, Quotient, Subscript, Sum,
    Variable, var)
from pystella_amd.field.expr import conj, exp, imag, real

KSHAPE = (12, 10, 8)        # 960 modes: three blocks of 256 and one of 192
SMALL = (5, 1, 3)           # 15 modes, one partial block, an extent of one
LENGTHS = (5., 3., 7.)
U = 2.0**-53
U_STORE = {np.dtype(np.complex64): 2.0**-24, np.dtype(np.float32): 2.0**-24,
           np.dtype(np.complex128): 0.0, np.dtype(np.float64): 0.0}


# ---------------------------------------------------------------------------
# the tree walker: value, magnitude and node count

def _leaf(x):
    x = np.asarray(x)
    wide = np.complex128 if np.iscomplexobj(x) else np.float64
    x = x.astype(wide)
    return x, np.abs(x), 0


def evaluate(expr, env):
    """(value, magnitude, nodes) of ``expr``.  ``env`` maps names to
    arrays or numbers as stored, temporaries to such triples."""
    if isinstance(expr, (int, float, complex)):
        return _leaf(expr)
    if isinstance(expr, Subscript):
        (idx,) = expr.index
        return _leaf(env[expr.aggregate.name][int(idx)])
    if isinstance(expr, Field):
        x = env[expr.name]
        if len(expr.indices) == 1:
            shape = [1, 1, 1]
            shape["ijk".index(expr.indices[0])] = -1
            x = np.asarray(x).reshape(shape)
        return _leaf(x)
    if isinstance(expr, Variable):
        x = env[expr.name]
        return x if isinstance(x, tuple) else _leaf(x)
    if isinstance(expr, (Sum, Product)):
        parts = [evaluate(c, env) for c in expr.children]
        val, mag, n = parts[0]
        for v, m, k in parts[1:]:
            val, mag = (val + v, mag + m) if isinstance(expr, Sum) \
                else (val * v, mag * m)
            n += k
        return val, mag, n + 1
    if isinstance(expr, Quotient):
        num, nmag, n1 = evaluate(expr.num, env)
        den, _, n2 = evaluate(expr.den, env)
        return num / den, nmag / np.abs(den), n1 + n2 + 1
    if isinstance(expr, Power):
        base, mag, n = evaluate(expr.base, env)
        e = int(expr.exponent)
        assert e == expr.exponent
        if e >= 0:
            return base**e, mag**e, n + 1
        return base**e, np.abs(base)**float(e), n + 1
    if isinstance(expr, Call):
        (arg,) = expr.args
        val, mag, n = evaluate(arg, env)
        if expr.func == "exp":
            assert (np.abs(val) <= 4).all()
            return np.exp(val), np.exp(val.real), n + 1
        fn = {"conj": np.conj, "real": np.real, "imag": np.imag,
              "abs": np.abs}[expr.func]
        return fn(val).astype(val.dtype if expr.func == "conj"
                              else np.float64), mag, n + 1
    if isinstance(expr, Comparison):
        left, right = evaluate(expr.left, env)[0], evaluate(expr.right,
                                                            env)[0]
        assert expr.op == ">"
        return left > right, None, 0
    if isinstance(expr, If):
        cond = evaluate(expr.condition, env)[0]
        tv, tm, tn = evaluate(expr.then, env)
        ev, em, en = evaluate(expr.else_, env)
        return np.where(cond, tv, ev), np.where(cond, tm, em), tn + en + 1
    raise TypeError(type(expr))


def evaluate_case(case, inputs):
    """``{(output name, component): (value, magnitude, nodes)}``, every
    statement on the inputs as they were before the call (no case reads
    what an earlier statement of it stored)."""
    env = dict(inputs)
    for lhs, rhs in case.tmp.items():
        env[lhs.name] = evaluate(rhs, env)
    out = {}
    for lhs, rhs in case.statements.items():
        name, comp = (lhs.aggregate.name, int(lhs.index[0])) \
            if isinstance(lhs, Subscript) else (lhs.name, None)
        out[name, comp] = evaluate(rhs, env)
    return out


def tolerance(want, mag, n, dtype):
    """Per real component (the same array for both)."""
    return {part: U_STORE[np.dtype(dtype)] * np.abs(getattr(want, part))
            + 16 * n * U * mag for part in ("real", "imag")}


def assert_close(got, want, mag, n, dtype, what):
    """``got`` (as stored) against ``want``; prints the worst error in
    units of the tolerance.  Two implementations are held against each
    other at this same tolerance: sixteen roundoffs per node leave room
    for both sides' double errors (a few per node each), and for a
    float32 target two doubles that close round to the same float."""
    got = np.asarray(got)
    assert got.dtype == np.dtype(dtype), (what, got.dtype)
    assert got.shape == np.broadcast_shapes(got.shape, np.shape(want)), what
    want = np.broadcast_to(want, got.shape)
    mag = np.broadcast_to(mag, got.shape)
    tol = tolerance(want.astype(np.complex128), mag, n, dtype)
    parts = ("real", "imag") if np.iscomplexobj(got) else ("real",)
    if not np.iscomplexobj(got):
        assert not np.iscomplexobj(want) or (want.imag == 0).all(), what
    for part in parts:
        g = getattr(got, part).astype(np.float64)
        w = getattr(want, part).astype(np.float64)
        assert np.isfinite(g).all(), (what, part)
        err, bound = np.abs(g - w), tol[part]
        ratio = float((err[err > 0] / np.maximum(bound[err > 0],
                                                  1e-300)).max(initial=0.0))
        print(f"{what}.{part}: worst error {ratio:.3f} of the tolerance "
              f"(n = {n})")
        assert (err <= bound).all(), (what, part, ratio)


# ---------------------------------------------------------------------------
# inputs

@functools.lru_cache(maxsize=None)
def tables(kshape):
    """(k1, k2): momenta of a box of LENGTHS (the last axis half, as of a
    real transform) and the effective momenta of a centred difference."""
    k1, k2 = [], []
    for mu, (n, length) in enumerate(zip(kshape, LENGTHS)):
        dk = 2 * np.pi / length
        if mu == 2:
            ngrid, m = 2 * (n - 1) or 1, np.arange(n)
        else:
            ngrid, m = n, np.fft.fftfreq(n, 1 / n)
        k = dk * m
        dx = length / ngrid
        k1.append(k)
        k2.append(np.sin(k * dx) / dx)
    return tuple(k1), tuple(k2)


def _rng(seed, kshape):
    return np.random.default_rng([seed, *kshape])


def modes(seed, kshape, outer=()):
    rng = _rng(seed, kshape)
    shape = tuple(outer) + tuple(kshape)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def away_from_zero(seed, kshape):
    """Complex values of modulus between 0.5 and 2."""
    rng = _rng(seed, kshape)
    return rng.uniform(0.5, 2.0, kshape) \
        * np.exp(2j * np.pi * rng.uniform(size=kshape))


# ---------------------------------------------------------------------------
# the cases

_kx, _ky, _kz = (Field(n, indices=(ix,))
                 for n, ix in (("kx", "i"), ("ky", "j"), ("kz", "k")))
_fk = Field("fk")


def _b(tabs):
    return (tabs[0][:, None, None], tabs[1][None, :, None],
            tabs[2][None, None, :])


class Case:
    """``statements``/``tmp``: the map; ``forms``: ``{form: {argument:
    numpy dtype}}``; ``outputs``: ``{name: outer shape}``; ``scalars``:
    values; ``make(kshape)``: double-precision inputs; ``want(inp,
    scalars)``: ``{(output, component): array}`` transcribed by hand on
    widened inputs."""

    def __init__(self, name, statements, tmp, forms, outputs, scalars, make,
                 want):
        self.name, self.statements, self.tmp = name, statements, tmp
        self.forms, self.outputs, self.scalars = forms, outputs, scalars
        self.make, self.want = make, want

    def inputs(self, kshape, form):
        """Inputs as stored, by name: the double-precision draws rounded
        once to the form's dtypes."""
        dtypes = self.forms[form]
        return {n: np.ascontiguousarray(a.astype(dtypes[n]))
                for n, a in self.make(tuple(kshape)).items()}


def _widen(inp):
    return {n: a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)
            for n, a in inp.items()}


def _forms(double, **narrow):
    return {"double": double, "mixed": {**double, **narrow}}


C128, C64, F64, F32 = np.complex128, np.complex64, np.float64, np.float32


def _derivs():
    k1 = [Field(f"k1{a}", indices=(ix,)) for a, ix in zip("xyz", "ijk")]
    k2 = [Field(f"k2{a}", indices=(ix,)) for a, ix in zip("xyz", "ijk")]
    outs = [Field(n) for n in ("pdx", "pdy", "pdz", "lap")]
    t, inv_n = var("t"), var("inv_n")
    statements = {o: 1j * k * t for o, k in zip(outs, k1)}
    statements[outs[3]] = -(k2[0]**2 + k2[1]**2 + k2[2]**2) * t

    def make(kshape):
        t1, t2 = tables(kshape)
        inp = {"fk": modes(1, kshape)}
        inp.update({f"k1{a}": k for a, k in zip("xyz", t1)})
        inp.update({f"k2{a}": k for a, k in zip("xyz", t2)})
        return inp

    def want(inp, scalars):
        w = _widen(inp)
        tt = w["fk"] * scalars["inv_n"]
        out = {(f"pd{a}", None): 1j * q * tt
               for a, q in zip("xyz", _b([w[f"k1{a}"] for a in "xyz"]))}
        qx, qy, qz = _b([w[f"k2{a}"] for a in "xyz"])
        out["lap", None] = -(qx * qx + qy * qy + qz * qz) * tt
        return out

    tabs = {f"k{i}{a}": F64 for i in "12" for a in "xyz"}
    allc = {n: C128 for n in ("fk", "pdx", "pdy", "pdz", "lap")}
    return Case(
        "derivs", statements, {t: _fk * inv_n},
        {"double": {**allc, **tabs},
         "mixed": {**{n: C64 for n in allc}, **tabs}},
        {n: () for n in ("pdx", "pdy", "pdz", "lap")},
        {"inv_n": 1.0 / (12 * 10 * 14)}, make, want)


def _filter():
    s = var("s")

    def make(kshape):
        t1, _ = tables(kshape)
        return {"fk": modes(2, kshape), "kx": t1[0], "ky": t1[1],
                "kz": t1[2]}

    def want(inp, scalars):
        w = _widen(inp)
        kx, ky, kz = _b([w["kx"], w["ky"], w["kz"]])
        return {("fk", None):
                w["fk"] * np.exp(-(kx**2 + ky**2 + kz**2) * scalars["s"])}

    return Case(
        "filter", {_fk: _fk * exp(-(_kx**2 + _ky**2 + _kz**2) * s)}, {},
        _forms({"fk": C128, "kx": F64, "ky": F64, "kz": F64},
               fk=C64, ky=F32),
        {"fk": ()}, {"s": 0.015}, make, want)


def _phase():
    x0, y0, z0 = var("x0"), var("y0"), var("z0")
    out = Field("out")

    def make(kshape):
        t1, _ = tables(kshape)
        return {"fk": modes(3, kshape), "kx": t1[0], "ky": t1[1],
                "kz": t1[2]}

    def want(inp, scalars):
        w = _widen(inp)
        kx, ky, kz = _b([w["kx"], w["ky"], w["kz"]])
        arg = kx * scalars["x0"] + ky * scalars["y0"] + kz * scalars["z0"]
        return {("out", None): w["fk"] * (np.cos(arg) + 1j * np.sin(arg))}

    return Case(
        "phase", {out: _fk * exp(1j * (_kx * x0 + _ky * y0 + _kz * z0))}, {},
        _forms({"fk": C128, "out": C128, "kx": F64, "ky": F64, "kz": F64},
               fk=C64, kz=F32),
        {"out": ()}, {"x0": 0.1, "y0": 0.15, "z0": 0.2}, make, want)


def _conj_div():
    a, b, k2, out = Field("a"), Field("b"), Field("k2"), Field("out")

    def make(kshape):
        return {"a": modes(4, kshape), "b": away_from_zero(5, kshape),
                "k2": _rng(6, kshape).standard_normal(kshape)}

    def want(inp, scalars):
        w = _widen(inp)
        va, vb = w["a"], w["b"]
        val = np.conj(va) / vb + np.abs(va) + vb.real - 1j * va.imag
        return {("out", None): np.where(w["k2"] > 0, val, 0)}

    return Case(
        "conj_div",
        {out: If(k2 > 0, conj(a) / b + abs(a) + real(b) - 1j * imag(a), 0)},
        {}, _forms({"a": C128, "b": C128, "k2": F64, "out": C128},
                   b=C64, k2=F32, out=C64),
        {"out": ()}, {}, make, want)


def _vector():
    vk, div, out3 = Field("vk", shape=(3,)), Field("div"), \
        Field("out3", shape=(3,))

    def make(kshape):
        t1, _ = tables(kshape)
        return {"vk": modes(7, kshape, (3,)), "kx": t1[0], "ky": t1[1],
                "kz": t1[2]}

    def want(inp, scalars):
        w = _widen(inp)
        kx, ky, kz = _b([w["kx"], w["ky"], w["kz"]])
        v = w["vk"]
        return {("div", None): 1j * kx * v[0] + 1j * ky * v[1]
                + 1j * kz * v[2],
                ("out3", 1): 2 * v[2] - v[0]}

    return Case(
        "vector",
        {div: 1j * _kx * vk[0] + 1j * _ky * vk[1] + 1j * _kz * vk[2],
         out3[1]: 2 * vk[2] - vk[0]}, {},
        _forms({"vk": C128, "div": C128, "out3": C128, "kx": F64, "ky": F64,
                "kz": F64}, vk=C64, out3=C64),
        {"div": (), "out3": (3,)}, {}, make, want)


def _mixed():
    a, w_, o128, o64 = Field("a"), Field("w"), Field("o128"), Field("o64")

    def make(kshape):
        t1, _ = tables(kshape)
        return {"a": modes(8, kshape),
                "w": _rng(9, kshape).uniform(0.5, 1.5, kshape),
                "kx": t1[0], "ky": t1[1]}

    def want(inp, scalars):
        w = _widen(inp)
        kx, ky, _ = _b([w["kx"], w["ky"], w["ky"]])
        return {("o128", None): w["a"] * w["w"] * kx,
                ("o64", None): np.conj(w["a"]) * (w["w"] + ky)}

    return Case(
        "mixed", {o128: a * w_ * _kx, o64: conj(a) * (w_ + _ky)}, {},
        _forms({"a": C128, "w": F64, "kx": F64, "ky": F64, "o128": C128,
                "o64": C128}, a=C64, w=F32, o64=C64),
        {"o128": (), "o64": ()}, {}, make, want)


CASES = {c.name: c for c in (_derivs(), _filter(), _phase(), _conj_div(),
                             _vector(), _mixed())}


def expected(case, inputs, scalars=None):
    """``{(output, component): (want, magnitude, nodes)}``; the hand
    transcription is held against the tree walk at one tolerance (both
    are double evaluations of one formula)."""
    scalars = case.scalars if scalars is None else scalars
    tree = evaluate_case(case, {**inputs, **scalars})
    want = case.want(inputs, scalars)
    assert want.keys() == tree.keys()
    out = {}
    for key, (val, mag, n) in tree.items():
        w = np.asarray(want[key], dtype=np.complex128)
        bound = 16 * n * U * mag
        assert (np.abs(w.real - val.real) <= bound).all(), (case.name, key)
        assert (np.abs(w.imag - np.imag(val)) <= bound).all(), \
            (case.name, key)
        out[key] = (w, mag, n)
    return out
