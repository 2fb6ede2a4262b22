"""Lower pystella_amd symbolic statements to HIP C++ source.

The emitted scalar code is spliced into hand-written CDNA4 kernel
templates (grid-stride elementwise map, hierarchical reduction, LDS
histogram — see ``backend/hip.py``) and compiled with hiprtc by the
native runtime (``csrc/module.cpp``).  This replaces the reference's
loopy→OpenCL codegen (reference: pystella/elementwise.py:164-298) with
direct CDNA4 source generation: grid geometry, halos and outer shapes
are baked in as compile-time constants; only array pointers and runtime
scalars are kernel arguments.
"""

from __future__ import annotations

import numbers

from pystella_amd.field import (
    Field, Variable, Subscript, Sum, Product, Quotient, Power, Call,
    Comparison, If, is_number,
)

_C_FUNCS = {
    "sin": "sin", "cos": "cos", "tan": "tan", "exp": "exp", "log": "log",
    "sqrt": "sqrt", "tanh": "tanh", "sinh": "sinh", "cosh": "cosh",
    "fabs": "fabs", "fmin": "fmin", "fmax": "fmax", "min": "fmin",
    "max": "fmax", "round": "round",
}


def _c_double(x):
    # literal as a functional cast so that float-mode kernels
    # (``using real = float``) do not silently promote to double
    return f"real({float(x)!r})"


class Codegen:
    """Expression → C emitter with field/scalar argument discovery.

    ``field_args``: list of FieldArg (declaration order = pointer
    argument order).  Scalar parameters (plain Variables and non-spatial
    Field accesses) are collected into ``self.scalars`` in first-use
    order; each entry is ``(c_name, value_key)`` where ``value_key`` is
    ``name`` or ``(name, idx_tuple)``.
    """

    def __init__(self, field_args, halo, rank_shape, tmp_names=()):
        self.field_specs = {fa.name: fa for fa in field_args}
        self.halo = halo
        self.rank_shape = rank_shape
        self.scalars = []           # [(c_name, value_key)]
        self._scalar_index = {}
        self.tmp_names = set(tmp_names)
        # spelling of the literal one in x**0 and x**-n; kernels that
        # must not promote a float expression set it to "real(1.0)"
        self.one = "1.0"

    def scalar_param(self, name, idx=()):
        key = (name, tuple(idx)) if idx else name
        if key in self._scalar_index:
            return self._scalar_index[key]
        c_name = name if not idx else name + "_" + "_".join(map(str, idx))
        c_name = "s_" + c_name
        # cache the real()-wrapped form so repeated references evaluate
        # in the kernel's real type consistently (scalars are passed as
        # double args; in float kernels an unwrapped later use would
        # silently promote the expression to double)
        self._scalar_index[key] = f"real({c_name})"
        self.scalars.append((c_name, key))
        return self._scalar_index[key]

    # ------------------------------------------------------------------
    def field_access(self, f: Field, outer_idx):
        if not f.is_spatial:
            return self.scalar_param(f.name, outer_idx)
        spec = self.field_specs[f.name]
        # linearize outer index over the field's outer shape
        outer_lin = 0
        for n, ix in zip(spec.outer_shape, outer_idx):
            outer_lin = outer_lin * n + int(ix)
        sx, sy, sz = f.shift
        if spec.padded:
            off = (f"((((long)(i+H+({sx})))*PSY + (j+H+({sy})))*PSZ"
                   f" + (k+H+({sz})))")
            if outer_lin:
                off = f"({outer_lin}L*PVOL + {off})"
        else:
            if any(f.shift):
                raise ValueError(
                    f"stencil shift on unpadded field {f.name}")
            off = "(((long)i*NY + j)*NZ + k)"
            if outer_lin:
                off = f"({outer_lin}L*UVOL + {off})"
        return f"{f.name}[{off}]"

    def emit(self, expr):
        if is_number(expr):
            if isinstance(expr, complex):
                raise NotImplementedError("complex JIT expressions")
            return _c_double(expr)
        if isinstance(expr, Field):
            return self.field_access(expr, ())
        if isinstance(expr, Subscript):
            agg = expr.aggregate
            idx = tuple(int(i) if is_number(i) else i for i in expr.index)
            if isinstance(agg, Field):
                return self.field_access(agg, idx)
            if isinstance(agg, Variable):
                return self.scalar_param(agg.name, idx)
            raise TypeError(f"cannot subscript {type(agg)}")
        if isinstance(expr, Variable):
            if expr.name in self.tmp_names:
                return expr.name
            return self.scalar_param(expr.name)
        if isinstance(expr, Sum):
            return "(" + " + ".join(self.emit(c) for c in expr.children) \
                + ")"
        if isinstance(expr, Product):
            return "(" + "*".join(self.emit(c) for c in expr.children) + ")"
        if isinstance(expr, Quotient):
            return f"({self.emit(expr.num)} / {self.emit(expr.den)})"
        if isinstance(expr, Power):
            base = self.emit(expr.base)
            if is_number(expr.exponent) and \
                    isinstance(expr.exponent, numbers.Integral):
                n = int(expr.exponent)
                if n == 0:
                    return self.one
                if 1 <= n <= 8:
                    return "ps_pow" + str(n) + f"({base})"
                if -8 <= n < 0:
                    return f"({self.one}/ps_pow{-n}({base}))"
            return f"pow({base}, {self.emit(expr.exponent)})"
        if isinstance(expr, Call):
            if expr.func == "parity":
                # checkerboard color of the GLOBAL site: (i+j+k+off)&1,
                # off = parity of the rank's global start offset
                off = self.emit(expr.args[0]) if expr.args else "0"
                return f"real(((i + j + k + (int)({off})) & 1))"
            fn = _C_FUNCS.get(expr.func)
            if fn is None:
                raise NotImplementedError(f"function {expr.func}")
            return fn + "(" + ", ".join(self.emit(a)
                                        for a in expr.args) + ")"
        if isinstance(expr, Comparison):
            return (f"({self.emit(expr.left)} {expr.op} "
                    f"{self.emit(expr.right)})")
        if isinstance(expr, If):
            return (f"({self.emit(expr.condition)} ? "
                    f"{self.emit(expr.then)} : {self.emit(expr.else_)})")
        raise TypeError(f"unhandled node {type(expr)}")

    def emit_statements(self, statements, tmp_statements=None):
        """Emit tmp defs then in-order stores; returns the body string."""
        lines = []
        for lhs, rhs in (tmp_statements or {}).items():
            name = lhs.name if hasattr(lhs, "name") else str(lhs)
            self.tmp_names.add(name)
            lines.append(f"const real {name} = {self.emit(rhs)};")
        for lhs, rhs in statements.items():
            lines.append(f"{self.emit(lhs)} = {self.emit(rhs)};")
        return "\n        ".join(lines)


PREAMBLE = """
#define ps_pow1(x) (x)
template <class T> __device__ inline T ps_pow2(T x) { return x*x; }
template <class T> __device__ inline T ps_pow3(T x) { return x*x*x; }
template <class T> __device__ inline T ps_pow4(T x)
{ T y = x*x; return y*y; }
template <class T> __device__ inline T ps_pow5(T x)
{ T y = x*x; return y*y*x; }
template <class T> __device__ inline T ps_pow6(T x)
{ T y = x*x; return y*y*y; }
template <class T> __device__ inline T ps_pow7(T x)
{ T y = x*x; return y*y*y*x; }
template <class T> __device__ inline T ps_pow8(T x)
{ T y = x*x; y = y*y; return y*y; }
"""


def geometry_defines(halo, rank_shape, max_h=None, rtype="double"):
    h = max(halo) if isinstance(halo, (tuple, list)) else halo
    nx, ny, nz = rank_shape
    return f"""
using real = {rtype};
#define H {h}
#define NX {nx}
#define NY {ny}
#define NZ {nz}
#define PSX (NX + 2*H)
#define PSY ((long)(NY + 2*H))
#define PSZ ((long)(NZ + 2*H))
#define PVOL ((long)PSX*PSY*PSZ)
#define UVOL ((long)NX*NY*NZ)
"""


# ---------------------------------------------------------------------------
# complex k-space maps (``KSpaceMap``): one mode per thread, every value a
# double or a pair of doubles whatever the arrays hold

KSPACE_DTYPES = {
    # storage type -> (pointer element, is it complex)
    "complex128": ("double2", True),
    "complex64": ("float2", True),
    "float64": ("double", False),
    "float32": ("float", False),
}

KSPACE_PREAMBLE = """
// a complex double.  Arithmetic is the textbook form; a quotient is
// a conj(b) / |b|^2 and does not guard against overflow of |b|^2.
struct cplx {
    double x, y;
    __device__ cplx() {}
    __device__ explicit cplx(double re, double im = 0.0) : x(re), y(im) {}
};
__device__ inline cplx operator-(cplx a) { return cplx(-a.x, -a.y); }
__device__ inline cplx operator+(cplx a, cplx b)
{ return cplx(a.x + b.x, a.y + b.y); }
__device__ inline cplx operator+(cplx a, double b)
{ return cplx(a.x + b, a.y); }
__device__ inline cplx operator+(double a, cplx b)
{ return cplx(a + b.x, b.y); }
__device__ inline cplx operator-(cplx a, cplx b)
{ return cplx(a.x - b.x, a.y - b.y); }
__device__ inline cplx operator-(cplx a, double b)
{ return cplx(a.x - b, a.y); }
__device__ inline cplx operator-(double a, cplx b)
{ return cplx(a - b.x, -b.y); }
__device__ inline cplx operator*(cplx a, cplx b)
{ return cplx(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline cplx operator*(cplx a, double b)
{ return cplx(a.x * b, a.y * b); }
__device__ inline cplx operator*(double a, cplx b)
{ return cplx(a * b.x, a * b.y); }
__device__ inline cplx operator/(cplx a, double b)
{ return cplx(a.x / b, a.y / b); }
__device__ inline cplx operator/(cplx a, cplx b)
{
    const double d = b.x * b.x + b.y * b.y;
    return cplx((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
__device__ inline cplx operator/(double a, cplx b)
{
    const double d = b.x * b.x + b.y * b.y;
    return cplx((a * b.x) / d, (-a * b.y) / d);
}
// i*c times a value: a quarter turn and a real scale
__device__ inline cplx ps_times_i(double c, cplx a)
{ return cplx(-c * a.y, c * a.x); }
__device__ inline cplx ps_times_i(double c, double a)
{ return cplx(0.0, c * a); }
__device__ inline cplx ps_conj(cplx a) { return cplx(a.x, -a.y); }
__device__ inline double ps_real(cplx a) { return a.x; }
__device__ inline double ps_imag(cplx a) { return a.y; }
__device__ inline double ps_abs(cplx a) { return hypot(a.x, a.y); }
__device__ inline cplx ps_cexp(cplx a)
{
    const double e = exp(a.x);
    return cplx(e * cos(a.y), e * sin(a.y));
}
// the widening loads: one access per value
__device__ inline cplx ps_load(const double2* p)
{ const double2 v = *p; return cplx(v.x, v.y); }
__device__ inline cplx ps_load(const float2* p)
{ const float2 v = *p; return cplx((double)v.x, (double)v.y); }
__device__ inline double ps_load(const double* p) { return *p; }
__device__ inline double ps_load(const float* p) { return (double)*p; }
"""


class KspaceCodegen(Codegen):
    """Emitter of complex k-space maps: :class:`Codegen` plus real/complex
    type inference, complex literals, per-axis table fields, loads that
    widen to double (``cplx`` for a complex array) and stores that round
    each real component once to the target's type.

    ``dtypes`` maps every array argument's name to its storage type, a
    key of ``KSPACE_DTYPES``.  A value read from an array is loaded once
    into a named local before the statement that first uses it; a store
    to that component makes the next read load it again, so a later
    statement sees what memory holds (the rounded value).
    """

    def __init__(self, field_args, dtypes, tmp_names=()):
        super().__init__(field_args, 0, None, tmp_names)
        for name, dt in dtypes.items():
            if dt not in KSPACE_DTYPES:
                raise TypeError(f"argument {name} has dtype {dt}; a k-space "
                                f"map takes {sorted(KSPACE_DTYPES)}")
        self.dtypes = dict(dtypes)
        self.tmp_types = {}         # name -> is it complex
        self.uses_axes = False
        self.stored = set()         # names of stored arrays
        self._loaded = {}           # (name, offset) -> local's name
        self._pending = []          # load lines not yet written out
        self._nlocal = 0

    # -- types ---------------------------------------------------------
    def is_complex(self, expr):
        """Whether ``expr`` has a complex value; raises for what a
        complex operand may not enter."""
        if is_number(expr):
            return isinstance(expr, complex)
        if isinstance(expr, Subscript):
            expr = expr.aggregate
        if isinstance(expr, Field):
            if not expr.is_spatial or len(expr.indices) == 1:
                return False
            return KSPACE_DTYPES[self.dtypes[expr.name]][1]
        if isinstance(expr, Variable):
            return self.tmp_types.get(expr.name, False)
        if isinstance(expr, (Sum, Product)):
            # every child is visited: each may hold a refusal
            return any([self.is_complex(c) for c in expr.children])
        if isinstance(expr, Quotient):
            return any([self.is_complex(expr.num), self.is_complex(expr.den)])
        if isinstance(expr, Power):
            base = self.is_complex(expr.base)
            expo = self.is_complex(expr.exponent)
            small_int = (is_number(expr.exponent)
                         and isinstance(expr.exponent, numbers.Integral)
                         and abs(expr.exponent) <= 8)
            if expo or (base and not small_int):
                raise NotImplementedError(
                    "pow: a Power with a complex operand needs an integer "
                    "exponent between -8 and 8")
            return base
        if isinstance(expr, Call):
            args = [self.is_complex(a) for a in expr.args]
            if expr.func in ("real", "imag", "abs"):
                return False
            if expr.func in ("conj", "exp"):
                return args[0]
            if any(args):
                raise NotImplementedError(
                    f"{expr.func} of a complex argument")
            return False
        if isinstance(expr, Comparison):
            if self.is_complex(expr.left) or self.is_complex(expr.right):
                raise TypeError(
                    f"comparison {expr.op} with a complex operand")
            return False
        if isinstance(expr, If):
            self.is_complex(expr.condition)
            return any([self.is_complex(expr.then),
                        self.is_complex(expr.else_)])
        raise TypeError(f"unhandled node {type(expr)}")

    def check(self, statements, tmp_statements=None):
        """Type every statement without emitting anything: the refusals
        of a k-space map, for the path that generates no code."""
        for lhs, rhs in (tmp_statements or {}).items():
            self.tmp_types[lhs.name] = self.is_complex(rhs)
        for lhs, rhs in statements.items():
            self._check_store(lhs, self.is_complex(rhs))

    def _check_store(self, lhs, value_is_complex):
        target_is_complex = self.is_complex(lhs)
        if value_is_complex and not target_is_complex:
            raise TypeError(f"a complex value is stored to {lhs.name}, "
                            f"which is {self.dtypes[lhs.name]}")
        return target_is_complex

    # -- emission ------------------------------------------------------
    def _offset(self, f, outer_idx):
        spec = self.field_specs[f.name]
        if spec.axis is not None:
            self.uses_axes = True
            return ("ii", "jj", "kk")[spec.axis]
        if len(outer_idx) != len(spec.outer_shape):
            raise ValueError(
                f"field {f.name} of outer shape {spec.outer_shape} is "
                f"indexed with {outer_idx}")
        lin = 0
        for n, ix in zip(spec.outer_shape, outer_idx):
            if not 0 <= int(ix) < n:
                raise IndexError(f"index {outer_idx} of field {f.name} is "
                                 f"outside its shape {spec.outer_shape}")
            lin = lin * n + int(ix)
        return f"{lin}L*VOLK + idx" if lin else "idx"

    def field_access(self, f, outer_idx):
        if not f.is_spatial:
            return self.scalar_param(f.name, outer_idx)
        off = self._offset(f, outer_idx)
        local = self._loaded.get((f.name, off))
        if local is None:
            local = f"v{self._nlocal}_{f.name}"
            self._nlocal += 1
            ctype = "cplx" if self.is_complex(f) else "double"
            self._pending.append(
                f"const {ctype} {local} = ps_load({f.name} + ({off}));")
            self._loaded[(f.name, off)] = local
        return local

    def emit(self, expr):
        if is_number(expr) and isinstance(expr, complex):
            return f"cplx({expr.real!r}, {expr.imag!r})"
        if isinstance(expr, Product) and is_number(expr.children[0]) \
                and isinstance(expr.children[0], complex) \
                and expr.children[0].real == 0 and len(expr.children) > 1:
            # i*c times the rest: no multiplications by zero
            rest = expr.children[1:]
            rest = self.emit(rest[0] if len(rest) == 1 else Product(rest))
            return f"ps_times_i({expr.children[0].imag!r}, {rest})"
        if isinstance(expr, Power) and is_number(expr.exponent) \
                and isinstance(expr.exponent, numbers.Integral) \
                and expr.exponent == 0:
            return "cplx(1.0)" if self.is_complex(expr.base) else self.one
        if isinstance(expr, Call) and expr.func in ("conj", "real", "imag",
                                                    "abs", "exp"):
            arg = self.emit(expr.args[0])
            if self.is_complex(expr.args[0]):
                fn = "ps_cexp" if expr.func == "exp" else "ps_" + expr.func
                return f"{fn}({arg})"
            return {"conj": arg, "real": arg, "imag": "0.0",
                    "abs": f"fabs({arg})", "exp": f"exp({arg})"}[expr.func]
        if isinstance(expr, Call) and expr.func == "parity":
            raise NotImplementedError("parity in a k-space map")
        if isinstance(expr, If):
            then, els = self.emit(expr.then), self.emit(expr.else_)
            if self.is_complex(expr):
                # both branches complex: ?: does not promote a class type
                if not self.is_complex(expr.then):
                    then = f"cplx({then})"
                if not self.is_complex(expr.else_):
                    els = f"cplx({els})"
            return f"({self.emit(expr.condition)} ? {then} : {els})"
        return super().emit(expr)

    def _flush(self, lines):
        lines.extend(self._pending)
        self._pending = []

    def emit_statements(self, statements, tmp_statements=None):
        """Body lines: temporaries, then one load per value read and one
        store per statement, in order."""
        lines = []
        for lhs, rhs in (tmp_statements or {}).items():
            name = lhs.name
            cplx = self.is_complex(rhs)
            code = self.emit(rhs)
            self.tmp_names.add(name)
            self.tmp_types[name] = cplx
            self._flush(lines)
            lines.append(
                f"const {'cplx' if cplx else 'double'} {name} = {code};")
        for n, (lhs, rhs) in enumerate(statements.items()):
            f, idx = (lhs.aggregate, tuple(int(i) for i in lhs.index)) \
                if isinstance(lhs, Subscript) else (lhs, ())
            spec = self.field_specs.get(f.name)
            if spec is None or not spec.spatial or spec.axis is not None:
                raise ValueError(f"statement target {f.name} is not a grid "
                                 "field")
            value_cplx = self.is_complex(rhs)
            target_cplx = self._check_store(lhs, value_cplx)
            code = self.emit(rhs)
            off = self._offset(f, idx)
            elem = KSPACE_DTYPES[self.dtypes[f.name]][0]
            self._flush(lines)
            if target_cplx:
                if not value_cplx:
                    code = f"cplx({code})"
                comp = elem[:-1]        # double2 -> double
                lines.append(f"const cplx o{n} = {code};")
                lines.append(f"{f.name}[{off}] = make_{elem}"
                             f"(({comp})o{n}.x, ({comp})o{n}.y);")
            else:
                lines.append(f"{f.name}[{off}] = ({elem})({code});")
            self.stored.add(f.name)
            # the next read of this component sees the stored value
            self._loaded.pop((f.name, off), None)
        return lines
