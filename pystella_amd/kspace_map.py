"""User-written complex k-space maps as one fused kernel.

:class:`KSpaceMap` is to the spectral stack what
:class:`~pystella_amd.ElementWiseMap` is to position space: a statement
dict over the modes of a k-space array (the reference writes all of its
k-space work this way: ``fk`` times per-axis momenta indexed by the loop
variables, pystella/fourier/derivs.py:93-108).  Filters, transfer
functions, phase shifts, propagators and any combination of modes,
conjugates and momenta become one launch with no temporaries.

Arguments, inferred from the expressions:

* grid fields, ``Field("fk")`` or ``Field("vk", shape=(3,))``: unpadded,
  unshifted arrays over k-space, complex128, complex64, float64 or
  float32 (the dtype is the tensor's, at the call);
* axis fields, ``Field("kx", indices=("i",))``: a float64 or float32
  table along axis 0 (``"i"``), 1 (``"j"``) or 2 (``"k"``);
* scalars: :class:`Variable`\\ s and index-free fields, run-time doubles.

The numerical definition is the complex64 k-space kernels', on the CPU
and the GPU alike: every loaded value is widened once to double (or a
pair of doubles), all arithmetic is double, and each real component of a
stored value is rounded once to its target's type.  Dtypes may therefore
be mixed freely within one map.  A complex quotient is the textbook
``a conj(b) / |b|^2``, which does not guard against overflow of
``|b|^2``.  A statement that reads a field an earlier one stored sees
the stored (rounded) value.
"""

from __future__ import annotations

import numpy as np
import torch

from pystella_amd.field import (
    Field, Variable, Subscript, collect_fields, get_field_args, iter_exprs,
    walk_expr,
)
from pystella_amd.backend.codegen import KSPACE_DTYPES, KspaceCodegen
from pystella_amd.backend.torcheval import EvalContext, eval_expr, _store

__all__ = ["KSpaceMap"]

_WIDE = {torch.complex64: torch.complex128, torch.float32: torch.float64}


def _extent(t):
    """[first, last) byte addresses that tensor ``t`` can touch."""
    if t.numel() == 0:
        return None
    span = 1 + sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


class KSpaceMap:
    """Maps ``{lhs: rhs}`` statement dicts to one fused per-mode kernel.

    :arg map_dict: statements whose keys are grid :class:`Field`\\ s (or
        Subscripts thereof) and whose values are real or complex
        expressions: ``1j`` and any Python complex number, ``conj``,
        ``real``, ``imag``, ``abs`` and ``exp`` of a complex argument,
        integer powers, and every real function on real arguments.
    :arg tmp_instructions: per-mode temporaries, real or complex,
        computed before the statements.
    :arg fixed_parameters: values for arguments that never change.

    Statements run in dict order with per-mode sequential semantics.
    A field may be stored and read under the same name (an in-place
    filter); overlapping memory under two names, one of them stored, is
    refused.
    """

    def __init__(self, map_dict, tmp_instructions=None, name="kspace_map",
                 fixed_parameters=None):
        self.name = name
        self.map_dict = dict(map_dict)
        self.tmp_instructions = dict(tmp_instructions or {})
        self.fixed_parameters = dict(fixed_parameters or {})

        all_exprs = {**self.tmp_instructions, **self.map_dict}
        for f in collect_fields(all_exprs):
            if not f.is_spatial:
                continue
            if f.is_padded or any(f.shift) or any(f.offset):
                raise ValueError(
                    f"field {f.name} is padded or shifted; a k-space map "
                    "reads and writes the mode it stands on")
            if len(f.indices) == 1:
                if f.indices[0] not in ("i", "j", "k"):
                    raise ValueError(
                        f'axis field {f.name} has index {f.indices[0]!r}; '
                        'the index is "i", "j" or "k"')
                if f.shape:
                    raise ValueError(
                        f"axis field {f.name} has an outer shape")
            elif f.indices != ("i", "j", "k"):
                raise ValueError(
                    f"field {f.name} has indices {f.indices}; a k-space "
                    'map takes ("i", "j", "k") or a single axis')
        self.field_args = get_field_args(all_exprs)
        self.grid_args = [fa for fa in self.field_args
                          if fa.spatial and fa.axis is None]
        self.axis_args = [fa for fa in self.field_args if fa.axis is not None]
        if not self.grid_args:
            raise ValueError("a k-space map needs at least one grid field")
        tmp_names = set()
        for lhs in self.tmp_instructions:
            if not isinstance(lhs, Variable) or isinstance(lhs, Field):
                raise ValueError(f"temporary {lhs} is not a Variable")
            tmp_names.add(lhs.name)
        self.stored = set()
        for lhs in self.map_dict:
            f = lhs.aggregate if isinstance(lhs, Subscript) else lhs
            if not isinstance(f, Field) or len(f.indices) != 3:
                raise ValueError(f"statement target {lhs} is not a grid "
                                 "field")
            self.stored.add(f.name)
        self.tensor_names = [fa.name for fa in self.field_args if fa.spatial]
        self.scalar_names = {fa.name for fa in self.field_args
                             if not fa.spatial}

        def visit(x):
            if isinstance(x, Variable) and not isinstance(x, Field) \
                    and x.name not in tmp_names:
                self.scalar_names.add(x.name)

        for e in iter_exprs(all_exprs):
            walk_expr(e, visit)
        self._kernels = {}

    # ------------------------------------------------------------------
    def _build_env(self, kwargs):
        env = dict(self.fixed_parameters)
        env.update(kwargs)
        missing = [n for n in (set(self.tensor_names) | self.scalar_names)
                   if n not in env]
        if missing:
            raise TypeError(f"missing kernel arguments: {sorted(missing)}")
        for n in sorted(self.scalar_names):
            v = env[n]
            if isinstance(v, complex) or (
                    isinstance(v, (torch.Tensor, np.ndarray, np.generic))
                    and "complex" in str(v.dtype)):
                raise TypeError(f"scalar {n} is complex; scalars are "
                                "run-time doubles (write a complex "
                                "constant into the expression)")
        return env

    def _check(self, env):
        """The shape, dtype, device and aliasing rules; returns
        (k-shape, {name: dtype name}, whether on a GPU)."""
        for n in self.tensor_names:
            if not isinstance(env[n], torch.Tensor):
                raise TypeError(f"argument {n} must be a tensor, got "
                                f"{type(env[n])}")
            if str(env[n].dtype)[len("torch."):] not in KSPACE_DTYPES:
                raise TypeError(
                    f"argument {n} has dtype {env[n].dtype}; a k-space map "
                    f"takes {sorted(KSPACE_DTYPES)}")
        devices = {env[n].device for n in self.tensor_names}
        if len(devices) > 1:
            raise TypeError(
                "the arguments of a k-space map must be on one device, got "
                + ", ".join(f"{n} on {env[n].device}"
                            for n in self.tensor_names))
        on_gpu = next(iter(devices)).type == "cuda"
        first = self.grid_args[0]
        if env[first.name].dim() < 3:
            raise ValueError(f"argument {first.name} has shape "
                             f"{tuple(env[first.name].shape)}: no k-space")
        kshape = tuple(env[first.name].shape[-3:])
        for fa in self.grid_args:
            shape = tuple(env[fa.name].shape)
            if shape != tuple(fa.outer_shape) + kshape:
                raise ValueError(
                    f"argument {fa.name} has shape {shape}, expected "
                    f"{tuple(fa.outer_shape) + kshape}")
        for fa in self.axis_args:
            t = env[fa.name]
            if t.is_complex():
                raise TypeError(f"axis table {fa.name} has dtype {t.dtype}; "
                                "tables are float64 or float32")
            if tuple(t.shape) != (kshape[fa.axis],):
                raise ValueError(
                    f"argument {fa.name} has shape {tuple(t.shape)}, "
                    f"expected ({kshape[fa.axis]},) along axis {fa.axis}")
        if on_gpu:
            for n in self.tensor_names:
                if not env[n].is_contiguous():
                    raise ValueError(f"argument {n} must be contiguous")
        spans = {n: _extent(env[n]) for n in self.tensor_names}
        for a in sorted(self.stored):
            for b in self.tensor_names:
                if a == b or spans[a] is None or spans[b] is None:
                    continue
                if spans[a][0] < spans[b][1] and spans[b][0] < spans[a][1]:
                    raise ValueError(
                        f"arguments {a} and {b} overlap in memory and {a} "
                        "is stored; pass one array under one name")
        dtypes = {n: str(env[n].dtype)[len("torch."):]
                  for n in self.tensor_names}
        return kshape, dtypes, on_gpu

    def __call__(self, queue=None, **kwargs):
        env = self._build_env(kwargs)
        kshape, dtypes, on_gpu = self._check(env)
        if on_gpu and int(np.prod(kshape)) > 0:
            self.kernel(kshape, dtypes)(env)
            return
        # the refusals of the code generator hold where none runs
        KspaceCodegen(self.field_args, dtypes).check(
            self.map_dict, self.tmp_instructions)
        if int(np.prod(kshape)) > 0:
            self._call_torch(env, kshape)

    def kernel(self, kshape, dtypes, compile=True):
        """The :class:`JitKspaceMap` for this layout, built once per
        (k-shape, argument dtypes); ``dtypes`` maps each tensor
        argument's name to its dtype (or the dtype's name).
        ``compile=False`` yields one that only holds its ``source`` and
        is not kept."""
        from pystella_amd.backend.hip import JitKspaceMap
        if not compile:
            return JitKspaceMap(self.map_dict, self.tmp_instructions,
                                self.field_args, dtypes, kshape,
                                name=self.name, compile=False)
        key = (tuple(kshape), tuple(str(dtypes[n])
                                    for n in self.tensor_names))
        kern = self._kernels.get(key)
        if kern is None:
            kern = JitKspaceMap(self.map_dict, self.tmp_instructions,
                                self.field_args, dtypes, kshape,
                                name=self.name)
            self._kernels[key] = kern
        return kern

    def source(self, kshape, dtypes):
        """HIP source for this layout.  Needs no device."""
        return self.kernel(kshape, dtypes, compile=False).source

    # ------------------------------------------------------------------
    def _call_torch(self, env, kshape):
        """The definition with torch ops: evaluate on widened copies and
        store through ``copy_``, which rounds once."""
        ctx = EvalContext(0, kshape)
        scratch = dict(env)
        narrow = {}
        for n in self.tensor_names:
            wide = _WIDE.get(env[n].dtype)
            if wide is not None:
                narrow[n] = env[n]
                scratch[n] = env[n].to(wide)
        for lhs, rhs in self.tmp_instructions.items():
            value = eval_expr(rhs, scratch, ctx)
            # a value of its own: real() and conj() give views, and a
            # temporary keeps its value when its operand is stored
            scratch[lhs.name] = value.clone() \
                if isinstance(value, torch.Tensor) else value
        for lhs, rhs in self.map_dict.items():
            value = eval_expr(rhs, scratch, ctx)
            if isinstance(value, torch.Tensor):
                value = value.clone()
            _store(lhs, value, scratch, ctx)
            if lhs.name in narrow:
                # the one rounding; later statements read what is stored
                narrow[lhs.name].copy_(scratch[lhs.name])
                scratch[lhs.name].copy_(narrow[lhs.name])
