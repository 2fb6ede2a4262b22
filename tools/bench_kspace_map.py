"""A/B of user-written k-space maps (KSpaceMap, a generated kernel)
against the hand-written k-space kernels and against a chain of torch
ops, on one GPU: the k-space pass only, no transforms.

Rows: the collocator's gradient + Laplacian (four outputs from one read
of fk) and the Poisson solve, each transcribed as a
KSpaceMap, at k-shape (n, n, n/2 + 1) in complex128 and complex64.
Three forms run interleaved in one process, --rounds times --calls
calls each, timed with HIP events after warm-up:

    map    the KSpaceMap
    hand   hip.kspace_derivs / hip.kspace_poisson and their _c64 forms,
           which move the same bytes
    torch  the same formulas as torch ops on the same tensors

One JSON line per (row, dtype): for each form the median over the rounds
of a round's ms per call, map/hand and torch/map, the spread of the
rounds ((max - min) / median), torch.cuda.max_memory_allocated() above the
allocation held just before the timed calls, and the largest difference
of the map's outputs from the hand-written kernel's relative to the
latter's largest magnitude.

Run each size in a process of its own, under a time limit:

    timeout 300 python tools/bench_kspace_map.py --n 256 && \\
    timeout 600 python tools/bench_kspace_map.py --n 512
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    p = ap.parse_args()

    import pystella_amd as ps
    from pystella_amd.backend import hip
    from pystella_amd.field import Field, If, var

    if not torch.cuda.is_available():
        sys.exit("bench_kspace_map.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    n = p.n
    kshape = (n, n, n // 2 + 1)
    lengths = (5., 3., 7.)
    inv_n = 1.0 / float(n)**3
    m2 = 1.7

    def table(fn):
        out = []
        for mu, length in enumerate(lengths):
            m = np.arange(kshape[2]) if mu == 2 \
                else np.fft.fftfreq(n, 1 / n)
            out.append(torch.as_tensor(
                fn(2 * np.pi / length * m, length / n), device=dev))
        return out

    k1 = table(lambda k, dx: k)
    k2 = table(lambda k, dx: np.sin(k * dx) / dx)
    eig = table(lambda k, dx: -(2 * np.sin(k * dx / 2) / dx)**2)
    b1, b2, be = ([t.reshape(s) for t, s in zip(
        tabs, ((-1, 1, 1), (1, -1, 1), (1, 1, -1)))] for tabs in
        (k1, k2, eig))

    # the collocator's and the solver's formulas as maps
    fk, t = Field("fk"), var("t")
    k1f = [Field(f"k1{a}", indices=(ix,)) for a, ix in zip("xyz", "ijk")]
    k2f = [Field(f"k2{a}", indices=(ix,)) for a, ix in zip("xyz", "ijk")]
    names = ("pdx", "pdy", "pdz", "lap")
    stmts = {Field(o): 1j * k * t for o, k in zip(names, k1f)}
    stmts[Field("lap")] = -(k2f[0]**2 + k2f[1]**2 + k2f[2]**2) * t
    derivs_map = ps.KSpaceMap(stmts, {t: fk * var("inv_n")},
                              name="bench_derivs_map")
    ex, ey, ez = (Field(f"e{a}", indices=(ix,)) for a, ix in zip("xyz", "ijk"))
    rhok, mk2 = Field("rhok"), var("mk2")
    poisson_map = ps.KSpaceMap(
        {Field("sol"): If(mk2 < 0, (rhok * var("inv_n")) / (mk2 - var("m2")),
                          0)},
        {mk2: ex + ey + ez}, name="bench_poisson_map")

    gen = torch.Generator(device="cpu").manual_seed(7)

    for ctype in (torch.complex128, torch.complex64):
        rdtype = torch.float64 if ctype == torch.complex128 \
            else torch.float32
        src = torch.view_as_complex(torch.randn(
            kshape + (2,), dtype=rdtype, generator=gen)).to(dev)
        outs = {o: torch.zeros(kshape, dtype=ctype, device=dev)
                for o in names}
        work = torch.zeros_like(src)
        c64 = ctype == torch.complex64
        derivs_fn = hip.kspace_derivs_c64 if c64 else hip.kspace_derivs
        poisson_fn = hip.kspace_poisson_c64 if c64 else hip.kspace_poisson
        tabs = {f"k1{a}": k for a, k in zip("xyz", k1)}
        tabs.update({f"k2{a}": k for a, k in zip("xyz", k2)})
        etabs = {f"e{a}": e for a, e in zip("xyz", eig)}

        def torch_derivs():
            tt = src * inv_n
            for o, q in zip(names, b1):
                outs[o].copy_(1j * q * tt)
            outs["lap"].copy_(-(b2[0]**2 + b2[1]**2 + b2[2]**2) * tt)

        def torch_poisson():
            mk = be[0] + be[1] + be[2]
            work.copy_(torch.where(mk < 0, (src * inv_n) / (mk - m2), 0))

        rows = {
            "grad_lap": ({
                "map": lambda: derivs_map(fk=src, inv_n=inv_n, **outs,
                                          **tabs),
                "hand": lambda: derivs_fn(src, outs, k1, k2, inv_n),
                "torch": torch_derivs}, lambda: list(outs.values())),
            "poisson": ({
                "map": lambda: poisson_map(rhok=src, sol=work, inv_n=inv_n,
                                           m2=m2, **etabs),
                "hand": lambda: poisson_fn(src, work, *eig, inv_n, m2),
                "torch": torch_poisson}, lambda: [work]),
        }

        for row, (forms, results_of) in rows.items():
            times = {form: [] for form in forms}
            peaks = {form: 0 for form in forms}
            results = {}
            for rnd in range(p.rounds):
                for form, call in forms.items():
                    for _ in range(p.warmup):
                        call()
                    torch.cuda.synchronize()
                    if rnd == 0:
                        results[form] = [o.clone() for o in results_of()]
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    # one window around the round's calls, back to back:
                    # host work of a call overlaps the kernel before it
                    start = torch.cuda.Event(enable_timing=True)
                    stop = torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(p.calls):
                        call()
                    stop.record()
                    stop.synchronize()
                    ms = start.elapsed_time(stop) / p.calls
                    times[form].append(ms)
                    peaks[form] = max(
                        peaks[form],
                        torch.cuda.max_memory_allocated() - base)
                torch.cuda.empty_cache()

            def median(form):
                return statistics.median(times[form])

            def spread(form):
                meds = times[form]
                return (max(meds) - min(meds)) / statistics.median(meds)

            def max_diff(form, against):
                return max(
                    ((a.to(torch.complex128) - b.to(torch.complex128))
                     .abs().max() / b.abs().max()).item()
                    for a, b in zip(results[form], results[against]))

            out = {"n": n, "kshape": list(kshape), "row": row,
                   "dtype": str(ctype).replace("torch.", "")}
            for form in forms:
                out[form + "_ms"] = round(median(form), 4)
            out.update({
                "map_over_hand": round(median("map") / median("hand"), 4),
                "torch_over_map": round(median("torch") / median("map"), 4),
                "peak_extra_bytes": {f: int(peaks[f]) for f in forms},
                "map_max_diff_vs_hand": max_diff("map", "hand"),
                "torch_max_diff_vs_hand": max_diff("torch", "hand"),
                "round_spread": {f: round(spread(f), 4) for f in forms},
                "rounds": p.rounds, "calls_per_round": p.calls})
            print(json.dumps(out), flush=True)
        del src, outs, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
