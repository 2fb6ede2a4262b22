"""A/B of precision="native" against the default precision="promote" for
SpectralCollocator and SpectralPoissonSolver built on a float32
transform, on one GPU, with the fused float64 path on the same box
alongside.

Rows: collocator gradient + Laplacian, collocator divergence, and the
Poisson solve.  Four forms run interleaved in one process, --rounds
times each, timed with HIP events after warm-up:

    promote       the torch chain in complex128 (the default)
    native        the complex64 kernels and complex64 inverse transforms
    native_torch  "native" with PYSTELLA_KSPACE=0: the same definition in
                  torch ops, so native_torch - native is what the kernels
                  buy and promote - native_torch what the complex64
                  inverse transforms (and the dropped output copy) buy
    f64           the same objects on a float64 transform (fused
                  complex128 kernels)

One JSON line per row: the median ms per call over all rounds for each
form, native/promote and the other ratios, the spread of the round
medians ((max - min) / median), torch.cuda.max_memory_allocated() above
the allocation held just before the timed calls for each form, the
scratch the native collocator holds for the row, and the largest
difference of the native outputs from the promote ones relative to the
latter's largest magnitude.

Run each size in a process of its own, under a time limit:

    timeout 300 python tools/bench_spectral_c64.py --n 256 && \\
    timeout 600 python tools/bench_spectral_c64.py --n 512
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
    from pystella_amd.derivs import SecondCenteredDifference
    from pystella_amd.fourier import DFT

    if not torch.cuda.is_available():
        sys.exit("bench_spectral_c64.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    grid = (p.n,) * 3
    lengths = (5., 3., 7.)
    dk = tuple(2 * np.pi / li for li in lengths)
    dx = tuple(li / n for li, n in zip(lengths, grid))
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    eig = SecondCenteredDifference(2).get_eigenvalues

    gen = torch.Generator(device="cpu").manual_seed(7)
    vec32 = torch.rand((3,) + grid, dtype=torch.float32, generator=gen)

    def rows_for(dtype, **kwargs):
        """({row: (call, outputs)}, collocator) on a transform of
        ``dtype``; the inputs are the same numbers for both dtypes."""
        rdtype = torch.float32 if dtype == np.float32 else torch.float64
        fft = DFT(decomp, grid_shape=grid, dtype=dtype, device=dev)
        coll = ps.SpectralCollocator(fft, dk, **kwargs)
        solver = ps.SpectralPoissonSolver(fft, dk, dx, eig, **kwargs)
        vec = vec32.to(device=dev, dtype=rdtype)
        fx = vec[0]
        lap = torch.zeros(grid, dtype=rdtype, device=dev)
        grd = torch.zeros((3,) + grid, dtype=rdtype, device=dev)
        return {
            "grad_lap": (lambda: coll(fx=fx, lap=lap, grd=grd), (lap, grd)),
            "divergence": (lambda: coll.divergence(vec=vec, div=lap),
                           (lap,)),
            "poisson": (lambda: solver(fx=lap, rho=fx, m_squared=1.7),
                        (lap,)),
        }, coll

    promote, _ = rows_for(np.float32)
    native, native_coll = rows_for(np.float32, precision="native")
    f64, _ = rows_for(np.float64)

    # form -> (rows, PYSTELLA_KSPACE)
    forms = {"promote": (promote, None), "native": (native, None),
             "native_torch": (native, "0"), "f64": (f64, None)}
    fk_bytes = native_coll.fft.fk.numel() * native_coll.fft.fk.element_size()
    scratch = {"grad_lap": 4, "divergence": 1, "poisson": 0}

    for row in promote:
        times = {form: [] for form in forms}
        peaks = {form: 0 for form in forms}
        results = {}
        for rnd in range(p.rounds):
            for form, (rows, switch) in forms.items():
                if switch is None:
                    os.environ.pop("PYSTELLA_KSPACE", None)
                else:
                    os.environ["PYSTELLA_KSPACE"] = switch
                call, outs = rows[row]
                for _ in range(p.warmup):
                    call()
                torch.cuda.synchronize()
                if rnd == 0:
                    results[form] = [o.clone() for o in outs]
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ms = []
                for _ in range(p.calls):
                    start = torch.cuda.Event(enable_timing=True)
                    stop = torch.cuda.Event(enable_timing=True)
                    start.record()
                    call()
                    stop.record()
                    stop.synchronize()
                    ms.append(start.elapsed_time(stop))
                times[form].append(ms)
                peaks[form] = max(peaks[form],
                                  torch.cuda.max_memory_allocated() - base)
        os.environ.pop("PYSTELLA_KSPACE", None)

        def median(form):
            return statistics.median(t for ms in times[form] for t in ms)

        def spread(form):
            meds = [statistics.median(ms) for ms in times[form]]
            return (max(meds) - min(meds)) / statistics.median(meds)

        def max_diff(form, against):
            return max(((a.double() - b.double()).abs().max()
                        / b.abs().max()).item()
                       for a, b in zip(results[form], results[against]))

        out = {"n": p.n, "row": row}
        for form in forms:
            out[form + "_ms"] = round(median(form), 4)
        out.update({
            "native_over_promote": round(
                median("native") / median("promote"), 4),
            "native_torch_over_promote": round(
                median("native_torch") / median("promote"), 4),
            "native_over_f64": round(median("native") / median("f64"), 4),
            "peak_extra_bytes": {f: int(peaks[f]) for f in forms},
            "native_scratch_bytes": scratch[row] * fk_bytes,
            "native_max_diff_vs_promote": max_diff("native", "promote"),
            "native_torch_max_diff_vs_native": max_diff("native_torch",
                                                        "native"),
            "round_spread": {f: round(spread(f), 4) for f in forms},
            "rounds": p.rounds, "calls_per_round": p.calls})
        print(json.dumps(out), flush=True)
    assert len(native_coll._scratch) == max(scratch.values())


if __name__ == "__main__":
    main()
