"""A/B of the fused k-space kernels against the torch chain
(PYSTELLA_KSPACE=0) for SpectralCollocator and SpectralPoissonSolver on
one GPU.

Three operations are timed with HIP events after warm-up: collocator
gradient + Laplacian, collocator divergence, and the Poisson solve.
Both forms run interleaved in the same process, --rounds times each.
One JSON line per (operation, form): the median ms per call over all
rounds, each round's median, and torch.cuda.max_memory_allocated()
above the allocation held just before the timed calls.  The fused
collocator's scratch buffers are allocated by the warm-up call, so they
are part of that baseline; what each operation holds of them for the
collocator's lifetime is reported separately as scratch_bytes.  Fused
rows also carry the largest difference of their outputs from the
chain's, relative to the chain's largest magnitude.

Usage: python tools/bench_spectral.py [--n 512] [--rounds 3] [--calls 5]
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
        sys.exit("bench_spectral.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    grid = (p.n,) * 3
    lengths = (5., 3., 7.)
    dk = tuple(2 * np.pi / li for li in lengths)
    dx = tuple(li / n for li, n in zip(lengths, grid))
    decomp = ps.DomainDecomposition((1, 1, 1), 0, rank_shape=grid)
    fft = DFT(decomp, grid_shape=grid, dtype=np.float64, device=dev)
    coll = ps.SpectralCollocator(fft, dk)
    solver = ps.SpectralPoissonSolver(
        fft, dk, dx, SecondCenteredDifference(2).get_eigenvalues)

    gen = torch.Generator(device="cpu").manual_seed(7)
    vec = torch.rand((3,) + grid, dtype=torch.float64,
                     generator=gen).to(dev)
    fx = vec[0]
    lap = torch.zeros(grid, dtype=torch.float64, device=dev)
    grd = torch.zeros((3,) + grid, dtype=torch.float64, device=dev)

    # (call, the arrays it writes)
    ops = {
        "grad_lap": (lambda: coll(fx=fx, lap=lap, grd=grd), (lap, grd)),
        "divergence": (lambda: coll.divergence(vec=vec, div=lap), (lap,)),
        "poisson": (lambda: solver(fx=lap, rho=fx, m_squared=1.7), (lap,)),
    }
    forms = {"fused": None, "chain": "0"}

    def set_form(form):
        if forms[form] is None:
            os.environ.pop("PYSTELLA_KSPACE", None)
        else:
            os.environ["PYSTELLA_KSPACE"] = forms[form]

    times = {(op, form): [] for op in ops for form in forms}
    peaks = {key: 0 for key in times}
    results = {}
    for rnd in range(p.rounds):
        for op, (call, outs) in ops.items():
            for form in forms:
                set_form(form)
                for _ in range(p.warmup):
                    call()
                torch.cuda.synchronize()
                if rnd == 0:
                    results[op, form] = [o.clone() for o in outs]
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
                times[op, form].append(ms)
                peaks[op, form] = max(
                    peaks[op, form],
                    torch.cuda.max_memory_allocated() - base)
    os.environ.pop("PYSTELLA_KSPACE", None)

    # scratch buffers each fused operation writes, of k-shape each
    fk_bytes = fft.fk.numel() * fft.fk.element_size()
    scratch = {"grad_lap": 4, "divergence": 1, "poisson": 0}
    assert len(coll._scratch) == max(scratch.values())
    for op in ops:
        for form in forms:
            rounds = times[op, form]
            row = {
                "n": p.n, "op": op, "form": form,
                "median_ms": round(statistics.median(
                    t for ms in rounds for t in ms), 4),
                "round_median_ms": [round(statistics.median(ms), 4)
                                    for ms in rounds],
                "peak_extra_bytes": int(peaks[op, form]),
                "rounds": p.rounds, "calls_per_round": p.calls,
            }
            if form == "fused":
                row["scratch_bytes"] = scratch[op] * fk_bytes
                row["max_diff_vs_chain"] = max(
                    ((a - b).abs().max() / b.abs().max()).item()
                    for a, b in zip(results[op, "fused"],
                                    results[op, "chain"]))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
