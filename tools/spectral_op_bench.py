#!/usr/bin/env python
"""Times the forward -> pointwise multiply -> inverse loop four ways on ONE plan and ONE set of dfft_malloc buffers:

  (a) execR2C + a torch multiply on the spectrum + execC2R        (what a caller writes without execSpectralOp)
  (b) execSpectralOp with an array multiplier                     (11 trips of a domain-sized buffer through memory instead of 15)
  (c) execSpectralOp with 1-D tables                              (10 instead of 15)
  (d) execSpectralOp with complex 1-D factor tables               (10 instead of 15; i * kx times a Gaussian in ky and kz)

The paths alternate within one process (a, b, c, d, a, b, c, d, ...): warm-ups first, then --reps repetitions each, every path bracketed by
device events on the stream the plan runs on.  One rank, R2C; shapes N^3 for --sizes, both precisions, both spectral_layout settings.
Prints one line per configuration and, with --out, appends them to a file.  The spread of (a) over repeated runs of the tool is the
yardstick for the ratios: run it more than once (--label names the run in the output).

--outputs K (2 .. 8) times something else: ONE execSpectralOps with K kind-5 operators (components of the gradient of a Poisson solution:
factor table i * k_d over the sums -|k|^2) against K calls of execSpectralOp with the same operators, on the same plan and buffers, the
two alternating in one process.  It prints both times, their ratio and the ratio the trip counts predict, (4 + 6 K) / (10 K).

--inputs K (2 .. 8): ONE execSpectralSum of K inputs (kind-3 operators, the factor table i * k_d: a divergence) against what a caller writes
without it -- K calls of execSpectralOp into K temporaries and their pointwise sum (torch, on the plan's stream) -- on the same plan and
buffers, alternating in one process.  Trips of a domain-sized buffer: 7 K + 3 against 10 K plus the caller's sum; the line prints both
ways of counting that sum, as one trip (10 K + 1, the figure the documents quote: 24/31 at K = 3) and as its K reads and one write
(11 K + 1: 24/34)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributedfft_amd as dfft  # noqa: E402


def measure(n, prec, layout, reps, warmup):
    cdt, rdt = (torch.complex128, torch.float64) if prec == "double" else (torch.complex64, torch.float32)
    esz = 16 if prec == "double" else 8
    pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision=prec)
    pl.setOption("spectral_op", 1 if n & (n - 1) == 0 else 2)      # 2: the mixed-radix x lengths (768, 1000, ...)
    pl.setOption("spectral_layout", layout)
    pl.initFFT(dfft.GlobalSize(n, n, n), dfft.Pencil_Partition(1, 1), True)
    stream = torch.cuda.current_stream()
    pl.setStream(stream.cuda_stream)      # the plan's launches and torch's multiply on one stream, between the same two events
    nreal, dom = n * n * n, pl.getDomainSize()
    nspec = n * n * (n // 2 + 1)
    bufs = [dfft.DeviceBuffer.alloc(b) for b in (nreal * esz // 2, nreal * esz // 2, dom, dom)]
    u, out, spec, mult = bufs[0].tensor(rdt), bufs[1].tensor(rdt), bufs[2].tensor(cdt), bufs[3].tensor(cdt)
    g = torch.Generator(device="cuda").manual_seed(7)
    u.copy_(torch.rand(nreal, generator=g, device="cuda", dtype=rdt) * 255 - 127.5)
    view = torch.view_as_real(mult[:nspec])
    view.copy_(torch.rand(view.shape, generator=g, device="cuda", dtype=rdt) - 0.5)
    k = lambda m, half=False: (torch.arange(m // 2 + 1 if half else m, device="cuda", dtype=rdt))      # noqa: E731
    sq = lambda v, m: -torch.minimum(v, m - v) ** 2      # noqa: E731
    tables = (sq(k(n), n), sq(k(n), n), sq(k(n, True), n))
    wrapped = lambda m: torch.where(k(m) < (m + 1) // 2, k(m), k(m) - m)      # noqa: E731
    gauss = lambda v: torch.exp(-0.5 * (4.0 / n) ** 2 * v ** 2).to(cdt)      # noqa: E731
    factors = ((1j * wrapped(n)).to(cdt), gauss(wrapped(n)), gauss(k(n, True)))
    scale = 1.0 / nreal

    def unfused():
        pl.execR2C(spec, u)
        spec[:nspec].mul_(mult[:nspec])      # the two blocks share one layout: a flat product
        pl.execC2R(out, spec)

    paths = {"a": unfused,
             "b": lambda: pl.execSpectralOp(out, u, multiplier=mult, scale=scale),
             "c": lambda: pl.execSpectralOp(out, u, tables=tables, scale=scale),
             "d": lambda: pl.execSpectralOp(out, u, factors=factors, scale=scale)}
    times = {p: [] for p in paths}
    for it in range(warmup + reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    del u, out, spec, mult
    for b in bufs:
        b.free()
    return {p: (statistics.median(v), min(v), max(v)) for p, v in times.items()}


def measure_outputs(n, prec, layout, K, reps, warmup):
    """(multi, singles): median, min, max in ms of one execSpectralOps with K operators and of K execSpectralOp calls"""
    cdt, rdt = (torch.complex128, torch.float64) if prec == "double" else (torch.complex64, torch.float32)
    esz = 16 if prec == "double" else 8
    pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision=prec)
    pl.setOption("spectral_op", 1 if n & (n - 1) == 0 else 2)
    pl.setOption("spectral_outputs", K)
    pl.setOption("spectral_layout", layout)
    pl.initFFT(dfft.GlobalSize(n, n, n), dfft.Pencil_Partition(1, 1), True)
    stream = torch.cuda.current_stream()
    pl.setStream(stream.cuda_stream)
    nreal = n * n * n
    bufs = [dfft.DeviceBuffer.alloc(nreal * esz // 2) for _ in range(1 + K)]
    u, outs = bufs[0].tensor(rdt), [b.tensor(rdt) for b in bufs[1:]]
    g = torch.Generator(device="cuda").manual_seed(7)
    u.copy_(torch.rand(nreal, generator=g, device="cuda", dtype=rdt) * 255 - 127.5)
    kx, ky, kz = (torch.from_numpy(k).cuda() for k in pl.wavenumbers())
    sums = tuple(-(k.to(rdt) ** 2) for k in (kx, ky, kz))
    ops = []
    for j in range(K):
        factors = [None, None, None]
        factors[j % 3] = (1j * (kx, ky, kz)[j % 3].to(rdt)).to(cdt)
        ops.append(dict(factors=tuple(factors), tables=sums, reciprocal=True, scale=1.0 / nreal))

    def singles():
        for out, op in zip(outs, ops):
            pl.execSpectralOp(out, u, **op)

    paths = {"multi": lambda: pl.execSpectralOps(outs, u, ops), "singles": singles}
    times = {p: [] for p in paths}
    for it in range(warmup + reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    del u, outs
    for b in bufs:
        b.free()
    return {p: (statistics.median(v), min(v), max(v)) for p, v in times.items()}


def measure_inputs(n, prec, layout, K, reps, warmup):
    """(sum, singles): median, min, max in ms of one execSpectralSum with K inputs and of K execSpectralOp calls plus the pointwise sum"""
    cdt, rdt = (torch.complex128, torch.float64) if prec == "double" else (torch.complex64, torch.float32)
    esz = 16 if prec == "double" else 8
    pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision=prec)
    pl.setOption("spectral_op", 1 if n & (n - 1) == 0 else 2)
    pl.setOption("spectral_inputs", K)
    pl.setOption("spectral_layout", layout)
    pl.initFFT(dfft.GlobalSize(n, n, n), dfft.Pencil_Partition(1, 1), True)
    stream = torch.cuda.current_stream()
    pl.setStream(stream.cuda_stream)
    nreal = n * n * n
    bufs = [dfft.DeviceBuffer.alloc(nreal * esz // 2) for _ in range(2 * K + 1)]
    us, tmps, out = [b.tensor(rdt) for b in bufs[:K]], [b.tensor(rdt) for b in bufs[K:2 * K]], bufs[2 * K].tensor(rdt)
    g = torch.Generator(device="cuda").manual_seed(7)
    for u in us:
        u.copy_(torch.rand(nreal, generator=g, device="cuda", dtype=rdt) * 255 - 127.5)
    ks = [torch.from_numpy(k).cuda() for k in pl.wavenumbers()]
    ops = []
    for j in range(K):
        factors = [None, None, None]
        factors[j % 3] = (1j * ks[j % 3].to(rdt)).to(cdt)
        ops.append(dict(factors=tuple(factors), scale=1.0 / nreal))

    def singles():
        for t, u, op in zip(tmps, us, ops):
            pl.execSpectralOp(t, u, **op)
        torch.add(tmps[0], tmps[1], out=out)
        for t in tmps[2:]:
            out.add_(t)

    paths = {"sum": lambda: pl.execSpectralSum(out, us, ops), "singles": singles}
    times = {p: [] for p in paths}
    for it in range(warmup + reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    del us, tmps, out
    for b in bufs:
        b.free()
    return {p: (statistics.median(v), min(v), max(v)) for p, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--precisions", nargs="+", default=["double", "float"], choices=["double", "float"])
    ap.add_argument("--layouts", type=int, nargs="+", default=[0, 1], choices=[0, 1])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--outputs", type=int, default=0, metavar="K",
                    help="time one execSpectralOps with K operators against K calls of execSpectralOp instead of the paths (a) .. (d)")
    ap.add_argument("--inputs", type=int, default=0, metavar="K",
                    help="time one execSpectralSum of K inputs against K calls of execSpectralOp plus the pointwise sum instead of the paths (a) .. (d)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.outputs and not 2 <= args.outputs <= 8:
        ap.error("--outputs must be 2 .. 8")
    if args.inputs and not 2 <= args.inputs <= 8:
        ap.error("--inputs must be 2 .. 8")
    if args.inputs and args.outputs:
        ap.error("--inputs and --outputs are separate measurements")
    lines = []
    for n in args.sizes:
        for prec in args.precisions:
            for layout in args.layouts:
                if args.outputs:
                    K = args.outputs
                    t = measure_outputs(n, prec, layout, K, args.reps, args.warmup)
                    line = (f"{args.label + ' ' if args.label else ''}{n}^3 R2C {prec:<6s} spectral_layout={layout}  outputs={K}  reps={args.reps}  ms median (min .. max):  "
                            + "  ".join(f"{name} {t[p][0]:8.3f} ({t[p][1]:.3f} .. {t[p][2]:.3f})" for p, name in
                                        (("multi", "one execSpectralOps"), ("singles", f"{K} x execSpectralOp")))
                            + f"   multi/singles = {t['multi'][0] / t['singles'][0]:.3f} (trips {4 + 6 * K}/{10 * K} = {(4 + 6 * K) / (10 * K):.3f})")
                    print(line, flush=True)
                    lines.append(line)
                    continue
                if args.inputs:
                    K = args.inputs
                    t = measure_inputs(n, prec, layout, K, args.reps, args.warmup)
                    line = (f"{args.label + ' ' if args.label else ''}{n}^3 R2C {prec:<6s} spectral_layout={layout}  inputs={K}  reps={args.reps}  ms median (min .. max):  "
                            + "  ".join(f"{name} {t[p][0]:8.3f} ({t[p][1]:.3f} .. {t[p][2]:.3f})" for p, name in
                                        (("sum", "one execSpectralSum"), ("singles", f"{K} x execSpectralOp + sum")))
                            + f"   sum/singles = {t['sum'][0] / t['singles'][0]:.3f} (trips {7 * K + 3}/{10 * K + 1} = {(7 * K + 3) / (10 * K + 1):.3f} "
                              f"with the caller's sum as one trip, {7 * K + 3}/{11 * K + 1} = {(7 * K + 3) / (11 * K + 1):.3f} with its K + 1)")
                    print(line, flush=True)
                    lines.append(line)
                    continue
                t = measure(n, prec, layout, args.reps, args.warmup)
                a = t["a"][0]
                line = (f"{args.label + ' ' if args.label else ''}{n}^3 R2C {prec:<6s} spectral_layout={layout}  reps={args.reps}  ms median (min .. max):  "
                        + "  ".join(f"({p}) {t[p][0]:8.3f} ({t[p][1]:.3f} .. {t[p][2]:.3f})" for p in "abcd")
                        + f"   b/a = {t['b'][0] / a:.3f} (bytes 11/15 = 0.733)   c/a = {t['c'][0] / a:.3f} (bytes 10/15 = 0.667)   d/a = {t['d'][0] / a:.3f} (bytes 10/15 = 0.667)")
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
