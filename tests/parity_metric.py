"""The forward-parity metric of the GPU tests (round-5 verdict, "tolerance hole").

SURVEY 8c scaled the forward error by max|X|.  For the reference's input -- uniform[0, 255), non-negative
(tests/src/pencil/base.cu:45-53) -- max|X| is the DC term, 180 N^3, while a typical entry is 104 sqrt(N^3): at 1024^3 the
old bound 1e-11 admitted a PER-ENTRY relative error of 4e-7, i.e. a twiddle table rounded to fp32 passed the fp64 forward
checks.  The bound used here is per entry:

        max_k  |got[k] - want[k]| / max(|want[k]|, rms(want))   <=   RMS_TOL[prec] * log2(points of the transform)

rms(want) = sqrt(mean |want|^2) (= sqrt(points) * rms(x) by Parseval: within 2x of the typical entry even for the
non-negative input, where the DC term contributes 180^2 of 208^2); an entry that is itself larger than the rms -- the DC
term of the non-negative input, sqrt(points) times larger -- is held to its own magnitude, every other one to the rms.  fp64: 1e-13 * log2(n) (3e-12 at 1024^3; measured
values are ~1e-15, profiles/r6_parity_table.txt; fp32-rounded twiddles give ~1e-8 and fail: profiles/r6_f32_twiddle_proof.txt).
fp32 against the fp64 oracle: 2e-7 * log2(n).  The old assertion stays beside it wherever it was.

Zero-mean inputs (uniform - 127.5, and the sine field of the reference's testcase 4, random_dist_3D.cu:748-762) are
added next to the reference's distribution: CENTER is what `center=True` subtracts.

fp32 and the NON-NEGATIVE distribution: the per-entry bound is asserted on the zero-mean inputs only.  With a mean of 127.5 the
z pass leaves 127.5 Nz in every kz = 0 entry, and the y and x passes on the planes through the DC point cancel numbers of that
size down to the noise: the rounding they leave is eps32 times the DC MASS (180 N^(3/2) per plane line), not eps32 times the
entry -- any fp32 FFT has it, and relative to rms(X) it reads 1e-5 ... 6e-4 (measured: profiles/r6_parity_table.txt, the rows
`float ... centred=False`; the same kernels on the centred input: <= 1.3e-6).  There the old bound (scaled by max|X| = the DC term,
which IS the scale of that error) stays the assertion and the per-entry figure is recorded only.  fp64 has 9 more digits and
passes the per-entry bound on both inputs.

Where it is asserted: beside the old bound in every test that compares a forward result with the oracle (check_forward, or
check_forward_blocks for the ranks' blocks of one spectrum) -- at fp64 on the reference's distribution, at both precisions on
zero-mean input: the kernel-level 1-D tests feed both inputs in both directions, and tests/test_gpu_entry_parity.py runs every
kernel family and option-forced form of the 3-D plans once more on the centred input.  factor = 1 everywhere there
(profiles/entry_parity_table.txt: the measured values; profiles/entry_parity_mutation.txt: the same assertions on a library whose
fp64 tables are rounded through fp32)."""
import math
import os

import numpy as np

RMS_TOL = {"double": 1e-13, "float": 2e-7}
CENTER = 127.5


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2)))


def current_test(zero_mean):
    """DFFT_PARITY_TABLE_ALL=1: checks without a label are recorded too, under the id of the running test (the mutation proof of
    profiles/entry_parity_mutation.txt reads both metrics of every check from the table)"""
    if os.environ.get("DFFT_PARITY_TABLE_ALL") == "1" and os.environ.get("DFFT_PARITY_TABLE"):
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        return f"{test} zero_mean={zero_mean}" if test else None
    return None


def forward_bound(prec, npoints):
    return RMS_TOL[prec] * max(1.0, math.log2(max(2, int(npoints))))


def rms_rel(got, want, want_rms=None):
    """max_k |got - want|[k] / max(|want[k]|, rms(want)); `want_rms` = the rms of the WHOLE spectrum when `want` is one rank's block"""
    r = max(want_rms if want_rms is not None else rms(want), 1e-300)
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got) - want) / np.maximum(np.abs(want), r)))


def entry_rel(got, want, want_rms):
    """the same for one entry"""
    return abs(got - want) / max(abs(want), want_rms, 1e-300)


def record(label, prec, npoints, value, bound, old=None):
    """appends one line to the table the round's profile is made from (DFFT_PARITY_TABLE=<file>)"""
    path = os.environ.get("DFFT_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(f"{label:<72s} {prec:<6s} n=2^{math.log2(max(1, npoints)):5.2f}  max|err|/rms = {value:.3e}  bound {bound:.1e}"
                    + (f"  (max|err|/max|X| = {old:.3e})" if old is not None else "") + "\n")


def worst_entry(got, want, want_rms=None):
    """where the per-entry figure is largest: "index (..): got .., want .., rms .." (for the message of a failed assertion)"""
    got, want = np.asarray(got), np.asarray(want)
    r = max(want_rms if want_rms is not None else rms(want), 1e-300)
    k = np.unravel_index(int(np.argmax(np.abs(got - want) / np.maximum(np.abs(want), r))), want.shape)
    return f"worst entry {tuple(int(i) for i in k)}: got {got[k]}, want {want[k]}, rms(want) {r:.6e}"


def check_forward(got, want, prec, npoints, label=None, want_rms=None, factor=1.0, zero_mean=True):
    """the per-entry forward bound; returns the measured value.  zero_mean=False (the reference's non-negative distribution):
    asserted at fp64, recorded only at fp32 (see the module docstring)"""
    v = rms_rel(got, want, want_rms)
    b = forward_bound(prec, npoints) * factor
    label = label or current_test(zero_mean)
    if label:
        old = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / max(float(np.max(np.abs(want))), 1e-300)
        record(label, prec, npoints, v, b, old)
    if prec == "float" and not zero_mean:
        return v
    assert v <= b, (f"forward error per entry {v:.3e} > {b:.1e} (max|got - want| / rms(want), {prec}, {npoints} points{', ' + label if label else ''}); "
                    + worst_entry(got, want, want_rms))
    return v


def check_forward_blocks(plans, spec, want, prec, npoints, label=None, factor=1.0, zero_mean=True):
    """check_forward for every rank's block (getOutSize / getOutStart of its plan) of the global spectrum `want`, each entry against
    the rms of the WHOLE spectrum; `label`: one line of the table, the worst rank.  Returns the largest value."""
    want_rms = rms(want)
    b = forward_bound(prec, npoints) * factor
    label = label or current_test(zero_mean)
    worst, old, at = -1.0, 0.0, None
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        v = rms_rel(spec[r], ref, want_rms)
        if label:
            old = max(old, float(np.max(np.abs(spec[r] - ref))) / max(float(np.max(np.abs(want))), 1e-300))
        if v > worst:
            worst, at = v, (r, ref)
    if label:
        record(label, prec, npoints, worst, b, old)
    if prec == "float" and not zero_mean:
        return worst
    assert worst <= b, (f"forward error per entry {worst:.3e} > {b:.1e} (max|got - want| / rms(want), {prec}, {npoints} points, rank {at[0]}"
                        f"{', ' + label if label else ''}); " + worst_entry(spec[at[0]], at[1], want_rms))
    return worst
