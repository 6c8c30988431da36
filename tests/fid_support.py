"""
What the tests of the FID transform share (NOT part of the nmrfit_amd package): the truth, the bar, the FIDs, the
restatement of the LDS swizzle, and the driver of the poisoned-allocation children,

    python -m tests.fid_support poison OUT.npz

NO GOLDENS FROM THE REFERENCE.  The reference's loader needs nmrglue, which is not installed where these tests run, and
the reference ships no FIDs: it cannot produce recorded outputs.  Its expression (nmrfit/core.py:51-60; nmrglue's
proc_base.fft is fftshift(fft(x))) is restated with np.fft in nmrfit_amd.fid.transform_host, and that restatement is
what the tests compare against.

THE TRUTH for the centred transform Y is np.fft.fft on np.clongdouble (numpy >= 2.0 computes it in the 80-bit format:
``truth_is_long_double`` checks that it is better than fp64 could be), then fftshift.

THE BAR is the first-order bound of a radix-2-equivalent fp64 FFT (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 24.2):   || Y^ - Y ||_2 <= log2(n) eta || Y ||_2,   eta = mu + gamma_4 (sqrt(2) + mu),
gamma_4 = 4 u / (1 - 4 u), u = 2^-53, with mu the twiddles' absolute error as include/nmrfit_amd_fid.h states it
(mu = u: eta = 6.66 u; numpy's own transform is held to mu = 2 u, eta = 7.66 u).  Every single point is held to the
same absolute amount.  Nothing here is fitted to an output.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MU_DEVICE = U            # include/nmrfit_amd_fid.h, TWIDDLES
MU_NUMPY = 2.0 * U       # pocketfft's twiddles: taken as good to 2 u
LDS_LOG2 = 12
# the lengths of the accuracy test: below a wave, wave and workgroup edges, both sides of the LDS-resident / two-pass
# switch (2^12 | 2^13: a two-pass length with odd log2; 2^14: with even log2), the workload's own 2^17
LENGTHS = (2, 4, 8, 32, 64, 128, 256, 512, 1 << 12, 1 << 13, 1 << 14, 1 << 17)


def eta(mu):
    g4 = 4.0 * U / (1.0 - 4.0 * U)
    return mu + g4 * (np.sqrt(2.0) + mu)


def bar(n, mu):
    """log2(n) eta: the bound on || Y^ - Y ||_2 / || Y ||_2."""
    return np.log2(n) * eta(mu)


def truth(x, n=None):
    """Y = fftshift(fft(x, n)) of every trace of x (T, n_in) in long double."""
    x = np.asarray(x).reshape(-1, np.shape(x)[-1]).astype(np.clongdouble)
    return np.fft.fftshift(np.fft.fft(x, n=n, axis=-1), axes=-1)


def truth_is_long_double():
    """np.fft on clongdouble really is more accurate than fp64: a transform and its inverse return the input to
    better than 2^-58."""
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.clongdouble)
    back = np.fft.ifft(np.fft.fft(x))
    return back.dtype == np.clongdouble and float(np.abs(back - x).max()) < 2.0 ** -58


def errors(got, want):
    """(|| got - want ||_2 / || want ||_2, max_i |got_i - want_i| / || want ||_2) per trace, the worst over the traces,
    in units of u.  ``want`` in long double."""
    got = np.asarray(got).reshape(-1, np.shape(got)[-1]).astype(np.clongdouble)
    d = np.abs(got - want)
    norm = np.sqrt((np.abs(want) ** 2).sum(axis=-1))
    return (float((np.sqrt((d ** 2).sum(axis=-1)) / norm).max() / U), float((d.max(axis=-1) / norm).max() / U))


def sample_fid(n_in, T=1, seed=0):
    """Noise plus three decaying lines plus a non-zero mean, (T, n_in) complex128."""
    from nmrfit_amd import synth
    lines = [(0.11, 8.0 / n_in, 1.0, 0.3), (-0.27, 3.0 / n_in, 0.6, -1.0), (0.402, 20.0 / n_in, 0.8, 2.0)]
    return synth.make_fid(n_in, lines, T=T, seed=1000 + 7 * seed + n_in % 997, noise=0.05, offset=0.25 - 0.125j).fid


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b):
    """Equal bit for bit, any NaN equal to any NaN (a NaN's payload is not part of the definition)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))


def same_result(got, want):
    """(u, v, row[, Y]) tuples equal bit for bit."""
    return len(got) == len(want) and all(same_values(np.asarray(g).view(np.float64) if np.iscomplexobj(g) else g,
                                                      np.asarray(w).view(np.float64) if np.iscomplexobj(w) else w)
                                         for g, w in zip(got, want))


def refusal_table(groups):
    """The recorded refusals of an entry point, (code, the complete nmrfit_last_error() text, the calls that get it), as
    {call: (code, text)}: the text of the library before the three entry points shared one body, which no later change
    of the host code may alter."""
    table = {}
    for code, text, keys in groups:
        for key in keys:
            assert key not in table, key
            table[key] = (code, text)
    return table


# ---- the LDS swizzle of csrc/fid.hip, restated ---------------------------------------------------------------------------

def swz(a):
    """csrc/fid.hip's swz(): where index a of the block lies in a plane of doubles."""
    h = a >> 4
    return a ^ ((15 if h & 1 else 0) ^ (10 if h & 2 else 0) ^ ((h >> 2) & 7))


def store_patterns():
    """name -> the index lists (relative to the start of an aligned span) that the 16 lanes of a store group write in
    one instruction, for every store the kernels make: output r of a stage whose runs of G = Ns C doubles lie R G apart
    (G < 16; longer runs are unit stride), the row loads of pass 2 (R doubles apart, R = 2 .. 32), unit stride."""
    pats = {"unit": [list(range(16))]}
    for g in range(4):
        for rho in (1, 2):
            G, R = 1 << g, 1 << rho
            pats["stage run %d radix %d" % (G, R)] = [[(lane >> g) * R * G + (lane & (G - 1)) + r * G for lane in range(16)]
                                                      for r in range(R)]
    for lr in range(1, 6):
        pats["row load stride %d" % (1 << lr)] = [[(lane << lr) + r for lane in range(16)] for r in range(1 << lr)]
    return pats


# ---- the poison driver -------------------------------------------------------------------------------------------------

def poison_jobs():
    """A ragged batch over every path: short lengths, both two-pass parities, several traces, zero filling, an
    all-zero FID and one that is not finite."""
    jobs = [sample_fid(n_in, T, seed=s) for s, (n_in, T) in enumerate(((2, 1), (64, 3), (300, 2), (4096, 2), (5000, 1), (1 << 14, 2),
                                                                     (1000, 5), (8192, 1)))]
    jobs.append(np.zeros((2, 16), dtype=np.complex128))
    bad = sample_fid(128, 2, seed=50)
    bad[1, 5] = np.inf
    jobs.append(bad)
    return jobs


def poison_run(out):
    """Every piece of the entry point's device block, with and without the transform output.  Host outputs start as NaN
    (np.empty is filled), so a copy that came up short shows."""
    from nmrfit_amd import fid
    from tests import poison_support
    arrays = {}
    with poison_support.nan_outputs():
        jobs = poison_jobs()
        full = fid.transform_many(jobs, zero_fill="pow2", return_transform=True)
        plain = fid.transform_many(jobs, zero_fill="pow2")
        for k, (f, p) in enumerate(zip(full, plain)):
            assert same_result(f[:3], p), k
            arrays["u%d" % k], arrays["v%d" % k], arrays["row%d" % k] = f[0], f[1], f[2]
            arrays["Y%d" % k] = f[3].view(np.float64)
        assert [int(f[2][0]) for f in full] == [0] * 8 + [1, 2]
        # a status-0 job leaves no NaN the driver put there
        assert all(np.isfinite(f[0]).all() and np.isfinite(f[1]).all() and np.isfinite(f[3].view(np.float64)).all() for f in full[:8])
    arrays["__poison__"] = np.array(os.environ.get("NMRFIT_POISON_ALLOC", ""))
    np.savez(out, **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "poison":
        sys.exit("usage: python -m tests.fid_support poison OUT.npz")
    poison_run(sys.argv[2])
