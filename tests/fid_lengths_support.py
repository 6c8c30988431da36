"""
What the tests of the FID transforms at every length class share (NOT part of the nmrfit_amd package): the lengths, the
factorisation csrc/fid.hip's fid_plan makes of them, inputs with closed-form transforms and the two bars derived for them.
The dense truth and bar, the chirp-z truth and bar and the conditioning's are tests/fid_support.py's,
tests/fid_any_support.py's and tests/fid_cond_support.py's, unchanged.

THE IMPULSE.  x = a delta_p has X[q] = a exp(-2 pi i (p q mod n) / n): ``impulse_truth`` evaluates that in long double
with the angle reduced exactly in integers and folded to an octant, for any n, without any transform.  A trace with a
few non-zero points is the sum of its impulses (``sparse_truth``).

THE BARS are derived, not fitted: ``impulse_bar`` (every point of a power-of-two transform of an impulse) and
``sparse_bar`` (the any-length header's bar with the trace's non-zero points in place of n_in'); their docstrings hold
the derivations.  No measured constant.
"""
import numpy as np

from nmrfit_amd import fid
from tests import fid_any_support as fa
from tests import fid_cond_support as fc
from tests import fid_support as fs

U = fs.U
# log2 of the two-pass lengths that tests/fid_support.py's LENGTHS leave out (13, 14 and 17 are there): with them every
# factorisation of 2^13 .. 2^22
FACTOR_LGS = (15, 16, 18, 19, 20, 21, 22)
# log2 of every length the impulses run at
IMPULSE_LGS = tuple(sorted({int(n).bit_length() - 1 for n in fs.LENGTHS} | set(FACTOR_LGS)))
# the chirp-z lengths: M = 2^15 .. 2^22, and the two a 64k Bruker FID comes out at (M = 2^17)
CHIRP_LENGTHS = (16383, 32767, 65466, 65467, 65535, 131071, 262143, 524287, 1048575, 2097151)
AMPLITUDE = 0.75 - 1.25j


def factorisation(lg):
    """(lg1, lg2, C, R) of a two-pass length 2^lg as csrc/fid.hip's fid_plan cuts it: pass 1 transforms C = 2^(12 - lg1)
    interleaved columns of 2^lg1 points, pass 2 R = 2^(12 - lg2) interleaved rows of 2^lg2 points."""
    lg1 = lg // 2
    lg2 = lg - lg1
    return lg1, lg2, 1 << (fs.LDS_LOG2 - lg1), 1 << (fs.LDS_LOG2 - lg2)


def unit_root(r, n):
    """exp(-2 pi i r / n) for integers 0 <= r < n (int64 array), any n, in np.clongdouble: the fraction of a turn is
    folded to an octant in integers as fid._chirp_cached does, so that 1, -i, sqrt(1/2) (1 - i) and their kin are exact and
    cos / sin are taken on at most pi / 4; pi itself is the long double's."""
    r = np.asarray(r, dtype=np.int64)
    octant, rem = np.divmod(8 * r, n)                            # 8 r / n = octant + rem / n
    odd = octant & 1
    # the angle is h quarter turns plus or minus th, th = (rem or n - rem) / n eighths of a turn, at most pi / 4
    h = (octant + 1) >> 1
    pi = np.arctan2(np.longdouble(0), np.longdouble(-1))
    th = np.where(odd == 1, n - rem, rem).astype(np.longdouble) * (pi / np.longdouble(4) / np.longdouble(n))
    cc, ss = np.cos(th), np.sin(th)
    odd_eighth = np.flatnonzero((rem == 0) & (odd == 1))         # exactly pi / 4 (rem == 0 in an even octant: th == 0)
    cc[odd_eighth] = ss[odd_eighth] = np.sqrt(np.longdouble(0.5))
    ss *= (1 - 2 * odd).astype(np.longdouble)
    # cos and sin of h quarter turns are 0 and +-1: the products are exact and every sum has a zero operand
    ch = np.array([1, 0, -1, 0, 1], dtype=np.longdouble)[h]
    sh = np.array([0, 1, 0, -1, 0], dtype=np.longdouble)[h]
    out = np.empty(r.shape, dtype=np.clongdouble)
    out.real = cc * ch - ss * sh
    out.imag = -(ss * ch + cc * sh)                              # the negative angle
    return out


def impulse_truth(n, p, a):
    """Y (n,) of x = a delta_p at length n, any n, in np.clongdouble: X[q] = a exp(-2 pi i (p q mod n) / n) with p q
    reduced in int64 (p q < 2^44), centred as fs.truth centres (numpy's fftshift: Y[i] = X[(i + n - n // 2) mod n]).  No
    transform is involved."""
    n, p = int(n), int(p)
    assert 0 <= p < n <= 1 << 22
    q = (np.arange(n, dtype=np.int64) + (n - n // 2)) % n
    return np.clongdouble(a) * unit_root((p * q) % n, n)


def sparse_truth(N, points, values):
    """Y (N,) of the trace whose only non-zero points are ``values`` at ``points``: the sum of its impulses."""
    Y = np.zeros(N, dtype=np.clongdouble)
    for p, a in zip(points, values):
        Y = Y + impulse_truth(N, p, a)
    return Y


def impulse_positions(lg):
    """Where the impulses of the device test sit.  A two-pass length reads index j1 n2 + j2 and multiplies column j2's
    output q1 by omega_n^(j2 q1): p = 1 is j2 = 1 alone, p = n2 is j1 = 1 alone (every split twiddle is 1), n2 - 1 and
    n - n2 are the last column and the last row alone, n - 1 gives the largest j2 q1.  At 2^21 and 2^22 three of them, to
    keep the host's truth to seconds."""
    n = 1 << lg
    if lg <= fs.LDS_LOG2:
        return tuple(sorted({0, 1, n // 2, n - 1}))
    n2 = 1 << factorisation(lg)[1]
    return (1, n2, n - 1) if lg >= 21 else (0, 1, n2 - 1, n2, n - n2, n - 1)


def products(lg):
    """m: the twiddle products between an input point and an output point of the transform of 2^lg points.  A block of
    2^L points makes L // 2 stages of radix 4, each with one product per path, and an odd L one stage of radix 2 first,
    which has none; a two-pass length is a block of lg1, the split twiddle, a block of lg2."""
    if lg <= fs.LDS_LOG2:
        return lg // 2
    lg1, lg2 = factorisation(lg)[:2]
    return lg1 // 2 + lg2 // 2 + 1


def impulse_bar(lg, mu=fs.MU_DEVICE):
    """The bound on |Y^[q] - Y[q]| / |a| at EVERY point q of the device's transform of x = a delta_p, n = 2^lg.

    After s stages the block holds the transforms of the interleaved subsequences of 4^s (or 2 4^s) points; the impulse
    lies in one of them, so of the R inputs of a butterfly of the next stage at most one is not zero.  In csrc/fid.hip's
    lds_stage every addition and subtraction then has an exact zero as its other operand and is exact, the rotation by
    -i swaps and negates parts and is exact, and the radix-2 stage has no product.  What is left on the way from x[p]
    to Y[q] is a chain of m = products(lg) complex products, each by a twiddle within mu of the exact one (absolute, as
    a complex number: include/nmrfit_amd_fid.h, TWIDDLES) and each rounded as Higham's Lemma 3.5 has it, relative error
    at most sqrt(2) gamma_2.  One link takes a value v to v w (1 + d) + v dw, |dw| <= mu, |d| <= sqrt(2) gamma_2, |w| = 1:
    its modulus grows by at most 1 + kappa, kappa = mu + sqrt(2) gamma_2 (1 + mu) -- tests/fid_any_support.py's kappa --
    and the error after m links is at most ((1 + kappa)^m - 1) |a|.  m = 0 at n = 2: the transform of an impulse is
    exact there."""
    kappa = mu + np.sqrt(2.0) * fc.GAMMA2 * (1.0 + mu)
    return float(np.expm1(products(lg) * np.log1p(kappa)))


def sparse_bar(x, N, mu=fs.MU_DEVICE):
    """The absolute bar on || Y^ - Y ||_2 per trace of x (T, n_in') at the any-length transform of length N, for traces
    with few non-zero points: fa.bar with s, the number of non-zero points of the trace, in place of n_in'.

    include/nmrfit_amd_fid_any.h's derivation uses n_in' only through max|A| <= ||a||_1 <= sqrt(n_in') ||x'||_2
    (Cauchy-Schwarz over the points that can be non-zero); for s non-zero points ||a||_1 <= sqrt(s) ||x'||_2.  The bar of
    a trace is therefore fa.bar of its non-zero points alone -- the same norm, s points -- and beta stays
    fid.filter_peak(N)."""
    x = np.asarray(x).reshape(-1, np.shape(x)[-1])
    return np.array([fa.bar(t[t != 0][None, :], N, mu)[0] for t in x])


def sparse_traces(N, seed=0):
    """(3, N) complex128 and the (points, values) of each trace: one point at 0, one at N - 1, four at
    {1, N // 2, N - 2, N - 1} with seeded values."""
    rng = np.random.default_rng(4000 + seed + N % 1009)
    four = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    support = [((0,), (AMPLITUDE,)), ((N - 1,), (AMPLITUDE,)), ((1, N // 2, N - 2, N - 1), tuple(four))]
    x = np.zeros((3, N), dtype=np.complex128)
    for t, (points, values) in enumerate(support):
        x[t, list(points)] = values
    return x, support


def tiny_pool():
    """Sixteen tiny FIDs for the call of more than 32768 spectra: n in {2, 4, 8, 64}, T in {1, 2}, one all-zero FID and
    one that is not finite."""
    pool = [fs.sample_fid(n, T, seed=300 + 10 * k + T) for k, n in enumerate((2, 4, 8, 64, 8, 4, 64)) for T in (1, 2)]
    pool.append(np.zeros((2, 8), dtype=np.complex128))
    bad = fs.sample_fid(4, 2, seed=399)
    bad[1, 2] = np.inf
    pool.append(bad)
    assert len(pool) == 16
    return pool


def stacked_same(got, alone):
    """Every tuple of ``got`` equals the tuple ``alone`` bit for bit (any NaN equal to any NaN), compared as stacks."""
    for piece, want in zip(zip(*got), alone):
        have = np.stack([np.asarray(g) for g in piece])
        have = have.view(np.float64) if np.iscomplexobj(have) else have
        want = np.asarray(want)
        want = want.view(np.float64) if np.iscomplexobj(want) else want
        if not fs.same_values(have, np.broadcast_to(want, have.shape)):
            return False
    return True
