"""numpy restatement of the neighbourhood moments of include/hidegs_moments.h (test infrastructure): every
rounding of the rule in float32, the fused multiply-adds through nearest_oracle.fma32, the additions in the
rule's order -- the 64 positions of a block one after the other, vectorised over the lists x blocks matrix, then
the blocks in block order.  Also the figures by which the eigen outputs are judged (residual, orthonormality,
eigenvalue error, in float64) for any decomposition, and for single-precision LAPACK on the same matrices."""
import numpy as np

from nearest_oracle import fma32

BLOCK = 64
U = 2.0 ** -24


def gamma(n):
    """n u / (1 - n u): the bound factor of a sum of n terms in any order."""
    return n * U / (1 - n * U)


def bits(a):
    """uint32 bits of float32 values, every NaN as one value (sign and payload are not part of the rule)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def as_lists(neighbors, starts=None, capacity=None):
    """A list of int64 arrays, one per query: of a (Q, k) table its rows; of CSR (rows, starts) the positions
    max(starts[j], 0) .. min(starts[j + 1], capacity) of rows."""
    neighbors = np.asarray(neighbors)
    if starts is None:
        assert neighbors.ndim == 2
        return [row.astype(np.int64) for row in neighbors]
    cap = len(neighbors) if capacity is None else capacity
    out = []
    for j in range(len(starts) - 1):
        a, e = max(int(starts[j]), 0), min(int(starts[j + 1]), cap)
        out.append(neighbors[a:e].astype(np.int64) if e > a else np.zeros(0, np.int64))
    return out


def _padded(lists):
    """(n, nb, width) int64 entries, -1 past a list's end, and (n,) the blocks of every list.  width is 64, or
    the longest list where no list has a second block (an invalid entry adds nothing, so neither does padding)."""
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    longest = int(lens.max()) if len(lists) else 0
    nb = max(1, -(-longest // BLOCK))
    width = BLOCK if nb > 1 else max(1, longest)
    E = np.full((len(lists), nb * width), -1, dtype=np.int64)
    if len(lists) and (lens == longest).all():
        E[:, :longest] = np.asarray(lists, dtype=np.int64).reshape(len(lists), longest)
    else:
        for j, x in enumerate(lists):
            E[j, :len(x)] = x
    return E.reshape(len(lists), nb, width), -(-lens // BLOCK)


def _totals(partials, blocks):
    """Block 0's partial plus those of blocks 1, 2, ... of the list's own blocks, in block order.
    partials: (n, nb, C) float32."""
    total = partials[:, 0].copy()
    for b in range(1, partials.shape[1]):
        total = np.where((b < blocks)[:, None], total + partials[:, b], total)
    return total


def moments(points, lists, weights=None):
    """(count int32 (n,), mean float32 (n, 3), cov float32 (n, 6)) of `lists` (a list of integer arrays, or a
    2-D table) over points (P, 3) float32 and weights (P,) float32 or None, by the rule of the header."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = len(points)
    if not isinstance(lists, list):
        lists = as_lists(lists)
    n = len(lists)
    count, mean, cov = np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32)
    # lists of like length together, so that the padding to the longest of them stays small
    size_class = np.array([max(len(x) - 1, 0).bit_length() if len(x) > BLOCK else 0 for x in lists], dtype=np.int64)
    for c in np.unique(size_class):
        at = np.flatnonzero(size_class == c)
        count[at], mean[at], cov[at] = _moments([lists[j] for j in at], points, weights)
    return count, mean, cov


def _moments(lists, points, weights):
    """moments() of lists that are padded to the longest of them."""
    n, P = len(lists), len(points)
    E, blocks = _padded(lists)
    inside = (E >= 0) & (E < P)
    r = np.where(inside, E, 0)
    if P == 0:
        pts = np.zeros(E.shape + (3,), np.float32)
        valid = inside
        w = np.ones(E.shape, np.float32)
    else:
        pts = points[r]
        valid = inside & np.isfinite(pts).all(-1)
        w = np.ones(E.shape, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)[r]
    nb = E.shape[1]
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    with np.errstate(all="ignore"):
        part = np.zeros((n, nb, 4), np.float32)   # W, Sx, Sy, Sz
        for i in range(E.shape[2]):
            v, wi = valid[:, :, i], w[:, :, i]
            part[:, :, 0] = np.where(v, part[:, :, 0] + wi, part[:, :, 0])
            for c in range(3):
                part[:, :, 1 + c] = np.where(v, fma32(f64(wi), f64(pts[:, :, i, c]), f64(part[:, :, 1 + c])), part[:, :, 1 + c])
        tot = _totals(part, blocks)
        W = tot[:, 0]
        mean = (tot[:, 1:] / W[:, None]).astype(np.float32)
        part = np.zeros((n, nb, 6), np.float32)   # xx, xy, xz, yy, yz, zz
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        for i in range(E.shape[2]):
            v, wi = valid[:, :, i], w[:, :, i]
            d = (pts[:, :, i, :] - mean[:, None, :]).astype(np.float32)
            t = (wi[:, :, None] * d).astype(np.float32)
            for s, (a, b) in enumerate(pairs):
                part[:, :, s] = np.where(v, fma32(f64(t[:, :, a]), f64(d[:, :, b]), f64(part[:, :, s])), part[:, :, s])
        cov = (_totals(part, blocks) / W[:, None]).astype(np.float32)
    count = valid.reshape(n, -1).sum(1).astype(np.int32)
    return count, mean, cov


def full(cov6):
    """(n, 3, 3) symmetric matrices of (n, 6) xx, xy, xz, yy, yz, zz."""
    c = np.asarray(cov6)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def six(A):
    """(n, 6) of (n, 3, 3)."""
    return np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], axis=1)


def eigen_figures(cov6, evals, evecs):
    """(residual, orthonormality, eigenvalue error): the worst over the matrices, everything promoted to float64.
    evecs' rows are the eigenvectors.  Matrices of Frobenius norm 0 are left out (their eigenvalues must be 0
    exactly: `zero_norm_evals_are_zero`)."""
    A = full(np.asarray(cov6, dtype=np.float64))
    lam = np.asarray(evals, dtype=np.float64)
    V = np.asarray(evecs, dtype=np.float64)
    norm = np.sqrt((A * A).sum((1, 2)))
    keep = norm > 0
    orth = np.abs(V @ V.transpose(0, 2, 1) - np.eye(3)).max() if len(A) else 0.0
    if not keep.any():
        return 0.0, float(orth), 0.0
    A, lam, V, norm = A[keep], lam[keep], V[keep], norm[keep]
    Av = np.einsum("nab,nib->nia", A, V)                       # row i: A v_i
    res = np.sqrt(((Av - lam[:, :, None] * V) ** 2).sum(2)).max(1) / norm
    ref = np.linalg.eigvalsh(A)
    err = np.abs(lam - ref).max(1) / norm
    return float(res.max()), float(orth), float(err.max())


def zero_norm_evals_are_zero(cov6, evals):
    A = np.asarray(cov6, dtype=np.float64)
    zero = (A == 0).all(1)
    return bool((np.asarray(evals)[zero] == 0).all())


def lapack_figures(cov6):
    """The same three figures for numpy.linalg.eigh of the float32 matrices: LAPACK in single precision."""
    A = full(np.ascontiguousarray(cov6, dtype=np.float32))
    lam, vec = np.linalg.eigh(A)
    assert lam.dtype == np.float32 and vec.dtype == np.float32
    return eigen_figures(cov6, lam, vec.transpose(0, 2, 1))


FLOOR = 2.0 ** -24
FACTOR = 8.0


def eigen_bounds(cov6):
    """What the kernel's worst figures over a family may be: 8 x max(LAPACK's worst, 2^-24), per figure."""
    return tuple(FACTOR * max(f, FLOOR) for f in lapack_figures(cov6))


def sign_rule_holds(evecs):
    """Rows 0 and 1: the component of largest magnitude (lowest index among equals) is positive; det > 0."""
    V = np.asarray(evecs, dtype=np.float32)
    top = np.abs(V[:, :2, :]).argmax(2)                        # argmax takes the lowest index among equals
    lead = np.take_along_axis(V[:, :2, :], top[:, :, None], 2)[:, :, 0]
    return bool((lead > 0).all()) and bool((np.linalg.det(V.astype(np.float64)) > 0).all())


def rotations(n, rng):
    """(n, 3, 3) float64 random rotations (QR of Gaussian matrices, det made +1)."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q


def crafted(spectrum, n, rng, scale=1.0):
    """(n, 6) float32: R diag(spectrum) R^T in float64 with random rotations, scaled, rounded to fp32 (the six
    kept entries are the symmetrised matrix)."""
    R = rotations(n, rng)
    A = np.einsum("nab,b,ncb->nac", R, np.asarray(spectrum, dtype=np.float64), R) * scale
    A = 0.5 * (A + A.transpose(0, 2, 1))
    return six(A).astype(np.float32)
