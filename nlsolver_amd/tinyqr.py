"""Host-side mirror of the reference's tinyqr::lm for batches of systems on the device.

Reference interface (tinyqr.h:461-470):
    std::vector<T> lm(const std::vector<T>& X, const std::vector<T>& y, T tol = 1e-12)
with X column-major n x p (n = y.size(), p = X.size() / n), one system per call. Here lm() takes
one system — X of shape (p, n), i.e. the same memory — or a batch (batch, p, n) with y (batch, n),
solved side by side on the GPU (n >= p, p <= 64). There is no CPU fallback.
qr_decomposition() and lm(..., reference_order=True) run the reference's own order of operations
on the device (nlsg_tinyqr_qr): Q, R and beta equal the reference's bit for bit, any p.
"""
import numpy as np

from ._capi import check, lib
from ._engine import pd_of, timed_ms


def _reference_order(X, y, tol, device, want_q, want_r, want_beta):
    """nlsg_tinyqr_qr: the reference's own order of operations on the device (a parity mode)."""
    batch, p, n = X.shape
    Q = np.empty((batch, p, n)) if want_q else None
    R = np.empty((batch, p, p)) if want_r else None
    beta = np.empty((batch, p)) if want_beta else None
    check(lib().nlsg_tinyqr_qr(pd_of(X), pd_of(y), batch, n, p, float(tol), device, pd_of(Q), pd_of(R),
                               pd_of(beta)))
    return Q, R, beta


def qr_decomposition(X, tol=1e-8, *, device=0):
    """tinyqr::qr_decomposition(X, n, p, tol) (tinyqr.h:291-310) per system on the device, in the
    reference's order of operations: returns (Q, R) with Q[..., i, j] = the reference's Q[i * n + j]
    (the thin Q, p rows of n) and R[..., j, i] = its R[j * p + i] = R(i, j) — bit for bit.
    X: (p, n) or (batch, p, n), the column-major n x p systems; n >= p, n + p <= 1280."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    single = X.ndim == 2
    if single:
        X = X[None]
    if X.ndim != 3:
        raise TypeError("X must be (p, n) or (batch, p, n) [column-major n x p systems]")
    Q, R, _ = _reference_order(X, None, tol, device, True, True, False)
    return (Q[0], R[0]) if single else (Q, R)


def lm(X, y, tol=1e-12, *, device=0, return_ms=False, reference_order=False):
    """Least-squares coefficients beta (p,) or (batch, p): tinyqr::lm(X, y, tol) per system.
    X[..., j, i] is element (i, j) of the system's n x p matrix (column-major, as tinyqr takes it).
    reference_order=True: the parity mode — Q formed, the reference's summation orders, beta equal to
    the reference's bit for bit (slower: one wave per system, serial rotations).
    As in the reference, two zeros stacked in a pivot column are 0 / 0 in the Givens pair: a zero column,
    a one-hot design or zero rows at the bottom return NaN in every coefficient of THAT system (its
    neighbours in the batch are untouched), and entries of R below tol are read as 0 and divided by
    (a column scaled to 2^-160 needs tol = 0). DESIGN.md §6c, "Off the benign path"."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    single = X.ndim == 2
    if single:
        X, y = X[None], y[None]
    if X.ndim != 3 or y.ndim != 2 or y.shape != (X.shape[0], X.shape[2]):
        raise TypeError("X must be (batch, p, n) [column-major n x p systems] and y (batch, n)")
    batch, p, n = X.shape
    if reference_order:
        beta = _reference_order(X, y, tol, device, False, False, True)[2]
        return beta[0] if single else beta
    beta = np.empty((batch, p))
    ms = timed_ms(lib().nlsg_tinyqr_lm, pd_of(X), pd_of(y), batch, n, p, float(tol), device, pd_of(beta))
    out = beta[0] if single else beta
    return (out, ms) if return_ms else out
