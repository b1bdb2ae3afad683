"""Objectives and gradients (drop-in for obj_problems.py), evaluated on the GPU.

Same names, signatures, return types and edge cases as the reference:
  logistic_objective(w, X, y, lambda_reg)            obj_problems.py:3-11
  logistic_stochastic_gradient(w, Xb, yb, lambda_reg) obj_problems.py:13-20
  logistic_full_gradient(w, workers, lambda_reg)     obj_problems.py:22-36
  quadratic_objective(w, X, y, mu_reg)               obj_problems.py:39-44
  quadratic_stochastic_gradient(w, Xb, yb, mu_reg)   obj_problems.py:46-53
  quadratic_full_gradient(w, workers, mu_reg)        obj_problems.py:55-69
Empty inputs return 0.0 / zeros_like(w) on the host exactly as upstream; every
other call runs the float64 HIP kernels through libdopt.so (no CPU fallback).
The trainers do NOT call these per worker: their rounds run batched on the
device (trainer.py in this package).

softmax_objective / softmax_gradient have no counterpart upstream: they are the
readable definition of the multinomial logistic objective that Engine.run_softmax
optimises, in plain numpy float64 on the host (no device path).
"""
import numpy as np

import _dopt


def _eng():
    return _dopt.default_engine()


def logistic_objective(w, X, y, lambda_reg):
    if X.shape[0] == 0:
        return 0.0
    return _eng().eval_objective("logistic", w, X, y, lambda_reg)


def logistic_stochastic_gradient(w, X_batch, y_batch, lambda_reg):
    if X_batch.shape[0] == 0:
        return np.zeros_like(w)
    return _eng().eval_gradient("logistic", w, X_batch, y_batch, lambda_reg)


def _full(problem, w, workers, reg):
    Xs = [wk.X_local for wk in workers if wk.X_local.shape[0] > 0]
    if not Xs:
        return np.zeros_like(w)
    ys = [wk.y_local for wk in workers if wk.X_local.shape[0] > 0]
    # sum over every shard / total rows + reg * w == the gradient over the union
    return _eng().eval_gradient(problem, w, np.vstack(Xs), np.concatenate(ys), reg)


def logistic_full_gradient(w, workers, lambda_reg):
    """full gradient for across all workers' data."""
    return _full("logistic", w, workers, lambda_reg)


def quadratic_objective(w, X, y, mu_reg):
    if X.shape[0] == 0:
        return 0.0
    return _eng().eval_objective("quadratic", w, X, y, mu_reg)


def quadratic_stochastic_gradient(w, X_batch, y_batch, mu_reg):
    if X_batch.shape[0] == 0:
        return np.zeros_like(w)
    return _eng().eval_gradient("quadratic", w, X_batch, y_batch, mu_reg)


def quadratic_full_gradient(w, workers, mu_reg):
    """full gradient across all workers' data"""
    return _full("quadratic", w, workers, mu_reg)


def _softmax_terms(W, X, y):
    """Max-subtracted log-sum-exp and probabilities of the rows: z = X W^T, (lse [m], P [m x C])."""
    z = np.asarray(X, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    zmax = z.max(axis=1, keepdims=True)
    e = np.exp(z - zmax)
    s = e.sum(axis=1, keepdims=True)
    return z, (zmax + np.log(s))[:, 0], e / s


def softmax_objective(W, X, y, reg):
    """(1/m) sum_k (logsumexp(W x_k) - (W x_k)[y_k]) + (reg / 2) ||W||_F^2; W is C x d, y in {0 .. C-1}.
    Empty data gives 0.0, as the other objectives."""
    if X.shape[0] == 0:
        return 0.0
    W = np.asarray(W, dtype=np.float64)
    k = np.asarray(y).astype(np.int64)
    z, lse, _ = _softmax_terms(W, X, k)
    return float(np.mean(lse - z[np.arange(len(k)), k]) + 0.5 * reg * np.sum(W * W))


def softmax_gradient(W, X_batch, y_batch, reg):
    """(1/b) sum_k (softmax(W x_k) - e_{y_k}) x_k^T + reg W, C x d; zeros for an empty batch."""
    W = np.asarray(W, dtype=np.float64)
    if X_batch.shape[0] == 0:
        return np.zeros_like(W)
    k = np.asarray(y_batch).astype(np.int64)
    _, _, P = _softmax_terms(W, X_batch, k)
    P[np.arange(len(k)), k] -= 1.0
    return P.T @ np.asarray(X_batch, dtype=np.float64) / len(k) + reg * W
