"""Host restatement of one push-sum gradient-tracking round
(dol_gt_push_csr_f32, ops.gt_push_csr), shared by tests/test_gt_push_host.py
(CPU) and tests/test_gt_push_gpu.py (GPU).  Built like gt_cases.gt_round, from
golden-pinned oracle calls and single numpy float32 operations:

  au, as   oracle.mix_csr on U and on S           (+0 start, ascending e, no FMA)
  av       oracle.mix_csr on v[:, None]           (the same rounding on the n-vector)
  self w   gt_cases.add_self on all three: fl(a + fl(d a_i))
  u'       gt_cases.sgd_step(au, S, lr): fmaf(-lr, s, au)
  z, z'    fl(u / v), fl(u' / av)                 numpy float32 division, correctly rounded
  s'       fl(fl(as + g(z', t)) - g(z, t))        numpy float32
  v'       av

C = c + diag(d) is column-stochastic; row i of c lists i's in-neighbours.
Matrices are agent-major [n, P], v is [n].  `grad` as in gt_cases.gt_round.
Below it, the graphs the two tiers share: digraph(n), the reference ring's W as
column-stochastic weights, and gt_cases.irregular under this module's name."""
import functools

import numpy as np

import gt_cases
import oracle
from gt_cases import F32, irregular, ls_grad  # noqa: F401  (irregular: used through this module too)


def gt_push_round(U, S, T, v, c, d, lr, grad=ls_grad):
    """(U', S', v') of one round on agent-major U, S, T [n, P] and v [n] with C = c + diag(d)."""
    U, S, T = (np.ascontiguousarray(a, F32) for a in (U, S, T))
    vc = np.ascontiguousarray(np.asarray(v, F32)[:, None])
    au = gt_cases.add_self(oracle.mix_csr(U, c.rowptr, c.col, c.val), d, U)
    as_ = gt_cases.add_self(oracle.mix_csr(S, c.rowptr, c.col, c.val), d, S)
    av = gt_cases.add_self(oracle.mix_csr(vc, c.rowptr, c.col, c.val), d, vc)
    Un = gt_cases.sgd_step(au, S, lr)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        z = (U / vc).astype(F32)
        zn = (Un / av).astype(F32)
        Sn = ((as_ + grad(zn, T)).astype(F32) - grad(z, T)).astype(F32)
    return Un, Sn, np.ascontiguousarray(av[:, 0])


def estimate(U, v):
    """z = U / v in fp64 (a read-out)."""
    return np.asarray(U, np.float64) / np.asarray(v, np.float64)[:, None]


@functools.lru_cache(maxsize=None)
def digraph(n):
    """The irregular directed pattern i -> i+1, i -> i+3 and, for i % 3 == 0,
    i -> i+2 (mod n), as a CSR whose row j lists j's in-neighbours.  Strongly
    connected (it holds the cycle i -> i+1); out-degrees 2 and 3."""
    from dolhip import graph as G
    A = np.zeros((n, n), F32)
    for i in range(n):
        for k in (1, 3) + ((2,) if i % 3 == 0 else ()):
            A[(i + k) % n, i] = 1.0
    return G.csr_from_dense(A).validate()


@functools.lru_cache(maxsize=None)
def reference_ring_weights(n):
    """(C_off, d) from gt_cases.ring(n)'s W, the reference's row-stochastic
    circle: C = 1/2 (I + W^T), that is C_off = fl(W^T / 2) (exact: a power of
    two) and d = 1/2 -- column-stochastic with a positive diagonal."""
    from dolhip import graph as G
    wt = gt_cases.ring(n)[0].transpose()
    c = G.CSR(wt.n_rows, wt.n_cols, wt.rowptr, wt.col, (wt.val * F32(0.5)).astype(F32)).validate()
    return c, np.full(n, 0.5, F32)
