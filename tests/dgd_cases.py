"""Shared inputs of the fused DGD round's tests (tests/test_dgd_ref_host.py on
the CPU, tests/test_dgd_graphs_gpu.py on the GPU): one irregular graph builder,
one generator of non-finite inputs, the saturation points of the logistic
step, the fp64 reference of the local steps, and a host restatement of the
parameter-major launch geometry with the shapes the GPU tests run.  A plain
module (no fixtures): tests import it by name, tests/ being on sys.path."""
import functools

import numpy as np
import torch

from dolhip import graph as G

LOGISTIC_TOL = dict(rtol=2e-6, atol=1e-6)  # tests/test_dgd_gpu.py states why

# Row degrees of irregular_csr, in cycle order.  The period is 11, coprime to 8
# and 16: rows r and r + 8 (the two passes of one thread of csr_xcd_kernel<32, 2>)
# meet as (4, 4), (4, other), (other, 4) and (other, other), and every 16-row
# block, 4-row quad and 64-lane wave holds mixed degrees.
DEGREES = [0, 1, 2, 3, 4, 4, 5, 8, 15, 16, 40]


def row_degrees(n_rows, x_rows):
    """Row r has DEGREES[(r - 1) % 11] (row 0 the longest), capped at x_rows;
    the last row is empty and the row before it long."""
    if n_rows < 3:
        raise ValueError("irregular_csr needs >= 3 rows (a long first row, a long row, an empty last row)")
    d = np.array([DEGREES[(r - 1) % len(DEGREES)] for r in range(n_rows)])
    d[n_rows - 2] = DEGREES[-1]
    d[n_rows - 1] = 0
    return np.minimum(d, x_rows)


@functools.lru_cache(maxsize=None)
def irregular_csr(n_rows, x_rows, seed):
    """An n_rows x x_rows mixing matrix with every row shape a CSR kernel
    distinguishes: degrees 0, 1, 2, 3, 4 (the register / fast-path width), 5,
    8, 15, 16 and 40 (the long-row fallback) in one graph.  Columns ascend
    without duplicates; rows 0 and n_rows - 2 hold column 0 and column
    x_rows - 1.  Weights are float32 in (0, 1]; one of them is 1e-40 (a
    subnormal: its product underflows).  Validated: every column is in
    [0, x_rows).  Cached: callers must not write into the arrays."""
    rng = np.random.default_rng(seed)
    deg = row_degrees(n_rows, x_rows)
    col = []
    for r, d in enumerate(deg):
        if r in (0, n_rows - 2) and 2 <= d < x_rows:  # both end columns, the rest from between them
            c = np.concatenate([[0, x_rows - 1], 1 + rng.choice(x_rows - 2, d - 2, replace=False)])
        else:
            c = rng.choice(x_rows, d, replace=False)
        col.append(np.sort(c))
    col = np.concatenate(col).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    val = (1.0 - rng.random(col.size)).astype(np.float32)
    val[rng.integers(col.size)] = 1e-40
    assert val.min() > 0 and val.max() <= 1 and 0 in col and x_rows - 1 in col
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return G.CSR(n_rows, x_rows, rowptr, col, val).validate()


def special(n, P, seed, scale=1.0):
    """N(0, scale) float32 [n, P] with NaN, +/-Inf, -0.0, 3e38 and a subnormal
    at seeded places (special_x of tests/test_slab_gpu.py, with a scale)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, P)) * scale).astype(np.float32)
    for value, count in ((np.nan, 3), (np.inf, 3), (-np.inf, 3), (-0.0, 5), (3e38, 5), (1e-40, 5)):
        X[rng.integers(0, n, count), rng.integers(0, P, count)] = value
    return X


def normal(n, P, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, P)) * scale).astype(np.float32)


# The logistic step where expf leaves its easy range, one plain step at lr 0.1:
# t x = +/-100 (g = -0 / g = -t: exp underflows to a subnormal), 100 (exp
# overflows at 88.73), +/-Inf (x t = +/-1e60), x = +/-0 (g = -t / 2), and 88.7
# / 88.8 on either side of the overflow (88.7: g = -3e-39, a subnormal quotient).
SAT_X = np.array([100, -100, 50, 1e30, -1e30, 0, -0.0, 88.7, 88.8], np.float32)
SAT_T = np.array([1, 1, 2, 1e30, 1e30, 3, 3, 1, 1], np.float32)
SAT_LR = 0.1
SAT_WANT = np.array([100, -99.9, 50, 1e30, -9e29, 0.15, 0.15, 88.7, 88.8], np.float32)


def dgd_local_fp64(Y, T, M, steps, lr, momentum, first):
    """The logistic local steps the way the reference's client takes them
    (DIST/clients.py:43-49): fp64 torch.optim.SGD(lr, momentum) on
    softplus(-t x).sum(); a continuing momentum buffer starts from M.
    Returns (x, buffer) as fp64 arrays (buffer None without momentum)."""
    x = torch.tensor(np.asarray(Y, np.float64), requires_grad=True)
    t = torch.tensor(np.asarray(T, np.float64))
    opt = torch.optim.SGD([x], lr=float(np.float32(lr)), momentum=float(np.float32(momentum)))
    if momentum and not first:
        opt.state[x]["momentum_buffer"] = torch.tensor(np.asarray(M, np.float64))
    for _ in range(steps):
        opt.zero_grad()
        torch.nn.functional.softplus(-t * x).sum().backward()
        opt.step()
    buf = opt.state[x]["momentum_buffer"].numpy() if momentum else None
    return x.detach().numpy(), buf


# ----------------------------------------------------------------------------
# The parameter-major launch geometry (csrc/pmajor.hip, mix_csr_pm_impl)
# ----------------------------------------------------------------------------
K_T1 = 1024          # kT1: threads per workgroup
PM_MAX = 8192        # kMaxAgents
PM_DGD_MAX = 4096    # the fused round's limit (nq > kT1 || xw > 4096 is refused)


def pm_geometry(x_rows, n_rows, ne):
    """mix_csr_pm_impl's geometry for XT of x_rows agents, YT of n_rows agents
    and ne epilogue operands staged per p-row (0 the plain mix, 1 a target, 2
    target + momentum: `ne = obj < 0 ? 0 : (mode == 2 ? 2 : 1)`).  Restates, in
    the order of the function body:
      xw = (x_rows + 255) / 256 * 256; nq = (n_rows + 3) / 4; nw = 4 * nq
      big = nq > kT1 || xw > 4096
      SF = big ? 8192 : (ne == 2 ? 20480 : 16384)
      sr = SF / (xw + ne * nw)
      !big: qp_log2 = ceil(log2(nq)); gr = kT1 >> qp_log2;
            if (sr >= gr) sr = min(sr / gr * gr, 4 * gr); spt = (sr + gr - 1) / gr
      big:  sr = 1; spt = 2   (two quads per thread: QPT = 2, GR = 1)"""
    xw = (x_rows + 255) // 256 * 256
    nq = (n_rows + 3) // 4
    nw = 4 * nq
    big = nq > K_T1 or xw > 4096
    SF = 8192 if big else (20480 if ne == 2 else 16384)
    sr = SF // (xw + ne * nw)
    qp_log2 = 0
    if not big:
        while (1 << qp_log2) < nq:
            qp_log2 += 1
        gr = K_T1 >> qp_log2
        if sr >= gr:
            sr = min(sr // gr * gr, 4 * gr)
        spt = (sr + gr - 1) // gr
    else:
        gr, sr, spt = 1, 1, 2
    return dict(xw=xw, nq=nq, nw=nw, big=big, SF=SF, sr=sr, qp_log2=qp_log2, gr=gr, spt=spt)


def pm_classes(x_rows, n_rows, ne):
    """The names of the geometry classes one launch belongs to."""
    g = pm_geometry(x_rows, n_rows, ne)
    if g["big"]:
        c = set()
        if g["nq"] > K_T1:
            c.add("big by nq")
        if g["xw"] > 4096:
            c.add("big by xw")
        return c
    c = {f"spt {g['spt']}", f"SF {g['SF']}"}
    sr0 = g["SF"] // (g["xw"] + ne * g["nw"])
    if sr0 < g["gr"]:
        c.add("sr < gr")
    elif sr0 // g["gr"] >= 4:
        c.add("sr capped at 4 gr")
    else:
        c.add("sr a multiple of gr below the cap")
    return c


# (x_rows, n_rows) of the GPU tests, P in PM_P each.  (200, 1026) is the fused
# round's only shape with sr capped at 4 gr (spt 4) under both stage sizes;
# (100, 100) and (1100, 516) give the plain mix spt 2 and spt 3
# (tests/test_dgd_ref_host.py checks the cover).
PM_DGD_SHAPES = [(5, 5), (100, 100), (257, 257), (1025, 1025), (3000, 3000), (4096, 4096), (64, 1000), (4096, 100),
                 (100, 4096), (4096, 9), (200, 1026)]
PM_MIX_SHAPES = [(5000, 5000), (8192, 8192), (8190, 8190), (5000, 50), (50, 5000), (4096, 9), (100, 4096),
                 (100, 100), (1100, 516)]
PM_P = [1, 7, 300]
