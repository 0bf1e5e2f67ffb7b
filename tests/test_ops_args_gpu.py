"""dolhip.ops argument rules, pinned without launching anything.

ops.py is the only check between a caller's tensors and kernels that trust
their arguments.  Every test here replaces ops._native.call by a recorder, so
no kernel runs -- not with good arguments and above all not with bad ones.

ACCEPT: valid calls; the recorded (entry point, arguments) is compared with a
literal, pointers written as "<tensor>+<byte offset>" ("alloc" for a buffer
the wrapper allocated itself) and the stream as "stream".
REJECT: one argument wrong per call; exception type, full message text and an
empty recorder.  The generic row-matrix rules (CPU tensor, dtype, rank, inner
stride, columns < P) are generated for every row matrix of every op from
CALLS; the rest is listed op by op.

tests/test_ops_args_host.py reuses CALLS for its CPU-tensor sweep.
"""
import pytest
import torch

from dolhip import ops
from dolhip.ops import DolNativeError

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def mat(dev, rows, cols, ld=None, dtype=F32):
    """[rows, cols] view of a [rows, ld] matrix (ld > cols: padded rows)."""
    return torch.zeros(rows, ld or cols, dtype=dtype, device=dev)[:, :cols]


def vec(dev, n, dtype=F32):
    return torch.zeros(n, dtype=dtype, device=dev)


def ids(dev, *values):
    return torch.tensor(values, dtype=I32, device=dev)


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append((name, args))


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


def named(calls, tensors, dev):
    """The recorded calls with every pointer replaced by "<name>+<offset>" of
    the tensor whose storage holds it and the trailing stream by "stream"."""
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    spans = []
    for k, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.numel():
            s = t.untyped_storage()
            spans.append((k, t.data_ptr(), s.data_ptr(), s.data_ptr() + s.nbytes()))
    out = []
    for name, args in calls:
        assert args[-1] == stream, "the last argument is the current stream"
        row = [name]
        for a in args[:-1]:
            if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 32:
                hit = [f"{k}+{a - p}" for k, p, lo, hi in spans if lo <= a < hi]
                a = hit[0] if hit else "alloc"
            row.append(a)
        out.append(tuple(row) + ("stream",))
    return out


# ---------------------------------------------------------------------------
# CALLS: per op, (make(dev) -> arguments by name, call(t)).  The arguments are
# the smallest valid set with every optional tensor present and momentum on;
# P (and its like) is passed explicitly so one narrower matrix is one fault.
# Row matrices carry the name the messages use.  ROWS: the row matrices of
# each op and the P their columns are checked against (None: not checked).
# ---------------------------------------------------------------------------
def _csr(dev, nnz=4):
    return dict(rowptr=vec(dev, 3, I32), col=vec(dev, nnz, I32), val=vec(dev, nnz))


def _ring(dev, halos=True):
    return dict(X=mat(dev, 4, 10, 12), Y=mat(dev, 4, 10, 12), w_prev=vec(dev, 4), w_next=vec(dev, 4),
                halo_prev=vec(dev, 10) if halos else None, halo_next=vec(dev, 10) if halos else None, P=10, n_rows=4)


def _dgd(dev, rows=4):
    return dict(target=mat(dev, rows, 10, 12), mom=mat(dev, rows, 10, 12), objective="logistic", steps=2, lr=0.5,
                momentum=0.25, first_step=True)


def _pm(dev):
    return dict(XT=mat(dev, 10, 2, 4), YT=mat(dev, 10, 2, 4), **_csr(dev), x_agents=None, P=10, nseg=16)


def _admm(dev):
    return dict(w=mat(dev, 2, 10, 12), alpha=mat(dev, 2, 10, 12), target=mat(dev, 2, 10, 12), theta=vec(dev, 10),
                agents=ids(dev, 1, 0), first=vec(dev, 2, I32), buf=mat(dev, 2, 10, 12), rho=0.5, lr=0.25,
                momentum=0.125, local_steps=3, work=None, P=10)


def _mlp(dev):
    return dict(w=mat(dev, 2, 30, 32), X=torch.zeros(2, 2, 4, device=dev), y=torch.zeros(2, 2, dtype=I64, device=dev),
                grad=mat(dev, 2, 30, 32), mom=mat(dev, 2, 30, 32), theta=vec(dev, 30), alpha=mat(dev, 2, 30, 32),
                loss=vec(dev, 2), lr=0.5, momentum=0.25, rho=0.125, first_step=True, update=True, work=None)


def _slab(dev):
    hdr_len = int(ops._native.lib().dol_csr_slab_hdr_len(2, 2))
    return dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), ent=vec(dev, 8, I32), hdr=vec(dev, hdr_len, I32),
                n_rows=2, x_rows=2, P=10)


_DGD_KW = ("objective", "steps", "lr", "momentum", "first_step")


def _kw(t, *names):
    return {k: t[k] for k in names}


CALLS = {
    "mix_csr": (lambda dev: dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), **_csr(dev), P=10),
                lambda t: ops.mix_csr(t["X"], t["Y"], t["rowptr"], t["col"], t["val"], P=t["P"])),
    "mix_csr_pm": (_pm, lambda t: ops.mix_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"],
                                                 **_kw(t, "x_agents", "P", "nseg"))),
    "dgd_csr_pm": (lambda dev: dict(_pm(dev), TT=mat(dev, 10, 2, 4), MT=mat(dev, 10, 2, 4), objective="logistic",
                                    steps=2, lr=0.5, momentum=0.25, first_step=True),
                   lambda t: ops.dgd_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], t["TT"], t["MT"],
                                            **_kw(t, *_DGD_KW, "x_agents", "P", "nseg"))),
    "csr_slab_pack": (lambda dev: dict(_csr(dev), x_rows=2, ent=None, hdr=None, balance=False),
                      lambda t: ops.csr_slab_pack(t["rowptr"], t["col"], t["val"], t["x_rows"], t["ent"], t["hdr"],
                                                  t["balance"])),
    "mix_csr_slab": (_slab, lambda t: ops.mix_csr_slab(t["X"], t["Y"], t["ent"], t["hdr"], t["n_rows"], t["x_rows"],
                                                       t["P"])),
    "dense_to_csr": (lambda dev: dict(W=mat(dev, 2, 3, 4), rowptr=None, col=None, val=None),
                     lambda t: ops.dense_to_csr(t["W"], t["rowptr"], t["col"], t["val"])),
    "transpose": (lambda dev: dict(A=mat(dev, 2, 10, 12), B=mat(dev, 10, 2, 4), rows=2, cols=10),
                  lambda t: ops.transpose(t["A"], t["B"], t["rows"], t["cols"])),
    "mix_ring_steps": (lambda dev: dict(X=mat(dev, 4, 8), Y=mat(dev, 4, 8), w_prev=vec(dev, 4), w_next=vec(dev, 4),
                                        steps=2, P=8, n_rows=4, variant=3),
                       lambda t: ops.mix_ring_steps(t["X"], t["Y"], t["w_prev"], t["w_next"], t["steps"], t["P"],
                                                    t["n_rows"], t["variant"])),
    "mix_ring": (_ring, lambda t: ops.mix_ring(t["X"], t["Y"], t["w_prev"], t["w_next"], t["halo_prev"],
                                               t["halo_next"], t["P"], t["n_rows"])),
    "mix_ring_edges": (_ring, lambda t: ops.mix_ring_edges(t["X"], t["Y"], t["w_prev"], t["w_next"], t["halo_prev"],
                                                           t["halo_next"], t["P"], t["n_rows"])),
    "dgd_ring": (lambda dev: dict(_ring(dev), **_dgd(dev)),
                 lambda t: ops.dgd_ring(t["X"], t["Y"], t["w_prev"], t["w_next"], t["target"], t["mom"],
                                        **_kw(t, *_DGD_KW, "halo_prev", "halo_next", "P", "n_rows"))),
    "dgd_ring_edges": (lambda dev: dict(_ring(dev), **_dgd(dev)),
                       lambda t: ops.dgd_ring_edges(t["X"], t["Y"], t["w_prev"], t["w_next"], t["target"],
                                                    t["halo_prev"], t["halo_next"], t["mom"],
                                                    **_kw(t, *_DGD_KW, "P", "n_rows"))),
    "dgd_csr": (lambda dev: dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), **_csr(dev), **_dgd(dev, 2), P=10),
                lambda t: ops.dgd_csr(t["X"], t["Y"], t["rowptr"], t["col"], t["val"], t["target"], t["mom"],
                                      **_kw(t, *_DGD_KW, "P"))),
    "mix_dense": (lambda dev: dict(W=mat(dev, 2, 2), X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), P=10),
                  lambda t: ops.mix_dense(t["W"], t["X"], t["Y"], t["P"])),
    "mix_dense_split3": (lambda dev: dict(W=mat(dev, 2, 2), X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), P=10,
                                          work=None, w_ready=False, fuse=None),
                         lambda t: ops.mix_dense_split3(t["W"], t["X"], t["Y"], t["P"], t["work"], t["w_ready"],
                                                        t["fuse"])),
    "er_stochastic": (lambda dev: dict(W=mat(dev, 3, 3, 4), p=0.5, seed=7),
                      lambda t: ops.er_stochastic(t["W"], t["p"], t["seed"])),
    "prox_admm_sgd": (lambda dev: dict(w=mat(dev, 2, 10, 12), g=mat(dev, 2, 10, 12), buf=mat(dev, 2, 10, 12),
                                       theta=vec(dev, 10), alpha=mat(dev, 2, 10, 12), rho=0.5, lr=0.25,
                                       momentum=0.125, first_step=True, write_grad=False, P=10),
                      lambda t: ops.prox_admm_sgd(t["w"], t["g"], t["buf"], t["theta"], t["alpha"],
                                                  **_kw(t, "rho", "lr", "momentum", "first_step", "write_grad", "P"))),
    "admm_step_dual": (lambda dev: dict(w=mat(dev, 2, 10, 12), g=mat(dev, 2, 10, 12), theta=vec(dev, 10),
                                        alpha=mat(dev, 2, 10, 12), buf=mat(dev, 2, 10, 12), rho=0.5, lr=0.25,
                                        momentum=0.125, first_step=True, write_grad=False, P=10),
                       lambda t: ops.admm_step_dual(t["w"], t["g"], t["theta"], t["alpha"], t["buf"],
                                                    **_kw(t, "rho", "lr", "momentum", "first_step", "write_grad",
                                                          "P"))),
    "prox_grad": (lambda dev: dict(g=mat(dev, 2, 10, 12), w=mat(dev, 2, 10, 12), theta=vec(dev, 10), rho=0.5,
                                   alpha=mat(dev, 2, 10, 12), P=10),
                  lambda t: ops.prox_grad(t["g"], t["w"], t["theta"], t["rho"], t["alpha"], t["P"])),
    "admm_dual": (lambda dev: dict(alpha=mat(dev, 2, 10, 12), w=mat(dev, 2, 10, 12), theta=vec(dev, 10), rho=0.5,
                                   resid_sq=vec(dev, 2, F64), work=None, P=10),
                  lambda t: ops.admm_dual(t["alpha"], t["w"], t["theta"], t["rho"], t["resid_sq"], t["work"], t["P"])),
    "admm_ls_round": (lambda dev: dict(_admm(dev), resid_sq=vec(dev, 2, F64), alpha_sq=vec(dev, 2, F64)),
                      lambda t: ops.admm_ls_round(t["w"], t["alpha"], t["target"], t["theta"],
                                                  **_kw(t, "agents", "first", "buf", "rho", "lr", "momentum",
                                                        "local_steps", "resid_sq", "alpha_sq", "work", "P"))),
    "admm_ls_round_mean": (lambda dev: dict(_admm(dev), out=vec(dev, 10), scale=None, resid_total=vec(dev, 2, F64),
                                            validate=True),
                           lambda t: ops.admm_ls_round_mean(t["w"], t["alpha"], t["target"], t["theta"],
                                                            **_kw(t, "agents", "first", "buf", "rho", "lr", "momentum",
                                                                  "local_steps", "out", "scale", "resid_total", "work",
                                                                  "P", "validate"))),
    "ordered_mean": (lambda dev: dict(W=mat(dev, 2, 10, 12), order=ids(dev, 1, 0, 1), out=vec(dev, 10), P=10),
                     lambda t: ops.ordered_mean(t["W"], t["order"], t["out"], t["P"])),
    "ordered_sum": (lambda dev: dict(W=mat(dev, 2, 10, 12), order=ids(dev, 1, 0, 1), acc_in=vec(dev, 10),
                                     out=vec(dev, 10), scale=0.5, P=10),
                    lambda t: ops.ordered_sum(t["W"], t["order"], t["acc_in"], t["out"], t["scale"], t["P"])),
    "stream_copy": (lambda dev: dict(src=vec(dev, 6), dst=vec(dev, 6)),
                    lambda t: ops.stream_copy(t["src"], t["dst"])),
    "stream_copy_rows": (lambda dev: dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 10, 12), P=10),
                         lambda t: ops.stream_copy_rows(t["X"], t["Y"], t["P"])),
    "mlp_step": (_mlp, lambda t: ops.mlp_step(t["w"], t["X"], t["y"], 4, 4, 2,
                                              **_kw(t, "grad", "mom", "theta", "alpha", "loss", "lr", "momentum",
                                                    "rho", "first_step", "update", "work"))),
}

ROWS = {
    "mix_csr": {"X": 10, "Y": 10}, "mix_csr_pm": {"XT": None, "YT": None},
    "dgd_csr_pm": {"XT": None, "YT": None, "TT": None, "MT": None}, "csr_slab_pack": {},
    "mix_csr_slab": {"X": 10, "Y": 10}, "dense_to_csr": {"W": None}, "transpose": {"A": 10, "B": 2},
    "mix_ring_steps": {"X": 8, "Y": 8}, "mix_ring": {"X": 10, "Y": 10}, "mix_ring_edges": {"X": 10, "Y": 10},
    "dgd_ring": {"X": 10, "Y": 10, "target": 10, "mom": 10},
    "dgd_ring_edges": {"X": 10, "Y": 10, "target": 10, "mom": 10},
    "dgd_csr": {"X": 10, "Y": 10, "target": 10, "mom": 10}, "mix_dense": {"W": None, "X": 10, "Y": 10},
    "mix_dense_split3": {"W": None, "X": 10, "Y": 10}, "er_stochastic": {"W": None},
    "prox_admm_sgd": {"w": 10, "g": 10, "buf": 10, "alpha": 10},
    "admm_step_dual": {"w": 10, "g": 10, "alpha": 10, "buf": 10}, "prox_grad": {"g": 10, "w": 10, "alpha": 10},
    "admm_dual": {"alpha": 10, "w": 10}, "admm_ls_round": {"w": 10, "alpha": 10, "target": 10, "buf": 10},
    "admm_ls_round_mean": {"w": 10, "alpha": 10, "target": 10, "buf": 10}, "ordered_mean": {"W": 10},
    "ordered_sum": {"W": 10}, "stream_copy": {}, "stream_copy_rows": {"X": 10, "Y": 10},
    "mlp_step": {"w": 30, "grad": 30, "mom": 30, "alpha": 30},
}


def test_every_launching_op_is_in_the_table():
    not_launching = {"DolNativeError", "pm_stage_order", "tune_pm_stage_order", "ring_steps_variant",
                     "tune_ring_steps_variant", "tuned_choices", "autotune_enabled", "ring_steps_choice",
                     "pm_stage_order_choice", "dense_split3_workspace_bytes", "split3_x_flags", "dual_workspace_bytes",
                     "admm_ls_round_workspace_bytes", "slab_layout_ok", "slab_variant"}
    launching = {n for n in ops.__all__ if callable(getattr(ops, n))} - not_launching
    assert launching - {"admm_ls_round_mean"} == set(CALLS) - {"admm_ls_round_mean"}
    assert set(ROWS) == set(CALLS)


# ---------------------------------------------------------------------------
# ACCEPT
# ---------------------------------------------------------------------------
def _split3_need(flags, M=2, K=2, P=10):
    return ops.dense_split3_workspace_bytes(M, K, P, flags)


def _acc_mix_csr(dev):
    t = dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 3, 10, 12), **_csr(dev))
    return t, lambda: ops.mix_csr(t["X"], t["Y"], t["rowptr"], t["col"], t["val"]), [
        ("dol_mix_csr_f32", "X+0", 12, 2, "Y+0", 12, 2, 10, "rowptr+0", "col+0", "val+0", "stream")]


def _acc_mix_csr_empty_one_row(dev):
    t = dict(X=mat(dev, 1, 10), Y=mat(dev, 1, 10), rowptr=vec(dev, 2, I32), col=vec(dev, 0, I32), val=vec(dev, 0))
    return t, lambda: ops.mix_csr(t["X"], t["Y"], t["rowptr"], t["col"], t["val"], P=8), [
        ("dol_mix_csr_f32", "X+0", 10, 1, "Y+0", 10, 1, 8, "rowptr+0", None, None, "stream")]


def _acc_mix_csr_pm_auto(dev):
    t = dict(XT=mat(dev, 10, 3, 4), YT=mat(dev, 10, 2, 4), **_csr(dev))
    return t, lambda: ops.mix_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], x_agents=3), [
        ("dol_mix_csr_pm_ex_f32", "XT+0", 4, 3, "YT+0", 4, 2, 10, "rowptr+0", "col+0", "val+0", 0, "stream")]


def _acc_mix_csr_pm_nseg16(dev):
    # val shorter than col: the parameter-major ops do not compare the lengths
    t = dict(XT=mat(dev, 8, 2, 4), YT=mat(dev, 8, 2, 4), rowptr=vec(dev, 3, I32), col=vec(dev, 4, I32), val=vec(dev, 3))
    return t, lambda: ops.mix_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], nseg=16), [
        ("dol_mix_csr_pm_ex_f32", "XT+0", 4, 2, "YT+0", 4, 2, 8, "rowptr+0", "col+0", "val+0", 16, "stream")]


def _acc_mix_csr_pm_empty(dev):
    t = dict(XT=mat(dev, 1, 2), YT=mat(dev, 1, 2), rowptr=vec(dev, 3, I32), col=vec(dev, 0, I32), val=vec(dev, 0))
    return t, lambda: ops.mix_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], nseg=0), [
        ("dol_mix_csr_pm_ex_f32", "XT+0", 2, 2, "YT+0", 2, 2, 1, "rowptr+0", None, None, 0, "stream")]


def _acc_dgd_csr_pm_auto(dev):
    t = CALLS["dgd_csr_pm"][0](dev)
    t["nseg"] = None
    return t, lambda: CALLS["dgd_csr_pm"][1](t), [
        ("dol_dgd_csr_pm_ex_f32", "XT+0", 4, 2, "YT+0", 4, 2, 10, "rowptr+0", "col+0", "val+0", "TT+0", 4, "MT+0", 4,
         1, 2, 0.5, 0.25, 1, 0, "stream")]


def _acc_dgd_csr_pm_nseg16_no_momentum(dev):
    # MT is ignored (NULL, ld 0) when momentum == 0; col / val lengths may differ here too
    t = dict(_pm(dev), TT=mat(dev, 10, 2, 4), MT=mat(dev, 10, 2, 4), val=vec(dev, 5))
    return t, lambda: ops.dgd_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], t["TT"], t["MT"], nseg=16), [
        ("dol_dgd_csr_pm_ex_f32", "XT+0", 4, 2, "YT+0", 4, 2, 10, "rowptr+0", "col+0", "val+0", "TT+0", 4, None, 0,
         0, 1, 0.01, 0.0, 0, 16, "stream")]


def _acc_dgd_csr_pm_empty(dev):
    t = dict(XT=mat(dev, 8, 2, 4), YT=mat(dev, 8, 2, 4), rowptr=vec(dev, 3, I32), col=vec(dev, 0, I32),
             val=vec(dev, 0), TT=mat(dev, 8, 2, 4))
    return t, lambda: ops.dgd_csr_pm(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], t["TT"]), [
        ("dol_dgd_csr_pm_ex_f32", "XT+0", 4, 2, "YT+0", 4, 2, 8, "rowptr+0", None, None, "TT+0", 4, None, 0,
         0, 1, 0.01, 0.0, 0, 0, "stream")]


def _acc_csr_slab_pack_alloc(dev):
    t = CALLS["csr_slab_pack"][0](dev)
    return t, lambda: CALLS["csr_slab_pack"][1](t), [
        ("dol_csr_slab_pack", "rowptr+0", "col+0", "val+0", 2, 2, 0, "alloc", "alloc", "stream")]


def _acc_csr_slab_pack_given_empty(dev):
    t = dict(rowptr=vec(dev, 3, I32), col=vec(dev, 0, I32), val=vec(dev, 0), ent=vec(dev, 4096, I32),
             hdr=vec(dev, 4096, I32))
    return t, lambda: ops.csr_slab_pack(t["rowptr"], t["col"], t["val"], 3, t["ent"], t["hdr"], balance=True), [
        ("dol_csr_slab_pack", "rowptr+0", None, None, 2, 3, 1, "ent+0", "hdr+0", "stream")]


def _acc_mix_csr_slab(dev):
    t = _slab(dev)
    return t, lambda: ops.mix_csr_slab(t["X"], t["Y"], t["ent"], t["hdr"], 2), [
        ("dol_mix_csr_slab_f32", "X+0", 12, 2, "Y+0", 12, 2, 10, "ent+0", "hdr+0", "stream")]


def _acc_mix_csr_slab_x_rows(dev):
    hdr_len = int(ops._native.lib().dol_csr_slab_hdr_len(1, 2))
    t = dict(X=mat(dev, 3, 8), Y=mat(dev, 1, 8), ent=vec(dev, 8, I32), hdr=vec(dev, hdr_len, I32))
    return t, lambda: ops.mix_csr_slab(t["X"], t["Y"], t["ent"], t["hdr"], 1, x_rows=2, P=8), [
        ("dol_mix_csr_slab_f32", "X+0", 8, 2, "Y+0", 8, 1, 8, "ent+0", "hdr+0", "stream")]


def _acc_dense_to_csr_alloc(dev):
    t = CALLS["dense_to_csr"][0](dev)
    return t, lambda: CALLS["dense_to_csr"][1](t), [
        ("dol_dense_to_csr_f32", "W+0", 4, 2, 3, "alloc", "alloc", "alloc", 6, "stream")]


def _acc_dense_to_csr_given(dev):
    t = dict(W=mat(dev, 2, 3), rowptr=vec(dev, 3, I32), col=vec(dev, 7, I32), val=vec(dev, 6))
    return t, lambda: ops.dense_to_csr(t["W"], t["rowptr"], t["col"], t["val"]), [
        ("dol_dense_to_csr_f32", "W+0", 3, 2, 3, "rowptr+0", "col+0", "val+0", 6, "stream")]


def _acc_transpose(dev):
    t = dict(A=mat(dev, 2, 10, 12), B=mat(dev, 10, 2, 4))
    return t, lambda: ops.transpose(t["A"], t["B"]), [
        ("dol_transpose_f32", "A+0", 12, "B+0", 4, 2, 10, "stream")]


def _acc_transpose_part(dev):
    t = dict(A=mat(dev, 2, 10, 12), B=mat(dev, 10, 2, 4))
    return t, lambda: ops.transpose(t["A"], t["B"], rows=1, cols=8), [
        ("dol_transpose_f32", "A+0", 12, "B+0", 4, 1, 8, "stream")]


def _acc_mix_ring_steps_auto(dev):
    t = dict(X=mat(dev, 4, 8, 12), Y=mat(dev, 5, 8), w_prev=vec(dev, 4), w_next=vec(dev, 4))
    return t, lambda: ops.mix_ring_steps(t["X"], t["Y"], t["w_prev"], t["w_next"], 2), [
        ("dol_mix_ring_steps_ex_f32", "X+0", 12, "Y+0", 8, 4, 8, 2, "w_prev+0", "w_next+0", 0, "stream")]


def _acc_mix_ring_steps_variant3(dev):
    t = CALLS["mix_ring_steps"][0](dev)
    return t, lambda: CALLS["mix_ring_steps"][1](t), [
        ("dol_mix_ring_steps_ex_f32", "X+0", 8, "Y+0", 8, 4, 8, 2, "w_prev+0", "w_next+0", 3, "stream")]


def _acc_mix_ring_steps_one_step(dev):
    t = dict(X=mat(dev, 5, 8), Y=mat(dev, 5, 8), w_prev=vec(dev, 5), w_next=vec(dev, 5))
    return t, lambda: ops.mix_ring_steps(t["X"], t["Y"], t["w_prev"], t["w_next"], 1, n_rows=4), [
        ("dol_mix_ring_steps_ex_f32", "X+0", 8, "Y+0", 8, 4, 8, 1, "w_prev+0", "w_next+0", 0, "stream")]


def _acc_mix_ring_halos(dev):
    t = _ring(dev)
    return t, lambda: ops.mix_ring(t["X"], t["Y"], t["w_prev"], t["w_next"], t["halo_prev"], t["halo_next"]), [
        ("dol_mix_ring_f32", "X+0", 12, "Y+0", 12, 4, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "stream")]


def _acc_mix_ring_wrap(dev):
    t = dict(X=mat(dev, 4, 8), Y=mat(dev, 4, 8), w_prev=vec(dev, 4), w_next=vec(dev, 4))
    return t, lambda: ops.mix_ring(t["X"], t["Y"], t["w_prev"], t["w_next"]), [
        ("dol_mix_ring_f32", "X+0", 8, "Y+0", 8, 4, 8, None, None, "w_prev+0", "w_next+0", "stream")]


def _acc_mix_ring_one_row_halos(dev):
    t = dict(X=mat(dev, 1, 10), Y=mat(dev, 1, 10), w_prev=vec(dev, 1), w_next=vec(dev, 1), halo_prev=vec(dev, 10),
             halo_next=vec(dev, 10))
    return t, lambda: ops.mix_ring(t["X"], t["Y"], t["w_prev"], t["w_next"], t["halo_prev"], t["halo_next"]), [
        ("dol_mix_ring_f32", "X+0", 10, "Y+0", 10, 1, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "stream")]


def _acc_mix_ring_edges(dev):
    t = _ring(dev)
    return t, lambda: ops.mix_ring_edges(t["X"], t["Y"], t["w_prev"], t["w_next"], t["halo_prev"], t["halo_next"],
                                         n_rows=3), [
        ("dol_mix_ring_edges_f32", "X+0", 12, "Y+0", 12, 3, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "stream")]


def _acc_dgd_ring_full(dev):
    t = CALLS["dgd_ring"][0](dev)
    return t, lambda: CALLS["dgd_ring"][1](t), [
        ("dol_dgd_ring_f32", "X+0", 12, "Y+0", 12, 4, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "target+0", 12, "mom+0", 12, 1, 2, 0.5, 0.25, 1, "stream")]


def _acc_dgd_ring_plain(dev):
    # mom is ignored (NULL, ld 0) when momentum == 0
    t = dict(X=mat(dev, 4, 8), Y=mat(dev, 4, 8), w_prev=vec(dev, 4), w_next=vec(dev, 4), target=mat(dev, 4, 8),
             mom=mat(dev, 4, 8))
    return t, lambda: ops.dgd_ring(t["X"], t["Y"], t["w_prev"], t["w_next"], t["target"], t["mom"]), [
        ("dol_dgd_ring_f32", "X+0", 8, "Y+0", 8, 4, 8, None, None, "w_prev+0", "w_next+0", "target+0", 8, None, 0,
         0, 1, 0.01, 0.0, 0, "stream")]


def _acc_dgd_ring_edges_full(dev):
    t = CALLS["dgd_ring_edges"][0](dev)
    return t, lambda: CALLS["dgd_ring_edges"][1](t), [
        ("dol_dgd_ring_edges_f32", "X+0", 12, "Y+0", 12, 4, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "target+0", 12, "mom+0", 12, 1, 2, 0.5, 0.25, 1, "stream")]


def _acc_dgd_ring_edges_plain(dev):
    t = dict(_ring(dev), target=mat(dev, 4, 10))
    return t, lambda: ops.dgd_ring_edges(t["X"], t["Y"], t["w_prev"], t["w_next"], t["target"], t["halo_prev"],
                                         t["halo_next"]), [
        ("dol_dgd_ring_edges_f32", "X+0", 12, "Y+0", 12, 4, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "target+0", 10, None, 0, 0, 1, 0.01, 0.0, 0, "stream")]


def _acc_dgd_csr_full(dev):
    t = CALLS["dgd_csr"][0](dev)
    return t, lambda: CALLS["dgd_csr"][1](t), [
        ("dol_dgd_csr_f32", "X+0", 12, 2, "Y+0", 12, 2, 10, "rowptr+0", "col+0", "val+0", "target+0", 12, "mom+0", 12,
         1, 2, 0.5, 0.25, 1, "stream")]


def _acc_dgd_csr_plain_empty(dev):
    # col / val lengths may differ in dgd_csr (mix_csr refuses that)
    t = dict(X=mat(dev, 3, 8), Y=mat(dev, 2, 8), rowptr=vec(dev, 3, I32), col=vec(dev, 0, I32), val=vec(dev, 1),
             target=mat(dev, 2, 8))
    return t, lambda: ops.dgd_csr(t["X"], t["Y"], t["rowptr"], t["col"], t["val"], t["target"]), [
        ("dol_dgd_csr_f32", "X+0", 8, 3, "Y+0", 8, 2, 8, "rowptr+0", None, "val+0", "target+0", 8, None, 0,
         0, 1, 0.01, 0.0, 0, "stream")]


def _acc_mix_dense(dev):
    t = CALLS["mix_dense"][0](dev)
    return t, lambda: ops.mix_dense(t["W"], t["X"], t["Y"]), [
        ("dol_mix_dense_f32", "W+0", 2, "X+0", 12, "Y+0", 12, 2, 2, 10, "stream")]


def _acc_split3_auto_padded(dev):
    # split3_x_flags accepts X (ld 12 >= round_up(10, 4)): fused, FUSE_X | X_ROWS_PADDED
    t = CALLS["mix_dense_split3"][0](dev)
    assert ops.split3_x_flags(t["X"], 10) == 2
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"]), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 12, "Y+0", 12, 2, 2, 10, "alloc", max(_split3_need(6), 1), 6,
         "stream")]


def _acc_split3_auto_unpadded(dev):
    # split3_x_flags rejects X (ld 10 is no multiple of 4): the split pass
    t = dict(W=mat(dev, 2, 2), X=mat(dev, 2, 10), Y=mat(dev, 2, 10))
    assert ops.split3_x_flags(t["X"], 10) == 0
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"]), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 10, "Y+0", 10, 2, 2, 10, "alloc", max(_split3_need(0), 1), 0,
         "stream")]


def _acc_split3_fuse_true_unpadded(dev):
    # fuse=True with P % 4 == 0 fuses without X_ROWS_PADDED when the rows are not padded (ld 10)
    t = dict(W=mat(dev, 2, 2), X=mat(dev, 2, 8, 10), Y=mat(dev, 2, 8))
    assert ops.split3_x_flags(t["X"], 8) == 0
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"], fuse=True), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 10, "Y+0", 8, 2, 2, 8, "alloc",
         max(_split3_need(4, P=8), 1), 4, "stream")]


def _acc_split3_fuse_true_odd_p(dev):
    # fuse=True cannot fuse P % 4 != 0 on rows that are not padded
    t = dict(W=mat(dev, 2, 2), X=mat(dev, 2, 10), Y=mat(dev, 2, 10))
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"], fuse=True), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 10, "Y+0", 10, 2, 2, 10, "alloc", max(_split3_need(0), 1), 0,
         "stream")]


def _acc_split3_fuse_false_work(dev):
    t = dict(CALLS["mix_dense_split3"][0](dev), work=vec(dev, _split3_need(0) + 16, U8))
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"], work=t["work"], fuse=False), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 12, "Y+0", 12, 2, 2, 10, "work+0", _split3_need(0) + 16, 0,
         "stream")]


def _acc_split3_w_ready(dev):
    t = dict(CALLS["mix_dense_split3"][0](dev), work=vec(dev, _split3_need(7), U8))
    return t, lambda: ops.mix_dense_split3(t["W"], t["X"], t["Y"], work=t["work"], w_ready=True), [
        ("dol_mix_dense_split3_f32", "W+0", 2, "X+0", 12, "Y+0", 12, 2, 2, 10, "work+0", _split3_need(7), 7,
         "stream")]


def _acc_er_stochastic(dev):
    t = CALLS["er_stochastic"][0](dev)
    return t, lambda: CALLS["er_stochastic"][1](t), [("dol_er_stochastic_f32", "W+0", 4, 3, 0.5, 7, "stream")]


def _acc_prox_admm_sgd_full(dev):
    t = CALLS["prox_admm_sgd"][0](dev)
    return t, lambda: CALLS["prox_admm_sgd"][1](t), [
        ("dol_prox_admm_sgd_f32", "w+0", 12, "buf+0", 12, "g+0", 12, "theta+0", "alpha+0", 12, 0.5, 0.25, 0.125, 1, 0,
         2, 10, "stream")]


def _acc_prox_admm_sgd_plain(dev):
    # buf is ignored (NULL, ld 0) when momentum == 0
    t = dict(w=mat(dev, 1, 8), g=mat(dev, 2, 8), buf=mat(dev, 1, 8))
    return t, lambda: ops.prox_admm_sgd(t["w"], t["g"], t["buf"]), [
        ("dol_prox_admm_sgd_f32", "w+0", 8, None, 0, "g+0", 8, None, None, 0, 0.0, 0.01, 0.0, 0, 1, 1, 8, "stream")]


def _acc_prox_admm_sgd_prox(dev):
    t = dict(w=mat(dev, 2, 10, 12), g=mat(dev, 2, 10), theta=vec(dev, 12))
    return t, lambda: ops.prox_admm_sgd(t["w"], t["g"], theta=t["theta"], rho=0.5), [
        ("dol_prox_admm_sgd_f32", "w+0", 12, None, 0, "g+0", 10, "theta+0", None, 0, 0.5, 0.01, 0.0, 0, 1, 2, 10,
         "stream")]


def _acc_admm_step_dual_full(dev):
    t = CALLS["admm_step_dual"][0](dev)
    return t, lambda: CALLS["admm_step_dual"][1](t), [
        ("dol_admm_step_dual_f32", "w+0", 12, "buf+0", 12, "g+0", 12, "theta+0", "alpha+0", 12, 0.5, 0.25, 0.125, 1, 0,
         2, 10, "stream")]


def _acc_admm_step_dual_plain(dev):
    t = dict(w=mat(dev, 2, 8), g=mat(dev, 2, 8), theta=vec(dev, 8), alpha=mat(dev, 2, 8))
    return t, lambda: ops.admm_step_dual(t["w"], t["g"], t["theta"], t["alpha"]), [
        ("dol_admm_step_dual_f32", "w+0", 8, None, 0, "g+0", 8, "theta+0", "alpha+0", 8, 0.0, 0.01, 0.0, 0, 1, 2, 8,
         "stream")]


def _acc_prox_grad_alpha(dev):
    t = CALLS["prox_grad"][0](dev)
    return t, lambda: CALLS["prox_grad"][1](t), [
        ("dol_prox_grad_f32", "g+0", 12, "w+0", 12, "theta+0", "alpha+0", 12, 0.5, 2, 10, "stream")]


def _acc_prox_grad_plain(dev):
    t = dict(g=mat(dev, 2, 8), w=mat(dev, 2, 8), theta=vec(dev, 8))
    return t, lambda: ops.prox_grad(t["g"], t["w"], t["theta"], 0.5), [
        ("dol_prox_grad_f32", "g+0", 8, "w+0", 8, "theta+0", None, 0, 0.5, 2, 8, "stream")]


def _acc_admm_dual_plain(dev):
    # work is ignored without resid_sq
    t = dict(alpha=mat(dev, 2, 10, 12), w=mat(dev, 2, 10), theta=vec(dev, 10), work=vec(dev, 8, U8))
    return t, lambda: ops.admm_dual(t["alpha"], t["w"], t["theta"], 0.5, work=t["work"]), [
        ("dol_admm_dual_f32", "alpha+0", 12, "w+0", 10, "theta+0", 0.5, 2, 10, None, None, "stream")]


def _acc_admm_dual_resid_alloc(dev):
    t = CALLS["admm_dual"][0](dev)
    return t, lambda: CALLS["admm_dual"][1](t), [
        ("dol_admm_dual_f32", "alpha+0", 12, "w+0", 12, "theta+0", 0.5, 2, 10, "resid_sq+0", "alloc", "stream")]


def _acc_admm_dual_resid_work(dev):
    t = dict(CALLS["admm_dual"][0](dev), work=vec(dev, ops.dual_workspace_bytes(2, 10) + 8, U8))
    return t, lambda: CALLS["admm_dual"][1](t), [
        ("dol_admm_dual_f32", "alpha+0", 12, "w+0", 12, "theta+0", 0.5, 2, 10, "resid_sq+0", "work+0", "stream")]


def _acc_admm_ls_round_full(dev):
    t = dict(CALLS["admm_ls_round"][0](dev))
    t["work"] = vec(dev, ops.admm_ls_round_workspace_bytes(2, 10) + 8, U8)
    return t, lambda: CALLS["admm_ls_round"][1](t), [
        ("dol_admm_ls_round_f32", "w+0", 12, "buf+0", 12, "alpha+0", 12, "target+0", 12, "theta+0", "agents+0",
         "first+0", 2, 10, 0.5, 0.25, 0.125, 3, "resid_sq+0", "alpha_sq+0", "work+0", "stream")]


def _acc_admm_ls_round_alloc_work(dev):
    t = CALLS["admm_ls_round"][0](dev)
    return t, lambda: CALLS["admm_ls_round"][1](t), [
        ("dol_admm_ls_round_f32", "w+0", 12, "buf+0", 12, "alpha+0", 12, "target+0", 12, "theta+0", "agents+0",
         "first+0", 2, 10, 0.5, 0.25, 0.125, 3, "resid_sq+0", "alpha_sq+0", "alloc", "stream")]


def _acc_admm_ls_round_plain(dev):
    # buf and work are ignored (NULL) without momentum / without the norms
    t = dict(w=mat(dev, 2, 8), alpha=mat(dev, 2, 8), target=mat(dev, 3, 8), theta=vec(dev, 8), buf=mat(dev, 2, 8),
             work=vec(dev, 8, U8))
    return t, lambda: ops.admm_ls_round(t["w"], t["alpha"], t["target"], t["theta"], buf=t["buf"], work=t["work"]), [
        ("dol_admm_ls_round_f32", "w+0", 8, None, 0, "alpha+0", 8, "target+0", 8, "theta+0", None, None, 2, 8,
         0.1, 0.1, 0.0, 1, None, None, None, "stream")]


def _acc_admm_ls_round_subset(dev):
    t = dict(w=mat(dev, 2, 8), alpha=mat(dev, 2, 8), target=mat(dev, 2, 8), theta=vec(dev, 8), agents=ids(dev, 1))
    return t, lambda: ops.admm_ls_round(t["w"], t["alpha"], t["target"], t["theta"], agents=t["agents"],
                                        local_steps=0), [
        ("dol_admm_ls_round_f32", "w+0", 8, None, 0, "alpha+0", 8, "target+0", 8, "theta+0", "agents+0", None, 1, 8,
         0.1, 0.1, 0.0, 0, None, None, None, "stream")]


def _acc_admm_ls_round_mean_full(dev):
    t = dict(CALLS["admm_ls_round_mean"][0](dev))
    t["work"] = vec(dev, int(ops._native.lib().dol_admm_ls_round_mean_workspace_bytes(10)) + 8, U8)
    return t, lambda: CALLS["admm_ls_round_mean"][1](t), [
        ("dol_admm_ls_round_mean_f32", "w+0", 12, "buf+0", 12, "alpha+0", 12, "target+0", 12, "theta+0", "agents+0",
         "first+0", 2, 10, 0.5, 0.25, 0.125, 3, "out+0", 2.0, "resid_total+0", "work+0", "stream")]


def _acc_admm_ls_round_mean_alloc(dev):
    t = dict(CALLS["admm_ls_round_mean"][0](dev), out=None, scale=1.0, validate=False)
    return t, lambda: CALLS["admm_ls_round_mean"][1](t), [
        ("dol_admm_ls_round_mean_f32", "w+0", 12, "buf+0", 12, "alpha+0", 12, "target+0", 12, "theta+0", "agents+0",
         "first+0", 2, 10, 0.5, 0.25, 0.125, 3, "alloc", 1.0, "resid_total+0", "alloc", "stream")]


def _acc_admm_ls_round_mean_plain(dev):
    t = dict(w=mat(dev, 2, 8), alpha=mat(dev, 2, 8), target=mat(dev, 2, 8), theta=vec(dev, 8), out=vec(dev, 8),
             work=vec(dev, 8, U8))
    return t, lambda: ops.admm_ls_round_mean(t["w"], t["alpha"], t["target"], t["theta"], out=t["out"],
                                             work=t["work"]), [
        ("dol_admm_ls_round_mean_f32", "w+0", 8, None, 0, "alpha+0", 8, "target+0", 8, "theta+0", None, None, 2, 8,
         0.1, 0.1, 0.0, 1, "out+0", 2.0, None, None, "stream")]


def _acc_admm_ls_round_mean_unvalidated(dev):
    # validate=False: repeated ids are the caller's business (no host copy of the ids)
    t = dict(w=mat(dev, 2, 8), alpha=mat(dev, 2, 8), target=mat(dev, 2, 8), theta=vec(dev, 8), out=vec(dev, 8),
             agents=ids(dev, 1, 1))
    return t, lambda: ops.admm_ls_round_mean(t["w"], t["alpha"], t["target"], t["theta"], agents=t["agents"],
                                             out=t["out"], validate=False), [
        ("dol_admm_ls_round_mean_f32", "w+0", 8, None, 0, "alpha+0", 8, "target+0", 8, "theta+0", "agents+0", None,
         2, 8, 0.1, 0.1, 0.0, 1, "out+0", 2.0, None, None, "stream")]


def _acc_ordered_mean(dev):
    t = CALLS["ordered_mean"][0](dev)
    return t, lambda: CALLS["ordered_mean"][1](t), [
        ("dol_ordered_mean_f32", "W+0", 12, "order+0", 3, 10, "out+0", "stream")]


def _acc_ordered_mean_alloc(dev):
    t = dict(W=mat(dev, 1, 8), order=ids(dev, 0))
    return t, lambda: ops.ordered_mean(t["W"], t["order"]), [
        ("dol_ordered_mean_f32", "W+0", 8, "order+0", 1, 8, "alloc", "stream")]


def _acc_ordered_sum_full(dev):
    t = CALLS["ordered_sum"][0](dev)
    return t, lambda: CALLS["ordered_sum"][1](t), [
        ("dol_ordered_sum_f32", "W+0", 12, "order+0", 3, 10, "acc_in+0", "out+0", 0.5, "stream")]


def _acc_ordered_sum_plain(dev):
    t = dict(W=mat(dev, 2, 8), order=ids(dev, 1))
    return t, lambda: ops.ordered_sum(t["W"], t["order"]), [
        ("dol_ordered_sum_f32", "W+0", 8, "order+0", 1, 8, None, "alloc", 1.0, "stream")]


def _acc_ordered_sum_no_rows(dev):
    t = dict(acc_in=vec(dev, 8), out=vec(dev, 8))
    return t, lambda: ops.ordered_sum(None, None, t["acc_in"], t["out"], scale=0.25), [
        ("dol_ordered_sum_f32", None, 8, None, 0, 8, "acc_in+0", "out+0", 0.25, "stream")]


def _acc_ordered_sum_empty_order(dev):
    t = dict(W=mat(dev, 2, 10, 12), order=vec(dev, 0, I32), acc_in=vec(dev, 10))
    return t, lambda: ops.ordered_sum(t["W"], t["order"], t["acc_in"]), [
        ("dol_ordered_sum_f32", None, 12, None, 0, 10, "acc_in+0", "alloc", 1.0, "stream")]


def _acc_stream_copy(dev):
    t = CALLS["stream_copy"][0](dev)
    return t, lambda: CALLS["stream_copy"][1](t), [("dol_stream_copy_f32", "src+0", "dst+0", 6, "stream")]


def _acc_stream_copy_rows(dev):
    t = dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 3, 10))
    return t, lambda: ops.stream_copy_rows(t["X"], t["Y"]), [
        ("dol_stream_copy_rows_f32", "X+0", 12, "Y+0", 10, 2, 10, "stream")]


def _acc_stream_copy_rows_p(dev):
    t = dict(X=mat(dev, 2, 10, 12), Y=mat(dev, 2, 8))
    return t, lambda: ops.stream_copy_rows(t["X"], t["Y"], P=8), [
        ("dol_stream_copy_rows_f32", "X+0", 12, "Y+0", 8, 2, 8, "stream")]


def _acc_mlp_step_full(dev):
    t = dict(_mlp(dev))
    t["work"] = vec(dev, int(ops._native.lib().dol_mlp_step_workspace_bytes(2, 2, 4)) + 8, U8)
    return t, lambda: CALLS["mlp_step"][1](t), [
        ("dol_mlp_step_f32", "w+0", 32, "grad+0", 32, "mom+0", 32, "theta+0", "alpha+0", 32, "X+0", 8, 4, "y+0", 2,
         "loss+0", 2, 2, 4, 4, 2, 0.5, 0.25, 0.125, 1, 1, "work+0", "stream")]


def _acc_mlp_step_plain(dev):
    # mom is ignored (NULL, ld 0) when momentum == 0
    t = dict(w=mat(dev, 2, 30), X=torch.zeros(2, 2, 4, device=dev), y=torch.zeros(2, 2, dtype=I64, device=dev),
             mom=mat(dev, 2, 30))
    return t, lambda: ops.mlp_step(t["w"], t["X"], t["y"], 4, 4, 2, mom=t["mom"]), [
        ("dol_mlp_step_f32", "w+0", 30, None, 0, None, 0, None, None, 0, "X+0", 8, 4, "y+0", 2, None, 2, 2, 4, 4, 2,
         0.01, 0.0, 0.0, 0, 1, "alloc", "stream")]


def _acc_mlp_step_grad_only(dev):
    # update=False: no momentum buffer is needed or passed whatever momentum says
    t = dict(w=mat(dev, 2, 30, 32), X=torch.zeros(2, 2, 4, device=dev), y=torch.zeros(2, 2, dtype=I64, device=dev),
             grad=mat(dev, 2, 30), theta=vec(dev, 30))
    return t, lambda: ops.mlp_step(t["w"], t["X"], t["y"], 4, 4, 2, grad=t["grad"], theta=t["theta"], momentum=0.5,
                                   rho=0.25, update=False), [
        ("dol_mlp_step_f32", "w+0", 32, "grad+0", 30, None, 0, "theta+0", None, 0, "X+0", 8, 4, "y+0", 2, None, 2, 2,
         4, 4, 2, 0.01, 0.5, 0.25, 0, 0, "alloc", "stream")]


def _acc_mlp_step_one_agent_one_sample(dev):
    # the shape[0] == 1 branches of every ld: [1, 1, d] views of wider buffers
    t = dict(w=mat(dev, 1, 30, 32), X=torch.zeros(3, 5, 4, device=dev)[:1, :1],
             y=torch.zeros(3, 5, dtype=I64, device=dev)[:1, :1])
    return t, lambda: ops.mlp_step(t["w"], t["X"], t["y"], 4, 4, 2), [
        ("dol_mlp_step_f32", "w+0", 30, None, 0, None, 0, None, None, 0, "X+0", 4, 4, "y+0", 1, None, 1, 1, 4, 4, 2,
         0.01, 0.0, 0.0, 0, 1, "alloc", "stream")]


ACCEPT = [v for k, v in sorted(globals().items()) if k.startswith("_acc_")]


@pytest.mark.parametrize("case", ACCEPT, ids=lambda f: f.__name__[5:])
def test_accept(case, gpu, rec):
    tensors, call, want = case(gpu)
    call()
    assert named(rec.calls, tensors, gpu) == want


# ---------------------------------------------------------------------------
# REJECT
# ---------------------------------------------------------------------------
def _on_cpu(k):
    def f(t):
        t[k] = t[k].cpu()
    return f


def _as(k, dtype):
    def f(t):
        t[k] = t[k].to(dtype)
    return f


def _set(**kw):
    def f(t):
        t.update({k: (v(t) if callable(v) else v) for k, v in kw.items()})
    return f


def _strided(k):
    def f(t):
        a = t[k]
        t[k] = torch.zeros(a.shape[0], 2 * a.shape[1], dtype=a.dtype, device=a.device)[:, ::2]
    return f


def _generic_row_cases():
    cases = []
    for op, rows in ROWS.items():
        for k, P in rows.items():
            cases += [
                (op, f"{k}_cpu", _on_cpu(k), DolNativeError, f"{k}: tensor is on cpu; the HIP engine has no CPU path"),
                (op, f"{k}_dtype", _as(k, F64), TypeError, f"{k}: expected float32, got torch.float64"),
                (op, f"{k}_rank", _set(**{k: lambda t, k=k: t[k][0]}), ValueError,
                 lambda t, k=k: f"{k}: expected a 2-D [rows, P] tensor, got shape {tuple(t[k].shape)}"),
                (op, f"{k}_stride", _strided(k), ValueError, f"{k}: rows must be contiguous (stride(1) == 1)"),
            ]
            if P is not None:
                cases.append((op, f"{k}_columns", _set(**{k: lambda t, k=k, P=P: t[k][:, :P - 1]}), ValueError,
                              f"{k}: has {P - 1} columns < P={P}"))
    return cases


def _vec_cases(op, k, P, name=None):
    """The rules of a float32 vector argument (theta, halos, out, acc_in)."""
    name = name or k
    bad = f"{name}: expected a contiguous float32 vector of >= {P} elements"
    return [
        (op, f"{k}_cpu", _on_cpu(k), DolNativeError, lambda t: f"{name}: on cpu, expected {_dev(t)}"),
        (op, f"{k}_dtype", _as(k, F64), ValueError, bad),
        (op, f"{k}_short", _set(**{k: lambda t: t[k][:P - 1]}), ValueError, bad),
        (op, f"{k}_rank", _set(**{k: lambda t: t[k].reshape(1, -1)}), ValueError, bad),
        (op, f"{k}_stride", _set(**{k: lambda t: vec(_dev(t), 2 * P)[::2]}), ValueError, bad),
    ]


def _dev(t):
    return next((v.device for v in t.values() if isinstance(v, torch.Tensor) and v.device.type != "cpu"), "cpu")


def _csr_cases(op, lengths):
    def msg(nm, dt):
        return lambda t: f"{nm}: expected contiguous {dt} on {_dev(t)}"
    cases = [
        (op, "rowptr_dtype", _as("rowptr", I64), ValueError, msg("rowptr", I32)),
        (op, "col_dtype", _as("col", I64), ValueError, msg("col", I32)),
        (op, "val_dtype", _as("val", F64), ValueError, msg("val", F32)),
        (op, "col_cpu", _on_cpu("col"), ValueError, msg("col", I32)),
        (op, "val_cpu", _on_cpu("val"), ValueError, msg("val", F32)),
        (op, "col_stride", _set(col=lambda t: vec(_dev(t), 8, I32)[::2]), ValueError, msg("col", I32)),
    ]
    if op != "csr_slab_pack":  # there rowptr's device is the reference; see its own cases
        cases.append((op, "rowptr_cpu", _on_cpu("rowptr"), ValueError, msg("rowptr", I32)))
    if lengths:
        cases.append((op, "col_val_lengths", _set(val=lambda t: t["val"][:3]), ValueError, "col and val lengths differ"))
    return cases


def _ring_weight_cases(op, n=4):
    def msg(nm):
        return lambda t: f"{nm}: expected contiguous float32 [{n}] on {_dev(t)}"
    return [
        (op, "w_prev_short", _set(w_prev=lambda t: t["w_prev"][:n - 1]), ValueError, msg("w_prev")),
        (op, "w_next_short", _set(w_next=lambda t: t["w_next"][:n - 1]), ValueError, msg("w_next")),
        (op, "w_prev_dtype", _as("w_prev", F64), ValueError, msg("w_prev")),
        (op, "w_next_cpu", _on_cpu("w_next"), ValueError, msg("w_next")),
        (op, "w_prev_stride", _set(w_prev=lambda t: vec(_dev(t), 2 * n)[::2]), ValueError, msg("w_prev")),
    ]


def _xy_rows_cases(op):
    short = "X/Y have fewer rows than n_rows"
    return [(op, "X_rows", _set(n_rows=5, w_prev=lambda t: vec(_dev(t), 5), w_next=lambda t: vec(_dev(t), 5),
                                Y=lambda t: mat(_dev(t), 5, t["P"])), ValueError, short),
            (op, "Y_rows", _set(Y=lambda t: t["Y"][:3]), ValueError, short)]


JACOBI = "X and Y alias: the Jacobi mix needs two buffers"


def _dgd_cases(op, n, pm=False):
    tk, mk = ("TT", "MT") if pm else ("target", "mom")
    if pm:
        def short(k):
            return lambda t: f"{k}: expected [>= 10, >= {n}] on {_dev(t)}"
    else:
        def short(k):
            return lambda t: f"{k}: expected >= {n} rows on {_dev(t)}"
    cases = [
        (op, "objective", _set(objective="hinge"), ValueError, "objective must be one of ['least_squares', 'logistic']"),
        (op, "steps", _set(steps=0), ValueError, "local steps must be >= 1"),
        (op, f"{mk}_missing", _set(**{mk: None}), ValueError, f"momentum != 0 needs {mk}"),
    ]
    if pm:
        cases += [(op, f"{k}_rows", _set(**{k: lambda t, k=k: t[k][:9]}), ValueError, short(k)) for k in (tk, mk)]
        cases += [(op, f"{k}_agents", _set(**{k: lambda t, k=k: t[k][:, :1]}), ValueError, short(k)) for k in (tk, mk)]
    else:
        cases += [(op, f"{k}_rows", _set(**{k: lambda t, k=k: t[k][:n - 1]}), ValueError, short(k)) for k in (tk, mk)]
    return cases


def _momentum_cases(op, k="buf", short="buf has fewer rows than w"):
    return [(op, f"{k}_missing", _set(**{k: None}), ValueError, f"momentum != 0 needs {k}"),
            (op, f"{k}_rows", _set(**{k: lambda t: t[k][:1]}), ValueError, short)]


def _pm_cases(op):
    return [
        (op, "XT_rows", _set(XT=lambda t: t["XT"][:9]), ValueError, "XT/YT need >= 10 parameter rows"),
        (op, "YT_rows", _set(YT=lambda t: t["YT"][:9]), ValueError, "XT/YT need >= 10 parameter rows"),
        (op, "XT_agents", _set(x_agents=3), ValueError, "XT needs >= 3 agent columns, YT >= 2"),
        (op, "YT_agents", _set(YT=lambda t: t["YT"][:, :1]), ValueError, "XT needs >= 2 agent columns, YT >= 2"),
        (op, "alias", _set(YT=lambda t: t["XT"]), ValueError, "XT and YT alias: the Jacobi mix needs two buffers"),
    ]


def _ls_round_cases(op):
    def first(t):
        return f"first: expected contiguous int32 [2] on {_dev(t)}"
    order = "order: expected contiguous int32 on the rows' device"
    return [
        (op, "alpha_rows", _set(alpha=lambda t: t["alpha"][:1]), ValueError, "alpha/target have fewer rows than w"),
        (op, "target_rows", _set(target=lambda t: t["target"][:1]), ValueError, "alpha/target have fewer rows than w"),
        (op, "local_steps", _set(local_steps=-1), ValueError, "local_steps must be >= 0"),
        (op, "agents_dtype", _as("agents", I64), ValueError, order),
        (op, "agents_cpu", _on_cpu("agents"), ValueError, order),
        (op, "agents_stride", _set(agents=lambda t: vec(_dev(t), 4, I32)[::2]), ValueError, order),
        (op, "first_dtype", _as("first", I64), ValueError, first),
        (op, "first_short", _set(first=lambda t: t["first"][:1]), ValueError, first),
        (op, "first_cpu", _on_cpu("first"), ValueError, first),
        (op, "work_cpu", _set(work=lambda t: torch.zeros(1 << 16, dtype=U8)), ValueError,
         lambda t: f"work: need {_ls_need(op)} bytes on {_dev(t)}"),
        (op, "work_small", _set(work=lambda t: vec(_dev(t), _ls_need(op) - 1, U8)), ValueError,
         lambda t: f"work: need {_ls_need(op)} bytes on {_dev(t)}"),
    ] + _momentum_cases(op) + _vec_cases(op, "theta", 10)


def _ls_need(op):
    if op == "admm_ls_round":
        return ops.admm_ls_round_workspace_bytes(2, 10)
    return int(ops._native.lib().dol_admm_ls_round_mean_workspace_bytes(10))


def _mlp_x(t):
    return f"X: expected float32 [2, B, 4] on {_dev(t)}"


def _mlp_y(t):
    return f"y: expected int64 [2, 2] on {_dev(t)}"


def _mlp_loss(t):
    return f"loss: expected a contiguous float32 [2] on {_dev(t)}"


def _mlp_need():
    return int(ops._native.lib().dol_mlp_step_workspace_bytes(2, 2, 4))


SLAB_LAYOUT = ("mix_csr_slab: X, Y need 16-B aligned rows with strides % 4 == 0 and X readable to "
               "round_up(P, 4) floats per row")

REJECT = _generic_row_cases() + [
    # --- CSR mixes
    ("mix_csr", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "Y has 1 rows < 2"),
    ("mix_csr", "alias", _set(Y=lambda t: t["X"]), ValueError, JACOBI),
    *_csr_cases("mix_csr", lengths=True),
    *_pm_cases("mix_csr_pm"), *_csr_cases("mix_csr_pm", lengths=False),
    *_pm_cases("dgd_csr_pm"), *_csr_cases("dgd_csr_pm", lengths=False), *_dgd_cases("dgd_csr_pm", 2, pm=True),
    ("dgd_csr", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "Y has 1 rows < 2"),
    ("dgd_csr", "alias", _set(Y=lambda t: t["X"]), ValueError, JACOBI),
    *_csr_cases("dgd_csr", lengths=False), *_dgd_cases("dgd_csr", 2),
    # --- the slab pair
    *_csr_cases("csr_slab_pack", lengths=True),
    ("csr_slab_pack", "all_cpu", _set(rowptr=lambda t: t["rowptr"].cpu(), col=lambda t: t["col"].cpu(),
                                      val=lambda t: t["val"].cpu()), DolNativeError,
     "rowptr: tensor is on cpu; the HIP engine has no CPU path"),
    ("csr_slab_pack", "rowptr_cpu", _on_cpu("rowptr"), DolNativeError,
     "rowptr: tensor is on cpu; the HIP engine has no CPU path"),
    ("mix_csr_slab", "X_rows", _set(x_rows=3), ValueError, "X has 2 rows (need 3), Y 2 (need 2)"),
    ("mix_csr_slab", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "X has 2 rows (need 2), Y 1 (need 2)"),
    ("mix_csr_slab", "layout_ld", _set(X=lambda t: mat(_dev(t), 2, 10)), ValueError, SLAB_LAYOUT),
    ("mix_csr_slab", "layout_ldy", _set(Y=lambda t: mat(_dev(t), 2, 10)), ValueError, SLAB_LAYOUT),
    ("mix_csr_slab", "layout_align", _set(X=lambda t: mat(_dev(t), 2, 13, 16)[:, 1:11]), ValueError, SLAB_LAYOUT),
    ("mix_csr_slab", "layout_last_row", _set(X=lambda t: torch.zeros(22, device=_dev(t)).as_strided((2, 10), (12, 1))),
     ValueError, SLAB_LAYOUT),
    ("mix_csr_slab", "ent_dtype", _as("ent", I64), ValueError, lambda t: f"ent: expected contiguous int32 on {_dev(t)}"),
    ("mix_csr_slab", "hdr_cpu", _on_cpu("hdr"), ValueError, lambda t: f"hdr: expected contiguous int32 on {_dev(t)}"),
    ("mix_csr_slab", "hdr_short", _set(hdr=lambda t: t["hdr"][:-1]), ValueError,
     "hdr too short for these row counts (rebuild with csr_slab_pack)"),
    ("mix_csr_slab", "alias", _set(Y=lambda t: t["X"]), ValueError, JACOBI),
    # --- layout helpers
    ("transpose", "A_rows", _set(A=lambda t: t["A"][:1]), ValueError, "shapes: A (1, 10), B (10, 2), rows 2, cols 10"),
    ("transpose", "B_rows", _set(B=lambda t: t["B"][:9]), ValueError, "shapes: A (2, 10), B (9, 2), rows 2, cols 10"),
    ("stream_copy", "src_cpu", _on_cpu("src"), DolNativeError, "stream_copy: device tensors required"),
    ("stream_copy", "dst_cpu", _on_cpu("dst"), DolNativeError, "stream_copy: device tensors required"),
    ("stream_copy", "sizes", _set(dst=lambda t: vec(_dev(t), 5)), ValueError,
     "stream_copy: contiguous tensors of equal size required"),
    ("stream_copy", "stride", _set(src=lambda t: vec(_dev(t), 12)[::2]), ValueError,
     "stream_copy: contiguous tensors of equal size required"),
    ("stream_copy_rows", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "Y has fewer rows than X"),
    # --- ring
    *_ring_weight_cases("mix_ring_steps"),
    ("mix_ring_steps", "alias", _set(Y=lambda t: t["X"]), ValueError, "X and Y alias"),
    ("mix_ring_steps", "X_rows", _set(n_rows=5, w_prev=lambda t: vec(_dev(t), 5), w_next=lambda t: vec(_dev(t), 5),
                                      Y=lambda t: mat(_dev(t), 5, 8)), ValueError, "X/Y have fewer rows than n_rows"),
    ("mix_ring_steps", "Y_rows", _set(Y=lambda t: t["Y"][:3]), ValueError, "X/Y have fewer rows than n_rows"),
]
for _op in ("mix_ring", "mix_ring_edges", "dgd_ring", "dgd_ring_edges"):
    REJECT += [*_ring_weight_cases(_op), *_xy_rows_cases(_op), (_op, "alias", _set(Y=lambda t: t["X"]), ValueError, JACOBI),
               *_vec_cases(_op, "halo_prev", 10), *_vec_cases(_op, "halo_next", 10)]
for _op, _other in (("mix_ring", "mix_csr"), ("dgd_ring", "dgd_csr")):
    REJECT += [
        (_op, "one_halo", _set(halo_next=None), ValueError, "pass both halos or neither"),
        (_op, "other_halo", _set(halo_prev=None), ValueError, "pass both halos or neither"),
        (_op, "short_ring", _set(halo_prev=None, halo_next=None, n_rows=2), ValueError,
         f"a wrap-around ring needs >= 3 rows (use {_other})"),
    ]
for _op in ("mix_ring_edges", "dgd_ring_edges"):
    REJECT += [(_op, "no_halo_prev", _set(halo_prev=None), ValueError, f"{_op} needs both halos"),
               (_op, "no_halo_next", _set(halo_next=None), ValueError, f"{_op} needs both halos")]
REJECT += [
    *_dgd_cases("dgd_ring", 4), *_dgd_cases("dgd_ring_edges", 4),
    # --- dense
    ("mix_dense", "X_rows", _set(X=lambda t: t["X"][:1]), ValueError, "shapes: W (2, 2), X (1, 10), Y (2, 10)"),
    ("mix_dense", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "shapes: W (2, 2), X (2, 10), Y (1, 10)"),
    ("mix_dense", "alias", _set(Y=lambda t: t["X"]), ValueError, "X and Y alias"),
    ("mix_dense_split3", "X_rows", _set(X=lambda t: t["X"][:1]), ValueError, "shapes: W (2, 2), X (1, 10), Y (2, 10)"),
    ("mix_dense_split3", "Y_rows", _set(Y=lambda t: t["Y"][:1]), ValueError, "shapes: W (2, 2), X (2, 10), Y (1, 10)"),
    ("mix_dense_split3", "alias_X", _set(Y=lambda t: t["X"]), ValueError, "Y aliases an input"),
    ("mix_dense_split3", "alias_W", _set(Y=lambda t: t["W"], X=lambda t: mat(_dev(t), 2, 2), P=2), ValueError,
     "Y aliases an input"),
    ("mix_dense_split3", "w_ready_without_work", _set(w_ready=True), ValueError,
     "w_ready needs the workspace of the call that split W"),
    ("mix_dense_split3", "work_small", _set(work=lambda t: vec(_dev(t), _split3_need(6) - 1, U8)), ValueError,
     lambda t: f"work: need a uint8 tensor of >= {_split3_need(6)} bytes on {_dev(t)}"),
    ("mix_dense_split3", "work_dtype", _set(work=lambda t: vec(_dev(t), 1 << 16, F32)), ValueError,
     lambda t: f"work: need a uint8 tensor of >= {_split3_need(6)} bytes on {_dev(t)}"),
    ("mix_dense_split3", "work_cpu", _set(work=lambda t: torch.zeros(1 << 16, dtype=U8)), ValueError,
     lambda t: f"work: need a uint8 tensor of >= {_split3_need(6)} bytes on {_dev(t)}"),
    ("er_stochastic", "W_narrow", _set(W=lambda t: t["W"][:, :2]), ValueError, "W: expected [n, >= n], got (3, 2)"),
    # --- primal / dual steps
    ("prox_admm_sgd", "g_rows", _set(g=lambda t: t["g"][:1]), ValueError, "g has fewer rows than w"),
    *_momentum_cases("prox_admm_sgd"),
    ("prox_admm_sgd", "alpha_without_theta", _set(theta=None), ValueError, "alpha needs theta"),
    ("prox_admm_sgd", "alpha_rows", _set(alpha=lambda t: t["alpha"][:1]), ValueError, "alpha has fewer rows than w"),
    *_vec_cases("prox_admm_sgd", "theta", 10),
    ("admm_step_dual", "g_rows", _set(g=lambda t: t["g"][:1]), ValueError, "g/alpha have fewer rows than w"),
    ("admm_step_dual", "alpha_rows", _set(alpha=lambda t: t["alpha"][:1]), ValueError, "g/alpha have fewer rows than w"),
    *_momentum_cases("admm_step_dual"), *_vec_cases("admm_step_dual", "theta", 10),
    ("prox_grad", "w_rows", _set(w=lambda t: t["w"][:1]), ValueError, "w has fewer rows than g"),
    ("prox_grad", "alpha_rows", _set(alpha=lambda t: t["alpha"][:1]), ValueError, "alpha has fewer rows than g"),
    *_vec_cases("prox_grad", "theta", 10),
    ("admm_dual", "w_rows", _set(w=lambda t: t["w"][:1]), ValueError, "w has fewer rows than alpha"),
    *_vec_cases("admm_dual", "theta", 10),
    ("admm_dual", "resid_sq_dtype", _as("resid_sq", F32), ValueError,
     "resid_sq: expected float64 [n_agents] on the same device"),
    ("admm_dual", "resid_sq_short", _set(resid_sq=lambda t: t["resid_sq"][:1]), ValueError,
     "resid_sq: expected float64 [n_agents] on the same device"),
    ("admm_dual", "resid_sq_cpu", _on_cpu("resid_sq"), ValueError,
     "resid_sq: expected float64 [n_agents] on the same device"),
    ("admm_dual", "work_small", _set(work=lambda t: vec(_dev(t), ops.dual_workspace_bytes(2, 10) - 1, U8)), ValueError,
     lambda t: f"work: need {ops.dual_workspace_bytes(2, 10)} bytes"),
    *_ls_round_cases("admm_ls_round"),
    ("admm_ls_round", "resid_sq_alone", _set(alpha_sq=None), ValueError, "pass both resid_sq and alpha_sq or neither"),
    ("admm_ls_round", "alpha_sq_alone", _set(resid_sq=None), ValueError, "pass both resid_sq and alpha_sq or neither"),
    ("admm_ls_round", "resid_sq_dtype", _as("resid_sq", F32), ValueError,
     lambda t: f"resid_sq: expected contiguous float64 [2] on {_dev(t)}"),
    ("admm_ls_round", "alpha_sq_short", _set(alpha_sq=lambda t: t["alpha_sq"][:1]), ValueError,
     lambda t: f"alpha_sq: expected contiguous float64 [2] on {_dev(t)}"),
    ("admm_ls_round", "alpha_sq_cpu", _on_cpu("alpha_sq"), ValueError,
     lambda t: f"alpha_sq: expected contiguous float64 [2] on {_dev(t)}"),
    *_ls_round_cases("admm_ls_round_mean"), *_vec_cases("admm_ls_round_mean", "out", 10),
    ("admm_ls_round_mean", "more_agents_than_rows", _set(agents=lambda t: ids(_dev(t), 0, 1, 0),
                                                         first=lambda t: vec(_dev(t), 3, I32)), ValueError,
     "admm_ls_round_mean: 3 agents but w has 2 rows (agents must be distinct)"),
    ("admm_ls_round_mean", "duplicate_agents", _set(agents=lambda t: ids(_dev(t), 1, 1)), ValueError,
     "admm_ls_round_mean: agents must be distinct rows in [0, 2)"),
    ("admm_ls_round_mean", "agent_past_the_rows", _set(agents=lambda t: ids(_dev(t), 0, 2)), ValueError,
     "admm_ls_round_mean: agents must be distinct rows in [0, 2)"),
    ("admm_ls_round_mean", "negative_agent", _set(agents=lambda t: ids(_dev(t), -1, 0)), ValueError,
     "admm_ls_round_mean: agents must be distinct rows in [0, 2)"),
    ("admm_ls_round_mean", "no_agents", _set(agents=lambda t: vec(_dev(t), 0, I32)), ValueError,
     "admm_ls_round_mean needs at least one agent (the average indexes w[0])"),
    ("admm_ls_round_mean", "resid_total_dtype", _as("resid_total", F32), ValueError,
     lambda t: f"resid_total: expected contiguous float64 [2] on {_dev(t)}"),
    ("admm_ls_round_mean", "resid_total_short", _set(resid_total=lambda t: t["resid_total"][:1]), ValueError,
     lambda t: f"resid_total: expected contiguous float64 [2] on {_dev(t)}"),
    ("admm_ls_round_mean", "resid_total_cpu", _on_cpu("resid_total"), ValueError,
     lambda t: f"resid_total: expected contiguous float64 [2] on {_dev(t)}"),
    # --- ordered reductions
    ("ordered_mean", "order_dtype", _as("order", I64), ValueError, "order: expected contiguous int32 on the rows' device"),
    ("ordered_mean", "order_cpu", _on_cpu("order"), ValueError, "order: expected contiguous int32 on the rows' device"),
    ("ordered_mean", "order_empty", _set(order=lambda t: t["order"][:0]), ValueError,
     "ordered_mean needs at least one row (the reference indexes w[0])"),
    *_vec_cases("ordered_mean", "out", 10),
    ("ordered_sum", "order_dtype", _as("order", I64), ValueError, "order: expected contiguous int32 on the rows' device"),
    ("ordered_sum", "order_cpu", _on_cpu("order"), ValueError, "order: expected contiguous int32 on the rows' device"),
    *_vec_cases("ordered_sum", "out", 10), *_vec_cases("ordered_sum", "acc_in", 10),
    # --- the fused MLP step
    ("mlp_step", "X_cpu", _on_cpu("X"), ValueError, _mlp_x),
    ("mlp_step", "X_dtype", _as("X", F64), ValueError, _mlp_x),
    ("mlp_step", "X_rank", _set(X=lambda t: t["X"][:, 0]), ValueError, _mlp_x),
    ("mlp_step", "X_agents", _set(X=lambda t: t["X"][:1]), ValueError, _mlp_x),
    ("mlp_step", "X_features", _set(X=lambda t: t["X"][:, :, :3]), ValueError, _mlp_x),
    ("mlp_step", "X_stride", _set(X=lambda t: torch.zeros(2, 2, 8, device=_dev(t))[:, :, ::2]), ValueError,
     "X: samples must be contiguous"),
    ("mlp_step", "y_cpu", _on_cpu("y"), ValueError, _mlp_y),
    ("mlp_step", "y_dtype", _as("y", I32), ValueError, _mlp_y),
    ("mlp_step", "y_shape", _set(y=lambda t: t["y"][:, :1]), ValueError, _mlp_y),
    ("mlp_step", "y_stride", _set(y=lambda t: torch.zeros(2, 4, dtype=I64, device=_dev(t))[:, ::2]), ValueError, _mlp_y),
    ("mlp_step", "mom_missing", _set(mom=None), ValueError, "momentum != 0 needs mom"),
    ("mlp_step", "alpha_without_theta", _set(theta=None), ValueError, "alpha needs theta"),
    ("mlp_step", "grad_rows", _set(grad=lambda t: t["grad"][:1]), ValueError, "grad has fewer rows than w"),
    ("mlp_step", "mom_rows", _set(mom=lambda t: t["mom"][:1]), ValueError, "mom has fewer rows than w"),
    ("mlp_step", "alpha_rows", _set(alpha=lambda t: t["alpha"][:1]), ValueError, "alpha has fewer rows than w"),
    *_vec_cases("mlp_step", "theta", 30),
    ("mlp_step", "loss_dtype", _as("loss", F64), ValueError, _mlp_loss),
    ("mlp_step", "loss_short", _set(loss=lambda t: t["loss"][:1]), ValueError, _mlp_loss),
    ("mlp_step", "loss_cpu", _on_cpu("loss"), ValueError, _mlp_loss),
    ("mlp_step", "loss_stride", _set(loss=lambda t: vec(_dev(t), 4)[::2]), ValueError, _mlp_loss),
    ("mlp_step", "work_small", _set(work=lambda t: vec(_dev(t), _mlp_need() - 1, U8)), ValueError,
     lambda t: f"work: need {_mlp_need()} bytes on {_dev(t)}"),
    ("mlp_step", "work_cpu", _set(work=lambda t: torch.zeros(1 << 16, dtype=U8)), ValueError,
     lambda t: f"work: need {_mlp_need()} bytes on {_dev(t)}"),
]


@pytest.mark.parametrize("op,what,spoil,exc,message", REJECT, ids=[f"{c[0]}-{c[1]}" for c in REJECT])
def test_reject(op, what, spoil, exc, message, gpu, rec):
    make, call = CALLS[op]
    t = make(gpu)
    spoil(t)
    with pytest.raises(exc) as e:
        call(t)
    assert type(e.value) is exc
    assert str(e.value) == (message(t) if callable(message) else message)
    assert rec.calls == []


def test_reject_base_calls_are_valid(gpu, rec):
    """Every REJECT case spoils a call that is accepted as it stands."""
    for op, (make, call) in CALLS.items():
        call(make(gpu))
    assert len(rec.calls) == len(CALLS)
