"""Golden FedAvg / FedProx least-squares trajectories from the REFERENCE (needs
the reference checkout that make_golden.py's DEC_SRC names):
    python tests/golden/make_golden_fed_ls.py

make_golden_admm.py's recipe -- the shipped Server.run (DEC/servers.py:50-81)
unchanged, on the least-squares "model", dataset and criterion of that file
(imported from it) -- for the other two servers that the same run drives:
FedAvg_Server (FedAvg_Client.update_model, DEC/clients.py:85-95) and
FedProx_Server (FedProx_Client.update_model, :101-115), whose update_duals is
the base class's no-op (:58-59).  The same three CASES, which is what
dol_fed_ls_round_f32 computes with DOL_FED_AVG / DOL_FED_PROX.
Recorded (npz, no pickles, no alpha): the targets, theta_0, every round's
sampled order and theta, and the final per-client w and momentum rows, under
"<algorithm>__<case>__<name>" with algorithm = fedavg / fedprox.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import DEC_SRC, _import_project, _placeholder_torchvision  # noqa: E402
from make_golden_admm import CASES, LAYOUTS, _TargetSet, flat, ls_criterion, make_model_cls  # noqa: E402

SERVERS = {"fedavg": "FedAvg_Server", "fedprox": "FedProx_Server"}


def run_case(algorithm, name):
    layout, N, frac, rounds, local_ep, items, bs, lr, mom, rho, seed = CASES[name]
    lay = LAYOUTS[layout]
    P = int(sum(np.prod(s) for _, s in lay))
    mods = _import_project(DEC_SRC, ["utils", "sampling", "servers"])
    U, S, srv = mods["utils"], mods["sampling"], mods["servers"]
    rng = np.random.default_rng(1000 + seed)
    targets = rng.standard_normal((N, P)).astype(np.float32)
    n_train = N * items

    def get_dataset(args):
        train, test = _TargetSet(n_train, P), _TargetSet(4, P)
        groups = S.mnist_iid(train, args.num_users)
        owner = np.zeros((n_train, P), np.float32)
        for u, idxs in groups.items():
            for i in idxs:
                owner[int(i)] = targets[u]
        train.owner_targets = owner
        test.owner_targets = np.zeros((4, P), np.float32)
        return train, test, groups

    srv.get_dataset = get_dataset
    srv.Model1 = make_model_cls(lay)
    args = U.DotDict(dict(num_users=N, local_ep=local_ep, local_bs=bs, lr=lr, model="Model1", dataset="synthetic",
                          iid=True, rho=rho, seed=seed, momentum=mom, verbose=False, device="cpu"))
    orders, thetas = [], []
    choice = np.random.choice

    def recording_choice(*a, **kw):
        r = choice(*a, **kw)
        orders.append(np.asarray(r, np.int64))
        return r

    with contextlib.redirect_stdout(io.StringIO()):
        s = getattr(srv, SERVERS[algorithm])(args)
        for c in s.clients + [s.global_client]:
            c.criterion = ls_criterion
        theta0 = flat(s.global_client.model.state_dict())
        steps = [len(c.loaders["train"]) for c in s.clients]
        np.random.choice = recording_choice
        try:
            for _ in range(rounds):
                s.run(frac, 1)
                thetas.append(flat(s.global_client.model.state_dict()))
        finally:
            np.random.choice = choice
    assert len(set(steps)) == 1, steps
    moms = []
    for c in s.clients:
        st = c.optimizer.state
        ps = list(c.model.parameters())
        moms.append(np.concatenate([st[p]["momentum_buffer"].numpy().reshape(-1) if p in st and
                                    st[p].get("momentum_buffer") is not None else np.zeros(p.numel(), np.float32)
                                    for p in ps]))
    key = f"{algorithm}__{name}"
    return {
        f"{key}__targets": targets, f"{key}__theta0": theta0, f"{key}__orders": np.stack(orders),
        f"{key}__thetas": np.stack(thetas), f"{key}__w": np.stack([flat(c.model.state_dict()) for c in s.clients]),
        f"{key}__mom": np.stack(moms).astype(np.float32),
        f"{key}__params": np.array([N, frac, rounds, local_ep * steps[0], lr, mom, rho], np.float64),
    }


def main():
    _placeholder_torchvision()
    out = {}
    for algorithm in SERVERS:
        for name in CASES:
            out.update(run_case(algorithm, name))
    np.savez_compressed(os.path.join(HERE, "fed_ls.npz"), **out)
    print("wrote fed_ls.npz", sorted(k for k in out if k.endswith("__params")))


if __name__ == "__main__":
    main()
