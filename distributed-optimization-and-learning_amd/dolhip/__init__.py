"""dolhip — MI355X (gfx950) engine for the per-round consensus step of
AlirezaMoseni/Distributed-Optimization-and-Learning.

Layers:
  _native   ctypes binding of libdol_hip.so (C-ABI: include/dol_hip.h)
  ops       tensor-level wrappers (validation, current torch stream)
  graph     communication_graph / Neighbors-as-CSR / ring plan (host)
  bank      AgentBank: stacked [N, ld] agent state in HBM, module views
  parallel  agent sharding over ranks: ring halo exchange, global mean
  synthetic the separable workloads: SeparableDGD, and the server round of
            SeparableADMM / SeparableFedAvg / SeparableFedProx (ops.fed_ls_round*)
            and SeparableScaffold (ops.scaffold_ls_round); gradient tracking:
            SeparableGT (agent-major ring, ops.gt_ring), SeparableGTCSR (agent-major
            bank, any sparse W, ops.gt_csr), SeparableGTPM, and SeparableGTPush
            (push-sum, column-stochastic weights, ops.gt_push_csr); EXTRA, which
            mixes the parameters only: SeparableEXTRA (ops.extra_csr / ops.extra_ring)
            and SeparableEXTRAPM (parameter-major bank, ops.extra_csr_pm)
  mlp       BatchedMLP: every agent's MLP forward / backward / step in one kernel
  mlp_exact ExactMLPGossip: gradient tracking and EXTRA for those agents, the
            gradients fed as bank rows (ops.gt_grad_csr / ops.extra_grad_csr)
The reference-shaped APIs live beside this package:
  weighted_average/  (Simulator, DecFedAvg, FedLCon, Client, ...)
  primal_dual/       (Server, FedAvg_/FedProx_/FedAdmm_Server/_Client)
"""
from ._native import DolNativeError, build, lib  # noqa: F401
from . import ops, graph, bank  # noqa: F401
from .bank import AgentBank  # noqa: F401
from .graph import MixingPlan, communication_graph, csr_from_dense  # noqa: F401
from .mlp_exact import ExactMLPGossip  # noqa: F401
from .synthetic import SeparableEXTRA, SeparableGT, SeparableGTCSR, SeparableGTPush, SeparableScaffold  # noqa: F401

__version__ = "0.1.0"
