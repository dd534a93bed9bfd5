"""Energy-and-force evaluation: F = -dE/dpos through the twice-differentiable SchNet and
DimeNet++ paths, and the stress of a periodic structure.

A loss on the forces needs the gradient of a gradient.  Inside `second_order()` (gmp_amd.ops) the
SchNet path, and a DimeNetPPModel built (or set) with twice_differentiable=True, record autograd
Functions whose backward is itself recorded, so the forces returned here (create_graph=True) can
be trained on.  EGNN, GVP, TFN, MACE, SphereNet and a DimeNetPPModel without the flag keep
once-differentiable Functions: a second-order backward through them raises.
"""
import copy

import torch

from . import ops
from .ops import second_order


def _strained(batch, eps):
    """Shallow copy of `batch` under the symmetric strain sym(eps), eps (B, 3, 3):
    pos -> pos + pos @ sym(eps)[batch], cell -> cell + cell @ sym(eps)."""
    sym = 0.5 * (eps + eps.transpose(1, 2))
    per_node = ops.gather(sym.reshape(-1, 9), batch.batch, 0).view(-1, 3, 3)
    if getattr(batch, "edge_shift_idx", None) is not None and \
            getattr(batch, "edge_graph", None) is None:
        batch.edge_graph = batch.batch[batch.edge_index[1]]  # kept: its CSR stays cached
    out = copy.copy(batch)
    out.pos = batch.pos + (batch.pos.unsqueeze(2) * per_node).sum(1)
    cell = batch.cell.reshape(-1, 3, 3)
    out.cell = cell + (cell.unsqueeze(3) * sym.unsqueeze(1)).sum(2)
    return out


def energy_and_forces(model, batch, create_graph=None, stress=False):
    """(energy, forces) of `model` on `batch`, forces = -d energy.sum() / d batch.pos, (N, 3).

    Sets requires_grad on batch.pos if needed, runs the model under second_order() and calls
    torch.autograd.grad, so no .grad is touched.  create_graph defaults to
    torch.is_grad_enabled() and model.training: forces that a loss can be back-propagated through
    while training, plain forces in evaluation.

    stress=True (the batch carries a cell) returns (energy, forces, sigma) with sigma (B, 3, 3)
    = (1 / V) dE / d eps at eps = 0 under the symmetric strain pos -> pos + pos @ sym(eps)[batch],
    cell -> cell + cell @ sym(eps), applied to a shallow copy of the batch; V = |det cell|.
    Periodic batches (edge_shift_idx, cell) run through SchNet, MACE, TFN and a DimeNetPPModel or
    SphereNetModel built (or set) with periodic=True; with twice_differentiable=True as well,
    forces and sigma of DimeNet++ can be trained on (SphereNet: first order only, inference
    forces and stress, and training on the energy)."""
    if create_graph is None:
        create_graph = torch.is_grad_enabled() and model.training
    pos = batch.pos
    if not pos.requires_grad:
        pos.requires_grad_(True)
    if not stress:
        with torch.enable_grad(), second_order():
            energy = model(batch)
            (g,) = torch.autograd.grad(energy.sum(), pos, create_graph=create_graph)
        if not create_graph:
            energy = energy.detach()
        return energy, -g
    if getattr(batch, "cell", None) is None:
        raise ValueError("stress=True needs batch.cell")
    cell = batch.cell.reshape(-1, 3, 3)
    eps = torch.zeros_like(cell, requires_grad=True)
    with torch.enable_grad(), second_order():
        energy = model(_strained(batch, eps))
        g, g_eps = torch.autograd.grad(energy.sum(), (pos, eps), create_graph=create_graph)
        vol = (cell[:, 0] * torch.linalg.cross(cell[:, 1], cell[:, 2])).sum(1).abs()
        sigma = g_eps / vol.detach().view(-1, 1, 1)
    if not create_graph:
        energy, sigma = energy.detach(), sigma.detach()
    return energy, -g, sigma
