"""Energy-and-force evaluation: F = -dE/dpos through the twice-differentiable SchNet path.

A loss on the forces needs the gradient of a gradient.  Inside `second_order()` (gmp_amd.ops) the
SchNet path records autograd Functions whose backward is itself recorded, so the forces returned
here (create_graph=True) can be trained on.  EGNN, GVP, TFN and MACE keep once-differentiable
Functions: a second-order backward through them raises.
"""
import torch

from .ops import second_order


def energy_and_forces(model, batch, create_graph=None):
    """(energy, forces) of `model` on `batch`, forces = -d energy.sum() / d batch.pos, (N, 3).

    Sets requires_grad on batch.pos if needed, runs the model under second_order() and calls
    torch.autograd.grad, so no .grad is touched.  create_graph defaults to
    torch.is_grad_enabled() and model.training: forces that a loss can be back-propagated through
    while training, plain forces in evaluation."""
    if create_graph is None:
        create_graph = torch.is_grad_enabled() and model.training
    pos = batch.pos
    if not pos.requires_grad:
        pos.requires_grad_(True)
    with torch.enable_grad(), second_order():
        energy = model(batch)
        (g,) = torch.autograd.grad(energy.sum(), pos, create_graph=create_graph)
    if not create_graph:
        energy = energy.detach()
    return energy, -g
