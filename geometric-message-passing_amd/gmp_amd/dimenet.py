"""DimeNet++ (models/dimenet.py: PyG 2.3.1 DimeNetPlusPlus) on K11 / K18d / K19d.

PyG materialises the per-triplet spherical basis sbf (T, n k) once and every interaction block
re-reads it for its first projection.  Here

* K11 (triplets.dimenet_angles) emits the triplets and the angle at vertex i;
* K18d evaluates the per-edge parts rbf and sbe = env N j_l (stably, as K18; the envelope carries
  PyG's [x < 1] factor) and projects sbf = sbe[idx_kj] * Y_l0(angle) through lin_sbf1 of every
  block at once without writing it to memory;
* K19d forms the triplet messages of one block and sums them per edge over K11's contiguous
  triplet ranges, deterministically.

Module names, constructor arguments, defaults and state_dict keys are PyG's.  The basis tables
are spherenet.basis_tables (no sympy): non-persistent buffers of `sbf`.
"""
import math
from math import sqrt

import torch
from torch.nn import Embedding, Linear

from . import ops
from .spherenet import ResidualLayer, basis_tables, glorot_orthogonal, swish
from .triplets import dimenet_angles, model_geometry_inputs, triplet_offsets


def _activation(act):
    if callable(act):
        return act
    if act in ("swish", "silu"):
        return swish
    raise ValueError(f"DimeNetPPModel: unknown activation {act!r} (use 'swish' or a callable)")


def _segment_sum(x, csr, twice):
    """The segmented sum as today's SegmentReduceFn, or through ops.segment_reduce_fn (recorded
    backward inside second_order()) on the twice-differentiable path."""
    if twice:
        return ops.segment_reduce_fn(x, csr, "sum")
    return ops.SegmentReduceFn.apply(x, csr, "sum")


class BesselBasisLayer(torch.nn.Module):
    """Holds freq; the values come from K18d together with sbe (DimeNetPPModel.bases)."""

    def __init__(self, num_radial, cutoff=5.0, envelope_exponent=5):
        super().__init__()
        self.cutoff = cutoff
        self.envelope_exponent = envelope_exponent
        self.freq = torch.nn.Parameter(torch.empty(num_radial))
        self.reset_parameters()

    def reset_parameters(self):
        self.freq.data = torch.arange(1, self.freq.numel() + 1).float().mul_(math.pi)


class SphericalBasisLayer(torch.nn.Module):
    """No parameters; the host tables of the basis as non-persistent buffers."""

    def __init__(self, num_spherical, num_radial, cutoff=5.0, envelope_exponent=5):
        super().__init__()
        self.num_spherical, self.num_radial = num_spherical, num_radial
        self.cutoff, self.envelope_exponent = cutoff, envelope_exponent
        zeros, norm, pref = basis_tables(num_spherical, num_radial)
        self.register_buffer("zeros", torch.from_numpy(zeros.copy()), persistent=False)
        self.register_buffer("norm", torch.from_numpy(norm.copy()), persistent=False)
        self.register_buffer("pref", torch.from_numpy(pref).float(), persistent=False)


class EmbeddingBlock(torch.nn.Module):
    def __init__(self, num_radial, hidden_channels, act):
        super().__init__()
        self.act = act
        self.emb = Embedding(95, hidden_channels)
        self.lin_rbf = Linear(num_radial, hidden_channels)
        self.lin = Linear(3 * hidden_channels, hidden_channels)
        self.reset_parameters()

    def reset_parameters(self):
        self.emb.weight.data.uniform_(-sqrt(3), sqrt(3))
        self.lin_rbf.reset_parameters()
        self.lin.reset_parameters()

    def forward(self, x, rbf, i, j):
        x = self.emb(x)
        rbf = self.act(ops.linear(rbf, self.lin_rbf.weight, self.lin_rbf.bias))
        cat = torch.cat([ops.gather(x, i), ops.gather(x, j), rbf], dim=-1)
        return self.act(ops.linear(cat, self.lin.weight, self.lin.bias))


class InteractionPPBlock(torch.nn.Module):
    def __init__(self, hidden_channels, int_emb_size, basis_emb_size, num_spherical, num_radial,
                 num_before_skip, num_after_skip, act):
        super().__init__()
        self.act = act
        self.lin_rbf1 = Linear(num_radial, basis_emb_size, bias=False)
        self.lin_rbf2 = Linear(basis_emb_size, hidden_channels, bias=False)
        self.lin_sbf1 = Linear(num_spherical * num_radial, basis_emb_size, bias=False)
        self.lin_sbf2 = Linear(basis_emb_size, int_emb_size, bias=False)

        self.lin_kj = Linear(hidden_channels, hidden_channels)
        self.lin_ji = Linear(hidden_channels, hidden_channels)

        self.lin_down = Linear(hidden_channels, int_emb_size, bias=False)
        self.lin_up = Linear(int_emb_size, hidden_channels, bias=False)

        self.layers_before_skip = torch.nn.ModuleList(
            [ResidualLayer(hidden_channels, act) for _ in range(num_before_skip)])
        self.lin = Linear(hidden_channels, hidden_channels)
        self.layers_after_skip = torch.nn.ModuleList(
            [ResidualLayer(hidden_channels, act) for _ in range(num_after_skip)])
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_rbf1, self.lin_rbf2, self.lin_sbf1, self.lin_sbf2, self.lin_kj,
                    self.lin_ji, self.lin_down, self.lin_up, self.lin):
            glorot_orthogonal(lin.weight, scale=2.0)
            if lin.bias is not None:
                lin.bias.data.fill_(0)
        for res_layer in list(self.layers_before_skip) + list(self.layers_after_skip):
            res_layer.reset_parameters()

    def forward(self, x, rbf, S, idx_kj, idx_ji, offsets, twice=False):
        """x (E, hidden): the edge features; S (T, basis_emb_size): this block's first
        projection lin_sbf1(sbf) from K18d.  twice: record the twice-differentiable K19d."""
        x_ji = self.act(ops.linear(x, self.lin_ji.weight, self.lin_ji.bias))
        x_kj = self.act(ops.linear(x, self.lin_kj.weight, self.lin_kj.bias))
        rbf = ops.linear(ops.linear(rbf, self.lin_rbf1.weight), self.lin_rbf2.weight)
        x_kj = self.act(ops.linear(x_kj * rbf, self.lin_down.weight))
        interact = ops.TripletInteract1_2Fn if twice else ops.TripletInteract1Fn
        m = interact.apply(x_kj, S, self.lin_sbf2.weight, idx_kj, idx_ji, offsets)
        h = x_ji + self.act(ops.linear(m, self.lin_up.weight))
        for layer in self.layers_before_skip:
            h = layer(h)
        h = self.act(ops.linear(h, self.lin.weight, self.lin.bias)) + x
        for layer in self.layers_after_skip:
            h = layer(h)
        return h


class OutputPPBlock(torch.nn.Module):
    def __init__(self, num_radial, hidden_channels, out_emb_channels, out_channels, num_layers,
                 act):
        super().__init__()
        self.act = act
        self.lin_rbf = Linear(num_radial, hidden_channels, bias=False)
        self.lin_up = Linear(hidden_channels, out_emb_channels, bias=False)
        self.lins = torch.nn.ModuleList(
            [Linear(out_emb_channels, out_emb_channels) for _ in range(num_layers)])
        self.lin = Linear(out_emb_channels, out_channels, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_orthogonal(self.lin_rbf.weight, scale=2.0)
        glorot_orthogonal(self.lin_up.weight, scale=2.0)
        for lin in self.lins:
            glorot_orthogonal(lin.weight, scale=2.0)
            lin.bias.data.fill_(0)
        self.lin.weight.data.fill_(0)

    def forward(self, x, rbf, i, num_nodes, twice=False):
        """Sum of lin_rbf(rbf) * x over each node's incoming edges, then the output MLP."""
        x = ops.linear(rbf, self.lin_rbf.weight) * x
        v = _segment_sum(x, ops.checked_csr(i, num_nodes), twice)
        v = ops.linear(v, self.lin_up.weight)
        for lin in self.lins:
            v = self.act(ops.linear(v, lin.weight, lin.bias))
        return ops.linear(v, self.lin.weight)


class DimeNetPPModel(torch.nn.Module):
    """DimeNet++, "Fast and Uncertainty-Aware Directional Message Passing for Non-Equilibrium
    Molecules" (models/dimenet.py).  in_dim and max_num_neighbors are accepted and unused, as in
    the reference (its forward takes batch.edge_index).

    twice_differentiable (keyword-only; a plain attribute, not in the state_dict): inside
    gmp_amd.second_order() the model records twice-differentiable Functions (K11, K18d and K19d
    with their *_bwd2 kernels), so a loss on the forces -dE/dpos can be trained.  False, or
    outside the context: the once-differentiable path, on which a second backward raises.

    periodic (keyword-only; a plain attribute as well): a batch that carries edge_shift_idx (and
    cell) runs K11p, the image-aware triplets of include/gmp.h, with dist and angle from the
    edge vectors (pos[j] - pos[i]) + graph.edge_shift(batch); forces, the stress
    (energy_and_forces(stress=True)) and, with twice_differentiable, training on them work as for
    an open structure.  Off (the default), such a batch raises NotImplementedError; a batch
    without edge_shift_idx runs the open-boundary path either way."""

    def __init__(self, hidden_channels=128, in_dim=1, out_dim=1, num_layers=4, int_emb_size=64,
                 basis_emb_size=8, out_emb_channels=256, num_spherical=7, num_radial=6, cutoff=10,
                 max_num_neighbors=32, envelope_exponent=5, num_before_skip=1, num_after_skip=2,
                 num_output_layers=3, act='swish', *, twice_differentiable=False, periodic=False):
        super().__init__()
        self.twice_differentiable = bool(twice_differentiable)
        self.periodic = bool(periodic)
        if num_spherical < 2:
            raise ValueError("num_spherical should be greater than 1")
        act = _activation(act)
        self.cutoff = cutoff
        self.num_spherical, self.num_radial = num_spherical, num_radial
        self.envelope_exponent = envelope_exponent
        self.rbf = BesselBasisLayer(num_radial, cutoff, envelope_exponent)
        self.sbf = SphericalBasisLayer(num_spherical, num_radial, cutoff, envelope_exponent)
        self.emb = EmbeddingBlock(num_radial, hidden_channels, act)
        self.output_blocks = torch.nn.ModuleList([
            OutputPPBlock(num_radial, hidden_channels, out_emb_channels, out_dim,
                          num_output_layers, act) for _ in range(num_layers + 1)])
        self.interaction_blocks = torch.nn.ModuleList([
            InteractionPPBlock(hidden_channels, int_emb_size, basis_emb_size, num_spherical,
                               num_radial, num_before_skip, num_after_skip, act)
            for _ in range(num_layers)])

    def reset_parameters(self):
        self.rbf.reset_parameters()
        self.emb.reset_parameters()
        for out in self.output_blocks:
            out.reset_parameters()
        for interaction in self.interaction_blocks:
            interaction.reset_parameters()

    def _twice(self):
        return bool(getattr(self, "twice_differentiable", False)) and ops.second_order_enabled()

    def bases(self, dist):
        """(rbf (E, k), sbe (E, n k)): the per-edge parts of the two bases from K18d."""
        fn = ops.DimeEdgeBasis2Fn if self._twice() else ops.DimeEdgeBasisFn
        return fn.apply(dist, self.rbf.freq, self.sbf.zeros, self.sbf.norm, self.cutoff,
                        self.envelope_exponent)

    def projections(self, sbe, angle, idx_kj):
        """S[l] (T, basis_emb_size) = lin_sbf1 of block l applied to sbf, for every block (K18d)."""
        blocks = self.interaction_blocks
        L, n, k = len(blocks), self.num_spherical, self.num_radial
        if not L:
            return ()
        weights = [blk.lin_sbf1.weight for blk in blocks]
        if self._twice():
            wt = ops.dime_feature_major(weights, n * k)
            S = ops.DimeTripletProj2Fn.apply(sbe, angle, wt, idx_kj, self.sbf.pref, n, k, L,
                                             weights[0].shape[0])
            return S.unbind(0)
        return ops.DimeTripletProjFn.apply(sbe, angle, idx_kj, self.sbf.pref, n, k, L, *weights)

    def forward(self, batch):
        twice = self._twice()
        pos, shift, shift_idx = model_geometry_inputs("DimeNetPPModel", self, batch, not twice)
        z = batch.atoms
        dist, angle, i, j, _, _, _, idx_kj, idx_ji = dimenet_angles(
            pos, batch.edge_index, z.size(0), twice_differentiable=twice, shift=shift,
            shift_idx=shift_idx)
        return self.forward_from_geometry(z, dist, angle, i, j, idx_kj, idx_ji, batch.batch,
                                          num_graphs=getattr(batch, "num_graphs", None))

    def forward_from_geometry(self, atoms, dist, angle, i, j, idx_kj, idx_ji, batch,
                              num_graphs=None):
        """The model downstream of dimenet_angles: dist (E), angle (T, at vertex i), i / j (E)
        the target / source of each edge, idx_kj / idx_ji (T) the edges of each triplet with
        idx_ji non-decreasing (as K11 and PyG emit it), batch (N).  -> (num_graphs, out_dim).
        Gradients flow to dist and angle (and through TripletGeomFn to pos); twice
        differentiable where twice_differentiable is set inside gmp_amd.second_order()."""
        ops._need_cuda(atoms, dist, angle, i, j, idx_kj, idx_ji, batch)
        N, E, L = atoms.size(0), dist.numel(), len(self.interaction_blocks)
        if num_graphs is None:
            num_graphs = int(batch.max().item()) + 1 if N else 0
        offsets = triplet_offsets(idx_ji, E)
        twice = self._twice()
        rbf, sbe = self.bases(dist)
        S = self.projections(sbe, angle, idx_kj)
        x = self.emb(atoms, rbf, i, j)
        P = self.output_blocks[0](x, rbf, i, N, twice)
        for l, blk in enumerate(self.interaction_blocks):
            x = blk(x, rbf, S[l], idx_kj, idx_ji, offsets, twice)
            P = P + self.output_blocks[l + 1](x, rbf, i, N, twice)
        return _segment_sum(P, ops.checked_csr(batch, num_graphs), twice)
