"""SphereNet (models/spherenet.py, models/layers/spherenet_layer.py) on K18 / K19.

The reference builds its spherical basis with sympy (closed forms of j_l, lambdified) and
materialises two per-triplet embeddings, angle_emb (n k wide) and torsion_emb (n^2 k wide), that
every layer re-reads for its first projections.  Here

* the host tables (zeros of j_l, normalisers, harmonic prefactors) come from plain math: the
  zeros by bisection between the zeros of the previous order, rounded to fp32 as the reference's
  Jn_zeros stores them, the normalisers N_lq = (0.5 j_{l+1}(z_lq)^2)^-1/2 with the reference's
  fp32 rounding.  No sympy, no scipy;
* K18 evaluates the per-edge basis (stably: series / recurrence, never the closed form) and
  projects the per-triplet embeddings of all layers at once without writing them to memory;
* K19 forms the triplet messages of one layer and sums them per edge over K11's contiguous
  triplet ranges, deterministically.

Module names, constructor arguments, defaults and state_dict keys are the reference's.  The
reference computes and discards init_v and every update_v but the last (and the e2 branches
only they read); that work is skipped, so those parameters keep .grad None as they do there.
"""
import math
from math import sqrt

import numpy as np
import torch
from torch import nn
from torch.nn import Embedding, Linear

from . import ops
from .triplets import model_geometry_inputs, triplet_offsets, xyz_to_dat


def swish(x):
    return x * torch.sigmoid(x)


# ----------------------------------------------------------------------------------- host tables
def sph_jl(l, x):
    """Spherical Bessel function j_l(x) in double, x > 0: the power series below x = l + 1, the
    upward recurrence from j_0, j_1 above (the evaluation K18 uses on the device)."""
    x = float(x)
    if x < l + 1:
        pre = 1.0
        for i in range(1, l + 1):
            pre *= x / (2 * i + 1)
        h, term, total = -0.5 * x * x, 1.0, 1.0
        for k in range(1, 31):
            term *= h / (k * (2 * l + 2 * k + 1))
            total += term
        return pre * total
    s, c = math.sin(x), math.cos(x)
    j0 = s / x
    if l == 0:
        return j0
    j1 = (j0 - c) / x
    for i in range(1, l):
        j0, j1 = j1, (2 * i + 1) / x * j1 - j0
    return j1


def _bisect(f, a, b):
    fa = f(a)
    for _ in range(200):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        fm = f(m)
        if (fm < 0) == (fa < 0):
            a, fa = m, fm
        else:
            b = m
    return 0.5 * (a + b)


_TABLES = {}


def basis_tables(n, k):
    """(zeros (n, k) fp32, norm (n, k) fp32, pref (n^2) fp64) for num_spherical n and num_radial
    k, cached.  zeros[l, q]: the (q+1)-th positive zero of j_l; the zeros of j_l interlace
    those of j_{l-1}.  norm: the reference evaluates 0.5 j_{l+1}(z)^2 on the fp32 zero in fp32
    (Jn_zeros returns float32), so the same roundings are applied here.  pref[l^2 + p]: the
    prefactor of the p-th harmonic of order l in the order m = 0, 1..l (cos), -l..-1 (sin),
    sqrt(2) of m != 0 included."""
    key = (int(n), int(k))
    if key in _TABLES:
        return _TABLES[key]
    n, k = key
    points = [q * math.pi for q in range(1, k + n)]
    zeros = np.zeros((n, k), dtype=np.float32)
    zeros[0] = np.asarray(points[:k])
    for l in range(1, n):
        points = [_bisect(lambda x: sph_jl(l, x), points[q], points[q + 1])
                  for q in range(len(points) - 1)]
        zeros[l] = np.asarray(points[:k])
    norm = np.zeros((n, k), dtype=np.float32)
    for l in range(n):
        for q in range(k):
            r = zeros[l, q]
            # J_{l+1.5}(r) as the reference's fp32 Bessel call returns it, times sqrt(pi / 2r)
            jv = np.float32(math.sqrt(2.0 * float(r) / math.pi) * sph_jl(l + 1, float(r)))
            jn = np.sqrt(np.float32(np.pi) / (np.float32(2) * r)) * jv
            norm[l, q] = 0.5 * jn ** 2
    norm = (1 / norm ** 0.5).astype(np.float32)
    pref = np.zeros(n * n)
    for l in range(n):
        for p in range(2 * l + 1):
            m = 0 if p == 0 else (p if p <= l else 2 * l + 1 - p)
            f = ((2 * l + 1) * math.factorial(l - m) / (4 * math.pi * math.factorial(l + m))) ** 0.5
            pref[l * l + p] = f if m == 0 else 2 ** 0.5 * f
    _TABLES[key] = (zeros, norm, pref)
    return _TABLES[key]


def glorot_orthogonal(tensor, scale):
    """PyG's inits.glorot_orthogonal: orthogonal_, then rescaled to variance
    scale / (fan_in + fan_out)."""
    if tensor is not None:
        torch.nn.init.orthogonal_(tensor.data)
        s = scale / ((tensor.size(-2) + tensor.size(-1)) * tensor.var())
        tensor.data *= s.sqrt()


# ----------------------------------------------------------------------------------- layers
class dist_emb(torch.nn.Module):
    def __init__(self, num_radial, cutoff=5.0, envelope_exponent=5):
        super().__init__()
        self.cutoff = cutoff
        self.envelope_exponent = envelope_exponent
        self.freq = torch.nn.Parameter(torch.empty(num_radial))
        self.reset_parameters()

    def reset_parameters(self):
        self.freq.data = torch.arange(1, self.freq.numel() + 1).float().mul_(math.pi)


class emb(torch.nn.Module):
    """The three bases.  forward returns (rbf (E, k), jb (E, n k)): the per-edge parts; the
    per-triplet embeddings exist only inside K18 (materialise() forms them for tests)."""

    def __init__(self, num_spherical, num_radial, cutoff, envelope_exponent):
        super().__init__()
        self.num_spherical, self.num_radial = num_spherical, num_radial
        self.cutoff, self.envelope_exponent = cutoff, envelope_exponent
        self.dist_emb = dist_emb(num_radial, cutoff, envelope_exponent)
        zeros, norm, pref = basis_tables(num_spherical, num_radial)
        self.register_buffer("zeros", torch.from_numpy(zeros.copy()), persistent=False)
        self.register_buffer("norm", torch.from_numpy(norm.copy()), persistent=False)
        self.register_buffer("pref", torch.from_numpy(pref).float(), persistent=False)
        self.reset_parameters()

    def reset_parameters(self):
        self.dist_emb.reset_parameters()

    def forward(self, dist):
        return ops.SphEdgeBasisFn.apply(dist, self.dist_emb.freq, self.zeros, self.norm,
                                        self.cutoff, self.envelope_exponent)

    def materialise(self, dist, angle, torsion, idx_kj):
        """(dist_emb, angle_emb, torsion_emb) as the reference's emb.forward returns them."""
        rbf, jb = self.forward(dist)
        a, t = ops.sph_triplet_embeddings(jb.detach(), angle, torsion, idx_kj, self.pref,
                                          self.num_spherical, self.num_radial)
        return rbf, a, t


class ResidualLayer(torch.nn.Module):
    def __init__(self, hidden_channels, act=swish):
        super().__init__()
        self.act = act
        self.lin1 = Linear(hidden_channels, hidden_channels)
        self.lin2 = Linear(hidden_channels, hidden_channels)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_orthogonal(self.lin1.weight, scale=2.0)
        self.lin1.bias.data.fill_(0)
        glorot_orthogonal(self.lin2.weight, scale=2.0)
        self.lin2.bias.data.fill_(0)

    def forward(self, x):
        h = self.act(ops.linear(x, self.lin1.weight, self.lin1.bias))
        return x + self.act(ops.linear(h, self.lin2.weight, self.lin2.bias))


class init(torch.nn.Module):
    def __init__(self, num_radial, hidden_channels, act=swish, use_node_features=True):
        super().__init__()
        self.act = act
        self.use_node_features = use_node_features
        if self.use_node_features:
            self.emb = Embedding(95, hidden_channels)
        else:
            self.node_embedding = nn.Parameter(torch.empty((hidden_channels,)))
            nn.init.normal_(self.node_embedding)
        self.lin_rbf_0 = Linear(num_radial, hidden_channels)
        self.lin = Linear(3 * hidden_channels, hidden_channels)
        self.lin_rbf_1 = nn.Linear(num_radial, hidden_channels, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        if self.use_node_features:
            self.emb.weight.data.uniform_(-sqrt(3), sqrt(3))
        self.lin_rbf_0.reset_parameters()
        self.lin.reset_parameters()
        glorot_orthogonal(self.lin_rbf_1.weight, scale=2.0)

    def forward(self, x, rbf, i, j, want_e2=True):
        if self.use_node_features:
            x = self.emb(x)
        else:
            x = self.node_embedding[None, :].expand(x.shape[0], -1)
        rbf0 = self.act(ops.linear(rbf, self.lin_rbf_0.weight, self.lin_rbf_0.bias))
        cat = torch.cat([ops.gather(x, i), ops.gather(x, j), rbf0], dim=-1)
        e1 = self.act(ops.linear(cat, self.lin.weight, self.lin.bias))
        e2 = ops.linear(rbf, self.lin_rbf_1.weight) * e1 if want_e2 else None
        return e1, e2


class update_e(torch.nn.Module):
    def __init__(self, hidden_channels, int_emb_size, basis_emb_size_dist, basis_emb_size_angle,
                 basis_emb_size_torsion, num_spherical, num_radial, num_before_skip,
                 num_after_skip, act=swish):
        super().__init__()
        self.act = act
        self.lin_rbf1 = nn.Linear(num_radial, basis_emb_size_dist, bias=False)
        self.lin_rbf2 = nn.Linear(basis_emb_size_dist, hidden_channels, bias=False)
        self.lin_sbf1 = nn.Linear(num_spherical * num_radial, basis_emb_size_angle, bias=False)
        self.lin_sbf2 = nn.Linear(basis_emb_size_angle, int_emb_size, bias=False)
        self.lin_t1 = nn.Linear(num_spherical * num_spherical * num_radial,
                                basis_emb_size_torsion, bias=False)
        self.lin_t2 = nn.Linear(basis_emb_size_torsion, int_emb_size, bias=False)
        self.lin_rbf = nn.Linear(num_radial, hidden_channels, bias=False)

        self.lin_kj = nn.Linear(hidden_channels, hidden_channels)
        self.lin_ji = nn.Linear(hidden_channels, hidden_channels)

        self.lin_down = nn.Linear(hidden_channels, int_emb_size, bias=False)
        self.lin_up = nn.Linear(int_emb_size, hidden_channels, bias=False)

        self.layers_before_skip = torch.nn.ModuleList(
            [ResidualLayer(hidden_channels, act) for _ in range(num_before_skip)])
        self.lin = nn.Linear(hidden_channels, hidden_channels)
        self.layers_after_skip = torch.nn.ModuleList(
            [ResidualLayer(hidden_channels, act) for _ in range(num_after_skip)])
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_rbf1, self.lin_rbf2, self.lin_sbf1, self.lin_sbf2, self.lin_t1,
                    self.lin_t2):
            glorot_orthogonal(lin.weight, scale=2.0)
        glorot_orthogonal(self.lin_kj.weight, scale=2.0)
        self.lin_kj.bias.data.fill_(0)
        glorot_orthogonal(self.lin_ji.weight, scale=2.0)
        self.lin_ji.bias.data.fill_(0)
        glorot_orthogonal(self.lin_down.weight, scale=2.0)
        glorot_orthogonal(self.lin_up.weight, scale=2.0)
        for res_layer in self.layers_before_skip:
            res_layer.reset_parameters()
        glorot_orthogonal(self.lin.weight, scale=2.0)
        self.lin.bias.data.fill_(0)
        for res_layer in self.layers_after_skip:
            res_layer.reset_parameters()
        glorot_orthogonal(self.lin_rbf.weight, scale=2.0)

    def forward(self, x1, rbf0, S, P, idx_kj, idx_ji, offsets, want_e2=True):
        """x1 (E, hidden): the edge features; S (T, ba), P (T, bt): this layer's first
        projections from K18.  -> (e1, e2), e2 None unless want_e2."""
        x_ji = self.act(ops.linear(x1, self.lin_ji.weight, self.lin_ji.bias))
        x_kj = self.act(ops.linear(x1, self.lin_kj.weight, self.lin_kj.bias))
        rbf = ops.linear(ops.linear(rbf0, self.lin_rbf1.weight), self.lin_rbf2.weight)
        x_kj = self.act(ops.linear(x_kj * rbf, self.lin_down.weight))
        m = ops.TripletInteractFn.apply(x_kj, S, P, self.lin_sbf2.weight, self.lin_t2.weight,
                                        idx_kj, idx_ji, offsets)
        x_kj = self.act(ops.linear(m, self.lin_up.weight))
        e1 = x_ji + x_kj
        for layer in self.layers_before_skip:
            e1 = layer(e1)
        e1 = self.act(ops.linear(e1, self.lin.weight, self.lin.bias)) + x1
        for layer in self.layers_after_skip:
            e1 = layer(e1)
        e2 = ops.linear(rbf0, self.lin_rbf.weight) * e1 if want_e2 else None
        return e1, e2


class update_v(torch.nn.Module):
    def __init__(self, hidden_channels, out_emb_channels, out_channels, num_output_layers, act,
                 output_init):
        super().__init__()
        self.act = act
        self.output_init = output_init
        self.lin_up = nn.Linear(hidden_channels, out_emb_channels, bias=True)
        self.lins = torch.nn.ModuleList(
            [nn.Linear(out_emb_channels, out_emb_channels) for _ in range(num_output_layers)])
        self.lin = nn.Linear(out_emb_channels, out_channels, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_orthogonal(self.lin_up.weight, scale=2.0)
        for lin in self.lins:
            glorot_orthogonal(lin.weight, scale=2.0)
            lin.bias.data.fill_(0)
        if self.output_init == 'zeros':
            self.lin.weight.data.fill_(0)
        if self.output_init == 'GlorotOrthogonal':
            glorot_orthogonal(self.lin.weight, scale=2.0)

    def forward(self, e2, i, num_nodes):
        """Sum of e2 over each node's incoming edges (the receiver CSR), then the output MLP."""
        v = ops.SegmentReduceFn.apply(e2, ops.checked_csr(i, num_nodes), "sum")
        v = ops.linear(v, self.lin_up.weight, self.lin_up.bias)
        for lin in self.lins:
            v = self.act(ops.linear(v, lin.weight, lin.bias))
        return ops.linear(v, self.lin.weight)


class update_u(torch.nn.Module):
    def forward(self, u, v, batch):
        return u + ops.SegmentReduceFn.apply(v, ops.checked_csr(batch, u.shape[0]), "sum")


# ----------------------------------------------------------------------------------- model
class SphereNetModel(torch.nn.Module):
    """SphereNet, "Spherical Message Passing for 3D Molecular Graphs" (models/spherenet.py).

    periodic (keyword-only; a plain attribute, present only when set): a batch that carries
    edge_shift_idx (and cell) runs K11p, the image-aware triplets of include/gmp.h, with dist,
    angle and torsion from the edge vectors (pos[j] - pos[i]) + graph.edge_shift(batch); forces
    and the stress (energy_and_forces(stress=True)) and training on the energy work as for an
    open structure (first order only).  Off (the default), such a batch raises
    NotImplementedError; a batch without edge_shift_idx runs the open-boundary path either
    way."""

    def __init__(self, cutoff=10, num_layers=4, hidden_channels=128, in_dim=1, out_dim=1,
                 int_emb_size=64, basis_emb_size_dist=8, basis_emb_size_angle=8,
                 basis_emb_size_torsion=8, out_emb_channels=128, num_spherical=7, num_radial=6,
                 envelope_exponent=5, num_before_skip=1, num_after_skip=2, num_output_layers=2,
                 act=swish, output_init='GlorotOrthogonal', use_node_features=True, *,
                 periodic=False):
        super().__init__()
        if num_layers < 1:
            raise ValueError("SphereNetModel needs at least one layer")
        if periodic:  # a plain attribute, set only when asked for (forward reads it by getattr)
            self.periodic = True
        self.cutoff = cutoff
        self.num_spherical, self.num_radial = num_spherical, num_radial
        self.init_e = init(num_radial, hidden_channels, act, use_node_features=use_node_features)
        self.init_v = update_v(hidden_channels, out_emb_channels, out_dim, num_output_layers, act,
                               output_init)
        self.init_u = update_u()
        self.emb = emb(num_spherical, num_radial, self.cutoff, envelope_exponent)
        self.update_vs = torch.nn.ModuleList([
            update_v(hidden_channels, out_emb_channels, out_dim, num_output_layers, act,
                     output_init) for _ in range(num_layers)])
        self.update_es = torch.nn.ModuleList([
            update_e(hidden_channels, int_emb_size, basis_emb_size_dist, basis_emb_size_angle,
                     basis_emb_size_torsion, num_spherical, num_radial, num_before_skip,
                     num_after_skip, act) for _ in range(num_layers)])
        self.update_us = torch.nn.ModuleList([update_u() for _ in range(num_layers)])
        self.reset_parameters()

    def reset_parameters(self):
        self.init_e.reset_parameters()
        self.init_v.reset_parameters()
        self.emb.reset_parameters()
        for ue in self.update_es:
            ue.reset_parameters()
        for uv in self.update_vs:
            uv.reset_parameters()

    def forward(self, batch_data):
        pos, shift, shift_idx = model_geometry_inputs("SphereNetModel", self, batch_data, True)
        z, batch = batch_data.atoms, batch_data.batch
        dist, angle, torsion, i, j, idx_kj, idx_ji = xyz_to_dat(
            pos, batch_data.edge_index, z.size(0), use_torsion=True, shift=shift,
            shift_idx=shift_idx)
        return self.forward_from_geometry(z, dist, angle, torsion, i, j, idx_kj, idx_ji, batch,
                                          num_graphs=getattr(batch_data, "num_graphs", None))

    def forward_from_geometry(self, atoms, dist, angle, torsion, i, j, idx_kj, idx_ji, batch,
                              num_graphs=None):
        """The model downstream of xyz_to_dat: dist (E), angle / torsion (T), i / j (E) the
        target / source of each edge, idx_kj / idx_ji (T) the edges of each triplet with idx_ji
        non-decreasing (as K11 and the reference emit it), batch (N).  -> (num_graphs,
        out_dim).  Gradients flow to dist, angle and torsion (and through TripletGeomFn to
        pos)."""
        ops._need_cuda(atoms, dist, angle, torsion, i, j, idx_kj, idx_ji, batch)
        N, E, L = atoms.size(0), dist.numel(), len(self.update_es)
        if num_graphs is None:
            num_graphs = int(batch.max().item()) + 1 if N else 0
        n, k = self.num_spherical, self.num_radial
        offsets = triplet_offsets(idx_ji, E)
        rbf, jb = self.emb(dist)
        weights = [ue.lin_sbf1.weight for ue in self.update_es] + \
                  [ue.lin_t1.weight for ue in self.update_es]
        SP = ops.SphTripletProjFn.apply(jb, angle, torsion, idx_kj, self.emb.pref, n, k, L,
                                        *weights)
        # init_v and all update_vs but the last are computed and discarded by the reference
        # (the virtual-node sum is disabled there): their inputs (e2) are not formed
        e1, _ = self.init_e(atoms, rbf, i, j, want_e2=False)
        e2 = None
        for l, ue in enumerate(self.update_es):
            e1, e2 = ue(e1, rbf, SP[l], SP[L + l], idx_kj, idx_ji, offsets, want_e2=l == L - 1)
        v = self.update_vs[-1](e2, i, N)
        return ops.SegmentReduceFn.apply(v, ops.checked_csr(batch, num_graphs), "sum")
