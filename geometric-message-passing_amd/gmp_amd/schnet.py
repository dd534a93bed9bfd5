"""SchNet on the MI355X kernels — drop-in for models/schnet.py:9-80 (SchNetModel over PyG 2.3.1
SchNet: InteractionBlock / CFConv / GaussianSmearing / ShiftedSoftplus), same module tree and
state_dict keys (interactions.<k>.mlp.* shared with interactions.<k>.conv.nn.*).

CFConv keeps PyG's MessagePassing contract (aggr 'add', x_j = x[edge_index[0]], sum at
edge_index[1] with dim_size = N) through gmp_amd.MessagePassing: the x_j gather is the HIP gather
kernel and the sum the HIP segmented reduce over the receiver CSR.  Config C1 (k-chains) is
tiny; on the C2-sized graphs the filter network's edge Linears take ops.linear: library GEMMs
forward / dx, weight gradients by the deterministic edge outer sum (the library's K = E
reductions ran at 1.8 ms each, profiles/r01_schnet_kernels.md).  PyG itself is absent: the internals follow
PyG 2.3.1's published code (parity unpinned, see oracle/schnet.py).
"""
import math

import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .graph import edge_shift
from .message_passing import MessagePassing
from .scatter import global_add_pool, global_mean_pool


class ShiftedSoftplus(nn.Module):
    def __init__(self):
        super().__init__()
        self.shift = math.log(2.0)

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.float32 and x.numel() % 4 == 0
                and x.data_ptr() % 16 == 0):
            return ops.shifted_softplus(x, self.shift)  # K14: one pass each way
        return F.softplus(x) - self.shift


class GaussianSmearing(nn.Module):
    def __init__(self, start=0.0, stop=5.0, num_gaussians=50):
        super().__init__()
        offset = torch.linspace(start, stop, num_gaussians)
        self.coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
        self.register_buffer("offset", offset)

    def forward(self, dist):
        dist = dist.view(-1, 1) - self.offset.view(1, -1)
        return torch.exp(self.coeff * torch.pow(dist, 2))


class CFConv(MessagePassing):
    def __init__(self, in_channels, out_channels, num_filters, nn_module, cutoff):
        super().__init__(aggr="add")
        self.lin1 = nn.Linear(in_channels, num_filters, bias=False)
        self.lin2 = nn.Linear(num_filters, out_channels)
        self.nn = nn_module
        self.cutoff = cutoff

    def forward(self, x, edge_index, edge_weight, edge_attr, edge_cut=None):
        """edge_cut: the cosine cutoff C of edge_weight when the caller already has it
        (SchNetModel computes it once per graph in the featurisation kernel)."""
        if edge_cut is None:
            C = 0.5 * (torch.cos(edge_weight * math.pi / self.cutoff) + 1.0)
        else:
            C = edge_cut
        W = self._filter(edge_attr)
        x = self.lin1(x)
        if ((ops.second_order_enabled() or not (C.requires_grad and torch.is_grad_enabled()))
                and self.fused_supported(x, W)):
            # K13 with the cutoff applied to W at load time: W * C is never materialised (inside
            # ops.second_order() also when C carries a gradient: dC is gmp_cfconv_cgrad_f32)
            x = ops.cfconv_propagate(edge_index, x, W, C)
        else:
            x = self.propagate(edge_index, x=x, W=W * C.view(-1, 1))
        return self.lin2(x)

    def _filter(self, edge_attr):
        """self.nn(edge_attr); the Linear -> act -> Linear filter network goes through
        ops.linear (same parameters, same arithmetic order per output element)."""
        m = self.nn
        if (isinstance(m, nn.Sequential) and len(m) == 3 and isinstance(m[0], nn.Linear)
                and isinstance(m[2], nn.Linear)):
            return ops.linear(m[1](ops.linear(edge_attr, m[0].weight, m[0].bias)),
                              m[2].weight, m[2].bias)
        return m(edge_attr)

    def fused_supported(self, x, W):
        return (x.is_cuda and x.dtype == torch.float32 and W.dtype == torch.float32
                and x.dim() == 2 and W.dim() == 2 and x.shape[1] % 4 == 0
                and W.shape[1] == x.shape[1])

    def fused_propagate(self, edge_index, x, W):
        """K13: message x_j * W and the sum at edge_index[1] in one pass over W."""
        return ops.cfconv_propagate(edge_index, x, W)

    def message(self, x_j, W):
        return x_j * W


class InteractionBlock(nn.Module):
    def __init__(self, hidden_channels, num_gaussians, num_filters, cutoff):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(num_gaussians, num_filters), ShiftedSoftplus(),
                                 nn.Linear(num_filters, num_filters))
        self.conv = CFConv(hidden_channels, hidden_channels, num_filters, self.mlp, cutoff)
        self.act = ShiftedSoftplus()
        self.lin = nn.Linear(hidden_channels, hidden_channels)

    def forward(self, x, edge_index, edge_weight, edge_attr, edge_cut=None):
        x = self.conv(x, edge_index, edge_weight, edge_attr, edge_cut)
        return self.lin(self.act(x))


class SchNetModel(nn.Module):
    """models/schnet.py:9-80 (+ PyG SchNet.__init__ internals)."""

    def __init__(self, hidden_channels=128, in_dim=1, out_dim=1, num_filters=128, num_layers=6,
                 num_gaussians=50, cutoff=10, max_num_neighbors=32, pool="sum"):
        super().__init__()
        self.hidden_channels, self.num_filters = hidden_channels, num_filters
        self.num_interactions, self.num_gaussians = num_layers, num_gaussians
        self.cutoff, self.max_num_neighbors = cutoff, max_num_neighbors
        self.embedding = nn.Embedding(100, hidden_channels, padding_idx=0)
        self.distance_expansion = GaussianSmearing(0.0, cutoff, num_gaussians)
        self.interactions = nn.ModuleList(
            InteractionBlock(hidden_channels, num_gaussians, num_filters, cutoff)
            for _ in range(num_layers))
        self.lin1 = nn.Linear(hidden_channels, hidden_channels // 2)
        self.act = ShiftedSoftplus()
        self.lin2 = nn.Linear(hidden_channels // 2, out_dim)
        self.pool = {"mean": global_mean_pool, "sum": global_add_pool}[pool]

    def forward(self, batch):
        w, pad = self.embedding.weight, self.embedding.padding_idx
        if pad is not None:  # nn.Embedding(padding_idx): that row receives no gradient
            w = torch.cat([w[:pad], w[pad:pad + 1].detach(), w[pad + 1:]], 0)
        h = ops.gather(w, batch.atoms, 0)
        # edge_weight, Gaussians and the cosine cutoff from one pass over the edges (K1,
        # gmp_schnet_featurize_f32); the cutoff is computed once and shared by every CFConv
        ds = self.distance_expansion
        feat = ops.SchNetFeaturize2Fn if ops.second_order_enabled() else ops.SchNetFeaturizeFn
        edge_weight, edge_attr, C = feat.apply(
            batch.pos, batch.edge_index, ds.offset, ds.coeff, self.cutoff, edge_shift(batch))
        if not all(isinstance(i.conv, CFConv) and i.conv.cutoff == self.cutoff
                   for i in self.interactions):
            C = None
        for interaction in self.interactions:
            h = h + interaction(h, batch.edge_index, edge_weight, edge_attr, C)
        out = self.pool(h, batch.batch, getattr(batch, "num_graphs", None))
        return self.lin2(self.act(self.lin1(out)))
