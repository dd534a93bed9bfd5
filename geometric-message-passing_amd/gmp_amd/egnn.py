"""EGNN layer / model on the MI355X fused kernels — drop-in for the reference's
models/layers/egnn_layer.py:7-89 (EGNNLayer) and models/egnn.py:9-87 (EGNNModel).

Same constructor arguments, module tree and state_dict keys (mlp_msg.{0,1,3,4},
mlp_pos.{0,1,3}, mlp_upd.{0,1,3,4}, emb_in, pred.*), same forward signatures.

The message + aggregation of every layer runs in one fused HIP kernel (K4,
gmp_egnn_edge_fwd_f32 / _bwd_f32) when the configuration is supported (LayerNorm, relu/swish,
sum/add/mean, emb_dim in {32, 64, 128}); otherwise propagate() takes the generic
gather -> message -> segmented-reduce path.  Node-level MLPs (mlp_upd, embeddings, readout) are
small (N rows) and use the PyTorch GEMMs.

Reference quirk preserved/documented: the reference's aggregate omits dim_size
(egnn_layer.py:77,79) so it only works when max(edge_index[1]) == N-1; the fused path always
produces N rows (identical whenever the reference runs).
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .message_passing import MessagePassing
from .scatter import scatter, global_add_pool, global_mean_pool


class EGNNLayer(MessagePassing):
    def __init__(self, emb_dim, activation="relu", norm="layer", aggr="add"):
        super().__init__(aggr=aggr)
        self.emb_dim = emb_dim
        self.activation_name = activation
        self.norm_name = norm
        self.activation = {"swish": nn.SiLU(), "relu": nn.ReLU()}[activation]
        self.norm = {"layer": nn.LayerNorm, "batch": nn.BatchNorm1d}[norm]
        d = emb_dim
        self.mlp_msg = nn.Sequential(nn.Linear(2 * d + 1, d), self.norm(d), self.activation,
                                     nn.Linear(d, d), self.norm(d), self.activation)
        self.mlp_pos = nn.Sequential(nn.Linear(d, d), self.norm(d), self.activation,
                                     nn.Linear(d, 1))
        self.mlp_upd = nn.Sequential(nn.Linear(2 * d, d), self.norm(d), self.activation,
                                     nn.Linear(d, d), self.norm(d), self.activation)

    def forward(self, h, pos, edge_index):
        return self.propagate(edge_index, h=h, pos=pos)

    # ---------------------------------------------------------------- generic (reference) hooks
    def message(self, h_i, h_j, pos_i, pos_j):
        pos_diff = pos_i - pos_j
        dists = torch.norm(pos_diff, dim=-1).unsqueeze(1)
        msg = self.mlp_msg(torch.cat([h_i, h_j, dists], dim=-1))
        return msg, pos_diff * self.mlp_pos(msg)

    def aggregate(self, inputs, index):
        msgs, pos_diffs = inputs
        reduce = "sum" if self.aggr in ("add", "sum") else self.aggr
        return (scatter(msgs, index, dim=self.node_dim, reduce=reduce),
                scatter(pos_diffs, index, dim=self.node_dim, reduce="mean"))

    def update(self, aggr_out, h, pos):
        msg_aggr, pos_aggr = aggr_out
        return self.mlp_upd(torch.cat([h, msg_aggr], dim=-1)), pos + pos_aggr

    # ---------------------------------------------------------------- fused path (K4)
    def fused_supported(self, h, pos):
        lns = (self.mlp_msg[1], self.mlp_msg[4], self.mlp_pos[1])
        return (self.norm_name == "layer" and self.emb_dim in (32, 64, 128)
                and self.aggr in ("add", "sum", "mean") and h.is_cuda
                and h.dtype == torch.float32 and pos.dtype == torch.float32
                and all(ln.elementwise_affine and ln.eps == lns[0].eps for ln in lns))

    def fused_message(self, edge_index, h, pos, AB=None, need_pos=True):
        """(m_aggr, pos_aggr) of the fused message block (K4); AB: the node projections when the
        previous layer's K15 update produced them.  need_pos=False: the caller drops the position
        output — (m_aggr, None), and the kernels leave the mlp_pos branch out."""
        graph = ops.egnn_graph(edge_index, h.shape[0])
        m0, ln1, m3, ln2 = self.mlp_msg[0], self.mlp_msg[1], self.mlp_msg[3], self.mlp_msg[4]
        p0, ln3, p3 = self.mlp_pos[0], self.mlp_pos[1], self.mlp_pos[3]
        return ops.EgnnMessageFn.apply(
            h, pos, graph, self.activation_name, self.aggr == "mean", ln1.eps,
            m0.weight, m0.bias, ln1.weight, ln1.bias, m3.weight, m3.bias, ln2.weight, ln2.bias,
            p0.weight, p0.bias, ln3.weight, ln3.bias, p3.weight, p3.bias, torch.is_grad_enabled(),
            AB, need_pos)

    def fused_propagate(self, edge_index, h, pos):
        m_aggr, p_aggr = self.fused_message(edge_index, h, pos)
        return self._mlp_upd(h, m_aggr), pos + p_aggr

    def node_fusable(self):
        """K15 applies: LayerNorm update MLP with affine norms (the fused message already
        requires LayerNorm and emb_dim in {32, 64, 128})."""
        n1, n4 = self.mlp_upd[1], self.mlp_upd[4]
        return (self.norm_name == "layer" and n1.elementwise_affine and n4.elementwise_affine
                and n1.eps == n4.eps)

    def fused_update(self, h, m_aggr, next_layer=None, residual=True, image=None):
        """(h', AB') = K15: h' = h + mlp_upd([h | m_aggr]) (or the update alone without residual)
        and the next layer's node projections (None when next_layer is None).  image: this
        layer's row of ops.egnn_node_images (built here when not given)."""
        l0, n1, l3, n4 = self.mlp_upd[0], self.mlp_upd[1], self.mlp_upd[3], self.mlp_upd[4]
        if image is None:
            image = ops.egnn_node_images([self], [next_layer])[0]
        return ops.EgnnNodeFn.apply(h, m_aggr, l0.weight, l0.bias, n1.weight, n1.bias, l3.weight,
                                    l3.bias, n4.weight, n4.bias, image, next_layer is not None,
                                    self.activation_name, residual, n1.eps,
                                    torch.is_grad_enabled())

    def _mlp_upd(self, h, m_aggr):
        """mlp_upd(cat([h, m_aggr])) (egnn_layer.py:37-39, :84) with the first Linear split over
        the two inputs (no concatenation) and the Linears through ops (node rows: weight
        gradients by the deterministic outer sum, deferred to the side stream)."""
        l0, n1, l3, n4 = self.mlp_upd[0], self.mlp_upd[1], self.mlp_upd[3], self.mlp_upd[4]
        x = ops.split_linear(h, m_aggr, l0.weight, l0.bias)
        if self.norm_name == "layer" and n1.elementwise_affine and n4.elementwise_affine:
            # LayerNorm + activation fused (K12)
            x = ops.ln_act(x, n1, self.activation_name)
            return ops.ln_act(ops.linear(x, l3.weight, l3.bias), n4, self.activation_name)
        x = self.activation(n1(x))
        return self.activation(n4(ops.linear(x, l3.weight, l3.bias)))

    def __repr__(self):
        return f"{self.__class__.__name__}(emb_dim={self.emb_dim}, aggr={self.aggr})"


class EGNNModel(nn.Module):
    """models/egnn.py:9-87 (same kwargs and defaults)."""

    def __init__(self, num_layers=5, emb_dim=128, in_dim=1, out_dim=1, activation="relu",
                 norm="layer", aggr="sum", pool="sum", residual=True, equivariant_pred=False):
        super().__init__()
        self.equivariant_pred = equivariant_pred
        self.residual = residual
        self.emb_in = nn.Embedding(in_dim, emb_dim)
        self.convs = nn.ModuleList(EGNNLayer(emb_dim, activation, norm, aggr)
                                   for _ in range(num_layers))
        self.pool = {"mean": global_mean_pool, "sum": global_add_pool}[pool]
        if equivariant_pred:
            self.pred = nn.Linear(emb_dim + 3, out_dim)
        else:
            self.pred = nn.Sequential(nn.Linear(emb_dim, emb_dim), nn.ReLU(),
                                      nn.Linear(emb_dim, out_dim))

    def _layers_fused(self, h, pos):
        return (len(self.convs) > 0 and all(c.fused_supported(h, pos) and c.node_fusable()
                                            for c in self.convs)
                and not ops.compiling() and not ops.egnn_exact_mode())

    def forward(self, batch):
        if getattr(batch, "edge_shift_idx", None) is not None:
            raise NotImplementedError(
                "EGNNModel takes no periodic images (batch.edge_shift_idx): its edge geometry "
                "is computed inside the fused kernels")
        h = ops.gather(self.emb_in.weight, batch.atoms)  # == emb_in(atoms); bwd = segmented sum
        pos = batch.pos
        if self._layers_fused(h, pos):
            # per layer: K4 message block, then K15 (update + residual + the next layer's AB)
            convs = list(self.convs)
            nexts = convs[1:] + [None]
            images = ops.egnn_node_images(convs, nexts)  # one launch for every layer
            # the first layer's node projections: the embedding table projected once (in_dim
            # rows), then gathered — AB0 = emb[atoms] [W1a | W1b]^T without an (N, d) GEMM
            with torch.no_grad():
                W1 = convs[0].mlp_msg[0].weight
                d = h.shape[1]
                table = self.emb_in.weight.mm(torch.cat([W1[:, :d], W1[:, d:2 * d]], 0).t())
                AB = ops.gather_rows(table, batch.atoms)
            for k, conv in enumerate(convs):
                # the last layer's positions are read only by the equivariant readout
                need_pos = self.equivariant_pred or nexts[k] is not None
                m_aggr, p_aggr = conv.fused_message(batch.edge_index, h, pos, AB, need_pos)
                h, AB = conv.fused_update(h, m_aggr, nexts[k], self.residual, images[k])
                if need_pos:
                    pos = pos + p_aggr
        else:
            for conv in self.convs:
                h_update, pos = conv(h, pos, batch.edge_index)
                h = h + h_update if self.residual else h_update
        feats = torch.cat([h, pos], dim=-1) if self.equivariant_pred else h
        out = self.pool(feats, batch.batch, getattr(batch, "num_graphs", None))
        return self.pred(out)
