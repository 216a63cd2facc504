"""Graph network (mirror of reference ``torchmdnet/models/torchmd_gn.py``, the SchNet-style model).

Same constructor arguments, attribute names, module tree and creation / reset order as the reference
(torchmd_gn.py:60-138, 187-259), so ``create_model`` + ``torch.manual_seed`` reproduce reference weights and
reference checkpoints load.  The per-edge work runs in HIP kernels:
  * neighbour list: CSR EdgeGraph from ``tmdnet_nl_build`` (no self loops, pairs below the lower cutoff
    dropped, as the reference ``Distance`` does);
  * RBF + cosine cutoff: the fused ``tmdnet_edge_geom_*`` kernel, computed once and shared by every layer
    (all layers use the same CosineCutoff(cl, cu));
  * message + aggregation (add / mean / max): ``tmdnet_cfconv_*`` -- the filter network's output is used as
    is, the cutoff multiply happens inside the kernel (no E x F elementwise launch).
The filter network and the node Linears are GEMMs on the package's ``linear`` / ``mlp_act`` paths.  The model
runs eagerly (and under HIP-graph capture); TorchScript is refused.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .. import kernels
from .utils import CosineCutoff, NeighborEmbedding, OptimizedDistance, act_class_mapping, as_graph, rbf_class_mapping

_SCRIPT_ERROR = ("torchmd-net_amd: the graph-network model runs eagerly (its continuous-filter convolution has "
                 "no scripted operator); call the eager module or capture it with GraphedEnergyForces")


def _linear(mod, x):
    """nn.Linear on the hand-written GEMM path (weight gradients as TN GEMMs, also in the second order)."""
    return kernels.linear(x, mod.weight, mod.bias) if x.is_cuda else mod(x)


def _linear_act(mod, act, x):
    """act(Linear(x)): the activation in the GEMM's epilogue where the fused path takes the shape."""
    if x.is_cuda:
        return kernels.mlp_act(x, [mod.weight], [mod.bias], act)
    return act(mod(x))


class TorchMD_GN(nn.Module):
    r"""The TorchMD Graph Network architecture (reference torchmd_gn.py:14-184)."""

    def __init__(self, hidden_channels=128, num_filters=128, num_layers=6, num_rbf=50, rbf_type="expnorm",
                 trainable_rbf=True, activation="silu", neighbor_embedding=True, cutoff_lower=0.0,
                 cutoff_upper=5.0, max_z=100, max_num_neighbors=32, aggr="add", dtype=torch.float32):
        super().__init__()
        assert rbf_type in rbf_class_mapping, (
            f'Unknown RBF type "{rbf_type}". Choose from {", ".join(rbf_class_mapping.keys())}.')
        assert activation in act_class_mapping, (
            f'Unknown activation function "{activation}". Choose from {", ".join(act_class_mapping.keys())}.')
        assert aggr in ["add", "mean", "max"], 'Argument aggr must be one of: "add", "mean", or "max"'

        self.hidden_channels = hidden_channels
        self.num_filters = num_filters
        self.num_layers = num_layers
        self.num_rbf = num_rbf
        self.rbf_type = rbf_type
        self.trainable_rbf = trainable_rbf
        self.activation = activation
        self.neighbor_embedding = neighbor_embedding
        self.cutoff_lower = cutoff_lower
        self.cutoff_upper = cutoff_upper
        self.max_z = max_z
        self.aggr = aggr

        act_class = act_class_mapping[activation]

        self.embedding = nn.Embedding(self.max_z, hidden_channels, dtype=dtype)
        # the reference's Distance (radius_graph, no self loops, r >= cutoff_lower) on the native list; more
        # than max_num_neighbors * N pairs is an error
        self.distance = OptimizedDistance(cutoff_lower, cutoff_upper, max_num_pairs=-max_num_neighbors,
                                          loop=False, return_vecs=False)
        self.distance_expansion = rbf_class_mapping[rbf_type](cutoff_lower, cutoff_upper, num_rbf, trainable_rbf,
                                                              dtype=dtype)
        self.neighbor_embedding = (
            NeighborEmbedding(hidden_channels, num_rbf, cutoff_lower, cutoff_upper, self.max_z, dtype=dtype).jittable()
            if neighbor_embedding else None)

        self.interactions = nn.ModuleList()
        for _ in range(num_layers):
            block = InteractionBlock(hidden_channels, num_rbf, num_filters, act_class, cutoff_lower, cutoff_upper,
                                     aggr=self.aggr, dtype=dtype)
            self.interactions.append(block)

        self.reset_parameters()

    def reset_parameters(self):
        self.embedding.reset_parameters()
        self.distance_expansion.reset_parameters()
        if self.neighbor_embedding is not None:
            self.neighbor_embedding.reset_parameters()
        for interaction in self.interactions:
            interaction.reset_parameters()

    def __prepare_scriptable__(self):
        raise RuntimeError(_SCRIPT_ERROR)

    def forward(self, z: Tensor, pos: Tensor, batch: Tensor, s: Optional[Tensor] = None,
                q: Optional[Tensor] = None, box: Optional[Tensor] = None
                ) -> Tuple[Tensor, Optional[Tensor], Tensor, Tensor, Tensor]:
        """``box``: this call's periodic box, ``(3, 3)`` or one per molecule ``(n_molecules, 3, 3)``, handed to
        ``self.distance.graph`` (``None``: the distance module's own box)."""
        if torch.jit.is_scripting():
            raise RuntimeError(_SCRIPT_ERROR)
        x = self.embedding(z)
        graph = self.distance.graph(pos, batch) if box is None else self.distance.graph(pos, batch, box)
        de = self.distance_expansion
        if self.trainable_rbf and torch.is_grad_enabled():
            # trainable basis: parameters need gradients -> differentiable torch basis on the GPU
            edge_attr = de(graph.distances)
            _, C, _ = kernels.edge_geometry(graph, *de.kernel_params(), self.cutoff_lower, self.cutoff_upper,
                                            de.rbf_type, want=(False, True, False))
        else:
            edge_attr, C, _ = kernels.edge_geometry(graph, *de.kernel_params(), self.cutoff_lower,
                                                    self.cutoff_upper, de.rbf_type, want=(True, True, False))
        graph.cutoff = C
        if self.neighbor_embedding is not None:
            x = self.neighbor_embedding(z, x, graph, graph.distances, edge_attr, cutoff=C)
        for interaction in self.interactions:
            x = x + interaction(x, graph, graph.distances, edge_attr)
        return x, None, z, pos, batch

    def __repr__(self):
        return (f"{self.__class__.__name__}(hidden_channels={self.hidden_channels}, "
                f"num_filters={self.num_filters}, num_layers={self.num_layers}, num_rbf={self.num_rbf}, "
                f"rbf_type={self.rbf_type}, trainable_rbf={self.trainable_rbf}, activation={self.activation}, "
                f"neighbor_embedding={self.neighbor_embedding}, cutoff_lower={self.cutoff_lower}, "
                f"cutoff_upper={self.cutoff_upper}, aggr={self.aggr})")


class InteractionBlock(nn.Module):
    """Reference torchmd_gn.py:187-233."""

    def __init__(self, hidden_channels, num_rbf, num_filters, activation, cutoff_lower, cutoff_upper, aggr="add",
                 dtype=torch.float32):
        super().__init__()
        self.mlp = nn.Sequential(
            nn.Linear(num_rbf, num_filters, dtype=dtype),
            activation(),
            nn.Linear(num_filters, num_filters, dtype=dtype),
        )
        self.conv = CFConv(hidden_channels, hidden_channels, num_filters, self.mlp, cutoff_lower, cutoff_upper,
                           aggr=aggr, dtype=dtype).jittable()
        self.act = activation()
        self.lin = nn.Linear(hidden_channels, hidden_channels, dtype=dtype)

        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.mlp[0].weight)
        self.mlp[0].bias.data.fill_(0)
        nn.init.xavier_uniform_(self.mlp[2].weight)
        self.mlp[2].bias.data.fill_(0)
        self.conv.reset_parameters()
        nn.init.xavier_uniform_(self.lin.weight)
        self.lin.bias.data.fill_(0)

    def forward(self, x, edge_index, edge_weight, edge_attr):
        # conv's lin2 -> act -> lin: lin2 and the activation as one launch where the fused path applies
        x = self.conv(x, edge_index, edge_weight, edge_attr, act=self.act)
        return _linear(self.lin, x)


class CFConv(nn.Module):
    """Reference torchmd_gn.py:236-272 (a torch_geometric MessagePassing there).  ``edge_index`` may be a
    (2, E) tensor (any symmetric edge list) or the model's CSR EdgeGraph (fast path)."""

    def __init__(self, in_channels, out_channels, num_filters, net, cutoff_lower, cutoff_upper, aggr="add",
                 dtype=torch.float32):
        super().__init__()
        assert aggr in ["add", "mean", "max"], 'Argument aggr must be one of: "add", "mean", or "max"'
        self.aggr = aggr
        self.lin1 = nn.Linear(in_channels, num_filters, bias=False, dtype=dtype)
        self.lin2 = nn.Linear(num_filters, out_channels, bias=True, dtype=dtype)
        self.net = net
        self.cutoff = CosineCutoff(cutoff_lower, cutoff_upper)

        self.reset_parameters()

    def jittable(self):
        return self

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin1.weight)
        nn.init.xavier_uniform_(self.lin2.weight)
        self.lin2.bias.data.fill_(0)

    def forward(self, x, edge_index, edge_weight, edge_attr, act=None):
        """``act``: an activation applied to the output (InteractionBlock's, fused behind lin2)."""
        if torch.jit.is_scripting():
            raise RuntimeError(_SCRIPT_ERROR)
        graph, perm = as_graph(edge_index, x.shape[0])
        if perm is not None:
            edge_weight, edge_attr = edge_weight[perm], edge_attr[perm]
        C = graph.cutoff if (perm is None and graph.cutoff is not None) else self.cutoff(edge_weight)
        # the filter rows BEFORE the cutoff: the convolution kernel multiplies by C
        W = _linear(self.net[2], _linear_act(self.net[0], self.net[1], edge_attr))
        x = _linear(self.lin1, x)
        x = kernels.cfconv(x, W, C, graph, self.aggr)
        if act is None:
            return _linear(self.lin2, x)
        return _linear_act(self.lin2, act, x)
