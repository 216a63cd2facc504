"""Invariant Transformer (mirror of reference ``torchmdnet/models/torchmd_t.py``).

Same constructor arguments, attribute names, module tree and creation / reset order as the reference
(torchmd_t.py:53-142, 185-244), so ``torch.manual_seed`` reproduces reference weights and reference
checkpoints load with ``strict=True``.  The per-edge work runs in HIP kernels:
  * neighbour list: CSR EdgeGraph from ``tmdnet_nl_build`` with self loops (kept at distance 0, as the
    reference ``Distance(loop=True)`` keeps them);
  * RBF + cosine cutoff: the fused ``tmdnet_edge_geom_*`` kernel, computed once and shared by every layer;
  * message + aggregation: ``kernels.t_message``, the scalar form of the ET message entry points -- the dk / dv
    rows are handed over BEFORE their activation, which the kernel applies, as it applies the attention
    activation and the cutoff.
LayerNorm, the node Linears and the dk / dv projection run on the package's ``layer_norm`` / ``linear`` paths.
The model runs eagerly (and under HIP-graph capture); TorchScript is refused.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .. import kernels
from .torchmd_gn import _linear
from .utils import CosineCutoff, NeighborEmbedding, OptimizedDistance, act_class_mapping, as_graph, rbf_class_mapping

_SCRIPT_ERROR = ("torchmd-net_amd: the Transformer model runs eagerly (its message kernel has no scripted "
                 "operator); call the eager module or capture it with GraphedEnergyForces")


class TorchMD_T(nn.Module):
    r"""The TorchMD Transformer architecture (reference torchmd_t.py:14-182)."""

    def __init__(self, hidden_channels=128, num_layers=6, num_rbf=50, rbf_type="expnorm", trainable_rbf=True,
                 activation="silu", attn_activation="silu", neighbor_embedding=True, num_heads=8,
                 distance_influence="both", cutoff_lower=0.0, cutoff_upper=5.0, max_z=100, max_num_neighbors=32,
                 dtype=torch.float):
        super().__init__()
        assert distance_influence in ["keys", "values", "both", "none"]
        assert rbf_type in rbf_class_mapping, (
            f'Unknown RBF type "{rbf_type}". Choose from {", ".join(rbf_class_mapping.keys())}.')
        assert activation in act_class_mapping, (
            f'Unknown activation function "{activation}". Choose from {", ".join(act_class_mapping.keys())}.')

        self.hidden_channels = hidden_channels
        self.num_layers = num_layers
        self.num_rbf = num_rbf
        self.rbf_type = rbf_type
        self.trainable_rbf = trainable_rbf
        self.activation = activation
        self.attn_activation = attn_activation
        self.neighbor_embedding = neighbor_embedding
        self.num_heads = num_heads
        self.distance_influence = distance_influence
        self.cutoff_lower = cutoff_lower
        self.cutoff_upper = cutoff_upper
        self.max_z = max_z

        act_class = act_class_mapping[activation]
        attn_act_class = act_class_mapping[attn_activation]

        self.embedding = nn.Embedding(self.max_z, hidden_channels, dtype=dtype)
        # the reference's Distance(loop=True) on the native list; more than max_num_neighbors * N pairs is an error
        self.distance = OptimizedDistance(cutoff_lower, cutoff_upper, max_num_pairs=-max_num_neighbors, loop=True,
                                          return_vecs=False)
        self.distance_expansion = rbf_class_mapping[rbf_type](cutoff_lower, cutoff_upper, num_rbf, trainable_rbf,
                                                              dtype=dtype)
        self.neighbor_embedding = (
            NeighborEmbedding(hidden_channels, num_rbf, cutoff_lower, cutoff_upper, self.max_z, dtype=dtype).jittable()
            if neighbor_embedding else None)

        self.attention_layers = nn.ModuleList()
        for _ in range(num_layers):
            layer = MultiHeadAttention(hidden_channels, num_rbf, distance_influence, num_heads, act_class,
                                       attn_act_class, cutoff_lower, cutoff_upper, dtype=dtype).jittable()
            self.attention_layers.append(layer)

        self.out_norm = nn.LayerNorm(hidden_channels, dtype=dtype)

        self.reset_parameters()

    def reset_parameters(self):
        self.embedding.reset_parameters()
        self.distance_expansion.reset_parameters()
        if self.neighbor_embedding is not None:
            self.neighbor_embedding.reset_parameters()
        for attn in self.attention_layers:
            attn.reset_parameters()
        self.out_norm.reset_parameters()

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
        for attn in self.attention_layers:
            x = x + attn(x, graph, graph.distances, edge_attr)
        on = self.out_norm
        x = kernels.layer_norm(x, on.weight, on.bias, on.eps)
        return x, None, z, pos, batch

    def __repr__(self):
        return (f"{self.__class__.__name__}(hidden_channels={self.hidden_channels}, "
                f"num_layers={self.num_layers}, num_rbf={self.num_rbf}, rbf_type={self.rbf_type}, "
                f"trainable_rbf={self.trainable_rbf}, activation={self.activation}, "
                f"attn_activation={self.attn_activation}, neighbor_embedding={self.neighbor_embedding}, "
                f"num_heads={self.num_heads}, distance_influence={self.distance_influence}, "
                f"cutoff_lower={self.cutoff_lower}, cutoff_upper={self.cutoff_upper})")


class MultiHeadAttention(nn.Module):
    """Reference torchmd_t.py:185-283 (a torch_geometric MessagePassing there).  ``edge_index`` may be a (2, E)
    tensor (any symmetric edge list) or the model's CSR EdgeGraph (fast path)."""

    def __init__(self, hidden_channels, num_rbf, distance_influence, num_heads, activation, attn_activation,
                 cutoff_lower, cutoff_upper, dtype=torch.float):
        super().__init__()
        assert hidden_channels % num_heads == 0, (
            f"The number of hidden channels ({hidden_channels}) must be evenly divisible by the number of "
            f"attention heads ({num_heads})")

        self.distance_influence = distance_influence
        self.num_heads = num_heads
        self.head_dim = hidden_channels // num_heads

        self.layernorm = nn.LayerNorm(hidden_channels, dtype=dtype)
        self.act = activation()
        self.attn_activation = attn_activation()
        self.cutoff = CosineCutoff(cutoff_lower, cutoff_upper)

        self.q_proj = nn.Linear(hidden_channels, hidden_channels, dtype=dtype)
        self.k_proj = nn.Linear(hidden_channels, hidden_channels, dtype=dtype)
        self.v_proj = nn.Linear(hidden_channels, hidden_channels, dtype=dtype)
        self.o_proj = nn.Linear(hidden_channels, hidden_channels, dtype=dtype)

        self.dk_proj = None
        if distance_influence in ["keys", "both"]:
            self.dk_proj = nn.Linear(num_rbf, hidden_channels, dtype=dtype)

        self.dv_proj = None
        if distance_influence in ["values", "both"]:
            self.dv_proj = nn.Linear(num_rbf, hidden_channels, dtype=dtype)

        self.reset_parameters()

    def jittable(self):
        return self

    def __prepare_scriptable__(self):
        raise RuntimeError(_SCRIPT_ERROR)

    def reset_parameters(self):
        self.layernorm.reset_parameters()
        nn.init.xavier_uniform_(self.q_proj.weight)
        self.q_proj.bias.data.fill_(0)
        nn.init.xavier_uniform_(self.k_proj.weight)
        self.k_proj.bias.data.fill_(0)
        nn.init.xavier_uniform_(self.v_proj.weight)
        self.v_proj.bias.data.fill_(0)
        nn.init.xavier_uniform_(self.o_proj.weight)
        self.o_proj.bias.data.fill_(0)
        if self.dk_proj:
            nn.init.xavier_uniform_(self.dk_proj.weight)
            self.dk_proj.bias.data.fill_(0)
        if self.dv_proj:
            nn.init.xavier_uniform_(self.dv_proj.weight)
            self.dv_proj.bias.data.fill_(0)

    def forward(self, x, edge_index, r_ij, f_ij):
        if torch.jit.is_scripting():
            raise RuntimeError(_SCRIPT_ERROR)
        # both activations as the edge kernels' codes (SiLU / ShiftedSoftplus / Tanh / Sigmoid)
        acts = kernels.et_act_flags(kernels.act_code(self.act), kernels.act_code(self.attn_activation))
        graph, perm = as_graph(edge_index, x.shape[0])
        if perm is not None:
            r_ij, f_ij = r_ij[perm], f_ij[perm]
        C = graph.cutoff if (perm is None and graph.cutoff is not None) else self.cutoff(r_ij)
        H = self.num_heads * self.head_dim
        ln = self.layernorm
        x = kernels.layer_norm(x, ln.weight, ln.bias, ln.eps)
        q = _linear(self.q_proj, x)
        k = _linear(self.k_proj, x)
        v = _linear(self.v_proj, x)
        # the dk / dv rows BEFORE their activation (the message kernel applies it); with both present, one GEMM
        # into one [E, 2H] buffer whose column blocks the kernel reads in place
        pk = pv = None
        if self.dk_proj is not None and self.dv_proj is not None:
            w = torch.cat([self.dk_proj.weight, self.dv_proj.weight], 0)
            b = torch.cat([self.dk_proj.bias, self.dv_proj.bias], 0)
            pkv = kernels.linear(f_ij, w, b) if f_ij.is_cuda else torch.nn.functional.linear(f_ij, w, b)
            pk, pv = pkv[:, :H], pkv[:, H:]
        elif self.dk_proj is not None:
            pk = _linear(self.dk_proj, f_ij)
        elif self.dv_proj is not None:
            pv = _linear(self.dv_proj, f_ij)
        out = kernels.t_message(q, k, v, pk, pv, C, graph, self.num_heads, acts)
        return _linear(self.o_proj, out)
