"""``optimize(model)``: the graph network on the fused filter convolution (mirror of reference
``torchmdnet/optimize.py``, whose ``TorchMD_GN_optimized`` runs NNPOps' CFConv).

The unoptimized ``TorchMD_GN`` evaluates each layer's filter network (``Linear(R, F)``, activation,
``Linear(F, F)``) as two GEMMs over all E edges and streams the E x F filter rows back into the convolution.
The optimized model forms the filter per edge inside the convolution kernel (``kernels.cfconv_fused``,
``tmdnet_cfconv_fused_*``): no E x F rows, and no E x R basis rows either unless the neighbour embedding needs
them.

Differences from the reference:
  * a superset of its configurations: any ``batch``, both bases (trainable or not, read live), the neighbour
    embedding, any ``cutoff_lower``, ``aggr`` add / mean, ``ssp`` / ``silu``;
  * refused with a ``ValueError`` naming the limit: ``aggr="max"``, precision 64 / 16, tanh / sigmoid,
    ``num_filters`` not a multiple of 16 in [16, 128], ``num_rbf`` outside [1, 64];
  * the fused op treats each block's filter network (``interactions[i].mlp``) and the basis parameters as
    CONSTANTS.  ``optimize`` therefore calls ``requires_grad_(False)`` on them: their ``.grad`` stays ``None``
    instead of being silently partial.  They are still read live on every call (nothing is cached: the weight
    image is rebuilt from the parameters per evaluation, inside the captured graph when captured);
  * optimized models are inference-only: energies and forces, eager or under ``GraphedEnergyForces``.  A second
    derivative through the forces (a force loss, ``LNNPStep``) raises a ``RuntimeError``; TorchScript is
    refused as for the unoptimized graph network.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import kernels
from .models.model import TorchMD_Net
from .models.torchmd_gn import _SCRIPT_ERROR, TorchMD_GN, _linear, _linear_act

__all__ = ["optimize", "TorchMD_GN_optimized"]


def _refusal(model):
    """Why ``model`` (a TorchMD_GN) cannot run on the fused convolution, or None."""
    dtype = model.embedding.weight.dtype
    if dtype != torch.float32:
        return f"float32 (precision 32) only, this model stores {dtype}"
    if model.aggr not in ("add", "mean"):
        return f'aggr="{model.aggr}" is not supported (the fused convolution aggregates with "add" or "mean")'
    if model.activation not in ("ssp", "silu"):
        return f'activation="{model.activation}" is not supported ("ssp" or "silu")'
    return kernels.cfconv_fused_limits(model.num_filters, model.num_rbf)


class TorchMD_GN_optimized(nn.Module):
    """Equivalent to ``TorchMD_GN`` (kept as ``self.model``, so ``state_dict`` keys gain a ``model.`` level as in
    the reference) with every interaction block's filter network fused into its convolution kernel."""

    def __init__(self, model):
        if not isinstance(model, TorchMD_GN):
            raise ValueError("Unsupported model! Only TorchMD_GN is supported.")
        why = _refusal(model)
        if why is not None:
            raise ValueError("optimize: " + why)
        super().__init__()
        self.model = model
        # constants of the fused op: no (partial) gradients
        for inter in model.interactions:
            inter.mlp.requires_grad_(False)
        model.distance_expansion.requires_grad_(False)

    @property
    def distance(self):
        """The wrapped network's neighbour list (GraphedEnergyForces sizes and checks its capacity)."""
        return self.model.distance

    def reset_parameters(self):
        self.model.reset_parameters()

    def __prepare_scriptable__(self):
        raise RuntimeError(_SCRIPT_ERROR)

    def forward(self, z: Tensor, pos: Tensor, batch: Tensor, s: Optional[Tensor] = None,
                q: Optional[Tensor] = None, box: Optional[Tensor] = None
                ) -> Tuple[Tensor, Optional[Tensor], Tensor, Tensor, Tensor]:
        if torch.jit.is_scripting():
            raise RuntimeError(_SCRIPT_ERROR)
        m = self.model
        x = m.embedding(z)
        graph = m.distance.graph(pos, batch) if box is None else m.distance.graph(pos, batch, box)
        de = m.distance_expansion
        rbf_params = de.kernel_params()
        # the E x R basis rows only for the neighbour embedding
        want_rbf = m.neighbor_embedding is not None
        edge_attr, C, _ = kernels.edge_geometry(graph, *rbf_params, m.cutoff_lower, m.cutoff_upper, de.rbf_type,
                                                want=(want_rbf, True, False))
        graph.cutoff = C
        if want_rbf:
            x = m.neighbor_embedding(z, x, graph, graph.distances, edge_attr, cutoff=C)
        if len(m.interactions) == 0:
            return x, None, z, pos, batch
        # every layer's weight image from the live parameters, one launch
        images, _, _ = kernels.cfconv_fused_image([inter.mlp for inter in m.interactions])
        for i, inter in enumerate(m.interactions):
            conv = inter.conv
            y = _linear(conv.lin1, x)
            y = kernels.cfconv_fused(y, graph.distances, C, graph, inter.mlp[0].weight, inter.mlp[0].bias,
                                     inter.mlp[2].weight, inter.mlp[2].bias, rbf_params, m.cutoff_lower,
                                     m.cutoff_upper, de.rbf_type, kernels.act_code(inter.mlp[1]), m.aggr,
                                     image=images[i])
            y = _linear_act(conv.lin2, inter.act, y)
            x = x + _linear(inter.lin, y)
        return x, None, z, pos, batch

    def __repr__(self):
        return "Optimized: " + repr(self.model)


def optimize(model):
    """Replaces ``model.representation_model`` (a ``TorchMD_GN``) in place by ``TorchMD_GN_optimized`` and
    returns ``model``.  Raises ``ValueError`` for any other model or an unsupported configuration.  Freezes
    (``requires_grad_(False)``) the parameters the fused op treats as constants: every block's ``mlp`` and the
    basis."""
    assert isinstance(model, TorchMD_Net)
    rep = model.representation_model
    if not isinstance(rep, TorchMD_GN):
        raise ValueError("Unsupported model! Only TorchMD_GN is supported.")
    if getattr(model, "_half_storage", False):
        raise ValueError("optimize: float32 (precision 32) only, this model stores torch.float16")
    model.representation_model = TorchMD_GN_optimized(rep)
    return model
