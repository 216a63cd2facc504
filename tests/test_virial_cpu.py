"""CPU tests of the virial: the strain convention of the yardstick (tests/virial_ref.py) against finite
differences of the untouched fp64 oracle, the plain-torch composite against the two lines of the definition
(include/tmdnet.h, tmdnet_nl_backward_virial), and what ``energy_forces_virial`` refuses."""
import itertools

import pytest
import torch

import virial_ref as VR
from conftest import yaml_args
from torchmdnet.kernels import nl_backward_virial_composite


# ----------------------------------------------------------------------------- strain convention
@pytest.mark.parametrize("name", ["et_tiny_periodic_f64", "tn_tiny_periodic_dyn_f64"])
def test_strain_derivative_matches_finite_differences(name):
    """virial = -dE/d eps for pos -> pos (I + eps)^T, box -> box (I + eps)^T: central differences (h = 1e-5, all
    nine entries) of the untouched oracle.  Gate 1e-8 of the largest entry: the truncation + rounding error of
    the difference quotient measured on these fixtures is 1.4e-10 and 1.8e-10, a sign or
    index mix-up is O(1).  The static-shapes fixture is not used here: with padding, a pair crossing the cutoff
    changes the padded energy discontinuously."""
    sd, cfg, z, pos, batch, static = VR.fixture_case(name)
    _, _, W = VR.fixture_virial(name)
    assert W.shape == (1, 3, 3)
    box = torch.as_tensor(cfg["box"], dtype=torch.float64)
    h = 1e-5
    fd = torch.zeros(3, 3, dtype=torch.float64)
    for a, b in itertools.product(range(3), range(3)):
        e = []
        for sgn in (1.0, -1.0):
            m = torch.eye(3, dtype=torch.float64)
            m[a, b] += sgn * h
            c = dict(cfg)
            c["box"] = (box @ m.T).numpy()
            e.append(VR.oracle_energy(sd, c, z, pos @ m.T, batch, static_shapes=static).sum())
        fd[a, b] = (e[0] - e[1]) / (2 * h)
    err = float((W[0] + fd).abs().max() / W.abs().max())
    print(f"{name}: max |W + dE/d eps (FD)| / max|W| = {err:.3e}")
    assert err < 1e-8, err


# ----------------------------------------------------------------------------- composite vs definition
def _hand_list():
    """Eight directed edges over five atoms, symmetric: self loops 0->0 and 2->2 (r = 0), the pairs 0-1, 1-2
    (across the two molecules) and 2-3; atom 4 has no edge.  Destination-grouped, as the CSR build."""
    src = torch.tensor([0, 1, 0, 2, 1, 2, 3, 2], dtype=torch.int32)
    dst = torch.tensor([0, 0, 1, 1, 2, 2, 2, 3], dtype=torch.int32)
    batch = torch.tensor([0, 0, 1, 1, 1])
    g = torch.Generator().manual_seed(7)
    pos = torch.randn(5, 3, generator=g, dtype=torch.float64)
    dl = pos[src.long()] - pos[dst.long()]
    r = dl.norm(dim=1)
    assert int((r == 0).sum()) == 2
    return src, dst, batch, dl, r, g


@pytest.mark.parametrize("has", list(itertools.product([True, False], repeat=3)))
def test_composite_is_the_definition(has):
    """out[m][a][b] = sum over edges e into molecule m of g_e[a] * delta_e[b], g_e = gd_e + delta_e / r_e *
    (gr_e + gr2_e), 0 where r_e == 0 -- written out with Python floats -- for gd, gr, gr2 each given or None."""
    src, dst, batch, dl, r, g = _hand_list()
    E = src.numel()
    gd = torch.randn(E, 3, generator=g, dtype=torch.float64) if has[0] else None
    gr = torch.randn(E, generator=g, dtype=torch.float64) if has[1] else None
    gr2 = torch.randn(E, generator=g, dtype=torch.float64) if has[2] else None
    ref = [[[0.0] * 3 for _ in range(3)] for _ in range(2)]
    for e in range(E):
        re = float(r[e])
        if re == 0.0:
            continue
        gs = (float(gr[e]) if has[1] else 0.0) + (float(gr2[e]) if has[2] else 0.0)
        ge = [(float(gd[e, a]) if has[0] else 0.0) + float(dl[e, a]) / re * gs for a in range(3)]
        m = int(batch[int(dst[e])])
        for a in range(3):
            for b in range(3):
                ref[m][a][b] += ge[a] * float(dl[e, b])
    out = nl_backward_virial_composite(gd, gr, gr2, dl, r, dst, batch, 2)
    assert out.shape == (2, 3, 3) and out.dtype == torch.float64
    assert torch.allclose(out, torch.tensor(ref, dtype=torch.float64), rtol=1e-13, atol=1e-13)


def test_composite_ignores_padding_slots():
    """Static-capacity padding: r == 0, destination -1, anything in the other buffers -- no contribution."""
    src, dst, batch, dl, r, g = _hand_list()
    gr = torch.randn(src.numel(), generator=g, dtype=torch.float64)
    ref = nl_backward_virial_composite(None, gr, None, dl, r, dst, batch, 2)
    nan = float("nan")
    out = nl_backward_virial_composite(None, torch.cat([gr, torch.full((3,), nan, dtype=gr.dtype)]), None,
                                       torch.cat([dl, torch.full((3, 3), nan, dtype=dl.dtype)]),
                                       torch.cat([r, torch.zeros(3, dtype=r.dtype)]),
                                       torch.cat([dst, torch.full((3,), -1, dtype=dst.dtype)]), batch, 2)
    assert torch.equal(out, ref)


# ----------------------------------------------------------------------------- refusals
def _inputs():
    z = torch.tensor([8, 1, 1], dtype=torch.long)
    return z, torch.randn(3, 3), torch.zeros(3, dtype=torch.long)


def test_refuses_a_model_without_forces():
    from torchmdnet.models.model import create_model
    m = create_model(yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=1, derivative=False))
    with pytest.raises(ValueError, match="derivative=True"):
        m.energy_forces_virial(*_inputs())


def test_refuses_a_wrapped_representation_model():
    from torchmdnet.models.model import create_model
    m = create_model(yaml_args("graph-network", embedding_dimension=32, num_layers=1, derivative=False,
                               atom_filter=1, aggr="add", neighbor_embedding=True, output_model="Scalar",
                               reduce_op="add"))
    m.derivative = True  # create_model itself refuses derivative + atom filter; reach the wrapper check
    with pytest.raises(ValueError, match="AtomFilter"):
        m.energy_forces_virial(*_inputs())


@pytest.mark.parametrize("model", ["equivariant-transformer", "tensornet"])
def test_torchscript_leaves_the_virial_out(model):
    """The models that script today still script; the scripted module calls forward as before and refuses
    energy_forces_virial (a @torch.jit.unused method), it does not fail to compile over it."""
    from torchmdnet import _native
    from torchmdnet.models.model import create_model
    _native.load_torch_ops()
    m = create_model(yaml_args(model, embedding_dimension=32, num_layers=1, derivative=True))
    assert hasattr(m, "energy_forces_virial")
    s = torch.jit.script(m)
    assert s._c._has_method("forward")
    assert not s._c._has_method("energy_forces_virial")
