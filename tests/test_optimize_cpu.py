"""CPU tests of ``torchmdnet.optimize`` and ``torchmdnet.calculators`` (no GPU): what ``optimize`` accepts and
refuses, what it changes on the model (state_dict keys, repr, frozen parameters), and ``External``'s handling of
``output_transform``."""
import pytest
import torch

from conftest import yaml_args


def _args(**kw):
    base = dict(embedding_dimension=32, num_layers=2, num_rbf=16, aggr="add", derivative=True, output_model="Scalar",
                precision=32, max_z=10)
    base.update(kw)
    return yaml_args("graph-network", **base)


def _model(**kw):
    from torchmdnet.models.model import create_model
    return create_model(_args(**kw))


def test_optimize_refuses_other_models():
    from torchmdnet.models.model import create_model
    from torchmdnet.optimize import optimize
    with pytest.raises(ValueError, match="Only TorchMD_GN"):
        optimize(create_model(yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=1, num_rbf=8,
                                        num_heads=4)))
    with pytest.raises(AssertionError):
        optimize(torch.nn.Linear(2, 2))


@pytest.mark.parametrize("kw,match", [
    (dict(aggr="max"), "aggr"),
    (dict(precision=64), "float32"),
    (dict(precision=16), "float32"),
    (dict(embedding_dimension=24), "num_filters"),
    (dict(embedding_dimension=144), "num_filters"),
    (dict(num_rbf=65), "num_rbf"),
    (dict(activation="tanh"), "activation"),
    (dict(activation="sigmoid"), "activation"),
], ids=["max", "f64", "f16", "F24", "F144", "R65", "tanh", "sigmoid"])
def test_optimize_refusal_matrix(kw, match):
    from torchmdnet.models.torchmd_gn import TorchMD_GN
    from torchmdnet.optimize import optimize
    model = _model(**kw)
    with pytest.raises(ValueError, match=match):
        optimize(model)
    assert isinstance(model.representation_model, TorchMD_GN), "a refused model must stay as it was"


@pytest.mark.parametrize("kw", [
    dict(), dict(aggr="mean", activation="ssp", rbf_type="gauss", trainable_rbf=False, neighbor_embedding=False),
    dict(embedding_dimension=128, num_rbf=50, cutoff_lower=1.0), dict(embedding_dimension=16, num_rbf=1),
    dict(num_rbf=64, trainable_rbf=True),
])
def test_optimize_accepts_and_wraps(kw):
    from torchmdnet.models.torchmd_gn import TorchMD_GN
    from torchmdnet.optimize import TorchMD_GN_optimized, optimize
    model = _model(**kw)
    rep = model.representation_model
    text = repr(rep)
    keys = list(model.state_dict())
    out = optimize(model)
    assert out is model
    opt = model.representation_model
    assert isinstance(opt, TorchMD_GN_optimized) and opt.model is rep and isinstance(opt.model, TorchMD_GN)
    assert repr(opt) == "Optimized: " + text
    assert opt.distance is rep.distance
    new = list(model.state_dict())
    assert new == [k.replace("representation_model.", "representation_model.model.", 1) for k in keys]
    assert any(k.startswith("representation_model.model.interactions.0.mlp.0.") for k in new)


def test_optimize_freezes_the_bypassed_parameters():
    from torchmdnet.optimize import optimize
    model = optimize(_model(trainable_rbf=True))
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen, "nothing frozen"
    for n, p in model.named_parameters():
        bypassed = ".mlp." in n or ".distance_expansion." in n
        assert p.requires_grad != bypassed, n
    assert sum(".mlp." in n for n in frozen) == 4 * 2 and sum(".distance_expansion." in n for n in frozen) == 2


def test_optimized_wrapper_refuses_other_modules_and_torchscript():
    from torchmdnet.optimize import TorchMD_GN_optimized, optimize
    with pytest.raises(ValueError, match="Only TorchMD_GN"):
        TorchMD_GN_optimized(torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match="runs eagerly"):
        torch.jit.script(optimize(_model()))


def test_optimized_model_has_no_cpu_path():
    from torchmdnet.optimize import optimize
    model = optimize(_model())
    z = torch.tensor([1, 6, 8])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(z, torch.randn(3, 3), torch.zeros(3, dtype=torch.long))


def _checkpoint(path):
    from torchmdnet.models.model import create_model
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                     max_z=10, derivative=False)
    torch.manual_seed(3)
    model = create_model(args)
    torch.save({"state_dict": {"model." + k: v for k, v in model.state_dict().items()}, "hyper_parameters": args},
               path)
    return str(path)


def test_external_output_transform(tmp_path):
    from torchmdnet import calculators
    from torchmdnet.calculators import External
    ckpt = _checkpoint(tmp_path / "et.ckpt")
    z = torch.tensor([[1, 6, 8, 1]])
    with pytest.raises(ValueError, match="output_transform"):
        External(ckpt, z, output_transform="lambda energy, forces: (energy, forces)")
    with pytest.raises(ValueError, match="output_transform"):
        External(ckpt, z, output_transform="eV -> kcal")
    assert set(calculators.tranforms) == {"eV/A -> kcal/mol/A", "Hartree/Bohr -> kcal/mol/A",
                                          "Hartree/A -> kcal/mol/A"}
    calc = External(ckpt, z, output_transform="Hartree/Bohr -> kcal/mol/A")
    e, f = calc.output_transformer(torch.ones(1, 1), torch.ones(1, 4, 3))
    assert torch.allclose(e, torch.full((1, 1), 627.509)) and torch.allclose(f, torch.full((1, 4, 3), 627.509 / 0.529177))
    calc = External(ckpt, torch.tensor([[1, 6], [8, 1]]), output_transform=lambda e, f: (2 * e, -f))
    assert calc.n_atoms == 2 and calc.batch.tolist() == [0, 0, 1, 1] and calc.embeddings.tolist() == [1, 6, 8, 1]
    assert not calc.model.training and calc.model.derivative
    e, f = calc.output_transformer(torch.ones(2, 1), torch.ones(2, 2, 3))
    assert float(e[0]) == 2 and float(f[0, 0, 0]) == -1
