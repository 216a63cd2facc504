"""Pair priors (ZBL, D2, Coulomb) without a GPU: the dense restatement of tests/pair_prior_ref.py against the
reference's recorded outputs (tests/golden/priors_ref.npz, written by tests/golden/gen_prior_fixtures.py), and
the classes' construction contract -- signatures, init-arg round trip, checkpoint keys, dataset fallbacks,
the list form of ``prior_model``, and the errors raised where no GPU kernel can run."""
import inspect
import io
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, golden, yaml_args
import pair_prior_ref as R
from torchmdnet.priors import D2, ZBL, Atomref, Coulomb

SCALES = dict(distance_scale=1e-10, energy_scale=4.35974e-18)
NUMBERS = list(range(100))


def _inputs():
    d = golden("priors_ref.npz")
    return (d, torch.tensor(d["z"]), torch.tensor(d["pos"]), torch.tensor(d["batch"]),
            torch.tensor(d["partial_charges"]))


def _restatement(kind, z, batch, q, n_mol):
    if kind == "zbl":
        return lambda p: R.zbl_energy(p, z, batch, n_mol, 5.0, NUMBERS, **SCALES)
    if kind == "d2":
        prior = D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
        return lambda p: R.d2_energy(p, z, batch, n_mol, 10.0, NUMBERS, c6=prior.C_6, r_r=prior.R_r, **SCALES)
    return lambda p: R.coulomb_energy(p, q, batch, n_mol, 0.3, **SCALES)


# D2 and Coulomb restate the reference operation for operation (measured 2e-16 and 5e-15 on the energies).
# ZBL: the reference forms Z^0.23 in float32 (<= 6e-8 relative on a), the restatement in float64; measured
# 2.1e-8 (y), 1.7e-8 (F), 2.5e-8 (second order) relative to the largest entry.
@pytest.mark.parametrize("kind,rtol", [("zbl", 1e-6), ("d2", 1e-12), ("coulomb", 1e-12)])
def test_restatement_matches_reference_fixture(kind, rtol):
    d, z, pos, batch, q = _inputs()
    assert pos.dtype == torch.float64 and pos.shape[0] == 57
    n_mol = int(batch.max()) + 1
    y, f, h = R.energy_forces_second(_restatement(kind, z, batch, q, n_mol), pos)
    for name, got, ref in (("y", y.reshape(-1), d[kind + "/y"].reshape(-1)), ("forces", f, d[kind + "/forces"]),
                           ("dF2", h, d[kind + "/dF2"])):
        ref = torch.tensor(ref)
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"{kind} {name}: max|d|/max|ref| = {err:.3e}")
        assert err <= rtol, (kind, name, err)


def test_constructor_signatures_match_the_reference():
    def names(cls):
        return list(inspect.signature(cls.__init__).parameters)[1:]
    assert names(ZBL) == ["cutoff_distance", "max_num_neighbors", "atomic_number", "distance_scale", "energy_scale",
                          "dataset"]
    assert names(D2) == ["cutoff_distance", "max_num_neighbors", "atomic_number", "distance_scale", "energy_scale",
                         "dataset", "dtype"]
    assert names(Coulomb) == ["alpha", "max_num_neighbors", "distance_scale", "energy_scale", "dataset"]
    assert inspect.signature(D2.__init__).parameters["dtype"].default == torch.float32


def test_init_args_round_trip_and_state_dict_keys():
    zbl = ZBL(5.0, 40, atomic_number=NUMBERS, **SCALES)
    d2 = D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
    cou = Coulomb(0.3, 40, **SCALES)
    assert zbl.get_init_args() == dict(cutoff_distance=5.0, max_num_neighbors=40, atomic_number=NUMBERS, **SCALES)
    assert d2.get_init_args() == dict(cutoff_distance=10.0, max_num_neighbors=128, atomic_number=NUMBERS, **SCALES)
    assert cou.get_init_args() == dict(alpha=0.3, max_num_neighbors=40, **SCALES)
    for p in (zbl, d2, cou):
        again = type(p)(**p.get_init_args())
        assert again.get_init_args() == p.get_init_args()
        assert p.static_capacity is None
        # no neighbour-list submodule: the capture wrapper would hand it the representation's capacity
        assert list(p.children()) == []
    assert list(zbl.state_dict()) == ["atomic_number"] and zbl.atomic_number.dtype == torch.long
    assert list(d2.state_dict()) == ["Z_map", "C_6", "R_r"]
    assert list(cou.state_dict()) == []
    assert (zbl.cutoff_distance, zbl.max_num_neighbors, cou.alpha, cou.max_num_neighbors) == (5.0, 40, 0.3, 40)
    assert (d2.cutoff_distance, d2.max_num_neighbors, d2.d, d2.s_6) == (10.0, 128, 20, 1)


def test_d2_table_is_grimme_2006_table_1():
    d2 = D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
    assert d2.C_6.shape == d2.R_r.shape == (55,) and d2.C_6.dtype == torch.float64
    assert torch.isnan(d2.C_6[0]) and torch.isnan(d2.R_r[0])
    for Z, c6, r0 in ((1, 0.14, 1.001), (6, 1.75, 1.452), (8, 0.70, 1.342), (17, 5.07, 1.639), (26, 10.80, 1.562),
                      (35, 12.47, 1.749), (46, 24.67, 1.639), (54, 29.99, 1.881)):
        assert float(d2.C_6[Z]) == c6 and float(d2.R_r[Z]) == pytest.approx(0.1 * r0, rel=1e-15)
    assert D2(10.0, 128, atomic_number=NUMBERS, **SCALES).C_6.dtype == torch.float32


def test_dataset_fallbacks():
    class Stub:
        atomic_number = [0, 1, 6, 8]
        distance_scale = 1e-9
        energy_scale = 1.6e-19

    zbl, d2, cou = ZBL(3.0, 8, dataset=Stub()), D2(3.0, 8, dataset=Stub()), Coulomb(0.5, 8, dataset=Stub())
    assert zbl.atomic_number.tolist() == [0, 1, 6, 8] and d2.atomic_number == [0, 1, 6, 8]
    assert d2.Z_map.tolist() == [0, 1, 6, 8]
    for p in (zbl, d2, cou):
        assert p.distance_scale == pytest.approx(1e-9) and p.energy_scale == pytest.approx(1.6e-19)
    # explicit arguments win over the dataset
    assert ZBL(3.0, 8, atomic_number=[1], distance_scale=2.0, energy_scale=3.0, dataset=Stub()).distance_scale == 2.0


def _prior_list():
    from torchmdnet.models.model import create_prior_models
    with open(os.path.join(GOLDEN, "configs", "priors.yaml")) as f:
        return create_prior_models(yaml.safe_load(f))


def test_create_prior_models_list_config():
    ps = _prior_list()
    assert [type(p) for p in ps] == [ZBL, D2, Atomref]
    assert ps[0].cutoff_distance == 4.0 and ps[0].max_num_neighbors == 50
    assert ps[1].cutoff_distance == 9.0 and ps[1].max_num_neighbors == 100
    assert ps[2].initial_atomref.shape == (10, 1)


def _tiny_model(prior_model, precision=64):
    from torchmdnet.models.model import create_model
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                     max_num_neighbors=32, derivative=True, output_model="Scalar", precision=precision)
    args["prior_model"] = prior_model
    return create_model(args)


def test_model_with_priors_saves_and_loads():
    with open(os.path.join(GOLDEN, "configs", "priors.yaml")) as f:
        m = _tiny_model(yaml.safe_load(f)["prior_model"])
    assert [type(p) for p in m.prior_model] == [ZBL, D2, Atomref]
    keys = set(m.state_dict())
    assert {"prior_model.0.atomic_number", "prior_model.1.Z_map", "prior_model.1.C_6", "prior_model.1.R_r",
            "prior_model.2.atomref.weight"} <= keys
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert [type(p) for p in m2.prior_model] == [ZBL, D2, Atomref]
    assert m2.prior_model[0].get_init_args() == m.prior_model[0].get_init_args()
    assert m2.prior_model[1].get_init_args() == m.prior_model[1].get_init_args()
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v, ) or (torch.isnan(v) == torch.isnan(m2.state_dict()[k])).all()
    # the state dict alone loads into a freshly built model, too
    with open(os.path.join(GOLDEN, "configs", "priors.yaml")) as f:
        m3 = _tiny_model(yaml.safe_load(f)["prior_model"])
    m3.load_state_dict(m.state_dict())


def test_coulomb_needs_detached_partial_charges():
    cou = Coulomb(0.3, 40, **SCALES)
    _, z, pos, batch, q = _inputs()
    y = torch.zeros(3, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="partial_charges"):
        cou.post_reduce(y, z, pos, batch, None)
    with pytest.raises(RuntimeError, match="partial_charges"):
        cou.post_reduce(y, z, pos, batch, {"other": q})
    with pytest.raises(RuntimeError, match="require grad"):
        cou.post_reduce(y, z, pos, batch, {"partial_charges": q.clone().requires_grad_(True)})


@pytest.mark.parametrize("kind", ["zbl", "d2", "coulomb"])
def test_no_cpu_fallback(kind):
    _, z, pos, batch, q = _inputs()
    prior = {"zbl": lambda: ZBL(5.0, 40, atomic_number=NUMBERS, **SCALES),
             "d2": lambda: D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES),
             "coulomb": lambda: Coulomb(0.3, 40, **SCALES)}[kind]()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        prior.post_reduce(torch.zeros(3, 1, dtype=torch.float64), z, pos, batch, {"partial_charges": q})
