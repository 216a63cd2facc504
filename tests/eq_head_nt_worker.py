"""Child process of tests/test_gpu_eq_head_widths.py::test_four_atoms_per_workgroup.  csrc/eq_head.hip reads
TMDNET_HEAD_NT once per process, so the env-only form of four atoms per workgroup needs a process of its own:
the parent starts this file with TMDNET_HEAD_NT=4.  N = 37 atoms (nine full tiles and one live atom in the
last), a zero-vector atom, forward + Jacobian and the weight-gradient factors against the float64 composite with
the measure of tests/eq_head_ref.py.  Forms by LDS size (29.5 H + 8 values per atom, 1536 more for the split
transposed products, 64 KB): fp32 H = 20 and 64 split (scalar / 16-byte loads), 100 and 136 unsplit (scalar /
16-byte), fp64 H = 8 and 12 split, 20 and 64 unsplit; fp32 H = 256 does not fit four atoms and must step down
to two.  Prints every figure and the worst fp32 ratio; exits non-zero on a miss."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

F32, F64 = torch.float32, torch.float64
CASES = [(20, F32), (64, F32), (100, F32), (136, F32), (8, F64), (12, F64), (20, F64), (64, F64), (256, F32)]
N = 37


def main():
    import eq_head_ref as R
    from test_eq_head import _head
    from torchmdnet import kernels
    assert os.environ.get("TMDNET_HEAD_NT") == "4"
    kernels.HEAD_X3 = False
    worst = [0.0]
    for H, dtype in CASES:
        head = _head(H, dtype)
        ps = kernels.eq_head_params(head.output_network)
        x, vec, gy, _, _ = R.inputs(N, H, dtype, zero=2)
        y_ref, first, _ = R.reference(ps, x, vec, gy)
        head = head.to("cuda")
        ps = kernels.eq_head_params(head.output_network)
        xs, vs = x.to("cuda").requires_grad_(True), vec.to("cuda").requires_grad_(True)
        y = kernels.eq_scalar_head(xs, vs, head.output_network)
        what = f"NT=4 H={H} {str(dtype)[6:]}"
        R.close(y, y_ref, dtype, f"{what} y", worst)
        jac = torch.autograd.grad(y, (xs, vs), gy.to("cuda"), retain_graph=True)  # the Jacobian path
        for name, a, b in zip(R.FIRST, jac, first):
            R.close(a, b, dtype, f"{what} jacobian {name}", worst)
        got = torch.autograd.grad(y, [xs, vs] + ps, gy.to("cuda"))  # the weight-gradient factors
        for name, a, b in zip(R.FIRST, got, first):
            R.close(a, b, dtype, f"{what} {name}", worst)
        for g in (jac[1], got[1]):
            assert not bool(g[2].any()), f"{what}: the zero-vector atom's g_vec"
    print(f"worst fp32 ratio {worst[0]:.2e} (bar 1e-4)")


if __name__ == "__main__":
    main()
