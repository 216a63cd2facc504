"""Child process of tests/test_gpu_gemm_edges.py::test_env_only_forms.  csrc/gemm.hip reads TMDNET_GEMM_NW and
TMDNET_GEMM_KB4 once per process, so the k_gemm forms behind them (<8,2>, <8,8>, <2,8>, <4,2>) need a process of
their own: the parent starts this file with the switches set.  Runs the K ladder of tests/gemm_ref.py (M = 37,
N = 70, NT and NN, bias) in exact mode -- bit-equal to the fp64 reference, no NaN, padding untouched -- prints the
forms the restated dispatch expects and a digest of the results; exits non-zero on a miss."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))


def main():
    import gemm_ref as R
    from torchmdnet import kernels
    nw = os.environ.get("TMDNET_GEMM_NW")
    kb4 = int(os.environ.get("TMDNET_GEMM_KB4", "1"))
    assert nw is not None or kb4 != 1, "started without a switch"
    small, large = (int(v) for v in nw.split(",")) if nw else (4, 16)
    forms = sorted({R.grouped_form(K, small, large, kb4)[:2] for K in R.K_LADDER})
    print(f"TMDNET_GEMM_NW={nw} TMDNET_GEMM_KB4={kb4}: forms {forms}")
    outs, bad = [], []
    for s in R.ladder_specs():
        o = R.build(s, "exact", "cuda")
        assert kernels.gemm_launch([kernels.Gemm(*R.gemm_args(s, o))]) is True
        torch.cuda.synchronize()
        ref, _ = R.reference(s, o)
        if not (torch.equal(o["C"], ref.to(torch.float32)) and R.padding_untouched(o["Cbuf"], s.M, s.N)):
            bad.append(R.spec_name(s))
        outs.append(o["C"])
    print(f"digest {R.digest(outs)}")
    if bad:
        print("MISSED", bad)
        sys.exit(1)


if __name__ == "__main__":
    main()
