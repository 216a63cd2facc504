# C5 energy + forces under each edge-kernel route of et_stack (TMDNET_FEP: projection fused into the edge
# kernels or pair rows; TMDNET_FEP_BWD: the backward recomputed unfused, or fused).  Separate processes: the
# switches are read at import.
set -o pipefail
mkdir -p gpurun_out
for v in "0 off" "auto off" "auto lazy" "auto fused"; do
  set -- $v
  TMDNET_FEP=$1 TMDNET_FEP_BWD=$2 timeout -k 10 300 python -u tools/c5_time.py 50001 5 2>&1 | grep -v amdgpu.ids || exit 1
done
