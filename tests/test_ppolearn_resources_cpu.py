"""Scratch of the MAPPO learner kernels (csrc/lnw_ppolearn.hip), read from the
in-tree liblnw.so exactly as test_qlearn_resources_cpu.py does: none of them
spills. The per-row conv passes hold a 49-value conv1 map or four 9-value conv2
maps in registers at 128 threads per workgroup (DESIGN.md "MAPPO learner"); a
spill there would sit inside the rolled channel loops."""
import os

import pytest

from test_kernel_resources_cpu import LIB, _tool, kernel_scratch

LIMITS = {
    "pl_features_kernel": 0,
    "pl_linear_fwd_kernel": 0,
    "pl_linear_bwd_kernel": 0,
    "pl_linear_wgrad_kernel": 0,
    "pl_reduce_lin_kernel": 0,
    "pl_advantage_kernel": 0,
    "pl_actorloss_kernel": 0,
    "pl_actorloss_sum_kernel": 0,
    "pl_lnbwd_kernel": 0,
    "pl_lnwgrad_kernel": 0,
    "pl_conv2grad_kernel": 0,
    "pl_conv1grad_kernel": 0,
    "pl_reduce_conv_kernel": 0,
    "pl_running_kernel": 0,
    "pl_norm_kernel": 0,
    "pl_adam_kernel": 0,
    "pl_advance_kernel": 0,
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="liblnw.so not built")
@pytest.mark.skipif(not (_tool("llvm-objcopy") and _tool("clang-offload-bundler") and _tool("llvm-readelf")),
                    reason="ROCm LLVM tools not found")
def test_ppolearn_kernels_scratch(tmp_path):
    sc = kernel_scratch(LIB, str(tmp_path))
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
