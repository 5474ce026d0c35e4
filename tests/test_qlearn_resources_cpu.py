"""Scratch of the DDQN learner kernels (csrc/lnw_qlearn.hip), read from the
in-tree liblnw.so like test_qnet_resources_cpu.py: none of them spills. The
per-row passes hold a 49-value conv1 map or four 9-value conv2 maps in registers
at 128 threads per workgroup (119-222 VGPRs, DESIGN.md "DDQN learner"); a spill
there would sit inside the rolled channel loops."""
import os

import pytest

from test_kernel_resources_cpu import LIB, _tool, kernel_scratch

LIMITS = {
    "ql_moments1_kernel": 0,
    "ql_moments2_kernel": 0,
    "ql_forward_kernelILi32E": 0,
    "ql_forward_kernelILi64E": 0,
    "ql_headgrad_kernel": 0,
    "ql_conv2grad_kernel": 0,
    "ql_conv1grad_kernel": 0,
    "ql_reduce_kernel": 0,
    "ql_reduce_d_kernel": 0,
    "ql_stats_kernel": 0,
    "ql_adam_kernel": 0,
    "ql_advance_kernel": 0,
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="liblnw.so not built")
@pytest.mark.skipif(not (_tool("llvm-objcopy") and _tool("clang-offload-bundler") and _tool("llvm-readelf")),
                    reason="ROCm LLVM tools not found")
def test_qlearn_kernels_scratch(tmp_path):
    sc = kernel_scratch(LIB, str(tmp_path))
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
