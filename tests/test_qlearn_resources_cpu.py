"""Scratch of the DDQN learner kernels (csrc/lnw_qlearn.hip), read from the
in-tree liblnw.so like test_qnet_resources_cpu.py: none of them spills. The
per-row passes hold a 49-value conv1 map or four 9-value conv2 maps in registers
at 128 threads per workgroup (119-222 VGPRs, DESIGN.md "DDQN learner"); a spill
there would sit inside the rolled channel loops."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

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


@needs_lib
@needs_tools
def test_qlearn_kernels_scratch():
    sc = kernel_scratch(LIB)
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
