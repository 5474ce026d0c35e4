"""Scratch of the MAPPO learner kernels (csrc/lnw_ppolearn.hip), read from the
in-tree liblnw.so exactly as test_qlearn_resources_cpu.py does: none of them
spills. The per-row conv passes hold a 49-value conv1 map or four 9-value conv2
maps in registers at 128 threads per workgroup (DESIGN.md "MAPPO learner"); a
spill there would sit inside the rolled channel loops."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

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


@needs_lib
@needs_tools
def test_ppolearn_kernels_scratch():
    sc = kernel_scratch(LIB)
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
