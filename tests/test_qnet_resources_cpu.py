"""Scratch of the DDQN acting kernels, read from the in-tree liblnw.so like
test_kernel_resources_cpu.py: qnet_act_kernel (both instantiations) spills one
32-bit value around the conv head, 8 B per lane at 256 VGPRs and two waves per
SIMD, below the 20 B the policy kernel is allowed; untrained red's kernel has
none."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

LIMITS = {
    "qnet_act_kernelILi32E": 8,
    "qnet_act_kernelILi64E": 8,
    "qnet_red_random_kernel": 0,
}


@needs_lib
@needs_tools
def test_qnet_kernels_scratch():
    sc = kernel_scratch(LIB)
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
