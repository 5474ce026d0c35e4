"""Scratch (private segment) of the policy kernels with the `script_self` mode
in them, read on the CPU from the in-tree liblnw.so's gfx950 metadata like
tests/test_kernel_resources_cpu.py does. The mode is a run-time branch beside
`forced`, after the conv head (where the register file is full): the four
policy_act_kernel instantiations stay as they were, one kernel per name, within
20 B per lane, and so does any other kernel whose name speaks of the policy
(the mode added none)."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

LIMIT = 20  # bytes per lane
POLICY_KERNELS = ("policy_act_kernelILi32ELb0E", "policy_act_kernelILi64ELb0E",
                  "policy_act_kernelILi32ELb1E", "policy_act_kernelILi64ELb1E")


@needs_lib
@needs_tools
def test_policy_kernels_scratch_with_script_self():
    sc = kernel_scratch(LIB)
    for frag in POLICY_KERNELS:
        hits = {k: v for k, v in sc.items() if frag in k}
        assert len(hits) == 1, f"kernel {frag}: {sorted(hits)}"
        for k, v in hits.items():
            assert v <= LIMIT, f"{k}: {v} B/lane of scratch (limit {LIMIT})"
    # whatever else acts for a policy (a newly named kernel sharing the body)
    for k, v in sc.items():
        if "policy" in k and not any(f in k for f in POLICY_KERNELS):
            assert v <= LIMIT, f"{k}: {v} B/lane of scratch (limit {LIMIT})"
